"""Convolve / Reverb without a GPU: the overlap-save identity in float64 against np.convolve and scipy, the float32 model's own
error, the table builder, the block rule, the plan, the argument checks of the C entry points through ctypes, the layer surface,
and the records (header, README)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.signal

import kapre_amd as kapre
from kapre_amd import _ffi, backend
from conftest import REPO

import convolve_model as cm

RNG = np.random.default_rng(20262)
NULL = ctypes.c_void_p(0)
SOME = ctypes.c_void_p(0x10000)             # never dereferenced: every call below fails its argument checks first


# ------------------------------------------------------------------ the models
@pytest.mark.parametrize("t,n,L", cm.IDENTITY_SHAPES)
def test_overlap_save_identity_float64(t, n, L):
    x, h = RNG.standard_normal((2, t)), RNG.standard_normal(n)
    y = cm.overlap_save64(x, h, L)
    want = np.stack([np.convolve(r, h) for r in x])
    assert y.shape == want.shape
    scale = np.max(np.abs(want))
    assert np.max(np.abs(y - want)) <= 1e-12 * scale
    assert np.max(np.abs(y - scipy.signal.fftconvolve(x, h[None, :], axes=-1))) <= 1e-12 * scale


@pytest.mark.parametrize("t,n,L", cm.IDENTITY_SHAPES)
def test_float32_model_is_a_float32_convolution(t, n, L):
    """the yardstick of the GPU tests stays at float32 round-off of the scale ||h||_1 max|x| (2e-7 in the issue's runs)"""
    x, h = RNG.standard_normal((2, t)).astype(np.float32), RNG.standard_normal(n)
    y = cm.overlap_save32(x, h, L)
    assert y.dtype == np.float32
    want = np.stack([np.convolve(r.astype(np.float64), h) for r in x])
    worst = max(cm.figure(y[i], want[i], h, x[i]) for i in range(2))
    print("float32 model, T %d, len %d, L %d: %.3g" % (t, n, L, worst))
    assert worst <= 1e-6


def test_frame_counts_are_enough_and_needed():
    for t, n, L in cm.IDENTITY_SHAPES:
        k_in, k_out, P = cm.frame_counts(t, n, L)
        assert (k_in - 1) * L >= t > (k_in - 2) * L or t <= 0          # the last analysis frame still starts inside x
        assert k_out * L >= t + n - 1 > (k_out - 1) * L
        assert (P - 1) * L < n <= P * L


def test_spec_fir_model_matches_the_plain_sum():
    X = RNG.standard_normal((2, 2, 5, 6)) + 1j * RNG.standard_normal((2, 2, 5, 6))
    H = RNG.standard_normal((3, 3, 3)) + 1j * RNG.standard_normal((3, 3, 3))
    Y, bre, bim = cm.spec_fir64(X, H, [2, 7], 7, band_div=2)
    for item, ir in ((0, 2), (1, 2)):                                  # 7 is clamped to 2
        for k in range(7):
            for i in range(6):
                want = sum(X[item, 1, k - p, i] * H[ir, p, i // 2] for p in range(3) if 0 <= k - p < 5)
                assert abs(Y[item, 1, k, i] - want) < 1e-12
    assert np.all(bre >= np.abs(Y.real) - 1e-12) and np.all(bim >= np.abs(Y.imag) - 1e-12)


def test_index_draw_model():
    a = cm.index_draw(1234, 0, 4096, 7)
    assert a.dtype == np.int32 and a.min() >= 0 and a.max() <= 6
    assert np.array_equal(a, cm.index_draw(1234, 0, 4096, 7))
    assert not np.array_equal(a, cm.index_draw(1234, 1, 4096, 7))
    assert np.array_equal(a[:7], cm.index_draw(1234, 0, 7, 7))           # an entry does not depend on the item count
    assert np.all(cm.index_draw(99, 5, 100, 1) == 0)
    sigma = np.sqrt(4096 * (1 / 7) * (6 / 7))
    assert np.all(np.abs(np.bincount(a, minlength=7) - 4096 / 7) <= 6 * sigma)


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("n,L", [(1, 256), (300, 256), (700, 256), (4097, 1024), (1024, 512)])
def test_table_is_the_rfft_of_the_partitions(n, L):
    h = RNG.standard_normal((2, n))
    tab = backend.convolve_table(h, L)
    P = -(-n // L)
    assert tab.shape == (2, P, L + 1) and tab.dtype == np.complex64
    for i in range(2):
        for p in range(P):
            want = np.fft.rfft(h[i, p * L:(p + 1) * L], n=2 * L)
            assert np.array_equal(tab[i, p], want.astype(np.complex64))
    adj = backend.convolve_table(h, L, adjoint=True)
    assert np.array_equal(adj, backend.convolve_table(h[:, ::-1], L))
    assert np.array_equal(backend.convolve_table(h[0], L), tab[:1])


def test_table_size_limit_names_the_size():
    with pytest.raises(ValueError, match=r"MiB"):
        backend.convolve_table(np.zeros((1100, 32 * 1024)), 1024)
    with pytest.raises(ValueError):
        backend.convolve_table(np.array([1.0, np.nan]), 256)
    with pytest.raises(ValueError):
        backend.convolve_table(np.zeros((2, 2, 2)), 256)


# ------------------------------------------------------------------ block rule and plan
def test_block_rule():
    assert backend.convolve_block(1) == 256
    assert backend.convolve_block(16 * 256) == 256
    assert backend.convolve_block(16 * 256 + 1) == 512
    assert backend.convolve_block(16 * 512) == 512
    assert backend.convolve_block(16 * 512 + 1) == 1024
    assert backend.convolve_block(16 * 1024 + 1) == 1024
    assert backend.convolve_block(32 * 1024) == 1024
    with pytest.raises(ValueError, match="32768"):
        backend.convolve_block(32 * 1024 + 1)
    with pytest.raises(ValueError):
        backend.convolve_block(0)
    assert backend.convolve_block(300, block_size=1024) == 1024
    assert backend.convolve_block(32 * 256, block_size=256) == 256
    with pytest.raises(ValueError, match="partitions"):
        backend.convolve_block(32 * 256 + 1, block_size=256)
    for bad in (128, 2048, 300, 256.0, True):
        with pytest.raises(ValueError):
            backend.convolve_block(300, block_size=bad)


def test_plan_values_and_errors():
    for P, bucket in ((1, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32)):
        rows, waves, b = _ffi.spec_fir_plan(100, 129, P)
        assert (rows, waves, b) == (8, 4, bucket)
    assert _ffi.spec_fir_plan(0, 0, 1) == (8, 4, 4)
    out = (ctypes.c_int * 3)()
    L = _ffi.lib()
    assert L.kpr_spec_fir_plan(10, 10, 0, out) == -1
    assert L.kpr_spec_fir_plan(10, 10, 33, out) == -1
    assert L.kpr_spec_fir_plan(-1, 10, 4, out) == -1
    assert L.kpr_spec_fir_plan(10, -1, 4, out) == -1
    assert L.kpr_spec_fir_plan(10, 10, 4, None) == -1
    assert b"n_part" in L.kpr_last_error() or b"NULL" in L.kpr_last_error()


# ------------------------------------------------------------------ the C entry points, argument errors only
def _fir(x=SOME, outer=2, frames_in=4, inner=6, band_div=1, h=ctypes.c_void_p(0x20000), n_ir=1, n_part=2, idx=NULL, items=2,
         out=ctypes.c_void_p(0x30000), frames_out=5):
    return _ffi.lib().kpr_spec_fir_c64(x, outer, frames_in, inner, band_div, h, n_ir, n_part, idx, items, out, frames_out, NULL)


def test_spec_fir_argument_errors():
    assert _fir(x=NULL) == -1
    assert _fir(h=NULL) == -1
    assert _fir(out=NULL) == -1
    for kw in (dict(outer=-1), dict(frames_in=-1), dict(inner=-1), dict(frames_out=-1), dict(band_div=0), dict(n_ir=0),
               dict(n_part=0), dict(n_part=33), dict(items=0), dict(items=-1), dict(outer=3, items=2), dict(inner=7, band_div=2)):
        assert _fir(**kw) == -1, kw
    assert _fir(out=SOME) == -1                                            # in place
    assert b"overlap" in _ffi.lib().kpr_last_error()
    assert _fir(out=ctypes.c_void_p(0x10000 + 8 * 6 * 4)) == -1            # out starts inside x
    assert _fir(out=ctypes.c_void_p(0x20000)) == -1                        # out on the table
    assert _fir(idx=ctypes.c_void_p(0x30000)) == -1                        # out on the index
    assert _fir(x=ctypes.c_void_p(0x10004)) == -1                          # alignment
    assert _fir(idx=ctypes.c_void_p(0x40002)) == -1
    assert _fir(frames_in=1 << 24, inner=64) == -2                         # 2^30 elements per outer item
    assert _fir(frames_out=1 << 24, inner=64) == -2
    # zero-sized problems: 0, nothing launched (no device is touched: the pointers are never read)
    assert _fir(outer=0, items=0) == 0
    assert _fir(frames_out=0) == 0
    assert _fir(inner=0) == 0


def test_index_draw_argument_errors():
    L = _ffi.lib()
    assert L.kpr_index_draw(SOME, 4, 0, ctypes.c_void_p(0x20000), NULL) == -1
    assert L.kpr_index_draw(SOME, -1, 3, ctypes.c_void_p(0x20000), NULL) == -1
    assert L.kpr_index_draw(SOME, 4, 3, NULL, NULL) == -1
    assert L.kpr_index_draw(NULL, 4, 3, ctypes.c_void_p(0x20000), NULL) == -1
    assert L.kpr_index_draw(SOME, 4, 3, ctypes.c_void_p(0x10008), NULL) == -1       # out on the state
    assert L.kpr_index_draw(SOME, (1 << 20) + 1, 3, ctypes.c_void_p(0x2000000), NULL) == -2


# ------------------------------------------------------------------ the layer surface
def test_convolve_config_round_trip():
    ir = RNG.standard_normal(37)
    layer = kapre.Convolve(ir, mode='same', block_size=512, input_data_format='channels_first', name='rir')
    cfg = layer.get_config()
    assert cfg['mode'] == 'same' and cfg['block_size'] == 512 and cfg['input_data_format'] == 'channels_first'
    assert np.array_equal(np.asarray(cfg['ir']), ir)
    again = kapre.Convolve.from_config(cfg)
    assert again.get_config() == cfg
    two = kapre.Convolve(RNG.standard_normal((2, 5)))
    assert np.asarray(two.get_config()['ir']).shape == (2, 5)
    assert kapre.Convolve.from_config(two.get_config()).get_config() == two.get_config()
    from kapre_amd.keras_shim import get_registered_object
    assert get_registered_object('Kapre>Convolve') is kapre.Convolve
    assert get_registered_object('Kapre>Reverb') is kapre.Reverb
    assert kapre.signal.Convolve is kapre.Convolve and kapre.augmentation.Reverb is kapre.Reverb


@pytest.mark.parametrize("fmt", ["channels_first", "channels_last"])
def test_convolve_output_shape(fmt):
    shape = (None, 2, 1000) if fmt == "channels_first" else (None, 1000, 2)
    want = lambda t: (None, 2, t) if fmt == "channels_first" else (None, t, 2)
    for mode, t in (('full', 1036), ('same', 1000), ('valid', 964)):
        layer = kapre.Convolve(np.ones(37), mode=mode, input_data_format=fmt, input_shape=shape[1:])
        assert layer.compute_output_shape(shape) == want(t)
        assert layer.output_shape == want(t)
    layer = kapre.Convolve(np.ones(37), mode='valid', input_data_format=fmt)
    with pytest.raises(ValueError):
        layer.compute_output_shape(want(36))
    assert layer.compute_output_shape(want(None)) == want(None)


def test_convolve_argument_errors():
    with pytest.raises(ValueError):
        kapre.Convolve(np.ones(4), mode='wrap')
    with pytest.raises(ValueError):
        kapre.Convolve(np.ones(32 * 1024 + 1))
    with pytest.raises(ValueError):
        kapre.Convolve(np.ones(4), block_size=100)
    with pytest.raises(ValueError):
        kapre.Convolve([])
    with pytest.raises(ValueError):
        kapre.Convolve(np.ones(4), input_data_format='weird')
    with pytest.raises(ValueError):
        backend.fftconvolve(np.zeros((1, 8, 1), np.float32), np.ones(4), mode='wrap')


def test_float64_is_a_type_error():
    x = np.zeros((2, 100, 1), dtype=np.float64)
    with pytest.raises(TypeError):
        kapre.Convolve(np.ones(4))(x)
    with pytest.raises(TypeError):
        backend.fftconvolve(x, np.ones(4))
    with pytest.raises(TypeError):
        kapre.Reverb(np.ones((2, 4)))(x, training=True)
    with pytest.raises(ValueError):
        backend.fftconvolve(np.zeros((2, 100), np.float32), np.ones(4))


def test_reverb_without_training_returns_its_input():
    layer = kapre.Reverb(RNG.standard_normal((3, 50)))
    x = np.zeros((2, 100, 1), dtype=np.float32)
    assert layer(x) is x
    assert layer(x, training=False) is x
    assert layer(x, training=None) is x
    assert layer.compute_output_shape((None, 100, 1)) == (None, 100, 1)
    cfg = layer.get_config()
    assert cfg['normalize'] is True and np.asarray(cfg['irs']).shape == (3, 50)
    again = kapre.Reverb.from_config(cfg)
    assert again.get_config() == cfg
    # normalize: unit energy per impulse response, on the host, at construction
    assert np.allclose(np.sum(layer._plan.h ** 2, axis=1), 1.0, rtol=1e-12)
    raw = kapre.Reverb(np.asarray(cfg['irs']), normalize=False)
    assert np.array_equal(raw._plan.h, np.asarray(cfg['irs']))
    with pytest.raises(ValueError):
        kapre.Reverb(np.zeros((2, 4)))


# ------------------------------------------------------------------ records
def test_header_and_exports_agree_on_the_new_entry_points():
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    for name in ("kpr_spec_fir_plan", "kpr_spec_fir_c64", "kpr_index_draw"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _ffi.EXPORTS
        assert hasattr(_ffi.lib(), name)
    assert re.search(r"#define KPR_VERSION 120\b", text)


def test_readme_and_design_name_the_new_kernel():
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "kpr_spec_fir_kernels.h" in readme and "Convolve" in readme and "Reverb" in readme
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "4.18" in design and "k_spec_fir" in design


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='convolve expects a rank-3 waveform batch'):
        kapre.Convolve(np.ones(4))(np.zeros((2, 100), np.float32))
    with pytest.raises(TypeError, match='convolve has float32 kernels only; got a float64 input'):
        kapre.Convolve(np.ones(4))(np.zeros((2, 100, 1), np.float64))
    with pytest.raises(ValueError, match='convolve expects a rank-3 waveform batch'):
        kapre.Convolve(np.ones(4))(np.zeros((2, 100), np.float64))
    with pytest.raises(ValueError, match='convolve expects a rank-3 waveform batch'):
        backend.fftconvolve(np.zeros((2, 100), np.float32), np.ones(4))
    with pytest.raises(TypeError, match='convolve has float32 kernels only; got a float64 input'):
        backend.fftconvolve(np.zeros((2, 100, 1), np.float64), np.ones(4))
    with pytest.raises(ValueError, match='convolve expects a rank-3 waveform batch'):
        backend.fftconvolve(np.zeros((2, 100), np.float64), np.ones(4))
    with pytest.raises(ValueError, match='Reverb expects a rank-3 waveform batch'):
        kapre.Reverb(np.ones((2, 4)))(np.zeros((2, 100), np.float32), training=True)
    with pytest.raises(TypeError, match='Reverb has float32 kernels only; got a float64 input'):
        kapre.Reverb(np.ones((2, 4)))(np.zeros((2, 100, 1), np.float64), training=True)
    with pytest.raises(ValueError, match='Reverb expects a rank-3 waveform batch'):
        kapre.Reverb(np.ones((2, 4)))(np.zeros((2, 100), np.float64), training=True)
