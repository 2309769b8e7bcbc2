"""HPSS without a GPU: the numpy model against scipy and hand-written cases, the softmask rules, parameter validation, the C ABI
surface, and the layer's constructor, config, shapes and exports."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import hpss_model as hm
import kapre_amd as kapre
from conftest import REPO
from kapre_amd import _ffi, backend


# ---- the model -------------------------------------------------------------------------------------------------------------
def _tied(shape, seed):
    """values with many ties (a few levels), some zeros and one negative level"""
    rng = np.random.default_rng(seed)
    return rng.integers(-1, 4, size=shape).astype(np.float32) * np.float32(0.37)


@pytest.mark.parametrize("k", [3, 7, 17, 31])
def test_model_against_scipy(k):
    """median_reflect is scipy.ndimage.median_filter(mode='reflect') on every axis length but 2 (k >= 17), ties included"""
    ndimage = pytest.importorskip("scipy.ndimage")
    for frames in (1, 3, 7, 15, 16, 31, 40, 70):
        x = _tied((frames, 6), frames * 100 + k)
        assert np.array_equal(hm.median_reflect(x, k, 0), ndimage.median_filter(x, size=(k, 1), mode='reflect')), (k, frames)
    for freq in (1, 5, 17, 33, 65):
        x = _tied((5, freq), freq * 100 + k)
        assert np.array_equal(hm.median_reflect(x, k, 1), ndimage.median_filter(x, size=(1, k), mode='reflect')), (k, freq)


def test_reflect_index():
    assert hm.reflect_index(np.arange(-5, 9), 4).tolist() == [3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0]     # d c b a | a b c d | d c b a
    assert hm.reflect_index(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert hm.reflect_index(np.arange(-4, 6), 2).tolist() == [0, 1, 1, 0, 0, 1, 1, 0, 0, 1]


@pytest.mark.parametrize("k, centre_wins", [(3, True), (5, False), (7, False), (9, True), (17, True), (31, False)])
def test_axis_of_length_two_by_hand(k, centre_wins):
    """n = 2, x = (a, b): r() reads ... a | a b | b a | a b | b a ..., index i holding a when i mod 4 is 0 or 3.  Counted by hand,
    the window of k taps centred on a holds a 2, 2, 3, 5, 9, 15 times for k = 3, 5, 7, 9, 17, 31: more than half of k for
    k = 3, 9, 17 (the centre is the median) and less than half for k = 5, 7, 31 (the neighbour is).  By symmetry the same
    holds centred on b."""
    a, b = 1.0, 5.0
    x = np.array([[a], [b]], np.float32)
    got = hm.median_reflect(x, k, 0)
    assert got.tolist() == ([[a], [b]] if centre_wins else [[b], [a]])
    assert np.array_equal(hm.median_reflect(x.T.copy(), k, 1), got.T)


def test_median_is_a_selection_with_nan_last():
    x = np.array([3.0, np.nan, 1.0, np.inf, 2.0, -0.0, 7.0], np.float32)[:, None]
    got = hm.median_reflect(x, 3, 0)[:, 0]
    assert got.dtype == np.float32
    # windows: (3 3 nan) (3 nan 1) (nan 1 inf) (1 inf 2) (inf 2 -0) (2 -0 7) (-0 7 7)
    assert np.array_equal(got, np.array([3.0, 3.0, np.inf, 2.0, 2.0, 2.0, 7.0], np.float32))
    x[1, 0] = np.inf
    assert np.array_equal(hm.median_reflect(x, 3, 0)[:, 0], got)          # an isolated NaN acts as +Inf


def test_softmask_rules():
    z = np.zeros(4)
    assert np.array_equal(hm.softmask(z, z, 2.0, True), np.full(4, 0.5))
    assert np.array_equal(hm.softmask(z, z * 3.0, 2.0, False), np.zeros(4))
    assert np.array_equal(hm.softmask(z + 2.0 ** -130, z, 1.0, True), np.full(4, 0.5))
    X, R = np.array([1.0, 2.0, 2.0, 0.0]), np.array([2.0, 1.0, 2.0, 0.0])
    assert np.array_equal(hm.softmask(X, R, np.inf), np.array([0.0, 1.0, 0.0, 0.0]))
    np.testing.assert_allclose(hm.softmask(X, R, 1.0)[:3], [1 / 3, 2 / 3, 0.5], rtol=1e-15)
    np.testing.assert_allclose(hm.softmask(X, R, 2.0)[:3], [0.2, 0.8, 0.5], rtol=1e-15)
    rng = np.random.default_rng(1)
    S = (rng.random((40, 33)) * (rng.random((40, 33)) > 0.3)).astype(np.float32)
    for power in (0.5, 1.0, 2.0, 3.0):
        Mh, Mp = hm.hpss_model(S, 7, 5, power, 1.0, 1.0, True)
        np.testing.assert_allclose(Mh + Mp, 1.0, rtol=0, atol=4e-16)
        h, p = hm.hpss_model(S, 7, 5, power, 1.0, 1.0, False)
        np.testing.assert_allclose(h + p, S.astype(np.float64), rtol=1e-15)
    Mh, Mp = hm.hpss_model(S, 7, 5, 2.0, 2.0, 3.0, True)
    assert (Mh + Mp <= 1.0 + 1e-15).all() and (Mh[S == 0][:1] >= 0).all()
    H, P = hm.medians(S, 7, 5)
    assert ((H == 0) & (P == 0)).any() and (Mh[(H == 0) & (P == 0)] == 0).all()


# ---- parameters ------------------------------------------------------------------------------------------------------------
def test_parameters():
    assert backend.hpss_parameters() == ((31, 31), 2.0, (1.0, 1.0))
    assert backend.hpss_parameters((17, 7), 1, (1, 2.5)) == ((17, 7), 1.0, (1.0, 2.5))
    assert backend.hpss_parameters(np.int64(3), np.float32(0.5), [np.float64(3.0), 1]) == ((3, 3), 0.5, (3.0, 1.0))
    assert backend.hpss_parameters(5.0, float('inf'))[:2] == ((5, 5), float('inf'))


@pytest.mark.parametrize("kwargs", [
    dict(kernel_size=30), dict(kernel_size=1), dict(kernel_size=33), dict(kernel_size=(31, 4)), dict(kernel_size=(2, 31)),
    dict(kernel_size=True), dict(kernel_size=7.5), dict(kernel_size=(3, 5, 7)), dict(kernel_size="7"), dict(kernel_size=None),
    dict(margin=0.99), dict(margin=(1.0, 0.5)), dict(margin=float('nan')), dict(margin=float('inf')), dict(margin=False),
    dict(margin=(1, 2, 3)), dict(power=0), dict(power=-1.0), dict(power=float('nan')), dict(power=True), dict(power=(1, 2)),
    dict(power="2"),
])
def test_parameters_are_validated(kwargs):
    with pytest.raises(ValueError):
        backend.hpss_parameters(**kwargs)
    with pytest.raises(ValueError):
        kapre.HPSS(**kwargs)
    with pytest.raises(ValueError):
        kapre.get_hpss_layer(**kwargs)


def test_output_and_format_are_validated():
    with pytest.raises(ValueError):
        kapre.HPSS(output='residual')
    with pytest.raises(ValueError):
        kapre.HPSS(data_format='channels_middle')
    with pytest.raises(ValueError):
        kapre.get_hpss_layer(output='all')
    with pytest.raises(ValueError):
        backend.hpss(np.zeros((1, 9, 17, 1), np.float32), data_format='channels_middle')


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
NAMES = ("kpr_hpss_plan", "kpr_hpss_f32", "kpr_hpss_c64")


def test_abi_surface():
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
    for name in NAMES[1:]:
        assert _ffi.EXPORTS[name][1][-1] is ctypes.c_void_p               # the stream comes last
        assert len(_ffi.EXPORTS[name][1]) == 16
        m = re.search(r"int %s\(([^;]*)\);" % name, text, flags=re.S)
        assert m and len(m.group(1).split(",")) == 16
        assert re.search(r"out_h, \w+\*? ?\*? ?out_p, int out_ch, kpr_stream_t stream$", m.group(1))
    assert len(_ffi.EXPORTS["kpr_hpss_plan"][1]) == 6
    assert _ffi.lib().kpr_version() == 120
    for fn in ("hpss_plan", "hpss"):
        assert callable(getattr(_ffi, fn))
    assert "kpr_hpss_kernels.h" in open(os.path.join(REPO, "kapre_amd", "csrc", "kapre_hip.hip")).read()


def _hpss_rc(fn, x, batch, ch, frames, freq, layout=0, kh=31, kp=31, power=2.0, mh=1.0, mp=1.0, mask=0, out_h=None, out_p=None,
             out_ch=None):
    return getattr(_ffi.lib(), fn)(x, batch, ch, frames, freq, layout, kh, kp, power, mh, mp, mask, out_h, out_p,
                                   ch if out_ch is None else out_ch, None)


def test_plan_and_empty_shapes():
    tf, tq = _ffi.hpss_plan(434, 513)
    assert tf > 0 and tq > 0
    assert _ffi.hpss_plan(0, 0, 3, 31) == (tf, tq) and _ffi.hpss_plan(1, 10 ** 6, 17, 7) == (tf, tq)
    L = _ffi.lib()
    ints = lambda: (ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int()))
    assert L.kpr_hpss_plan(-1, 4, 31, 31, *ints()) == -1
    assert L.kpr_hpss_plan(4, 4, 31, 31, None, ints()[0]) == -1
    for kh, kp in ((30, 31), (31, 2), (1, 31), (31, 33), (-3, 5)):
        assert L.kpr_hpss_plan(4, 4, kh, kp, *ints()) == -1
        assert b"odd" in L.kpr_last_error()
    for fn in NAMES[1:]:
        # an empty shape returns 0 before any pointer is looked at and before the device is asked for
        for batch, ch, frames, freq in ((0, 1, 5, 9), (2, 0, 5, 9), (2, 1, 0, 9), (2, 1, 5, 0)):
            assert _hpss_rc(fn, None, batch, ch, frames, freq) == 0
        assert _hpss_rc(fn, None, -1, 1, 5, 9) == -1
        assert _hpss_rc(fn, None, 1, 1, 5, 9, layout=2) == -1
        for kh, kp in ((30, 31), (31, 2), (1, 31), (31, 33)):
            assert _hpss_rc(fn, None, 0, 1, 5, 9, kh=kh, kp=kp) == -1
        assert _hpss_rc(fn, None, 0, 1, 5, 9, mh=0.5) == -1 and _hpss_rc(fn, None, 0, 1, 5, 9, mp=0.999) == -1
        assert _hpss_rc(fn, None, 0, 1, 5, 9, power=0.0) == -1 and _hpss_rc(fn, None, 0, 1, 5, 9, power=float('nan')) == -1
        assert _hpss_rc(fn, None, 0, 1, 5, 9, power=float('inf')) == 0
        assert _hpss_rc(fn, None, 0, 1, 5, 9, mask=3) == -1
        assert _hpss_rc(fn, None, 1, 2, 5, 9, out_ch=1) == -1
        assert _hpss_rc(fn, None, 1, 1, 2 ** 20, 2 ** 10) == -2
        assert b"2^30" in L.kpr_last_error()
        assert _hpss_rc(fn, None, 1, 1, 5, 9) == -1                        # x is NULL


# ---- the layer -------------------------------------------------------------------------------------------------------------
def test_exports():
    assert "HPSS" in kapre.__all__ and "HPSS" in kapre.time_frequency.__all__
    assert "get_hpss_layer" in kapre.__all__
    assert kapre.HPSS is kapre.time_frequency.HPSS
    assert kapre.get_hpss_layer is kapre.composed.get_hpss_layer
    assert kapre.keras_shim.get_registered_object('Kapre>HPSS') is kapre.HPSS
    for fn in ("hpss_parameters", "hpss"):
        assert callable(getattr(backend, fn))
    assert "grad_fn" in kapre.HPSS.__doc__ and "detached" in kapre.HPSS.__doc__


def test_inputs_are_checked_before_the_device():
    layer = kapre.HPSS()
    with pytest.raises(ValueError):
        layer(np.zeros((9, 129, 1), np.float32))
    with pytest.raises(TypeError):
        layer(np.zeros((1, 9, 129, 1), np.float64))
    with pytest.raises(TypeError):
        layer(np.zeros((1, 9, 129, 1), np.complex128))
    with pytest.raises(TypeError):
        kapre.HPSS(dtype='float64')(np.zeros((1, 9, 129, 1), np.float32))
    with pytest.raises(TypeError):
        backend.hpss(np.zeros((1, 9, 129, 1), np.float64))
    with pytest.raises(ValueError):
        backend.hpss(np.zeros((1, 9, 129), np.float32))
    import torch
    with pytest.raises(TypeError):
        layer(torch.zeros((1, 9, 129, 1), dtype=torch.complex128))
    with pytest.raises(TypeError):
        layer(torch.zeros((1, 9, 129, 1), dtype=torch.float64))


def test_config_round_trip(tmp_path):
    layer = kapre.HPSS(kernel_size=(17, 7), power=1, margin=(1.0, 2.5), output='percussive', mask=True,
                       data_format='channels_first', name='hp')
    cfg = layer.get_config()
    assert cfg['kernel_size'] == [17, 7] and cfg['power'] == 1.0 and cfg['margin'] == [1.0, 2.5]
    assert cfg['output'] == 'percussive' and cfg['mask'] is True and cfg['data_format'] == 'channels_first'
    again = kapre.HPSS.from_config(cfg)
    assert again.get_config() == cfg and again.name == 'hp' and again.data_format == 'channels_first'
    assert again.kernel_size == (17, 7) and again.margin == (1.0, 2.5)
    json.dumps(cfg)
    assert kapre.HPSS().get_config()['output'] == 'both' and kapre.HPSS().kernel_size == (31, 31)
    from kapre_amd.keras_shim import load_model
    model = kapre.Sequential([kapre.STFT(n_fft=256, hop_length=64, input_shape=(4000, 1)), layer])
    path = str(tmp_path / "hpss_model")
    model.save(path)
    loaded = load_model(path)
    assert isinstance(loaded.layers[-1], kapre.HPSS)
    assert loaded.layers[-1].get_config() == cfg and loaded.output_shape == model.output_shape
    chain = kapre.get_hpss_layer(n_fft=512, hop_length=128, output='both', margin=(2.0, 3.0), input_shape=(16000, 1))
    path = str(tmp_path / "hpss_chain")
    chain.save(path)
    loaded = load_model(path)
    assert [type(l).__name__ for l in loaded.layers] == ['STFT', 'HPSS', 'InverseSTFT']
    assert loaded.layers[1].get_config() == chain.layers[1].get_config() and loaded.output_shape == chain.output_shape


def test_output_shapes():
    for output, mult in (('harmonic', 1), ('percussive', 1), ('both', 2)):
        last = kapre.HPSS(output=output)
        assert last.compute_output_shape((None, 7, 257, 3)) == (None, 7, 257, 3 * mult)
        assert last.compute_output_shape((4, None, 257, None)) == (4, None, 257, None)
        first = kapre.HPSS(output=output, data_format='channels_first')
        assert first.compute_output_shape((None, 3, 7, 257)) == (None, 3 * mult, 7, 257)
        for fmt, shape, axis, ch_axis in (('channels_last', (16000, 1), 0, 1), ('channels_first', (2, 16000), 1, 0)):
            model = kapre.get_hpss_layer(n_fft=512, hop_length=128, output=output, input_shape=shape, input_data_format=fmt)
            assert [type(l).__name__ for l in model.layers] == ['STFT', 'HPSS', 'InverseSTFT']
            frames = 1 + (16000 - 512) // 128
            want = list(shape)
            want[axis] = (frames - 1) * 128 + 512
            want[ch_axis] *= mult
            assert model.output_shape == (None,) + tuple(want), (fmt, output)
    model = kapre.get_hpss_layer()
    stft, hp, inv = model.layers
    assert stft.n_fft == 2048 and stft.hop_length == 512 and stft.win_length == 2048 and stft.window_name == 'hann_window'
    assert not stft.pad_begin and not stft.pad_end and inv.forward_window_name == 'hann_window'
    assert hp.output == 'harmonic' and hp.kernel_size == (31, 31) and hp.power == 2.0 and hp.margin == (1.0, 1.0)
    stft = kapre.get_hpss_layer(n_fft=1024, win_length=800).layers[0]
    assert stft.win_length == 800 and stft.hop_length == 200


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='HPSS expects a rank-4 input'):
        kapre.HPSS()(np.zeros((9, 129, 1), np.float32))
    with pytest.raises(TypeError, match='HPSS has float32 kernels only; got a float64 input'):
        kapre.HPSS()(np.zeros((1, 9, 129, 1), np.float64))
    with pytest.raises(ValueError, match='HPSS expects a rank-4 input'):
        kapre.HPSS()(np.zeros((9, 129, 1), np.float64))
    with pytest.raises(ValueError, match='HPSS expects a rank-4 input'):
        backend.hpss(np.zeros((9, 129, 1), np.float32))
    with pytest.raises(TypeError, match='HPSS has float32 kernels only; got a float64 input'):
        backend.hpss(np.zeros((1, 9, 129, 1), np.float64))
    with pytest.raises(ValueError, match='HPSS expects a rank-4 input'):
        backend.hpss(np.zeros((9, 129, 1), np.float64))
    with pytest.raises(TypeError, match='HPSS has float32 kernels only; got a complex128 input'):
        kapre.HPSS()(np.zeros((1, 9, 129, 1), np.complex128))
    with pytest.raises(ValueError, match='HPSS expects a rank-4 input'):
        kapre.HPSS()(np.zeros((9, 129, 1), np.complex128))
