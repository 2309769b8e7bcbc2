"""TimeStretch without a GPU: the two float64 models agree (why the layer has no hop_length), the index tables, the C ABI
surface, and the layer's constructor, config, shapes and exports."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import time_stretch_model as tsm
import kapre_amd as kapre
from conftest import REPO
from kapre_amd import _ffi, backend

RATES = [0.5, 0.8, 1.0, 1.3, 2.0]


# ---- the models --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [64, 160, 256])
@pytest.mark.parametrize("frames", [1, 2, 50, 1000])
def test_textbook_and_definition_agree(frames, hop):
    """the expected phase advance drops out: within 1e-7 of the largest magnitude, whatever the hop length"""
    X = tsm.random_spectrum((frames, 9), seed=frames + hop)
    worst = 0.0
    for rate in RATES:
        idx, alpha = tsm.table(frames, rate)
        a, b = tsm.textbook(X, rate, hop), tsm.definition(X, idx, alpha)
        assert a.shape == b.shape == (len(idx), 9)
        worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(X))))
    print("textbook against definition, frames %d hop %d: %.2e of the largest magnitude" % (frames, hop, worst))
    assert worst <= 1e-7


def test_model_identity_and_words():
    X = tsm.random_spectrum((20, 5), seed=3)
    X[4, 1] = 0.0
    X[5, 2] = -3.0                                                       # angle pi
    idx, alpha = tsm.table(20, 1.0)
    th = tsm.angle_words(X)
    assert th[4, 1] == 0 and th[5, 2] == 2 ** 31
    assert np.array_equal(tsm.phase_words(th, idx), th)                  # rate 1: P[t] = Theta(X[t])
    np.testing.assert_allclose(tsm.definition(X, idx, alpha), X.astype(np.complex128), atol=1e-8)
    # the unrounded sum and the words differ by the words' rounding only
    idx, alpha = tsm.table(20, 0.7)
    d = np.abs(tsm.definition(X, idx, alpha) - tsm.definition(X, idx, alpha, words=False))
    assert d.max() <= np.pi * 2.0 ** -31 * 2 * 20 * np.abs(X).max()
    # the coefficients reproduce the recurrence
    K = tsm.coefficients(20, idx)
    want = (K @ np.concatenate([th, np.zeros((2, 5), np.uint32)]).astype(np.int64)) % 2 ** 32
    assert np.array_equal(want.astype(np.uint32), tsm.phase_words(th, idx))
    out_bound, phase_bound = tsm.bound(X, idx, alpha)
    assert out_bound.shape == phase_bound.shape == (len(idx), 5) and (phase_bound >= 2.0 ** -25).all()


# ---- the tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES + [1 / 3, 0.1, 0.3, 3.7, 1 / 7, 2.5, 0.6])
@pytest.mark.parametrize("frames", [1, 2, 3, 5, 7, 50, 99, 1000])
def test_table(frames, rate):
    idx, alpha = backend.time_stretch_table(frames, rate)
    n = len(idx)
    assert idx.dtype == np.int32 and alpha.dtype == np.float32 and len(alpha) == n
    assert n == backend.time_stretch_length(frames, rate)
    assert abs(n - frames / rate) < 1 + 1e-9 and n >= 1
    if rate in RATES or rate in (2.5,):                                  # rates whose products are exact enough in float64
        assert n == math.ceil(frames / rate)
    assert idx[0] == 0 and alpha[0] == 0 and (np.diff(idx) >= 0).all()
    assert (alpha >= 0).all() and (alpha < 1).all()
    assert idx[-1] <= frames - 1 and math.floor(n * float(rate)) >= frames        # the last frame that starts inside the input
    s = np.arange(n) * float(rate)
    assert np.array_equal(idx, np.floor(s).astype(np.int32))
    np.testing.assert_allclose(alpha, s - np.floor(s), atol=2.0 ** -24)
    m_idx, m_alpha = tsm.table(frames, rate)
    assert np.array_equal(idx, m_idx) and np.array_equal(alpha, m_alpha)


def test_table_edges():
    assert backend.time_stretch_length(0, 0.5) == 0 and backend.time_stretch_length(None, 0.5) is None
    idx, alpha = backend.time_stretch_table(0, 2.0)
    assert len(idx) == 0 and len(alpha) == 0
    assert backend.time_stretch_length(3, 100.0) == 1


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NAMES = ("kpr_time_stretch_plan", "kpr_time_stretch_c64")


def test_abi_surface():
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
    assert _ffi.EXPORTS["kpr_time_stretch_c64"][1][-1] is ctypes.c_void_p            # the stream comes last
    assert len(_ffi.EXPORTS["kpr_time_stretch_c64"][1]) == 10
    assert re.search(r"uint32_t\*\s*phase_out[^;]*kpr_stream_t stream\);", text, flags=re.S)
    assert _ffi.lib().kpr_version() == 120
    for fn in ("time_stretch_plan", "time_stretch"):
        assert callable(getattr(_ffi, fn))
    assert "kpr_time_stretch_kernels.h" in open(os.path.join(REPO, "kapre_amd", "csrc", "kapre_hip.hip")).read()


def test_plan_and_empty_shapes():
    rows, waves = _ffi.time_stretch_plan(100, 513)
    assert rows > 0 and waves > 0
    assert _ffi.time_stretch_plan(0, 0) == (rows, waves)                 # the same for every shape
    L = _ffi.lib()
    assert L.kpr_time_stretch_plan(-1, 4, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) == -1
    assert L.kpr_time_stretch_plan(4, 4, None, ctypes.byref(ctypes.c_int())) == -1
    # an empty shape returns 0 before any pointer is looked at and before the device is asked for
    for outer, f_in, f_out, inner in ((0, 5, 10, 4), (3, 5, 0, 4), (3, 5, 10, 0), (3, 0, 0, 4)):
        assert L.kpr_time_stretch_c64(None, outer, f_in, f_out, inner, None, None, None, None, None) == 0
    assert L.kpr_time_stretch_c64(None, -1, 5, 10, 4, None, None, None, None, None) == -1
    assert L.kpr_time_stretch_c64(None, 1, 2 ** 20, 4, 2 ** 10, None, None, None, None, None) == -2
    assert b"2^30" in L.kpr_last_error()
    assert L.kpr_time_stretch_c64(None, 1, 4, 2 ** 20, 2 ** 10, None, None, None, None, None) == -2


# ---- the layer -----------------------------------------------------------------------------------------------------------
def test_exports():
    assert "TimeStretch" in kapre.__all__ and "TimeStretch" in kapre.time_frequency.__all__
    assert "get_time_stretch_layer" in kapre.__all__
    assert kapre.TimeStretch is kapre.time_frequency.TimeStretch
    assert kapre.get_time_stretch_layer is kapre.composed.get_time_stretch_layer
    assert kapre.keras_shim.get_registered_object('Kapre>TimeStretch') is kapre.TimeStretch
    for fn in ("time_stretch_parameters", "time_stretch_table", "phase_vocoder"):
        assert callable(getattr(backend, fn))
    assert "hop_length" in kapre.TimeStretch.__doc__ and "2^32" in kapre.TimeStretch.__doc__


@pytest.mark.parametrize("rate", [0, 0.0, -1.0, float('nan'), float('inf'), True, False, "2", None, [1.0], np.array([1.0, 2.0])])
def test_rate_is_validated(rate):
    with pytest.raises(ValueError):
        kapre.TimeStretch(rate)
    with pytest.raises(ValueError):
        backend.time_stretch_parameters(rate)
    with pytest.raises(ValueError):
        kapre.get_time_stretch_layer(rate)


def test_inputs_are_checked_before_the_device():
    layer = kapre.TimeStretch(0.8)
    with pytest.raises(ValueError):
        layer(np.zeros((9, 129, 1), np.complex64))
    with pytest.raises(TypeError):
        layer(np.zeros((1, 9, 129, 1), np.float32))
    with pytest.raises(TypeError):
        layer(np.zeros((1, 9, 129, 1), np.complex128))
    with pytest.raises(TypeError):
        kapre.TimeStretch(0.8, dtype='float64')(np.zeros((1, 9, 129, 1), np.complex64))
    with pytest.raises(TypeError):
        backend.phase_vocoder(np.zeros((1, 9, 129, 1), np.float64), 0.8)
    with pytest.raises(ValueError):
        backend.phase_vocoder(np.zeros((1, 9, 129, 1), np.complex64), 0.8, data_format='channels_middle')
    with pytest.raises(ValueError):
        kapre.TimeStretch(0.8, data_format='channels_middle')
    import torch
    with pytest.raises(TypeError):
        layer(torch.zeros((1, 9, 129, 1), dtype=torch.complex128))
    with pytest.raises(TypeError):
        layer(torch.zeros((1, 9, 129, 1), dtype=torch.float32))


def test_config_round_trip(tmp_path):
    layer = kapre.TimeStretch(1.25, data_format='channels_first', name='ts')
    cfg = layer.get_config()
    assert cfg['rate'] == 1.25 and cfg['data_format'] == 'channels_first'
    again = kapre.TimeStretch.from_config(cfg)
    assert again.get_config() == cfg and again.name == 'ts' and again.data_format == 'channels_first'
    assert kapre.TimeStretch(2).rate == 2.0 and isinstance(kapre.TimeStretch(2).rate, float)
    assert kapre.TimeStretch(np.float32(0.5)).get_config()['rate'] == 0.5
    import json
    json.dumps(cfg)
    from kapre_amd.keras_shim import load_model
    model = kapre.Sequential([kapre.STFT(n_fft=256, hop_length=64, input_shape=(4000, 1)), layer])
    path = str(tmp_path / "ts_model")
    model.save(path)
    loaded = load_model(path)
    assert isinstance(loaded.layers[-1], kapre.TimeStretch)
    assert loaded.layers[-1].get_config() == cfg and loaded.output_shape == model.output_shape


def test_output_shapes():
    layer = kapre.TimeStretch(0.8)
    assert layer.compute_output_shape((None, 7, 257, 2)) == (None, 9, 257, 2)
    assert layer.compute_output_shape((4, None, 257, 1)) == (4, None, 257, 1)
    assert layer.compute_output_shape((4, 0, 257, 1)) == (4, 0, 257, 1)
    first = kapre.TimeStretch(2.0, data_format='channels_first')
    assert first.compute_output_shape((None, 2, 7, 257)) == (None, 2, 4, 257)
    assert first.compute_output_shape((None, 2, None, 257)) == (None, 2, None, 257)
    for fmt, shape, axis in (('channels_last', (16000, 1), 0), ('channels_first', (2, 16000), 1)):
        for rate in (0.5, 1.0, 1.3, 2.0):
            model = kapre.get_time_stretch_layer(rate, n_fft=512, hop_length=128, input_shape=shape, input_data_format=fmt)
            assert [type(l).__name__ for l in model.layers] == ['STFT', 'TimeStretch', 'InverseSTFT']
            frames = 1 + (16000 - 512) // 128
            want = list(shape)
            want[axis] = (math.ceil(frames / rate) - 1) * 128 + 512
            assert model.output_shape == (None,) + tuple(want), (fmt, rate)
    stft = kapre.get_time_stretch_layer(0.5).layers[0]
    assert stft.n_fft == 2048 and stft.hop_length == 512 and stft.win_length == 2048 and stft.window_name == 'hann_window'
    assert not stft.pad_begin and not stft.pad_end
    assert kapre.get_time_stretch_layer(0.5).layers[2].forward_window_name == 'hann_window'


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='TimeStretch expects a rank-4 input'):
        kapre.TimeStretch(0.8)(np.zeros((9, 129, 1), np.complex64))
    with pytest.raises(TypeError, match='TimeStretch has float32 kernels only; got a complex128 input'):
        kapre.TimeStretch(0.8)(np.zeros((1, 9, 129, 1), np.complex128))
    with pytest.raises(ValueError, match='TimeStretch expects a rank-4 input'):
        kapre.TimeStretch(0.8)(np.zeros((9, 129, 1), np.complex128))
    with pytest.raises(ValueError, match='TimeStretch expects a rank-4 input'):
        backend.phase_vocoder(np.zeros((9, 129, 1), np.complex64), 0.8)
    with pytest.raises(TypeError, match='TimeStretch has float32 kernels only; got a complex128 input'):
        backend.phase_vocoder(np.zeros((1, 9, 129, 1), np.complex128), 0.8)
    with pytest.raises(ValueError, match='TimeStretch expects a rank-4 input'):
        backend.phase_vocoder(np.zeros((9, 129, 1), np.complex128), 0.8)
    with pytest.raises(TypeError, match='TimeStretch expects a complex spectrogram'):
        kapre.TimeStretch(0.8)(np.zeros((1, 9, 129, 1), np.float64))
    with pytest.raises(ValueError, match='TimeStretch expects a rank-4 input'):
        kapre.TimeStretch(0.8)(np.zeros((9, 129, 1), np.float64))
