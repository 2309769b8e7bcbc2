"""Resample without a GPU: the numpy model of tests/resample_model.py against independent forms of the definition, and the host
side of the feature (the polyphase tables of the C ABI, layer configuration, validation, exports)."""
import ctypes
import os
import re

import numpy as np
import pytest

import kapre_amd as kapre
import resample_model as rm
from conftest import REPO
from kapre_amd import _ffi, backend

RATIOS = [(44100, 16000), (16000, 44100), (48000, 44100), (3, 2), (2, 3), (1, 2), (2, 1)]


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("orig,new", RATIOS)
def test_model_equals_upfirdn(orig, new):
    rng = np.random.default_rng(orig + new)
    for T in (1, 5, 333, 1000):
        x = rng.standard_normal(T)
        y = rm.resample(x, orig, new)
        assert y.shape == (rm.out_length(T, orig, new),)
        want = rm.upfirdn_reference(x, orig, new)
        assert np.max(np.abs(y - want)) <= 1e-12 * np.max(np.abs(y)), (T, np.max(np.abs(y - want)))


@pytest.mark.parametrize("orig,new", RATIOS)
def test_model_equals_the_dense_matrix_of_the_definition(orig, new):
    rng = np.random.default_rng(7)
    for T in (1, 5, 97):
        x = rng.standard_normal((2, T))
        y = rm.resample(x, orig, new)
        want = x @ rm.dense(T, orig, new).T
        assert np.max(np.abs(y - want)) <= 1e-12 * max(np.max(np.abs(want)), 1e-300)
        # other axis, same numbers
        assert np.array_equal(rm.resample(x.T, orig, new, axis=0), y.T)


@pytest.mark.parametrize("orig,new", RATIOS)
def test_model_adjoint_identity(orig, new):
    rng = np.random.default_rng(11)
    for T in (1, 5, 333, 1000):
        x = rng.standard_normal(T)
        y = rm.resample(x, orig, new)
        g = rng.standard_normal(y.shape)
        gx = rm.adjoint(g, T, orig, new)
        assert gx.shape == x.shape
        lhs, rhs = float(np.dot(y, g)), float(np.dot(x, gx))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (T, lhs, rhs)


def test_model_adjoint_equals_torch_autograd_through_the_dense_matrix():
    import torch

    T = 50
    for orig, new in RATIOS:
        rng = np.random.default_rng(5)
        x = torch.tensor(rng.standard_normal(T), dtype=torch.float64, requires_grad=True)
        A = torch.tensor(rm.dense(T, orig, new), dtype=torch.float64)
        y = A @ x
        g = rng.standard_normal(y.shape[0])
        y.backward(torch.tensor(g))
        got = rm.adjoint(g, T, orig, new)
        want = x.grad.numpy()
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_dc_gain_is_the_ripple_of_the_definition():
    y = rm.resample(np.ones(44100), 44100, 16000)
    mid = y[100:-100]
    assert np.all(np.abs(mid - 1.00047) <= 1e-4), (mid.min(), mid.max())


# ------------------------------------------------------------------ the tables of the C ABI
def _rebuild(x, table, first, step, out_len):
    """out[i] = sum_k table[i mod P][k] x[(i div P) step + first[i mod P] + k] in float64"""
    P, n_taps = table.shape
    i = np.arange(out_len)
    b, p = i // P, i % P
    y = np.zeros(out_len)
    for k in range(n_taps):
        n = b * step + first[p] + k
        ok = (n >= 0) & (n < x.shape[0])
        y += np.where(ok, table[p, k].astype(np.float64) * x[np.clip(n, 0, x.shape[0] - 1)], 0.0)
    return y


@pytest.mark.parametrize("orig,new", RATIOS + [(48000, 8000)])
@pytest.mark.parametrize("adjoint", [False, True])
def test_c_tables_against_the_model(orig, new, adjoint):
    P, Q, m_first, m_count = rm.bands(orig, new, adjoint=adjoint)
    n_phases, n_taps, step = _ffi.resample_table_size(orig, new, 6, 0.99, adjoint)
    table, first, step2 = _ffi.resample_table(orig, new, 6, 0.99, adjoint)
    assert (n_phases, step) == (P, Q) and step2 == step and table.shape == (P, n_taps) and first.shape == (P,)
    assert table.dtype == np.float32 and first.dtype == np.int32
    assert m_count.max() <= n_taps <= m_count.max() + 2
    # no tap with a non-zero coefficient outside the model's support
    k = np.arange(n_taps)[None, :]
    j = first[:, None].astype(np.int64) + k
    inside = (j >= m_first[:, None]) & (j < (m_first + m_count)[:, None])
    assert np.all(table[~inside] == 0.0)
    assert np.all(np.diff(first) >= 0)                                   # what the kernel's staged span relies on
    rng = np.random.default_rng(3)
    for T in (1, 5, 333, 1000):
        if adjoint:
            x = rng.standard_normal(rm.out_length(T, orig, new))
            want, budget = rm.adjoint(x, T, orig, new), rm.abs_budget(x, orig, new, adjoint=True, T=T)
        else:
            x = rng.standard_normal(T)
            want, budget = rm.resample(x, orig, new), rm.abs_budget(x, orig, new)
        got = _rebuild(x, table, first, step, want.shape[0])
        assert np.all(np.abs(got - want) <= 2.0 ** -23 * budget + 1e-12), np.max(np.abs(got - want) / (2.0 ** -23 * budget + 1e-12))


def test_table_shapes_the_issue_names():
    assert _ffi.resample_table_size(44100, 16000, 6, 0.99, False) == (160, 34, 441)
    assert _ffi.resample_table_size(44100, 16000, 6, 0.99, True) == (441, 13, 160)
    assert _ffi.resample_table_size(48000, 8000, 6, 0.99, False) == (1, 73, 6)
    rates = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
    for a in rates:
        for b in rates:
            if a != b:
                for adjoint in (False, True):
                    P, n, q = _ffi.resample_table_size(a, b, 6, 0.99, adjoint)
                    assert n <= 128 and P * n * 4 <= 1 << 20
                    tile = _ffi.resample_plan(P, n, q)
                    assert tile >= P and tile % P == 0


# ------------------------------------------------------------------ refusals
def test_refusals():
    L = _ffi.lib()
    with pytest.raises(ValueError, match=r"16001 phases x (about )?\d+ taps = \d+ bytes"):
        kapre.Resample(44100, 16001)
    with pytest.raises(ValueError, match="1 MiB"):
        backend.resample(np.zeros((1, 8, 1), dtype=np.float32), 44100, 16001)
    with pytest.raises(ValueError, match="taps"):                        # 1 phase, but 12 * 40 taps
        kapre.Resample(40, 1)
    out = [ctypes.c_int(0) for _ in range(3)]
    refs = [ctypes.byref(o) for o in out]
    assert L.kpr_resample_table_size(44100, 16001, 6, 0.99, 0, *refs) == -2 and b"bytes" in L.kpr_last_error()
    assert L.kpr_resample_table_size(0, 16000, 6, 0.99, 0, *refs) == -1 and b"positive" in L.kpr_last_error()
    assert L.kpr_resample_table_size(44100, -1, 6, 0.99, 0, *refs) == -1 and b"positive" in L.kpr_last_error()
    assert L.kpr_resample_table_size(2, 1, 0, 0.99, 0, *refs) == -1 and b"lowpass_filter_width" in L.kpr_last_error()
    for bad in (0.0, 1.5, -0.1, float("nan")):
        assert L.kpr_resample_table_size(2, 1, 6, bad, 0, *refs) == -1 and b"rolloff" in L.kpr_last_error()
    assert L.kpr_resample_plan(0, 13, 1, refs[0]) == -1 and L.kpr_resample_plan(2, 129, 1, refs[0]) == -2
    for bad in (0, -44100, 44100.0, "44100", True):
        with pytest.raises(ValueError, match="orig_freq must be a positive integer"):
            kapre.Resample(bad, 16000)
        with pytest.raises(ValueError, match="new_freq must be a positive integer"):
            kapre.Resample(16000, bad)
    for bad in (0.0, 1.0001, -1, float("nan")):
        with pytest.raises(ValueError, match="0 < rolloff <= 1"):
            kapre.Resample(2, 1, rolloff=bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="lowpass_filter_width"):
            kapre.Resample(2, 1, lowpass_filter_width=bad)
    with pytest.raises(TypeError, match="float32"):
        kapre.Resample(2, 1)(np.zeros((1, 8, 1), dtype=np.float64))
    with pytest.raises(TypeError, match="float32"):
        backend.resample(np.zeros((1, 8, 1), dtype=np.float64), 2, 1)
    with pytest.raises(ValueError, match="data_format must be one of"):
        kapre.Resample(2, 1, data_format="channels_middle")
    with pytest.raises(ValueError, match="rank-3"):
        kapre.Resample(2, 1)(np.zeros((8, 1), dtype=np.float32))


def test_launch_entry_argument_checks():
    """every call returns before a launch (no device here): the pointers are never dereferenced"""
    L = _ffi.lib()
    fake, tab, fst, dst, null = (ctypes.c_void_p(v) for v in (0x1000, 0x100000, 0x200000, 0x300000, 0))

    def run(x=fake, batch=2, channels=1, in_len=100, layout=1, table=tab, first=fst, P=2, n_taps=13, step=1, out_len=200, out=dst):
        return L.kpr_resample_f32(x, batch, channels, in_len, layout, table, first, P, n_taps, step, out_len, out, null)

    assert run(batch=0) == 0 and run(out_len=0) == 0 and run(batch=0, x=null, out=null) == 0
    for bad in (dict(x=null), dict(out=null), dict(table=null), dict(first=null), dict(batch=-1), dict(channels=0), dict(in_len=-1),
                dict(layout=2), dict(P=0), dict(n_taps=0), dict(step=0), dict(out=fake), dict(x=ctypes.c_void_p(0x1002))):
        assert run(**bad) == -1, bad
    assert run(n_taps=129) == -2 and run(P=1 << 18, n_taps=13) == -2
    assert run(in_len=1 << 30) == -2 and b"2^30" in L.kpr_last_error()
    assert run(in_len=1 << 29, channels=2) == -2 and b"2^30" in L.kpr_last_error()
    assert run(out_len=1 << 30, layout=0) == -2


# ------------------------------------------------------------------ the layer
@pytest.mark.parametrize("fmt", ["channels_last", "channels_first"])
def test_config_round_trip_and_output_shape(fmt):
    layer = kapre.Resample(44100, 16000, lowpass_filter_width=8, rolloff=0.95, data_format=fmt, name="down")
    config = layer.get_config()
    assert {k: config[k] for k in ("orig_freq", "new_freq", "lowpass_filter_width", "rolloff", "data_format", "name")} == dict(
        orig_freq=44100, new_freq=16000, lowpass_filter_width=8, rolloff=0.95, data_format=fmt, name="down")
    again = kapre.Resample.from_config(config)
    assert again.get_config() == config
    from kapre_amd.keras_shim import get_registered_object
    assert get_registered_object("Kapre>Resample") is kapre.Resample
    for T, want in ((0, 0), (1, 1), (441, 160), (44100, 16000), (None, None), (442, 161)):
        shape = (None, T, 2) if fmt == "channels_last" else (None, 2, T)
        out = (None, want, 2) if fmt == "channels_last" else (None, 2, want)
        assert layer.compute_output_shape(shape) == out
    up = kapre.Resample(16000, 44100, data_format=fmt)
    assert _ffi.dims_of(up.compute_output_shape(_ffi.shape_of(fmt, 3, 1, 5)), fmt) == (3, 1, 14)
    model = kapre.Sequential([kapre.Resample(44100, 16000, input_shape=_ffi.shape_of(fmt, 0, 1, 22050)[1:], data_format=fmt)])
    assert model.output_shape == _ffi.shape_of(fmt, None, 1, 8000)


def test_default_arguments():
    c = kapre.Resample(48000, 16000).get_config()
    assert (c["lowpass_filter_width"], c["rolloff"], c["data_format"]) == (6, 0.99, "default")


def test_identity_returns_its_input_without_a_device():
    x = np.zeros((1, 8, 1), dtype=np.float32)
    assert kapre.Resample(16000, 16000)(x) is x
    assert backend.resample(x, 7, 7) is x


def test_exports():
    assert "Resample" in kapre.__all__ and "Resample" in kapre.signal.__all__
    assert kapre.Resample is kapre.signal.Resample


def test_header_prototypes_and_exports():
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("kpr_resample_table_size", "kpr_resample_table", "kpr_resample_plan", "kpr_resample_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
    assert _ffi.EXPORTS["kpr_resample_f32"][1][-1] is ctypes.c_void_p          # the stream comes last
    assert re.search(r"#define\s+KPR_VERSION\s+120\b", text) and _ffi.lib().kpr_version() == 120


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='resample expects a rank-3 waveform batch'):
        kapre.Resample(2, 1)(np.zeros((8, 1), np.float32))
    with pytest.raises(TypeError, match='resample has float32 kernels only; got a float64 input'):
        kapre.Resample(2, 1)(np.zeros((1, 8, 1), np.float64))
    with pytest.raises(ValueError, match='resample expects a rank-3 waveform batch'):
        kapre.Resample(2, 1)(np.zeros((8, 1), np.float64))
    with pytest.raises(ValueError, match='resample expects a rank-3 waveform batch'):
        backend.resample(np.zeros((8, 1), np.float32), 2, 1)
    with pytest.raises(TypeError, match='resample has float32 kernels only; got a float64 input'):
        backend.resample(np.zeros((1, 8, 1), np.float64), 2, 1)
    with pytest.raises(ValueError, match='resample expects a rank-3 waveform batch'):
        backend.resample(np.zeros((8, 1), np.float64), 2, 1)
    with pytest.raises(ValueError, match='resample expects a rank-3 waveform batch'):
        backend.resample(np.zeros((8, 1), np.float32), 2, 2)
    with pytest.raises(TypeError, match='resample has float32 kernels only; got a float64 input'):
        backend.resample(np.zeros((1, 8, 1), np.float64), 2, 2)
    with pytest.raises(ValueError, match='resample expects a rank-3 waveform batch'):
        backend.resample(np.zeros((8, 1), np.float64), 2, 2)
