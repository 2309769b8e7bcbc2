"""CMVN without a GPU: the numpy model of tests/cmvn_model.py against independent forms of the definition, the evidence that the
GPU test's yardstick tells a shifted evaluation from an unshifted one, and the host side of the feature (layer configuration,
validation, exports, the C ABI's host-only calls)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import cmvn_model as cm
import kapre_amd as kapre
from conftest import REPO, rel_err
from kapre_amd import _ffi, backend


def _inputs(shape=(2, 37, 5), seed=0):
    rng = np.random.default_rng(seed)
    return [rng.random(shape), -60 + 3 * rng.normal(size=shape), np.exp(rng.normal(-6, 3, shape))]


def offset_inputs(frames, seed=11):
    """the two inputs the contract's shift exists for, as float32 (frames, 256): -60 + 0.1 N(0, 1) and 1000 + N(0, 1)"""
    g = np.random.default_rng(seed).normal(size=(frames, 256))
    return {"-60 +- 0.1": (-60 + 0.1 * g).astype(np.float32), "1000 +- 1": (1000 + g).astype(np.float32)}


def unshifted_float32(x, norm_vars, eps=1e-5):
    """the float32 model's sums (two passes, sequential, time on axis 0) WITHOUT the shift by x[0]"""
    f32 = np.float32
    n = f32(x.shape[0])
    s = np.zeros(x.shape[1:], f32)
    for row in x:
        s = s + row
    c = x - s / n
    q = np.zeros(x.shape[1:], f32)
    for row in c:
        q = q + row * row
    assert c.dtype == f32 and q.dtype == f32
    return c * (f32(1) / np.sqrt(q / n + f32(eps))) if norm_vars else c


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("norm_vars", [True, False])
def test_model_is_mean_and_population_variance(norm_vars):
    for x in _inputs():
        for eps in (1e-5, 0.0, 0.3):
            m, v = np.mean(x, axis=1, keepdims=True), np.var(x, axis=1, keepdims=True)
            want = (x - m) / np.sqrt(v + eps) if norm_vars else x - m
            got = cm.cmvn(x, norm_vars, eps, axis=1)
            assert got.dtype == np.float64 and np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    assert cm.cmvn(np.zeros((2, 0, 3)), norm_vars, axis=1).shape == (2, 0, 3)
    const = cm.cmvn(np.full((1, 9, 2), -80.0), norm_vars, axis=1)
    assert const.tobytes() == np.zeros((1, 9, 2)).tobytes()                       # +0.0, bit for bit


@pytest.mark.parametrize("norm_vars", [True, False])
def test_model_gradient_against_torch_autograd(norm_vars):
    import torch

    for x in _inputs((2, 13, 3), seed=5):
        gy = np.random.default_rng(6).normal(size=x.shape)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        c = xt - xt.mean(dim=1, keepdim=True)
        y = c / torch.sqrt(xt.var(dim=1, unbiased=False, keepdim=True) + 1e-5) if norm_vars else c
        y.backward(torch.tensor(gy))
        want = xt.grad.numpy()
        got = cm.cmvn_grad(x, gy, norm_vars, 1e-5, axis=1)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
        assert np.max(np.abs(got.sum(axis=1))) <= 1e-12 * np.max(np.abs(want))     # the centring: sum over t of gx is 0


@pytest.mark.parametrize("norm_vars", [True, False])
def test_model_gradient_against_central_differences(norm_vars):
    x = _inputs((1, 9, 2), seed=3)[0]
    gy = np.random.default_rng(4).normal(size=x.shape)
    got = cm.cmvn_grad(x, gy, norm_vars, 1e-5, axis=1)
    want = np.empty_like(x)
    h = 1e-6
    for idx in np.ndindex(x.shape):
        up, dn = x.copy(), x.copy()
        up[idx] += h
        dn[idx] -= h
        want[idx] = np.sum(gy * (cm.cmvn(up, norm_vars, axis=1) - cm.cmvn(dn, norm_vars, axis=1))) / (2 * h)
    assert np.max(np.abs(got - want)) <= 1e-6 * np.max(np.abs(want))


@pytest.mark.parametrize("norm_vars", [True, False])
@pytest.mark.parametrize("frames", [83, 998])
def test_the_yardstick_tells_the_shift_from_its_absence(frames, norm_vars):
    """On data far from 0 the float32 model (shifted) stays within 1e-6 of the oracle, and the same float32 sums without the shift
    land outside the limit of tests/test_cmvn_gpu.py: min(max(8 x float32 model, first-order bound), 1e-4)."""
    plan = _ffi.cmvn_plan(frames, 256)
    for name, x in offset_inputs(frames).items():
        y64 = cm.cmvn(x, norm_vars, axis=0)
        e32 = rel_err(cm.cmvn(x, norm_vars, axis=0, dtype=np.float32), y64)
        bound = cm.first_order_bound(x, norm_vars, axis=0, plan=plan)
        limit = min(max(8 * e32, bound), 1e-4)
        plain = rel_err(unshifted_float32(x, norm_vars), y64)
        print("cmvn F=%d %s norm_vars=%d: float32 model %.3e | bound %.3e | limit %.3e | unshifted float32 %.3e"
              % (frames, name, norm_vars, e32, bound, limit, plain))
        assert e32 <= 1e-6
        assert e32 <= bound <= 1e-4                              # the bound covers the plain float32 evaluation it describes
        assert plain > limit


def test_float32_model_rounds_every_operation():
    x = _inputs((2, 50, 4), seed=8)[1].astype(np.float32)
    y32 = cm.cmvn(x, axis=1, dtype=np.float32)
    g32 = cm.cmvn_grad(x, x[::-1], axis=1, dtype=np.float32)
    assert y32.dtype == np.float32 and g32.dtype == np.float32
    assert 0 < rel_err(y32, cm.cmvn(x, axis=1)) <= cm.first_order_bound(x, axis=1)
    assert cm.chain_length(83, (16, 8, 128)) == 16 + 8 + 1 and cm.chain_length(259, (16, 8, 128)) == 16 + 8 + 3


# ------------------------------------------------------------------ layer and backend, host side
def test_exports():
    assert "CMVN" in kapre.__all__ and "CMVN" in kapre.time_frequency.__all__
    assert kapre.CMVN is kapre.time_frequency.CMVN and callable(backend.cmvn)
    assert callable(_ffi.cmvn_plan) and callable(_ffi.cmvn) and callable(_ffi.cmvn_bwd)


def test_config_round_trip_and_serialisation():
    layer = kapre.CMVN(norm_vars=False, eps=1e-3, data_format="channels_first", name="cmvn_x")
    cfg = layer.get_config()
    assert cfg["norm_vars"] is False and cfg["eps"] == 1e-3 and cfg["data_format"] == "channels_first" and cfg["name"] == "cmvn_x"
    again = kapre.CMVN.from_config(json.loads(json.dumps(cfg)))
    assert again.get_config() == cfg
    assert layer.compute_output_shape((None, 2, 83, 40)) == (None, 2, 83, 40)
    d = kapre.CMVN().get_config()
    assert (d["norm_vars"], d["eps"], d["data_format"]) == (True, 1e-5, "default")
    from kapre_amd import keras_shim
    model = keras_shim.Sequential([kapre.CMVN(eps=0.5)])
    assert keras_shim.Sequential.from_config(model.get_config()).layers[-1].get_config()["eps"] == 0.5


@pytest.mark.parametrize("kw", [dict(eps=-1e-6), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=[1e-5]), dict(eps="1e-5"),
                                dict(norm_vars=1), dict(norm_vars=None), dict(norm_vars="yes"),
                                dict(data_format="weird")])
def test_validation_errors(kw):
    with pytest.raises(ValueError):
        kapre.CMVN(**kw)
    if "data_format" not in kw:
        with pytest.raises(ValueError):
            backend.cmvn_parameters(**{**dict(norm_vars=True, eps=1e-5), **kw})


def test_boundary_values_are_accepted():
    kapre.CMVN(eps=0.0, norm_vars=np.bool_(False))
    assert backend.cmvn_parameters(True, 0) == (True, 0.0)


def test_float64_and_rank_are_refused_before_the_device():
    with pytest.raises(NotImplementedError):
        kapre.CMVN(dtype="float64")(np.zeros((1, 4, 3, 1), dtype=np.float32))
    with pytest.raises(NotImplementedError):
        kapre.CMVN()(np.zeros((1, 4, 3, 1), dtype=np.float64))
    for bad in (np.zeros((4, 3, 1), dtype=np.float32), np.zeros((1, 2, 4, 3, 1), dtype=np.float32)):
        with pytest.raises(ValueError, match="rank-4"):
            kapre.CMVN()(bad)
        with pytest.raises(ValueError, match="rank-4"):
            backend.cmvn(bad)


# ------------------------------------------------------------------ C ABI
def test_header_prototypes_and_exports():
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("kpr_cmvn_plan", "kpr_cmvn_f32", "kpr_cmvn_bwd_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
        assert name == "kpr_cmvn_plan" or _ffi.EXPORTS[name][1][-1] is ctypes.c_void_p       # the stream comes last
    assert re.search(r"#define\s+KPR_VERSION\s+120\b", text) and _ffi.lib().kpr_version() == 120
    assert "float* rstd_out" in code and "int* resident_frames" in code
    assert "kpr_cmvn_kernels.h" in open(os.path.join(REPO, "kapre_amd", "csrc", "kapre_hip.hip")).read()


def test_plan_is_shape_independent():
    rows, waves, resident = _ffi.cmvn_plan(83, 128)
    assert rows >= 1 and 1 <= waves <= 16 and resident >= 128 and resident % (rows * waves) == 0
    for shape in ((1, 1), (998, 80), (1 << 20, 4096), (0, 0)):
        assert _ffi.cmvn_plan(*shape) == (rows, waves, resident)
    L = _ffi.lib()
    r_, w_, f_ = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert L.kpr_cmvn_plan(-1, 4, ctypes.byref(r_), ctypes.byref(w_), ctypes.byref(f_)) == -1
    assert L.kpr_cmvn_plan(8, 4, ctypes.byref(r_), ctypes.byref(w_), None) == -1


def test_the_variant_option():
    assert _ffi.set_option("cmvn_variant", 1) == 0
    try:
        assert _ffi.set_option("cmvn_variant", 0) == 1
        with pytest.raises(RuntimeError, match="cmvn_variant"):
            _ffi.set_option("cmvn_variant", 2)
        with pytest.raises(RuntimeError):
            _ffi.set_option("cmvn_variant", -1)
    finally:
        _ffi.set_option("cmvn_variant", 0)


def test_host_only_argument_checks():
    L = _ffi.lib()
    fake, out0, third = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000)
    stat = ctypes.c_void_p(0x300000)                 # never dereferenced: every call below returns before a launch
    null = ctypes.c_void_p(0)

    def fwd(x=fake, outer=2, frames=5, inner=6, norm_vars=1, eps=1e-5, out=out0, rstd_out=null):
        return L.kpr_cmvn_f32(x, outer, frames, inner, norm_vars, eps, out, rstd_out, null)

    def bwd(y=fake, rstd=stat, gy=third, frames=5, inner=6, norm_vars=1, gx=out0):
        return L.kpr_cmvn_bwd_f32(y, rstd, gy, 2, frames, inner, norm_vars, gx, null)

    for zero in (dict(outer=0), dict(frames=0), dict(inner=0)):
        assert fwd(**zero) == 0 and fwd(x=null, out=null, **zero) == 0 and _ffi.last_launches() == ""
    assert bwd(frames=0) == 0 and bwd(inner=0, y=null, rstd=null, gy=null, gx=null) == 0
    for bad in (dict(x=null), dict(out=null), dict(outer=-1), dict(frames=-1), dict(inner=-1), dict(out=fake), dict(eps=-1e-6),
                dict(eps=float("nan")), dict(eps=float("inf")), dict(norm_vars=2), dict(norm_vars=0, rstd_out=stat),
                dict(x=ctypes.c_void_p(0x1002)), dict(rstd_out=fake), dict(rstd_out=out0),
                dict(norm_vars=0, rstd_out=stat, frames=0)):
        assert fwd(**bad) == -1, bad
    assert b"rstd_out" in (fwd(norm_vars=0, rstd_out=stat), L.kpr_last_error())[1]
    for bad in (dict(y=null), dict(rstd=null), dict(gy=null), dict(gx=null), dict(gx=fake), dict(gx=third), dict(gx=stat),
                dict(norm_vars=0, gy=null), dict(norm_vars=-1)):
        assert bwd(**bad) == -1, bad
    # frames * inner reaches 2^31: refused (one element below is not: that call would launch and is not made here)
    assert fwd(frames=1 << 20, inner=1 << 11) == -2 and b"2^31" in L.kpr_last_error()
    assert bwd(frames=1 << 21, inner=1 << 10) == -2


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='CMVN expects a rank-4 input'):
        kapre.CMVN()(np.zeros((4, 3, 1), np.float32))
    with pytest.raises(NotImplementedError, match='CMVN has float32 kernels only; got a float64 input'):
        kapre.CMVN()(np.zeros((1, 4, 3, 1), np.float64))
    with pytest.raises(ValueError, match='CMVN expects a rank-4 input'):
        kapre.CMVN()(np.zeros((4, 3, 1), np.float64))
    with pytest.raises(ValueError, match='CMVN expects a rank-4 input'):
        backend.cmvn(np.zeros((4, 3, 1), np.float32))
    with pytest.raises(NotImplementedError, match='CMVN has float32 kernels only; got a float64 input'):
        backend.cmvn(np.zeros((1, 4, 3, 1), np.float64))
    with pytest.raises(ValueError, match='CMVN expects a rank-4 input'):
        backend.cmvn(np.zeros((4, 3, 1), np.float64))
