"""PCEN without a GPU: the numpy model of tests/pcen_model.py against independent forms of the definition, and the host side of
the feature (layer configuration, validation, exports, the C ABI's host-only calls)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import kapre_amd as kapre
import pcen_model as pm
from conftest import REPO
from kapre_amd import _ffi, backend

PARAM_SETS = [dict(pm.DEFAULTS), dict(s=0.04, alpha=0.8, delta=10.0, r=0.25, eps=1e-6),
              dict(s=0.5, alpha=0.98, delta=2.0, r=0.5, eps=1e-6), dict(s=0.015, alpha=0.6, delta=1e-3, r=1.0, eps=1e-6)]


def _inputs(shape=(2, 37, 5), seed=0):
    rng = np.random.default_rng(seed)
    return [rng.random(shape), rng.random(shape) * 1e-4, np.exp(rng.normal(-6, 3, shape))]


# ------------------------------------------------------------------ the model
def test_smoother_is_lfilter_with_the_first_frame_as_state():
    from scipy.signal import lfilter

    for E in _inputs():
        for s in (0.025, 0.5, 1.0, 0.015):
            want = lfilter([s], [1, s - 1], E, axis=1, zi=(1 - s) * E[:, :1])[0]
            got = pm.smoother(E, s, axis=1)
            assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))


def test_model_per_band_vectors_equal_scalar_runs_per_band():
    E = _inputs((2, 20, 3, 2))[0]
    vec = dict(s=[0.02, 0.5, 0.1], alpha=[0.98, 0.5, 0.0], delta=[2.0, 1e-3, 10.0], r=[0.5, 1.0, 0.25])
    y = pm.pcen(E, axis=1, eps=1e-6, **{k: pm.band_params(v, "channels_last") for k, v in vec.items()})
    for m in range(3):
        one = pm.pcen(E[:, :, m], axis=1, eps=1e-6, **{k: v[m] for k, v in vec.items()})
        np.testing.assert_allclose(y[:, :, m], one, rtol=1e-13, atol=1e-15)    # (numpy's scalar and array powers differ by an ulp)


@pytest.mark.parametrize("p", PARAM_SETS)
def test_model_gradient_against_central_differences(p):
    E = _inputs((1, 9, 2), seed=3)[0] + 0.05
    gy = np.random.default_rng(4).normal(size=E.shape)
    got = pm.pcen_grad(E, gy, axis=1, **p)
    want = np.empty_like(E)
    h = 1e-6
    for idx in np.ndindex(E.shape):
        up, dn = E.copy(), E.copy()
        up[idx] += h
        dn[idx] -= h
        want[idx] = np.sum(gy * (pm.pcen(up, axis=1, **p) - pm.pcen(dn, axis=1, **p))) / (2 * h)
    assert np.max(np.abs(got - want)) <= 1e-6 * np.max(np.abs(want))


@pytest.mark.parametrize("p", PARAM_SETS)
def test_model_gradient_against_torch_autograd(p):
    import torch

    E = _inputs((2, 13, 3), seed=5)[2]
    gy = np.random.default_rng(6).normal(size=E.shape)
    x = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    S, rows = x[:, 0], []
    for t in range(E.shape[1]):
        if t:
            S = (1 - p["s"]) * S + p["s"] * x[:, t]
        rows.append((x[:, t] * (p["eps"] + S) ** (-p["alpha"]) + p["delta"]) ** p["r"] - p["delta"] ** p["r"])
    y = torch.stack(rows, dim=1)
    np.testing.assert_allclose(y.detach().numpy(), pm.pcen(E, axis=1, **p), rtol=1e-13, atol=1e-15)
    y.backward(torch.tensor(gy))
    want = x.grad.numpy()
    assert np.max(np.abs(pm.pcen_grad(E, gy, axis=1, **p) - want)) <= 1e-12 * np.max(np.abs(want))


def test_float32_model_stays_near_the_oracle_and_the_bound_covers_it():
    for E in _inputs((2, 64, 8), seed=7):
        for p in PARAM_SETS:
            y64 = pm.pcen(E.astype(np.float32), axis=1, **p)
            y32 = pm.pcen(E.astype(np.float32), axis=1, dtype=np.float32, **p)
            err = np.max(np.abs(y32 - y64)) / np.max(np.abs(y64))
            assert err <= pm.first_order_bound(E.astype(np.float32), axis=1, **p) <= 1e-4


# ------------------------------------------------------------------ layer and backend, host side
def test_exports():
    assert "PCEN" in kapre.__all__ and "PCEN" in kapre.time_frequency.__all__
    assert kapre.PCEN is kapre.time_frequency.PCEN and callable(backend.pcen)


def test_config_round_trip_and_serialisation():
    layer = kapre.PCEN(smooth_coef=0.04, alpha=[0.9, 0.8], delta=np.array([2.0, 3.0], dtype=np.float32), r=0.25, eps=1e-5,
                       data_format="channels_first", name="pcen_x")
    cfg = layer.get_config()
    assert cfg["smooth_coef"] == 0.04 and cfg["alpha"] == [0.9, 0.8] and cfg["delta"] == [2.0, 3.0] and cfg["r"] == 0.25
    assert cfg["eps"] == 1e-5 and cfg["data_format"] == "channels_first" and cfg["name"] == "pcen_x"
    again = kapre.PCEN.from_config(json.loads(json.dumps(cfg)))
    assert again.get_config() == cfg
    assert layer.compute_output_shape((None, 2, 83, 2)) == (None, 2, 83, 2)
    d = kapre.PCEN().get_config()
    assert (d["smooth_coef"], d["alpha"], d["delta"], d["r"], d["eps"], d["data_format"]) == (0.025, 0.98, 2.0, 0.5, 1e-6, "default")
    from kapre_amd import keras_shim
    model = keras_shim.Sequential([kapre.PCEN(alpha=0.5)])
    assert keras_shim.Sequential.from_config(model.get_config()).layers[-1].get_config()["alpha"] == 0.5


@pytest.mark.parametrize("kw", [dict(smooth_coef=0.0), dict(smooth_coef=1.5), dict(smooth_coef=-0.1), dict(alpha=-0.1),
                                dict(delta=0.0), dict(r=0.0), dict(r=-1.0), dict(eps=0.0), dict(eps=-1e-6),
                                dict(smooth_coef=[0.1, 0.0]), dict(alpha=float("nan")), dict(delta=[[2.0]]),
                                dict(data_format="weird")])
def test_validation_errors(kw):
    with pytest.raises(ValueError):
        kapre.PCEN(**kw)
    if "data_format" not in kw:
        kw = {("s" if k == "smooth_coef" else k): v for k, v in kw.items()}
        with pytest.raises(ValueError):
            backend.pcen_parameters(**{**pm.DEFAULTS, **kw})


def test_boundary_values_are_accepted():
    kapre.PCEN(smooth_coef=1.0, alpha=0.0, delta=1e-30, r=4.0, eps=1e-30)


def test_band_table_checks_vector_lengths():
    params = backend.pcen_parameters([0.1, 0.2, 0.3], 0.98, 2.0, 0.5, 1e-6)[:4]
    table = backend.pcen_band_table(params, 3)
    assert table.dtype == np.float32 and table.shape == (4, 3)
    np.testing.assert_array_equal(table, np.float32([[0.1, 0.2, 0.3], [0.98] * 3, [2.0] * 3, [0.5] * 3]))
    with pytest.raises(ValueError, match="3 values"):
        backend.pcen_band_table(params, 4)


def test_float64_is_refused_before_the_device():
    with pytest.raises(NotImplementedError):
        kapre.PCEN(dtype="float64")(np.zeros((1, 4, 3, 1), dtype=np.float32))
    with pytest.raises(NotImplementedError):
        kapre.PCEN()(np.zeros((1, 4, 3, 1), dtype=np.float64))
    with pytest.raises(ValueError, match="rank-4"):
        kapre.PCEN()(np.zeros((4, 3, 1), dtype=np.float32))


# ------------------------------------------------------------------ C ABI
def test_header_prototypes_and_exports():
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("kpr_pcen_plan", "kpr_pcen_f32", "kpr_pcen_bwd_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
    assert re.search(r"#define\s+KPR_VERSION\s+120\b", text) and _ffi.lib().kpr_version() == 120
    assert "float* smooth_out" in code


def test_plan_and_host_only_argument_checks():
    L = _ffi.lib()
    rows, waves = _ffi.pcen_plan(83, 128)
    assert rows >= 1 and 1 <= waves <= 16
    assert _ffi.pcen_plan(1, 1) == (rows, waves) and _ffi.pcen_plan(1 << 20, 4096) == (rows, waves)
    r_, w_ = ctypes.c_int(0), ctypes.c_int(0)
    assert L.kpr_pcen_plan(-1, 4, ctypes.byref(r_), ctypes.byref(w_)) == -1
    assert L.kpr_pcen_plan(8, 4, None, ctypes.byref(w_)) == -1

    fake = ctypes.c_void_p(0x1000)               # never dereferenced: every call below returns before a launch
    null = ctypes.c_void_p(0)

    def fwd(x=fake, outer=2, frames=5, inner=6, band_div=2, n_bands=3, par=fake, eps=1e-6, out=ctypes.c_void_p(0x100000)):
        return L.kpr_pcen_f32(x, outer, frames, inner, band_div, n_bands, par, par, par, par, eps, out, null, null)

    def bwd(x=fake, smooth=ctypes.c_void_p(0x200000), gy=ctypes.c_void_p(0x300000), frames=5, inner=6, n_bands=3,
            gx=ctypes.c_void_p(0x100000)):
        return L.kpr_pcen_bwd_f32(x, smooth, gy, 2, frames, inner, 2, n_bands, fake, fake, fake, fake, 1e-6, gx, null)

    for zero in (dict(outer=0), dict(frames=0), dict(inner=0)):
        assert fwd(**zero) == 0 and fwd(x=null, out=null, **zero) == 0
    assert bwd(frames=0) == 0
    for bad in (dict(x=null), dict(out=null), dict(par=null), dict(outer=-1), dict(frames=-1), dict(band_div=0), dict(n_bands=0),
                dict(inner=7), dict(out=fake), dict(eps=0.0), dict(x=ctypes.c_void_p(0x1002))):
        assert fwd(**bad) == -1, bad
    assert b"n_bands" in (fwd(inner=7), L.kpr_last_error())[1]
    for bad in (dict(smooth=null), dict(gy=null), dict(gx=null), dict(gx=fake), dict(inner=8)):
        assert bwd(**bad) == -1, bad
    # frames * inner reaches 2^31: refused, one element below is not (it would launch: not called here)
    assert fwd(frames=1 << 20, inner=1 << 11, band_div=1, n_bands=1 << 11) == -2 and b"2^31" in L.kpr_last_error()
    assert bwd(frames=1 << 21, inner=1 << 10, n_bands=1 << 9) == -2


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='PCEN expects a rank-4 input'):
        kapre.PCEN()(np.zeros((4, 3, 1), np.float32))
    with pytest.raises(NotImplementedError, match='PCEN has float32 kernels only; got a float64 input'):
        kapre.PCEN()(np.zeros((1, 4, 3, 1), np.float64))
    with pytest.raises(ValueError, match='PCEN expects a rank-4 input'):
        kapre.PCEN()(np.zeros((4, 3, 1), np.float64))
    with pytest.raises(ValueError, match='PCEN expects a rank-4 input'):
        backend.pcen(np.zeros((4, 3, 1), np.float32))
    with pytest.raises(NotImplementedError, match='PCEN has float32 kernels only; got a float64 input'):
        backend.pcen(np.zeros((1, 4, 3, 1), np.float64))
    with pytest.raises(ValueError, match='PCEN expects a rank-4 input'):
        backend.pcen(np.zeros((4, 3, 1), np.float64))
