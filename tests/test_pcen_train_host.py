"""Trainable PCEN without a GPU: the numpy model of the parameter gradients (tests/pcen_train_model.py: pcen_param_grad) against
torch's float64 autograd of the sequential loop and against central differences, the C ABI's host-only side of
kpr_pcen_bwd_params_f32, and the layer's parameter plumbing on CPU tensors (no launch)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import kapre_amd as kapre
import pcen_model as pm
import pcen_train_model as ptm
from conftest import REPO
from kapre_amd import _ffi, keras_shim

PARAM_SETS = [dict(pm.DEFAULTS), dict(s=0.04, alpha=0.8, delta=10.0, r=0.25, eps=1e-6),
              dict(s=0.5, alpha=0.98, delta=2.0, r=0.5, eps=1e-6), dict(s=0.015, alpha=0.6, delta=1e-3, r=1.0, eps=1e-6),
              dict(s=1.0, alpha=0.98, delta=2.0, r=0.5, eps=1e-6)]
NAMES = ("s", "alpha", "delta", "r")


def _inputs(shape, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.random(shape), rng.random(shape) * 1e-4, np.exp(rng.normal(-6, 3, shape))]


def _spread(p, m, clip=True):
    """the parameter set as per-band vectors with a +-10 % spread (s stays in (0, 1])"""
    k = np.linspace(-0.1, 0.1, m) if m > 1 else np.zeros(1)
    out = {n: p[n] * (1 + k * (1 if i % 2 else -1)) for i, n in enumerate(NAMES)}
    out["s"] = np.minimum(out["s"], 1.0)
    out["eps"] = p["eps"]
    return out


def _torch_loop_grads(E, gy, vec, eps):
    """float64 autograd of the sequential loop over (b, t, m): gradients of the per-band vectors"""
    import torch

    x = torch.tensor(E, dtype=torch.float64)
    par = {n: torch.tensor(np.asarray(vec[n], dtype=np.float64), requires_grad=True) for n in NAMES}
    S, rows = x[:, 0], []
    for t in range(E.shape[1]):
        if t:
            S = (1 - par["s"]) * S + par["s"] * x[:, t]
        rows.append((x[:, t] * (eps + S) ** (-par["alpha"]) + par["delta"]) ** par["r"] - par["delta"] ** par["r"])
    (torch.stack(rows, dim=1) * torch.tensor(gy)).sum().backward()
    return np.stack([par[n].grad.numpy() for n in NAMES])


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("p", PARAM_SETS)
def test_model_parameter_gradients_against_torch_autograd(p):
    for k, E in enumerate(_inputs((2, 13, 3), seed=5)):
        gy = np.random.default_rng(6).normal(size=E.shape)
        vec = _spread(p, 3)
        want = _torch_loop_grads(E, gy, vec, p["eps"])
        got = ptm.pcen_param_grad(E, gy, axis=1, band_axis=2, **{n: vec[n] for n in NAMES}, eps=p["eps"])
        assert got.shape == (4, 3)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print("model vs autograd, input family %d, s = %g: %.2e" % (k, p["s"], err))
        assert err <= 1e-11
        # scalars: the gradient of a scalar is the sum over the bands of the gradient of the equal vector
        flat = {n: np.full(3, float(p[n])) for n in NAMES}
        want = _torch_loop_grads(E, gy, flat, p["eps"]).sum(axis=1)
        got = ptm.pcen_param_grad(E, gy, axis=1, **p).sum(axis=(1, 2))
        assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want))


def test_model_parameter_gradients_against_central_differences():
    p = PARAM_SETS[1]
    E = _inputs((1, 9, 2), seed=3)[0] + 0.05
    gy = np.random.default_rng(4).normal(size=E.shape)
    got = ptm.pcen_param_grad(E, gy, axis=1, **p).sum(axis=(1, 2))
    for i, n in enumerate(NAMES):
        h = 1e-6 * p[n]
        up, dn = dict(p), dict(p)
        up[n] += h
        dn[n] -= h
        want = np.sum(gy * (pm.pcen(E, axis=1, **up) - pm.pcen(E, axis=1, **dn))) / (2 * h)
        assert abs(got[i] - want) <= 1e-6 * abs(want), (n, got[i], want)


def test_model_edge_cases_and_the_bound_covers_the_float32_model():
    E = _inputs((3, 1, 5))[0]
    gy = np.ones_like(E)
    assert not ptm.pcen_param_grad(E, gy, axis=1, band_axis=2)[0].any()                   # one frame: S = E, nothing of s
    z = ptm.pcen_param_grad(np.zeros((2, 7, 3)), np.ones((2, 7, 3)), axis=1, band_axis=2)
    assert not z[0].any() and not z[1].any()
    for shape in ((3, 13, 5), (5, 130, 6)):
        for E in _inputs(shape, seed=7):
            E = E.astype(np.float32)
            gy = np.random.default_rng(8).normal(size=shape).astype(np.float32)
            for p in PARAM_SETS:
                vec = _spread(p, shape[2])
                kw = {n: np.float32(vec[n]).astype(np.float64) for n in NAMES}
                g64 = ptm.pcen_param_grad(E, gy, axis=1, band_axis=2, eps=p["eps"], **kw)
                g32 = ptm.pcen_param_grad(E, gy, axis=1, band_axis=2, eps=p["eps"], dtype=np.float32, **kw)
                bound = ptm.param_grad_bound(E, gy, eps=p["eps"], axis=1, band_axis=2, **kw)
                for i in range(4):
                    err = np.max(np.abs(g32[i] - g64[i])) / np.max(np.abs(g64[i]))
                    print(shape, p["s"], NAMES[i], "float32 model %.2e, bound %.2e" % (err, bound[i]))
                    assert err <= bound[i] and np.isfinite(bound[i]), (shape, p, NAMES[i], err, bound[i])


# ------------------------------------------------------------------ C ABI
def test_header_prototypes_exports_and_version():
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    assert re.search(r"\bsize_t\s+kpr_pcen_bwd_params_workspace_bytes\s*\(", code)
    assert re.search(r"\bint\s+kpr_pcen_bwd_params_f32\s*\(", code)
    for name in ("kpr_pcen_bwd_params_workspace_bytes", "kpr_pcen_bwd_params_f32"):
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
    assert re.search(r"#define\s+KPR_VERSION\s+120\b", text) and _ffi.lib().kpr_version() == 120
    assert callable(_ffi.pcen_bwd_params)


def test_workspace_bytes():
    ws = _ffi.lib().kpr_pcen_bwd_params_workspace_bytes
    assert ws(2, 5, 6) == 16 * 2 * 6 and ws(2048, 998, 80) == 16 * 2048 * 80 and ws(1, 1, 1) == 16
    assert ws(3, 5, 6) > ws(2, 5, 6) and ws(2, 5, 7) > ws(2, 5, 6) and ws(2, 9, 6) == ws(2, 5, 6)
    for empty in ((0, 5, 6), (2, 0, 6), (2, 5, 0), (-1, 5, 6)):
        assert ws(*empty) == 0


def test_host_only_argument_checks():
    L = _ffi.lib()
    fake, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)           # never dereferenced: every call returns before a launch
    need = 16 * 2 * 6

    def call(x=fake, smooth=ctypes.c_void_p(0x200000), gy=ctypes.c_void_p(0x300000), frames=5, inner=6, n_bands=3,
             gx=ctypes.c_void_p(0x100000), gparams=ctypes.c_void_p(0x400000), ws=ctypes.c_void_p(0x500000), ws_bytes=need - 4):
        return L.kpr_pcen_bwd_params_f32(x, smooth, gy, 2, frames, inner, 2, n_bands, fake, fake, fake, fake, 1e-6, gx, gparams,
                                         ws, ws_bytes, null)

    # a workspace one float short is what every accepted argument list below ends in: the last check before the launch
    assert call() == -4 and b"workspace" in L.kpr_last_error()
    assert call(ws=null, ws_bytes=need) == -4 and call(ws_bytes=0) == -4
    assert call(gx=null) == -4                                       # no input gradient wanted: accepted up to that point
    assert call(gparams=null) == -1 and call(gparams=null, frames=0) == -1
    for bad in (dict(x=null), dict(smooth=null), dict(gy=null), dict(gx=fake), dict(gx=ctypes.c_void_p(0x200000)), dict(inner=8),
                dict(n_bands=0), dict(frames=-1), dict(gparams=ctypes.c_void_p(0x400002)), dict(ws=ctypes.c_void_p(0x500002)),
                dict(gparams=ctypes.c_void_p(0x500010)), dict(ws=fake), dict(gparams=fake)):
        assert call(**bad) == -1, bad
    assert call(frames=1 << 21, inner=1 << 10, n_bands=1 << 9, ws_bytes=1 << 40) == -2 and b"2^31" in L.kpr_last_error()
    # the overlap predicate at its boundary: gparams is 16 * n_bands bytes.  A range that ends exactly where x begins touches x
    # and passes on to the workspace check; one that reaches 4 bytes into x is refused before it
    x = 0x600000
    assert call(x=ctypes.c_void_p(x), gparams=ctypes.c_void_p(x - 16 * 3)) == -4 and b"workspace" in L.kpr_last_error()
    assert call(x=ctypes.c_void_p(x), gparams=ctypes.c_void_p(x - 16 * 3 + 4)) == -1 and b"overlaps" in L.kpr_last_error()


# ------------------------------------------------------------------ the layer, on CPU tensors
def test_trainable_params_validation():
    for bad in ("alpha", ["beta"], ["alpha", "alpha"], 1, None, [1]):
        with pytest.raises(ValueError, match="trainable_params"):
            kapre.PCEN(trainable_params=bad)
    assert kapre.PCEN(trainable_params=["r", "alpha"]).trainable_params == ["alpha", "r"]
    assert kapre.PCEN(trainable_params=()).trainable_params == [] and kapre.PCEN().trainable_params is False
    with pytest.raises(ValueError, match="3 values"):
        kapre.PCEN(alpha=[0.9, 0.8, 0.7], trainable_params=True).build((None, 10, 4, 1))
    with pytest.raises(ValueError, match="bands"):
        kapre.PCEN(trainable_params=True).build((None, 10, None, 1))
    with pytest.raises(RuntimeError, match="build"):
        kapre.PCEN(trainable_params=True).parameters()


def test_default_layer_is_unchanged():
    layer = kapre.PCEN()
    assert sorted(layer.get_config()) == sorted(["name", "trainable", "dtype", "smooth_coef", "alpha", "delta", "r", "eps",
                                                 "data_format"])
    layer.build((None, 10, 4, 1))
    assert layer.parameters() == [] and layer.weights == [] and layer.count_params() == 0
    assert layer.constrain_() is layer
    assert kapre.STFT().parameters() == [] and keras_shim.Sequential([kapre.PCEN()]).parameters() == []


def test_parameters_weights_and_count():
    import torch

    layer = kapre.PCEN(smooth_coef=0.04, alpha=[0.9, 0.8, 0.7], trainable_params=True, data_format="channels_last")
    assert layer.weights == [] and layer.count_params() == 0
    layer.build((None, 10, 3, 2))
    ps = layer.parameters()
    assert len(ps) == 4 and all(isinstance(p, torch.nn.Parameter) and p.dtype == torch.float32 and tuple(p.shape) == (3,)
                                and p.requires_grad for p in ps)
    assert [p.tolist() for p in ps] == [np.float32([0.04] * 3).tolist(), np.float32([0.9, 0.8, 0.7]).tolist(), [2.0] * 3, [0.5] * 3]
    assert all(a is b for a, b in zip(layer.weights, ps)) and layer.count_params() == 12
    layer.build((None, 10, 3, 2))
    assert all(a is b for a, b in zip(layer.parameters(), ps))            # built once
    torch.optim.SGD(layer.parameters(), lr=0.1)
    first = kapre.PCEN(trainable_params=["delta"], data_format="channels_first", input_shape=(1, 10, 5))
    assert [tuple(p.shape) for p in first.parameters()] == [(5,)] and first.count_params() == 5
    frozen = kapre.PCEN(trainable_params=True, trainable=False)
    frozen.build((None, 10, 3, 2))
    assert len(frozen.parameters()) == 4 and not any(p.requires_grad for p in frozen.parameters())
    model = keras_shim.Sequential([kapre.Magnitude(), layer, keras_shim.Sequential([first])])
    assert [id(p) for p in model.parameters()] == [id(p) for p in ps + first.parameters()]
    assert [id(p) for p in model.weights] == [id(p) for p in model.parameters()] and model.count_params() == 17
    lines = []
    model.summary(print_fn=lines.append)
    assert lines[-1] == "Total params: 17"


def test_config_round_trip_with_learned_values():
    import torch

    layer = kapre.PCEN(alpha=0.9, delta=[2.0, 3.0], trainable_params=["alpha", "delta"], name="pcen_t")
    cfg = layer.get_config()
    assert cfg["alpha"] == 0.9 and cfg["delta"] == [2.0, 3.0] and cfg["trainable_params"] == ["alpha", "delta"]
    layer.build((None, 7, 2, 1))
    with torch.no_grad():
        layer.parameters()[0].copy_(torch.tensor([0.75, 0.5]))
        layer.parameters()[1].mul_(2)
    cfg = json.loads(json.dumps(layer.get_config()))
    assert cfg["alpha"] == [0.75, 0.5] and cfg["delta"] == [4.0, 6.0] and cfg["smooth_coef"] == 0.025 and cfg["r"] == 0.5
    again = kapre.PCEN.from_config(cfg)
    assert again.get_config() == cfg
    again.build((None, 7, 2, 1))
    assert [p.tolist() for p in again.parameters()] == [[0.75, 0.5], [4.0, 6.0]] and again.get_config() == cfg
    model = keras_shim.Sequential([layer])
    loaded = keras_shim.Sequential.from_config(json.loads(json.dumps(model.get_config())))
    assert loaded.layers[-1].get_config() == cfg
    every = kapre.PCEN(trainable_params=True)
    assert kapre.PCEN.from_config(every.get_config()).trainable_params is True


def test_constrain_clamps_into_the_domain():
    import torch

    layer = kapre.PCEN(trainable_params=True)
    layer.build((None, 7, 3, 1))
    tiny = float(np.finfo(np.float32).tiny)
    with torch.no_grad():
        for p, v in zip(layer.parameters(), ([-0.5, 0.5, 1.5], [-1.0, 0.0, 3.0], [-2.0, 0.0, 5.0], [0.0, -1e-3, 2.0])):
            p.copy_(torch.tensor(v))
    assert layer.constrain_() is layer
    s, alpha, delta, r = (p.tolist() for p in layer.parameters())
    assert s == [2.0 ** -10, 0.5, 1.0] and alpha == [0.0, 0.0, 3.0] and delta == [tiny, tiny, 5.0] and r == [tiny, tiny, 2.0]
    kapre.PCEN.from_config(layer.get_config())                         # the clamped values pass the constructor's validation
    part = kapre.PCEN(trainable_params=["r"])
    part.build((None, 7, 3, 1))
    with torch.no_grad():
        part.parameters()[0].fill_(-1.0)
    assert part.constrain_().parameters()[0].tolist() == [tiny] * 3
