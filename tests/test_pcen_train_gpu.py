"""Trainable PCEN on the GPU: kpr_pcen_bwd_params_f32 (``_ffi.pcen_bwd_params``), ``backend.pcen`` with tensor parameters and
``PCEN(trainable_params=...)`` against the float64 numpy model of tests/pcen_train_model.py (``pcen_param_grad``).

Limit.  Per parameter, err = max_b |g_dev[b] - g_64[b]| / max_b |g_64[b]| must not exceed min(max(Y1, Y2), 1e-4):
  Y1 = 8 x the same figure of the float32 numpy model (the factor DESIGN 4.11 uses for gradients);
  Y2 = pcen_train_model.param_grad_bound: a first-order bound on the per-term error of the powers and logarithms plus the rounding
       of the summation (float32 along a lane's frames and the workgroup's waves, float64 behind that), evaluated on the float64
       model's intermediates only (the derivation is that function's docstring).
Neither is a device result.  A parameter whose float64 gradient is exactly zero everywhere must come out exactly zero.
Every check prints its figures.  R and W are what kpr_pcen_plan reports."""
import numpy as np
import pytest

import pcen_model as pm
import pcen_train_model as ptm
from conftest import speech

pytestmark = pytest.mark.gpu

NAMES = ("s", "alpha", "delta", "r")
PARAM_SETS = {"defaults": dict(pm.DEFAULTS), "wide": dict(s=0.04, alpha=0.8, delta=10.0, r=0.25, eps=1e-6),
              "fast": dict(s=0.5, alpha=0.98, delta=2.0, r=0.5, eps=1e-6),
              "linear": dict(s=0.015, alpha=0.6, delta=1e-3, r=1.0, eps=1e-6), "s=1": dict(s=1.0, alpha=0.98, delta=2.0, r=0.5, eps=1e-6)}
FAMILIES = ("uniform", "uniform 1e-4", "lognormal")
FRAMES = {"1": lambda R, W: 1, "2": lambda R, W: 2, "R": lambda R, W: R, "R+1": lambda R, W: R + 1, "WR-1": lambda R, W: W * R - 1,
          "WR": lambda R, W: W * R, "WR+1": lambda R, W: W * R + 1, "2WR+2": lambda R, W: 2 * W * R + 2}
# (format, shape with F for the frames, the instance's V)
COLUMNS = {"cf 3x1xFx5 V1, a wave spanning items": ("channels_first", (3, 1, "F", 5), 1),
           "cf 2x3xFx8 V4, channels as outer items": ("channels_first", (2, 3, "F", 8), 4),
           "cf 70x1xFx8 V4, three workgroups": ("channels_first", (70, 1, "F", 8), 4),
           "cl 5xFx3x2 V1, band_div 2": ("channels_last", (5, "F", 3, 2), 1),
           "cl 5xFx4x3 V4, bands straddle a group": ("channels_last", (5, "F", 4, 3), 4)}


def plan():
    from kapre_amd import _ffi
    return _ffi.pcen_plan(83, 128)


def inputs(kind, shape, seed=0):
    rng = np.random.default_rng(seed)
    x = {"uniform": lambda: rng.random(shape), "uniform 1e-4": lambda: rng.random(shape) * 1e-4,
         "lognormal": lambda: np.exp(rng.normal(-6, 3, shape))}[kind]()
    return x.astype(np.float32), rng.normal(size=shape).astype(np.float32)


def spread(p, m):
    """the set as float32 per-band vectors with a +-10 % spread (s capped at 1)"""
    k = np.linspace(-0.1, 0.1, m) if m > 1 else np.zeros(1)
    out = {n: (p[n] * (1 + k * (1 if i % 2 else -1))).astype(np.float32) for i, n in enumerate(NAMES)}
    out["s"] = np.minimum(out["s"], np.float32(1.0))
    return out


def n_bands_of(shape, fmt):
    return shape[2] if fmt == "channels_last" else shape[3]


def model_kwargs(vec, eps, fmt):
    kw = {n: pm.band_params(np.asarray(vec[n], dtype=np.float32).astype(np.float64), fmt) for n in NAMES}
    kw.update(eps=float(np.float32(eps)), axis=pm.time_axis(fmt), band_axis=2 if fmt == "channels_last" else 3)
    return kw


def device_run(x, gy, vec, eps, fmt, want_gx=True):
    """forward keeping S, then the new backward, on device tensors (x may be a tensor: a view)"""
    import torch
    from kapre_amd import _ffi
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).cuda()
    params = tuple(torch.from_numpy(np.ascontiguousarray(vec[n], dtype=np.float32)).cuda() for n in NAMES)
    _, smooth = _ffi.pcen(xt, fmt, params, eps, want_smooth=True)
    gx, gp = _ffi.pcen_bwd_params(xt, smooth, torch.from_numpy(gy).cuda(), fmt, params, eps, want_gx=want_gx)
    return gx, gp, _ffi.last_launches(), (xt, smooth, params)


def check_limit(gp, x, gy, vec, eps, fmt, label, sum_bands=False):
    """gp: (4, n_bands) device result as numpy (or (4,) band sums with ``sum_bands``)"""
    R, W = plan()
    kw = model_kwargs(vec, eps, fmt)
    g64 = ptm.pcen_param_grad(x, gy, **kw)
    g32 = ptm.pcen_param_grad(x, gy, dtype=np.float32, **kw)
    bound = ptm.param_grad_bound(x, gy, rows=R, waves=W, **kw)
    if sum_bands:                                     # a scalar parameter: the band sums; the bound's numerator adds up
        scale = np.max(np.abs(g64), axis=1)
        bound = [b * s * g64.shape[1] / max(abs(t), 1e-300) for b, s, t in zip(bound, scale, g64.sum(axis=1))]
        g64, g32 = g64.sum(axis=1, keepdims=True), g32.sum(axis=1, keepdims=True)
        gp = gp.reshape(4, 1)
    assert gp.shape == g64.shape and gp.dtype == np.float32, (gp.shape, g64.shape)
    for i, n in enumerate(NAMES):
        scale = np.max(np.abs(g64[i]))
        if scale == 0:
            print("pcen g_%s %s: the model's gradient is exactly zero" % (n, label))
            assert not gp[i].any(), (label, n, gp[i])
            continue
        err = np.max(np.abs(gp[i] - g64[i])) / scale
        y1 = 8 * np.max(np.abs(g32[i] - g64[i])) / scale
        limit = min(max(y1, bound[i]), 1e-4)
        print("pcen g_%s %s: device %.3e | 8 x float32 model %.3e | first-order bound %.3e | limit %.3e" % (n, label, err, y1, bound[i], limit))
        assert err <= limit, (label, n, err, limit)


# ------------------------------------------------------------------ the launcher against the model
@pytest.mark.parametrize("cname", list(COLUMNS))
@pytest.mark.parametrize("fname", list(FRAMES))
def test_parameter_gradients_at_the_tile_boundaries(fname, cname):
    import kapre_amd as kapre
    from kapre_amd import _ffi
    fmt, shape, V = COLUMNS[cname]
    f = FRAMES[fname](*plan())
    shape = tuple(f if d == "F" else d for d in shape)
    k = list(FRAMES).index(fname) + list(COLUMNS).index(cname)
    kind, pname = FAMILIES[k % 3], list(PARAM_SETS)[k % 5]
    x, gy = inputs(kind, shape, seed=k)
    vec, eps = spread(PARAM_SETS[pname], n_bands_of(shape, fmt)), PARAM_SETS[pname]["eps"]
    gx, gp, launches, (xt, smooth, params) = device_run(x, gy, vec, eps, fmt)
    assert launches == "k_pcen_bwd_params<%d> + k_pcen_param_reduce" % V
    label = "%s F=%s(%d) %s / %s" % (cname, fname, f, kind, pname)
    check_limit(gp.cpu().numpy(), x, gy, vec, eps, fmt, label)
    # the input gradient is the input-only launch's, bit for bit; without it the parameter gradients keep their bits
    import torch
    old = _ffi.pcen_bwd(xt, smooth, torch.from_numpy(gy).cuda(), fmt, params, eps)
    assert gx.cpu().numpy().tobytes() == old.cpu().numpy().tobytes(), label
    none, gp2, launches, _ = device_run(x, gy, vec, eps, fmt, want_gx=False)
    assert none is None and launches == "k_pcen_bwd_params_only<%d> + k_pcen_param_reduce" % V
    assert gp2.cpu().numpy().tobytes() == gp.cpu().numpy().tobytes(), label
    if f == 1:
        assert gp[0].cpu().numpy().tobytes() == np.zeros(n_bands_of(shape, fmt), np.float32).tobytes()    # g_s: +0.0
    kapre.check_device()


@pytest.mark.parametrize("pname", list(PARAM_SETS))
@pytest.mark.parametrize("kind", FAMILIES)
def test_parameter_gradients_over_inputs_and_parameters(kind, pname):
    import kapre_amd as kapre
    R, W = plan()
    for fmt, shape in (("channels_first", (2, 3, 2 * W * R + 2, 8)), ("channels_last", (5, W * R + 1, 4, 3))):
        x, gy = inputs(kind, shape, seed=11)
        vec, eps = spread(PARAM_SETS[pname], n_bands_of(shape, fmt)), PARAM_SETS[pname]["eps"]
        gx, gp, _, _ = device_run(x, gy, vec, eps, fmt)
        check_limit(gp.cpu().numpy(), x, gy, vec, eps, fmt, "%s %s / %s" % (fmt, kind, pname))
    kapre.check_device()


def test_a_view_off_by_one_float_takes_the_scalar_form():
    import torch
    import kapre_amd as kapre
    R, W = plan()
    shape = (2, 3, W * R + 1, 8)
    x, gy = inputs("uniform", shape, seed=2)
    buf = torch.zeros(x.size + 1, device="cuda")
    view = buf[1:].view(shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    vec, eps = spread(PARAM_SETS["defaults"], 8), 1e-6
    gx, gp, launches, _ = device_run(view, gy, vec, eps, "channels_first")
    assert launches == "k_pcen_bwd_params<1> + k_pcen_param_reduce"
    check_limit(gp.cpu().numpy(), x, gy, vec, eps, "channels_first", "view one float off")
    _, gp4, launches, _ = device_run(x, gy, vec, eps, "channels_first")
    assert launches == "k_pcen_bwd_params<4> + k_pcen_param_reduce"
    check_limit(gp4.cpu().numpy(), x, gy, vec, eps, "channels_first", "the same block, aligned")
    kapre.check_device()


# ------------------------------------------------------------------ behaviour
def test_same_inputs_same_bits_and_empty_shapes():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    R, W = plan()
    x, gy = inputs("lognormal", (70, 1, 2 * W * R + 2, 8), seed=4)
    vec = spread(PARAM_SETS["wide"], 8)
    runs = [device_run(x, gy, vec, 1e-6, "channels_first")[1].cpu().numpy().tobytes() for _ in range(2)]
    assert runs[0] == runs[1]
    empty = torch.zeros((2, 3, 0, 8), device="cuda")
    params = tuple(torch.from_numpy(vec[n]).cuda() for n in NAMES)
    gx, gp = _ffi.pcen_bwd_params(empty, empty, empty, "channels_first", params, 1e-6)
    assert tuple(gx.shape) == (2, 3, 0, 8) and _ffi.last_launches() == ""
    assert gp.cpu().numpy().tobytes() == np.zeros((4, 8), np.float32).tobytes()
    kapre.check_device()


def test_zero_input_gives_exact_zeros_for_alpha_and_s():
    import kapre_amd as kapre
    R, W = plan()
    for fmt, shape in (("channels_first", (2, 3, W * R + 1, 8)), ("channels_last", (5, R + 1, 3, 2))):
        gy = inputs("uniform", shape, seed=5)[1]
        for pname, p in PARAM_SETS.items():
            gp = device_run(np.zeros(shape, np.float32), gy, spread(p, n_bands_of(shape, fmt)), p["eps"], fmt)[1].cpu().numpy()
            assert not gp[0].any() and not gp[1].any(), (fmt, pname, gp[:2])
            assert not gp[2].any() and not gp[3].any(), (fmt, pname, gp[2:])       # u = delta bit for bit: these vanish too
    kapre.check_device()


def test_a_nan_stays_in_its_band():
    import kapre_amd as kapre
    R, W = plan()
    f = 2 * W * R + 2
    for fmt, shape, at, band in (("channels_first", (2, 3, f, 8), (1, 2, R + 2, 5), 5), ("channels_last", (5, f, 4, 3), (3, R + 2, 1, 2), 1)):
        x, gy = inputs("uniform", shape, seed=6)
        vec = spread(PARAM_SETS["defaults"], n_bands_of(shape, fmt))
        clean = device_run(x, gy, vec, 1e-6, fmt)[1].cpu().numpy()
        bad = x.copy()
        bad[at] = np.nan
        for want_gx in (True, False):
            got = device_run(bad, gy, vec, 1e-6, fmt, want_gx=want_gx)[1].cpu().numpy()
            assert np.isnan(got[:, band]).all(), (fmt, got[:, band])
            others = np.arange(got.shape[1]) != band
            assert np.isfinite(clean).all() and got[:, others].tobytes() == clean[:, others].tobytes()
    kapre.check_device()                                             # a NaN is data, not a fault


# ------------------------------------------------------------------ through autograd
def _record_backward_launches(monkeypatch):
    """the backward pass runs on autograd's thread and kpr_last_launches is per thread: note it where the launcher returns"""
    from kapre_amd import _ffi
    seen = []
    for name in ("pcen_bwd", "pcen_bwd_params"):
        def wrapped(*a, _inner=getattr(_ffi, name), **kw):
            out = _inner(*a, **kw)
            seen.append(_ffi.last_launches())
            return out
        monkeypatch.setattr(_ffi, name, wrapped)
    return seen


def test_backend_pcen_with_tensor_parameters(monkeypatch):
    import torch
    import kapre_amd as kapre
    seen = _record_backward_launches(monkeypatch)
    R, W = plan()
    fmt, shape = "channels_last", (5, W * R + 1, 4, 3)
    x, gy = inputs("uniform", shape, seed=7)
    vec, eps = spread(PARAM_SETS["wide"], 4), 1e-6
    for x_grad in (False, True):
        par = {n: torch.from_numpy(vec[n]).cuda().requires_grad_(True) for n in NAMES}
        xt = torch.from_numpy(x).cuda().requires_grad_(x_grad)
        y = kapre.backend.pcen(xt, **par, eps=eps, data_format=fmt)
        assert y.grad_fn is not None
        y.backward(torch.from_numpy(gy).cuda())
        assert seen[-1] == "k_pcen_bwd_params%s<4> + k_pcen_param_reduce" % ("" if x_grad else "_only")
        gp = np.stack([par[n].grad.cpu().numpy() for n in NAMES])
        check_limit(gp, x, gy, vec, eps, fmt, "backend.pcen, x.requires_grad = %s" % x_grad)
        if x_grad:
            kw = model_kwargs(vec, eps, fmt)
            kw.pop("band_axis")
            g64 = pm.pcen_grad(x, gy, **kw)
            err = np.max(np.abs(xt.grad.cpu().numpy() - g64)) / np.max(np.abs(g64))
            limit = min(8 * np.max(np.abs(pm.pcen_grad(x, gy, dtype=np.float32, **kw) - g64)) / np.max(np.abs(g64)), 1e-4)
            print("x.grad next to the parameter gradients: device %.3e | limit %.3e" % (err, limit))
            assert err <= limit
        else:
            assert xt.grad is None
    # only alpha learned, as a 0-d tensor: the band-summed gradient, shape (); the others are numbers and a constant tensor
    alpha0 = torch.tensor(0.8, device="cuda", requires_grad=True)
    delta_t = torch.from_numpy(vec["delta"]).cuda()
    y = kapre.backend.pcen(x, s=0.04, alpha=alpha0, delta=delta_t, r=0.25, eps=eps, data_format=fmt)
    y.backward(torch.from_numpy(gy).cuda())
    assert tuple(alpha0.grad.shape) == () and delta_t.grad is None
    flat = dict(s=np.float32([0.04] * 4), alpha=np.float32([0.8] * 4), delta=vec["delta"], r=np.float32([0.25] * 4))
    g64 = ptm.pcen_param_grad(x, gy, **model_kwargs(flat, eps, fmt))[1].sum()
    g32 = ptm.pcen_param_grad(x, gy, dtype=np.float32, **model_kwargs(flat, eps, fmt))[1].sum(dtype=np.float32)
    R_, W_ = plan()
    kw = model_kwargs(flat, eps, fmt)
    per_band = ptm.param_grad_bound(x, gy, rows=R_, waves=W_, **kw)[1] * np.max(np.abs(ptm.pcen_param_grad(x, gy, **kw)[1]))
    limit = min(max(8 * abs(float(g32) - g64), 4 * per_band + 4 * 2.0 ** -24 * abs(g64)) / abs(g64), 1e-4)
    err = abs(float(alpha0.grad) - g64) / abs(g64)
    print("0-d alpha: device %.3e | limit %.3e" % (err, limit))
    assert err <= limit
    with pytest.raises(ValueError, match="shape"):
        kapre.backend.pcen(x, alpha=torch.ones(3, device="cuda"), data_format=fmt)
    with pytest.raises(ValueError, match="float32"):
        kapre.backend.pcen(x, alpha=torch.ones(4, device="cuda", dtype=torch.float64), data_format=fmt)
    with pytest.raises(ValueError, match="is on"):
        kapre.backend.pcen(x, alpha=torch.ones(4), data_format=fmt)
    kapre.check_device()


def test_all_scalar_parameters(monkeypatch):
    import torch
    import kapre_amd as kapre
    R, W = plan()
    fmt, shape = "channels_first", (2, 3, W * R + 1, 8)
    x, gy = inputs("lognormal", shape, seed=8)
    p = PARAM_SETS["defaults"]
    par = {n: torch.tensor(p[n], device="cuda", requires_grad=True) for n in NAMES}
    y = kapre.backend.pcen(x, **par, eps=p["eps"], data_format=fmt)
    y.backward(torch.from_numpy(gy).cuda())
    gp = np.float32([float(par[n].grad) for n in NAMES])
    assert all(tuple(par[n].grad.shape) == () for n in NAMES)
    flat = {n: np.full(8, p[n], np.float32) for n in NAMES}
    check_limit(gp, x, gy, flat, p["eps"], fmt, "all scalars", sum_bands=True)
    kapre.check_device()


def test_trainable_layer_behind_the_mel_chain(monkeypatch):
    import torch
    import kapre_amd as kapre
    seen = _record_backward_launches(monkeypatch)
    fmt = "channels_last"
    wave = np.stack([speech(8000, 4000 * i) for i in range(4)])[:, :, None]
    mel = kapre.composed.get_melspectrogram_layer(input_shape=wave.shape[1:], n_fft=512, hop_length=128, sample_rate=16000,
                                                  n_mels=40, return_decibel=False, input_data_format=fmt, output_data_format=fmt)
    layer = kapre.PCEN(trainable_params=True, data_format=fmt)
    model = kapre.Sequential([mel, layer])
    y = model(wave)                                                  # a plain batch: no gradient into the front end
    assert y.grad_fn is not None and model.count_params() == 160
    ps = model.parameters()
    assert len(ps) == 4 and all(p.is_cuda and p.grad is None for p in ps) and all(a is b for a, b in zip(ps, layer.parameters()))
    e = mel(wave).cpu().numpy()
    gy = np.random.default_rng(9).normal(size=e.shape).astype(np.float32)
    y.backward(torch.from_numpy(gy).cuda())
    assert seen == ["k_pcen_bwd_params_only<4> + k_pcen_param_reduce"]
    flat = {n: np.full(40, pm.DEFAULTS[n], np.float32) for n in NAMES}
    check_limit(np.stack([p.grad.cpu().numpy() for p in ps]), e, gy, flat, 1e-6, fmt, "Sequential([mel, PCEN(trainable)])")
    # one optimiser step and the clamp; the learned values travel through the config
    opt = torch.optim.SGD(ps, lr=1e-3)
    opt.step()
    layer.constrain_()
    again = kapre.Sequential.from_config(model.get_config())
    assert again(wave).detach().cpu().numpy().tobytes() == model(wave).detach().cpu().numpy().tobytes()
    assert again.layers[-1].get_config() == layer.get_config()
    # frozen by the Keras keyword: the parameters are used, nothing is recorded
    frozen = kapre.PCEN(trainable_params=True, trainable=False, data_format=fmt)
    assert frozen(e).grad_fn is None and not any(p.requires_grad for p in frozen.parameters())
    kapre.check_device()


def test_constant_parameters_keep_the_input_only_backward(monkeypatch):
    import torch
    import kapre_amd as kapre
    seen = _record_backward_launches(monkeypatch)
    x, gy = inputs("uniform", (2, 3, 20, 8), seed=10)
    for fmt in ("channels_first", "channels_last"):
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        y = kapre.PCEN(trainable_params=False, data_format=fmt)(xt)
        y.backward(torch.from_numpy(gy).cuda())
        assert seen[-1] == "k_pcen_bwd<4>"                           # the instance of the layer without learned parameters
        p = pm.DEFAULTS
        g64 = pm.pcen_grad(x, gy, axis=pm.time_axis(fmt), **p)
        assert np.max(np.abs(xt.grad.cpu().numpy() - g64)) <= 1e-4 * np.max(np.abs(g64))
    kapre.check_device()


def test_device_status_is_clean_at_the_end():
    import kapre_amd as kapre
    kapre.check_device()
