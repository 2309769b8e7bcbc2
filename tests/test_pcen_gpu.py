"""PCEN on the GPU (kapre_amd.PCEN / backend.pcen, kpr_pcen_f32 / kpr_pcen_bwd_f32) against the float64 numpy model of
tests/pcen_model.py.

Parity rule.  err = conftest.rel_err(device, float64 model) must not exceed min(max(Y1, Y2), 1e-4):
  Y1 = 8 x rel_err(float32 numpy model, float64 model) on the same input -- how far float32 arithmetic by itself strays;
       the device's exp2 / log2 differ from numpy's powers, hence the factor;
  Y2 = pcen_model.first_order_bound: unit roundoff 2^-24 per arithmetic operation of the smoother (the error obeys
       e[t] <= a e[t-1] + 4 u S[t]), one unit in the last place (2^-23) for each hardware log2 and exp2, and the rounding of the
       exponent product scaled by |alpha log2(eps + S)| (about 20 for quiet bands), pushed through the formula to first order
       and evaluated on the float64 model's own intermediates (the derivation is that function's docstring).
Neither yardstick is a device result.  The float64 model takes the parameters as the float32 values the kernel receives.
Gradients are held to Y1 alone (8 x the float32 model's gradient error, at most 1e-4).  Every check prints its figures.

Shapes: R and W are what kpr_pcen_plan reports (rows per wave, waves per workgroup); the frame counts sit on both sides of a
wave's chunk (R) and of a workgroup's super-block (W R), the band counts cover the scalar and the 16-byte forms and a tail."""
import os

import numpy as np
import pytest

import pcen_model as pm
from conftest import rel_err, speech

pytestmark = pytest.mark.gpu

FRAMES = {"1": lambda R, W: 1, "2": lambda R, W: 2, "R-1": lambda R, W: R - 1, "R": lambda R, W: R, "R+1": lambda R, W: R + 1,
          "WR-1": lambda R, W: W * R - 1, "WR": lambda R, W: W * R, "WR+1": lambda R, W: W * R + 1,
          "2WR+3": lambda R, W: 2 * W * R + 3}
BANDS = (1, 3, 4, 5, 40, 128, 129)
LAYOUTS = [("channels_first", 1, 1), ("channels_first", 3, 1), ("channels_last", 2, 1), ("channels_last", 2, 2),
           ("channels_last", 1, 3)]                                  # (format, batch, channels): B C in {1, 3}, C in {1, 2, 3}
PARAM_SETS = {"defaults": dict(pm.DEFAULTS), "wide": dict(s=0.04, alpha=0.8, delta=10.0, r=0.25, eps=1e-6),
              "fast": dict(s=0.5, alpha=0.98, delta=2.0, r=0.5, eps=1e-6), "linear": dict(s=0.015, alpha=0.6, delta=1e-3, r=1.0, eps=1e-6)}


def band_vectors(m):
    k = np.arange(m, dtype=np.float64)
    return dict(s=0.015 + 0.4 * ((k * 7) % 5) / 5, alpha=0.5 + 0.48 * ((k * 3) % 4) / 3, delta=1e-3 + 2.0 * ((k * 5) % 3),
                r=0.25 + 0.25 * (k % 4), eps=1e-6)


def plan():
    from kapre_amd import _ffi
    rw = _ffi.pcen_plan(83, 128)
    for f in (1, 1000):
        for inner in (1, 129):
            assert _ffi.pcen_plan(f, inner) == rw        # one tiling for every shape: the frame counts below straddle it
    return rw


def shape_of(fmt, b, c, f, m):
    return (b, f, m, c) if fmt == "channels_last" else (b, c, f, m)


def model_kwargs(p, fmt):
    """the parameters as the kernel receives them (float32 values), shaped for pcen_model"""
    kw = {k: pm.band_params(np.asarray(p[k], dtype=np.float32).astype(np.float64), fmt) for k in ("s", "alpha", "delta", "r")}
    kw["eps"] = float(np.float32(p["eps"]))
    kw["axis"] = pm.time_axis(fmt)
    return kw


def layer_of(p, fmt):
    import kapre_amd as kapre
    return kapre.PCEN(smooth_coef=p["s"], alpha=p["alpha"], delta=p["delta"], r=p["r"], eps=p["eps"], data_format=fmt)


def check_parity(out, x, p, fmt, label):
    kw = model_kwargs(p, fmt)
    o64 = pm.pcen(x, **kw)
    err = rel_err(out, o64)
    y1 = 8 * rel_err(pm.pcen(x, dtype=np.float32, **kw), o64)
    y2 = pm.first_order_bound(x, **{k: kw[k] for k in ("s", "alpha", "delta", "r", "eps", "axis")})
    limit = min(max(y1, y2), 1e-4)
    print("pcen %s: device %.3e | 8 x float32 model %.3e | first-order bound %.3e | limit %.3e" % (label, err, y1, y2, limit))
    assert out.shape == x.shape and out.dtype == np.float32
    assert err <= limit, (label, err, limit)
    return err


def check_gradient(gx, x, gy, p, fmt, label):
    kw = model_kwargs(p, fmt)
    g64 = pm.pcen_grad(x, gy, **kw)
    err = rel_err(gx, g64)
    limit = min(8 * rel_err(pm.pcen_grad(x, gy, dtype=np.float32, **kw), g64), 1e-4)
    print("pcen gradient %s: device %.3e | limit (8 x float32 model) %.3e" % (label, err, limit))
    assert gx.shape == x.shape and err <= limit, (label, err, limit)


def inputs(kind, shape, axis, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x = rng.random(shape)
    elif kind == "uniform 1e-4":
        x = rng.random(shape) * 1e-4
    elif kind == "lognormal":
        x = np.exp(rng.normal(-6, 3, shape))
    elif kind == "live then silence":
        x = rng.random(shape)
        x[(slice(None),) * axis + (slice(300, None),)] = 0.0
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def speech_mel(fmt="channels_last"):
    """mel magnitudes of the speech fixture, computed by the library's own fused chain: (4, 59, 40, 1) or (4, 1, 59, 40)"""
    import kapre_amd as kapre
    wave = np.stack([speech(8000, 4000 * i) for i in range(4)])[:, :, None]
    if fmt == "channels_first":
        wave = np.ascontiguousarray(wave.transpose(0, 2, 1))
    mel = kapre.composed.get_melspectrogram_layer(input_shape=wave.shape[1:], n_fft=512, hop_length=128, sample_rate=16000,
                                                  n_mels=40, return_decibel=False, input_data_format=fmt, output_data_format=fmt)
    return wave, mel


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("fmt,batch,ch", LAYOUTS)
@pytest.mark.parametrize("fname", list(FRAMES))
def test_parity_at_the_tile_boundaries(fname, fmt, batch, ch):
    import kapre_amd as kapre
    from kapre_amd import _ffi
    f = FRAMES[fname](*plan())
    for i, m in enumerate(BANDS):
        x = inputs("uniform", shape_of(fmt, batch, ch, f, m), pm.time_axis(fmt), seed=m)
        p = band_vectors(m) if i % 2 else PARAM_SETS["defaults"]
        out = layer_of(p, fmt)(x)
        inner = m * ch if fmt == "channels_last" else m
        assert _ffi.last_launches() == "k_pcen<%d>" % (4 if inner % 4 == 0 else 1)
        check_parity(out.cpu().numpy(), x, p, fmt, "F=%s(%d) M=%d %s b=%d c=%d" % (fname, f, m, fmt, batch, ch))
    kapre.check_device()


@pytest.mark.parametrize("pname", list(PARAM_SETS) + ["per band"])
@pytest.mark.parametrize("kind", ["uniform", "uniform 1e-4", "lognormal", "live then silence", "speech mel"])
def test_parity_over_inputs_and_parameters(kind, pname):
    import kapre_amd as kapre
    fmt = "channels_last"
    if kind == "speech mel":
        wave, mel = speech_mel(fmt)
        x = mel(wave).cpu().numpy()
        assert x.shape[2] == 40 and x.min() >= 0
    else:
        x = inputs(kind, (2, 331, 40, 2), 1)
    p = band_vectors(40) if pname == "per band" else PARAM_SETS[pname]
    out = kapre.backend.pcen(x, **{k: p[k] for k in ("s", "alpha", "delta", "r", "eps")}, data_format=fmt)
    check_parity(out.cpu().numpy(), x, p, fmt, "%s / %s" % (kind, pname))
    kapre.check_device()


def test_a_base_pointer_off_by_one_float_takes_the_scalar_form():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    R, W = plan()
    shape = (3, W * R + 1, 40)
    x = inputs("uniform", (1,) + shape, 2)
    buf = torch.zeros(x.size + 1, device="cuda")
    view = buf[1:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    p = PARAM_SETS["defaults"]
    out = layer_of(p, "channels_first")(view)
    assert _ffi.last_launches() == "k_pcen<1>"
    check_parity(out.cpu().numpy(), x, p, "channels_first", "view one float off")
    aligned = layer_of(p, "channels_first")(x)
    assert _ffi.last_launches() == "k_pcen<4>"
    check_parity(aligned.cpu().numpy(), x, p, "channels_first", "the same block, aligned")
    kapre.check_device()


def test_non_contiguous_input_and_no_frames():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    x = inputs("uniform", (2, 40, 19, 3), 1)                     # stored (b, mel, t, ch): the layer sees a transposed view
    xt = torch.from_numpy(x).cuda().transpose(1, 2)
    assert not xt.is_contiguous()
    p = PARAM_SETS["wide"]
    out = layer_of(p, "channels_last")(xt)
    check_parity(out.cpu().numpy(), np.ascontiguousarray(x.transpose(0, 2, 1, 3)), p, "channels_last", "transposed view")
    empty = layer_of(p, "channels_last")(np.zeros((2, 0, 40, 3), np.float32))
    assert tuple(empty.shape) == (2, 0, 40, 3) and empty.dtype == torch.float32 and _ffi.last_launches() == ""
    with pytest.raises(ValueError, match="bands"):
        layer_of(band_vectors(39), "channels_last")(xt)
    kapre.check_device()


def test_zeros_give_exact_zeros():
    import kapre_amd as kapre
    R, W = plan()
    for fmt in ("channels_last", "channels_first"):
        for pname, p in list(PARAM_SETS.items()) + [("per band", band_vectors(5))]:
            out = layer_of(p, fmt)(np.zeros(shape_of(fmt, 2, 3, 2 * W * R + 3, 5), np.float32)).cpu().numpy()
            assert out.tobytes() == np.zeros_like(out).tobytes(), (fmt, pname)            # +0.0, bit for bit
    kapre.check_device()


def test_a_nan_stays_in_its_column():
    import kapre_amd as kapre
    R, W = plan()
    f, t0 = 2 * W * R + 3, R + 2
    for fmt, col in (("channels_first", (0, 2, slice(None), 17)), ("channels_last", (1, slice(None), 17, 2))):
        x = inputs("uniform", shape_of(fmt, 2, 3, f, 40), pm.time_axis(fmt), seed=3)
        layer = layer_of(PARAM_SETS["defaults"], fmt)
        clean = layer(x).cpu().numpy()
        bad = x.copy()
        series = bad[col]
        series[t0] = np.nan
        bad[col] = series
        got = layer(bad).cpu().numpy()
        assert not np.isfinite(got[col][t0:]).any()
        assert got[col][:t0].tobytes() == clean[col][:t0].tobytes()
        mask = np.ones(x.shape, bool)
        mask[col] = False
        assert np.isfinite(got[mask]).all() and got[mask].tobytes() == clean[mask].tobytes()
    kapre.check_device()                                             # a NaN is data, not a fault


# ------------------------------------------------------------------ gradient
@pytest.mark.parametrize("fmt,batch,ch", [("channels_first", 1, 3), ("channels_last", 2, 2)])
@pytest.mark.parametrize("fname", list(FRAMES))
def test_input_gradient(fname, fmt, batch, ch):
    import torch
    import kapre_amd as kapre
    f = FRAMES[fname](*plan())
    for m, p, pname in ((5, PARAM_SETS["defaults"], "defaults"), (40, PARAM_SETS["defaults"], "defaults"),
                        (40, band_vectors(40), "per band")):
        x = inputs("uniform", shape_of(fmt, batch, ch, f, m), pm.time_axis(fmt), seed=m + 1) + np.float32(0.01)
        gy = np.random.default_rng(9).normal(size=x.shape).astype(np.float32)
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        y = layer_of(p, fmt)(xt)
        assert y.grad_fn is not None
        y.backward(torch.from_numpy(gy).cuda())
        check_gradient(xt.grad.cpu().numpy(), x, gy, p, fmt, "F=%s(%d) M=%d %s %s" % (fname, f, m, fmt, pname))
        check_parity(y.detach().cpu().numpy(), x, p, fmt, "forward with the smoother kept, F=%s M=%d %s" % (fname, m, fmt))
    kapre.check_device()


# ------------------------------------------------------------------ in a model
def test_behind_the_fused_mel_chain_and_through_save_load(tmp_path):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, keras_shim
    for fmt in ("channels_last", "channels_first"):
        wave, mel = speech_mel(fmt)
        model = kapre.Sequential([mel, kapre.PCEN(data_format=fmt)])
        y = model(wave)
        assert _ffi.last_launches() == "k_pcen<4>"                   # a launch of its own behind the fused mel launch
        e = mel(wave)
        assert tuple(y.shape) == tuple(e.shape) == tuple(model.compute_output_shape(wave.shape))
        assert y.cpu().numpy().tobytes() == kapre.PCEN(data_format=fmt)(e).cpu().numpy().tobytes()
        check_parity(y.cpu().numpy(), e.cpu().numpy(), PARAM_SETS["defaults"], fmt, "behind the mel chain, %s" % fmt)

        w = torch.from_numpy(wave).cuda().requires_grad_(True)
        model(w).square().sum().backward()
        g = w.grad.cpu().numpy()
        assert g.shape == wave.shape and np.isfinite(g).all() and np.abs(g).max() > 0

        path = os.path.join(str(tmp_path), "mel_pcen_%s.keras" % fmt)
        model.save(path)
        again = keras_shim.load_model(path)
        assert type(again.layers[-1]) is kapre.PCEN
        assert again(wave).cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    kapre.check_device()


def test_device_status_is_clean_at_the_end():
    import kapre_amd as kapre
    kapre.check_device()
