"""CMVN on the GPU (kapre_amd.CMVN / backend.cmvn, kpr_cmvn_f32 / kpr_cmvn_bwd_f32) against the float64 numpy model of
tests/cmvn_model.py.

Parity rule, forward.  err = conftest.rel_err(device, float64 model) must not exceed min(max(Y1, Y2), 1e-4):
  Y1 = 8 x rel_err(float32 numpy model, float64 model) on the same input -- how far float32 arithmetic by itself strays; the
       device's reciprocal square root (v_rsq_f32) is a hardware transcendental, hence the factor (that of tests/test_pcen_gpu.py);
  Y2 = cmvn_model.first_order_bound: unit roundoff 2^-24 per arithmetic operation, one unit in the last place for the reciprocal
       square root, sums of at most R + W + ceil(F / (W R)) terms in a row (kpr_cmvn_plan), pushed to first order through c rstd and
       evaluated on the float64 model's own intermediates (the derivation is that function's docstring).
Neither yardstick is a device result; 1e-4 is the project's cap.  tests/test_cmvn_host.py shows that the limit tells the contract's
shifted sums from unshifted ones.  Gradients are held to min(8 x the float32 model's gradient error, 1e-4).  Every check prints
its figures.

Measured on an MI355X: over the 903 forward checks of this file the device strays at most 3.4e-7 from the float64
model, at most 0.12 of its limit (7.8e-7 ... 3.4e-5); over the 96 gradient checks 2.9e-8 ... 6.0e-7, at most 0.16 of the limit
(2.3e-7 ... 1.5e-5); the column sums of the gradient at most 0.28 of it.

Shapes: R, W and F_res are what kpr_cmvn_plan reports (rows per wave, waves per workgroup, the longest resident series); the frame
counts sit on both sides of a wave's chunk (R), of a workgroup's super-block (W R) and of the switch between the two forms
(F_res); the band counts cover the scalar and the 16-byte forms and a tail."""
import os

import numpy as np
import pytest

import cmvn_model as cm
from conftest import rel_err, speech
from test_pcen_gpu import LAYOUTS

pytestmark = pytest.mark.gpu

FRAMES = {"1": lambda R, W, Fr: 1, "2": lambda R, W, Fr: 2, "R-1": lambda R, W, Fr: R - 1, "R": lambda R, W, Fr: R,
          "R+1": lambda R, W, Fr: R + 1, "WR-1": lambda R, W, Fr: W * R - 1, "WR": lambda R, W, Fr: W * R,
          "WR+1": lambda R, W, Fr: W * R + 1, "Fres-1": lambda R, W, Fr: Fr - 1, "Fres": lambda R, W, Fr: Fr,
          "Fres+1": lambda R, W, Fr: Fr + 1, "2Fres+3": lambda R, W, Fr: 2 * Fr + 3}
BANDS = (1, 3, 4, 5, 40, 128, 129)
EPS = 1e-5


def plan():
    from kapre_amd import _ffi
    p = _ffi.cmvn_plan(83, 128)
    for f in (1, 1000):
        for inner in (1, 129):
            assert _ffi.cmvn_plan(f, inner) == p         # one tiling for every shape: the frame counts below straddle it
    assert p[2] >= 128
    return p


def shape_of(fmt, b, c, f, m):
    return (b, f, m, c) if fmt == "channels_last" else (b, c, f, m)


def label_of(f, inner, backward=False):
    return "k_cmvn%s<%d,%s>" % ("_bwd" if backward else "", 4 if inner % 4 == 0 else 1, "res" if f <= plan()[2] else "str")


def layer_of(fmt, norm_vars=True):
    import kapre_amd as kapre
    return kapre.CMVN(norm_vars=norm_vars, eps=EPS, data_format=fmt)


def check_parity(out, x, norm_vars, fmt, label):
    axis = cm.time_axis(fmt)
    o64 = cm.cmvn(x, norm_vars, EPS, axis)
    err = rel_err(out, o64)
    y1 = 8 * rel_err(cm.cmvn(x, norm_vars, EPS, axis, dtype=np.float32), o64)
    y2 = cm.first_order_bound(x, norm_vars, EPS, axis, plan=plan())
    limit = min(max(y1, y2), 1e-4)
    print("cmvn %s: device %.3e | 8 x float32 model %.3e | first-order bound %.3e | limit %.3e" % (label, err, y1, y2, limit))
    assert out.shape == x.shape and out.dtype == np.float32
    assert err <= limit, (label, err, limit)
    return err


def gradient_limit(x, gy, norm_vars, fmt):
    axis = cm.time_axis(fmt)
    g64 = cm.cmvn_grad(x, gy, norm_vars, EPS, axis)
    return g64, min(8 * rel_err(cm.cmvn_grad(x, gy, norm_vars, EPS, axis, dtype=np.float32), g64), 1e-4)


def inputs(kind, shape, axis, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x = rng.random(shape)
    elif kind == "-60 +- 0.1":
        x = -60 + 0.1 * rng.normal(size=shape)
    elif kind == "1000 +- 1":
        x = 1000 + rng.normal(size=shape)
    elif kind == "live then silence":
        x = rng.random(shape)
        x[(slice(None),) * axis + (slice(shape[axis] // 3, None),)] = 0.0
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def record_backward_launches(monkeypatch):
    """what the backward launcher's own thread (autograd's) sees in the thread-local launch log, call after call"""
    from kapre_amd import _ffi
    seen = []

    def wrapped(*a, _inner=_ffi.cmvn_bwd, **kw):
        out = _inner(*a, **kw)
        seen.append(_ffi.last_launches())
        return out
    monkeypatch.setattr(_ffi, "cmvn_bwd", wrapped)
    return seen


def speech_logmel(fmt="channels_last", frames=None):
    """log-mel decibels of the speech fixture through the library's own fused chain; (4, F, 40, 1) or (4, 1, F, 40)"""
    import kapre_amd as kapre
    length = 8000 if frames is None else 128 * (frames - 1) + 512
    wave = np.stack([speech(length, 1000 * i) for i in range(4)])[:, :, None]
    if fmt == "channels_first":
        wave = np.ascontiguousarray(wave.transpose(0, 2, 1))
    mel = kapre.composed.get_melspectrogram_layer(input_shape=wave.shape[1:], n_fft=512, hop_length=128, sample_rate=16000,
                                                  n_mels=40, return_decibel=True, input_data_format=fmt, output_data_format=fmt)
    return wave, mel


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("fmt,batch,ch", LAYOUTS)
@pytest.mark.parametrize("fname", list(FRAMES))
def test_parity_at_the_tile_boundaries(fname, fmt, batch, ch):
    import kapre_amd as kapre
    from kapre_amd import _ffi
    f = FRAMES[fname](*plan())
    for m in BANDS:
        x = inputs("uniform", shape_of(fmt, batch, ch, f, m), cm.time_axis(fmt), seed=m)
        inner = m * ch if fmt == "channels_last" else m
        for norm_vars in (True, False):
            out = layer_of(fmt, norm_vars)(x)
            assert _ffi.last_launches() == label_of(f, inner)
            check_parity(out.cpu().numpy(), x, norm_vars, fmt,
                         "F=%s(%d) M=%d %s b=%d c=%d norm_vars=%d" % (fname, f, m, fmt, batch, ch, norm_vars))
    kapre.check_device()


def test_resident_and_streamed_forms_give_the_same_bits(monkeypatch):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    seen = record_backward_launches(monkeypatch)
    R, W, f_res = plan()
    frames = sorted({fn(R, W, f_res) for fn in FRAMES.values() if fn(R, W, f_res) <= f_res})
    assert frames[-1] == f_res
    for f in frames:
        for fmt, batch, ch, m in (("channels_first", 1, 3, 5), ("channels_last", 2, 2, 40)):
            inner = m * ch if fmt == "channels_last" else m
            x = inputs("-60 +- 0.1", shape_of(fmt, batch, ch, f, m), cm.time_axis(fmt), seed=f)
            gy = torch.from_numpy(np.random.default_rng(f).normal(size=x.shape).astype(np.float32)).cuda()
            for norm_vars in (True, False):
                got = {}
                try:
                    for variant in (0, 1):
                        _ffi.set_option("cmvn_variant", variant)
                        form = "str" if variant else "res"
                        plain = layer_of(fmt, norm_vars)(x)
                        assert _ffi.last_launches() == "k_cmvn<%d,%s>" % (4 if inner % 4 == 0 else 1, form)
                        xt = torch.from_numpy(x).cuda().requires_grad_(True)
                        y = layer_of(fmt, norm_vars)(xt)
                        y.backward(gy)
                        assert seen[-1] == "k_cmvn_bwd<%d,%s>" % (4 if inner % 4 == 0 else 1, form)
                        got[variant] = (plain.cpu().numpy().tobytes(), y.detach().cpu().numpy().tobytes(),
                                        xt.grad.cpu().numpy().tobytes())
                finally:
                    _ffi.set_option("cmvn_variant", 0)
                assert got[0][0] == got[1][0] == got[0][1] == got[1][1], ("forward", f, fmt, norm_vars)
                assert got[0][2] == got[1][2], ("backward", f, fmt, norm_vars)
    kapre.check_device()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kind", ["uniform", "-60 +- 0.1", "1000 +- 1", "live then silence", "speech log-mel"])
def test_parity_over_inputs_in_both_forms(kind, variant):
    """F = 83 (resident, or streamed by the option) and F = 2 F_res + 3 (streamed either way)"""
    import kapre_amd as kapre
    from kapre_amd import _ffi
    fmt = "channels_last"
    f_res = plan()[2]
    try:
        _ffi.set_option("cmvn_variant", variant)
        for f in (83, 2 * f_res + 3):
            if kind == "speech log-mel":
                wave, mel = speech_logmel(fmt, f)
                x = mel(wave).cpu().numpy()
                assert x.shape == (4, f, 40, 1) and x.min() < -20
            else:
                x = inputs(kind, (2, f, 40, 2), 1, seed=f)
            for norm_vars in (True, False):
                out = kapre.backend.cmvn(x, norm_vars=norm_vars, eps=EPS, data_format=fmt)
                assert _ffi.last_launches() == "k_cmvn<4,%s>" % ("res" if f <= f_res and not variant else "str")
                check_parity(out.cpu().numpy(), x, norm_vars, fmt, "%s F=%d variant=%d norm_vars=%d" % (kind, f, variant, norm_vars))
    finally:
        _ffi.set_option("cmvn_variant", 0)
    kapre.check_device()


# ------------------------------------------------------------------ exactness, non-finite values, memory
def test_constant_columns_give_exact_zeros():
    import kapre_amd as kapre
    from kapre_amd import _ffi
    f_res = plan()[2]
    zero = np.zeros(1, np.float32).tobytes()
    try:
        for variant in (0, 1):
            _ffi.set_option("cmvn_variant", variant)
            for fmt in ("channels_last", "channels_first"):
                axis = cm.time_axis(fmt)
                for f in (1, 83, 2 * f_res + 3):
                    for norm_vars in (True, False):
                        layer = layer_of(fmt, norm_vars)
                        for value in (0.0, -80.0, 1000.5):
                            out = layer(np.full(shape_of(fmt, 2, 3, f, 5), value, np.float32)).cpu().numpy()
                            assert out.tobytes() == zero * out.size, (fmt, f, norm_vars, value)        # +0.0, bit for bit
                        # a band at the decibel floor inside live data: (b, ch, t, band 2) / (b, t, band 2, ch)
                        x = inputs("-60 +- 0.1", shape_of(fmt, 2, 3, f, 5), axis, seed=f)
                        band = (slice(None), slice(None), 2) if fmt == "channels_last" else (slice(None), slice(None), slice(None), 2)
                        x[band] = -80.0
                        out = layer(x).cpu().numpy()
                        assert out[band].tobytes() == zero * out[band].size, (fmt, f, norm_vars)
                        if f > 1:
                            assert np.abs(out).max() > 0
                            check_parity(out, x, norm_vars, fmt, "a floor band, %s F=%d variant=%d norm_vars=%d" % (fmt, f, variant, norm_vars))
    finally:
        _ffi.set_option("cmvn_variant", 0)
    kapre.check_device()


def test_a_nan_makes_exactly_its_own_column_non_finite():
    import kapre_amd as kapre
    R, W, f_res = plan()
    t0 = R + 2
    for f in (f_res - 1, 2 * f_res + 3):
        for fmt, col in (("channels_first", (0, 2, slice(None), 17)), ("channels_last", (1, slice(None), 17, 2))):
            for norm_vars in (True, False):
                for bad_value in (np.nan, np.inf):
                    x = inputs("uniform", shape_of(fmt, 2, 3, f, 40), cm.time_axis(fmt), seed=3)
                    layer = layer_of(fmt, norm_vars)
                    clean = layer(x).cpu().numpy()
                    bad = x.copy()
                    series = bad[col]
                    series[t0] = bad_value
                    bad[col] = series
                    got = layer(bad).cpu().numpy()
                    assert not np.isfinite(got[col]).any(), (f, fmt, norm_vars, bad_value)
                    mask = np.ones(x.shape, bool)
                    mask[col] = False
                    assert np.isfinite(got[mask]).all() and got[mask].tobytes() == clean[mask].tobytes()
    kapre.check_device()                                             # a NaN is data, not a fault


def test_a_base_pointer_off_by_one_float_takes_the_scalar_form():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    R, W, f_res = plan()
    for f in (W * R + 1 if W * R < f_res else f_res - 1, f_res + 1):
        x = inputs("-60 +- 0.1", (1, 3, f, 40), 2)
        buf = torch.zeros(x.size + 1, device="cuda")
        view = buf[1:].view(x.shape)
        view.copy_(torch.from_numpy(x))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        form = "res" if f <= f_res else "str"
        out = layer_of("channels_first")(view)
        assert _ffi.last_launches() == "k_cmvn<1,%s>" % form
        check_parity(out.cpu().numpy(), x, True, "channels_first", "view one float off, F=%d" % f)
        aligned = layer_of("channels_first")(x)
        assert _ffi.last_launches() == "k_cmvn<4,%s>" % form
        check_parity(aligned.cpu().numpy(), x, True, "channels_first", "the same block, aligned, F=%d" % f)
    kapre.check_device()


def test_non_contiguous_input_no_frames_and_rank():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    x = inputs("uniform", (2, 40, 19, 3), 1)                     # stored (b, mel, t, ch): the layer sees a transposed view
    xt = torch.from_numpy(x).cuda().transpose(1, 2)
    assert not xt.is_contiguous()
    out = layer_of("channels_last")(xt)
    check_parity(out.cpu().numpy(), np.ascontiguousarray(x.transpose(0, 2, 1, 3)), True, "channels_last", "transposed view")
    layer_of("channels_last")(x)                                 # (a launch, so that the log is not empty before the next call)
    assert _ffi.last_launches() != ""
    for shape in ((2, 0, 40, 3), (0, 7, 40, 3), (2, 7, 0, 3)):
        empty = layer_of("channels_last")(np.zeros(shape, np.float32))
        assert tuple(empty.shape) == shape and empty.dtype == torch.float32 and _ffi.last_launches() == ""
    with pytest.raises(ValueError, match="rank-4"):
        layer_of("channels_last")(torch.zeros((7, 40, 3), device="cuda"))
    kapre.check_device()


def test_the_same_call_twice_gives_the_same_bits():
    import torch
    import kapre_amd as kapre
    f_res = plan()[2]
    for f in (83, 2 * f_res + 3):
        x = inputs("-60 +- 0.1", (2, f, 40, 2), 1, seed=5)
        gy = torch.from_numpy(inputs("uniform", x.shape, 1, seed=6)).cuda()
        runs = []
        for _ in range(2):
            xt = torch.from_numpy(x).cuda().requires_grad_(True)
            y = layer_of("channels_last")(xt)
            y.backward(gy)
            runs.append((y.detach().cpu().numpy().tobytes(), xt.grad.cpu().numpy().tobytes()))
        assert runs[0] == runs[1]
    kapre.check_device()


# ------------------------------------------------------------------ gradient
@pytest.mark.parametrize("fmt,batch,ch", [("channels_first", 1, 3), ("channels_last", 2, 2)])
@pytest.mark.parametrize("fname", list(FRAMES))
def test_input_gradient(fname, fmt, batch, ch, monkeypatch):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    seen = record_backward_launches(monkeypatch)
    f = FRAMES[fname](*plan())
    axis = cm.time_axis(fmt)
    for m in (5, 40):
        inner = m * ch if fmt == "channels_last" else m
        for norm_vars in (True, False):
            x = inputs("uniform", shape_of(fmt, batch, ch, f, m), axis, seed=m + 1)
            gy = np.random.default_rng(9).normal(size=x.shape).astype(np.float32)
            plain = layer_of(fmt, norm_vars)(x)
            assert _ffi.last_launches() == label_of(f, inner)
            xt = torch.from_numpy(x).cuda().requires_grad_(True)
            y = layer_of(fmt, norm_vars)(xt)
            assert y.grad_fn is not None and _ffi.last_launches() == label_of(f, inner)
            assert y.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()     # keeping rstd changes no bit of y
            y.backward(torch.from_numpy(gy).cuda())
            assert seen[-1] == label_of(f, inner, backward=True)
            gx = xt.grad.cpu().numpy()
            g64, limit = gradient_limit(x, gy, norm_vars, fmt)
            err = rel_err(gx, g64)
            # the defining property of the centring: the gradient of every column sums to 0 over time.  The yardstick of a sum
            # is the sum of its terms' magnitudes (a float32 mean(gy) alone is off by 2^-24 |mean|, F times in the column sum;
            # measured against max |g| the float32 MODEL's own column sums exceed the gradient limit from F = 16 on): in the manner
            # of rel_err, max over the columns of |sum_t gx| over max over the columns of sum_t |g64| must stay within the gradient
            # limit (F = 1: the gradient is 0 and so must the device's be)
            col_sum, col_abs = np.abs(gx.astype(np.float64).sum(axis=axis)), np.abs(g64).sum(axis=axis)
            centre = float(np.max(col_sum) / max(np.max(col_abs), 1e-30))
            print("cmvn gradient F=%s(%d) M=%d %s norm_vars=%d: device %.3e | column sums %.3e | limit (8 x float32 model) %.3e"
                  % (fname, f, m, fmt, norm_vars, err, centre, limit))
            assert gx.shape == x.shape and err <= limit, (fname, m, fmt, norm_vars, err, limit)
            assert centre <= limit, (fname, m, fmt, norm_vars, centre, limit)
    kapre.check_device()


# ------------------------------------------------------------------ in a model
def test_behind_the_fused_mel_chain_and_through_save_load(tmp_path):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, keras_shim
    for fmt in ("channels_last", "channels_first"):
        wave, mel = speech_logmel(fmt)
        model = kapre.Sequential([mel, kapre.CMVN(data_format=fmt)])
        y = model(wave)
        assert _ffi.last_launches() == "k_cmvn<4,res>"               # a launch of its own behind the fused mel launch
        e = mel(wave)
        assert tuple(y.shape) == tuple(e.shape) == tuple(model.compute_output_shape(wave.shape))
        assert tuple(model.layers[-1].compute_output_shape((None,) + tuple(e.shape[1:]))) == (None,) + tuple(y.shape[1:])
        assert y.cpu().numpy().tobytes() == kapre.CMVN(data_format=fmt)(e).cpu().numpy().tobytes()
        check_parity(y.cpu().numpy(), e.cpu().numpy(), True, fmt, "behind the mel chain, %s" % fmt)

        w = torch.from_numpy(wave).cuda().requires_grad_(True)
        model(w).square().sum().backward()
        g = w.grad.cpu().numpy()
        assert g.shape == wave.shape and np.isfinite(g).all() and np.abs(g).max() > 0

        path = os.path.join(str(tmp_path), "mel_cmvn_%s.keras" % fmt)
        model.save(path)
        again = keras_shim.load_model(path)
        assert type(again.layers[-1]) is kapre.CMVN
        assert again(wave).cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    kapre.check_device()


def test_spec_augment_masks_in_place_and_delta_and_mfcc_chain_behind_it():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    fmt = "channels_last"
    wave, mel = speech_logmel(fmt)
    cmvn = kapre.CMVN(data_format=fmt)
    y = cmvn(mel(wave)).cpu().numpy()
    aug = kapre.SpecAugment(freq_mask_param=5, time_mask_param=10, n_freq_masks=2, n_time_masks=2, mask_value=-7.0, data_format=fmt)
    model = kapre.Sequential([mel, cmvn, aug])
    assert model(wave).cpu().numpy().tobytes() == y.tobytes()        # inference: the augmentation is the identity
    assert _ffi.last_launches() == "k_cmvn<4,res>"
    live = torch.cuda.memory_allocated()
    out = model(wave, training=True)
    assert _ffi.last_launches() == "k_specaug_apply"
    assert torch.cuda.memory_allocated() - live < 1.5 * y.size * 4   # one block: CMVN's output, masked in place
    out = out.cpu().numpy()
    masked = out != y
    assert masked.any() and (out[masked] == -7.0).all()
    d = kapre.Sequential([mel, cmvn, kapre.Delta(data_format=fmt)])(wave)
    c = kapre.Sequential([mel, cmvn, kapre.LogmelToMFCC(n_mfccs=13, data_format=fmt)])(wave)
    assert tuple(d.shape) == y.shape and tuple(c.shape) == y.shape[:2] + (13, 1)
    assert np.isfinite(d.cpu().numpy()).all() and np.isfinite(c.cpu().numpy()).all() and np.abs(d.cpu().numpy()).max() > 0
    kapre.check_device()


def test_device_status_is_clean_at_the_end():
    import kapre_amd as kapre
    kapre.check_device()
