"""kpr_yin_f32 / kapre_amd.YIN on the GPU against the float64 model of tests/yin_model.py.

The curve: |y - y64| <= (2 W + tau_hi + 8) 2^-24 |y64| elementwise, in either form.  The decision: taken by the
model from the DEVICE's float32 curve, it reproduces tau* and cmnd exactly and f0 within 6 * 2^-24.  Worst curve error measured
on an MI355X: 0.061 of the bound (64/32/8), 0.021 at 2048/1024/512."""
import numpy as np
import pytest

import yin_model
from kapre_amd import _ffi

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SR = 22050.0
TONES = (110.0, 147.0, 196.0, 262.0, 349.0, 493.0)
GEOMETRIES = [(2048, 1024, 512), (512, 256, 64), (64, 32, 8), (400, 200, 160), (67, 30, 7)]
LAYOUTS = [("channels_last", 3, False), ("channels_first", 2, True), ("channels_last", 1, True)]


def tone(f, n, harmonics=3):
    t = np.arange(n) / SR
    return sum(np.sin(2 * np.pi * h * f * t) / h for h in range(1, harmonics + 1))


def signals(n_series, n, tau_hi, seed):
    """(n_series, n) float32: harmonic tones, then white noise, a constant and an impulse"""
    rng = np.random.default_rng(seed)
    kinds = [lambda k=k: tone(max(TONES[k % 6], SR / (0.7 * tau_hi)), n) for k in range(n_series)]
    kinds[1:4] = [lambda: rng.standard_normal(n), lambda: np.full(n, 0.37), lambda: (np.arange(n) == n // 3) * 1.0][:n_series - 1]
    return np.stack([k() for k in kinds]).astype(np.float32)


def run(x, fmt, geometry, tau_min, tau_hi, thr, pad_end):
    """x (b, c, n) -> f0 (b, c, frames), cmnd, curve (b, c, frames, tau_hi + 1) as numpy, and the launch label"""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 1, 2) if fmt == "channels_last" else x)).cuda()
    f0, cmnd, curve = _ffi.yin(xt, fmt, SR, *geometry, tau_min, tau_hi, thr, pad_end, want_curve=True)
    label = _ffi.last_launches()
    back = (lambda a: np.moveaxis(a.cpu().numpy(), 1, 2)) if fmt == "channels_last" else (lambda a: a.cpu().numpy())
    return back(f0), back(cmnd), curve.cpu().numpy(), label


def check(x, ref, fmt, geometry, tau_min, tau_hi, thr, pad_end, form):
    """the curve against ``ref`` (float64, per series), the decision against the model on the device's curve -> worst error / bound"""
    fl, W, hop = geometry
    f0, cmnd, y, label = run(x, fmt, geometry, tau_min, tau_hi, thr, pad_end)
    assert label.startswith("k_yin<%s," % form), label
    worst = 0.0
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            y64 = ref[b][c]
            assert y[b, c].shape == y64.shape
            if not pad_end and (x[b, c] == x[b, c, 0]).all():
                assert (y[b, c] == 1.0).all()                                          # a constant frame: exactly 1
            err, bound = np.abs(y[b, c] - y64), (2 * W + tau_hi + 8) * U * np.abs(y64)
            assert (err <= bound).all(), (b, c, float((err / np.maximum(bound, 1e-300)).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            for t in range(y64.shape[0]):
                want_f0, want_c, _ = yin_model.decide(y[b, c, t], SR, tau_min, tau_hi, np.float32(thr))
                assert cmnd[b, c, t] == want_c
                assert abs(f0[b, c, t] - want_f0) <= 6 * U * want_f0
    return worst


@pytest.mark.parametrize("fmt,ch,pad_end", LAYOUTS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_curve_and_decision(geometry, fmt, ch, pad_end):
    fl, W, hop = geometry
    tau_min, tau_hi = (11, 340) if fl - W - 1 >= 340 else (2, fl - W - 1)
    F, form = _ffi.yin_plan(fl, W, hop, tau_min, tau_hi)
    assert form == (_ffi.YIN_SHARED if W % hop == 0 else _ffi.YIN_DIRECT)
    worst = 0.0
    for n_frames in sorted({1, 2, max(F - 1, 1), F, F + 1, 2 * F + 1}):
        n = (n_frames - 1) * hop + (hop // 2 + 1 if pad_end else fl + hop // 2)        # not a multiple of hop
        x = signals(2 * ch, n, tau_hi, n_frames).reshape(2, ch, n)
        ref = [[yin_model.curve(x[b, c], fl, W, hop, tau_hi, pad_end) for c in range(ch)] for b in range(2)]
        for thr in (0.1, 1e-6):                                                       # 1e-6: no trough passes, the argmin branch
            worst = max(worst, check(x, ref, fmt, geometry, tau_min, tau_hi, thr, pad_end,
                                     "shared" if form == _ffi.YIN_SHARED else "direct"))
        old = _ffi.set_option("yin_variant", 1)
        try:
            worst = max(worst, check(x, ref, fmt, geometry, tau_min, tau_hi, 0.1, pad_end, "direct"))
        finally:
            _ffi.set_option("yin_variant", old)
    print("worst curve error / bound %s: %.4f" % (geometry, worst))


@pytest.mark.parametrize("period,want", [(12, 12), (31, 31)])
def test_trough_at_tau_min_and_choice_of_tau_hi(period, want):
    """a tone of period tau_min: the trough at tau_min; lags 29 ... 31 on a tone of period 31: the minimum at tau_hi, unrefined"""
    tau_min, tau_hi = (12, 31) if period == 12 else (29, 31)
    x = tone(SR / period, 64 + 8 * 9, harmonics=1).astype(np.float32).reshape(1, 1, -1)
    f0, cmnd, y, _ = run(x, "channels_first", (64, 32, 8), tau_min, tau_hi, 0.1, False)
    for t in range(y.shape[2]):
        assert yin_model.decide(y[0, 0, t], SR, tau_min, tau_hi, np.float32(0.1))[2] == want
        assert f0[0, 0, t] == np.float32(SR) / np.float32(want) and cmnd[0, 0, t] == y[0, 0, t, want]


def test_end_to_end_tones_with_noise():
    """the six tones with 1 % noise at 2048/1024/512: the lag of the all-float64 model, f0 within 1e-4"""
    rng = np.random.default_rng(7)
    n = 2048 + 3 * 512
    x = np.stack([tone(f, n) for f in TONES]) + 0.01 * rng.standard_normal((6, n))
    x = x.astype(np.float32).reshape(6, 1, n)
    f0, cmnd, y, _ = run(x, "channels_last", (2048, 1024, 512), 11, 340, 0.1, False)
    for k in range(6):
        y64 = yin_model.curve(x[k, 0], 2048, 1024, 512, 340)
        for t in range(4):
            f64, _, tau64 = yin_model.decide(y64[t], SR, 11, 340, 0.1)
            assert yin_model.decide(y[k, 0, t], SR, 11, 340, np.float32(0.1))[2] == tau64
            assert abs(f0[k, 0, t] - f64) <= 1e-4 * f64 and abs(f64 - TONES[k]) < 0.01 * TONES[k]


def test_non_finite_samples_stay_in_their_frames():
    geometry, tau_min, tau_hi = (64, 32, 8), 2, 31
    x = signals(2, 64 + 8 * 20, tau_hi, 3).reshape(1, 2, -1)
    clean = run(x, "channels_first", geometry, tau_min, tau_hi, 0.1, False)
    bad = x.copy()
    bad[0, 0, 77], bad[0, 1, 130] = np.nan, np.inf
    got = run(bad, "channels_first", geometry, tau_min, tau_hi, 0.1, False)
    for c, p in ((0, 77), (1, 130)):
        for t in range(clean[0].shape[2]):
            reads = t * 8 <= p < t * 8 + 32 + tau_hi                                  # the W + tau_hi samples a frame reads
            for a, b in zip(got[:3], clean[:3]):
                assert np.isnan(a[0, c, t]).all() if reads else np.array_equal(a[0, c, t], b[0, c, t]), (c, t)


def test_no_frames_and_repeatability():
    x = signals(2, 50, 31, 1).reshape(1, 2, -1)
    f0, cmnd, y, label = run(x, "channels_first", (64, 32, 8), 2, 31, 0.1, False)      # time < frame_length, no pad_end
    assert f0.shape == (1, 2, 0) and cmnd.shape == (1, 2, 0) and label == ""
    x = signals(6, 5000, 340, 2).reshape(2, 3, -1)
    first, again = (run(x, "channels_first", (2048, 1024, 512), 11, 340, 0.1, True) for _ in range(2))
    assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3]))


def test_layer_in_a_sequential_behind_resample():
    import torch
    import kapre_amd as kapre
    x = torch.from_numpy(tone(220.0, 8000).astype(np.float32).reshape(1, -1, 1)).cuda().requires_grad_(True)
    model = kapre.Sequential([kapre.Resample(22050, 16000, input_shape=(8000, 1)),
                              kapre.YIN(80, 1000, 16000, frame_length=1024, return_cmnd=True)])
    out = model(x)
    assert tuple(out.shape) == (1, 19, 1, 2)                                          # 5805 samples, frames of 1024 every 256
    assert out.grad_fn is None and not out.requires_grad
    f0, cmnd = out[0, 1:-1, 0, 0], out[0, 1:-1, 0, 1]
    assert bool((abs(f0 - 220.0) < 1.0).all()) and bool((cmnd < 0.1).all())
