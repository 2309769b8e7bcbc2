"""k_mdct / k_imdct on the device against the float64 model (tests/mdct_model.py).  Error rule: elementwise
|X - X64| <= K 2^-24 s sum_n |w[n] x[n]| per frame, and K 2^-24 s' |w[n]| sum_k |X[t, k]| summed over the two frames of an output
sample, K derived from the roundings on the longest path: 2 (fold, or window and overlap-add) + log2(N/4) (butterfly levels)
+ 3.25 per complex twiddle product (2 + 4 of them for the radices (16, 8) and (16, 16), 2 + 6 for (16, 16, 2) and (16, 16, 4))."""
import numpy as np
import pytest
import torch

import kapre_amd
import mdct_model as mm
from conftest import rel_err
from kapre_amd import _ffi, backend

pytestmark = pytest.mark.gpu
K = {512: 28.5, 1024: 29.5, 2048: 37.0, 4096: 38.0}
U = 2.0 ** -24
CL, CF = "channels_last", "channels_first"


def series_last(a, fmt):
    """(b, t, ch) / (b, ch, t) or (b, frames, M, ch) / (b, ch, frames, M) -> the series axes first, numpy float64"""
    a = a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    return np.moveaxis(a, -1, 1) if fmt == CL else a


def as_fmt(a, fmt):
    return np.ascontiguousarray(np.moveaxis(a, 1, -1) if fmt == CL else a, dtype=np.float32)


def window64(N, name=None):
    return backend.window_values(backend.mdct_window_fn(name), N, np.float32).astype(np.float64)


def seam_run(N):
    """a run that is no multiple of the frames per wave step, and T = 2 run + 3 frames: two seams, T % G != 0 where G > 1"""
    return 64 // _ffi.mdct_plan(N)[1] + 1


def signals(N, T, rng):
    """waveform (2, 2, time) for T frames: noise, and a unit impulse in each quarter of a frame; coefficients (2, 2, T, M): noise,
    and a unit at k = 0, 1, M-2, M-1"""
    M = N // 2
    x = rng.uniform(-1, 1, (2, 2, (T + 1) * M + 5))
    x[1, 0] = 0
    x[1, 0, [M + 3, 2 * M + N // 4 + 5, 4 * M - N // 4 - 1, 5 * M - 2]] = 1
    X = rng.uniform(-1, 1, (2, 2, T, M))
    X[1, 1] = 0
    X[1, 1, [0, 1, 3, T - 1], [0, 1, M - 2, M - 1]] = 1
    return x, X


def check(got, want, bound, N, what):
    ratio = float((np.abs(got - want) / np.maximum(K[N] * U * bound, 1e-300))[np.broadcast_to(bound, want.shape) > 0].max())
    print("%s N=%d: worst error %.3f of the bound, rel_err %.2e" % (what, N, ratio, rel_err(got, want)))
    assert got.shape == want.shape and ratio <= 1 and rel_err(got, want) <= 1e-4
    assert not np.any(got[np.broadcast_to(bound, want.shape) == 0])


@pytest.mark.parametrize("norm", [None, "ortho"])
@pytest.mark.parametrize("fmt,cfmt", [(CL, CL), (CF, CF), (CL, CF), (CF, CL)])
@pytest.mark.parametrize("N", sorted(K))
def test_against_model(N, fmt, cfmt, norm):
    run, w, (s, si) = seam_run(N), window64(N), mm.scales(N, norm)
    x, X = signals(N, 2 * run + 3, np.random.default_rng(N))
    old = _ffi.set_option("mdct_run", run)
    try:
        got = backend.mdct(as_fmt(x, fmt), N, norm=norm, data_format=fmt, output_data_format=cfmt)
        inv = backend.inverse_mdct(as_fmt(X, cfmt), norm=norm, data_format=cfmt, output_data_format=fmt)
    finally:
        _ffi.set_option("mdct_run", old)
    x32, X32 = as_fmt(x, CF).astype(np.float64), as_fmt(X, CF).astype(np.float64)
    check(series_last(got, cfmt), mm.mdct(x32, N, w, s), mm.mdct_bound(x32, N, w, s), N, "mdct")
    check(series_last(inv, fmt), mm.inverse_mdct(X32, N, w, si), mm.inverse_bound(X32, N, w, si), N, "imdct")


@pytest.mark.parametrize("pad_begin,pad_end,time", [(True, False, 2000), (False, True, 2000), (False, False, 500), (True, True, 100)])
def test_padding_and_length(pad_begin, pad_end, time):
    N, M, w, (s, si) = 512, 256, window64(512, "sine_window"), mm.scales(512, None)
    x = np.random.default_rng(5).uniform(-1, 1, (1, 2, time)).astype(np.float32)
    got = backend.mdct(x, N, "sine_window", pad_begin=pad_begin, pad_end=pad_end, data_format=CF)
    want = mm.mdct(x, N, w, s, pad_begin, pad_end)
    assert tuple(got.shape) == want.shape
    if want.shape[2] == 0:
        assert "k_mdct" not in _ffi.last_launches()
    else:
        check(series_last(got, CF), want, mm.mdct_bound(x, N, w, s, pad_begin, pad_end), N, "mdct")
    X = want.astype(np.float32)
    for length in (None, time, want.shape[2] * M + 3 * M + 1):        # the default, trimmed (or extended), zero-extended
        inv = series_last(backend.inverse_mdct(X, "sine_window", pad_begin=pad_begin, length=length, data_format=CF), CF)
        ref = mm.inverse_mdct(X, N, w, si, pad_begin, length)
        bound = mm.inverse_bound(X, N, w, si, pad_begin, length)
        assert inv.shape == ref.shape and np.all(np.abs(inv - ref) <= K[N] * U * bound)
        assert not np.any(inv[bound == 0]) and not np.any(np.signbit(inv[bound == 0]))


@pytest.mark.parametrize("N", [512, 2048])
def test_bits_do_not_depend_on_position(N):
    M, run = N // 2, seam_run(N)
    x, X = (torch.from_numpy(a.astype(np.float32)).cuda() for a in signals(N, 2 * run + 3, np.random.default_rng(7)))
    auto = backend.mdct(x, N, data_format=CF), backend.inverse_mdct(X, data_format=CF)
    old = _ffi.set_option("mdct_run", run)
    try:
        small = backend.mdct(x, N, data_format=CF), backend.inverse_mdct(X, data_format=CF)
        shifted = backend.mdct(x[..., M:].contiguous(), N, data_format=CF)
    finally:
        _ffi.set_option("mdct_run", old)
    again = backend.mdct(x, N, data_format=CF), backend.inverse_mdct(X, data_format=CF)
    for a, b, c in zip(auto, small, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert torch.equal(shifted.view(torch.int32), auto[0][:, :, 1:].view(torch.int32))


def test_round_trip_through_the_layers():
    x = np.random.default_rng(9).uniform(-1, 1, (2, 9001, 2)).astype(np.float32)
    kw = dict(window_name=None, norm="ortho", pad_begin=True)
    rec = kapre_amd.InverseMDCT(**kw)(kapre_amd.MDCT(2048, pad_end=True, **kw)(x))[:, :9001].cpu().numpy()
    w, (s, si) = window64(2048), mm.scales(2048, "ortho")
    x64 = np.moveaxis(x.astype(np.float64), -1, 1)
    model = rel_err(mm.inverse_mdct(mm.mdct(x64, 2048, w, s, True, True), 2048, w, si, True)[..., :9001], x64)
    print("round trip rel_err: device %.2e, float64 model with the float32 window %.2e" % (rel_err(rec, x), model))
    assert rel_err(rec, x) <= 1e-4


@pytest.mark.parametrize("fmt", [CL, CF])
def test_gradients_are_the_other_transform(fmt):
    N, M, run = 512, 256, seam_run(512)
    T, w, (s, si), rng = 2 * run + 3, window64(512), mm.scales(512, None), np.random.default_rng(11)
    x, X = signals(N, T, rng)
    g, gy = rng.uniform(-1, 1, (2, 2, T, M)), rng.uniform(-1, 1, (2, 2, (T + 1) * M + 7))
    xt = torch.from_numpy(as_fmt(x, fmt)).cuda().requires_grad_(True)
    Xt = torch.from_numpy(as_fmt(X, fmt)).cuda().requires_grad_(True)
    old = _ffi.set_option("mdct_run", run)
    try:
        y = kapre_amd.MDCT(N, input_data_format=fmt, output_data_format=fmt)(xt)
        (y * torch.from_numpy(as_fmt(g, fmt)).cuda()).sum().backward()
        z = kapre_amd.InverseMDCT(length=gy.shape[-1], input_data_format=fmt, output_data_format=fmt)(Xt)
        (z * torch.from_numpy(as_fmt(gy, fmt)).cuda()).sum().backward()
    finally:
        _ffi.set_option("mdct_run", old)
    g32, gy32, x32 = (as_fmt(a, CF).astype(np.float64) for a in (g, gy[..., :(T + 1) * M], x))
    time = x.shape[-1]
    check(series_last(xt.grad, fmt), mm.inverse_mdct(g32, N, w, s, length=time), mm.inverse_bound(g32, N, w, s, length=time), N, "mdct^T")
    check(series_last(Xt.grad, fmt), mm.mdct(gy32, N, w, si), mm.mdct_bound(gy32, N, w, si), N, "imdct^T")
    # <MDCT x, g> = <x, MDCT^T g> from the device's two results, summed in float64: each side is within K u of the exact value
    lhs, rhs = float((series_last(y, fmt) * g32).sum()), float((x32 * series_last(xt.grad, fmt)).sum())
    assert abs(lhs - rhs) <= 2 * K[N] * U * float((mm.mdct_bound(x32, N, w, s) * np.abs(g32)).sum())


def test_nan_stays_in_its_frames():
    N, M = 512, 256
    x, X = (torch.from_numpy(a.astype(np.float32)).cuda() for a in signals(N, 9, np.random.default_rng(13)))
    clean = backend.mdct(x, N, data_format=CF), backend.inverse_mdct(X, data_format=CF)
    x[0, 1, 3 * M + 17] = float("nan")
    X[1, 0, 4, 100] = float("nan")
    got = backend.mdct(x, N, data_format=CF), backend.inverse_mdct(X, data_format=CF)
    hit = torch.zeros_like(clean[0], dtype=torch.bool), torch.zeros_like(clean[1], dtype=torch.bool)
    hit[0][0, 1, 2:4] = True
    hit[1][1, 0, 4 * M:4 * M + N] = True
    for c, g, h in zip(clean, got, hit):
        assert torch.isnan(g[h]).all() and torch.equal(g[~h].view(torch.int32), c[~h].view(torch.int32))
