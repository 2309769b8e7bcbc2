"""The table-free resampler on the GPU (backend.resample(method='direct'), kpr_resample_direct_f32) against the float64 model
of tests/resample_direct_model.py.

Parity rule, derived and not tuned, per output:

    |y - y64| <= (n_taps + 3) 2^-24 sum_k |tap_k x_k| + C 2^-24 s sum_{k in support} |x_k| + 1e-37,   C = 17 + 6 / L

The first term is the table kernel's: n_taps float32 FMAs and three roundings of a tap.  The second is what computed taps
add: the position's rounding moves a tap by an amount that is absolute near the zeros of the sinc, and the evaluation's
roundings beyond the three are bounded by |tap| <= s.  A float32 position misses this rule by orders of magnitude
(test_resample_direct_host.py).  Every check prints its worst |y - y64| / bound; on an MI355X the worst of a pair is 0.041 ..
0.066 forward and 0.043 .. 0.076 for the adjoint.

Lengths: 1; 5 (shorter than the support); 3 n_taps + 7; three tiles of kpr_resample_direct_plan's outputs_per_tile and a
ragged tail."""
import numpy as np
import pytest

import resample_direct_model as dm
import resample_model as rm
from conftest import speech

pytestmark = pytest.mark.gpu

PAIRS = [(25427, 24000), (24000, 25427), (10079, 8000), (55, 49), (2, 1), (1, 2), (48000, 47999), (2147483647, 2147483629),
         (44100, 16000)]
IDS = ["%dto%d" % p for p in PAIRS]
BATCH = 3


def shape_of(fmt, b, c, t):
    return (b, t, c) if fmt == "channels_last" else (b, c, t)


def to_layout(x_bct, fmt):
    """(b, c, t) -> the layout of ``fmt``, contiguous"""
    return np.ascontiguousarray(np.moveaxis(x_bct, 1, 2)) if fmt == "channels_last" else np.ascontiguousarray(x_bct)


def from_layout(y, fmt):
    return np.moveaxis(y, 2, 1) if fmt == "channels_last" else y


def plan(orig, new, adjoint):
    """(n_taps, outputs_per_tile)"""
    from kapre_amd import _ffi
    return _ffi.resample_direct_plan(orig, new, 6, 0.99, adjoint)


def three_tiles(orig, new, adjoint):
    """an input length T whose pass in that direction writes three whole tiles and a ragged tail"""
    tile = plan(orig, new, adjoint)[1]
    want = 3 * tile + tile // 3 + 1                                   # outputs of that direction
    if adjoint:
        return want                                                   # the adjoint writes T samples
    ro, rn = rm.reduced(orig, new)
    T = -(-want * ro // rn)
    assert rm.out_length(T, orig, new) >= want
    return T


def signals(kind, n, T, seed):
    """(n, T) float32: different data per row"""
    if kind == "noise":
        return np.random.default_rng(seed).standard_normal((n, T)).astype(np.float32)
    rows = [speech(T, offset=12000 * i) for i in range(n)]
    return np.stack([np.pad(r, (0, T - r.shape[0])) for r in rows]).astype(np.float32)


def check(y, y64, bound, label):
    err = np.abs(y.astype(np.float64) - y64)
    worst = float(np.max(err / bound)) if err.size else 0.0
    print("resample direct %s: worst |y - y64| / bound = %.3f" % (label, worst))
    assert y.dtype == np.float32 and y.shape == y64.shape
    assert np.all(err <= bound), (label, worst)
    return worst


def to_np(t):
    return t.detach().cpu().numpy()


def run(x_bct, orig, new, fmt, length=None):
    from kapre_amd import backend
    return from_layout(to_np(backend.resample(to_layout(x_bct, fmt), orig, new, data_format=fmt, method='direct', length=length)), fmt)


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("orig,new", PAIRS, ids=IDS)
def test_forward_parity(orig, new):
    import kapre_amd as kapre

    n_taps = plan(orig, new, False)[0]
    worst = 0.0
    for T in (1, 5, 3 * n_taps + 7, three_tiles(orig, new, False)):
        n_out = rm.out_length(T, orig, new)
        for kind in ("speech", "noise"):
            x = signals(kind, BATCH * 3, T, seed=T).reshape(BATCH, 3, T)
            y64, bound = dm.resample(x, orig, new), dm.bound(x, n_out, orig, new)          # once, shared by the shapes below
            for fmt in ("channels_last", "channels_first"):
                layer = kapre.Resample(orig, new, data_format=fmt, method='direct')
                for C in (1, 2, 3):
                    y = to_np(layer(to_layout(x[:, :C], fmt)))
                    assert y.shape == shape_of(fmt, BATCH, C, n_out)
                    worst = max(worst, check(from_layout(y, fmt), y64[:, :C], bound[:, :C],
                                             "%d->%d T=%d %s %s C=%d" % (orig, new, T, kind, fmt, C)))
    print("resample direct forward %d->%d: worst ratio %.3f" % (orig, new, worst))
    kapre.check_device()


def test_long_tone():
    """one mono item of 300 000 samples at 0.45 cycles per sample, 25427 -> 24000: a float32 position is wrong by 2^-24 i
    samples and misses this bound by three orders of magnitude (test_resample_direct_host.py)"""
    import kapre_amd as kapre

    T = 300000
    x = np.sin(2.0 * np.pi * 0.45 * np.arange(T)).astype(np.float32)[None, None]
    n_out = rm.out_length(T, 25427, 24000)
    y = run(x, 25427, 24000, "channels_first")
    check(y, dm.resample(x, 25427, 24000), dm.bound(x, n_out, 25427, 24000), "long tone")
    kapre.check_device()


@pytest.mark.parametrize("orig,new", [(25427, 24000), (1, 2), (44100, 16000), (2147483647, 2147483629)])
def test_free_out_len(orig, new):
    import kapre_amd as kapre

    T = 700
    natural, n_taps = rm.out_length(T, orig, new), plan(orig, new, False)[0]
    x = signals("noise", BATCH * 2, T, seed=3).reshape(BATCH, 2, T)
    for length in (natural // 2, natural + n_taps, natural + 1000):
        for fmt in ("channels_last", "channels_first"):
            y = run(x, orig, new, fmt, length)
            assert y.shape == (BATCH, 2, length)
            check(y, dm.resample(x, orig, new, length=length), dm.bound(x, length, orig, new),
                  "%d->%d length %d of %d %s" % (orig, new, length, natural, fmt))
    P, Q, H = dm.shape(orig, new)[:3]
    tail = y[..., natural + H * P // Q + 2:]                          # past the filter's tail: exact +0.0
    assert tail.shape[-1] > 500 and not tail.any() and not np.signbit(tail).any()
    kapre.check_device()


@pytest.mark.parametrize("orig,new", PAIRS, ids=IDS)
def test_tile_seams(orig, new):
    """one impulse per signal, at every input position within n_taps of a tile seam, of the signal's start and of its end"""
    import kapre_amd as kapre

    n_taps, tile = plan(orig, new, False)
    P, Q = dm.shape(orig, new)[:2]
    T = three_tiles(orig, new, False)
    spots = set(range(0, n_taps + 1)) | set(range(T - n_taps - 1, T))
    for m in (tile, 2 * tile, 3 * tile):
        centre = m * Q // P
        spots |= set(range(centre - n_taps - 1, centre + n_taps + 2))
    spots = sorted(s for s in spots if 0 <= s < T)
    if len(spots) % 2:
        spots.append(T // 2)
    x = np.zeros((len(spots), T), dtype=np.float32)
    x[np.arange(len(spots)), spots] = np.float32(0.7) * (1 + np.arange(len(spots)) % 3)
    n_out = rm.out_length(T, orig, new)
    y64, bound = dm.resample(x, orig, new), dm.bound(x, n_out, orig, new)
    y = run(x[:, None, :], orig, new, "channels_first")[:, 0]
    check(y, y64, bound, "%d->%d seams, channels_first" % (orig, new))
    pairs = x.reshape(-1, 2, T)                                                # two impulses per item, interleaved
    y = run(pairs, orig, new, "channels_last")
    check(y.reshape(len(spots), -1), y64, bound, "%d->%d seams, channels_last" % (orig, new))
    kapre.check_device()


# ------------------------------------------------------------------ adjoint
@pytest.mark.parametrize("orig,new", PAIRS, ids=IDS)
def test_adjoint_parity_and_inner_products(orig, new):
    import torch
    import kapre_amd as kapre

    n_taps = plan(orig, new, True)[0]
    worst = 0.0
    lengths = (1, 5, 3 * n_taps + 7, three_tiles(orig, new, True))
    for T in lengths:
        x = signals("noise", BATCH * 3, T, seed=T + 1).reshape(BATCH, 3, T)
        T_out = rm.out_length(T, orig, new)
        for kind in ("speech", "noise"):
            gy = signals(kind, BATCH * 3, T_out, seed=T + 2).reshape(BATCH, 3, T_out)
            gx64, bound = dm.adjoint(gy, T, orig, new), dm.bound(gy, T, orig, new, adjoint=True)
            for fmt in ("channels_last", "channels_first"):
                layer = kapre.Resample(orig, new, data_format=fmt, method='direct')
                for C in (1, 2, 3):
                    xt = torch.from_numpy(to_layout(x[:, :C], fmt)).cuda().requires_grad_(True)
                    gt = torch.from_numpy(to_layout(gy[:, :C], fmt)).cuda()
                    y = layer(xt)
                    (y * gt).sum().backward()
                    gx = to_np(xt.grad)
                    assert gx.shape == xt.shape
                    label = "%d->%d adjoint T=%d %s %s C=%d" % (orig, new, T, kind, fmt, C)
                    worst = max(worst, check(from_layout(gx, fmt), gx64[:, :C], bound[:, :C], label))
                    y64_, g64_, x64_ = (to_np(v).astype(np.float64) for v in (y, gt, xt))
                    lhs, rhs = float(np.sum(y64_ * g64_)), float(np.sum(x64_ * gx.astype(np.float64)))
                    scale = max(float(np.sum(np.abs(y64_ * g64_))), float(np.sum(np.abs(x64_ * gx))))
                    print("resample direct %s: <y, gy> = %.9e, <x, gx> = %.9e, sum of |terms| %.3e" % (label, lhs, rhs, scale))
                    # A random cotangent's inner product is a sum that cancels -- to a hundredth of its terms' size at some lengths
                    # -- so at every length and for both kinds the two sides agree within 1e-5 of the sum of |terms|, which
                    # cancellation cannot excuse; within 1e-5 of the inner product itself where it sums tens of thousands of terms;
                    assert abs(lhs - rhs) <= 1e-5 * scale, (label, lhs, rhs, scale)
                    if T == lengths[-1] and kind == "noise":
                        assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (label, lhs, rhs)
                    if kind == "noise":
                        # and, at every length, within 1e-5 of the inner product for the cotangent gy = y: <y, y> cannot cancel
                        xs = xt.detach().clone().requires_grad_(True)
                        ys = layer(xs)
                        (ys * ys.detach()).sum().backward()
                        lhs = float(np.sum(to_np(ys).astype(np.float64) ** 2))
                        rhs = float(np.sum(x64_ * to_np(xs.grad).astype(np.float64)))
                        print("resample direct %s: <y, y> = %.9e, <x, R^T y> = %.9e" % (label, lhs, rhs))
                        assert lhs > 0 and abs(lhs - rhs) <= 1e-5 * lhs, (label, lhs, rhs)
    print("resample direct adjoint %d->%d: worst ratio %.3f" % (orig, new, worst))
    kapre.check_device()


def test_adjoint_of_a_free_length():
    import torch
    from kapre_amd import backend

    orig, new, T = 10079, 8000, 900
    for length in (300, rm.out_length(T, orig, new) + 200):
        x = torch.from_numpy(signals("noise", 2, T, 1).reshape(2, T, 1)).cuda().requires_grad_(True)
        gy = signals("noise", 2, length, 2).reshape(2, 1, length)
        y = backend.resample(x, orig, new, method='direct', length=length)
        assert y.shape == (2, length, 1) and y.grad_fn is not None
        (y * torch.from_numpy(to_layout(gy, "channels_last")).cuda()).sum().backward()
        check(from_layout(to_np(x.grad), "channels_last"), dm.adjoint(gy, T, orig, new), dm.bound(gy, T, orig, new, adjoint=True),
              "adjoint of length %d" % length)


# ------------------------------------------------------------------ the same bits
def test_same_bits_across_runs_channel_counts_layouts_and_batch_positions():
    import torch
    import kapre_amd as kapre
    from kapre_amd import backend

    orig, new = 25427, 24000
    T = three_tiles(orig, new, False)
    sig = signals("noise", 1, T, 11)[0]
    other = signals("noise", BATCH * 3, T, 12).reshape(BATCH, 3, T)
    ref = None
    for fmt in ("channels_last", "channels_first"):
        for C in (1, 2, 3):
            for pos in (0, 2):
                x = other[:, :C].copy()
                x[pos, 0] = sig
                xt = torch.from_numpy(to_layout(x, fmt)).cuda()
                a = backend.resample(xt, orig, new, data_format=fmt, method='direct')
                b = backend.resample(xt, orig, new, data_format=fmt, method='direct')
                assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
                got = from_layout(to_np(a), fmt)[pos, 0]
                if ref is None:
                    ref = got
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (fmt, C, pos)
                xg = xt.clone().requires_grad_(True)
                g = torch.from_numpy(to_layout(other[:, :C, :a.shape[1 if fmt == "channels_last" else 2]], fmt)).cuda()
                (g1,) = torch.autograd.grad(backend.resample(xg, orig, new, data_format=fmt, method='direct'), xg, g)
                (g2,) = torch.autograd.grad(backend.resample(xg, orig, new, data_format=fmt, method='direct'), xg, g)
                assert torch.equal(g1, g2)
    kapre.check_device()


def test_nan_stays_inside_its_support():
    import kapre_amd as kapre

    for orig, new in ((25427, 24000), (44100, 16000), (1, 2)):
        T = three_tiles(orig, new, False)
        n_out = rm.out_length(T, orig, new)
        x = signals("noise", 4, T, 21).reshape(2, 2, T)
        j0 = plan(orig, new, False)[1] * dm.shape(orig, new)[1] // dm.shape(orig, new)[0] + 3     # next to a tile seam
        bad = x.copy()
        bad[1, 0, j0] = np.nan
        lo, hi = dm.support_range(n_out, orig, new)
        far = (j0 < lo - 1) | (j0 > hi + 1)                           # more than one position outside the support
        near = (j0 >= lo) & (j0 <= hi)
        assert far.sum() > n_out - 200 and near.sum() >= 1
        for fmt in ("channels_last", "channels_first"):
            clean, dirty = run(x, orig, new, fmt), run(bad, orig, new, fmt)
            assert np.array_equal(clean[0].view(np.uint32), dirty[0].view(np.uint32))
            assert np.array_equal(clean[1, 1].view(np.uint32), dirty[1, 1].view(np.uint32))
            assert np.array_equal(clean[1, 0, far].view(np.uint32), dirty[1, 0, far].view(np.uint32))
            assert np.isnan(dirty[1, 0, near]).all()
    kapre.check_device()


# ------------------------------------------------------------------ beside the table kernel
@pytest.mark.parametrize("orig,new", [(44100, 16000), (55, 49)])
def test_against_the_table_kernel(orig, new):
    """method='direct' and method='polyphase' differ by at most the sum of their two bounds"""
    import kapre_amd as kapre
    from kapre_amd import _ffi, backend

    T = three_tiles(orig, new, False)
    n_out = rm.out_length(T, orig, new)
    table_taps = _ffi.resample_table_size(orig, new, 6, 0.99, False)[1]
    for kind in ("speech", "noise"):
        x = signals(kind, BATCH * 2, T, 31).reshape(BATCH, 2, T)
        both = dm.bound(x, n_out, orig, new) + (table_taps + 3) * 2.0 ** -24 * rm.abs_budget(x, orig, new) + 1e-37
        for fmt in ("channels_last", "channels_first"):
            xt = to_layout(x, fmt)
            d = from_layout(to_np(backend.resample(xt, orig, new, data_format=fmt, method='direct')), fmt).astype(np.float64)
            p = from_layout(to_np(backend.resample(xt, orig, new, data_format=fmt, method='polyphase')), fmt).astype(np.float64)
            worst = float(np.max(np.abs(d - p) / both))
            print("direct against table %d->%d %s %s: worst |d - p| / (sum of bounds) = %.3f" % (orig, new, kind, fmt, worst))
            assert worst <= 1.0
    kapre.check_device()


# ------------------------------------------------------------------ launches
def test_launches_and_what_launches_nothing():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, backend

    x = torch.zeros((2, 64, 1), device="cuda")
    params = (50854, 48000, 6, 0.99)
    assert _ffi.resample_direct(x[:0], "channels_last", params, False, 9).shape == (0, 9, 1)       # an empty call: the log restarts
    assert _ffi.last_launches() == ""
    assert _ffi.resample_direct(x, "channels_last", params, False, 0).shape == (2, 0, 1) and _ffi.last_launches() == ""
    assert backend.resample(x, 16000, 16000, method='direct') is x and backend.resample(x, 5, 5, method='direct', length=64) is x
    assert _ffi.last_launches() == ""
    y = backend.resample(x, 5, 5, method='direct', length=80)                 # equal rates, another length: the low-pass itself
    assert y.shape == (2, 80, 1) and _ffi.last_launches() == "k_resample_direct<1>"
    layer = kapre.Resample(50854, 48000, method='direct')
    y = layer(x)
    assert y.grad_fn is None and _ffi.last_launches() == "k_resample_direct<1>"
    layer(torch.zeros((2, 64, 2), device="cuda"))
    assert _ffi.last_launches() == "k_resample_direct<2>"
    layer(torch.zeros((2, 64, 3), device="cuda"))
    assert _ffi.last_launches() == "k_resample_direct<1>"
    xg = x.clone().requires_grad_(True)
    y = layer(xg)
    assert y.grad_fn is not None and _ffi.last_launches() == "k_resample_direct<1>"
    y.sum().backward()
    assert _ffi.last_launches() == "k_resample_direct<1>" and xg.grad.shape == x.shape
    kapre.check_device()
