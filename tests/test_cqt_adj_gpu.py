"""kpr_cqt_adjoint_f32 / CQT(differentiable=True) on the GPU against the float64 model of tests/cqt_adj_model.py.

Every sample: |gx - gx64| <= (M_s + 4) 2^-24 sum |g| |w| (no addition behind the accumulation chain, c = 0); a sample
that no kernel covers is +0.0 bit for bit.  The worst ratio is printed per case; measured on an MI355X: at most 0.367 (bank
1000/50/20/6, hop 167), 0.233 in three chunks, 0.212 in twelve, 0.280 through autograd."""
import numpy as np
import pytest

import cqt_adj_model
import cqt_model
from kapre_amd import _ffi, backend

pytestmark = pytest.mark.gpu

BANKS = [(1000, 50, 20, 6), (1000, 60, 9, 3), (1000, 60, 1, 3)]          # L = 164: tiles of 8 + 8 + 4; L = 65: 8 + 1; one bin
# (waveform format, channels, spectrogram format, center, pad_end): the rows of test_cqt_gpu.py
LAYOUTS = [("channels_last", 3, "channels_last", False, False), ("channels_first", 2, "channels_first", True, False),
           ("channels_last", 1, "channels_first", False, True)]


def bank_of(args, hop):
    lengths, _, kernels = backend.cqt_kernels(*args)
    return lengths, kernels, _ffi.cqt_pack_adjoint(lengths, kernels, hop)


def run(G, time, fmt, g_fmt, lengths, table, hop, center, pad_end):
    """G (b, c, frames, K) complex -> gx (b, c, time) as numpy, and the launch label"""
    import torch
    g = torch.from_numpy(np.ascontiguousarray(np.moveaxis(G, 1, 3) if g_fmt == "channels_last" else G)).cuda()
    out = _ffi.cqt_adjoint(g, g_fmt, fmt, time, lengths, torch.from_numpy(table).cuda(), hop, center, pad_end)
    label = _ffi.last_launches()
    out = out.cpu().numpy()
    return (np.moveaxis(out, 2, 1) if fmt == "channels_last" else out), label


def within_bound(got, G, time, lengths, kernels, hop, center):
    """every series of got (b, c, time) against the model -> worst error / bound"""
    worst = 0.0
    for b in range(G.shape[0]):
        for c in range(G.shape[1]):
            gx, bound, covered = cqt_adj_model.cqt_adjoint(G[b, c], time, lengths, kernels, hop, center)
            err = np.abs(got[b, c] - gx)
            assert (err <= bound).all(), (b, c, float((err / np.maximum(bound, 1e-300)).max()))
            assert (got[b, c][~covered].view(np.uint32) == 0).all(), (b, c)
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    return worst


def case(rng, blocks, ch, lengths, hop, center, pad_end):
    """(cotangent (2, ch, frames, K), time): a signal of ``blocks`` hop blocks whose length is no multiple of the hop (>= 7)"""
    L = int(lengths[0])
    time = (blocks - 1) * hop + hop // 2 + 1 - (L // 2 if center else 0)
    time += time % hop == 0
    if time <= 0:                                                         # centred: the first blocks lie in front of the signal
        return None, time
    shape = (2, ch, cqt_model.frame_count(time, L, hop, center, pad_end), len(lengths))
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64), time


@pytest.mark.parametrize("fmt,ch,g_fmt,center,pad_end", LAYOUTS)
@pytest.mark.parametrize("hop", [32, 20, 7, "L+3"])
@pytest.mark.parametrize("bank", BANKS)
def test_against_the_model(bank, hop, fmt, ch, g_fmt, center, pad_end):
    L = int(backend.cqt_kernels(*bank)[0][0])
    hop = L + 3 if hop == "L+3" else hop
    lengths, kernels, table = bank_of(bank, hop)
    F = _ffi.cqt_adjoint_plan(lengths, hop)[0]
    rng, worst = np.random.default_rng(L + hop), 0.0
    for blocks in sorted({1, F - 1, F, F + 1, 2 * F + 1}):
        G, time = case(rng, blocks, ch, lengths, hop, center, pad_end)
        if G is not None:
            got, label = run(G, time, fmt, g_fmt, lengths, table, hop, center, pad_end)
            assert label.startswith("k_cqt_adj<g") and "+" not in label, label
            worst = max(worst, within_bound(got, G, time, lengths, kernels, hop, center))
    print("worst error / bound %s hop %d: %.4f" % (bank, hop, worst))


@pytest.mark.parametrize("hop", [32, 7, 167])
def test_chunked_reduction(hop):
    """cqt_adjoint_rows = a run + 1 on L = 164: two d per chunk, three chunks at hop 32, twelve at hop 7, the accumulators
    kept across them (hop 167 > L has one d, so one chunk: that case pins the option on a plan it cannot split)"""
    lengths, kernels, table = bank_of(BANKS[0], hop)
    D = -(-164 // hop)
    old = _ffi.set_option("cqt_adjoint_rows", 65)
    try:
        F, rows, _ = _ffi.cqt_adjoint_plan(lengths, hop)
        assert (F, rows) == (64, 64 + min(D, 2) - 1) and -(-D // (rows - F + 1)) == {32: 3, 7: 12, 167: 1}[hop]
        G, time = case(np.random.default_rng(hop), F + 3, 2, lengths, hop, False, False)
        got, _ = run(G, time, "channels_first", "channels_last", lengths, table, hop, False, False)
        worst = within_bound(got, G, time, lengths, kernels, hop, False)
    finally:
        _ffi.set_option("cqt_adjoint_rows", old)
    print("worst error / bound, chunked, hop %d: %.4f" % (hop, worst))


def test_runs_repeat_and_a_nan_stays_in_its_reach():
    hop, L = 20, 164
    lengths, kernels, table = bank_of(BANKS[0], hop)
    G, time = case(np.random.default_rng(5), 80, 2, lengths, hop, False, False)
    args = (time, "channels_first", "channels_first", lengths, table, hop, False, False)
    clean, again = run(G, *args)[0], run(G, *args)[0]
    assert np.array_equal(clean.view(np.uint32), again.view(np.uint32))
    bad = G.copy()
    bad[0, 0, 33, 2], bad[0, 1, 50, 19] = np.nan, np.nan
    got, s = run(bad, *args)[0], np.arange(time)
    for c, t in ((0, 33), (1, 50)):
        outside = (s < t * hop - 15) | (s >= t * hop + L + 15)
        assert np.array_equal(got[0, c][outside].view(np.uint32), clean[0, c][outside].view(np.uint32)), c
        assert np.isnan(got[0, c][t * hop + 70:t * hop + 90]).all()       # the middle of every kernel of the bank


def test_layer_through_autograd_behind_preemphasis_and_the_magnitude_route():
    """l = sum(a Re y + b Im y): the cotangent is exactly a + i b, so x.grad is held to the kernel's own bound.  Behind Preemphasis
    the gradient reaches the waveform: Preemphasis' backward of the adjoint's output.  output='magnitude' is bit for bit the
    complex layer followed by Magnitude, in value and in x.grad; the default layer still detaches."""
    import torch
    import kapre_amd as kapre
    rng, time = np.random.default_rng(11), 164 + 20 * 66 + 9
    lengths, _, kernels = backend.cqt_kernels(*BANKS[0])
    x = rng.standard_normal((2, time, 2)).astype(np.float32)
    a, b = (rng.standard_normal((2, cqt_model.frame_count(time, 164, 20, False, False), 20, 2)).astype(np.float32) for _ in range(2))
    at, bt = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    leaf = lambda v: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v.detach()).requires_grad_(True)
    loss = lambda y: (at * y.real + bt * y.imag).sum()
    args = dict(sample_rate=1000, hop_length=20, fmin=50, n_bins=20, bins_per_octave=6)
    layer, pre = kapre.CQT(differentiable=True, **args), kapre.Preemphasis(0.97)
    x1 = leaf(x)
    y = layer(x1)
    assert y.grad_fn is not None and y.dtype == torch.complex64
    loss(y).backward()
    G = np.moveaxis(a + 1j * b, 3, 1)                                     # (b, c, frames, K)
    print("worst error / bound through autograd: %.4f"
          % within_bound(np.moveaxis(x1.grad.cpu().numpy(), 2, 1), G, time, lengths, kernels, 20, False))
    with torch.no_grad():                                                 # nothing to carry: the forward launch alone
        assert layer(x1).grad_fn is None and _ffi.last_launches().startswith("k_cqt<")
    x2, x3 = leaf(x), leaf(x)
    loss(kapre.Sequential([pre, layer])(x2)).backward()
    mid = leaf(pre(torch.from_numpy(x).cuda()))
    loss(layer(mid)).backward()
    pre(x3).backward(mid.grad)
    assert bool((x2.grad != 0).any()) and torch.equal(x2.grad, x3.grad)
    x4, x5 = leaf(x), leaf(x)
    y4 = kapre.CQT(output="magnitude", differentiable=True, **args)(x4)
    y5 = kapre.Sequential([kapre.CQT(differentiable=True, **args), kapre.Magnitude()])(x5)
    assert y4.grad_fn is not None and y4.dtype == torch.float32 and torch.equal(y4, y5)
    (at * y4).sum().backward()
    (at * y5).sum().backward()
    assert torch.equal(x4.grad, x5.grad) and bool((x4.grad != 0).any())
    assert kapre.CQT(output="magnitude", **args)(x4).grad_fn is None     # the default layer detaches, as before
