"""kpr_cqt_f32 / kapre_amd.CQT on the GPU against the float64 model of tests/cqt_model.py.

Every element: |dRe|, |dIm| <= (N_k + 4) 2^-24 sum |x| |w_k|; magnitudes: the modulus of that plus 3 * 2^-24 |C|.
The worst ratio is printed per case; measured on an MI355X: at most 0.130 (bank 1000/60/9/3, hop 32), 0.066 in four chunks."""
import numpy as np
import pytest

import cqt_model
from kapre_amd import _ffi, backend

pytestmark = pytest.mark.gpu

BANKS = [(1000, 50, 20, 6), (1000, 60, 9, 3), (1000, 60, 1, 3)]          # L = 164: tiles of 8 + 8 + 4; L = 65: 8 + 1; one bin
HOPS = [32, 20, 7, "L+3"]                                                # padded banks, 16-byte reads unpadded, scalar, no overlap
# (input format, channels, output format, center, pad_end)
LAYOUTS = [("channels_last", 3, "channels_last", False, False), ("channels_first", 2, "channels_first", True, False),
           ("channels_last", 1, "channels_first", False, True)]


def bank_of(args):
    lengths, _, kernels = backend.cqt_kernels(*args)
    return lengths, kernels, _ffi.cqt_pack(lengths, kernels)


def run(x, fmt, out_fmt, lengths, table, hop, center, pad_end, magnitude):
    """x (b, c, n) -> (b, c, frames, K) as numpy, and the launch label"""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 1, 2) if fmt == "channels_last" else x)).cuda()
    out = _ffi.cqt(xt, fmt, out_fmt, lengths, torch.from_numpy(table).cuda(), hop, center, pad_end, magnitude)
    label = _ffi.last_launches()
    out = out.cpu().numpy()
    return (np.moveaxis(out, 3, 1) if out_fmt == "channels_last" else out), label


def check(x, lengths, kernels, table, hop, fmt, out_fmt, center, pad_end):
    """both outputs of every series against the model -> worst error / bound"""
    worst = 0.0
    got, label = run(x, fmt, out_fmt, lengths, table, hop, center, pad_end, False)
    mag, mlabel = run(x, fmt, out_fmt, lengths, table, hop, center, pad_end, True)
    assert label.startswith("k_cqt<v") and label.endswith(",cplx>") and mlabel == label.replace("cplx", "mag"), (label, mlabel)
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            C, bound = cqt_model.cqt(x[b, c], lengths, kernels, hop, center, pad_end)
            assert got[b, c].shape == C.shape == mag[b, c].shape
            m64, mbound = cqt_model.magnitude_bound(C, bound)
            for err, bnd in ((np.abs(got[b, c].real - C.real), bound), (np.abs(got[b, c].imag - C.imag), bound),
                             (np.abs(mag[b, c] - m64), mbound)):
                assert (err <= bnd).all(), (b, c, float((err / np.maximum(bnd, 1e-300)).max()))
                worst = max(worst, float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0)
    return worst


def length_for(frames, L, hop, center, pad_end):
    """a signal length that is no multiple of the hop and gives ``frames`` frames"""
    n = (frames - 1) * hop + (hop // 2 if center else hop // 2 + 1 if pad_end else L + hop // 2)
    assert cqt_model.frame_count(n, L, hop, center, pad_end) == frames
    return n


@pytest.mark.parametrize("fmt,ch,out_fmt,center,pad_end", LAYOUTS)
@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("bank", BANKS)
def test_against_the_model(bank, hop, fmt, ch, out_fmt, center, pad_end):
    lengths, kernels, table = bank_of(bank)
    L = int(lengths[0])
    hop = L + 3 if hop == "L+3" else hop
    F = _ffi.cqt_plan(lengths, hop)[0]
    rng = np.random.default_rng(L + hop)
    worst = 0.0
    for frames in sorted({1, F - 1, F, F + 1, 2 * F + 1}):
        x = rng.standard_normal((2, ch, length_for(frames, L, hop, center, pad_end))).astype(np.float32)
        worst = max(worst, check(x, lengths, kernels, table, hop, fmt, out_fmt, center, pad_end))
    print("worst error / bound %s hop %d: %.4f" % (bank, hop, worst))


@pytest.mark.parametrize("hop", [32, 7, 167])
def test_chunked_reduction(hop):
    """cqt_chunk 48 on L = 164: four pieces for the first tile, the accumulators kept across them"""
    lengths, kernels, table = bank_of(BANKS[0])
    old = _ffi.set_option("cqt_chunk", 48)
    try:
        F, chunk, _ = _ffi.cqt_plan(lengths, hop)
        assert chunk == 48 and -(-176 // chunk) >= 3
        x = np.random.default_rng(hop).standard_normal((2, 2, length_for(F + 3, 164, hop, False, False))).astype(np.float32)
        worst = check(x, lengths, kernels, table, hop, "channels_first", "channels_last", False, False)
    finally:
        _ffi.set_option("cqt_chunk", old)
    print("worst error / bound, chunked, hop %d: %.4f" % (hop, worst))


def test_non_finite_samples_stay_in_their_frames_and_runs_repeat():
    lengths, kernels, table = bank_of(BANKS[0])
    offsets = (164 - lengths) // 2
    x = np.random.default_rng(5).standard_normal((1, 2, 164 + 20 * 70 + 9)).astype(np.float32)
    args = ("channels_first", "channels_first", lengths, table, 20, False, False)
    clean, again = run(x, *args, False)[0], run(x, *args, False)[0]
    assert np.array_equal(clean.view(np.float32), again.view(np.float32))
    bad = x.copy()
    bad[0, 0, 777], bad[0, 1, 1030] = np.nan, np.inf
    got = run(bad, *args, False)[0]
    for c, p in ((0, 777), (1, 1030)):
        for t in range(clean.shape[2]):
            if not t * 20 <= p < t * 20 + 164:
                assert np.array_equal(got[0, c, t].view(np.float32), clean[0, c, t].view(np.float32)), (c, t)
            else:
                inside = (t * 20 + offsets <= p) & (p < t * 20 + offsets + lengths)
                assert inside.any() and not np.isfinite(got[0, c, t][inside]).any(), (c, t)


def test_no_frames():
    lengths, kernels, table = bank_of(BANKS[1])
    out, label = run(np.zeros((2, 3, 64), np.float32), "channels_last", "channels_last", lengths, table, 7, False, False, True)
    assert out.shape == (2, 3, 0, 9) and label == ""


def test_layer_end_to_end():
    """a unit 440 Hz sine through the default bank: bin 45 (A4) carries 0.5 sqrt(N_45) = 14.5172 (float64: 14.5171 ... 14.5173)"""
    import torch
    import kapre_amd as kapre
    n = 11339 + 4 * 512
    x = np.sin(2 * np.pi * 440.0 * np.arange(n) / 22050.0).astype(np.float32).reshape(1, n, 1)
    out = kapre.Sequential([kapre.CQT(22050, output="magnitude", input_shape=(n, 1))])(x)
    assert tuple(out.shape) == (1, 5, 84, 1) and out.dtype == torch.float32
    s = out[0, :, :, 0].cpu().numpy()
    assert (s.argmax(axis=1) == 45).all() and (np.abs(s[:, 45] - 14.5172) < 1e-3).all()
    assert (s[:, 43] < 0.04 * s[:, 45]).all() and (s[:, 47] < 0.04 * s[:, 45]).all()
    xt = torch.from_numpy(x).cuda().requires_grad_(True)                  # behind Resample and LFilter; complex into Magnitude
    chain = kapre.Sequential([kapre.Resample(22050, 16000, input_shape=(n, 1)), kapre.Preemphasis(0.97),
                              kapre.CQT(16000, hop_length=160, n_bins=72), kapre.Magnitude()])
    y = chain(xt)
    resampled = chain.layers[0].compute_output_shape((1, n, 1))[1]
    assert tuple(y.shape) == (1, 1 + (resampled - chain.layers[2].frame_length) // 160, 72, 1) == (1,) + chain.output_shape[1:]
    assert y.grad_fn is None and bool(torch.isfinite(y).all())
