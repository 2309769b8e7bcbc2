"""TimeStretch on the GPU (kapre_amd.TimeStretch / backend.phase_vocoder, kpr_time_stretch_c64) against the float64 models of
tests/time_stretch_model.py.

 1. the angle words: at rate 1 phase_out[t] is Theta(X[t]), within e_Theta = 6 * 2^-24 |theta| / pi + 2^-31 half turns of the
    float64 angle on every bin (6 ulp: OpenCL's limit for atan2, a figure of the specification), zeros of all four sign
    combinations and the +-pi axis included;
 2. the scan is exact: at every other rate phase_out equals phase_words(Theta_device, idx) bit for bit -- a wrong carry across a
    wave or super-block boundary is a hard mismatch;
 3. the output within the first-order bound of the model on every bin (time_stretch_model.bound);
 4. rate 1 returns the input within that bound;
 5. the same bits: twice, across layouts, 16-byte against 8-byte accesses, another stream, with and without phase_out;
 6. a NaN / Inf bin touches only the frames that read it;
 7. the refusals of the C entry point;
 8. STFT -> TimeStretch -> InverseSTFT end to end.
Every check prints its figures.

Measured on an MI355X (profiles/time_stretch_times.md): the angle words use at most 0.994 of e_Theta -- that close
only for angles so small that the budget is the word's own rounding, 2^-31; for |theta| >= 2^-6 half turns at most 4.74 of the
6 * 2^-24 |theta| / pi --, the outputs at most 0.38 of the bound (0.35 at rate 1, 0.31 through the layer)."""
import ctypes

import numpy as np
import pytest

import time_stretch_model as tsm

pytestmark = pytest.mark.gpu

RATES = [0.5, 0.75, 1.0, 1.25, 2.0, 3.7]
FRAMES_OUT = {"1": lambda r, w: 1, "2": lambda r, w: 2, "R": lambda r, w: r, "R+1": lambda r, w: r + 1, "WR-1": lambda r, w: w * r - 1,
              "WR": lambda r, w: w * r, "WR+1": lambda r, w: w * r + 1, "2WR+1": lambda r, w: 2 * w * r + 1,
              "3WR+5": lambda r, w: 3 * w * r + 5}
INNER = [1, 3, 4, 5, 129, 130]


def plan():
    from kapre_amd import _ffi
    return _ffi.time_stretch_plan(1, 1)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def frames_in_for(frames_out, rate):
    """the smallest number of input frames that gives ``frames_out`` output frames at ``rate`` (None: there is none)"""
    from kapre_amd import backend
    lo = max(int(frames_out * rate) - 3, 1)
    for f in range(lo, lo + 8):
        if backend.time_stretch_length(f, rate) == frames_out:
            return f
    return None


def pairs_for(frames_out):
    got = [(rate, frames_in_for(frames_out, rate)) for rate in RATES]
    return [(rate, f) for rate, f in got if f is not None]


SPECIAL = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (-2.0, 0.0), (-2.0, -0.0), (3.0, 0.0), (0.0, 1.5), (0.0, -1.5),
           (-1e-3, 1e-12), (-1e-3, -1e-12), (1e-12, 1e-3)]


def spectrum(outer, frames, inner, seed):
    """(outer, frames, inner) complex64: normal bins of mixed scale with the special angles planted"""
    rng = np.random.default_rng(seed)
    X = tsm.random_spectrum((outer, frames, inner), seed) * np.exp(rng.uniform(-3, 3, (outer, frames, inner))).astype(np.float32)
    flat = X.reshape(outer, -1).view(np.float32).reshape(outer, -1, 2)
    for j, (re, im) in enumerate(SPECIAL):
        flat[:, (5 * j + 1) % flat.shape[1]] = (re, im)
    return X


def run(x4, fmt, rate, want_phase=True):
    """the kernel on the rank-4 device tensor ``x4``: (out, phase words as uint32) as numpy, and the tables"""
    from kapre_amd import _ffi, backend
    frames = _ffi.dims_of(x4.shape, fmt)[2]
    idx, alpha = backend.time_stretch_table(frames, rate)
    res = _ffi.time_stretch(x4, fmt, dev(idx), dev(alpha), len(idx), want_phase=want_phase)
    if not want_phase:
        return res.cpu().numpy(), None, idx, alpha
    return res[0].cpu().numpy(), res[1].cpu().numpy().view(np.uint32), idx, alpha


def time_first(a):
    """(outer, frames, inner) -> (frames, outer, inner): the models scan axis 0"""
    return np.moveaxis(a, 1, 0)


def share(err, bound):
    return float(np.max(err / bound)) if err.size else 0.0


# ---- 1. - 4. ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FRAMES_OUT))
def test_words_scan_and_output(name):
    R, W = plan()
    frames_out = FRAMES_OUT[name](R, W)
    pairs = pairs_for(frames_out)
    assert len(pairs) >= 2 and any(rate == 1.0 for rate, _ in pairs), pairs
    worst_angle = worst_out = worst_id = worst_ulps = 0.0
    for case, (outer, inner) in enumerate((o, i) for o in (1, 3) for i in INNER):
        for rate, frames_in in pairs:
            X = spectrum(outer, frames_in, inner, seed=1000 * frames_out + 10 * case + int(rate * 4))
            x4 = dev(X.reshape(outer, 1, frames_in, inner))                              # channels_first, one channel per item
            # the angle words of this input: the rate-1 run
            y1, th, idx1, alpha1 = run(x4, "channels_first", 1.0)
            th = time_first(th.reshape(outer, frames_in, inner))
            Xt = time_first(X)
            got = tsm.words_to_half_turns(th)
            d = got - tsm.half_turns(Xt)
            d = np.abs(d - 2.0 * np.round(d / 2.0))
            worst_angle = max(worst_angle, share(d, tsm.angle_bound(Xt)))
            assert (d <= tsm.angle_bound(Xt)).all()
            ht = np.abs(tsm.half_turns(Xt))
            far = ht >= 2.0 ** -6                                   # where the arc tangent's term is the budget, not the rounding
            worst_ulps = max(worst_ulps, share(d[far], tsm.U * ht[far]))
            assert (th[Xt == 0] == 0).all()
            # identity, independent of the model
            b1, _ = tsm.bound(Xt, idx1, alpha1)
            e1 = np.abs(time_first(y1.reshape(outer, frames_in, inner)).astype(np.complex128) - Xt.astype(np.complex128))
            worst_id = max(worst_id, share(e1[b1 > 0], b1[b1 > 0]))
            assert (e1 <= b1).all()
            if rate == 1.0:
                assert frames_in == frames_out
                continue
            y, P, idx, alpha = run(x4, "channels_first", rate)
            assert len(idx) == frames_out and y.shape == (outer, 1, frames_out, inner)
            P = time_first(P.reshape(outer, frames_out, inner))
            want = tsm.phase_words(th, idx)
            assert np.array_equal(P, want), "phase words differ at %s" % (np.argwhere(P != want)[:4].tolist(),)
            model = tsm.definition(Xt, idx, alpha, words=False)
            b, _ = tsm.bound(Xt, idx, alpha)
            e = np.abs(time_first(y.reshape(outer, frames_out, inner)).astype(np.complex128) - model)
            worst_out = max(worst_out, share(e[b > 0], b[b > 0]))
            assert (e <= b).all(), (rate, outer, inner, float(np.max(e / np.maximum(b, 1e-300))))
    print("frames_out %s = %d, rates %s: angle words use %.3f of e_Theta (%.2f of the 6 x 2^-24 |theta| / pi away from 0), outputs "
          "%.3f of the bound, identity %.3f" % (name, frames_out, [r for r, _ in pairs], worst_angle, worst_ulps, worst_out, worst_id))


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("fmt", ["channels_last", "channels_first"])
def test_layouts_through_the_layer(fmt, ch):
    """both layouts with 1, 2 and 3 channels through the public layer: the output within the bound, and one layout the
    transpose of the other bit for bit"""
    import kapre_amd as kapre
    from kapre_amd import backend
    R, W = plan()
    frames, freq, batch = W * R + 3, 65, 2
    X = spectrum(batch * ch, frames, freq, seed=77).reshape(batch, ch, frames, freq)                # channels_first
    for rate in (0.75, 1.25):
        first = kapre.TimeStretch(rate, data_format="channels_first")(dev(X)).cpu().numpy()
        if fmt == "channels_last":
            got = kapre.TimeStretch(rate, data_format=fmt)(dev(np.transpose(X, (0, 2, 3, 1)))).cpu().numpy()
            assert got.shape == (batch, first.shape[2], freq, ch)
            assert np.array_equal(np.ascontiguousarray(np.transpose(got, (0, 3, 1, 2))).view(np.int32), first.view(np.int32))
            also = backend.phase_vocoder(np.transpose(X, (0, 2, 3, 1)), rate, data_format=fmt).cpu().numpy()
            assert np.array_equal(also.view(np.int32), got.view(np.int32))
        idx, alpha = backend.time_stretch_table(frames, rate)
        Xt = time_first(X.reshape(batch * ch, frames, freq))
        model = tsm.definition(Xt, idx, alpha, words=False)
        b, _ = tsm.bound(Xt, idx, alpha)
        e = np.abs(time_first(first.reshape(batch * ch, len(idx), freq)).astype(np.complex128) - model)
        print("%s, %d channel(s), rate %g: %.3f of the bound" % (fmt, ch, rate, share(e[b > 0], b[b > 0])))
        assert (e <= b).all()


# ---- 5. the same bits ------------------------------------------------------------------------------------------------------
def test_same_bits():
    import torch
    from kapre_amd import _ffi
    R, W = plan()
    frames, outer, inner = 2 * W * R + 1, 3, 130
    X = spectrum(outer, frames, inner, seed=5)
    x4 = dev(X.reshape(outer, 1, frames, inner))
    for rate in (0.75, 2.0):
        y, P, idx, alpha = run(x4, "channels_first", rate)
        assert "k_time_stretch<2>" in _ffi.last_launches()
        y2, P2, _, _ = run(x4, "channels_first", rate)
        assert np.array_equal(y.view(np.int32), y2.view(np.int32)) and np.array_equal(P, P2)
        # without phase_out
        y3, _, _, _ = run(x4, "channels_first", rate, want_phase=False)
        assert np.array_equal(y.view(np.int32), y3.view(np.int32))
        # the 8-byte path: the same data at a base offset by 8 bytes
        buf = torch.empty(X.size + 1, dtype=torch.complex64, device="cuda")
        view = buf[1:].view(outer, 1, frames, inner)
        view.copy_(x4)
        assert view.data_ptr() % 16 == 8
        y4, P4, _, _ = run(view, "channels_first", rate)
        assert "k_time_stretch<1>" in _ffi.last_launches()
        assert np.array_equal(y.view(np.int32), y4.view(np.int32)) and np.array_equal(P, P4)
        # a stream of its own
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            y5, P5, _, _ = run(x4, "channels_first", rate)
        s.synchronize()
        assert np.array_equal(y.view(np.int32), y5.view(np.int32)) and np.array_equal(P, P5)


# ---- 6. non-finite bins -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.75, 1.0, 2.0])
def test_a_nonfinite_bin_stays_in_the_frames_that_read_it(rate):
    R, W = plan()
    frames, outer, inner = W * R + 5, 2, 6
    X = spectrum(outer, frames, inner, seed=9)
    spots = [(0, 2 * R, 1, complex(np.nan, 1.0)), (1, 3 * R + 2, 4, complex(np.inf, -2.0)), (1, 0, 2, complex(1.0, -np.inf))]
    bad, zeroed = X.copy(), X.copy()
    for o, r, c, v in spots:
        bad[o, r, c] = v
        zeroed[o, r, c] = 0.0
    yb, Pb, idx, _ = run(dev(bad.reshape(outer, 1, frames, inner)), "channels_first", rate)
    yz, Pz, _, _ = run(dev(zeroed.reshape(outer, 1, frames, inner)), "channels_first", rate)
    yb, yz = yb.reshape(outer, len(idx), inner), yz.reshape(outer, len(idx), inner)
    assert np.array_equal(Pb, Pz)                                              # a non-finite bin has the angle word 0
    reads = np.zeros(yb.shape, bool)
    for o, r, c, _ in spots:
        reads[o, :, c] |= (idx == r) | (idx + 1 == r)
    assert reads.sum() >= len(spots)
    finite = np.isfinite(yb.real) & np.isfinite(yb.imag)
    assert not finite[reads].any() and finite[~reads].all()
    assert np.array_equal(yb.view(np.int32).reshape(outer, len(idx), inner, 2)[~reads],
                          yz.view(np.int32).reshape(outer, len(idx), inner, 2)[~reads])
    assert np.isfinite(yz.real).all() and np.isfinite(yz.imag).all()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from kapre_amd import _ffi
    L = _ffi.lib()
    outer, f_in, f_out, inner = 2, 10, 20, 8
    buf = torch.zeros(outer * (f_in + f_out) * inner + 64, dtype=torch.complex64, device="cuda")
    idx = torch.zeros(f_out, dtype=torch.int32, device="cuda")
    alpha = torch.zeros(f_out, dtype=torch.float32, device="cuda")
    stream = _ffi.current_stream_ptr()
    p = buf.data_ptr()
    call = lambda x, out, fi=f_in, fo=f_out, o=outer, i=inner, ph=None: L.kpr_time_stretch_c64(
        ctypes.c_void_p(x), o, fi, fo, i, ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(alpha.data_ptr()), ctypes.c_void_p(out),
        ctypes.c_void_p(ph) if ph else None, stream)
    n_in = outer * f_in * inner * 8
    assert call(p, p + n_in) == 0                                              # side by side
    assert call(p, p) == -1 and b"overlap" in L.kpr_last_error()
    assert call(p, p + n_in - 8) == -1 and call(p + 16, p) == -1
    assert call(p, p + n_in, ph=p + 8) == -1 and b"phase_out" in L.kpr_last_error()
    assert call(p, p + n_in + 4) == -1 and b"aligned" in L.kpr_last_error()
    assert call(0, p) == -1
    assert L.kpr_time_stretch_c64(ctypes.c_void_p(p), outer, f_in, f_out, inner, None, None, ctypes.c_void_p(p + n_in), None, stream) == -1
    assert call(p, p + n_in, fi=2 ** 27, i=8) == -2 and b"2^30" in L.kpr_last_error()
    assert call(p, p + n_in, fo=2 ** 27, i=8) == -2
    for kw in (dict(o=0), dict(fo=0), dict(i=0)):
        assert call(p, p, **kw) == 0 and _ffi.last_launches() == ""            # nothing is launched
    torch.cuda.synchronize()
    import kapre_amd as kapre
    empty = kapre.TimeStretch(0.5)(torch.zeros((2, 0, 5, 1), dtype=torch.complex64, device="cuda"))
    assert tuple(empty.shape) == (2, 0, 5, 1) and empty.dtype == torch.complex64


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------
def test_end_to_end_keeps_the_pitch():
    import torch
    import kapre_amd as kapre
    sr, n_fft, hop, k = 16000, 512, 128, 32
    f0 = k * sr / n_fft                                                        # a bin centre: 1000 Hz
    x = np.sin(2 * np.pi * f0 * np.arange(sr) / sr).astype(np.float32).reshape(1, sr, 1)
    model = kapre.get_time_stretch_layer(0.5, n_fft=n_fft, hop_length=hop, input_shape=(sr, 1))
    xt = dev(x).requires_grad_(True)
    y = model(xt)
    frames = 1 + (sr - n_fft) // hop
    want_len = (2 * frames - 1) * hop + n_fft
    assert tuple(y.shape) == (1, want_len, 1) == (1,) + tuple(model.output_shape[1:])
    assert y.grad_fn is None and not y.requires_grad
    spec = kapre.STFT(n_fft=n_fft, hop_length=hop)(x)
    z = kapre.TimeStretch(0.5)(spec.detach().clone().requires_grad_(True))
    assert z.grad_fn is None and not z.requires_grad and z.shape[1] == 2 * frames
    yn = y.detach().cpu().numpy()[0, :, 0].astype(np.float64)
    assert np.isfinite(yn).all()
    mid = yn[n_fft:-n_fft]                                                     # away from the ramps of the first and last windows
    amp = np.abs(np.fft.rfft(mid * np.hanning(len(mid))))
    peak = np.argmax(amp) * sr / len(mid)
    print("peak at %.2f Hz (input %.2f Hz), %d samples for %d" % (peak, f0, want_len, sr))
    assert abs(peak - f0) <= sr / len(mid)                                     # one bin of this estimate
    kapre.check_device()
