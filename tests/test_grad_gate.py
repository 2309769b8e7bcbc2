"""-m gpu: the gradient gate.  tests/test_autograd.py checks every backward pass at batch 2 - 4 with a few dozen frames, where
the host dispatch (kapre_amd/csrc/kpr_host_*.h) only ever picks its smallest route.  Here the same float64 checker
(tests/grad_model.py) meets the backward passes at the launch sizes where the choice of kernel changes:

  A  STFT^T = an inverse-STFT launch (istft_route): barrier kernel up to 3072 frames, ring kernel above, k_istft_pw / _il from
     3/4 item per CU, k_istft_ws_mr, the two-kernel fallback -- with the window n_fft * w, pad_left and the crop on top
  B  InverseSTFT^T = an STFT launch (stft_pow2_kernel): k_stft3 / k_stft3_cl from 8 frame groups per CU, k_stft below
  C  ApplyFilterbank^T / LogmelToMFCC^T = the dense k_gemm (k_thin_gemm where the shape allows) at 63 ... 20 481 rows
  D  the grid-stride kernels of csrc/kpr_grad_kernels.h past their grid cap
  E  k_db_bwd: long items, many items, exact ties in one thread's stride and across threads
  F  ChainFn.backward: the chunk seam, a ragged last chunk, chunks of one item

Every case asserts the kernel that ran.  kpr_last_launches is per thread and autograd's backward runs on a thread of its own:
sections A - E call the vjp functions from the test thread and read the log there; where a backward has to go through
.backward() the log is noted where the launcher returns (record_launches).  The gradient entry points of
kpr_grad_kernels.h do not restart the log, an entry point of the forward path does: fresh_log() runs a one-element
Magnitude first, and the kernel under test is the last label of the log.

Shapes are derived from the dispatch for the CU count the device reports (256 on an MI355X); every case says which line of
the dispatch puts it on its route.  Each check prints its error as a fraction of its limit (WORST; DESIGN.md 4.8 quotes
them), the last test asserts the set of kernels the file reached under automatic options.
"""
import contextlib

import numpy as np
import pytest
import torch

import kapre_amd as kapre
from kapre_amd import STFT, InverseSTFT, Magnitude, ApplyFilterbank, Delta, _ffi, autograd, backend
from kapre_amd.composed import get_melspectrogram_layer
from kapre_amd.keras_shim import Sequential
from kapre_amd.signal import Frame, Energy, LogmelToMFCC
from grad_model import (CL, CF, ref_stft, ref_istft_ola, ref_db, ref_frame, ref_delta, chunked_grad, to_bct, spec_from_bcfk,
                        spec_to_bcfk, loss_of, cotangent, wave)

pytestmark = pytest.mark.gpu

SEEN_AUTO = set()         # kernel labels launched by a backward under automatic dispatch options
WORST = {}                # route -> worst error / limit
U32, U64 = 2.0 ** -24, 2.0 ** -53


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@contextlib.contextmanager
def options(**kw):
    old = {}
    try:
        for k, v in kw.items():
            old[k] = _ffi.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _ffi.set_option(k, v)


def labels_of(log, auto=True):
    labels = [l for l in log.split(' + ') if l]
    if auto:
        SEEN_AUTO.update(labels)
    return labels


def expect(labels, prefix):
    assert any(l.startswith(prefix) for l in labels), 'expected %s, the library launched %s' % (prefix, labels)


def fresh_log():
    """restart this thread's launch log (kpr_abs_c64 is an entry point of the forward path: it clears it)"""
    _ffi.cplx_to_real(torch.ones(1, dtype=torch.complex64, device='cuda'), False)
    assert _ffi.last_launches() == 'k_cplx_to_real'


def last_label(auto=True):
    return labels_of(_ffi.last_launches(), auto)[-1]


def poison(like_numel, dtype):
    """the next torch.empty of this size is handed this block by the caching allocator: what a kernel leaves unwritten is NaN"""
    t = torch.full((int(like_numel),), float('nan'), dtype=dtype, device='cuda')
    del t


def record_launches(monkeypatch, *names):
    """the backward pass runs on autograd's thread and kpr_last_launches is per thread: note it where the launcher returns"""
    seen = []
    for name in names:
        def wrapped(*a, _inner=getattr(_ffi, name), _name=name, **kw):
            out = _inner(*a, **kw)
            seen.append((_name, _ffi.last_launches()))
            return out
        monkeypatch.setattr(_ffi, name, wrapped)
    return seen


def measure(route, got, want, tol, what):
    got = got.detach().cpu()
    if got.is_complex():
        got, want = torch.view_as_real(got.to(torch.complex128)), torch.view_as_real(want)
    got, want = got.to(torch.float64), want.to(torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(want.abs().max())
    assert scale > 0, what
    err = float((got - want).abs().max()) / scale
    err = err if err == err else float('inf')                       # NaN: something was left unwritten
    WORST[route] = max(WORST.get(route, 0.0), err / tol)
    print('grad gate [%s] %s: error %.3g of the largest gradient entry = %.3f of the limit %.1g' % (route, what, err, err / tol, tol))
    assert err <= tol, '%s: max error %.3g of the largest gradient entry (limit %.1g)' % (what, err, tol)


def adjoint_identity(ax, g, x, atg, what):
    """<A x, g> = <x, A^T g>, both sides accumulated in float64 from the device outputs (complex tensors as (re, im) pairs)"""
    pairs = lambda t: torch.view_as_real(t) if t.is_complex() else t
    lhs = float((pairs(ax).double() * pairs(g).double()).sum())
    rhs = float((pairs(x).double() * pairs(atg).double()).sum())
    print('grad gate adjoint identity %s: <A x, g> = %.9e, <x, A^T g> = %.9e' % (what, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (what, lhs, rhs)


def f32(t):
    """float64 values that float32 holds exactly: device and checker see the same numbers"""
    return t.to(torch.float32).to(torch.float64)


# ---------------------------------------------------------------------------------------------
# A. STFT backward: one case per inverse route
# ---------------------------------------------------------------------------------------------
def n34():
    """istft_pw_plan: n_sig * segs * 4 >= 3 * cus -- the smallest item count k_istft_pw takes under automatic options"""
    return -(-3 * cus() // 4)


def pw_need(n_fft, hop, ch_il=1):
    """istft_pw_plan: frames a signal needs for one segment, runs * (R - 1); runs = 16 * G streams (/ C when interleaved),
    R = 16 / S, S = hop / (2 L), L = n_fft / 32 lanes per frame, G = 64 / L frames per wave"""
    lanes = n_fft // 32
    s = hop // (2 * lanes)
    assert s in (2, 4, 8)
    return (16 * (64 // lanes) // ch_il) * (16 // s - 1)


def pw_frames(n_fft, hop, n_sig, ch_il=1):
    """one segment per signal (F < 2 * need), and more than 3072 frames in the launch (istft_route: `small`)"""
    need = pw_need(n_fft, hop, ch_il)
    f = max(need + 1, 3072 // (n_sig * ch_il) + 1)
    assert f < 2 * need or n_sig * 4 >= 3 * cus()
    return f


def t_for(frames, n_fft, win, hop, pad_begin, pad_end, ragged):
    """a waveform length that frames into `frames` frames; ragged: not on the hop grid, so with pad_end the last frames run
    past the signal and the crop min(t_in, t_ola - pad_left) of stft_vjp bites"""
    pad = n_fft - hop if pad_begin else 0
    if pad_end:
        t = (frames - 1) * hop + (hop // 3 + 1 if ragged else hop)
    else:
        t = (frames - 1) * hop + win + (hop // 3 if ragged else 0)
    assert t - pad > 0
    return t - pad


def stft_cases():
    """id -> (n_fft, win, hop, pad_begin, pad_end, in_fmt, out_fmt, ch, batch, frames, ragged, expected label, options).
    Built at run time: the item thresholds follow the device's CU count."""
    q = n34()
    c = {}
    # istft_route: small = total_frames <= 3072 -> istft_fused_plan (the barrier kernel), exactly on the threshold
    c['barrier_on_3072'] = (512, None, 128, True, False, CL, CL, 1, 1, 3072, False, 'k_istft_fused<256>', {})
    # one frame beyond: !small, 1 signal x at most 16 segments < 3/4 item per CU -> istft_pw_plan refuses -> istft_ring_plan
    c['ring_on_3073'] = (512, None, 128, True, False, CL, CL, 1, 1, 3073, False, 'k_istft_ws<256,', {})
    # just below: 3 x 2 x 511 = 3066 frames, interleaved spectrogram (the barrier kernel takes any layout pair)
    c['barrier_3066_mixed'] = (1024, None, 256, False, True, CF, CL, 2, 3, 511, True, 'k_istft_fused<512>', {})
    # just above: 3 signals x 1025 = 3075 frames, 3 x at most 10 segments < 3/4 item per CU -> the ring kernel
    c['ring_3075'] = (1024, None, 256, True, True, CF, CF, 3, 1, 1025, True, 'k_istft_ws<512,', {})
    # istft_pw_plan: n_sig * segs * 4 >= 3 * cus with one segment per signal: exactly 3/4 item per CU, and one item short of it
    f = pw_frames(512, 128, q)
    c['pw_512_on_threshold'] = (512, None, 128, True, False, CL, CF, 1, q, f, False, 'k_istft_pw<256,s4>', {})
    c['ring_one_item_short'] = (512, None, 128, True, False, CL, CF, 1, q - 1, f, False, 'k_istft_ws<256,', {})
    c['pw_1024'] = (1024, None, 256, False, True, CF, CF, 1, q, pw_frames(1024, 256, q), True, 'k_istft_pw<512,s4>', {})
    # win_length 1500 of 2048: istft_pw_plan asks win <= n_fft and hop <= win only
    c['pw_2048_win1500'] = (2048, 1500, 512, True, True, CF, CL, 1, q, pw_frames(2048, 512, q), True, 'k_istft_pw<1024,s4>', {})
    c['pw_hop_half'] = (1024, None, 512, True, False, CF, CF, 1, q, pw_frames(1024, 512, q), True, 'k_istft_pw<512,s8>', {})
    c['pw_hop_eighth'] = (2048, None, 256, False, False, CL, CL, 1, q, pw_frames(2048, 256, q), False, 'k_istft_pw<1024,s2>', {})
    # il: channels_last with C = 2 on both sides, items = batch entries, runs = 32 / 2 streams
    c['pw_il'] = (1024, None, 256, True, True, CL, CL, 2, q, pw_frames(1024, 256, q, 2), True, 'k_istft_pw_il<512,s4>', {})
    # !fast_nfft -> istft_ws_mr_plan: R = 3 overlapping frames (rj 4), hop and win multiples of four
    c['ws_mr_400'] = (400, 400, 160, False, True, CL, CL, 1, 64, 100, True, 'k_istft_ws_mr<200,', {})
    # n_fft 1200 has no mixed-radix plan: fft_family -> the run-time FFT into the workspace, then k_ola
    c['two_kernel_1200'] = (1200, None, 300, False, True, CL, CL, 2, 8, 40, True, 'k_ola', {})
    # hop 250 is no multiple of four: istft_ws_mr_plan refuses (vec == 2) -> k_irfft_mr + k_ola
    c['two_kernel_1000'] = (1000, None, 250, True, False, CF, CF, 1, 8, 60, True, 'k_ola', {})
    # forced options: the geometry of the large kernels at a small size
    c['forced_pw'] = (512, None, 256, True, True, CF, CF, 1, 2, 70, True, 'k_istft_pw<256,s8>', dict(istft_path=4))
    c['forced_ring'] = (2048, None, 512, False, True, CL, CL, 1, 2, 20, True, 'k_istft_ws<1024,', dict(istft_path=3))
    return c


STFT_IDS = ['barrier_on_3072', 'ring_on_3073', 'barrier_3066_mixed', 'ring_3075', 'pw_512_on_threshold', 'ring_one_item_short',
            'pw_1024', 'pw_2048_win1500', 'pw_hop_half', 'pw_hop_eighth', 'pw_il', 'ws_mr_400', 'two_kernel_1200',
            'two_kernel_1000', 'forced_pw', 'forced_ring']


@pytest.mark.parametrize('case', STFT_IDS)
def test_stft_backward_routes(case):
    n_fft, win, hop, pad_begin, pad_end, in_fmt, out_fmt, ch, batch, frames, ragged, label, opts = stft_cases()[case]
    layer = STFT(n_fft=n_fft, win_length=win, hop_length=hop, pad_begin=pad_begin, pad_end=pad_end,
                 input_data_format=in_fmt, output_data_format=out_fmt)
    win = win or n_fft
    t = t_for(frames, n_fft, win, hop, pad_begin, pad_end, ragged)
    x_shape = (batch, t, ch) if in_fmt == CL else (batch, ch, t)
    y_shape = tuple(layer.compute_output_shape(x_shape))
    assert y_shape == ((batch, frames, n_fft // 2 + 1, ch) if out_fmt == CL else (batch, ch, frames, n_fft // 2 + 1))
    assert batch * ch * frames <= 40000
    r = f32(cotangent(y_shape, True, seed=n_fft + hop + frames))
    g = torch.view_as_complex(r.to(torch.float32).contiguous()).cuda()
    auto = not opts
    with options(**opts):
        poison(batch * ch * ((frames - 1) * hop + win), torch.float32)
        gx = autograd.stft_vjp(layer, g, x_shape)
        labels = labels_of(_ffi.last_launches(), auto)              # the inverse launch restarted the log
    expect(labels, label)
    assert tuple(gx.shape) == x_shape

    window = backend.get_window_fn(None)(win).astype(np.float64)
    fn = lambda xr: spec_from_bcfk(ref_stft(to_bct(xr, in_fmt), n_fft, win, hop, window, pad_begin, pad_end), out_fmt)
    want = chunked_grad(fn, torch.zeros(x_shape, dtype=torch.float64), r, max(1, batch // 8))     # linear: any x
    measure('STFT^T ' + label.rstrip(',<'), gx, want, 2e-4, case)
    if pad_end and ragged:                                           # frames run past the signal: the crop dropped their tail
        assert (frames - 1) * hop + win - (n_fft - hop if pad_begin else 0) > t

    xa = (gx / gx.abs().max()).contiguous()
    with options(**opts):
        ax = layer(xa)
    adjoint_identity(ax, g, xa, gx, case)
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# B. InverseSTFT backward: the STFT dispatch with pad_begin = pad_end = 0 and the window 2 w_s / n_fft
# ---------------------------------------------------------------------------------------------
def istft_cases():
    """id -> (n_fft, win, hop, in_fmt (spectrogram), out_fmt (waveform), ch, batch, frames, expected label, options).
    stft_pow2_kernel: G = 64 / (n_fft / 32) frames per wave, k_stft3 from ngroups = ceil(total_frames / G) >= 8 * cus."""
    g8 = 8 * cus()
    c = {}
    c['stft3_512_on_threshold'] = (1024, None, 256, CL, CL, 1, 1, 2 * g8 - 1, 'k_stft3<512,complex>', {})     # ceil(4095 / 2) = 2048 groups
    c['stft_512_one_group_short'] = (1024, None, 256, CL, CL, 1, 1, 2 * g8 - 2, 'k_stft<512,complex>', {})    # 2047 groups
    c['stft3_1024_on_threshold'] = (2048, None, 512, CF, CF, 1, 1, g8, 'k_stft3<1024,complex>', {})           # G = 1: 2048 groups
    c['stft_1024_one_frame_short'] = (2048, None, 512, CF, CF, 1, 1, g8 - 1, 'k_stft<1024,complex>', {})
    # cfast (an interleaved side, C > 1) and C % G == 0: the CL instance
    c['stft3_cl'] = (1024, None, 256, CL, CL, 2, 1, g8, 'k_stft3_cl<512,complex>', {})
    c['stft_256'] = (512, None, 128, CL, CF, 1, 1, 4 * g8 + 3, 'k_stft<256,complex', {})                      # NC < 512: k_stft at any size
    c['mixed_radix_400'] = (400, 400, 100, CF, CF, 2, 4, 200, 'k_stft_mr<200>', {})
    c['n_fft_1000'] = (1000, None, 250, CL, CL, 1, 4, 100, 'k_stft_', {})
    c['forced_stft3_cl'] = (1024, None, 256, CL, CF, 2, 2, 30, 'k_stft3_cl<512,complex>', dict(stft_variant=3))
    return c


ISTFT_IDS = ['stft3_512_on_threshold', 'stft_512_one_group_short', 'stft3_1024_on_threshold', 'stft_1024_one_frame_short',
             'stft3_cl', 'stft_256', 'mixed_radix_400', 'n_fft_1000', 'forced_stft3_cl']


def istft_reference(layer, n_fft, win, hop, in_fmt, out_fmt, spec_shape, r, crop=None):
    """d<istft(X), r>/dX; crop(sr) -> the n_fft / 2 + 1 bins the forward feeds the transform"""
    synth = backend.window_values(layer.window_fn, win, np.float64)

    def fn(sr):
        full = crop(sr) if crop else sr
        y = ref_istft_ola(spec_to_bcfk(full, in_fmt), n_fft, win, hop, synth)
        return y.permute(0, 2, 1) if out_fmt == CL else y
    return chunked_grad(fn, torch.zeros(spec_shape, dtype=torch.complex128), r, 1)


@pytest.mark.parametrize('case', ISTFT_IDS)
def test_istft_backward_routes(case):
    n_fft, win, hop, in_fmt, out_fmt, ch, batch, frames, label, opts = istft_cases()[case]
    layer = InverseSTFT(n_fft=n_fft, win_length=win, hop_length=hop, input_data_format=in_fmt, output_data_format=out_fmt)
    win = win or n_fft
    k = n_fft // 2 + 1
    assert batch * ch * frames <= 40000
    t = (frames - 1) * hop + win
    spec_shape = (batch, frames, k, ch) if in_fmt == CL else (batch, ch, frames, k)
    y_shape = (batch, t, ch) if out_fmt == CL else (batch, ch, t)
    r = f32(cotangent(y_shape, False, seed=n_fft + frames))
    g = r.to(torch.float32).cuda()
    auto = not opts
    with options(**opts):
        poison(2 * batch * ch * frames * k, torch.float32)
        gs = autograd.istft_vjp(layer, g, frames)
        labels = labels_of(_ffi.last_launches(), auto)              # the STFT launch restarted the log; edge_scale follows it
    expect(labels[:1], label)
    assert labels[-1] == 'k_spec_edge_scale'
    assert tuple(gs.shape) == spec_shape
    want = istft_reference(layer, n_fft, win, hop, in_fmt, out_fmt, spec_shape, r)
    measure('InverseSTFT^T ' + labels[0], gs, want, 2e-4, case)

    sa = (gs / gs.abs().max()).contiguous()
    with options(**opts):
        ay = layer(sa)
    assert tuple(ay.shape) == y_shape
    adjoint_identity(ay, g, sa, gs, case)
    kapre.check_device()


@pytest.mark.parametrize('k_in', [600, 400])
def test_istft_backward_cropped_or_padded_frequency_axis_at_the_large_route(monkeypatch, k_in):
    """ISTFTFn.backward on top of the k_stft3 launch (4095 frames at n_fft 1024 = 2048 groups = 8 per CU): 600 bins are cropped
    to 513 by the forward (the cropped bins get a zero gradient), 400 are zero-padded (the gradient is cut back)."""
    n_fft, hop, frames, k = 1024, 256, 2 * 8 * cus() - 1, 513
    seen = record_launches(monkeypatch, 'stft')
    layer = InverseSTFT(n_fft=n_fft, hop_length=hop)
    s0 = torch.view_as_complex(f32(cotangent((1, frames, k_in, 1), True, seed=k_in)))
    sg = s0.to(torch.complex64).cuda().requires_grad_(True)
    y = layer(sg)
    r = f32(cotangent(y.shape, False, seed=k_in + 1))
    poison(2 * frames * k, torch.float32)
    loss_of(y, r).backward()
    assert len(seen) == 1
    label = labels_of(seen[0][1])[0]
    assert label == 'k_stft3<512,complex>'

    def crop(sr):
        if k_in > k:
            return sr[:, :, :k]
        return torch.view_as_complex(torch.nn.functional.pad(torch.view_as_real(sr), (0, 0, 0, 0, 0, k - k_in)).contiguous())
    want = istft_reference(layer, n_fft, n_fft, hop, CL, CL, tuple(s0.shape), r, crop)
    assert tuple(sg.grad.shape) == (1, frames, k_in, 1)
    measure('InverseSTFT^T ' + label, sg.grad, want, 2e-4, 'with %d bins' % k_in)
    if k_in > k:
        assert float(torch.view_as_real(sg.grad[:, :, k:]).abs().max()) == 0.0
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# C. matrix backward: kpr_apply_filterbank_f32 with (n_freq, n_filt) := (n_out, n_in) of the layer
# ---------------------------------------------------------------------------------------------
ROWS = [63, 64, 65, 64 * 320 + 1]       # around the 64-row tile of k_gemm / k_thin_gemm, and a training batch (20 481 rows)


def gemm_label(n_in, n_out, contiguous):
    """kpr_apply_filterbank_f32 as the backward calls it (no k-ranges: the dense product; 1025 outputs are 65 tiles, over
    kMaxTiles).  thin_gemm_shape: at most 4 tiles of 16 outputs, an inner dimension that is a multiple of four, contiguous rows."""
    thin = (n_out + 15) // 16 <= 4 and n_in <= 512 and n_in % 4 == 0
    return 'k_thin_gemm' if thin and contiguous else 'k_gemm'


def run_matrix_backward(route, layer, mat_t, fmt, rows, n_in, n_out, seed):
    """mat_t: (n_out, n_in) on the device, the matrix the layer's backward hands to _ffi.freq_matmul.  channels_first: one
    channel, `rows` frames; channels_last: C = 3 interleaved, `rows` GEMM rows when 3 divides it, else `rows` frames."""
    c = 1 if fmt == CF else 3
    frames = rows if fmt == CF or rows % 3 else rows // 3
    g_shape = (1, frames, n_out, c) if fmt == CL else (1, c, frames, n_out)
    x_shape = (1, frames, n_in, c) if fmt == CL else (1, c, frames, n_in)
    r = f32(cotangent(g_shape, False, seed=seed))
    g = r.to(torch.float32).cuda()
    poison(frames * c * n_in, torch.float32)
    gx = _ffi.freq_matmul(g, fmt, mat_t)
    label = last_label()
    assert label == gemm_label(n_out, n_in, fmt == CF), (label, _ffi.last_launches())
    assert tuple(gx.shape) == x_shape
    m = mat_t.detach().cpu().to(torch.float64).t()                   # (n_in, n_out): what the forward applies
    xr = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    loss_of(torch.einsum('bfkc,km->bfmc', xr, m) if fmt == CL else xr @ m, r).backward()
    what = '%s %s rows %d (%d -> %d)' % (route, fmt, frames * c, n_out, n_in)
    measure(route + '^T ' + label, gx, xr.grad, 2e-5, what)
    xa = (gx / gx.abs().max()).contiguous()
    adjoint_identity(layer(xa), g, xa, gx, what)


@pytest.mark.parametrize('fmt', [CL, CF])
@pytest.mark.parametrize('kind,n_freq,n_filt', [('mel', 257, 40), ('mel', 1025, 128), ('log', 513, 84)])
def test_filterbank_backward_rows(fmt, kind, n_freq, n_filt):
    kw = dict(sample_rate=22050, n_freq=n_freq, n_mels=n_filt) if kind == 'mel' else dict(sample_rate=22050, n_freq=n_freq, n_bins=n_filt)
    layer = ApplyFilterbank(type=kind, filterbank_kwargs=kw, data_format=fmt)
    assert tuple(np.asarray(layer.filterbank).shape) == (n_freq, n_filt)
    mat_t = layer._fb_transposed_device(torch.device('cuda', torch.cuda.current_device()), False)
    for rows in ROWS:
        run_matrix_backward('ApplyFilterbank', layer, mat_t, fmt, rows, n_freq, n_filt, seed=rows)
    kapre.check_device()


@pytest.mark.parametrize('fmt', [CL, CF])
@pytest.mark.parametrize('n_mels,n_mfccs', [(40, 13), (40, 20), (80, 13), (80, 20)])
def test_mfcc_backward_rows(fmt, n_mels, n_mfccs):
    """inner dimension of the backward product = n_mfccs: 13 is odd (no float4 rows: k_gemm), 20 from 40 mels is the thin GEMM"""
    layer = LogmelToMFCC(n_mfccs=n_mfccs, data_format=fmt)
    mat_t = layer._matrix(n_mels, torch.device('cuda', torch.cuda.current_device())).t().contiguous()
    assert tuple(mat_t.shape) == (n_mfccs, n_mels)
    for rows in ROWS:
        run_matrix_backward('LogmelToMFCC', layer, mat_t, fmt, rows, n_mels, n_mfccs, seed=rows + 1)
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# D. elementwise and gather adjoints past the grid cap
# ---------------------------------------------------------------------------------------------
# grid_1d caps k_cplx_to_real_bwd and k_spec_edge_scale at 4096 blocks of 256 threads: from 4096 * 256 + 1 elements on a thread
# takes a second element, from 2 * 4096 * 256 + 1 a third.  Frame / Energy / Delta backward pass grid_1d a cap of 65536 blocks:
# their loops stride from 65536 * 256 + 1 elements (N_WIDE).
N_ONE, N_THREE = 4096 * 256 + 257, 3 * 4096 * 256 + 1
N_WIDE = 65536 * 256 + 257


@pytest.mark.parametrize('n', [N_ONE, N_THREE])
@pytest.mark.parametrize('phase', [0, 1])
def test_complex_to_real_backward_past_the_grid_cap(n, phase):
    s0 = torch.view_as_complex(f32(cotangent((n,), True, seed=n % 1000 + phase)))
    r = f32(cotangent((n,), False, seed=n % 1000 + 2))
    fresh_log()
    poison(2 * n, torch.float32)
    gx = _ffi.cplx_to_real_bwd(s0.to(torch.complex64).cuda(), r.to(torch.float32).cuda(), phase)
    assert last_label() == 'k_cplx_to_real_bwd'
    sr = s0.clone().requires_grad_(True)
    loss_of(torch.angle(sr) if phase else torch.abs(sr), r).backward()
    measure('Phase' if phase else 'Magnitude', gx, sr.grad, 2e-5, '%d elements' % n)
    # the largest entry of the phase gradient is 1 / min |x|: also element by element, relative to each entry's own size
    got = torch.view_as_real(gx.cpu().to(torch.complex128))
    want = torch.view_as_real(sr.grad)
    rel = float(((got - want).abs().amax(dim=1) / want.abs().amax(dim=1).clamp(min=1e-30)).max())
    print('grad gate [%s] %d elements: worst entry-relative error %.3g' % ('Phase' if phase else 'Magnitude', n, rel))
    assert rel <= 2e-5
    kapre.check_device()


@pytest.mark.parametrize('n_min', [N_ONE, N_THREE])
@pytest.mark.parametrize('n_fft', [512, 511])
@pytest.mark.parametrize('fmt', [CL, CF])
def test_edge_scale_past_the_grid_cap_is_exact(n_min, n_fft, fmt):
    """the kernel takes whole spectra: the smallest number of (K, C = 3) frames with at least n_min elements.  A factor of 0.5
    or 1 is exact, so the result is compared bit for bit; odd n_fft has no Nyquist bin."""
    k, c = n_fft // 2 + 1, 3
    frames = -(-n_min // (k * c))
    shape = (1, frames, k, c) if fmt == CL else (1, c, frames, k)
    s0 = torch.view_as_complex(cotangent(shape, True, seed=n_fft).to(torch.float32).contiguous())
    fresh_log()
    poison(2 * s0.numel(), torch.float32)
    out = _ffi.edge_scale(s0.cuda(), n_fft, fmt, 0.5, 1.0)
    assert last_label() == 'k_spec_edge_scale'
    scale = np.ones(k, np.float32)
    scale[0] = 0.5
    if n_fft % 2 == 0:
        scale[n_fft // 2] = 0.5
    want = s0.numpy() * (scale.reshape(1, 1, k, 1) if fmt == CL else scale.reshape(1, 1, 1, k))
    assert out.cpu().numpy().tobytes() == want.astype(np.complex64).tobytes()
    # in place, the way istft_vjp uses it
    sd = s0.cuda()
    assert _ffi.edge_scale(sd, n_fft, fmt, 0.5, 1.0, out=sd) is sd
    assert sd.cpu().numpy().tobytes() == want.astype(np.complex64).tobytes()
    kapre.check_device()


def frame_shape(n, fmt):
    """n elements of input cotangent: channels_last with C = 3 when 3 divides n, else one channel"""
    c = 3 if fmt == CL and n % 3 == 0 else 1
    return ((1, n // c, c) if fmt == CL else (1, c, n // c)), c


@pytest.mark.parametrize('n,length,hop', [(N_ONE, 200, 77), (N_THREE, 64, 48), (N_WIDE, 32, 24)])
@pytest.mark.parametrize('fmt', [CL, CF])
def test_frame_backward_large(n, length, hop, fmt):
    """pad_end on, a hop that divides neither the length nor the frame; N_WIDE is where k_frame_bwd's loop takes its stride"""
    x_shape, c = frame_shape(n, fmt)
    t = n // c
    assert t % hop != 0
    layer = Frame(frame_length=length, hop_length=hop, pad_end=True, pad_value=0.25, data_format=fmt)
    frames = -(-t // hop)
    g_shape = (1, frames, length, c) if fmt == CL else (1, c, frames, length)
    r = f32(cotangent(g_shape, False, seed=length))
    g = r.to(torch.float32).cuda()
    fresh_log()
    poison(n, torch.float32)
    gx = _ffi.frame_bwd(g, x_shape, fmt, length, hop, True)
    assert last_label() == 'k_frame_bwd'
    xr = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    yr = ref_frame(to_bct(xr, fmt), length, hop, True, 0.25)
    yr = yr.permute(0, 2, 3, 1) if fmt == CL else yr
    assert tuple(yr.shape) == g_shape
    loss_of(yr, r).backward()
    measure('Frame', gx, xr.grad, 1e-6, '%d elements %s' % (n, fmt))
    xa = (gx / gx.abs().max()).contiguous()
    # Frame is affine (pad_value 0.25): A x = Frame(x) - Frame(0), exact in float32
    adjoint_identity(layer(xa) - layer(torch.zeros_like(xa)), g, xa, gx, 'Frame %d %s' % (n, fmt))
    kapre.check_device()


@pytest.mark.parametrize('n,length,hop', [(N_ONE, 400, 160), (N_THREE, 2205, 1102), (N_WIDE, 64, 48)])
@pytest.mark.parametrize('fmt', [CL, CF])
def test_energy_backward_large(n, length, hop, fmt):
    x_shape, c = frame_shape(n, fmt)
    t = n // c
    assert t % hop != 0
    layer = Energy(sample_rate=22050, ref_duration=0.1, frame_length=length, hop_length=hop, pad_end=True, pad_value=0,
                   data_format=fmt)
    frames = -(-t // hop)
    g_shape = (1, frames, c) if fmt == CL else (1, c, frames)
    x0 = wave(1, c, t, fmt, seed=length)
    r = f32(cotangent(g_shape, False, seed=length + 1))
    fresh_log()
    poison(n, torch.float32)
    gx = _ffi.energy_bwd(x0.cuda(), r.to(torch.float32).cuda(), fmt, length, hop, True, layer._scale())
    assert last_label() == 'k_energy_bwd'
    xr = x0.to(torch.float64).requires_grad_(True)
    fr = ref_frame(to_bct(xr, fmt), length, hop, True, 0.0)
    yr = (fr * fr).sum(-1) * (0.1 / (length / 22050))
    yr = yr.permute(0, 2, 1) if fmt == CL else yr
    assert tuple(yr.shape) == g_shape
    loss_of(yr, r).backward()
    measure('Energy', gx, xr.grad, 2e-6, '%d elements %s' % (n, fmt))
    kapre.check_device()


@pytest.mark.parametrize('n,fmt,win', [(N_ONE, CL, 5), (N_THREE, CF, 9), (N_WIDE, CL, 5)])
@pytest.mark.parametrize('mode', ['symmetric', 'reflect', 'constant'])
def test_delta_backward_large(n, fmt, win, mode):
    """N_ONE = 9 * 116537: channels_last (1, T, 3, 3); N_THREE: channels_first (1, 1, T, 1), the time axis itself past the cap;
    N_WIDE (where k_delta_bwd's loop takes its stride): (1, T, 13, 1) and the largest n below a multiple of 13"""
    if n == N_ONE:
        shape, t_axis = (1, n // 9, 3, 3), 1
    elif n == N_THREE:
        shape, t_axis = (1, 1, n, 1), 2
    else:
        shape, t_axis = (1, -(-n // 13), 13, 1), 1
    total = int(np.prod(shape))
    assert total >= n and (n != N_ONE or total == n)
    layer = Delta(win_length=win, mode=mode, data_format=fmt)
    r = f32(cotangent(shape, False, seed=win))
    g = r.to(torch.float32).cuda()
    fresh_log()
    poison(total, torch.float32)
    gx = _ffi.delta(g, fmt, win, mode, backward=True)
    assert last_label() == 'k_delta_bwd'
    xr = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    loss_of(ref_delta(xr, t_axis, win, mode), r).backward()
    measure('Delta', gx, xr.grad, 2e-6, '%d elements %s %s' % (total, fmt, mode))
    xa = (gx / gx.abs().max()).contiguous()
    adjoint_identity(layer(xa), g, xa, gx, 'Delta %d %s %s' % (total, fmt, mode))
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# E. k_db_bwd
# ---------------------------------------------------------------------------------------------
REF, AMIN, DYN = 0.7, 1e-3, 15.0


def db_input(n_items, item, tdt, seed):
    """magnitudes over ~100 dB, some below amin, in the precision the layer sees.  The item maximum is made unique (x 1.5) and
    no value is left within 2e-3 dB of the floor (x 1.01 = 0.043 dB), so that float32 and float64 agree on both masks."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.exp(3.0 * torch.randn((n_items, item), generator=g, dtype=torch.float64)) * 1e-2).to(tdt).to(torch.float64)
    top = x.argmax(dim=1)
    x[torch.arange(n_items), top] = (x[torch.arange(n_items), top] * 1.5).to(tdt).to(torch.float64)
    for _ in range(8):
        l = 10.0 * torch.log10(torch.clamp(x, min=AMIN)) - 10.0 * np.log10(REF)
        near = ((l - (l.amax(dim=1, keepdim=True) - DYN)).abs() < 2e-3) & (x > AMIN)
        if not bool(near.any()):
            break
        x = torch.where(near, (x * 1.01).to(tdt).to(torch.float64), x)
    assert not bool(near.any())
    return x


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('n_items,item', [(1, 1024 * 37 + 5), (1, 252 * 128 * 6), (300, 1024 * 3 + 5)])
def test_decibel_backward_long_items_and_many_items(dtype, n_items, item):
    """dynamic_range 15: most of every item sits on the floor and its cotangent reaches the item's maximum.

    Limit for the entry of the maximum, derived: the kernel sums the n_f floor cotangents in the item's precision (unit
    round-off u = 2^-24 / 2^-53) as 1024 per-thread sums of at most m = ceil(item / 1024) terms and a 1024-way tree of 10 levels:
    every term passes through at most m - 1 + 10 additions, so |fsum - exact| <= (m + 9) u sum_floor |g| (first order).  The
    entry is (g_max + fsum / ties) * c / x_max with ties = 1: one addition, the constant c, one multiplication and one
    division add 4 u of the entry.  Every other entry: the project's limit (2e-4 / 1e-9 of the largest entry), skipping what
    lies within 1e-3 dB of the floor (more than 99 % must remain)."""
    tdt = torch.float64 if dtype == 'float64' else torch.float32
    u = U64 if dtype == 'float64' else U32
    x0 = db_input(n_items, item, tdt, seed=item % 997)
    r = cotangent((n_items, item), False, seed=item % 997 + 1).to(tdt).to(torch.float64)
    fresh_log()
    poison(n_items * item, tdt)
    gx = _ffi.mag_to_db_bwd(x0.to(tdt).cuda(), r.to(tdt).cuda(), REF, AMIN, DYN)
    assert last_label() == 'k_db_bwd'
    got = gx.cpu().to(torch.float64)

    xr = x0.clone().requires_grad_(True)
    yr = ref_db(xr, REF, AMIN, DYN)
    floor_share = (yr == yr.amin(dim=1, keepdim=True)).double().mean(dim=1)
    assert float(floor_share.min()) > 0.05
    loss_of(yr, r).backward()
    want = xr.grad
    l = 10.0 * torch.log10(torch.clamp(x0, min=AMIN)) - 10.0 * np.log10(REF)
    thr = l.amax(dim=1, keepdim=True) - DYN
    safe = (l - thr).abs() > 1e-3
    assert float(safe.double().mean()) > 0.99
    top = l.argmax(dim=1)
    rows = torch.arange(n_items)
    is_top = torch.zeros_like(safe)
    is_top[rows, top] = True
    tol = 2e-4 if dtype == 'float32' else 1e-9
    scale = float(want.abs().max())
    err = float(((got - want).abs() * (safe & ~is_top)).max()) / scale
    WORST['MagnitudeToDecibel ' + dtype] = max(WORST.get('MagnitudeToDecibel ' + dtype, 0.0), err / tol)
    print('grad gate [k_db_bwd %s] %d x %d: error %.3g of the largest entry = %.3f of the limit' % (dtype, n_items, item, err, err / tol))
    assert err <= tol
    # the entries of the maxima
    below = l < thr
    m = -(-item // 1024)
    e_sum = (m + 9) * u * (r.abs() * below).sum(dim=1)
    c = 10.0 / np.log(10.0)
    bound = (e_sum * c / x0[rows, top]) + 4 * u * want[rows, top].abs()
    ratio = float(((got[rows, top] - want[rows, top]).abs() / bound).max())
    WORST['k_db_bwd maximum ' + dtype] = max(WORST.get('k_db_bwd maximum ' + dtype, 0.0), ratio)
    print('grad gate [k_db_bwd %s] %d x %d: entry of the maximum, worst error / derived bound = %.3g' % (dtype, n_items, item, ratio))
    assert ratio <= 1.0
    kapre.check_device()


@pytest.mark.parametrize('second', [7 + 1024 * 2, 8 + 1024], ids=['same_thread', 'other_thread'])
def test_decibel_backward_ties_in_a_long_item(second):
    """Two maxima 16 at elements 7 and 7 + 2048 (thread 7 meets both in its stride) or 8 + 1024 (threads 7 and 8), one
    element 8 EXACTLY on the floor, everything else 4 / 2 / 1 / 0.5 below it.  Powers of two: l = fl(c k) in every kernel and
    dyn := l(16) - l(8) is exact (as in tests/test_autograd.py).  Cotangents are multiples of 1/8 below 2^10, so every float32
    partial sum is exact in any order.  TensorFlow's conventions in closed form: the maxima share the floor's cotangent
    evenly, the element on the floor keeps its own and feeds nothing:
        gl[max] = r + below / 2, gl[floor element] = r, gl[else] = 0, gx = gl * 10 / (ln 10 * x)."""
    c = np.float32(3.01029995663981195)
    l16, l8 = np.float32(c * np.float32(4.0)), np.float32(c * np.float32(3.0))
    dyn = float(np.float32(l16 - l8))
    assert np.float32(l16 - np.float32(dyn)) == l8
    item = 1024 * 3 + 5
    rng = np.random.default_rng(second)
    vals = rng.choice(np.array([4.0, 2.0, 1.0, 0.5], np.float32), size=(2, item))
    vals[:, 7] = 16.0
    vals[:, second] = 16.0
    vals[:, 100] = 8.0
    rn = rng.integers(-16, 17, size=(2, item)).astype(np.float64) / 8.0
    x = torch.from_numpy(vals).cuda()
    fresh_log()
    poison(2 * item, torch.float32)
    gx = _ffi.mag_to_db_bwd(x, torch.from_numpy(rn.astype(np.float32)).cuda(), 1.0, 1e-10, dyn)
    assert last_label() == 'k_db_bwd'
    y = _ffi.mag_to_db(x, 1.0, 1e-10, dyn).cpu().numpy()
    assert (y[:, [7, second]] == l16).all() and (y[:, 100] == l8).all() and (np.delete(y, [7, second], axis=1) == l8).all()
    below_mask = np.ones(item, bool)
    below_mask[[7, second, 100]] = False
    below = rn[:, below_mask].sum(axis=1)
    gl = np.zeros((2, item))
    gl[:, 7] = rn[:, 7] + below / 2
    gl[:, second] = rn[:, second] + below / 2
    gl[:, 100] = rn[:, 100]
    want = gl * 10.0 / (np.log(10.0) * vals.astype(np.float64))
    got = gx.cpu().numpy().astype(np.float64)
    assert (got[:, below_mask] == 0).all()
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# F. ChainFn.backward: chunked recomputation
# ---------------------------------------------------------------------------------------------
def chain_per_item(x, n_fft, hop):
    """the bytes ChainFn.backward books per batch entry: complex spectrum + magnitudes"""
    return (x.numel() // x.shape[0]) * x.element_size() * (n_fft // 2 + 1) * 3 // hop


def mel_reference(model, x0, r, n_fft, hop, fmt, decibel, dyn):
    xr = x0.to(torch.float64).requires_grad_(True)
    window = backend.get_window_fn(None)(n_fft).astype(np.float64)
    fb = torch.as_tensor(np.asarray(model.layers[2].filterbank, np.float64))
    mel = ref_stft(to_bct(xr, fmt), n_fft, n_fft, hop, window, False, True).abs() @ fb
    mel = mel.permute(0, 2, 3, 1) if fmt == CL else mel
    yr = ref_db(mel, 1.0, 1e-5, dyn) if decibel else mel
    loss_of(yr, r).backward()
    return xr.grad


@pytest.mark.parametrize('fmt', [CL, CF])
@pytest.mark.parametrize('decibel', [False, True])
@pytest.mark.parametrize('n_fft,hop,n_mels,sr,ch', [(2048, 512, 128, 44100, 1), (512, 128, 40, 22050, 2)])
def test_mel_chain_backward_in_chunks(monkeypatch, n_fft, hop, n_mels, sr, ch, decibel, fmt):
    """batch 5 with CHAIN_RECOMPUTE_BYTES set for chunks of 2 (2, 2, 1: a seam and a ragged last chunk), of 1, and of the whole
    batch.  Items differ in loudness (wave), so a decibel maximum taken over the wrong chunk would show; item 2 has a zero
    cotangent and must get an exactly zero gradient.  One inverse launch per chunk is the proof that the seam was walked."""
    t = 6 * n_fft
    model = get_melspectrogram_layer(input_shape=(t, ch) if fmt == CL else (ch, t), n_fft=n_fft, hop_length=hop,
                                     sample_rate=sr, n_mels=n_mels, return_decibel=decibel, db_dynamic_range=60.0,
                                     input_data_format=fmt, output_data_format=fmt, pad_end=True)
    seen = record_launches(monkeypatch, 'istft')
    x0 = wave(5, ch, t, fmt, seed=61)
    per_item = chain_per_item(x0, n_fft, hop)
    want = None
    for step, chunks in ((2, 3), (1, 5), (5, 1)):
        monkeypatch.setattr(autograd, 'CHAIN_RECOMPUTE_BYTES', step * per_item + per_item // 2 if step > 1 else 1)
        xg = x0.cuda().requires_grad_(True)
        y = model(xg)
        forward = _ffi.last_launches()
        assert 'k_mel_' in forward and 'k_stft' not in forward, forward          # the fused launch
        if want is None:
            r = f32(cotangent(y.shape, False, seed=62))
            r[2] = 0.0
            want = mel_reference(model, x0, r, n_fft, hop, fmt, decibel, 60.0)
            assert float(want[2].abs().max()) == 0.0
        del seen[:]
        loss_of(y, r).backward()
        assert len(seen) == chunks, (step, seen)
        for _, log in seen:
            expect(labels_of(log), 'k_istft_fused<%d>' % (n_fft // 2))
        measure('fused mel chain', xg.grad, want, 3e-4, 'n_fft %d %s dB %s, chunks of %d' % (n_fft, fmt, decibel, step))
        assert float(xg.grad[2].abs().max()) == 0.0
    kapre.check_device()


@pytest.mark.parametrize('fmt', [CL, CF])
def test_stft_magnitude_chain_backward_in_chunks(monkeypatch, fmt):
    n_fft, hop, ch, t = 1024, 256, 2, 5000
    model = Sequential([STFT(n_fft=n_fft, hop_length=hop, pad_begin=True, input_data_format=fmt, output_data_format=fmt),
                        Magnitude()])
    seen = record_launches(monkeypatch, 'istft')
    x0 = wave(5, ch, t, fmt, seed=71)
    per_item = chain_per_item(x0, n_fft, hop)
    want = None
    for step, chunks in ((2, 3), (1, 5), (5, 1)):
        monkeypatch.setattr(autograd, 'CHAIN_RECOMPUTE_BYTES', step * per_item + per_item // 2 if step > 1 else 1)
        xg = x0.cuda().requires_grad_(True)
        y = model(xg)
        forward = _ffi.last_launches()
        assert forward.startswith('k_stft<512,magnitude'), forward
        if want is None:
            r = f32(cotangent(y.shape, False, seed=72))
            r[2] = 0.0
            xr = x0.to(torch.float64).requires_grad_(True)
            window = backend.get_window_fn(None)(n_fft).astype(np.float64)
            loss_of(spec_from_bcfk(ref_stft(to_bct(xr, fmt), n_fft, n_fft, hop, window, True, False), fmt).abs(), r).backward()
            want = xr.grad
        del seen[:]
        loss_of(y, r).backward()
        assert len(seen) == chunks, (step, seen)
        for _, log in seen:
            expect(labels_of(log), 'k_istft_fused<512>')
        measure('fused STFT -> Magnitude', xg.grad, want, 3e-4, '%s, chunks of %d' % (fmt, step))
        assert float(xg.grad[2].abs().max()) == 0.0
    kapre.check_device()


@pytest.mark.parametrize('bytes_', [1, None])
def test_mel_chain_backward_batch_one(monkeypatch, bytes_):
    n_fft, hop = 512, 128
    model = get_melspectrogram_layer(input_shape=(3000, 1), n_fft=n_fft, hop_length=hop, sample_rate=22050, n_mels=40,
                                     return_decibel=True, db_dynamic_range=60.0, input_data_format=CL, output_data_format=CL,
                                     pad_end=True)
    seen = record_launches(monkeypatch, 'istft')
    if bytes_:
        monkeypatch.setattr(autograd, 'CHAIN_RECOMPUTE_BYTES', bytes_)
    x0 = wave(1, 1, 3000, CL, seed=63)
    xg = x0.cuda().requires_grad_(True)
    y = model(xg)
    r = f32(cotangent(y.shape, False, seed=64))
    loss_of(y, r).backward()
    assert len(seen) == 1
    expect(labels_of(seen[0][1]), 'k_istft_fused<256>')
    measure('fused mel chain', xg.grad, mel_reference(model, x0, r, n_fft, hop, CL, True, 60.0), 3e-4, 'batch 1')
    kapre.check_device()


def test_mel_chain_backward_at_a_training_batch(monkeypatch):
    """64 x 1 s of 16 kHz audio, n_fft 400 / hop 160 / 80 mels, decibels, the chunk budget untouched (one chunk of 64): the
    recomputed chain runs its layers at 6400 frames -- STFT^T on the mixed-radix ring kernel (istft_ws_mr_plan), the matrix
    backward on k_gemm with 6400 rows, k_db_bwd with 64 items."""
    n_fft, hop, t = 400, 160, 16000
    model = get_melspectrogram_layer(input_shape=(t, 1), n_fft=n_fft, hop_length=hop, sample_rate=16000, n_mels=80,
                                     return_decibel=True, db_dynamic_range=60.0, input_data_format=CL, output_data_format=CL,
                                     pad_end=True)
    assert autograd.CHAIN_RECOMPUTE_BYTES == 256 << 20
    seen = record_launches(monkeypatch, 'istft', 'freq_matmul', 'mag_to_db_bwd')
    x0 = wave(64, 1, t, CL, seed=65)
    xg = x0.cuda().requires_grad_(True)
    y = model(xg)
    forward = _ffi.last_launches()
    assert 'k_mel_' in forward and 'k_stft' not in forward, forward              # the fused launch
    assert tuple(y.shape) == (64, 100, 80, 1)
    r = f32(cotangent(y.shape, False, seed=66))
    loss_of(y, r).backward()
    by_name = {}
    for name, log in seen:
        by_name.setdefault(name, []).append(labels_of(log))
    assert len(by_name['istft']) == 1
    expect(by_name['istft'][0], 'k_istft_ws_mr<200,')
    assert any(l[-1] == 'k_db_bwd' for l in by_name['mag_to_db_bwd'])
    assert any(l[-1] in ('k_gemm', 'k_thin_gemm') for l in by_name['freq_matmul'])
    measure('fused mel chain', xg.grad, mel_reference(model, x0, r, n_fft, hop, CL, True, 60.0), 3e-4, '64 x 1 s at 16 kHz')
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# the routes this file reached
# ---------------------------------------------------------------------------------------------
REQUIRED = ['k_istft_fused<', 'k_istft_ws<', 'k_istft_pw<', 'k_istft_pw_il<', 'k_istft_ws_mr<', 'k_ola', 'k_stft3<', 'k_stft3_cl<',
            'k_stft<', 'k_gemm', 'k_thin_gemm', 'k_cplx_to_real_bwd', 'k_spec_edge_scale', 'k_frame_bwd', 'k_energy_bwd',
            'k_delta_bwd', 'k_db_bwd']


def test_every_backward_route_was_reached_under_automatic_options():
    """runs last: the kernels the backward passes above launched with istft_path 0 / stft_variant 0.  A later change of a
    dispatch threshold that empties a section shows here."""
    if not SEEN_AUTO:
        pytest.skip('the cases above did not run in this session')
    print('grad gate worst error / limit per route:')
    for route in sorted(WORST):
        print('  %-46s %.4f' % (route, WORST[route]))
    missing = [p for p in REQUIRED if not any(l.startswith(p) for l in SEEN_AUTO)]
    assert not missing, (missing, sorted(SEEN_AUTO))
