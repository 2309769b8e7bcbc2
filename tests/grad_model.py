"""The gradient checker of the suite: the layer arithmetic written with plain torch float64 ops on the CPU and differentiated
by torch's own autograd (test infrastructure only, no kernel of the package runs here).  The HIP backward passes
(kapre_amd/autograd.py, csrc/kpr_grad_kernels.h and the forward kernels they reuse as adjoints) must give the same input
gradient for the same scalar loss <y, R> with a fixed random R.

tests/test_autograd.py and tests/test_grad_gate.py compare the device against these functions;
tests/test_grad_model_host.py pins the functions themselves (forward values against oracle/kapre_oracle.py, gradients against
central differences) on a machine without a GPU.
"""
import numpy as np
import torch

CL, CF = 'channels_last', 'channels_first'


def ref_stft(x_bct, n_fft, win, hop, window, pad_begin, pad_end):
    """tf.signal.stft as STFT.call drives it (time_frequency.py:164-182): (B, C, T) -> (B, C, F, K) complex128."""
    x = x_bct
    if pad_begin:
        x = torch.nn.functional.pad(x, (n_fft - hop, 0))
    t = x.shape[-1]
    if pad_end:
        n_frames = -(-t // hop)
        x = torch.nn.functional.pad(x, (0, max(0, (n_frames - 1) * hop + win - t)))
    frames = x.unfold(-1, win, hop) * torch.as_tensor(window, dtype=torch.float64)
    return torch.fft.rfft(frames, n=n_fft)


def ref_istft(spec_bcfk, n_fft, win, hop, synth):
    """tf.signal.inverse_stft (time_frequency.py:307-314): (B, C, F, K) -> (B, C, (F - 1) hop + win)."""
    y = torch.fft.irfft(spec_bcfk, n=n_fft)[..., :win] * torch.as_tensor(synth, dtype=torch.float64)
    b, c, f, _ = y.shape
    out = torch.zeros(b, c, (f - 1) * hop + win, dtype=torch.float64)
    for i in range(f):
        out[..., i * hop:i * hop + win] = out[..., i * hop:i * hop + win] + y[..., i, :]
    return out


def ref_istft_ola(spec_bcfk, n_fft, win, hop, synth):
    """ref_istft with the overlap-add as one index_add instead of a loop over the frames: the same sums (in another order),
    for launches of thousands of frames.  tests/test_grad_model_host.py holds it to ref_istft."""
    y = torch.fft.irfft(spec_bcfk, n=n_fft)[..., :win] * torch.as_tensor(synth, dtype=torch.float64)
    b, c, f, _ = y.shape
    idx = (torch.arange(f).reshape(-1, 1) * hop + torch.arange(win).reshape(1, -1)).reshape(-1)
    out = torch.zeros(b, c, (f - 1) * hop + win, dtype=torch.float64)
    return out.index_add(2, idx, y.reshape(b, c, f * win))


def chunked_grad(fn, x, r, chunk):
    """d<fn(x), r>/dx for an fn that treats batch entries independently, differentiated `chunk` entries at a time (bounds
    the checker's memory at the large shapes; x and r are split along their first axis)."""
    out = torch.empty_like(x)
    for i0 in range(0, x.shape[0], chunk):
        xr = x[i0:i0 + chunk].detach().clone().requires_grad_(True)
        loss_of(fn(xr), r[i0:i0 + chunk]).backward()
        out[i0:i0 + chunk] = xr.grad
    return out


def ref_db(x, ref_value, amin, dyn):
    """backend.magnitude_to_decibel (backend.py:186-192), items = batch entries."""
    log10 = lambda v: torch.log(v) / np.log(10.0)
    amin_t = torch.tensor(amin, dtype=x.dtype)
    l = 10.0 * log10(torch.maximum(x, amin_t)) - 10.0 * np.log10(max(amin, ref_value))
    m = l.reshape(l.shape[0], -1).amax(dim=1).reshape([-1] + [1] * (l.dim() - 1))
    return torch.maximum(l, m - dyn)


def ref_frame(x_bct, length, hop, pad_end, pad_value):
    """tf.signal.frame on the last axis: (B, C, T) -> (B, C, F, L)."""
    t = x_bct.shape[-1]
    if pad_end:
        n_frames = -(-t // hop)
        x_bct = torch.nn.functional.pad(x_bct, (0, max(0, (n_frames - 1) * hop + length - t)), value=pad_value)
    return x_bct.unfold(-1, length, hop)


def ref_delta(x, t_axis, win, mode):
    """Delta.call (time_frequency.py:614-635): tf.pad along the time axis `t_axis` of the rank-4 x, then the correlation with
    [-n .. n] / (2 sum i^2)."""
    n, t = (win - 1) // 2, x.shape[t_axis]
    if mode == 'constant':
        idx = np.arange(-n, t + n)
        valid = torch.as_tensor(((idx >= 0) & (idx < t)).astype(np.float64))
        idx = np.clip(idx, 0, t - 1)
    else:
        idx = np.pad(np.arange(t), n, mode=mode)
        valid = torch.ones(len(idx), dtype=torch.float64)
    xp = x.index_select(t_axis, torch.as_tensor(idx))
    vshape = [1, 1, 1, 1]
    vshape[t_axis] = len(idx)
    xp = xp * valid.reshape(vshape)
    denom = 2.0 * sum(i * i for i in range(1, n + 1))
    return sum(j * xp.narrow(t_axis, n + j, t) for j in range(-n, n + 1)) / denom


def to_bct(x, fmt):
    return x.permute(0, 2, 1) if fmt == CL else x


def spec_from_bcfk(s, fmt):
    return s.permute(0, 2, 3, 1) if fmt == CL else s


def spec_to_bcfk(s, fmt):
    return s.permute(0, 3, 1, 2) if fmt == CL else s


def loss_of(y, r):
    """<y, R> with R real; a complex y is viewed as (re, im) pairs."""
    if y.is_complex():
        y = torch.view_as_real(y)
    return (y * r.to(y.device, y.dtype)).sum()


def cotangent(shape, complex_, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape) + ((2,) if complex_ else ()), generator=g, dtype=torch.float64)


def check(got, want, tol, what):
    got = got.detach().cpu()
    if got.is_complex():
        got, want = torch.view_as_real(got.to(torch.complex128)), torch.view_as_real(want)
    got, want = got.to(torch.float64), want.to(torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(want.abs().max())
    assert scale > 0, what
    err = float((got - want).abs().max()) / scale
    assert err <= tol, '%s: max error %.3g of the largest gradient entry (limit %.1g)' % (what, err, tol)


def wave(batch, ch, t, fmt, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((batch, ch, t), generator=g, dtype=torch.float64) * 2 - 1
    x = x * torch.linspace(0.2, 1.0, batch, dtype=torch.float64).reshape(-1, 1, 1)      # items of different loudness
    x = (x.permute(0, 2, 1) if fmt == CL else x).contiguous()
    return x.to(dtype)
