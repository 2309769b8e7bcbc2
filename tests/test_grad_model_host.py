"""The gradient checker is itself checked (no GPU): tests/grad_model.py is what every backward pass of the package is compared
with, so its forward values must be the oracle's (oracle/kapre_oracle.py, 1e-12) and the gradients torch's autograd derives
from it must be the derivative of those values (central differences in float64 on 64-sample cases).
"""
import numpy as np
import pytest
import torch

import kapre_oracle as o
from grad_model import CL, CF, ref_stft, ref_istft, ref_istft_ola, chunked_grad, ref_db, ref_delta, ref_frame, to_bct, spec_from_bcfk, loss_of, cotangent, check, wave


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max()) / float(np.abs(want).max())
    assert err <= 1e-12, '%s: %.3g of the largest value' % (what, err)


@pytest.mark.parametrize('n_fft,win,hop,pad_begin,pad_end,ch,t', [(64, 64, 16, True, True, 2, 331), (100, 72, 25, False, False, 1, 400)])
def test_ref_stft_is_the_oracle(n_fft, win, hop, pad_begin, pad_end, ch, t):
    x = wave(2, ch, t, CF, seed=n_fft, dtype=torch.float64)
    window = o.get_window(None, win)
    got = ref_stft(x, n_fft, win, hop, window, pad_begin, pad_end)
    want = o.kapre_stft(x.numpy(), n_fft, win, hop, None, pad_begin, pad_end, CF, CF)
    _close(got.numpy(), want, 'ref_stft')
    # the layout helpers are the oracle's transposes
    want_cl = o.kapre_stft(to_bct(x, CL).numpy(), n_fft, win, hop, None, pad_begin, pad_end, CL, CL)
    _close(spec_from_bcfk(got, CL).numpy(), want_cl, 'ref_stft, channels_last')


@pytest.mark.parametrize('n_fft,win,hop,ch,frames', [(64, 64, 16, 2, 9), (100, 72, 18, 1, 7)])
def test_ref_istft_is_the_oracle(n_fft, win, hop, ch, frames):
    s = torch.view_as_complex(cotangent((2, ch, frames, n_fft // 2 + 1), True, seed=hop))
    synth = o.inverse_stft_window(win, hop, o.get_window(None, win))
    got = ref_istft(s, n_fft, win, hop, synth)
    want = o.kapre_istft(s.numpy(), n_fft, win, hop, None, CF, CF)
    _close(got.numpy(), want, 'ref_istft')


@pytest.mark.parametrize('shape,ref_value,amin,dyn', [((3, 7, 5, 2), 0.7, 1e-3, 15.0), ((2, 40), 1.0, 1e-5, 80.0)])
def test_ref_db_is_the_oracle(shape, ref_value, amin, dyn):
    g = torch.Generator().manual_seed(len(shape))
    x = torch.exp(3.0 * torch.randn(shape, generator=g, dtype=torch.float64)) * 1e-2          # some below amin
    got = ref_db(x, ref_value, amin, dyn)
    want = o.magnitude_to_decibel(x.numpy(), ref_value, amin, dyn)
    _close(got.numpy(), want, 'ref_db')
    if dyn < 80:
        assert float((got == got.reshape(shape[0], -1).amin(dim=1).reshape([-1] + [1] * (len(shape) - 1))).double().mean()) > 0.05


def _central_differences(fn, x, eps):
    """d fn / d x[i] for every entry of the float64 tensor x, fn scalar."""
    flat = x.detach().clone().reshape(-1)
    out = torch.zeros_like(flat)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + eps
        hi = float(fn(flat.reshape(x.shape)))
        flat[i] = keep - eps
        lo = float(fn(flat.reshape(x.shape)))
        flat[i] = keep
        out[i] = (hi - lo) / (2 * eps)
    return out.reshape(x.shape)


def _autograd(fn, x):
    xr = x.detach().clone().requires_grad_(True)
    fn(xr).backward()
    return xr.grad


def test_ref_stft_gradient_is_the_derivative():
    """Linear in x: central differences are exact up to the round-off of the two loss values (~1e-16 |L| / eps)."""
    x = wave(1, 1, 64, CF, seed=1, dtype=torch.float64)
    window = o.get_window(None, 12)
    r = cotangent((1, 1, 19, 9), True, seed=2)
    fn = lambda v: loss_of(ref_stft(v, 16, 12, 4, window, True, True), r)
    assert tuple(ref_stft(x, 16, 12, 4, window, True, True).shape) == (1, 1, 19, 9)
    check(_autograd(fn, x), _central_differences(fn, x, 1e-4), 1e-9, 'ref_stft: autograd against central differences')


def test_ref_istft_gradient_is_the_derivative():
    s = cotangent((1, 1, 13, 9), True, seed=3)                        # (re, im) pairs: 13 frames of 9 bins
    synth = o.inverse_stft_window(12, 4, o.get_window(None, 12))
    r = cotangent((1, 1, 12 * 4 + 12), False, seed=4)                 # 60 samples
    fn = lambda v: loss_of(ref_istft(torch.view_as_complex(v), 16, 12, 4, synth), r)
    got, want = _autograd(fn, s), _central_differences(fn, s, 1e-4)
    # irfft ignores the imaginary parts of DC and Nyquist: their derivative is exactly zero in both
    assert float(got[..., 0, 1].abs().max()) == 0.0 and float(got[..., 8, 1].abs().max()) == 0.0
    check(got, want, 1e-9, 'ref_istft: autograd against central differences')


def test_the_vectorised_overlap_add_and_the_chunked_gradient_are_the_plain_ones():
    s = torch.view_as_complex(cotangent((3, 2, 11, 33), True, seed=8))
    synth = o.inverse_stft_window(50, 16, o.get_window(None, 50))
    r = cotangent((3, 2, 10 * 16 + 50), False, seed=9)
    plain = lambda v: ref_istft(v, 64, 50, 16, synth)
    fast = lambda v: ref_istft_ola(v, 64, 50, 16, synth)
    _close(fast(s).numpy(), plain(s).numpy(), 'ref_istft_ola')
    want = _autograd(lambda v: loss_of(plain(v), r), s)
    for chunk in (1, 2, 3):
        got = chunked_grad(fast, s, r, chunk)
        _close(torch.view_as_real(got).numpy(), torch.view_as_real(want).numpy(), 'chunked gradient of ref_istft_ola')


def test_ref_frame_gradient_counts_the_covering_frames():
    x = wave(1, 2, 64, CF, seed=5, dtype=torch.float64)
    fn = lambda v: ref_frame(v, 12, 5, True, 0.25).sum()
    got = _autograd(fn, x)
    cover = np.zeros(64)
    for f in range(-(-64 // 5)):
        cover[f * 5:min(64, f * 5 + 12)] += 1
    np.testing.assert_array_equal(got.numpy(), np.broadcast_to(cover, (1, 2, 64)))


@pytest.mark.parametrize('mode', ['symmetric', 'reflect', 'constant'])
def test_ref_delta_is_the_oracle(mode):
    x = cotangent((2, 11, 5, 3), False, seed=10)                      # channels_last: time axis 1
    want = o.kapre_delta(x.numpy(), win_length=5, mode=mode, data_format=CL)
    _close(ref_delta(x, 1, 5, mode).numpy(), want, 'ref_delta')
    xf = x.permute(0, 3, 1, 2).contiguous()
    _close(ref_delta(xf, 2, 5, mode).numpy(), np.transpose(want, (0, 3, 1, 2)), 'ref_delta, channels_first')


def test_ref_db_gradient_is_the_derivative():
    """64 values in 2 items, dynamic range 15 dB: a share of each item sits on the floor and sends its cotangent to the item's
    maximum.  Every value is at least 1e-3 dB away from the floor and from the maximum (asserted), so a step of 1e-7 relative
    (4e-7 dB) crosses neither: the map is smooth on the segment and central differences carry an error of the order
    eps^2 f''' / 6 + 1e-16 |L| / eps, far below the 1e-6 asked here."""
    g = torch.Generator().manual_seed(6)
    x = torch.exp(2.0 * torch.randn((2, 8, 4), generator=g, dtype=torch.float64)) * 0.05
    ref_value, amin, dyn = 0.7, 1e-3, 15.0
    l = 10.0 * torch.log10(torch.clamp(x, min=amin)) - 10.0 * np.log10(ref_value)
    top = l.reshape(2, -1).amax(dim=1).reshape(2, 1, 1)
    others = l.reshape(2, -1).sort(dim=1).values[:, -2].reshape(2, 1, 1)
    assert float((top - others).min()) > 1e-3, 'the maximum of an item is not isolated by 1e-3 dB'
    assert float((l - (top - dyn)).abs().min()) > 1e-3, 'a value sits within 1e-3 dB of the floor'
    assert float((x - amin).abs().min() / amin) > 1e-3
    on_floor = (l < top - dyn).double().mean()
    assert 0.05 < float(on_floor) < 0.9
    r = cotangent(x.shape, False, seed=7)
    fn = lambda v: loss_of(ref_db(v, ref_value, amin, dyn), r)
    got = _autograd(fn, x)
    want = torch.zeros_like(x).reshape(-1)
    flat = x.clone().reshape(-1)
    for i in range(flat.numel()):                                     # steps relative to each value
        keep, eps = float(flat[i]), 1e-7 * float(flat[i])
        flat[i] = keep + eps
        hi = float(fn(flat.reshape(x.shape)))
        flat[i] = keep - eps
        lo = float(fn(flat.reshape(x.shape)))
        flat[i] = keep
        want[i] = (hi - lo) / (2 * eps)
    check(got, want.reshape(x.shape), 1e-6, 'ref_db: autograd against central differences')
    # the floor's cotangent arrives at the maximum: closed form
    for b in range(2):
        i = int(l[b].reshape(-1).argmax())
        floor_sum = float(r[b][l[b] < top[b] - dyn].sum())
        want_top = (float(r[b].reshape(-1)[i]) + floor_sum) * 10.0 / (np.log(10.0) * float(x[b].reshape(-1)[i]))
        assert abs(float(got[b].reshape(-1)[i]) - want_top) <= 1e-12 * abs(want_top)
