"""float64 numpy model of the table-free resampler (backend.resample(method='direct'), kpr_resample_direct_f32), written per
output, and the float32 restatement of the kernel's arithmetic -- the checkers of tests/test_resample_direct_host.py,
test_resample_direct_gpu.py and the pitch-shift tests.

    out[i] = s sum_j in[j] w(c (j P - i Q)),   in[j] = 0 outside 0 .. in_len - 1
    w(t)   = sinc(t) cos^2(pi t / (2 L)) for |t| < L, else 0;   c = rolloff / max(orig, new);   s = rolloff min(orig, new) / orig

with the rates reduced by their gcd; forward (P, Q) = (new, orig), adjoint (orig, new).  The position of output i is the
integer pair i Q = a P + r, 0 <= r < P; every output sums the window in[a - H + 1 + k], k = 0 .. n_taps - 1, n_taps = 2 H,
H = ceil(L max / (rolloff P)), at u = (k - H + 1) P - r, an exact int64.  The window holds the support |u| < L max / rolloff and
at most one input more at either end, where w is an exact 0.  Nothing here is sized by P: no per-phase arrays.

The error rule of the float32 kernel, per output:

    |y - y64| <= (n_taps + 3) 2^-24 sum_k |tap_k x_k| + C 2^-24 s sum_{k in support} |x_k| + 1e-37,   C = C_of(L) = 17 + 6 / L
"""
import math

import numpy as np

from resample_model import _h_of_t, out_length, reduced  # noqa: F401  (out_length and reduced are re-exported)


def C_of(L):
    """the constant of the rule's second term: derived in DESIGN 4.20 from the kernel's arithmetic, not fitted"""
    return 17.0 + 6.0 / L


def shape(orig_freq, new_freq, L=6, rolloff=0.99, adjoint=False):
    """(P, Q, H, n_taps, c, s): H in the float64 operations of the library (L * max / rolloff / P, then ceil)"""
    orig, new = reduced(orig_freq, new_freq)
    P, Q = (orig, new) if adjoint else (new, orig)
    mx, mn = max(orig, new), min(orig, new)
    H = int(math.ceil(float(L) * float(mx) / rolloff / float(P)))
    return P, Q, H, 2 * H, rolloff / mx, rolloff * mn / orig


def positions(n_out, P, Q, first=0):
    """(a, r) int64 with i Q = a P + r for i = first .. first + n_out - 1 (i Q < 2^62)"""
    iq = np.arange(first, first + n_out, dtype=np.int64) * np.int64(Q)
    a = iq // np.int64(P)
    return a, iq - a * np.int64(P)


def support_range(n_out, orig_freq, new_freq, L=6, rolloff=0.99, adjoint=False):
    """(lo, hi) int64 per output: the first and the last input j with |j P - i Q| < L max / rolloff"""
    P, Q, H, n_taps, c, s = shape(orig_freq, new_freq, L, rolloff, adjoint)
    a, r = positions(int(n_out), P, Q)
    U = L * max(reduced(orig_freq, new_freq)) / rolloff
    lo = np.full(a.shape, np.iinfo(np.int64).max, dtype=np.int64)
    hi = np.full(a.shape, np.iinfo(np.int64).min, dtype=np.int64)
    for k in range(n_taps):
        inside = np.abs(np.int64(k - H + 1) * np.int64(P) - r) < U
        j = a - H + 1 + k
        lo = np.where(inside, np.minimum(lo, j), lo)
        hi = np.where(inside, np.maximum(hi, j), hi)
    return lo, hi


def _window(x, a, k, H):
    """in[a - H + 1 + k] along the last axis of x, 0 outside it"""
    T = x.shape[-1]
    j = a - H + 1 + k
    ok = (j >= 0) & (j < T)
    if T == 0:
        return np.zeros(x.shape[:-1] + a.shape, dtype=x.dtype)
    return np.where(ok, x[..., np.clip(j, 0, T - 1)], x.dtype.type(0))


def _gather(x, out_len, orig_freq, new_freq, L, rolloff, adjoint, mode):
    """mode 'sum': the model; 'abs': sum_k |tap_k x_k|; 'support': s sum_{k in support} |x_k|"""
    P, Q, H, n_taps, c, s = shape(orig_freq, new_freq, L, rolloff, adjoint)
    x = np.asarray(x, dtype=np.float64)
    a, r = positions(int(out_len), P, Q)
    y = np.zeros(x.shape[:-1] + (int(out_len),), dtype=np.float64)
    for k in range(n_taps):
        u = np.int64(k - H + 1) * np.int64(P) - r
        t = u.astype(np.float64) * c
        xk = _window(x, a, k, H)
        if mode == 'support':
            y += np.where(np.abs(t) < L, s, 0.0) * np.abs(xk)
        else:
            term = _h_of_t(t, s, L) * xk
            y += np.abs(term) if mode == 'abs' else term
    return y


def resample(x, orig_freq, new_freq, L=6, rolloff=0.99, axis=-1, length=None):
    """the forward pass along ``axis``: ``length`` outputs, the natural ceil(new T / orig) when None"""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    n = out_length(x.shape[-1], orig_freq, new_freq) if length is None else int(length)
    return np.moveaxis(_gather(x, n, orig_freq, new_freq, L, rolloff, False, 'sum'), -1, axis)


def adjoint(gy, T, orig_freq, new_freq, L=6, rolloff=0.99, axis=-1):
    """gx (length T along ``axis``) of the cotangent gy of resample(x of length T, any ``length``)"""
    gy = np.moveaxis(np.asarray(gy, dtype=np.float64), axis, -1)
    return np.moveaxis(_gather(gy, int(T), orig_freq, new_freq, L, rolloff, True, 'sum'), -1, axis)


def budgets(x, out_len, orig_freq, new_freq, L=6, rolloff=0.99, adjoint=False):
    """(sum_k |tap_k x_k|, s sum_{k in support} |x_k|) per output, along the last axis"""
    return (_gather(x, out_len, orig_freq, new_freq, L, rolloff, adjoint, 'abs'),
            _gather(x, out_len, orig_freq, new_freq, L, rolloff, adjoint, 'support'))


def bound(x, out_len, orig_freq, new_freq, L=6, rolloff=0.99, adjoint=False, C=None):
    """the error rule per output; ``C`` None: C_of(L)"""
    n_taps = shape(orig_freq, new_freq, L, rolloff, adjoint)[3]
    tap_budget, support_budget = budgets(x, out_len, orig_freq, new_freq, L, rolloff, adjoint)
    C = C_of(L) if C is None else C
    return (n_taps + 3) * 2.0 ** -24 * tap_budget + C * 2.0 ** -24 * support_budget + 1e-37


def dense(T, orig_freq, new_freq, L=6, rolloff=0.99, length=None):
    """(length, T) matrix of the definition itself, for tiny cases"""
    P, Q, H, n_taps, c, s = shape(orig_freq, new_freq, L, rolloff, False)
    n = out_length(T, orig_freq, new_freq) if length is None else int(length)
    j = np.arange(T, dtype=np.int64)[None, :]
    i = np.arange(n, dtype=np.int64)[:, None]
    return _h_of_t((j * P - i * Q).astype(np.float64) * c, s, L)


# ---- the kernel's arithmetic in float32 on the CPU ----------------------------------------------------------------------
def _f32(v):
    return np.asarray(v, dtype=np.float32)


def taps_f32(phi, d, beta, scale, inv_2l, L):
    """tap of the float32 phase ``phi`` at the window offset ``d`` (an integer): the kernel's operations one by one, sinpi and
    cospi being the correctly rounded ones"""
    xk = _f32(np.float32(d) - phi)
    t = _f32(beta * xk)
    sp = _f32(np.sin(np.pi * (t.astype(np.float64) - np.rint(t.astype(np.float64)))) * np.where(np.rint(t) % 2 == 0, 1.0, -1.0))
    cw = _f32(np.cos(np.pi * _f32(t * inv_2l).astype(np.float64)))
    den = _f32(np.float32(np.pi) * t)
    with np.errstate(divide='ignore', invalid='ignore'):
        sinc = np.where(t == 0, np.float32(1), _f32(sp / den))
    w = _f32(sinc * _f32(cw * cw))
    return np.where(np.abs(t) < np.float32(L), _f32(scale * w), np.float32(0)).astype(np.float32)


def resample_f32(x, out_len, orig_freq, new_freq, L=6, rolloff=0.99, adjoint=False, float_position=False):
    """the float32 restatement: exact integer position, phi = r / P rounded once, per-tap evaluation, FMA sums in ascending k
    from 0.  ``float_position``: the mistake the rule has to catch -- the position i Q / P in float32 arithmetic."""
    P, Q, H, n_taps, c, s = shape(orig_freq, new_freq, L, rolloff, adjoint)
    x = _f32(x)
    mx = max(reduced(orig_freq, new_freq))
    beta, scale, inv_2l = np.float32(rolloff * P / mx), np.float32(s), np.float32(1.0 / (2.0 * L))
    if float_position:
        pos = _f32(_f32(np.arange(int(out_len), dtype=np.float32) * np.float32(Q)) / np.float32(P))
        fl = np.floor(pos)
        a, phi = fl.astype(np.int64), _f32(pos - fl)
    else:
        a, r = positions(int(out_len), P, Q)
        phi = _f32(r.astype(np.float64) * (1.0 / float(P)))
    acc = np.zeros(x.shape[:-1] + (int(out_len),), dtype=np.float32)
    for k in range(n_taps):
        tap = taps_f32(phi, k - H + 1, beta, scale, inv_2l, L)
        xk = _window(x, a, k, H)
        # one rounding per step: the product of two float32 is exact in float64
        acc = _f32(acc.astype(np.float64) + tap.astype(np.float64) * xk.astype(np.float64))
    return acc
