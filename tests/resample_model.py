"""float64 numpy model of kapre_amd.signal.Resample -- the checker of tests/test_resample_host.py and test_resample_gpu.py.

    g = gcd(orig_freq, new_freq), orig = orig_freq / g, new = new_freq / g, base = rolloff min(orig, new), L = lowpass_filter_width
    h(tau) = (base / orig) sinc(base tau) cos^2(pi base tau / (2 L))   for |base tau| < L, else 0
    y[m]   = sum_n x[n] h(n / orig - m / new),   x[n] = 0 outside 0 <= n < T,   m = 0 .. ceil(new T / orig) - 1
    gx[n]  = sum_m gy[m] h(n / orig - m / new)                                  (the adjoint)

Banded: output i = b P + p (forward: P = new, Q = orig; adjoint: P = orig, Q = new) reads the inputs b Q + j with
|j P - p Q| < L max(orig, new) / rolloff, a loop over at most 2 L max / (rolloff P) + 3 taps -- O(T_out n_taps).  The offset
u = j P - p Q is an exact integer and base tau = +-rolloff u / max(orig, new).  ``dense`` is the T_out x T matrix of the
definition itself, for tiny cases.
"""
import math

import numpy as np


def reduced(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def out_length(T, orig_freq, new_freq):
    orig, new = reduced(orig_freq, new_freq)
    return -(-new * int(T) // orig)


def _h_of_t(t, scale, L):
    """scale sinc(t) cos^2(pi t / (2 L)) inside |t| < L, t = base tau"""
    t = np.asarray(t, dtype=np.float64)
    return np.where(np.abs(t) < L, scale * np.sinc(t) * np.cos(np.pi * t / (2.0 * L)) ** 2, 0.0)


def h(tau, orig_freq, new_freq, L=6, rolloff=0.99):
    orig, new = reduced(orig_freq, new_freq)
    base = rolloff * min(orig, new)
    return _h_of_t(base * np.asarray(tau, dtype=np.float64), base / orig, L)


def dense(T, orig_freq, new_freq, L=6, rolloff=0.99):
    """(T_out, T) matrix of the definition"""
    orig, new = reduced(orig_freq, new_freq)
    n = np.arange(T, dtype=np.float64)[None, :]
    m = np.arange(out_length(T, orig, new), dtype=np.float64)[:, None]
    return h(n / orig - m / new, orig, new, L, rolloff)


def bands(orig_freq, new_freq, L=6, rolloff=0.99, adjoint=False):
    """(P, Q, first, count): per output phase p the first input offset of its support and the number of inputs in it"""
    orig, new = reduced(orig_freq, new_freq)
    P, Q = (orig, new) if adjoint else (new, orig)
    U = L * max(orig, new) / rolloff
    p = np.arange(P, dtype=np.int64)
    first = np.floor((p * Q - U) / P).astype(np.int64) - 1
    last = np.ceil((p * Q + U) / P).astype(np.int64) + 1
    for _ in range(4):                                # walk to the strict support |j P - p Q| < U
        first = np.where(np.abs(first * P - p * Q) < U, first, first + 1)
        last = np.where(np.abs(last * P - p * Q) < U, last, last - 1)
    assert np.all(np.abs(first * P - p * Q) < U) and np.all(np.abs((first - 1) * P - p * Q) >= U)
    assert np.all(np.abs(last * P - p * Q) < U) and np.all(np.abs((last + 1) * P - p * Q) >= U)
    return P, Q, first, last - first + 1


def _gather(x, out_len, orig_freq, new_freq, L, rolloff, adjoint, absolute):
    """banded polyphase sum over the last axis of x; ``absolute``: sum of |coefficient * input| instead"""
    orig, new = reduced(orig_freq, new_freq)
    P, Q, first, count = bands(orig, new, L, rolloff, adjoint)
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    i = np.arange(out_len, dtype=np.int64)
    b, p = i // P, i % P
    scale, per_u = rolloff * min(orig, new) / orig, rolloff / max(orig, new)
    y = np.zeros(x.shape[:-1] + (out_len,), dtype=np.float64)
    for k in range(int(count.max()) if out_len else 0):
        j = first[p] + k
        n = b * Q + j
        c = _h_of_t((j * P - p * Q) * per_u, scale, L)
        ok = (n >= 0) & (n < T) & (k < count[p])
        term = np.where(ok, c, 0.0) * x[..., np.clip(n, 0, max(T - 1, 0))] if T else np.zeros_like(y)
        y += np.abs(term) if absolute else term
    return y


def resample(x, orig_freq, new_freq, L=6, rolloff=0.99, axis=-1):
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    y = _gather(x, out_length(x.shape[-1], orig_freq, new_freq), orig_freq, new_freq, L, rolloff, False, False)
    return np.moveaxis(y, -1, axis)


def adjoint(gy, T, orig_freq, new_freq, L=6, rolloff=0.99, axis=-1):
    """gx (length T along ``axis``) of the cotangent gy of resample(x of length T)"""
    gy = np.moveaxis(np.asarray(gy, dtype=np.float64), axis, -1)
    assert gy.shape[-1] == out_length(T, orig_freq, new_freq)
    return np.moveaxis(_gather(gy, int(T), orig_freq, new_freq, L, rolloff, True, False), -1, axis)


def abs_budget(x, orig_freq, new_freq, L=6, rolloff=0.99, axis=-1, adjoint=False, T=None):
    """sum_k |tab_k x_k| per output: of the forward pass, or with ``adjoint`` of the adjoint applied to x = gy (T: its output length)"""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    out_len = int(T) if adjoint else out_length(x.shape[-1], orig_freq, new_freq)
    return np.moveaxis(_gather(x, out_len, orig_freq, new_freq, L, rolloff, adjoint, True), -1, axis)


def upfirdn_reference(x, orig_freq, new_freq, L=6, rolloff=0.99):
    """the same conversion through scipy.signal.upfirdn (up = new, down = orig) with the prototype h(q / (orig new)): 1-D"""
    from scipy.signal import upfirdn
    orig, new = reduced(orig_freq, new_freq)
    x = np.asarray(x, dtype=np.float64)
    half = int(math.ceil(L * max(orig, new) / rolloff))              # |q| < L orig new / base
    q = np.arange(-half, half + 1, dtype=np.float64)
    proto = h(q / (orig * new), orig, new, L, rolloff)
    # y[m] = sum_n x[n] proto[m orig - n new + half] (h is even): sample m orig + half of the up-by-new convolution; zeros in
    # front of the prototype move that onto the grid of the decimation
    pad = (-half) % orig
    full = upfirdn(np.concatenate([np.zeros(pad), proto]), x, up=new, down=orig)
    start, n_out = (half + pad) // orig, out_length(x.shape[0], orig, new)
    out = np.zeros(n_out, dtype=np.float64)
    got = full[start:start + n_out]
    out[:got.shape[0]] = got
    return out
