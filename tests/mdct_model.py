"""The float64 model of MDCT / InverseMDCT: the definition as a dense cosine product, its transpose and the overlap-add, plus
the fast form (fold, pre-twiddle, N/4-point complex FFT, post-twiddle) the kernels implement.  Plain numpy; the reference of
tests/test_mdct_host.py and tests/test_mdct_gpu.py.  Arrays are (..., time) and (..., frames, M): the series axis is last."""
import functools

import numpy as np


WINDOWS = {"sine": lambda N: np.sin(np.pi * (np.arange(N) + 0.5) / N),
           "vorbis": lambda N: np.sin(np.pi / 2 * np.sin(np.pi * (np.arange(N) + 0.5) / N) ** 2)}


def scales(N, norm):
    """(s, s') of the definition."""
    M = N // 2
    return (2.0, 1.0 / M) if norm is None else (np.sqrt(2.0 / M),) * 2


@functools.lru_cache(maxsize=None)
def basis(N):
    """C[n, k] = cos((2 pi / N)(n + 1/2 + M/2)(k + 1/2)), (N, M)."""
    M = N // 2
    n, k = np.arange(N)[:, None], np.arange(M)[None, :]
    return np.cos(2 * np.pi / N * (n + 0.5 + M / 2) * (k + 0.5))


def frame_count(time, N, pad_begin, pad_end):
    M = N // 2
    t = time + (M if pad_begin else 0)
    if pad_end:
        return (t + M - 1) // M
    return 0 if t < N else 1 + (t - N) // M


def frames_of(x, N, pad_begin, pad_end):
    """(..., T, N) frames of x at hop M, zeros outside the signal."""
    M = N // 2
    x = np.asarray(x, np.float64)
    T = frame_count(x.shape[-1], N, pad_begin, pad_end)
    pad = M if pad_begin else 0
    buf = np.zeros(x.shape[:-1] + (max((T + 1) * M, pad + x.shape[-1]),))
    buf[..., pad:pad + x.shape[-1]] = x
    return np.stack([buf[..., t * M:t * M + N] for t in range(T)], axis=-2) if T else np.zeros(x.shape[:-1] + (0, N))


def mdct(x, N, window, scale, pad_begin=False, pad_end=False):
    """X[..., t, k] = scale sum_n w[n] x[start_t + n] C[n, k]."""
    return scale * (frames_of(x, N, pad_begin, pad_end) * window) @ basis(N)


def overlap_add(y, length, pad_begin):
    """(..., T, N) frames at hop M -> (..., length); with pad_begin the first M samples are dropped."""
    T, N = y.shape[-2:]
    M = N // 2
    full = np.zeros(y.shape[:-2] + (max((T + 1) * M, length + M),))
    for t in range(T):
        full[..., t * M:t * M + N] += y[..., t, :]
    off = M if pad_begin else 0
    return full[..., off:off + length]


def _length(X, pad_begin, length):
    return (X.shape[-2] + 1 - bool(pad_begin)) * X.shape[-1] if length is None else length


def inverse_mdct(X, N, window, scale, pad_begin=False, length=None):
    """overlap-add of y_t[n] = scale w[n] sum_k X[t, k] C[n, k]; length defaults to (T + 1) M (minus M with pad_begin)."""
    X = np.asarray(X, np.float64)
    return overlap_add(scale * (X @ basis(N).T) * window, _length(X, pad_begin, length), pad_begin)


def mdct_fast(frame, window, scale):
    """The fast form on one frame of length N."""
    N = frame.shape[-1]
    M, Q = N // 2, N // 4
    a, b, c, d = np.split(frame * window, 4)
    u = np.concatenate([-c[::-1] - d, a - b[::-1]])
    n = np.arange(Q)
    v = (u[2 * n] + 1j * u[M - 1 - 2 * n]) * np.exp(-1j * np.pi * (4 * n + 1) / (4 * M))
    Y = np.fft.fft(v) * np.exp(-1j * np.pi * n / M)
    X = np.empty(M)
    X[2 * n] = scale * Y.real
    X[M - 1 - 2 * n] = -scale * Y.imag
    return X


def mdct_bound(x, N, window, scale, pad_begin=False, pad_end=False):
    """scale sum_n |w[n] x[n]| per frame, (..., T, 1): the forward error rule's magnitude."""
    return scale * np.abs(frames_of(x, N, pad_begin, pad_end) * window).sum(-1, keepdims=True)


def inverse_bound(X, N, window, scale, pad_begin=False, length=None):
    """scale |w[n]| sum_k |X[t, k]| summed over the frames that cover a sample."""
    X = np.asarray(X, np.float64)
    return overlap_add(scale * np.abs(X).sum(-1, keepdims=True) * np.abs(window), _length(X, pad_begin, length), pad_begin)
