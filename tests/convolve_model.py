"""Models of kapre_amd.Convolve / backend.fftconvolve -- the checkers of tests/test_convolve_host.py and test_convolve_gpu.py.

Partitioned overlap-save with block length L (n_fft = 2 L, hop L, P = ceil(len(h) / L) partitions):

    X_k    = rfft(x[(k - 1) L ... (k + 1) L)),  k = 0 ... K_in - 1,  K_in = ceil((T + L) / L)      (x = 0 outside [0, T))
    H_p    = rfft(h[p L ... (p + 1) L), n = 2 L)
    Y_k[f] = sum_{p < P} X_{k - p}[f] H_p[f],   k = 0 ... K_out - 1,  K_out = ceil((T + len(h) - 1) / L)   (X = 0 outside [0, K_in))
    y[k L ... (k + 1) L) = the second half of irfft(Y_k)

``overlap_save64`` is that in float64 (equal to np.convolve to round-off: the identity itself); ``overlap_save32`` the same
partitioning with scipy.fft on float32 input, a complex64 table rounded once from float64 and complex64 sums in ascending p --
a float32 implementation by other means, the yardstick of the end-to-end tests.  ``spec_fir64`` is the middle step alone with the
budget of the kernel's bound, ``index_draw`` the numpy restatement of kpr_index_draw.
"""
import numpy as np
import scipy.fft

from augment_model import mulhi32, philox4x32_10

# (T, len(h), L) on which the identity is checked
IDENTITY_SHAPES = ((1000, 1, 256), (1000, 300, 256), (5000, 8000, 256), (16384, 4097, 1024), (255, 257, 256), (3, 700, 256))


def frame_counts(t, n, L):
    """(K_in, K_out, P)"""
    return -(-(t + L) // L), -(-(t + n - 1) // L), -(-n // L)


def _frames(x, L, k_in):
    """(..., k_in, 2 L): frame k = x[(k - 1) L ... (k + 1) L), zero outside x"""
    t = x.shape[-1]
    pad = np.zeros(x.shape[:-1] + ((k_in + 1) * L,), dtype=x.dtype)
    pad[..., L:L + t] = x
    return np.stack([pad[..., k * L:(k + 2) * L] for k in range(k_in)], axis=-2)


def table64(h, L):
    """complex128 (P, L + 1)"""
    h = np.asarray(h, dtype=np.float64)
    P = -(-h.shape[-1] // L)
    pad = np.zeros(P * L)
    pad[:h.shape[-1]] = h
    return np.fft.rfft(pad.reshape(P, L), n=2 * L, axis=-1)


def fir(X, H, k_out):
    """Y[..., k, f] = sum_p X[..., k - p, f] H[p, f] in ascending p, in the dtype of X and H"""
    k_in, P = X.shape[-2], H.shape[0]
    Y = np.zeros(X.shape[:-2] + (k_out, X.shape[-1]), dtype=np.result_type(X.dtype, H.dtype))
    for p in range(P):
        n = min(k_out - p, k_in)
        if n > 0:
            Y[..., p:p + n, :] += X[..., :n, :] * H[p]
    return Y


def overlap_save64(x, h, L):
    """float64: the full convolution of x (..., T) with h (len,) along the last axis, T + len - 1 samples"""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    t, n = x.shape[-1], h.shape[-1]
    k_in, k_out, _ = frame_counts(t, n, L)
    X = np.fft.rfft(_frames(x, L, k_in), axis=-1)
    Y = fir(X, table64(h, L), k_out)
    y = np.fft.irfft(Y, n=2 * L, axis=-1)[..., L:]
    return y.reshape(y.shape[:-2] + (k_out * L,))[..., :t + n - 1]


def overlap_save32(x, h, L):
    """The same partitioning in float32: scipy.fft on float32 / complex64 data (which it keeps), the table rounded once"""
    x = np.asarray(x, dtype=np.float32)
    t, n = x.shape[-1], np.shape(h)[-1]
    k_in, k_out, _ = frame_counts(t, n, L)
    X = scipy.fft.rfft(_frames(x, L, k_in), axis=-1)
    assert X.dtype == np.complex64
    Y = fir(X, table64(h, L).astype(np.complex64), k_out)
    assert Y.dtype == np.complex64
    y = scipy.fft.irfft(Y, n=2 * L, axis=-1)[..., L:]
    assert y.dtype == np.float32
    return y.reshape(y.shape[:-2] + (k_out * L,))[..., :t + n - 1]


def figure(y, y64, h, x):
    """max |y - y64| / (||h||_1 max |x|) over one item"""
    scale = float(np.sum(np.abs(np.asarray(h, dtype=np.float64))) * np.max(np.abs(np.asarray(x, dtype=np.float64))))
    d = float(np.max(np.abs(np.asarray(y, dtype=np.float64) - y64))) if np.size(y64) else 0.0
    return d / scale if scale > 0 else d


def spec_fir64(X, H, idx, frames_out, band_div=1):
    """The kernel's definition in float64 on the contiguous (outer, frames_in, inner) problem: X complex (items, per_item,
    frames_in, inner) -- per_item outer items share the filter of their batch item -- H complex (n_ir, P, n_freq), idx (items,)
    integers or None, the bin of inner index i being i // band_div.  Returns (Y, budget_re, budget_im) with

        budget_re = sum_p |Xr| |Hr| + |Xi| |Hi|,   budget_im = sum_p |Xr| |Hi| + |Xi| |Hr|

    so that a float32 FMA chain of the 2 P terms obeys |re(Y) - re(Y64)| <= (2 P + 1) 2^-24 budget_re + 2^-149 (each of the 2 P
    roundings is relative to a partial sum bounded by the budget; one more unit covers second-order terms)."""
    X = np.asarray(X, dtype=np.complex128)
    H = np.asarray(H, dtype=np.complex128)
    items, per_item, k_in, inner = X.shape
    n_ir, P, _ = H.shape
    sel = np.zeros(items, dtype=np.int64) if idx is None else np.clip(np.asarray(idx, dtype=np.int64), 0, n_ir - 1)
    bins = np.arange(inner) // band_div
    Y = np.zeros((items, per_item, frames_out, inner), dtype=np.complex128)
    bre = np.zeros(Y.shape)
    bim = np.zeros(Y.shape)
    for p in range(P):
        n = min(frames_out - p, k_in)
        if n <= 0:
            continue
        Hp = H[sel][:, p][:, bins][:, None, None, :]                     # (items, 1, 1, inner)
        Xs = X[:, :, :n, :]
        Y[:, :, p:p + n] += Xs * Hp
        bre[:, :, p:p + n] += np.abs(Xs.real) * np.abs(Hp.real) + np.abs(Xs.imag) * np.abs(Hp.imag)
        bim[:, :, p:p + n] += np.abs(Xs.real) * np.abs(Hp.imag) + np.abs(Xs.imag) * np.abs(Hp.real)
    return Y, bre, bim


def index_draw(seed, calls, n_items, n_choices):
    """int32 (n_items,): Philox4x32-10 with counter (item, 0, calls_lo, calls_hi) and key (seed_lo, seed_hi); word 0 times
    n_choices, shifted right by 32"""
    seed, calls = int(seed) & (2 ** 64 - 1), int(calls) & (2 ** 64 - 1)
    item = np.arange(n_items, dtype=np.uint64)
    r = philox4x32_10((item, 0, calls & 0xFFFFFFFF, calls >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return mulhi32(r[0], n_choices).astype(np.int32)
