"""numpy model of HPSS (kapre_amd.HPSS, kpr_hpss_f32 / kpr_hpss_c64): the exact medians with the library's edge rule, and the masks
of librosa's softmask evaluated in float64.  numpy only."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

TINY = 2.0 ** -126


def reflect_index(i, n):
    """r(i, n): j = i mod 2n (non-negative); j if j < n else 2n - 1 - j   (d c b a | a b c d | d c b a), for every n >= 1"""
    j = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def median_reflect(x, k, axis):
    """The k-tap (k odd) median of ``x`` along ``axis`` with the edge rule r().  A selection: np.partition orders NaN last, as
    numpy.sort does, and the result is one of the window's values in x's dtype."""
    assert k % 2 == 1 and k >= 1
    x = np.asarray(x)
    n = x.shape[axis]
    h = (k - 1) // 2
    padded = np.take(x, reflect_index(np.arange(-h, n + h), n), axis=axis)
    win = sliding_window_view(padded, k, axis=axis)                       # the window is the new last axis
    return np.partition(win, h, axis=-1)[..., h]


def softmask(X, R, power, both_margins_one=True):
    """librosa's softmask in the precision of X and R: Z = max(X, R); where Z < 2^-126 the mask is 0.5 (both margins 1) or 0"""
    X, R = np.asarray(X), np.asarray(R)
    if np.isinf(power):
        return (X > R).astype(X.dtype)
    Z = np.maximum(X, R)
    bad = Z < TINY
    Z = np.where(bad, 1, Z)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        a, c = (X / Z) ** power, (R / Z) ** power
        m = a / (a + c)
    return np.where(bad, 0.5 if both_margins_one else 0.0, m).astype(X.dtype)


def medians(S, kh, kp, time_axis=0, freq_axis=1):
    """(H, P) of a float32 array: the exact float32 medians along time and along frequency"""
    S = np.asarray(S, dtype=np.float32)
    return median_reflect(S, kh, time_axis), median_reflect(S, kp, freq_axis)


def hpss_model(S, kh, kp, power, mh, mp, mask, time_axis=0, freq_axis=1):
    """(harmonic, percussive) in float64 from the exact float32 medians of the float32 array S (any rank; the two axes named)"""
    H, P = medians(S, kh, kp, time_axis, freq_axis)
    H, P = H.astype(np.float64), P.astype(np.float64)
    one = mh == 1 and mp == 1
    Mh, Mp = softmask(H, P * mh, power, one), softmask(P, H * mp, power, one)
    if mask:
        return Mh, Mp
    S64 = np.asarray(S, dtype=np.float32).astype(np.float64)
    return S64 * Mh, S64 * Mp
