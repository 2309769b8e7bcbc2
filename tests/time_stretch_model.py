"""Float64 models of the phase vocoder (kapre_amd.TimeStretch, kpr_time_stretch_c64) in numpy.  Time is axis 0 of every array.

  textbook(X, rate, hop_length)   torchaudio.functional.phase_vocoder's formula: wrapped phase increments around the expected
                                  advance adv_f = pi hop f / (n_freq - 1), accumulated from angle X[0]
  definition(X, idx, alpha)       the package's definition: 32-bit angle words, summed sequentially in uint32
  phase_words(theta_words, idx)   that recurrence alone, from given angle words
  bound(X, idx, alpha)            the first-order error bound per output bin, and the phase part of it in half turns

The two agree because wrap() changes its argument by a whole number of turns and the output depends on the accumulated phase
modulo 2 pi only: adv, and with it the hop length, drops out of the definition."""
import numpy as np

U = 2.0 ** -24                      # float32 unit roundoff
ATAN2_ULPS = 6.0                    # OpenCL's limit for atan2 (full profile), which the device library is built to


def table(frames, rate):
    """(idx, alpha) by the definition: s = t * float64(rate), idx = floor(s), alpha = float32(s - idx) kept below 1, for the
    t >= 0 with floor(s) <= frames - 1"""
    rate = float(rate)
    idx, alpha, t = [], [], 0
    while frames > 0:
        s = t * rate
        i = int(np.floor(s))
        if i > frames - 1:
            break
        idx.append(i)
        alpha.append(min(np.float32(s - i), np.nextafter(np.float32(1), np.float32(0))))
        t += 1
    return np.asarray(idx, np.int32), np.asarray(alpha, np.float32)


def _padded(X):
    """X with the two zero frames X[T], X[T + 1] behind it"""
    return np.concatenate([X, np.zeros((2,) + X.shape[1:], X.dtype)], axis=0)


def _bcast(a, like):
    return np.asarray(a, np.float64).reshape((-1,) + (1,) * (like.ndim - 1))


def textbook(X, rate, hop_length):
    """(T, n_freq) complex -> (T', n_freq) complex128, the frequency axis being axis 1"""
    X = np.asarray(X, np.complex128)
    idx, alpha = table(X.shape[0], rate)
    n_freq = X.shape[1]
    adv = np.pi * hop_length * np.arange(n_freq) / max(n_freq - 1, 1)
    adv = adv.reshape((1, n_freq) + (1,) * (X.ndim - 2))
    Xp = _padded(X)
    x0, x1 = Xp[idx], Xp[idx + 1]
    a = _bcast(alpha, X)
    mag = a * np.abs(x1) + (1.0 - a) * np.abs(x0)
    step = np.angle(x1) - np.angle(x0) - adv
    step = step - 2.0 * np.pi * np.round(step / (2.0 * np.pi)) + adv
    first = np.angle(Xp[:1])
    acc = np.cumsum(np.concatenate([first, step[:-1]], axis=0), axis=0) if len(idx) else step
    return mag * np.exp(1j * acc)


def half_turns(X):
    """the angle of every bin in half turns, float64, in [-1, 1]; 0 for a zero or non-finite bin"""
    X = np.asarray(X, np.complex128)
    ok = np.isfinite(X.real) & np.isfinite(X.imag) & (X != 0)
    with np.errstate(invalid='ignore'):
        return np.where(ok, np.angle(np.where(ok, X, 1.0)) / np.pi, 0.0)


def angle_words(X):
    """Theta of every bin from the float64 angle: 2 rint(theta 2^30 / pi) as uint32"""
    w = np.rint(half_turns(X) * 2.0 ** 30).astype(np.int64) * 2
    return (w % 2 ** 32).astype(np.uint32)


def phase_words(theta_words, idx):
    """P[0] = Theta[0]; P[t + 1] = P[t] + Theta[idx[t] + 1] - Theta[idx[t]], sequentially in uint32 (rows behind the last are 0)"""
    th = _padded(np.asarray(theta_words, np.uint32))
    P = np.zeros((len(idx),) + th.shape[1:], np.uint32)
    acc = th[0].copy()
    for t, i in enumerate(idx):
        P[t] = acc
        acc = acc + th[i + 1] - th[i]                                   # uint32 arrays: wraps
    return P


def words_to_half_turns(P):
    return np.asarray(P, np.uint32).view(np.int32).astype(np.float64) * 2.0 ** -31


def magnitudes(X, idx, alpha):
    X = np.asarray(X, np.complex128)
    Xp = _padded(X)
    a = _bcast(alpha, X)
    with np.errstate(invalid='ignore'):
        return a * np.abs(Xp[np.asarray(idx) + 1]) + (1.0 - a) * np.abs(Xp[idx])


def definition(X, idx, alpha, words=True):
    """The definition in float64.  ``words``: the angles rounded to 32-bit words and summed in uint32 (what the device does);
    without, the same sum over the unrounded angles in float64 -- what the error bound is stated against."""
    X = np.asarray(X, np.complex128)
    if words:
        h = words_to_half_turns(phase_words(angle_words(X), idx))
    else:
        th = _padded(half_turns(X))
        h = np.zeros((len(idx),) + th.shape[1:])
        acc = th[0].copy()
        for t, i in enumerate(idx):
            h[t] = acc
            acc = acc + th[i + 1] - th[i]
    return magnitudes(X, idx, alpha) * np.exp(1j * np.pi * h)


def angle_bound(X):
    """e_Theta per bin in half turns: 6 ulp of atan2f, taken as 6 * 2^-24 |theta| / pi, and the rounding to a word, 2^-31"""
    return ATAN2_ULPS * U * np.abs(half_turns(X)) + 2.0 ** -31


def coefficients(n_rows, idx):
    """K[t, i]: the coefficient of Theta(X[i]) in P[t] after cancellation, (len(idx), n_rows + 2) integers"""
    K = np.zeros((len(idx), n_rows + 2), np.int64)
    k = np.zeros(n_rows + 2, np.int64)
    k[0] = 1
    for t, i in enumerate(idx):
        K[t] = k
        k[i + 1] += 1
        k[i] -= 1
    return K


def bound(X, idx, alpha):
    """(output bound, phase bound in half turns) per output bin:
    phase error <= sum_i |k_i| e_Theta(X[i]) + 2^-25 (the conversion of the word to a float32 h);
    output error <= m pi (phase error) + 4 * 2^-24 (|X[i_t]| + |X[i_t + 1]|): magnitudes, interpolation, sincospif"""
    X = np.asarray(X, np.complex128)
    e = _padded(angle_bound(X))
    K = np.abs(coefficients(X.shape[0], idx)).astype(np.float64)
    phase = np.tensordot(K, e, axes=(1, 0)) + 2.0 ** -25
    Xp = np.abs(_padded(X))
    idx = np.asarray(idx)
    m = magnitudes(X, idx, alpha)
    return m * np.pi * phase + 4.0 * U * (Xp[idx] + Xp[idx + 1]), phase


def random_spectrum(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
