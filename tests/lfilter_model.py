"""float64 model of kapre_amd.signal.LFilter -- the checker of tests/test_lfilter_host.py and test_lfilter_gpu.py.

One section, coef = (b0, b1, b2, a1, a2) (already divided by a0), zero initial state, along the LAST axis:

    y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2]          (``reverse``: the same on the flipped axis)

The model has no loop of its own: y64 = scipy.signal.lfilter(b, a, x.astype(float64)).  Next to it, the per-sample budget

    loc[t] = |b0 x[t]| + |b1 x[t-1]| + |b2 x[t-2]| + |a1 y64[t-1]| + |a2 y64[t-2]|,    bud = |g| * loc

with g the impulse response of 1 / A(z) at full length: loc is the magnitude every rounding of one step is relative to, and
every rounding travels on to the later samples through 1 / A(z).  The parity rule for a float32 result y of float64 arithmetic:

    |y - y64| <= 2^-24 |y64| + K 2^-53 bud + 2^-149,    K = 32

(one rounding to float32; K counts the float64 roundings that reach a sample to first order: five multiply-adds in the kernel,
the same five in the reference, at most four levels of carry combination at four operations each, rounded up).
"""
import numpy as np
import scipy.signal

K = 32

PREEMPHASIS = (1.0, -0.97, 0.0, 0.0, 0.0)
DEEMPHASIS = (1.0, 0.0, 0.0, -0.97, 0.0)


def coef_of(sos_row):
    r = np.asarray(sos_row, dtype=np.float64).reshape(6)
    return tuple(float(v) for v in np.concatenate([r[:3], r[4:]]) / r[3])


def test_filters():
    """name -> (b0, b1, b2, a1, a2) of the filters the issue names, float64"""
    from kapre_amd.backend import biquad_sos
    rbj = lambda kind, fs, f, q: coef_of(biquad_sos(kind, fs, f, q)[0])
    return {
        'hp5': rbj('highpass', 48000, 5, 0.7071),
        'hp20': rbj('highpass', 48000, 20, 0.7071),
        'hp80': rbj('highpass', 16000, 80, 0.7071),
        'lp100q8': rbj('lowpass', 44100, 100, 8),
        'lp4000': rbj('lowpass', 16000, 4000, 0.7071),
        'lp30dbl': rbj('lowpass', 48000, 30, 0.5),
        'bs1770': (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585),
        'allpass': rbj('allpass', 44100, 1000, 0.7071),
        'preemph': PREEMPHASIS,
        'deemph': DEEMPHASIS,
        'gain': (2.0, 0.0, 0.0, 0.0, 0.0),
        'delay': (0.0, 0.0, 1.0, 0.0, 0.0),
    }


test_filters.__test__ = False          # a table, not a test


def _ba(coef):
    b0, b1, b2, a1, a2 = (float(v) for v in coef)
    return np.array([b0, b1, b2]), np.array([1.0, a1, a2])


def lfilter(x, coef, reverse=False):
    """y64 along the last axis"""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] == 0:
        return x.copy()
    b, a = _ba(coef)
    if reverse:
        return scipy.signal.lfilter(b, a, x[..., ::-1], axis=-1)[..., ::-1].copy()
    return scipy.signal.lfilter(b, a, x, axis=-1)


def impulse(coef, n):
    """g[0 ... n-1] of 1 / A(z)"""
    d = np.zeros(n, dtype=np.float64)
    if n:
        d[0] = 1.0
    return scipy.signal.lfilter([1.0], _ba(coef)[1], d)


def budget(x, y64, coef, reverse=False):
    """bud = |g| * loc along the last axis"""
    x, y64 = np.asarray(x, dtype=np.float64), np.asarray(y64, dtype=np.float64)
    n = x.shape[-1]
    if n == 0:
        return np.zeros_like(x)
    if reverse:
        return budget(x[..., ::-1], y64[..., ::-1], coef)[..., ::-1].copy()
    b0, b1, b2, a1, a2 = (float(v) for v in coef)

    def sh(v, k):
        out = np.zeros_like(v)
        if k < n:
            out[..., k:] = v[..., :n - k]
        return out

    loc = (np.abs(b0 * x) + np.abs(b1 * sh(x, 1)) + np.abs(b2 * sh(x, 2)) + np.abs(a1 * sh(y64, 1)) + np.abs(a2 * sh(y64, 2)))
    g = np.abs(impulse(coef, n))
    if a1 == 0.0 and a2 == 0.0:
        return loc
    bud = scipy.signal.fftconvolve(loc, g.reshape((1,) * (loc.ndim - 1) + (n,)), axes=-1)[..., :n]
    # (the FFT's own error is relative to the largest product: far below the budget, which is >= loc since g[0] = 1)
    return np.maximum(bud, loc)


def worst_ratio(y, x, coef, reverse=False, y64=None):
    """max over the elements of |y - y64| / (2^-24 |y64| + K 2^-53 bud + 2^-149): the parity rule holds when it is <= 1.  Non-finite
    values of y count as a ratio of inf."""
    y = np.asarray(y)
    if y.size == 0:
        return 0.0
    if y64 is None:
        y64 = lfilter(x, coef, reverse)
    bud = budget(x, y64, coef, reverse)
    bound = 2.0 ** -24 * np.abs(y64) + K * 2.0 ** -53 * bud + 2.0 ** -149
    r = np.abs(y.astype(np.float64) - y64) / bound
    return float(np.max(np.where(np.isfinite(r), r, np.inf)))


def cascade(x, coefs, reverse=False, zero_phase=False):
    """float32 in, float32 out: every section's output rounded to float32, as the library does between launches"""
    y = np.asarray(x, dtype=np.float32)
    for c in coefs:
        y = lfilter(y, c, reverse and not zero_phase).astype(np.float32)
    if zero_phase:                                               # the whole cascade forward, then the whole cascade in reverse
        for c in coefs:
            y = lfilter(y, c, True).astype(np.float32)
    return y


def carry_decimal(coef, n, digits=80):
    """M_n = [[g[n], -a2 g[n-1]], [g[n-1], -a2 g[n-2]]] from the recurrence in ``decimal`` at ``digits`` digits, started from
    the float64 coefficients; entries as Decimal, row-major"""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        D = decimal.Decimal
        a1, a2 = D(float(coef[3])), D(float(coef[4]))
        if n == 0:
            return [D(1), D(0), D(0), D(1)]
        g0, g1, g2 = D(1), D(0), D(0)
        for _ in range(n):
            g0, g1, g2 = -a1 * g0 - a2 * g1, g0, g1
        return [g0, -a2 * g1, g1, (-a2 * g2 if n > 1 else D(0))]


def carries_longdouble(coef, lengths):
    """{n: M_n as a (2, 2) numpy longdouble array} from the impulse response run in numpy's long double"""
    a1, a2 = np.longdouble(float(coef[3])), np.longdouble(float(coef[4]))
    top = max(lengths)
    g = np.zeros(top + 3, dtype=np.longdouble)               # g[k + 2] holds g[k]; g[-1] = g[-2] = 0
    g[2] = 1
    for k in range(1, top + 1):
        g[k + 2] = -a1 * g[k + 1] - a2 * g[k]
    out = {}
    for n in lengths:
        out[n] = (np.eye(2, dtype=np.longdouble) if n == 0 else
                  np.array([[g[n + 2], -a2 * g[n + 1]], [g[n + 1], -a2 * g[n]]], dtype=np.longdouble))
    return out


def chunked_scan(x, coef, lane=16, lanes=64, waves=4, seg_steps=2, segmented=False, reverse=False, carries=None):
    """The library's chunked scan in numpy float64, one series (1-D).  Lanes of ``lane`` samples run the transposed direct form
    II (y = b0 x + z1; z1' = b1 x - a1 y + z2; z2' = b2 x - a2 y) from the zero state; a log-step scan with the matrices of
    lane 2^k samples over the ``lanes`` lanes of a wave; the waves chained with the matrix of lane lanes samples, the steps
    chained through the carry; every sample run again from its lane's carry-in.  ``segmented``: segments of ``seg_steps`` steps
    scanned from the zero state first and chained with the segment's matrix.  The state travels as
    w = (z1 + sigma z2, -sigma z2), sigma = +1 for a1 <= 0 and -1 otherwise, and the matrices are (T M_n T^-1)^T with
    T = [[1, 0], [1, -sigma]], rounded to float64 (``carries``: {n: M_n}, default ``carries_longdouble``).  float64 out."""
    x = np.asarray(x, dtype=np.float64)
    if reverse:
        return chunked_scan(x[::-1], coef, lane, lanes, waves, seg_steps, segmented, False, carries)[::-1].copy()
    b0, b1, b2, a1, a2 = (float(v) for v in coef)
    n = x.shape[0]
    step = lane * lanes * waves
    n_steps = max(1, -(-n // step))
    xp = np.zeros(n_steps * step)
    xp[:n] = x
    xs = xp.reshape(n_steps, waves, lanes, lane)
    levels = int(np.log2(lanes))
    want = sorted(set([lane << k for k in range(levels)] + [lane * i for i in range(lanes)] + [lane * lanes, step * seg_steps]))
    if carries is None:
        carries = carries_longdouble(coef, want)
    sigma = 1.0 if a1 <= 0.0 else -1.0
    T = np.array([[1, 0], [1, -sigma]], dtype=np.longdouble)
    Ti = np.array([[1, 0], [sigma, -sigma]], dtype=np.longdouble)
    carry_of = lambda k: ((T @ np.asarray(carries[k], dtype=np.longdouble) @ Ti).T).astype(np.float64)
    M_scan = [carry_of(lane << k) for k in range(levels)]
    M_wave, M_lane = carry_of(lane * lanes), np.stack([carry_of(lane * i) for i in range(lanes)])
    y = np.zeros(xs.shape)

    def run(xc, z1, z2, keep):
        out = np.zeros(xc.shape) if keep else None
        for q in range(lane):
            xq = xc[..., q]
            yq = b0 * xq + z1
            z1 = (b1 * xq - a1 * yq) + z2
            z2 = b2 * xq - a2 * yq
            if keep:
                out[..., q] = yq
        return z1, z2, out

    def one_step(si, c, keep):
        xc = xs[si]                                                  # (waves, lanes, lane)
        z1, z2, _ = run(xc, np.zeros((waves, lanes)), np.zeros((waves, lanes)), False)
        l1, l2 = z1 + sigma * z2, -sigma * z2
        for k, M in enumerate(M_scan):
            d = 1 << k
            n1, n2 = l1.copy(), l2.copy()
            n1[:, d:] = M[0, 0] * l1[:, :-d] + M[0, 1] * l2[:, :-d] + l1[:, d:]
            n2[:, d:] = M[1, 0] * l1[:, :-d] + M[1, 1] * l2[:, :-d] + l2[:, d:]
            l1, l2 = n1, n2
        e1, e2 = np.zeros_like(l1), np.zeros_like(l2)
        e1[:, 1:], e2[:, 1:] = l1[:, :-1], l2[:, :-1]
        wc = np.zeros((waves, 2))
        for w in range(waves):
            wc[w] = c
            c = M_wave @ c + np.array([l1[w, -1], l2[w, -1]])
        if keep:
            s1 = M_lane[None, :, 0, 0] * wc[:, None, 0] + M_lane[None, :, 0, 1] * wc[:, None, 1] + e1
            s2 = M_lane[None, :, 1, 0] * wc[:, None, 0] + M_lane[None, :, 1, 1] * wc[:, None, 1] + e2
            y[si] = run(xc, s1 + s2, -sigma * s2, True)[2]
        return c

    if not segmented:
        c = np.zeros(2)
        for si in range(n_steps):
            c = one_step(si, c, True)
    else:
        n_seg = -(-n_steps // seg_steps)
        M_seg = carry_of(step * seg_steps)
        ends = []
        for sg in range(n_seg - 1):
            c = np.zeros(2)
            for si in range(sg * seg_steps, (sg + 1) * seg_steps):
                c = one_step(si, c, False)
            ends.append(c)
        c = np.zeros(2)
        for sg in range(n_seg):
            cc = c
            for si in range(sg * seg_steps, min((sg + 1) * seg_steps, n_steps)):
                cc = one_step(si, cc, True)
            if sg + 1 < n_seg:
                c = M_seg @ c + ends[sg]
    return y.reshape(-1)[:n].copy()
