"""numpy model of PCEN as kapre_amd defines it (include/kapre_hip.h): a sequential loop over time.

    S[0] = E[0], S[t] = (1 - s) S[t-1] + s E[t];   y[t] = (E[t] (eps + S[t])^-alpha + delta)^r - delta^r

``dtype`` is the arithmetic: float64 is the oracle of the GPU tests, float32 their yardstick (how far float32 arithmetic by
itself strays from the oracle).  All functions take the time axis of ``E`` as ``axis`` and parameters that broadcast
against ``E`` with that axis removed (scalars, or arrays shaped by ``band_params``)."""
import numpy as np

DEFAULTS = dict(s=0.025, alpha=0.98, delta=2.0, r=0.5, eps=1e-6)


def band_params(values, data_format, ndim=4):
    """a scalar or per-band vector -> an array that broadcasts against one time slice of a rank-4 batch:
    (b, mel, ch) for channels_last, (b, ch, mel) for channels_first"""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 0:
        return v
    return v.reshape(1, -1, 1) if data_format == "channels_last" else v.reshape(1, 1, -1)


def time_axis(data_format):
    return 1 if data_format == "channels_last" else 2


def smoother(E, s, axis, dtype=np.float64):
    E = np.moveaxis(np.asarray(E, dtype=dtype), axis, 0)
    s = np.asarray(s, dtype=dtype)
    a = (dtype(1) - s).astype(dtype)
    S = np.empty_like(E)
    if E.shape[0]:
        S[0] = E[0]
    for t in range(1, E.shape[0]):
        S[t] = a * S[t - 1] + s * E[t]
    return np.moveaxis(S, 0, axis)


def pcen(E, s=0.025, alpha=0.98, delta=2.0, r=0.5, eps=1e-6, axis=1, dtype=np.float64, return_smoother=False):
    S = np.moveaxis(smoother(E, s, axis, dtype), axis, 0)
    E = np.moveaxis(np.asarray(E, dtype=dtype), axis, 0)
    alpha, delta, r = (np.asarray(v, dtype=dtype) for v in (alpha, delta, r))
    with np.errstate(invalid="ignore"):
        y = (E * (dtype(eps) + S) ** (-alpha) + delta) ** r - delta ** r
    y = np.moveaxis(y.astype(dtype), 0, axis)
    return (y, np.moveaxis(S, 0, axis)) if return_smoother else y


def pcen_grad(E, gy, s=0.025, alpha=0.98, delta=2.0, r=0.5, eps=1e-6, axis=1, dtype=np.float64):
    """d sum(gy * pcen(E)) / dE, analytically: the reverse recurrence N[t] = q[t] + (1 - s) N[t+1]"""
    S = np.moveaxis(smoother(E, s, axis, dtype), axis, 0)
    E = np.moveaxis(np.asarray(E, dtype=dtype), axis, 0)
    gy = np.moveaxis(np.asarray(gy, dtype=dtype), axis, 0)
    s, alpha, delta, r = (np.asarray(v, dtype=dtype) for v in (s, alpha, delta, r))
    a = (dtype(1) - s).astype(dtype)
    es = dtype(eps) + S
    G = es ** (-alpha)
    u = E * G + delta
    p = gy * r * u ** (r - dtype(1))
    q = p * E * (-alpha) * es ** (-alpha - dtype(1))
    gE = np.empty_like(E)
    N = np.zeros_like(E[0]) if E.shape[0] else None
    for t in range(E.shape[0] - 1, -1, -1):
        N = q[t] + a * N
        gE[t] = p[t] * G[t] + (s * N if t else N)
    return np.moveaxis(gE.astype(dtype), 0, axis)


def first_order_bound(E, s, alpha, delta, r, eps, axis):
    """A first-order bound on max |y_f32 - y| / max |y| for ANY float32 evaluation of the definition that (i) runs the
    smoother with one multiply-add pair per frame, each operation rounded once (unit roundoff u = 2^-24), also where a
    chunked scan hands a carry across chunk boundaries, and (ii) takes each power as exp2(p * log2(x)) with a logarithm and
    an exponential good to one unit in the last place (2^-23 relative) and a rounded product.  Evaluated on the float64
    oracle's own intermediate values, never on a device result:

      smoother    e[t] <= a e[t-1] + 4 u S[t]           (two roundings of positive terms <= S[t], the rounding of a = 1 - s,
                                                          one more for the fused / chunked forms)
      G = (eps + S)^-alpha
                  dG / G <= alpha (e / (eps + S) + u) + ln2 |z| (2^-23 + u) + 2^-23,   z = alpha log2(eps + S)
                  (the error of S and of the sum, the logarithm's ulp and the product's rounding scaled by |z|, the exponential)
      u = E G + delta (one rounding, positive terms)
                  du <= E G dG / G + u_ 2^-24
      y = u^r - delta^r
                  dy <= r u^(r-1) du + u^r (ln2 |r log2 u| (2^-23 + 2^-24) + 2^-23) + the same term for delta^r + 2^-24 u^r"""
    u32, ulp = 2.0 ** -24, 2.0 ** -23
    ln2 = np.log(2.0)
    y, S = pcen(E, s, alpha, delta, r, eps, axis, np.float64, return_smoother=True)
    E = np.moveaxis(np.asarray(E, dtype=np.float64), axis, 0)
    S = np.moveaxis(S, axis, 0)
    s, alpha, delta, r = (np.asarray(v, dtype=np.float64) for v in (s, alpha, delta, r))
    a = 1.0 - s
    e = np.zeros_like(S)
    for t in range(1, S.shape[0]):
        e[t] = a * e[t - 1] + 4 * u32 * S[t]
    es = eps + S
    G = es ** (-alpha)
    z = np.abs(alpha * np.log2(es))
    dG = alpha * (e / es + u32) + ln2 * z * (ulp + u32) + ulp
    uu = E * G + delta
    du = E * G * dG + uu * u32

    def power_err(base):
        return base ** r * (ln2 * np.abs(r * np.log2(base)) * (ulp + u32) + ulp)

    dy = r * uu ** (r - 1.0) * du + power_err(uu) + power_err(delta + 0 * uu) + u32 * uu ** r
    scale = np.max(np.abs(y)) if y.size else 1.0
    return float(np.max(dy) / max(scale, 1e-30)) if y.size else 0.0
