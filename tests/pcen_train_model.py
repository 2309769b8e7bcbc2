"""numpy model of the parameter gradients of PCEN (include/kapre_hip.h: kpr_pcen_bwd_params_f32), beside
tests/pcen_model.py, whose conventions hold: the time axis of ``E`` is ``axis``, the parameters broadcast against ``E`` with that
axis removed, ``dtype`` is the arithmetic (float64: the oracle of the GPU tests, float32: their yardstick)."""
import numpy as np

from pcen_model import smoother


def _band_sums(terms, axis, band_axis, dtype):
    """terms: (4, *E.shape) -> (4, *columns) summed over time, or (4, n_bands) summed over everything but ``band_axis``"""
    if band_axis is None:
        return np.sum(terms, axis=1 + axis, dtype=dtype)
    other = tuple(1 + k for k in range(terms.ndim - 1) if k != band_axis)
    return np.sum(terms, axis=other, dtype=dtype)


def _param_terms(E, gy, s, alpha, delta, r, eps, axis, dtype):
    """per element terms of the four parameter gradients, (4, *E.shape) in the order s, alpha, delta, r, and the intermediates"""
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
    N = np.zeros_like(E)
    carry = np.zeros_like(E[0]) if E.shape[0] else None
    for t in range(E.shape[0] - 1, -1, -1):
        carry = q[t] + a * carry
        N[t] = carry
    step = np.zeros_like(E)
    step[1:] = E[1:] - S[:-1]
    with np.errstate(invalid="ignore"):
        terms = np.stack([N * step,
                          -p * E * G * np.log(es),
                          p - gy * r * delta ** (r - dtype(1)),
                          gy * (u ** r * np.log(u) - delta ** r * np.log(delta))]).astype(dtype)
    mid = dict(E=E, S=S, gy=gy, a=a, es=es, G=G, u=u, p=p, q=q, N=N, step=step, s=s, alpha=alpha, delta=delta, r=r)
    return np.moveaxis(terms, 1, 1 + axis), mid


def pcen_param_grad(E, gy, s=0.025, alpha=0.98, delta=2.0, r=0.5, eps=1e-6, axis=1, dtype=np.float64, band_axis=None):
    """d sum(gy * pcen(E)) / d(s, alpha, delta, r), analytically, rows in that order.  With es = eps + S and the values of
    ``pcen_grad`` (N[t] = q[t] + (1 - s) N[t+1]):

        g_alpha = sum -p E G ln(es)        g_delta = sum p - gy r delta^(r-1)
        g_r     = sum gy (u^r ln u - delta^r ln delta)        g_s = sum_{t >= 1} N[t] (E[t] - S[t-1])

    ``band_axis`` None: summed over time only, shape (4, *columns) (E's shape without ``axis``); else the axis of ``E`` that
    holds the bands: summed over every other axis, shape (4, n_bands) -- the gradient of per-band parameters."""
    terms, _ = _param_terms(E, gy, s, alpha, delta, r, eps, axis, dtype)
    return _band_sums(terms, axis, band_axis, dtype)


def param_grad_bound(E, gy, s, alpha, delta, r, eps, axis, band_axis, rows=8, waves=8):
    """A first-order bound, per parameter (order s, alpha, delta, r), on max_b |g_f32[b] - g[b]| / max_b |g[b]| for a float32
    evaluation of ``pcen_param_grad`` that (i) reads an S computed as ``first_order_bound`` assumes (e[t] <= a e[t-1] + 4 u S[t]),
    (ii) takes powers as exp2(p log2 x) and logarithms as ln2 (k + log2 m), hardware log2 / exp2 / reciprocal good to one unit in
    the last place (2^-23), every other operation rounded once (u = 2^-24), (iii) adds the terms of a column in float32 along a
    chain of at most ``rows * ceil(F / (rows * waves)) + waves`` additions and everything behind that in float64.  Evaluated on
    the float64 model's own intermediates, never on a device result.  With d. the absolute error of a value:

      es = eps + S       d_es = e + u es;             ln es: d = d_es / es + ln2 (2^-23 + u |log2 es|) + u |ln es|
      G                  dG / G as in first_order_bound
      u_ = E G + delta   du = E G dG / G + u u_;      ln u_ likewise
      w = u_^(r-1)       dw / w = |r-1| du / u_ + ln2 |(r-1) log2 u_| (2^-23 + u) + 2^-23;   w0 = delta^(r-1) likewise (du = 0)
      p = gy r w         dp / |p| = dw / w + 2 u
      q = -alpha p E G / es      dq / |q| = dp / |p| + dG / G + d_es / es + 2^-23 + 4 u
      N[t] = q[t] + a N[t+1]     dN[t] = dq[t] + a dN[t+1] + 3 u (|q[t]| + a |N[t+1]|)
      terms      alpha: |p E G ln es| (dp/|p| + dG/G + 3 u) + |p E G| d(ln es)
                 delta: |gy r| (dw + dw0) + 3 u |gy r| |w - w0|
                 r:     |gy| (dA + dC) + 2 u |gy (A - C)|,  A = u_ w ln u_: dA = |A| (du/u_ + dw/w + 2 u) + u_ w d(ln u_), C likewise
                 s:     |N| (e[t-1] + u |E[t] - S[t-1]|) + |E[t] - S[t-1]| dN + u |N (E[t] - S[t-1])|
      a band's sum: sum of the terms' errors + (chain + 1) u sum |term|"""
    u32, ulp, ln2 = 2.0 ** -24, 2.0 ** -23, np.log(2.0)
    terms, m = _param_terms(E, gy, s, alpha, delta, r, eps, axis, np.float64)
    E_, S, gy_, a, es, G, uu, p, q, N, step = (m[k] for k in ("E", "S", "gy", "a", "es", "G", "u", "p", "q", "N", "step"))
    alpha_, delta_, r_ = m["alpha"], m["delta"] + 0 * uu, m["r"]
    F = E_.shape[0]
    e = np.zeros_like(S)
    for t in range(1, F):
        e[t] = a * e[t - 1] + 4 * u32 * S[t]
    d_es = e + u32 * es

    def ln_err(x, dx):
        return dx / x + ln2 * (ulp + u32 * np.abs(np.log2(x))) + u32 * np.abs(np.log(x))

    def pow_rel(x, dx, ex):
        return np.abs(ex) * dx / x + ln2 * np.abs(ex * np.log2(x)) * (ulp + u32) + ulp

    dG = alpha_ * (e / es + u32) + ln2 * np.abs(alpha_ * np.log2(es)) * (ulp + u32) + ulp            # relative
    du = E_ * G * dG + uu * u32
    w, w0 = uu ** (r_ - 1.0), delta_ ** (r_ - 1.0)
    dw, dw0 = w * pow_rel(uu, du, r_ - 1.0), w0 * pow_rel(delta_, 0.0, r_ - 1.0)
    dp = dw / w + 2 * u32                                                                            # relative
    dq = np.abs(q) * (dp + dG + d_es / es + ulp + 4 * u32)
    dN = np.zeros_like(E_)
    carry, nxt = np.zeros_like(E_[0]), np.zeros_like(E_[0])
    for t in range(F - 1, -1, -1):
        carry = dq[t] + a * carry + 3 * u32 * (np.abs(q[t]) + a * np.abs(nxt))
        dN[t], nxt = carry, N[t]
    e_prev = np.zeros_like(e)
    e_prev[1:] = e[:-1]
    peg = np.abs(p * E_ * G)
    A, C = uu * w * np.log(uu), delta_ * w0 * np.log(delta_)
    dA = np.abs(A) * (du / uu + dw / w + 2 * u32) + uu * w * ln_err(uu, du)
    dC = np.abs(C) * (dw0 / w0 + 2 * u32) + delta_ * w0 * ln_err(delta_, 0.0)
    gr = np.abs(gy_ * r_)
    errs = np.stack([np.abs(N) * (e_prev + u32 * np.abs(step)) + np.abs(step) * dN + u32 * np.abs(N * step),
                     peg * np.abs(np.log(es)) * (dp + dG + 3 * u32) + peg * ln_err(es, d_es),
                     gr * (dw + dw0) + 3 * u32 * gr * np.abs(w - w0),
                     np.abs(gy_) * (dA + dC) + 2 * u32 * np.abs(gy_ * (A - C))])
    errs[0, :1] = 0.0
    chain = rows * -(-F // (rows * waves)) + waves + 1
    total = np.moveaxis(errs, 1, 1 + axis) + chain * u32 * np.abs(terms)
    bound = _band_sums(total, axis, band_axis, np.float64)
    g = _band_sums(terms, axis, band_axis, np.float64)
    flat = lambda v: np.abs(v).reshape(4, -1)
    return [float(np.max(flat(bound)[i]) / max(np.max(flat(g)[i]), 1e-300)) if g.size else 0.0 for i in range(4)]
