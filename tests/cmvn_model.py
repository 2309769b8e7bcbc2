"""numpy model of CMVN as kapre_amd defines it (include/kapre_hip.h): per series along time, n frames,

    d[t] = x[t] - x[0];  m = (1/n) sum d[t];  c[t] = d[t] - m;  v = (1/n) sum c[t]^2;  rstd = (v + eps)^-1/2
    y[t] = c[t] rstd  (norm_vars)   or   y[t] = c[t]

``dtype`` is the arithmetic: float64 is the oracle of the GPU tests, float32 their yardstick -- every operation rounded to
float32: the shift, two passes, plain sequential sums in time order (no chunks, no pairwise merge: how far float32 arithmetic
by itself strays from the oracle).  All functions take the time axis of ``x`` as ``axis``."""
import numpy as np


def time_axis(data_format):
    return 1 if data_format == "channels_last" else 2


def _sum(rows, dtype):
    """rows[0] + rows[1] + ... in order, every addition rounded to ``dtype``"""
    s = np.zeros(rows.shape[1:], dtype=dtype)
    for t in range(rows.shape[0]):
        s = (s + rows[t]).astype(dtype)
    return s


def stats(x, eps=1e-5, axis=1, dtype=np.float64):
    """(d, m, c, v, rstd) of the definition, time moved to axis 0; m, v, rstd without that axis"""
    x = np.moveaxis(np.asarray(x, dtype=dtype), axis, 0)
    n = dtype(x.shape[0])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = (x - x[:1]).astype(dtype)
        m = (_sum(d, dtype) / n).astype(dtype)
        c = (d - m).astype(dtype)
        v = (_sum((c * c).astype(dtype), dtype) / n).astype(dtype)
        rstd = (dtype(1) / np.sqrt((v + dtype(eps)).astype(dtype))).astype(dtype)
    return d, m, c, v, rstd


def cmvn(x, norm_vars=True, eps=1e-5, axis=1, dtype=np.float64):
    x = np.asarray(x)
    if x.shape[axis] == 0:
        return np.zeros(x.shape, dtype=dtype)
    d, m, c, v, rstd = stats(x, eps, axis, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (c * rstd).astype(dtype) if norm_vars else c
    return np.moveaxis(y, 0, axis)


def cmvn_grad(x, gy, norm_vars=True, eps=1e-5, axis=1, dtype=np.float64):
    """d sum(gy * cmvn(x)) / dx, expressed through the forward pass's OUTPUT as the backward kernel does (it reads y, rstd and gy,
    nothing of x):  gx[t] = rstd (gy[t] - mean(gy) - y[t] mean(gy y)),  or  gx[t] = gy[t] - mean(gy)  without ``norm_vars``.
    The two means are plain sequential sums in time order, every operation rounded to ``dtype``."""
    x = np.asarray(x)
    if x.shape[axis] == 0:
        return np.zeros(x.shape, dtype=dtype)
    gy = np.moveaxis(np.asarray(gy, dtype=dtype), axis, 0)
    n = dtype(gy.shape[0])
    mg = (_sum(gy, dtype) / n).astype(dtype)
    t = (gy - mg).astype(dtype)
    if norm_vars:
        _, _, c, _, rstd = stats(x, eps, axis, dtype)
        y = (c * rstd).astype(dtype)
        mgy = (_sum((gy * y).astype(dtype), dtype) / n).astype(dtype)
        t = (rstd * (t - (y * mgy).astype(dtype)).astype(dtype)).astype(dtype)
    return np.moveaxis(t, 0, axis)


def chain_length(frames, plan):
    """the longest chain of additions behind one sum of the kernel: ``plan`` = (R, W, ...) of kpr_cmvn_plan -- R rows in a lane,
    the W chunks of a super-block, the ceil(F / (W R)) super-blocks"""
    R, W = int(plan[0]), int(plan[1])
    return R + W + -(-int(frames) // (W * R))


def first_order_bound(x, norm_vars=True, eps=1e-5, axis=1, plan=(16, 8)):
    """A first-order bound on max |y_f32 - y| / max |y| for ANY float32 evaluation of the definition that rounds every arithmetic
    operation once (unit roundoff u = 2^-24), takes the reciprocal square root from an instruction good to one unit in the last
    place (2^-23 relative), and adds no more than k = ``chain_length`` terms in a row (a sum of k terms is then off by at most
    (k - 1) u sum |term|, Higham 2002 section 4.2; chunked or merged orders only shorten the chains).  Evaluated on the float64
    oracle's own intermediate values, never on a device result; x (float32 data) is exact.

      d = x - x[0]         dd <= u |d|
      m = (1/n) sum d      dm <= ((k - 1) u sum |d| + sum dd) / n + u |m|           (the sum, its terms' errors, the division)
      c = d - m            dc <= dd + dm + u |c|
      v = (1/n) sum c^2    dv <= (sum (2 |c| dc + u c^2) + (k - 1) u sum c^2) / n + u v   (each square, the sum, the division)
      w = v + eps          dw <= dv + u w
      rstd = w^-1/2        drstd / rstd <= dw / (2 w) + 2^-23
      y = c rstd           dy <= rstd dc + |y| drstd / rstd + u |y|                  (norm_vars; else dy = dc)

    All columns, the maximum of dy over the block relative to the maximum of |y|; 0.0 for an empty or an all-zero output."""
    u, ulp = 2.0 ** -24, 2.0 ** -23
    x = np.asarray(x)
    if x.size == 0:
        return 0.0
    d, m, c, v, rstd = stats(x, eps, axis, np.float64)
    n = float(d.shape[0])
    k = chain_length(n, plan)
    dd = u * np.abs(d)
    dm = ((k - 1) * u * np.sum(np.abs(d), axis=0) + np.sum(dd, axis=0)) / n + u * np.abs(m)
    dc = dd + dm + u * np.abs(c)
    if not norm_vars:
        y, dy = c, dc
    else:
        dv = (np.sum(2 * np.abs(c) * dc + u * c * c, axis=0) + (k - 1) * u * np.sum(c * c, axis=0)) / n + u * v
        w = v + eps
        dw = dv + u * w
        with np.errstate(invalid="ignore", divide="ignore"):
            drel = np.where(w > 0, dw / (2 * np.where(w > 0, w, 1.0)), 0.0) + ulp
        y = c * rstd
        dy = rstd * dc + np.abs(y) * drel + u * np.abs(y)
    with np.errstate(invalid="ignore"):
        scale = np.max(np.abs(y))
    if not np.isfinite(scale) or scale == 0.0:
        return 0.0
    return float(np.max(dy) / scale)
