"""numpy model of YIN as kapre_amd defines it (include/kapre_hip.h): float64 throughout, one series at a time."""
import numpy as np


def frames(x, frame_length, hop, pad_end):
    """(n, frame_length) float64: frame t = x[t hop ...], zeros past the end with ``pad_end``"""
    x = np.asarray(x, np.float64)
    n = -(-len(x) // hop) if pad_end else (0 if len(x) < frame_length else 1 + (len(x) - frame_length) // hop)
    xp = np.concatenate([x, np.zeros(frame_length + hop)])
    return np.stack([xp[t * hop:t * hop + frame_length] for t in range(n)]) if n else np.zeros((0, frame_length))


def curve(x, frame_length, W, hop, tau_hi, pad_end=False):
    """(n, tau_hi + 1): the normalised difference function of every frame; a frame with a d that is not finite is all NaN"""
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for f in frames(x, frame_length, hop, pad_end):
            lagged = np.lib.stride_tricks.sliding_window_view(f[:W + tau_hi], W)[:tau_hi + 1]      # [tau, j] = f[j + tau]
            d = ((f[:W][None, :] - lagged) ** 2).sum(axis=1)
            c = np.concatenate([[0.0], np.cumsum(d[1:])])
            y = np.ones(tau_hi + 1)
            nz = c != 0
            y[nz] = d[nz] * np.arange(tau_hi + 1)[nz] / c[nz]
            out.append(y if np.isfinite(d).all() else np.full(tau_hi + 1, np.nan))
    return np.array(out).reshape(len(out), tau_hi + 1)


def decide(y, sr, tau_min, tau_hi, threshold):
    """(f0, cmnd, tau) of one curve (float64, or the device's float32): a and b in y's precision, the rest in float64"""
    y = np.asarray(y)
    if np.isnan(y).any():
        return np.nan, np.nan, -1
    tau = -1
    for i in range(tau_min, tau_hi):
        trough = y[i] < y[i + 1] if i == tau_min else (y[i] < y[i - 1] and y[i] <= y[i + 1])
        if trough and y[i] < threshold:
            tau = i
            break
    if tau < 0:
        tau = tau_min + int(np.argmin(y[tau_min:tau_hi + 1]))
    shift = 0.0
    if tau_min < tau < tau_hi:
        a = (y[tau + 1] - y[tau]) + (y[tau - 1] - y[tau])
        b = (y[tau + 1] - y[tau - 1]) * y.dtype.type(0.5)
        if abs(b) < abs(a):
            shift = -float(b) / float(a)
    return float(sr) / (tau + shift), y[tau], tau
