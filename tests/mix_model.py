"""Models of AddNoise (kapre_amd/csrc/kpr_mix_kernels.h) for the tests, numpy only.  Waveforms are (batch, channels, time) here,
whatever layout the call under test uses; ``bank`` / ``lengths`` are what ``backend.noise_bank`` returns.

    seg_b[t] = n_k[(o + t) mod L_k]                                     k = index_b, o = offset_b
    Sx_b = sum_{c,t} x[b,c,t]^2,  Sn_b = sum_t seg_b[t]^2               float64 sums of the exact float32 products
    g_b  = sqrt((Sx_b / (C T)) / (Sn_b / T)) 10^(-snr_b / 20)           0 when Sx_b == 0 or Sn_b == 0
    y    = x + g_b seg_b
    D_b  = sum_{c,t} gy[b,c,t] seg_b[t],  coef_b = D_b g_b / Sx_b (0 when Sx_b == 0),  gx = gy + coef_b x

``forward64`` / ``backward64``: everything in float64, the sums exactly rounded (math.fsum).  ``forward32``: the float32 restatement
of the kernels -- float64 sums, the gain rounded to float32, one rounding of g seg + x.  ``noise_draw``: kpr_noise_draw to the bit.
``forward_torch64``: the forward definition in torch float64 for autograd.  ``forward_bound`` / ``backward_bound``: the error
budgets of tests/test_addnoise_gpu.py."""
import math
from fractions import Fraction

import numpy as np

from augment_model import philox4x32_10, mulhi32


def segments(bank, lengths, index, offset, T):
    """float64 (batch, T): the noise each item gets, index / offset clamped as the kernels clamp them"""
    bank, lengths = np.asarray(bank), np.asarray(lengths)
    out = np.zeros((len(index), T), dtype=np.float64)
    for b, (k, o) in enumerate(zip(index, offset)):
        k = min(max(int(k), 0), bank.shape[0] - 1)
        L = min(max(int(lengths[k]), 1), bank.shape[1])
        o = min(max(int(o), 0), L - 1)
        out[b] = bank[k, (o + np.arange(T)) % L]
    return out


def gain64(Sx, Sn, C, T, snr):
    if Sx == 0.0 or Sn == 0.0:
        return 0.0
    return math.sqrt((Sx / (C * T)) / (Sn / T)) * 10.0 ** (-float(snr) / 20.0)


def forward64(x, seg, snr):
    """x (B, C, T), seg (B, T), snr (B,) -> y64 (B, C, T), stats (B, 4) = (Sx, Sn, g, 0)"""
    x = np.asarray(x, dtype=np.float64)
    B, C, T = x.shape
    stats = np.zeros((B, 4))
    y = np.empty_like(x)
    for b in range(B):
        Sx = math.fsum((x[b] * x[b]).ravel())
        Sn = math.fsum(seg[b] * seg[b])
        g = gain64(Sx, Sn, C, T, np.float64(np.float32(snr[b])))
        stats[b] = (Sx, Sn, g, 0.0)
        y[b] = x[b] + g * seg[b][None, :]
    return y, stats


def forward32(x, seg, snr):
    """the float32 restatement: float64 sums, float32 gain, g seg + x rounded once -> y float32 (B, C, T)"""
    x = np.asarray(x, dtype=np.float32)
    _, stats = forward64(x, seg, snr)
    y = np.empty_like(x)
    for b in range(x.shape[0]):
        g = np.float64(np.float32(stats[b, 2]))
        y[b] = (g * seg[b][None, :] + x[b].astype(np.float64)).astype(np.float32)
    return y


def forward_bound(y64, stats, seg):
    """|y - y64| <= 2^-24 |y64| + 2^-23 |g64 seg| + 2^-149: one rounding of g, one FMA"""
    gs = np.abs(stats[:, 2][:, None, None] * seg[:, None, :])
    return 2.0 ** -24 * np.abs(y64) + 2.0 ** -23 * gs + 2.0 ** -149


def backward64(x, gy, seg, stats):
    """-> gx64 (B, C, T), D (B,), coef64 (B,)"""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    B = x.shape[0]
    D, coef = np.zeros(B), np.zeros(B)
    gx = np.empty_like(x)
    for b in range(B):
        D[b] = math.fsum((gy[b] * seg[b][None, :]).ravel())
        coef[b] = 0.0 if stats[b, 0] == 0.0 else D[b] * stats[b, 2] / stats[b, 0]
        gx[b] = gy[b] + coef[b] * x[b]
    return gx, D, coef


def backward_bound(x, gy, seg, stats, gx64, coef64):
    """|gx - gx64| <= 2^-24 |gx64| + |x| (2^-23 |coef64| + N 2^-52 g64 sum|gy seg| / Sx) + 2^-149"""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    B, C, T = x.shape
    N = C * T
    out = np.empty_like(x)
    for b in range(B):
        Sx, g = stats[b, 0], stats[b, 2]
        sums = 0.0 if Sx == 0.0 else N * 2.0 ** -52 * g * np.sum(np.abs(gy[b] * seg[b][None, :])) / Sx
        out[b] = 2.0 ** -24 * np.abs(gx64[b]) + np.abs(x[b]) * (2.0 ** -23 * abs(coef64[b]) + sums) + 2.0 ** -149
    return out


def achieved_snr_db(x, y):
    """10 log10(mean signal power / mean power of what was added), per item"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = y - x
    return 10.0 * np.log10(np.mean(x * x, axis=(1, 2)) / np.mean(d * d, axis=(1, 2)))


def snr_value(lo, hi, r2):
    """(float32)fma(hi - lo, r2 2^-32, lo): the float64 difference, ONE exactly rounded float64 fma, one rounding to float32"""
    d = float(np.float64(hi) - np.float64(lo))
    exact = Fraction(d) * Fraction(int(r2), 2 ** 32) + Fraction(float(lo))
    return np.float32(float(exact))                     # Fraction -> float is correctly rounded


def noise_draw(seed, calls, n_items, lengths, lo, hi):
    """int32 (n_items, 4) = (index, offset, snr as float32 bits, 0): Philox4x32-10 with counter (item, 0, calls_lo, calls_hi)
    and key (seed_lo, seed_hi); index = mulhi32(r0, n_noise), offset = mulhi32(r1, lengths[index]), snr from r2"""
    seed, calls = int(seed) & (2 ** 64 - 1), int(calls) & (2 ** 64 - 1)
    lengths = np.asarray(lengths, dtype=np.int64)
    item = np.arange(n_items, dtype=np.uint64)
    r = philox4x32_10((item, 0, calls & 0xFFFFFFFF, calls >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    index = mulhi32(r[0], len(lengths))
    offset = mulhi32(r[1], np.maximum(lengths[index], 1))
    snr = np.array([snr_value(lo, hi, v) for v in r[2]], dtype=np.float32)
    out = np.zeros((n_items, 4), dtype=np.int32)
    out[:, 0], out[:, 1], out[:, 2] = index, offset, snr.view(np.int32)
    return out


def forward_torch64(x, seg, snr):
    """the forward definition on torch float64 tensors (x (B, C, T) may require grad; seg (B, T), snr (B,) constants)"""
    import torch
    _, C, T = x.shape
    Sx = (x * x).sum(dim=(1, 2))
    Sn = (seg * seg).sum(dim=1)
    g = torch.sqrt((Sx / (C * T)) / (Sn / T)) * 10.0 ** (-snr / 20.0)
    return x + g[:, None, None] * seg[:, None, :]
