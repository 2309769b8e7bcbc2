"""CPU model of SpecAugment as kapre_amd implements it (test infrastructure: the checker of tests/test_augmentation_*.py).

Two parts, both numpy:
* the draw: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with counter
  (item, mask, calls_lo, calls_hi) and key (seed_lo, seed_hi); width = mulhi32(r0, param), first = mulhi32(r1, limit - width),
  last = first + width -- the rule include/kapre_hip.h documents for kpr_spec_augment_draw;
* the masks: the reference's kapre/augmentation.py:211-214 (`first <= i <= first + width` along one axis, the masks of an axis
  OR-ed) and :264 (`where(mask, mask_value, x)`), restated.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK32 for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & _MASK32, (k1 + np.uint64(W1)) & _MASK32
    return [v.astype(np.uint32) for v in c]


def mulhi32(a, b):
    return ((np.asarray(a, dtype=np.uint64) * np.asarray(b, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def draw_table(seed, calls, n_items, n_time_masks, n_freq_masks, n_time, n_freq, time_mask_param, freq_mask_param):
    """int32 (n_items, n_time_masks + n_freq_masks, 2): inclusive (first, last), time masks first."""
    seed, calls = int(seed) & (2 ** 64 - 1), int(calls) & (2 ** 64 - 1)
    nm = n_time_masks + n_freq_masks
    item, m = np.meshgrid(np.arange(n_items, dtype=np.uint64), np.arange(nm, dtype=np.uint64), indexing='ij')
    r = philox4x32_10((item, m, calls & 0xFFFFFFFF, calls >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    is_time = m < n_time_masks
    param = np.where(is_time, time_mask_param, freq_mask_param)
    limit = np.where(is_time, n_time, n_freq)
    width = mulhi32(r[0], param)
    first = mulhi32(r[1], limit - width)
    return np.stack([first, first + width], axis=-1).astype(np.int32).reshape(n_items, nm, 2)


def mask_from_table(table, n_time_masks, n_time, n_freq):
    """bool (n_items, n_time, n_freq): True where a time interval holds the frame or a frequency interval the bin."""
    table = np.asarray(table)
    t = np.arange(n_time)[None, None, :]
    f = np.arange(n_freq)[None, None, :]
    tm, fm = table[:, :n_time_masks], table[:, n_time_masks:]
    rows = ((t >= tm[:, :, :1]) & (t <= tm[:, :, 1:])).any(axis=1)          # (items, n_time)
    cols = ((f >= fm[:, :, :1]) & (f <= fm[:, :, 1:])).any(axis=1)          # (items, n_freq)
    return rows[:, :, None] | cols[:, None, :]


def state_of(state_tensor):
    """(seed, calls) as unsigned integers from the int64[2] device state."""
    s = state_tensor.detach().cpu().numpy().astype(np.int64).view(np.uint64)
    return int(s[0]), int(s[1])
