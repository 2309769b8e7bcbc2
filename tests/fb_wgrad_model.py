"""float64 model of the filterbank weight gradient (include/kapre_hip.h) and the error bound of the device's float32
result.  x, g: (b, c, t, n_freq) and (b, c, t, n_filt), the channels_first view of either layout."""
import numpy as np

U = 2.0 ** -24


def fb_wgrad(x, g):
    """(gW, mass): gW[f][m] = sum_{b, c, t} x[b, c, t, f] g[b, c, t, m] and mass = the same sum of |x| |g|"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("bctf,bctm->fm", x, g), np.einsum("bctf,bctm->fm", np.abs(x), np.abs(g))


def bound(mass, S, n_slabs, folded):
    """gamma_K mass, K = S folded + n_slabs + 1: one float32 chain of the S rows of a slab (``folded`` products per row: the
    channels of a channels_last row, else 1; + 1 should the products be rounded on their own), then n_slabs - 1 ordered additions"""
    K = S * folded + n_slabs + 1
    return K * U / (1 - K * U) * mass
