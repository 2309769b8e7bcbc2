"""numpy model of the adjoint of the constant-Q transform as kapre_amd defines it (include/kapre_hip.h): float64,
one series at a time, the float32 kernels taken as given.  Also the error bound of the device's float32 result."""
import numpy as np

U = 2.0 ** -24


def cqt_adjoint(G, time, lengths, kernels, hop, center=False):
    """(gx, bound, covered): gx[s] = sum_{t, k} Re G[t, k] Re w_k[n] - Im G[t, k] Im w_k[n], n = s - o - t hop - off_k inside
    [0, N_k), for 0 <= s < time; bound[s] = (M_s + 4) 2^-24 sum |Re G| |Re w| + |Im G| |Im w| with M_s the number of (frame, bin,
    Re / Im) triples whose kernel covers s (one float32 accumulation chain on the matrix unit, in any order: the rule of
    tests/gemm_model.py; nothing is added behind the chain); covered[s] = M_s > 0."""
    G = np.asarray(G, np.complex128)
    L = int(lengths[0])
    o = -(L // 2) if center else 0
    reach = G.shape[0] * hop + L - o                                    # the samples o ... of every frame, shifted to index 0
    gx, mass, count = np.zeros(reach), np.zeros(reach), np.zeros(reach)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(lengths)):
            n, w = int(lengths[k]), np.asarray(kernels[k], np.complex128)
            off = (L - n) // 2
            for t in range(G.shape[0]):
                at = slice(t * hop + off, t * hop + off + n)
                gx[at] += G[t, k].real * w.real - G[t, k].imag * w.imag
                mass[at] += abs(G[t, k].real) * np.abs(w.real) + abs(G[t, k].imag) * np.abs(w.imag)
                count[at] += 2
    keep = slice(-o, -o + time)
    pad = np.zeros(max(0, time - (reach + o)))                          # samples behind the last frame's reach
    gx, mass, count = (np.concatenate([v[keep], pad]) for v in (gx, mass, count))
    return gx, (count + 4) * U * mass, count > 0
