"""Numpy model of the generic GEMM k_gemm<AMODE, EPI> (kapre_amd/csrc/kpr_misc_kernels.h), of run_gemm and the row maps
(kpr_host.h), of k_fill_cols, of the DFT tables build_dft_fwd / build_dft_inv (kpr_host_fft.h) and of what its four callers hand it
(stft_gemm, run_istft_f32, run_mel_f32, run_apply_filterbank_f32).  No import of the package: everything is restated from the source,
and tests/test_gemm_model_host.py compares the constants with the source text.

The kernel runs in five instances: <A_PLAIN, E_PLAIN> (ApplyFilterbank on everything that is not thin), <A_FRAME, E_CPLX> (the forward
DFT of every float32 n_fft without an FFT plan), <A_CPLX, E_WINDOW> (the inverse DFT of those sizes and of every non-power-of-two size
with win_length > n_fft), <A_CABS, E_PLAIN> and <A_CABS, E_DB> (the staged mel product).  emulate() walks the launch as the kernel
does: workgroup by workgroup (64 rows x 64 columns), k chunk by k chunk (16 deep), with every clamp, select and index of the
accessors and epilogues, in float64, and checks EVERY load and store against the extent of its buffer (Trace.violations).  The
mutants of MUTANTS change one line each; the host test proves that the case tables tell each of them from the plain float64 oracle,
or that the line changes no output at all (EQUIVALENT, with the reason).

Branch ids (BRANCHES): what a case reaches is recorded by the emulation itself (Trace.branches), not declared by the table.
  rows%64, rows=64k, grid.x>=2, tile.straddle      rows of the launch against the 64-row tile; a tile that holds rows of two signals
  N%64, N%16, N%4, N=64k, grid.y>=2                columns against the 64-column block, the 16-column MFMA tile and the lane's quad
  K%16, K%4, K=16k                                 the reduction length against the 16-deep chunk
  frame.*                                          A_FRAME: left / right padding (the clamped load and its select), a signal shorter
                                                   than one frame, win_length < n_fft, the four layout pairs, one channel
  inv.*, fill_cols*, dcnyq.imag                    E_WINDOW: the window against n_fft, k_fill_cols and its second trip (more than
                                                   4096 * 256 elements), spectra whose DC / Nyquist bins have imaginary parts
  kr.*                                             the k-range of a 64-column block: none, the raw kpr_filterbank_kranges values, the
                                                   schedule's padded values, a union of different tiles, a loop that reads past khi,
                                                   khi beyond Kdim, a tile without a non-zero
  cabs, db, db.straddle, db.slots>1, db.floor      |z| rows; decibels; a 64-row tile with rows of two batch items (two statistics
                                                   words from one workgroup); 32 statistics slots of which the kernel uses slot 0
  plain.cl, plain.misaligned, plain.N>64           <A_PLAIN, E_PLAIN> cases of tests/test_signal_gate.py (POINTERS names them)
  offset>=2^31                                     EXCLUDED: the 64-bit offsets need a buffer of more than 2^31 elements

Bounds (u = 2^-24; the GPU gate holds every element to them, next to max|err| / max|want| <= REG = 4e-6):
  forward DFT    X_n = sum_k fl(x_k w_k) D_kn with D the float32 table.  fl(x_k w_k) carries one rounding (u), D_kn one rounding of the
                 double-precision value (u), and a sum of Kdim terms in ANY order carries at most (Kdim - 1) u of sum |terms| to first
                 order, each product being exact in the MFMA's fused multiply-add; one u is kept for the second-order terms:
                     |err_n| <= (Kdim + 3) u sum_k |x_k w_k| |D_kn|  +  2^-50 sum_k |x_k w_k|
                 The second term is the ABSOLUTE error of the double-precision sine and cosine next to their zeros (cos(pi/2) is
                 computed from a rounded pi / 2: 6e-17, not 0): there |D_kn| is ~1e-16 and the first term is no bound at all.
  inverse DFT    y_n = synth_n sum_j a_j M_jn over the 2K interleaved parts a_j of the spectrum: the same count with one rounding
                 more for the window product, per frame
                     |err_n| <= |synth_n| ((2K + 4) u sum_j |a_j| |M_jn| + 2^-50 sum_j |a_j| c_j / n_fft)
                 then k_ola adds the overlapping frames: the frame bounds add up, plus (overlap - 1) u sum |terms| (generic_model).
  staged mel     m_n = sum_k fl(|z_k|) B_kn: |z| = sqrtf(re^2 + im^2) is within 2 u of the magnitude of the staged z (two squares, a
                 sum, a correctly rounded root: 2.5 u at most, the exact B_kn no rounding), the sum of K terms (K - 1) u:
                     |err_n| <= (K + 5) u sum_k |z_k| B_kn + sum_k stage_k B_kn
                 with stage_k the bound of the staged spectrum's own error (|z' - z| bounds ||z'| - |z||): generic_model.stft_bound
                 for a FAM_GEN stage, the forward bound above (both parts, as a complex modulus) for a FAM_GEMM stage.
  decibels       pointwise_model.to_db_bound on top: the linear bound b gives the interval [db(m - b), db(m + b)], widened by
                 to_db_bound at both ends; the kernel's value must lie inside (next to amin the interval, not the point, is the
                 reference).  The clamp run equals max(f, item max - dyn) in float32 on the first run's bits.
"""
import zlib

import numpy as np

import generic_model as gm
import pointwise_model as pm

# ---- constants restated from the source (tests/test_gemm_model_host.py reads the source text) ------------------------------
TM, TN, KC = 64, 64, 16            # k_gemm: constexpr int TM = 64, TN = 64, KC = 16
THREADS = 256
GRID_1D_CAP = 256 * 16             # grid_1d(n, block, cap = 256 * 16): k_fill_cols
MAX_TILES = 64                     # kMaxTiles: GemmArgs holds k-ranges for 64 tiles of 16 columns
CHUNK_ROWS = 32                    # kChunkRows: the schedule pads a tile's range to whole chunks
SCHED_MAX_ROWS = 32000             # get_sched: row bounds are 16-bit values
DB_SLOTS_SMALL_BATCH = 32          # db_slots of a batch of up to 32 items
U = 2.0 ** -24
TABLE_ABS = 2.0 ** -50
REG = 4e-6                         # tests/test_gpu_parity.py REG
CF, CL = 'channels_first', 'channels_last'
A_PLAIN, A_CABS, A_FRAME, A_CPLX = 0, 1, 2, 3
E_PLAIN, E_CPLX, E_WINDOW, E_DB = 0, 1, 2, 3
INSTANCES = {(A_PLAIN, E_PLAIN): 'plain', (A_FRAME, E_CPLX): 'frame', (A_CPLX, E_WINDOW): 'inverse', (A_CABS, E_PLAIN): 'cabs',
             (A_CABS, E_DB): 'db'}

BRANCHES = ('rows%64', 'rows=64k', 'grid.x>=2', 'tile.straddle', 'N%64', 'N%16', 'N%4', 'N=64k', 'grid.y>=2', 'K%16', 'K%4', 'K=16k',
            'frame', 'frame.pad_begin', 'frame.pad_end', 'frame.T<win', 'frame.win<n_fft', 'frame.cf-cf', 'frame.cf-cl', 'frame.cl-cf',
            'frame.cl-cl', 'frame.C1',
            'inverse', 'inv.win<n_fft', 'inv.win=n_fft', 'inv.win>n_fft', 'fill_cols', 'fill_cols.stride', 'dcnyq.imag', 'inv.odd',
            'inv.cl', 'inv.cf',
            'kr.none', 'kr.raw', 'kr.sched', 'kr.union', 'kr.overread', 'kr.khi>Kdim', 'kr.empty',
            'plain', 'cabs', 'db', 'db.straddle', 'db.slots>1', 'db.floor',
            'plain.cl', 'plain.misaligned', 'plain.N>64', 'offset>=2^31')
EXCLUDED = ('offset>=2^31',)       # RowMap's long long products: a case needs more than 2^31 elements of offset (8 GiB of float32)
# ids whose smallest cases tests/test_signal_gate.py already runs on this instance (signal_model.THIN_CASES ids, label k_gemm)
POINTERS = {'plain.cl': 'K40 N13 rows22 cl C3', 'plain.misaligned': 'K40 N13 rows65 misaligned', 'plain.N>64': 'K40 N65 rows65'}

MUTANTS = {
    'rc': 'gemm_row: rc = r (the row of an idle lane is not clamped to 0)',
    'rowret': 'k_gemm: the return at r >= ga.out.rows dropped',
    'ng': 'B staging: min(ng, N - 1) dropped',
    'kgmask': 'B staging: the kg < Kdim mask dropped',
    't>=0': 'A_FRAME: the t >= 0 select dropped (the clamped sample leaks in)',
    't<T': 'A_FRAME: the t < T select dropped',
    'pad_sign': 'gemm_row: t0 = r0 * hop + pad_left',
    't_es1': 'stft_gemm: t_es = 1 on interleaved input',
    'kr.first': 'k-range of a block taken from its first tile only',
    'kr.repair': 'klo > khi not repaired',
    'kr.guard': 'the t * 16 < N guard of the k-range loop dropped',
    'cplx.swap': 'A_CPLX: parts swapped (k & 1 inverted)',
    'ecplx.n': 'E_CPLX: written at complex element n, not n >> 1',
    'ewin': 'E_WINDOW: n < win dropped (the window is read at n whatever n is)',
    'stats.q': 'E_DB: the statistics word indexed by r / D0',
    'out.es1': 'frames_out_map: es = 1 on channels_last',
    'inv.edge': 'build_dft_inv: the DC / Nyquist rows not halved, their sine rows not zeroed',
}
# one-line changes that cannot change an output (the host test asserts exactly that, case by case)
EQUIVALENT = {
    'kgmask': 'gemm_load_a returns 0 for k >= Kdim, so the clamped B row is multiplied by 0 (finite B)',
    'kr.repair': 'klo starts above khi only when no tile was visited; `for (kc = klo; kc < khi; ...)` runs no trip either way',
    'kr.guard': 'GemmArgs is zero-initialised: a tile beyond N has klo = khi = 0, which only widens the range over exact zeros of B',
    'ewin': 'run_istft_f32 passes N = min(n_fft, win): n < N <= win always holds',
}


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def seed_of(case, salt=0):
    return (zlib.crc32(case['id'].encode()) + 7919 * salt) % (2 ** 31)


def shape_of(fmt, b, c, *inner):
    return (b, *inner, c) if fmt == CL else (b, c, *inner)


def to_layout(a, fmt):
    """(B, C, ...) -> the layout's array"""
    return np.ascontiguousarray(np.moveaxis(a, 1, -1)) if fmt == CL else np.ascontiguousarray(a)


def from_layout(a, fmt):
    return np.moveaxis(a, -1, 1) if fmt == CL else a


def fraction(err, bound):
    """worst error / bound; an error where the bound is 0 (and NaN anywhere) counts as infinite"""
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    frac = np.nan_to_num(frac, nan=np.inf)
    return float(frac.max()) if frac.size else 0.0


class Trace:
    def __init__(self):
        self.violations = []
        self.branches = set()

    def check(self, what, idx, n):
        idx = np.asarray(idx)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n):
            self.violations.append('%s: index range [%d, %d] outside [0, %d)' % (what, int(idx.min()), int(idx.max()), n))
            return np.clip(idx, 0, n - 1)
        return idx


class RowMap:
    """struct RowMap: base = r2 * s2 + r1 * s1 + r0 * s0 with r = (r2 * D1 + r1) * D0 + r0; es = element stride along k / n"""

    def __init__(self, rows, D0, D1, s2, s1, s0, es):
        self.rows, self.D0, self.D1, self.s2, self.s1, self.s0, self.es = rows, D0, D1, s2, s1, s0, es

    def split(self, r):
        r = np.asarray(r, np.int64)
        r0, q = r % self.D0, r // self.D0
        return r0, q % self.D1, q // self.D1

    def base(self, r):
        r0, r1, r2 = self.split(r)
        return r2 * self.s2 + r1 * self.s1 + r0 * self.s0, r2


def frames_out_map(total, F, C, Q, out_cl, mut=()):
    """rows are global frames g = (b C + c) F + f"""
    if out_cl:
        return RowMap(total, F, C, F * Q * C, 1, Q * C, 1 if 'out.es1' in mut else C)
    return RowMap(total, F, C, C * F * Q, F * Q, Q, 1)


def frames_contig_map(total, F, C, Q):
    return frames_out_map(total, F, C, Q, False)


def fb_map(rows, C, Q, cl, mut=()):
    """run_apply_filterbank_f32: channels_last rows r = (b F + f) C + c, else plain rows"""
    if cl:
        return RowMap(rows, C, 1, Q * C, 0, 1, 1 if 'out.es1' in mut else C)
    return RowMap(rows, 1, 1, Q, 0, 0, 1)


def frame_in_map(total, F, C, T, in_cl, mut=()):
    """stft_gemm: the offset of the signal (s0 = es = 0) and t_es, the stride of a sample"""
    if in_cl:
        return RowMap(total, F, C, T * C, 1, 0, 0), (1 if 't_es1' in mut else C)
    return RowMap(total, F, C, C * T, T, 0, 0), 1


class GemmArgs:
    def __init__(self, **kw):
        self.T = self.hop = self.pad_left = 0
        self.t_es = 1
        self.window = None
        self.win = 0
        self.db = None                # (amin_k, ref_term)
        self.has_kr = 0
        self.klo = np.zeros(MAX_TILES, np.int64)      # GemmArgs ga{}: zero-initialised
        self.khi = np.zeros(MAX_TILES, np.int64)
        self.__dict__.update(kw)


def run_gemm_grid(rows, N):
    return (rows + 63) // 64, (N + 63) // 64


def grid_1d(n, block, cap=GRID_1D_CAP):
    return int(min(max((n + block - 1) // block, 1), cap))


# ---------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------
def _load_a(amode, a, ga, base, t0, ok, k, mut, tr):
    kin = ok[:, None] & (k < ga.Kdim)[None, :]
    kc = np.minimum(k, ga.Kdim - 1)
    if amode == A_PLAIN:
        v = a[tr.check('A_PLAIN load', base[:, None] + kc[None, :] * ga.in_.es, a.size)]
    elif amode == A_CABS:                                     # `a` in float2 units
        v = np.abs(a[tr.check('A_CABS load', base[:, None] + kc[None, :] * ga.in_.es, a.size)])
    elif amode == A_CPLX:                                     # `a` in floats: complex element kc >> 1, part kc & 1
        part = (kc & 1) ^ (1 if 'cplx.swap' in mut else 0)
        v = a[tr.check('A_CPLX load', 2 * (base[:, None] + (kc >> 1)[None, :] * ga.in_.es) + part[None, :], a.size)]
    else:
        t = t0[:, None] + kc[None, :]
        tc = np.minimum(np.maximum(t, 0), ga.T - 1)
        v = a[tr.check('A_FRAME load', base[:, None] + tc * ga.t_es, a.size)] * ga.window[tr.check('window load', kc, ga.window.size)][None, :]
        if (kin & (t < 0)).any():
            tr.branches.add('frame.pad_begin')
        if (kin & (t >= ga.T)).any():
            tr.branches.add('frame.pad_end')
        if 't>=0' not in mut:
            kin = kin & (t >= 0)
        if 't<T' not in mut:
            kin = kin & (t < ga.T)
    return np.where(kin, v, 0.0)


def block_krange(ga, col0, mut, tr=None):
    klo, khi = 0, (ga.Kdim + 3) & ~3
    if ga.has_kr:
        klo, khi = 1 << 30, 0
        seen = set()
        t = col0 // 16
        while t < (col0 + TN) // 16 and (t * 16 < ga.N or 'kr.guard' in mut):
            klo, khi = min(klo, int(ga.klo[t])), max(khi, int(ga.khi[t]))
            seen.add((int(ga.klo[t]), int(ga.khi[t])))
            if ga.klo[t] == ga.khi[t] and t * 16 < ga.N and tr is not None:
                tr.branches.add('kr.empty')
            t += 1
            if 'kr.first' in mut:
                break
        if klo > khi and 'kr.repair' not in mut:
            klo = khi
        if tr is not None:
            if len(seen) > 1:
                tr.branches.add('kr.union')
            if (khi - klo) % KC:
                tr.branches.add('kr.overread')
            if khi > ga.Kdim:
                tr.branches.add('kr.khi>Kdim')
    return klo, khi


def emulate(amode, epi, a, bm, ga, out, stats=None, mut=(), tr=None):
    """one launch of k_gemm<amode, epi>: a, bm, out (and stats: 2 words per item and slot, as floats) are flat float64 arrays (a
    complex128 for A_CABS); returns the Trace"""
    tr = tr or Trace()
    rows, N, Kdim = ga.in_.rows, ga.N, ga.Kdim
    if rows <= 0 or N <= 0:
        return tr
    gx, gy = run_gemm_grid(rows, N)
    br = tr.branches
    br.add(INSTANCES[amode, epi])
    br.add('rows%64' if rows % TM else 'rows=64k')
    br.add('N%64' if N % TN else 'N=64k')
    br.add('K%16' if Kdim % KC else 'K=16k')
    br.update((['N%16'] if N % 16 else []) + (['N%4'] if N % 4 else []) + (['K%4'] if Kdim % 4 else []))
    br.update((['grid.x>=2'] if gx >= 2 else []) + (['grid.y>=2'] if gy >= 2 else []))
    if ga.in_.D0 % TM and rows > ga.in_.D0:
        br.add('tile.straddle')
    if not ga.has_kr:
        br.add('kr.none')
    written = np.zeros(out.size, bool)
    for bx in range(gx):
        r = bx * TM + np.arange(TM, dtype=np.int64)
        ok = r < rows
        rc = r if 'rc' in mut else np.where(ok, r, 0)
        if amode == A_FRAME:
            r0, r1, r2 = ga.in_.split(rc)
            base = r2 * ga.in_.s2 + r1 * ga.in_.s1
            t0 = r0 * ga.hop + (ga.pad_left if 'pad_sign' in mut else -ga.pad_left)
        else:
            base, _ = ga.in_.base(rc)
            t0 = np.zeros(TM, np.int64)
        for by in range(gy):
            col0 = by * TN
            klo, khi = block_krange(ga, col0, mut, tr)
            acc = np.zeros((TM, TN))
            ng = col0 + np.arange(TN, dtype=np.int64)
            ngc = ng if 'ng' in mut else np.minimum(ng, N - 1)
            for kc0 in range(klo, khi, KC):
                k = kc0 + np.arange(KC, dtype=np.int64)
                X = _load_a(amode, a, ga, base, t0, ok, k, mut, tr)
                kgc = np.minimum(k, Kdim - 1)
                v = bm[tr.check('B load', kgc[:, None] * ga.ldb + ngc[None, :], bm.size)]
                mask = np.broadcast_to((ng < N)[None, :], v.shape) if 'kgmask' in mut else (k < Kdim)[:, None] & (ng < N)[None, :]
                acc += X @ np.where(mask, v, 0.0)
            keep = np.ones(TM, bool) if 'rowret' in mut else r < ga.out.rows
            rr = r[keep]
            ob, r2 = ga.out.base(rr)
            if epi == E_DB and 'stats.q' in mut:
                r2 = rr // ga.out.D0
            n = ng[ng < N]
            v = acc[keep][:, :n.size]
            if epi == E_CPLX:
                ne = n if 'ecplx.n' in mut else n >> 1
                idx = 2 * (ob[:, None] + ne[None, :] * ga.out.es) + (n & 1)[None, :]
            else:
                idx = ob[:, None] + n[None, :] * ga.out.es
            if epi == E_WINDOW:
                inside = np.ones(n.size, bool) if 'ewin' in mut else n < ga.win
                w = np.zeros(n.size)
                w[inside] = ga.window[tr.check('synthesis window load', n[inside], ga.window.size)]
                v = v * w[None, :]
            elif epi == E_DB:
                amin_k, ref_term = ga.db
                v = 10.0 * np.log10(np.maximum(v, float(amin_k))) - float(ref_term)
                if np.unique(r2).size > 1:
                    br.add('db.straddle')
                for item in np.unique(r2):
                    sel = v[r2 == item]
                    w0 = int(tr.check('statistics word', np.array([2 * item + 1]), stats.size)[0]) - 1
                    stats[w0], stats[w0 + 1] = max(stats[w0], sel.max()), min(stats[w0 + 1], sel.min())
            idx = tr.check('store', idx, out.size)
            if written[idx].any() or np.unique(idx).size != idx.size:
                tr.violations.append('store: an output element is written twice')
            written[idx] = True
            out[idx] = v
    return tr


def emulate_fill_cols(out, rows, ld, n0, n1, tr):
    """k_fill_cols: grid_1d(rows * (n1 - n0), 256) workgroups, grid-stride over i"""
    total = rows * (n1 - n0)
    grid = grid_1d(total, THREADS)
    tr.branches.add('fill_cols')
    if total > grid * THREADS:
        tr.branches.add('fill_cols.stride')
    i = np.arange(total, dtype=np.int64)                      # every i < total is reached by thread i mod (grid * 256)
    out[tr.check('k_fill_cols store', (i // (n1 - n0)) * ld + n0 + i % (n1 - n0), out.size)] = 0.0


# ---------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------
def build_dft_fwd(n_fft, exact_zeros=True):
    """[n_fft rows n][2K cols]: col 2k = cos(2 pi k n / N), col 2k + 1 = -sin(...), double precision with the exact angle
    reduction k n mod N, rounded to float32; a sine whose exact value is 0 is stored as 0 (exact_zeros=False: the table before that)"""
    K = n_fft // 2 + 1
    kn = (np.arange(K, dtype=np.int64)[None, :] * np.arange(n_fft, dtype=np.int64)[:, None]) % n_fft
    a = 2.0 * np.pi * kn.astype(np.float64) / float(n_fft)
    h = np.empty((n_fft, 2 * K), np.float32)
    h[:, 0::2] = np.cos(a).astype(np.float32)
    s = (-np.sin(a)).astype(np.float32)
    h[:, 1::2] = np.where((2 * kn) % n_fft == 0, np.float32(0), s) if exact_zeros else s
    return h


def build_dft_inv(n_fft, mut=(), exact_zeros=True):
    """[2K rows][n_fft cols]: row 2k = c_k cos(2 pi k n / N) / N, row 2k + 1 = -c_k sin(...) / N, c_k = 1 for DC (and Nyquist when N is
    even) else 2; the sine rows of DC and Nyquist are zeros (their imaginary parts do not enter a real inverse transform)"""
    K = n_fft // 2 + 1
    k = np.arange(K, dtype=np.int64)[:, None]
    kn = (k * np.arange(n_fft, dtype=np.int64)[None, :]) % n_fft
    a = 2.0 * np.pi * kn.astype(np.float64) / float(n_fft)
    edge = (k == 0) | ((n_fft % 2 == 0) & (k == n_fft // 2))
    if 'inv.edge' in mut:
        edge = np.zeros_like(edge)
    ck = np.where(edge, 1.0, 2.0) / float(n_fft)
    h = np.empty((2 * K, n_fft), np.float32)
    h[0::2] = (ck * np.cos(a)).astype(np.float32)
    zero = edge | (((2 * kn) % n_fft == 0) if exact_zeros and 'inv.edge' not in mut else False)
    h[1::2] = np.where(zero, np.float32(0), (-ck * np.sin(a)).astype(np.float32))
    return h


def inv_scale(n_fft):
    """c_j / n_fft of the 2K interleaved parts"""
    K = n_fft // 2 + 1
    k = np.arange(K)
    edge = (k == 0) | ((n_fft % 2 == 0) & (k == n_fft // 2))
    return np.repeat(np.where(edge, 1.0, 2.0) / n_fft, 2)


# ---------------------------------------------------------------------------------------------
# route predicates (fft_family, mel_route, fb_route as far as they decide for or against this kernel)
# ---------------------------------------------------------------------------------------------
MR_SIZES = (160, 200, 320, 400, 640, 800, 1000, 96, 120, 192, 240, 360, 384, 480, 600, 720, 768, 960)     # with_mr


def fft_family(n_fft, win):
    """'gemm' where fft_family answers FAM_GEMM (win: the cropped win_length of a forward transform, the caller's of an inverse)"""
    if n_fft in (256, 512, 1024, 2048):
        return 'pow2'
    if gm.bluestein_m(n_fft) > 0 and win <= n_fft:
        return 'mr' if n_fft in MR_SIZES else 'bs'
    if n_fft in (4096, 8192):
        return 'big'
    if win <= n_fft and gm.gen_fits('f32', n_fft) is not None:
        return 'gen'
    return 'gemm'


def mel_staged_gemm(n_fft):
    """mel_route ends in MEL_STAGED with PROD_GEMM: no fused kernel for the size (512 / 1024 / 2048, 256, the mixed-radix sizes) and a
    stage that is neither FAM_MR / FAM_BS (k_mel_ws, k_band_mel) nor FAM_BIG (k_band_mel)"""
    return n_fft not in (256, 512, 1024, 2048) and n_fft not in MR_SIZES and fft_family(n_fft, n_fft) in ('gen', 'gemm')


def thin_gemm_shape(n_freq, n_filt):
    return (n_filt + 15) // 16 <= 4 and n_freq <= 512 and n_freq % 4 == 0


def fb_unpacked_generic(n_freq, n_filt, contiguous, packed):
    """fb_route == FB_UNPACKED (no packed filterbank handed in, n_freq <= 1025) and not the thin GEMM"""
    return not packed and n_freq <= 1025 and not (contiguous and thin_gemm_shape(n_freq, n_filt))


# ---------------------------------------------------------------------------------------------
# k-ranges: kpr_filterbank_kranges, tile_ranges / build_sched, what each caller passes
# ---------------------------------------------------------------------------------------------
def raw_kranges(fb):
    n_freq, n_filt = fb.shape
    out = []
    for t in range((n_filt + 15) // 16):
        nz = np.flatnonzero((fb[:, 16 * t:16 * t + 16] != 0).any(1) | np.isnan(fb[:, 16 * t:16 * t + 16]).any(1))
        lo, hi = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
        out.append((lo & ~3, (hi + 3) & ~3))
    return out


def mel_row_cap(K):
    return (K + CHUNK_ROWS - 1) // CHUNK_ROWS * CHUNK_ROWS


def sched_kranges(K, M, kr):
    """tile_ranges: lo rounded down to 8, the range padded to whole 32-row chunks inside [0, mel_row_cap(K)] -- hi may exceed K.
    None where get_sched refuses (more than 64 tiles, more than 32000 rows): run_mel_f32 then passes no k-ranges"""
    ntiles = (M + 15) // 16
    if ntiles > MAX_TILES or K > SCHED_MAX_ROWS:
        return None
    cap, out = mel_row_cap(K), []
    for t in range(ntiles):
        lo, hi = kr[t]
        lo &= ~7
        need = max(CHUNK_ROWS, (hi - lo + CHUNK_ROWS - 1) // CHUNK_ROWS * CHUNK_ROWS)
        hi = min(cap, lo + need)
        lo = max(0, hi - need)
        assert hi - lo == need
        out.append((lo, hi))
    return out


def set_kr(ga, kr, source, tr):
    if kr is None:
        return
    ga.has_kr = 1
    for t, (lo, hi) in enumerate(kr):
        ga.klo[t], ga.khi[t] = lo, hi
    tr.branches.add('kr.' + source)


# ---------------------------------------------------------------------------------------------
# forward: stft_gemm
# ---------------------------------------------------------------------------------------------
def fcase(id, n_fft, win, hop, B, C, T, pads=(False, False), fmts=(CF, CF)):
    return dict(id=id, n_fft=n_fft, win=win, hop=hop, B=B, C=C, T=T, pad_begin=pads[0], pad_end=pads[1], in_fmt=fmts[0], out_fmt=fmts[1],
                ty='f32', mode=gm.COMPLEX)


FWD_CASES = [
    fcase('67 2x2x9', 67, 67, 16, 2, 2, 195),                                               # 36 rows: the suite's old shape
    fcase('67 1x3x23 pads cl-cl', 67, 67, 16, 1, 3, 310, (True, True), (CL, CL)),           # 69 rows, both paddings
    fcase('71 win40 2x1x32 cl', 71, 40, 16, 2, 1, 536, (False, False), (CL, CL)),           # 64 rows, one channel, N 72, K 40
    fcase('127 win64 2x2x32 cf-cl', 127, 64, 16, 2, 2, 560, (False, False), (CF, CL)),      # 128 rows, N 128, K 64
    fcase('67 short pad_end cl-cf', 67, 67, 16, 2, 2, 30, (False, True), (CL, CF)),         # a signal shorter than one frame
    fcase('67 win40 pad_begin cf-cl', 67, 40, 16, 1, 3, 200, (True, False), (CF, CL)),
    fcase('67 pad_end cl-cf C3', 67, 67, 16, 1, 3, 150, (False, True), (CL, CF)),
    fcase('1028 1x2x5', 1028, 1028, 257, 1, 2, 2056),                                       # N 1030: the last quad half full
]
NYQUIST_CASE = '1028 1x2x5'


def frames_of(c):
    t = c['T'] + (c['n_fft'] - c['hop'] if c['pad_begin'] else 0)
    if c['pad_end']:
        return -(-t // c['hop'])
    return 0 if t < c['win'] else 1 + (t - c['win']) // c['hop']


def hann(n):
    """backend.get_window_fn(None): tf.signal.hann_window(periodic=True) in float32 (periodic only affects even lengths)"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / float(n + (1 - n % 2) - 1))).astype(np.float32)


def stft_input(c):
    return np.random.default_rng(seed_of(c)).standard_normal((c['B'], c['C'], c['T'])).astype(np.float32)


def emulate_stft(c, xin, window, mut=(), table=None):
    """xin: the waveform in the input layout; returns (spectrum in the output layout, complex128; Trace)"""
    n, B, C, T = c['n_fft'], c['B'], c['C'], c['T']
    F, K = frames_of(c), n // 2 + 1
    total = B * C * F
    in_cl, out_cl = c['in_fmt'] == CL and C > 1, c['out_fmt'] == CL and C > 1        # make_geom
    win = min(c['win'], n)                                                               # forward_geom
    tr = Trace()
    assert fft_family(n, win) == 'gemm'
    in_map, t_es = frame_in_map(total, F, C, T, in_cl, mut)
    ga = GemmArgs(in_=in_map, out=frames_out_map(total, F, C, K, out_cl, mut), Kdim=min(win, n), N=2 * K, ldb=2 * K, T=T, hop=c['hop'],
                  pad_left=n - c['hop'] if c['pad_begin'] else 0, t_es=t_es, window=np.asarray(window, np.float64), win=win)
    table = build_dft_fwd(n) if table is None else table
    out = np.full(2 * total * K, np.nan)
    emulate(A_FRAME, E_CPLX, np.asarray(xin, np.float64).ravel(), table.astype(np.float64).ravel(), ga, out, mut=mut, tr=tr)
    br = tr.branches
    br.add('frame.%s-%s' % ('cl' if in_cl else 'cf', 'cl' if out_cl else 'cf'))
    br.update((['frame.C1'] if C == 1 else []) + (['frame.T<win'] if T < win else []) + (['frame.win<n_fft'] if win < n else []))
    return out.view(np.complex128).reshape(shape_of(CL if out_cl else CF, B, C, F, K)).reshape(shape_of(c['out_fmt'], B, C, F, K)), tr


def stft_frames(c, x_bct, window, dtype=np.float64):
    """tf.signal.stft's frames, windowed: (B, C, F, min(win, n_fft))"""
    n, win, hop = c['n_fft'], c['win'], c['hop']
    x = np.asarray(x_bct, dtype)
    if c['pad_begin']:
        x = np.pad(x, ((0, 0), (0, 0), (n - hop, 0)))
    f_ = frames_of(c)
    x = np.pad(x, ((0, 0), (0, 0), (0, max(0, (f_ - 1) * hop + win - x.shape[-1]))))
    idx = np.arange(win)[None, :] + hop * np.arange(f_)[:, None]
    return (x[..., idx] * np.asarray(window, dtype))[..., :n]


def parts(z):
    """complex (..., K) -> real (..., 2K) interleaved"""
    return np.stack([z.real, z.imag], -1).reshape(z.shape[:-1] + (2 * z.shape[-1],))


def oracle_stft(c, x_bct, window, table):
    """the plain float64 product with the same table: (B, C, F, K) complex128"""
    fr = stft_frames(c, x_bct, window)
    y = fr @ table.astype(np.float64)[:fr.shape[-1]]
    return y[..., 0::2] + 1j * y[..., 1::2]


def stft_f32_product(c, x_bct, window, table):
    """numpy's float32 product of float32 frames with the float32 table: what the reference alone achieves"""
    fr = stft_frames(c, x_bct, window, np.float32)
    y = (fr.reshape(-1, fr.shape[-1]) @ table[:fr.shape[-1]]).reshape(fr.shape[:-1] + (table.shape[1],))
    return y[..., 0::2] + 1j * y[..., 1::2]


def stft_bound(c, x_bct, window, table):
    """(B, C, F, 2K): the bound of the real and imaginary parts, interleaved"""
    fr = np.abs(stft_frames(c, x_bct, window))
    kdim = fr.shape[-1]
    return (kdim + 3) * U * (fr @ np.abs(table.astype(np.float64))[:kdim]) + TABLE_ABS * fr.sum(-1, keepdims=True)


# ---------------------------------------------------------------------------------------------
# inverse: run_istft_f32's DFT-as-GEMM branch, k_fill_cols, the overlap-add
# ---------------------------------------------------------------------------------------------
def icase(id, n_fft, win, hop, B, C, F, fmts=(CF, CF)):
    return dict(id=id, n_fft=n_fft, win=win, hop=hop, B=B, C=C, F=F, spec_fmt=fmts[0], wave_fmt=fmts[1], ty='f32')


INV_CASES = [
    icase('6 win9 hop2', 6, 9, 2, 2, 2, 5, (CL, CL)),                        # Kdim 8, N 6, fill
    icase('67 win40 cl', 67, 40, 16, 2, 2, 9, (CL, CL)),                     # a window shorter than n_fft: N 40
    icase('67 win67 1x3x23', 67, 67, 16, 1, 3, 23),                          # 69 rows, odd size: no Nyquist bin
    icase('67 win80 cl-cf', 67, 80, 20, 2, 2, 9, (CL, CF)),
    icase('1028 win1028', 1028, 1028, 257, 1, 2, 3),                         # Kdim 1030, N 1028
    icase('400 win500 2x1x32', 400, 500, 100, 2, 1, 32),                     # 64 rows, Kdim 402
    icase('6 win506 2100 frames', 6, 506, 3, 1, 1, 2100),                    # k_fill_cols: 1 050 000 elements, a second trip
]


def synth_window(c):
    """a synthesis window without zeros"""
    return np.random.default_rng(seed_of(c, 2)).uniform(0.25, 1.0, c['win']).astype(np.float32)


def istft_input(c):
    """(B, C, F, K) complex64; the DC and Nyquist bins carry imaginary parts (a real inverse transform ignores them)"""
    rng = np.random.default_rng(seed_of(c, 1))
    shape = (c['B'], c['C'], c['F'], c['n_fft'] // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def ola(c, frames, wave_fmt, tr=None):
    """(B, C, F, win) -> the waveform in wave_fmt"""
    B, C, F, win = frames.shape
    out = np.zeros((B, C, (F - 1) * c['hop'] + win), frames.dtype)
    for i in range(F):
        out[..., i * c['hop']:i * c['hop'] + win] += frames[:, :, i]
    return to_layout(out, wave_fmt)


def emulate_istft(c, sin, synth, mut=(), table=None):
    """sin: the spectrum in spec_fmt; returns (waveform in wave_fmt, Trace)"""
    n, win, B, C, F = c['n_fft'], c['win'], c['B'], c['C'], c['F']
    K, total = n // 2 + 1, B * C * F
    spec_cl = c['spec_fmt'] == CL and C > 1                                  # make_geom: out_layout is the spectrogram's
    tr = Trace()
    assert fft_family(n, win) == 'gemm'
    ga = GemmArgs(in_=frames_out_map(total, F, C, K, spec_cl), out=frames_contig_map(total, F, C, win), Kdim=2 * K, N=min(n, win), ldb=n,
                  window=np.asarray(synth, np.float64), win=win)
    table = build_dft_inv(n, mut) if table is None else table
    frames = np.full(total * win, np.nan)
    a = np.ascontiguousarray(np.asarray(sin, np.complex128)).view(np.float64).ravel()
    emulate(A_CPLX, E_WINDOW, a, table.astype(np.float64).ravel(), ga, frames, mut=mut, tr=tr)
    if win > n:
        emulate_fill_cols(frames, total, win, n, win, tr)
    if np.isnan(frames).any():
        tr.violations.append('%d elements of the frame workspace were never written' % int(np.isnan(frames).sum()))
    br = tr.branches
    br.add('inv.win<n_fft' if win < n else 'inv.win=n_fft' if win == n else 'inv.win>n_fft')
    br.add('inv.cl' if spec_cl else 'inv.cf')
    if n % 2:
        br.add('inv.odd')
    edges = [0] + ([n // 2] if n % 2 == 0 else [])
    if np.any(np.asarray(from_layout(sin, c['spec_fmt']))[..., edges].imag != 0):
        br.add('dcnyq.imag')
    return ola(c, frames.reshape(B, C, F, win), c['wave_fmt']), tr


def oracle_istft(c, spec_bcfk, synth, table):
    n, win = c['n_fft'], c['win']
    y = parts(np.asarray(spec_bcfk, np.complex128)) @ table.astype(np.float64)
    y = y[..., :min(n, win)] * np.asarray(synth, np.float64)[:min(n, win)]
    if win > y.shape[-1]:
        y = np.pad(y, [(0, 0)] * 3 + [(0, win - y.shape[-1])])
    return ola(c, y, c['wave_fmt'])


def istft_f32_product(c, spec_bcfk, synth, table):
    n, win = c['n_fft'], c['win']
    a = parts(np.asarray(spec_bcfk, np.complex64)).astype(np.float32)
    y = (a.reshape(-1, a.shape[-1]) @ table).reshape(a.shape[:-1] + (n,))[..., :min(n, win)] * np.asarray(synth, np.float32)[:min(n, win)]
    if win > y.shape[-1]:
        y = np.pad(y, [(0, 0)] * 3 + [(0, win - y.shape[-1])])
    return ola(c, y, c['wave_fmt'])


def ref_istft(c, spec_bcfk, synth, table):
    """(waveform in wave_fmt from numpy's irfft in longdouble, its bound)"""
    n, win, hop, F = c['n_fft'], c['win'], c['hop'], c['F']
    K, m = n // 2 + 1, min(n, win)
    spec = np.asarray(spec_bcfk).astype(np.clongdouble)
    fr = np.fft.irfft(spec, n=n, axis=-1)[..., :m] * np.asarray(synth, gm.LD)[:m]
    a = np.abs(parts(np.asarray(spec_bcfk, np.complex128)))
    b = ((2 * K + 4) * U * (a @ np.abs(table.astype(np.float64)))[..., :m] + TABLE_ABS * (a @ inv_scale(n))[..., None]) * np.abs(np.asarray(synth, np.float64))[:m]
    pad = [(0, 0)] * 3 + [(0, win - m)]
    fr, b = np.pad(fr, pad), np.pad(b, pad)
    count = ola(c, np.ones(fr.shape), CF)
    bound = ola(c, b, CF) + np.maximum(count - 1, 0) * U * ola(c, np.abs(fr).astype(np.float64), CF)
    return ola(c, fr, c['wave_fmt']), to_layout(bound, c['wave_fmt'])


# ---------------------------------------------------------------------------------------------
# ApplyFilterbank: run_apply_filterbank_f32 on what is not thin, with the raw k-ranges
# ---------------------------------------------------------------------------------------------
def bcase(id, B, C, F, n_freq, n_filt, bank, kr=True):
    return dict(id=id, B=B, C=C, F=F, n_freq=n_freq, n_filt=n_filt, bank=bank, kr=kr, fmt=CL)


BANDS = ((4, 20), (41, 52), (64, 100), (109, 128))        # rows with non-zeros of the four 16-filter tiles: disjoint
FB_CASES = [
    bcase('banded 128->64 cl C2', 2, 2, 20, 128, 64, 'banded'),                   # 80 rows; one block whose four tiles differ
    bcase('banded, tile 2 empty', 2, 2, 20, 128, 64, 'banded-empty'),
    bcase('40->1 cl C2', 1, 2, 33, 40, 1, 'dense'), bcase('40->3 cl C2', 1, 2, 33, 40, 3, 'dense'),
    bcase('40->17 cl C2', 1, 2, 33, 40, 17, 'dense'), bcase('40->65 cl C2', 1, 2, 33, 40, 65, 'dense'),
]


def fb_input(c):
    """integers in [-7, 7]: every partial sum is below 2^24 and the float32 product is exact in any order"""
    rng = np.random.default_rng(seed_of(c))
    x = rng.integers(-7, 8, (c['B'], c['C'], c['F'], c['n_freq'])).astype(np.float32)
    fb = rng.integers(-7, 8, (c['n_freq'], c['n_filt'])).astype(np.float32)
    if c['bank'].startswith('banded'):
        keep = np.zeros(fb.shape, bool)
        for t, (lo, hi) in enumerate(BANDS):
            if not (c['bank'] == 'banded-empty' and t == 2):
                keep[lo:hi, 16 * t:16 * t + 16] = True
                fb[lo, 16 * t] = fb[hi - 1, 16 * t + 15] = 3.0          # the ends of the band are non-zeros
        fb = np.where(keep, fb, np.float32(0))
    assert 49 * c['n_freq'] < 2 ** 24
    return x, fb


def emulate_fb(c, xin, fb, mut=()):
    """xin in the case's layout (B, F, n_freq, C); returns (output in that layout, Trace)"""
    B, C, F, n_freq, n_filt = c['B'], c['C'], c['F'], c['n_freq'], c['n_filt']
    rows, cl = B * C * F, c['fmt'] == CL
    tr = Trace()
    assert fb_unpacked_generic(n_freq, n_filt, not cl or C == 1, packed=False)
    ga = GemmArgs(in_=fb_map(rows, C, n_freq, cl), out=fb_map(rows, C, n_filt, cl, mut), Kdim=n_freq, N=n_filt, ldb=n_filt)
    if c['kr'] and (n_filt + 15) // 16 <= MAX_TILES and n_freq <= SCHED_MAX_ROWS:
        set_kr(ga, raw_kranges(fb), 'raw', tr)
    out = np.full(rows * n_filt, np.nan)
    emulate(A_PLAIN, E_PLAIN, np.asarray(xin, np.float64).ravel(), fb.astype(np.float64).ravel(), ga, out, mut=mut, tr=tr)
    return out.reshape(shape_of(c['fmt'], B, C, F, n_filt)), tr


def oracle_fb(c, x_bcfk, fb):
    return to_layout(np.asarray(x_bcfk, np.float64) @ fb.astype(np.float64), c['fmt'])


# ---------------------------------------------------------------------------------------------
# the staged mel product: run_mel_f32, MEL_STAGED / PROD_GEMM
# ---------------------------------------------------------------------------------------------
def mcase(id, n_fft, hop, B, C, T, n_filt, bank, pads=(False, False), fmts=(CL, CL)):
    return dict(id=id, n_fft=n_fft, win=n_fft, hop=hop, B=B, C=C, T=T, n_filt=n_filt, bank=bank, pad_begin=pads[0], pad_end=pads[1],
                in_fmt=fmts[0], out_fmt=fmts[1], ty='f32', mode=gm.COMPLEX)


MEL_CASES = [
    mcase('15 -> 5 B1', 15, 4, 1, 2, 103, 5, 'tri'),                                    # FAM_GEN stage, K 8: khi 32
    mcase('15 -> 1025 dense B2', 15, 4, 2, 1, 63, 1025, 'dense'),                       # 65 tiles: get_sched refuses, no k-ranges
    mcase('67 -> 8 B3 straddle', 67, 16, 3, 1, 419, 8, 'tri', fmts=(CF, CF)),           # FAM_GEMM stage; 3 x 23 rows in 2 tiles
    mcase('67 -> 20 B2 cl', 67, 16, 2, 2, 195, 20, 'tri', (True, True)),
    mcase('1200 -> 40 B2 cf-cl', 1200, 300, 2, 2, 3000, 40, 'tri', fmts=(CF, CL)),      # FAM_GEN stage, K 601, cap 608
]
DB_DYN_OFF = 1000.0
DB_RUNS = ((1.0, 1e-5, DB_DYN_OFF), (1.0, 1e-5, 20.0))       # (ref_value, amin, dynamic_range): the floor off, the floor active


def mel_input(c):
    """noise under an envelope that falls by 10^-7 over the signal: the output spans more than the 20 dB of run (b), so its floor is
    active, and the last frames come out under amin = 1e-5, where the decibel reference is an interval"""
    env = 10.0 ** (-7.0 * np.arange(c['T'], dtype=np.float64) / c['T'])
    return (stft_input(c).astype(np.float64) * env).astype(np.float32)


def mel_bank(c):
    """a bank set by hand: overlapping triangles with random positive peaks over the K bins (exact zeros outside), or a dense one"""
    K, M = c['n_fft'] // 2 + 1, c['n_filt']
    rng = np.random.default_rng(seed_of(c, 3))
    if c['bank'] == 'dense':
        return rng.uniform(0.0, 1.0, (K, M)).astype(np.float32)
    edges = np.linspace(1.0, K - 1.0, M + 2)
    k = np.arange(K, dtype=np.float64)[:, None]
    up = (k - edges[:-2]) / (edges[1:-1] - edges[:-2])
    down = (edges[2:] - k) / (edges[2:] - edges[1:-1])
    return (np.maximum(0.0, np.minimum(up, down)) * rng.uniform(0.5, 2.0, M)).astype(np.float32)


def mel_stage(n_fft):
    return fft_family(n_fft, n_fft)


def emulate_mel(c, spec, fb, db=None, mut=()):
    """spec: the staged spectrum (B, C, F, K) complex128 (frame-contiguous, as the stage writes it); db = (ref_value, amin, dyn) or
    None.  Returns (output in out_fmt BEFORE the clamp, the statistics words of slot 0 as (B, 2) [max, min], Trace)"""
    B, C, F, K = spec.shape
    M, total = c['n_filt'], B * C * F
    out_cl = c['out_fmt'] == CL and C > 1
    tr = Trace()
    assert mel_staged_gemm(c['n_fft'])
    ga = GemmArgs(in_=frames_contig_map(total, F, C, K), out=frames_out_map(total, F, C, M, out_cl, mut), Kdim=K, N=M, ldb=M)
    set_kr(ga, sched_kranges(K, M, raw_kranges(fb)), 'sched', tr)
    out = np.full(total * M, np.nan)
    stats = None
    if db is not None:
        ga.db = pm.db_device_params(db[0], db[1])
        slots = DB_SLOTS_SMALL_BATCH
        stats = np.tile(np.array([-np.inf, np.inf]), B * slots)            # k_stats_init
        tr.branches.update(['db.slots>1'] + (['db.floor'] if db[2] < DB_DYN_OFF else []))
    emulate(A_CABS, E_DB if db is not None else E_PLAIN, np.asarray(spec, np.complex128).ravel(), fb.astype(np.float64).ravel(), ga, out,
            stats=stats, mut=mut, tr=tr)
    if stats is not None and not np.all(np.isinf(stats[2 * B:])):
        tr.violations.append('a statistics slot other than 0 was written')
    out = out.reshape(shape_of(CL if out_cl else CF, B, C, F, M)).reshape(shape_of(c['out_fmt'], B, C, F, M))
    return out, (stats[:2 * B].reshape(B, 2) if stats is not None else None), tr


def oracle_mel(c, spec, fb, db=None):
    """(output in out_fmt, per item [max, min]); decibels before the clamp"""
    y = np.abs(spec) @ fb.astype(np.float64)
    st = None
    if db is not None:
        amin_k, ref_term = pm.db_device_params(db[0], db[1])
        y = 10.0 * np.log10(np.maximum(y, float(amin_k))) - float(ref_term)
        st = np.stack([y.reshape(y.shape[0], -1).max(1), y.reshape(y.shape[0], -1).min(1)], 1)
    return to_layout(y, c['out_fmt']), st


def db_clamp(y, item_max, dyn):
    return np.maximum(y, (item_max - dyn).reshape((-1,) + (1,) * (y.ndim - 1)))


def mel_reference(c, x_bct, window, fb):
    """(|z| . B from numpy's rfft in longdouble, its linear bound), both (B, C, F, n_filt) float64"""
    z, s = gm.ref_stft(c, x_bct, window)
    K = z.shape[-1]
    if mel_stage(c['n_fft']) == 'gen':
        stage = gm.stft_bound(c, z, s)
    else:
        b = stft_bound(c, x_bct, window, build_dft_fwd(c['n_fft']))
        stage = np.hypot(b[..., 0::2], b[..., 1::2])
    mag = np.abs(z)
    fbl = fb.astype(np.float64)
    want = (mag @ fb.astype(gm.LD)).astype(np.float64)
    return want, (K + 5) * U * (mag.astype(np.float64) @ fbl) + stage @ fbl


def db_interval(want, bound, db):
    """the decibel reference as an interval: [db(want - bound), db(want + bound)] widened by to_db_bound at each end"""
    ref, amin, _ = db
    amin_k, ref_term = pm.db_device_params(ref, amin)

    def f(v):
        return 10.0 * np.log10(np.maximum(v, float(amin_k))) - float(ref_term)
    lo, hi = want - bound, want + bound
    return f(lo) - pm.to_db_bound(lo, amin, ref), f(hi) + pm.to_db_bound(hi, amin, ref)
