"""A checker for the tuned transforms at the sizes that are not 256 ... 2048: k_stft_mr<plan> (18 plans of kpr_fft_mr.h), k_stft_bs<M>,
k_stft_big<R> (kpr_stft_kernels.h) and their inverses k_irfft_mr, k_irfft_bs<M>, k_irfft_big<R>, k_irfft<NC> (kpr_istft_kernels.h) in
front of k_ola.  It needs no GPU and does not import the package.  Shared by tests/test_tuned_fft_model_host.py (CPU) and
tests/test_tuned_fft_gate.py (GPU).

  routes      fast_nfft, big_nfft, bluestein_m, bluestein_ok, the 18 plan typedefs (P, L, N, PIN, LIN, ROW, holds, bin, mr_row_stride),
              fft_family, forward_geom, the two-kernel part of istft_route under istft_path 2, and launch_framewise's grid with each
              kernel's per_block, per_cu and LDS size; the CU count is a parameter
  emulations  everything AROUND the transform core, index by index in the kernel's own decomposition: workgroup -> wave -> group ->
              lane with the idle lanes, every trip of the grid-stride loop (k_stft_mr: the samples, validity bits and output base
              fetched one trip ahead are state carried between trips), frame_pos with cfast = 0, the wave-uniform easy / slow fetch,
              clamped offsets and validity bits, the window pairs, k_stft_big's n = r + R j gather, the in-place pairing, the three
              epilogues, spec_base / spec_stride stores and the per-group readlane of the output base; for the inverses the Hermitian
              pre-pairing, the stores into [frame][win], the zero tail, then generic_model.emulate_ola.  The core (F::run,
              cfft_forward, the chirp products) is an exact float64 DFT of what the lanes hold: its arithmetic is what the GPU run
              measures.  Every load and store is checked against its buffer (OutOfBounds); an output element written twice or never
              is an error (WriteError).  Each emulation takes a named mutant = one wrong line.
  case tables FWD_CASES, INV_CASES (the smallest shapes at which each id of BRANCHES exists) and multi_trip_cases(cus), which are
              built from the CU count: a second trip of k_stft_mr needs more than 4 * 3 * CUs frame groups.

The bounds (per element, u = 2^-24, first order in u), derived the way generic_model derives R + 7
  A register butterfly of radix R (2, 3, 4, 5, 8 = the Dft<R> of kpr_fft.h / kpr_fft_mr.h) with the rounded twiddle and the product in
  front of it costs at most R + 7 per term relative to the term (generic_model's docstring: 4.83, 8.8, 5.83, 11.7; radix 8 is three
  radix-2 levels with W_8 inside: 3 * 4.83 = 14.5 <= 15).  The composite register DFTs are chains of those (dft_ab<A, B>: DFT-A,
  W_120 constant, DFT-B), so a plan's constant is the sum over the STAGES of its passes:
    MrFft<R2, R3>      DFT-20 = (4, 5), DFT-R2 (4 | 5 | 10 = (2, 5) | 20 = (4, 5)), DFT-R3 (2 | 4 | 5)
    TwoPassFft<N1, N2> DFT-N1, DFT-N2 with 6 = (2, 3), 8, 12 = (4, 3), 15 = (3, 5), 16 = (4, 4), 20 = (4, 5), 24 = (8, 3)
    cfft_forward<M>    log2 M radix-2 levels, whatever radices the passes group them into: 9 log2 M
    |Z^ - Z| <= u C sum_n |z_n|,  C = sum over stages of (R + 7)                                     (PLAN_CONST)
  k_stft_big / k_irfft_big: C = 9 * 10 (the 1024-point core) + (R + 7) (the W_NB^{rk} product and the radix-R combine).
  Bluestein: a_n = z_n w_n (rounded chirp and product: 3.83), A = FFT_M(a) (C_M sum |a|), A Bt (rounded Bt and product: 3.83 per term),
  the second FFT_M (C_M sum_j |A_j Bt_j|), the final chirp product (3.83).  With |A_j| <= sum |a_n| = sum |z_n| every one of these is
  relative to sum_j |Bt_j| * sum_n |z_n|, and the kernel's Bt carries the 1 / 2 of the pairing, so for the full-scale Z
    C = 2 * (2 * 9 log2 M + 3 * 3.83) * sum_j |Bt_j|                                                 (sum |Bt| from the restated table)
  forward   the frame sample x_n w_n is one product; X_k takes Z_k and Z_{N-k} with total weight 1 each, through the pairing
            (3.9 <= 4, generic_model):  c = 2 C + 4 + 1,  |X^_k - X_k| <= u c S,  S = sum_n |x_n w_n|.
            Magnitude and phase widen it as generic_model.stft_bound does.
  inverse   c = 2 (C + 4) + 3 on S_n = (Hermitian sum of |X_k|, DC / Nyquist imaginary parts dropped) / n_fft * |synth_n|; k_ola adds
            (overlap - 1) u sum |terms|  (generic_model.ref_istft).
Nothing here is fitted to what the kernels return.
"""
import numpy as np

import generic_model as gm
from generic_model import CL, CF, COMPLEX, MAGNITUDE, PHASE, LD, OutOfBounds, PHASE_FLOOR, PHASE_LEFT_OUT  # noqa: F401

U32 = 2.0 ** -24
K_PTS = 16                        # kPts: complex points per lane of the power-of-two FFT
MR_P = 20                         # kMrP
LDS_LIMIT = 160 * 1024            # launch_framewise
WAVES = 4                         # waves per workgroup of the mr / bs / pow2 kernels (256 threads)
REG_FWD = 2e-5                    # tests/test_gpu_parity.py: test_stft_non_power_of_two, test_stft_big_transform_sizes
REG_INV = 4e-6                    # tests/test_fft_family_labels.py REG
FAST = (256, 512, 1024, 2048)
BIG = {4096: 2, 8192: 4}          # n_fft -> R
# the plan typedefs of kpr_host_fft.h
MR_TYPEDEFS = {160: (4, 1), 200: (5, 1), 320: (4, 2), 400: (10, 1), 640: (4, 4), 800: (20, 1), 1000: (5, 5)}
TP_TYPEDEFS = {96: (8, 6), 120: (4, 15), 192: (8, 12), 240: (8, 15), 360: (12, 15), 384: (16, 12), 480: (16, 15), 600: (20, 15),
               720: (15, 24), 768: (16, 24), 960: (20, 24)}
STAGES = {1: (), 2: (2,), 3: (3,), 4: (4,), 5: (5,), 6: (2, 3), 8: (8,), 10: (2, 5), 12: (4, 3), 15: (3, 5), 16: (4, 4), 20: (4, 5),
          24: (8, 3)}
PASS_CONST = 7


class WriteError(Exception):
    """an emulation wrote an output element twice, or left one unwritten"""


# =================================================================================================================
# routes (kpr_host_fft.h, kpr_host_stft.h, kpr_host_istft.h, kpr_host.h)
# =================================================================================================================
def fast_nfft(n_fft):
    return n_fft in FAST


def big_nfft(n_fft):
    return n_fft in BIG


def bluestein_m(n_fft):
    if n_fft < 4 or n_fft & 1:
        return 0
    ncr, m = n_fft // 2, 128
    while m < 2 * ncr - 1:
        m *= 2
    return m if m <= 1024 else 0


def bluestein_ok(n_fft, win):
    return not fast_nfft(n_fft) and bluestein_m(n_fft) > 0 and win <= n_fft


class Plan:
    """MrFft<R2, R3> / TwoPassFft<N1, N2>: what the kernels need to know"""

    def __init__(self, n_fft):
        self.n_fft = n_fft
        if n_fft in MR_TYPEDEFS:
            r2, r3 = MR_TYPEDEFS[n_fft]
            self.two_pass, self.P, self.L = False, MR_P, r2 * r3
            self.N = self.P * self.L
            self.PIN, self.LIN, self.ROW = self.P, self.L, self.N
            self.RL = r3 if r3 > 1 else r2
            self.stages = STAGES[20] + STAGES[r2] + STAGES[r3]
        else:
            n1, n2 = TP_TYPEDEFS[n_fft]
            self.two_pass, self.N1, self.N2 = True, n1, n2
            self.N, self.P = n1 * n2, max(n1, n2)
            self.L = self.P
            self.PIN, self.LIN, self.ROW = n1, n2, (n2 | 1) * n1
            self.stages = STAGES[n1] + STAGES[n2]
        self.G = 64 // self.L

    def holds(self, l, r):
        return (l < self.N1) & (r < self.N2) if self.two_pass else np.ones(np.broadcast(l, r).shape, bool)

    def bin(self, l, r):
        if self.two_pass:
            return l + self.N1 * r
        return l + self.L * (r // self.RL) + (self.N // self.RL) * (r % self.RL)

    def row_stride(self):
        return max(self.ROW, self.N + 1) | 1

    def lds_bytes(self):
        return 4 * 2 * (4 * self.G * self.row_stride() + 3 * self.N)

    def const(self):
        return sum(r + PASS_CONST for r in self.stages)


PLANS = {n: Plan(n) for n in sorted(list(MR_TYPEDEFS) + list(TP_TYPEDEFS))}


def mixed_radix_plan(n_fft):
    return 0 if n_fft not in PLANS else 2 if PLANS[n_fft].two_pass else 1


FAM_POW2, FAM_MR, FAM_BS, FAM_BIG, FAM_OTHER = 'pow2', 'mr', 'bs', 'big', 'other'


def fft_family(n_fft, win, mixed_radix=1):
    """fft_family as far as the tuned families go (FAM_GEN / FAM_GEMM: 'other')"""
    if fast_nfft(n_fft):
        return FAM_POW2
    if bluestein_ok(n_fft, win):
        return FAM_MR if mixed_radix_plan(n_fft) and mixed_radix else FAM_BS
    if big_nfft(n_fft):
        return FAM_BIG
    return FAM_OTHER


def forward_family(c):
    """forward_geom crops win_length to n_fft before fft_family sees it"""
    return fft_family(c['n_fft'], min(c['win'], c['n_fft']), c.get('mixed_radix', 1))


def inverse_family(c):
    """istft_route under istft_path 2: fft_family of the caller's geometry, win_length as given"""
    return fft_family(c['n_fft'], c['win'], c.get('mixed_radix', 1))


def bs_row_words(m):
    return (m + m // 32 + 24 + 3) // 4 * 4


def bs_slot_words(m, ncr):
    return bs_row_words(m) + 2 * ncr + 2 * (ncr + 1) + 2


def launch_grid(groups, per_block, per_cu, lds, cus):
    """launch_framewise"""
    per_cu = max(1, min(per_cu, LDS_LIMIT // lds))
    return max(1, min(-(-groups // per_block), per_cu * cus))


def launch_of(kernel, n_fft, total_frames, cus):
    """(label of kpr_last_launches, frames per group G, groups, per_block, grid, trips) of one framewise launch"""
    ncr = n_fft // 2
    if kernel in ('k_stft_mr', 'k_irfft_mr'):
        pl = PLANS[n_fft]
        g_, per_block, per_cu, lds = pl.G, 4, 3 if kernel == 'k_stft_mr' else 2, pl.lds_bytes()
        label = 'k_stft_mr<%d>' % pl.N if kernel == 'k_stft_mr' else kernel
    elif kernel in ('k_stft_bs', 'k_irfft_bs'):
        m = bluestein_m(n_fft)
        g_, per_block, per_cu = 64 // (m // K_PTS), 4, 2
        slot = bs_slot_words(m, ncr) if kernel == 'k_stft_bs' else bs_row_words(m)
        lds, label = 4 * (4 * g_ * slot + 2 * (3 * m + ncr + 2)), kernel
    elif kernel in ('k_stft_big', 'k_irfft_big'):
        r = BIG[n_fft]
        nw = 4 if r == 2 else 2
        g_, per_block, label = 1, nw, kernel
        per_cu, lds = (2, 8 * nw * (r * 1024 + 1)) if kernel == 'k_stft_big' else (1, 8 * 2 * nw * (r * 1024 + 1))
    else:
        assert kernel == 'k_irfft'
        g1 = 64 // (ncr // K_PTS)
        g_, per_block, per_cu, lds, label = 4 * g1, 1, 2, 4 * (4 * g1 * ncr + 4 * g1 * (2 * ncr + 8)), kernel
    groups = -(-total_frames // g_)
    grid = launch_grid(groups, per_block, per_cu, lds, cus)
    return dict(label=label, G=g_, groups=groups, per_block=per_block, grid=grid, trips=-(-groups // (grid * per_block)), lds=lds)


FWD_KERNEL = {FAM_MR: 'k_stft_mr', FAM_BS: 'k_stft_bs', FAM_BIG: 'k_stft_big'}
INV_KERNEL = {FAM_MR: 'k_irfft_mr', FAM_BS: 'k_irfft_bs', FAM_BIG: 'k_irfft_big', FAM_POW2: 'k_irfft'}


def forward_launches(c, cus):
    return launch_of(FWD_KERNEL[forward_family(c)], c['n_fft'], c['B'] * c['C'] * gm.frames_of(c), cus)['label']


def inverse_launches(c, cus):
    """the launch list of kpr_istft_f32 under istft_path 2"""
    fam = inverse_family(c)
    if fam == FAM_OTHER:
        return 'k_gemm + k_fill_cols + k_ola' if c['win'] > c['n_fft'] else None
    return INV_KERNEL[fam] + ' + k_ola'


# =================================================================================================================
# tables (kpr_host_fft.h: build_twiddles, build_bluestein)
# =================================================================================================================
def build_twiddles(n_fft, f32=True):
    """build_twiddles: exp(-2 pi i j / n_fft) computed in double and rounded to float32 (f32 = False: left in double, which is what
    the emulations pair with -- the rounding of the table is part of what the GPU run measures)"""
    a = -2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / np.float64(n_fft)
    if not f32:
        return np.cos(a) + 1j * np.sin(a)
    return (np.cos(a).astype(np.float32) + 1j * np.sin(a).astype(np.float32)).astype(np.complex128)


_BS = {}


def build_bluestein(n_fft):
    """(w[M] (0 beyond NCr), Bt[M], t[NCr + 1]) with the float32 values the host uploads"""
    if n_fft in _BS:
        return _BS[n_fft]
    ncr, m = n_fft // 2, bluestein_m(n_fft)
    n = np.arange(ncr, dtype=np.int64)
    a = -np.pi * ((n * n) % (2 * ncr)).astype(np.float64) / np.float64(ncr)
    wr, wi = np.cos(a), np.sin(a)
    b = np.zeros(m, np.complex128)
    b[:ncr] = wr - 1j * wi
    b[m - np.arange(1, ncr)] = wr[1:] - 1j * wi[1:]
    kn = (np.arange(m, dtype=np.int64)[:, None] * np.arange(m, dtype=np.int64)[None, :]) % m
    ang = -2.0 * np.pi * kn.astype(np.float64) / np.float64(m)
    bt = ((np.cos(ang) + 1j * np.sin(ang)) * b[None, :]).sum(-1) / (2.0 * m)
    ak = -2.0 * np.pi * np.arange(ncr + 1, dtype=np.float64) / np.float64(n_fft)

    def f32(z):
        return (z.real.astype(np.float32) + 1j * z.imag.astype(np.float32)).astype(np.complex128)

    w = np.zeros(m, np.complex128)
    w[:ncr] = f32(wr + 1j * wi)
    _BS[n_fft] = (w, f32(bt), f32(np.cos(ak) + 1j * np.sin(ak)))
    return _BS[n_fft]


def pow2_const(m):
    return 9 * int(round(np.log2(m)))


def fft_const(fam, n_fft):
    """C of the docstring: |Z^ - Z| <= u C sum |z_n| for the full-scale half-size transform"""
    if fam == FAM_MR:
        return PLANS[n_fft].const()
    if fam == FAM_BIG:
        return pow2_const(1024) + BIG[n_fft] + PASS_CONST
    if fam == FAM_POW2:
        return pow2_const(n_fft // 2)
    assert fam == FAM_BS
    return 2 * (2 * pow2_const(bluestein_m(n_fft)) + 3 * 3.83) * float(np.abs(build_bluestein(n_fft)[1]).sum())


# =================================================================================================================
# geometry shared by the emulations
# =================================================================================================================
def geom_of(b, c, f, t_len, n_fft, win, hop, pad_left, in_cl, out_cl):
    return dict(B=b, C=c, F=f, T=t_len, total=b * c * f, n_fft=n_fft, win=win, hop=hop, pad_left=pad_left, K=n_fft // 2 + 1,
                in_cl=bool(in_cl and c > 1), out_cl=bool(out_cl and c > 1))


def frame_pos(g, gf):
    """frame_pos with cfast = 0 (below 2^31 frames)"""
    bc, f = gf // g['F'], gf % g['F']
    b, ch = bc // g['C'], bc % g['C']
    if g['in_cl']:
        sig_off, es = b * g['T'] * g['C'] + ch, np.full_like(bc, g['C'])
    else:
        sig_off, es = bc * g['T'], np.ones_like(bc)
    return dict(b=b, c=ch, f=f, bc=bc, sig_off=sig_off, es=es, s0=f * g['hop'] - g['pad_left'])


def spec_base(g, p, q):
    if g['out_cl']:
        return ((p['b'] * g['F'] + p['f']) * q) * g['C'] + p['c']
    return (p['bc'] * g['F'] + p['f']) * q


def spec_stride(g, mutant=None):
    return g['C'] if g['out_cl'] and mutant != 'ostride1' else 1


def _load(flat, addr, live):
    """flat[addr] with the addresses of the waves that run (`live`, broadcast against addr) checked against the buffer"""
    a = addr[np.broadcast_to(live, addr.shape)]
    if a.size and (int(a.min()) < 0 or int(a.max()) >= flat.size):
        raise OutOfBounds('load at %d .. %d of a buffer of %d' % (a.min(), a.max(), flat.size))
    return flat[np.clip(addr, 0, flat.size - 1)]


class Out:
    """an output buffer: NaN at first, every element written exactly once"""

    def __init__(self, size, dtype):
        self.v = np.full(size, np.nan, dtype)
        self.n = np.zeros(size, np.int32)

    def store(self, addr, vals):
        addr = np.asarray(addr).ravel()
        if addr.size and (int(addr.min()) < 0 or int(addr.max()) >= self.v.size):
            raise OutOfBounds('store at %d .. %d of a buffer of %d' % (addr.min(), addr.max(), self.v.size))
        np.add.at(self.n, addr, 1)
        self.v[addr] = np.asarray(vals).ravel()

    def done(self):
        if (self.n != 1).any():
            raise WriteError('%d elements written twice, %d never' % ((self.n > 1).sum(), (self.n == 0).sum()))
        return self.v


def window_pairs(window, win, count, scale, mutant=None):
    """stage_window_pairs (and the hand-written copies): (count, 2) with zeros from `win` on"""
    n = 2 * np.arange(count)
    a, b = window[np.minimum(n, win - 1)], window[np.minimum(n + 1, win - 1)]
    odd_ok = (n < win) if mutant == 'win_pair' else (n + 1 < win)
    return np.stack([np.where(n < win, scale * a, 0.0), np.where(odd_ok, scale * b, 0.0)], -1)


def epilogue(mode, v, mutant=None):
    """complex | magnitude | bin_phase: atan2 with the sign of a zero real part dropped (x + 0)"""
    if mode == COMPLEX:
        return v
    if mode == MAGNITUDE:
        return np.hypot(v.real, v.imag)
    return np.arctan2(v.imag, v.real if mutant == 'phase_zero' else v.real + 0.0)


def pair_forward(zk, zp, t, dc, mutant=None):
    """the in-place pairing on rows that hold Z / 2: (X[k], X[N - k])"""
    e, d = zk + np.conj(zp), zk - np.conj(zp)
    td = d * t
    xk, xq = e - 1j * td, np.conj(e + 1j * td)
    if mutant != 'dc_imag':
        xk, xq = np.where(dc, xk.real, xk), np.where(dc, xq.real, xq)
    return xk, xq


def fwd_geom(c):
    n = c['n_fft']
    return geom_of(c['B'], c['C'], gm.frames_of(c), c['T'], n, min(c['win'], n), c['hop'], n - c['hop'] if c['pad_begin'] else 0,
                   c['in_fmt'] == CL, c['out_fmt'] == CL)


def fwd_out_shape(c, g):
    return gm.shape_of(c['out_fmt'], g['B'], g['C'], g['F'], g['K'])


# =================================================================================================================
# forward: k_stft_mr
# =================================================================================================================
def emulate_stft_mr(c, x, window, cus, mutant=None, ids=None):
    """k_stft_mr<plan> on x (the memory image of c['in_fmt'], 8-byte aligned): the output's memory image.  ids: a set that
    receives the branch ids the run reaches"""
    ids = set() if ids is None else ids
    g, pl = fwd_geom(c), PLANS[c['n_fft']]
    L, N, G, PIN, LIN, K = pl.L, pl.N, pl.G, pl.PIN, pl.LIN, pl.N + 1
    la = launch_of('k_stft_mr', c['n_fft'], g['total'], cus)
    ngroups, nw = la['groups'], la['grid'] * WAVES
    xf = np.asarray(x, np.float64).ravel()
    window = np.asarray(window, np.float64)
    lane = np.arange(64)
    active = lane < G * L
    grp = np.where(active, lane // L, 0)
    l = np.where(active, lane - grp * L, 0)
    li = l if mutant == 'li_clamp' else np.minimum(l, LIN - 1)
    has_in = active if mutant == 'has_in' else active & (l < LIN)
    winl = window_pairs(window, g['win'], N, 0.5, mutant)
    tab = build_twiddles(c['n_fft'], f32=False)
    m_ = np.arange(PIN)
    ostride = spec_stride(g, mutant)
    out = Out(g['total'] * K, np.complex128 if c['mode'] == COMPLEX else np.float64)
    if (~active).any():
        ids.add('lanes.idle')
    if (active & (l >= LIN)).any():
        ids.add('lanes.no_input')
    if g['total'] < G:
        ids.add('frames<G')
    if g['total'] % G:
        ids.add('group.partial')

    def fetch(gi, live):
        """MR_FETCH of group gi[w] for the waves with live[w]: (zr (W, 64, PIN, 2), vm (W, 64, PIN, 2), ob (W, 64))"""
        gf = gi[:, None] * G + grp[None, :]
        there = active[None, :] & (gf < g['total'])
        valid = has_in[None, :] & (gf < g['total'])
        p = frame_pos(g, np.where(there, gf, 0))
        ob = np.where(there, spec_base(g, p, K), -1)
        aligned = (p['sig_off'] + p['s0']) % 2 == 0
        easy = valid & (p['es'] == 1) & (p['s0'] >= 0) & (p['s0'] + 2 * N <= g['T']) & (g['win'] >= 2 * N) & aligned
        wave_easy = (easy | ~has_in[None, :]).all(1)
        n_ = 2 * (li[:, None] + LIN * m_[None, :])                                     # (64, PIN)
        # the 8-byte fetch
        a_e = (p['sig_off'] + np.where(valid, p['s0'], 0))[:, :, None] + n_[None]
        # the clamped fetch
        es, omax = p['es'][:, :, None], ((g['T'] - 1) * p['es'])[:, :, None]
        o0 = ((p['s0'] + 2 * li[None, :]) * p['es'])[:, :, None] + m_[None, None, :] * (2 * LIN) * es
        o1 = o0 + es
        lo0, lo1 = (o0 >= 0, o1 >= 0) if mutant != 'lower_bound' else (True, True)
        k0 = valid[:, :, None] & (n_[None] < g['win']) & lo0 & (o0 <= omax)
        k1 = valid[:, :, None] & (n_[None] + 1 < g['win']) & lo1 & (o1 <= omax)
        a_s0, a_s1 = p['sig_off'][:, :, None] + np.clip(o0, 0, omax), p['sig_off'][:, :, None] + np.clip(o1, 0, omax)
        we = wave_easy[:, None, None]
        a0, a1 = np.where(we, a_e, a_s0), np.where(we, a_e + 1, a_s1)
        lv = live[:, None, None]
        zr = np.stack([_load(xf, a0, lv), _load(xf, a1, lv)], -1)
        vm = np.stack([np.where(we, valid[:, :, None], k0), np.where(we, valid[:, :, None], k1)], -1)
        # which fetch paths ran
        lw = live & (gi * G < g['total'])
        if (wave_easy & lw).any():
            ids.add('fetch.easy')
        slow = ~wave_easy & lw
        if slow.any():
            sv = valid & slow[:, None]
            if (sv & (p['s0'] < 0)).any():
                ids.add('fetch.slow.pad_begin')
            if (sv & (p['s0'] + min(g['win'], 2 * N) > g['T'])).any():
                ids.add('fetch.slow.pad_end')
            if (sv & ~aligned & (p['es'] == 1)).any():
                ids.add('fetch.slow.misaligned')
            if (sv & (p['es'] != 1)).any():
                ids.add('fetch.slow.interleaved')
            if g['win'] < 2 * N:
                ids.add('fetch.slow.win<n_fft')
            if (slow & (easy & has_in[None, :]).any(1)).any():
                ids.add('fetch.mixed_wave')
        return zr, vm, ob

    grpi = np.arange(nw)
    live = grpi < ngroups
    zr, vm, ob_next = fetch(grpi, live)
    # the cells of a frame: point n = l + LIN m of group q sits in lane q L + l, register m
    cell_l, cell_m = np.arange(N) % LIN, np.arange(N) // LIN
    rl, rr = np.meshgrid(np.arange(L), np.arange(pl.P), indexing='ij')
    held = pl.holds(rl, rr)
    bins = pl.bin(rl, rr)[held]
    k = np.arange(N // 2 + 1)
    kp = np.where(k == 0, 0, N - k)
    trips = 0
    while live.any():
        trips += 1
        ob = ob_next
        # (a lane index beyond the window pairs would read the twiddle table behind them in LDS: no fault, and no lane with input does)
        z = np.where(vm, zr, 0.0) * winl[np.minimum(li[:, None] + LIN * m_[None, :], N - 1)][None]       # (W, 64, PIN, 2)
        gn = grpi + nw
        nxt = gn < ngroups
        if nxt.any():
            zr2, vm2, ob2 = fetch(gn, nxt)
            zr, vm = np.where(nxt[:, None, None, None], zr2, zr), np.where(nxt[:, None, None, None], vm2, vm)
            ob_next = np.where(nxt[:, None], ob2, ob_next)
        if mutant == 'ob_wrong_trip':
            ob = ob_next
        zc = z[..., 0] + 1j * z[..., 1]
        frames = np.stack([zc[:, q * L + cell_l, cell_m] for q in range(G)], 1)           # (W, G, N): what the lanes with input hold
        spec = np.fft.fft(frames, axis=-1)                                                # F::run: Z / 2 (the window carries the 1 / 2)
        rows = np.full((nw, G, pl.row_stride()), np.nan + 0j)
        if bins.size != N or np.unique(bins).size != N:
            raise WriteError('bin over holds is no bijection onto [0, N)')
        rows[:, :, bins] = spec[:, :, bins]
        xk, xq = pair_forward(rows[:, :, k], rows[:, :, kp], tab[k][None, None], (k == 0)[None, None], mutant)
        rows[:, :, k] = xk
        upper = np.ones_like(k, bool) if mutant == 'nyq_guard' else 2 * k != N
        rows[:, :, N - k[upper]] = xq[:, :, upper]
        vals = epilogue(c['mode'], rows[:, :, :K], mutant)
        if c['mode'] == PHASE:
            if (rows[live][:, :, 0].real < 0).any():
                ids.add('phase.dc_negative')
            if (rows[live][:, :, N].real < 0).any():
                ids.add('phase.nyquist_negative')
        for gq in range(G):
            o = ob[:, gq if mutant == 'readlane' else gq * L]
            go = live if mutant == 'o_skip' else live & (o >= 0)
            out.store(o[go][:, None] + np.arange(K)[None, :] * ostride, vals[go, gq])
        grpi, live = gn, nxt
    ids.add('trips=1' if trips == 1 else 'trips>=2')
    if trips >= 2:
        ids.add('fwd.mr.trips>=2')
        if ngroups % nw:
            ids.add('trips>=2.last_partial')
    return out.done().reshape(fwd_out_shape(c, g))


# =================================================================================================================
# forward: k_stft_bs, k_stft_big
# =================================================================================================================
def fetch_frame_slow(xf, g, p, valid, n, live, mutant=None):
    """the clamped branch of fetch_frame + mask_frame: samples at frame offsets n (last axis), zero where the validity bit is clear.
    (Bluestein never takes the other branch: it asks for win >= 2 M > n_fft.)"""
    es, omax = p['es'][..., None], ((g['T'] - 1) * p['es'])[..., None]
    o = (p['s0'][..., None] + n) * es
    lo = (o >= 0) if mutant != 'lower_bound' else True
    ok = valid[..., None] & (n < g['win']) & lo & (o <= omax)
    v = _load(xf, p['sig_off'][..., None] + np.clip(o, 0, omax), live)
    return np.where(ok, v, 0.0)


def emulate_stft_bs(c, x, window, cus, mutant=None, ids=None):
    ids = set() if ids is None else ids
    g, n_fft = fwd_geom(c), c['n_fft']
    ncr, m = n_fft // 2, bluestein_m(n_fft)
    K, L = ncr + 1, m // K_PTS
    G = 64 // L
    la = launch_of('k_stft_bs', n_fft, g['total'], cus)
    ngroups, nw = la['groups'], la['grid'] * WAVES
    xf, window = np.asarray(x, np.float64).ravel(), np.asarray(window, np.float64)
    winl = window_pairs(window, g['win'], m, 1.0, mutant)
    tk = build_twiddles(n_fft, f32=False)                                                 # t[0 .. NCr] of the Bluestein table
    lane = np.arange(64)
    fl, grp = lane & (L - 1), lane // L
    j = fl[:, None] + L * np.arange(K_PTS)[None, :]                                       # (64, 16): point of lane and register
    ostride = spec_stride(g, mutant)
    out = Out(g['total'] * K, np.complex128 if c['mode'] == COMPLEX else np.float64)
    ids.add('bs.ncr.2' if ncr == 2 else 'bs.ncr.odd' if ncr & 1 else 'bs.ncr.even')
    if m == 2 * ncr:
        ids.add('bs.M.exact_fit')
    if g['total'] < G:
        ids.add('frames<G')
    if g['total'] % G:
        ids.add('group.partial')
    grpi, trips = np.arange(nw), 0
    while (grpi < ngroups).any():
        trips += 1
        live = grpi < ngroups
        gf = grpi[:, None] * G + grp[None, :]
        valid = gf < g['total']
        p = frame_pos(g, np.where(valid, gf, 0))
        sv = valid & live[:, None]
        for name, cond in (('pad_begin', p['s0'] < 0), ('pad_end', p['s0'] + g['win'] > g['T']), ('interleaved', p['es'] != 1)):
            if (sv & cond).any():
                ids.add('fetch.slow.' + name)
        zx = fetch_frame_slow(xf, g, p, valid, 2 * j[None], live[:, None, None], mutant) * winl[j, 0][None]
        zy = fetch_frame_slow(xf, g, p, valid, 2 * j[None] + 1, live[:, None, None], mutant) * winl[j, 1][None]
        # the chirp products and both M-point FFTs: Z / 2 of the NCr points (the chirp table is zero beyond NCr)
        pts = (zx + 1j * zy).reshape(nw, G, L, K_PTS).transpose(0, 1, 3, 2).reshape(nw, G, m)     # point fl + L m
        zrow = 0.5 * np.fft.fft(pts[:, :, :ncr], axis=-1)
        kk = np.arange(m)                                                                 # every lane / register: k = fl + L m
        kc = np.minimum(kk, ncr)
        kpi = ncr - kc
        zp = zrow[:, :, np.where(kpi == ncr, 0, kpi)]
        zk = np.where((kk < ncr)[None, None], zrow[:, :, np.minimum(kk, ncr - 1)], zrow[:, :, :1])
        e, d = zk + np.conj(zp), zk - np.conj(zp)
        xv = e - 1j * (d * tk[kc][None, None])
        if mutant != 'dc_imag':
            xv = np.where(((kc == 0) | (kc == ncr))[None, None], xv.real, xv)
        keep = kk < ncr if mutant == 'k_le_ncr' else kk <= ncr
        stage = np.full((nw, G, K), np.nan + 0j)
        stage[:, :, kk[keep]] = xv[:, :, keep]
        vals = epilogue(c['mode'], stage, mutant)
        if c['mode'] == PHASE:
            okf = (live[:, None] & valid.reshape(nw, G, L)[:, :, 0])
            if (stage[okf][:, 0].real < 0).any():
                ids.add('phase.dc_negative')
            if (stage[okf][:, ncr].real < 0).any():
                ids.add('phase.nyquist_negative')
        base = spec_base(g, p, K).reshape(nw, G, L)[:, :, 0]
        go = live[:, None] & valid.reshape(nw, G, L)[:, :, 0]
        out.store(base[go][:, None] + np.arange(K)[None, :] * ostride, vals[go])
        grpi = grpi + nw
    ids.add('trips=1' if trips == 1 else 'trips>=2')
    if trips >= 2:
        ids.add('fwd.bs.trips>=2')
        if ngroups % nw:
            ids.add('trips>=2.last_partial')
    return out.done().reshape(fwd_out_shape(c, g))


def emulate_stft_big(c, x, window, cus, mutant=None, ids=None):
    ids = set() if ids is None else ids
    g, n_fft = fwd_geom(c), c['n_fft']
    R = BIG[n_fft]
    NC, NB = 1024, R * 1024
    K = NB + 1
    la = launch_of('k_stft_big', n_fft, g['total'], cus)
    nw = la['grid'] * la['per_block']
    xf, window = np.asarray(x, np.float64).ravel(), np.asarray(window, np.float64)
    twbig = build_twiddles(n_fft, f32=False)
    ostride = spec_stride(g, mutant)
    out = Out(g['total'] * K, np.complex128 if c['mode'] == COMPLEX else np.float64)
    jj = np.arange(NC)                                                                    # j = fl + 64 m
    k = np.arange(NB // 2 + 1)
    kp = np.where(k == 0, 0, NB - k)
    gf, trips = np.arange(nw), 0
    while (gf < g['total']).any():
        trips += 1
        live = gf < g['total']
        p = frame_pos(g, np.where(live, gf, 0))
        sv = live
        for name, cond in (('pad_begin', p['s0'] < 0), ('pad_end', p['s0'] + g['win'] > g['T']), ('interleaved', p['es'] != 1)):
            if (sv & cond).any():
                ids.add('fetch.slow.' + name)
        e_r = []
        for r in range(R):
            n = r * NC + jj if mutant == 'gather' else r + R * jj
            wa = window[np.minimum(2 * n, g['win'] - 1)] * (2 * n < g['win'])
            wb = window[np.minimum(2 * n + 1, g['win'] - 1)] * (2 * n + 1 < g['win'])
            a = fetch_frame_slow(xf, g, p, live, 2 * n[None], live[:, None], mutant) * 0.5 * wa[None]
            b = fetch_frame_slow(xf, g, p, live, 2 * n[None] + 1, live[:, None], mutant) * 0.5 * wb[None]
            e_r.append(np.fft.fft(a + 1j * b, axis=-1))                                   # E_r[k], k < 1024
        zrow = np.full((nw, NB + 1), np.nan + 0j)
        for s in range(R):                                                                # Z[k + 1024 s] = sum_r W_R^{rs} W_NB^{rk} E_r[k]
            acc = 0
            for r in range(R):
                acc = acc + np.exp(-2j * np.pi * r * s / R) * np.exp(-2j * np.pi * r * jj / NB)[None] * e_r[r]
            zrow[:, NC * s + jj] = acc
        xk, xq = pair_forward(zrow[:, k], zrow[:, kp], twbig[k][None], (k == 0)[None], mutant)
        zrow[:, k] = xk
        upper = np.ones_like(k, bool) if mutant == 'nyq_guard' else 2 * k != NB
        zrow[:, NB - k[upper]] = xq[:, upper]
        vals = epilogue(c['mode'], zrow, mutant)
        if c['mode'] == PHASE:
            if (zrow[live][:, 0].real < 0).any():
                ids.add('phase.dc_negative')
            if (zrow[live][:, NB].real < 0).any():
                ids.add('phase.nyquist_negative')
        out.store(spec_base(g, p, K)[live][:, None] + np.arange(K)[None, :] * ostride, vals[live])
        gf = gf + nw
    ids.add('trips=1' if trips == 1 else 'trips>=2')
    if trips >= 2:
        ids.add('fwd.big.trips>=2')
        if g['total'] % nw:
            ids.add('trips>=2.last_partial')
    return out.done().reshape(fwd_out_shape(c, g))


FWD_EMULATION = {FAM_MR: emulate_stft_mr, FAM_BS: emulate_stft_bs, FAM_BIG: emulate_stft_big}


def emulate_stft(c, x, window, cus, mutant=None, ids=None):
    return FWD_EMULATION[forward_family(c)](c, x, window, cus, mutant, ids)


def static_fwd_ids(c):
    """the ids a forward case reaches whatever its data"""
    fam, n_fft, win = forward_family(c), c['n_fft'], c['win']
    ids = {'fwd.mr.%d' % n_fft if fam == FAM_MR else 'fwd.bs.M%d' % bluestein_m(n_fft) if fam == FAM_BS else 'fwd.big.R%d' % BIG[n_fft]}
    ids.add('win.<n_fft' if win < n_fft else 'win.=n_fft' if win == n_fft else 'win.>n_fft')
    if win & 1:
        ids.add('win.odd')
    if c['T'] < n_fft:
        ids.add('T<n_fft')
    ids.add('mode.' + ('complex', 'magnitude', 'phase')[c['mode']])
    if c['C'] == 1:
        ids.add('C1')
    else:
        ids.update({'in.cl' if c['in_fmt'] == CL else 'in.cf', 'out.cl' if c['out_fmt'] == CL else 'out.cf'})
    return ids


# =================================================================================================================
# inverse: k_irfft_mr, k_irfft_bs, k_irfft_big, k_irfft  (+ k_ola: generic_model.emulate_ola)
# =================================================================================================================
def inv_geom(c):
    return geom_of(c['B'], c['C'], c['F'], 0, c['n_fft'], c['win'], c['hop'], 0, c['wave_fmt'] == CL, c['spec_fmt'] == CL)


def pair_inverse(xk, xp, t, dc, mutant=None):
    """conj(2 Z[k]) from X[k] and X[N - k] (the kernels' e, d, od); dc: k == 0, where the imaginary parts are dropped"""
    if mutant != 'inv_dcnyq':
        xk, xp = np.where(dc, xk.real, xk), np.where(dc, xp.real, xp)
    xpc = np.conj(xp)
    e, d = xk + xpc, xk - xpc
    od = d * np.conj(t)
    return np.conj(e + 1j * od)


def emulate_irfft(c, spec, synth, cus, mutant=None, ids=None):
    """the inverse FFT kernel of the case's family on `spec` (the memory image of c['spec_fmt']): the [total_frames][win] workspace"""
    ids = set() if ids is None else ids
    fam, g, n_fft, win = inverse_family(c), inv_geom(c), c['n_fft'], c['win']
    N, K = n_fft // 2, n_fft // 2 + 1
    la = launch_of(INV_KERNEL[fam], n_fft, g['total'], cus)
    G = la['G']
    nslots = la['grid'] * la['per_block']                                                 # groups in flight per trip
    sf = np.asarray(spec, np.complex128).ravel()
    synth = np.asarray(synth, np.float64)
    tab = build_twiddles(n_fft, f32=False)                # (k_irfft_bs reads the same values from t[0 .. NCr] of its table)
    ostride = spec_stride(g, mutant)
    out = Out(g['total'] * win, np.float64)
    ids.add({FAM_MR: 'inv.mr.%d' % n_fft, FAM_BS: 'inv.bs.M%d' % bluestein_m(n_fft), FAM_BIG: 'inv.big.R%d' % BIG.get(n_fft, 0),
             FAM_POW2: 'inv.pow2.NC%d' % N}[fam])
    ids.add('inv.spec.cl' if g['out_cl'] else 'inv.spec.cf')
    if win > n_fft:
        ids.add('inv.pow2.win>n_fft' if fam == FAM_POW2 else 'inv.big.win>n_fft')
    if fam == FAM_MR:
        pl = PLANS[n_fft]
        if pl.L * pl.G < 64:
            ids.add('lanes.idle')
        if pl.L > pl.LIN:
            ids.add('lanes.no_input')
    if g['total'] % G:
        ids.add('group.partial')
    # the loads: bins k < N and N - k of every frame of the group (clamped lanes re-read bins that exist); k_irfft_big and the
    # channels_first branch of k_irfft stream the K bins of the row instead
    k = np.arange(N)
    sc = 1.0 / n_fft
    grpi, trips = np.arange(nslots), 0
    while (grpi < la['groups']).any():
        trips += 1
        live = grpi < la['groups']
        gf = grpi[:, None] * G + np.arange(G)[None, :]
        valid = (gf < g['total']) & live[:, None]
        p = frame_pos(g, np.where(valid, gf, 0))
        base = spec_base(g, p, K)
        # (k_irfft and k_irfft_bs form the address of a frame beyond the end from its own gf but mask the VALUE; here: frame 0)
        lv = live[:, None, None]
        xk = _load(sf, base[:, :, None] + k[None, None, :] * ostride, lv)
        xp = _load(sf, base[:, :, None] + (N - k)[None, None, :] * ostride, lv)
        if (xk[valid][:, 0].imag != 0).any() or (xp[valid][:, 0].imag != 0).any():
            ids.add('inv.dcnyq.imag')
        zc = pair_inverse(xk, xp, tab[k][None, None], (k == 0)[None, None], mutant)       # conj(2 Z)
        y = np.conj(np.fft.fft(zc, axis=-1))                                              # 2 N z[n], z[n] = x[2n] + i x[2n+1]
        fr = np.zeros(y.shape[:2] + (2 * N,))
        fr[..., 0::2], fr[..., 1::2] = y.real * sc, y.imag * sc                          # 1 / (2 N): the 1 / 2 of the pairing, the 1 / N of the inverse
        n = np.arange(N)
        ev, od_ = 2 * n < win, (2 * n < win if mutant == 'inv_store' else 2 * n + 1 < win)
        wv = synth[np.minimum(np.arange(2 * N), win - 1)]
        fo = gf[valid] * win
        out.store(fo[:, None] + 2 * n[ev][None, :], (fr[..., 0::2] * wv[0::2])[valid][:, ev])
        out.store(fo[:, None] + 2 * n[od_][None, :] + 1, (fr[..., 1::2] * wv[1::2])[valid][:, od_])
        if win > 2 * N and mutant != 'inv_tail':
            tail = np.arange(2 * N, win)
            out.store(fo[:, None] + tail[None, :], np.zeros((fo.size, tail.size)))
        grpi = grpi + nslots
    ids.add('trips=1' if trips == 1 else 'trips>=2')
    if trips >= 2:
        ids.add('inv.%s.trips>=2' % fam)
        if la['groups'] % nslots:
            ids.add('trips>=2.last_partial')
    return out.done().reshape(g['total'], win)


def emulate_istft(c, spec, synth, cus, mutant=None, ids=None):
    return gm.emulate_ola(dict(c, ty='f64'), emulate_irfft(c, spec, synth, cus, mutant, ids))


# =================================================================================================================
# references and bounds
# =================================================================================================================
def stft_bound(c, want, s):
    cc = 2 * fft_const(forward_family(c), c['n_fft']) + 5
    bound = U32 * cc * s * np.ones(want.shape)
    mag = np.abs(want).astype(np.float64)
    if c['mode'] == MAGNITUDE:
        return bound + 2 * U32 * mag
    if c['mode'] == PHASE:
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.arcsin(np.minimum(bound / mag, 1.0)) + 4 * U32 * np.pi
    return bound


def ref_istft(c, spec_bcfk, synth):
    """generic_model.ref_istft with this file's constant: (waveform (B, C, t_out) in longdouble, its bound)"""
    n, win, hop, f_ = c['n_fft'], c['win'], c['hop'], c['F']
    spec = np.asarray(spec_bcfk).astype(np.clongdouble)
    synth = np.asarray(synth, LD)
    frames = np.fft.irfft(spec, n=n, axis=-1)[..., :win]
    mag = np.abs(spec)
    edge = [0, n // 2]
    mag[..., edge] = np.abs(spec[..., edge].real)
    herm = 2 * mag.sum(-1, keepdims=True) - mag[..., edge].sum(-1, keepdims=True)
    if win > n:
        frames = np.pad(frames, [(0, 0)] * 3 + [(0, win - n)])
    frames = frames * synth
    s = herm / n * np.abs(synth) * (np.arange(win) < n)
    cc = 2 * (fft_const(inverse_family(c), n) + 4) + 3
    b_, c_ = spec.shape[:2]
    t_out = (f_ - 1) * hop + win
    out, bound, terms, count = (np.zeros((b_, c_, t_out), LD) for _ in range(4))
    for i in range(f_):
        sl = slice(i * hop, i * hop + win)
        out[..., sl] += frames[:, :, i]
        bound[..., sl] += U32 * cc * s[:, :, i]
        terms[..., sl] += np.abs(frames[:, :, i])
        count[..., sl] += 1
    bound += np.maximum(count - 1, 0) * U32 * terms
    return out, bound.astype(np.float64)


# =================================================================================================================
# branch ids and case tables
# =================================================================================================================
def _ids():
    ids = []
    for d in ('fwd', 'inv'):
        ids += ['%s.mr.%d' % (d, n) for n in PLANS] + ['%s.bs.M%d' % (d, m) for m in (128, 256, 512, 1024)]
        ids += ['%s.big.R%d' % (d, r) for r in (2, 4)]
    ids += ['inv.pow2.NC%d' % nc for nc in (128, 256, 512, 1024)]
    ids += ['lanes.idle', 'lanes.no_input', 'group.partial', 'frames<G', 'trips=1', 'trips>=2', 'trips>=2.last_partial']
    ids += ['%s.trips>=2' % k for k in ('fwd.mr', 'fwd.bs', 'fwd.big', 'inv.mr', 'inv.bs', 'inv.big', 'inv.pow2')]
    ids += ['fetch.easy', 'fetch.mixed_wave', 'T<n_fft'] + ['fetch.slow.' + s for s in ('pad_begin', 'pad_end', 'misaligned', 'interleaved', 'win<n_fft')]
    ids += ['win.odd', 'win.<n_fft', 'win.=n_fft', 'win.>n_fft', 'bs.ncr.odd', 'bs.ncr.even', 'bs.ncr.2', 'bs.M.exact_fit']
    ids += ['mode.complex', 'mode.magnitude', 'mode.phase', 'in.cf', 'in.cl', 'out.cf', 'out.cl', 'C1', 'phase.dc_negative', 'phase.nyquist_negative']
    ids += ['inv.dcnyq.imag', 'inv.spec.cf', 'inv.spec.cl', 'inv.pow2.win>n_fft', 'inv.big.win>n_fft']
    return tuple(ids)


BRANCHES = _ids()
EXCLUDED = {
    'frame_pos.2^31': 'the 64-bit division branch of frame_pos needs 2^31 frames: no output of that size fits a test',
    'cfast=1': 'channel-fastest frame numbering is set by stft_route for FAM_POW2 forward launches only',
    'inv.mr.win>n_fft': 'the zero-tail loop of k_irfft_mr never runs: bluestein_ok refuses win_length > n_fft, so fft_family sends these '
                        'calls to k_gemm + k_fill_cols + k_ola (asserted from the restated route)',
    'inv.bs.win>n_fft': 'as for k_irfft_mr: k_irfft_bs is never launched with win_length > n_fft',
}


def fcase(id, n_fft, win=None, hop=None, B=2, C=2, frames=3, T=None, pads=(False, False), fmts=(CF, CF), mode=COMPLEX, **kw):
    win = n_fft if win is None else win
    hop = max(1, (2 * n_fft) // 3) if hop is None else hop
    T = max(win, n_fft) + hop * (frames - 1) + hop // 2 if T is None else T
    return dict(id=id, ty='f32', n_fft=n_fft, win=win, hop=hop, B=B, C=C, T=T, pad_begin=pads[0], pad_end=pads[1], in_fmt=fmts[0],
                out_fmt=fmts[1], mode=mode, **kw)


def _fwd_cases():
    PB, PE = (True, False), (False, True)
    opts = [dict(), dict(pads=PB, fmts=(CL, CF)), dict(pads=PE, fmts=(CF, CL), mode=MAGNITUDE), dict(fmts=(CL, CL), mode=PHASE),
            dict(pads=PB, C=1), dict(pads=PE, B=1, C=3)]
    cases = [fcase('plan %d' % n, n, **opts[i % len(opts)]) for i, n in enumerate(PLANS)]
    cases += [
        # one aligned signal, even hop: every wave takes the 8-byte fetch; 41 frames leave the third group of 16 partial
        fcase('160 easy, last group partial', 160, hop=80, B=1, C=1, frames=41),
        # odd hop: every second frame of a wave is misaligned and moves the whole wave to the clamped fetch
        fcase('160 odd hop', 160, hop=81, B=1, C=1, frames=20),
        fcase('1000 two frames per wave', 1000, hop=500, B=1, C=1, frames=5),
        # odd T in channels_first: the second signal starts at an odd offset
        fcase('96 odd T', 96, hop=48, B=1, C=2, T=96 * 3 + 1),
        # eight signals of exactly one frame fill a wave that takes the 8-byte fetch: lanes 6, 7 of a frame (L 8 > LIN 6) hold no input
        # and fetch from the start of their signal, which is as long as the 96 samples that lane 5 reaches
        fcase('96 eight signals of one frame', 96, hop=96, B=4, C=2, T=96),
        fcase('160 T 30', 160, hop=10, B=2, C=1, T=30, pads=PE),
        fcase('400 win 301', 400, win=301, hop=100, pads=PB),
        fcase('400 win 500', 400, win=500, hop=100, frames=4, mode=MAGNITUDE),
        fcase('480 C 3 in cl', 480, B=1, C=3, fmts=(CL, CF)), fcase('600 C 3 out cl', 600, B=1, C=3, fmts=(CF, CL), mode=PHASE),
        # Bluestein at the edges of M, with odd n_fft / 2, and n_fft 400 on both kernels
        fcase('bs 4', 4, hop=1, frames=40, pads=PB), fcase('bs 6', 6, hop=2, frames=30, fmts=(CL, CL), mode=MAGNITUDE),
        fcase('bs 126', 126, pads=PE, mode=PHASE), fcase('bs 128', 128, fmts=(CF, CL)), fcase('bs 130', 130, fmts=(CL, CF), pads=PB),
        fcase('bs 254', 254, win=201, mode=MAGNITUDE), fcase('bs 258', 258, pads=PE, C=1), fcase('bs 510', 510, B=1, C=3, fmts=(CL, CL)),
        fcase('bs 514', 514, mode=PHASE), fcase('bs 1022', 1022, pads=PB, B=1), fcase('bs 400', 400, mixed_radix=0, pads=PE),
        fcase('bs 300 T 70', 300, hop=50, B=1, C=2, T=70, pads=PE),
        # the sub-FFT kernels
        fcase('big 4096 win 3001', 4096, win=3001, hop=1024, B=1, C=1, frames=5, pads=PB),
        fcase('big 8192 win 5000', 8192, win=5000, hop=4096, B=1, C=1, frames=5, pads=PE, mode=MAGNITUDE),
        fcase('big 4096 cl', 4096, hop=2048, B=1, C=2, frames=2, fmts=(CL, CL), mode=PHASE),
        fcase('big 8192', 8192, hop=8192, B=1, C=2, frames=1, fmts=(CF, CL)),
    ]
    return cases


FWD_CASES = _fwd_cases()


def icase(id, n_fft, win=None, hop=None, B=2, C=2, F=3, fmts=(CF, CF), **kw):
    win = n_fft if win is None else win
    hop = max(1, win // 3) if hop is None else hop
    return dict(id=id, ty='f32', n_fft=n_fft, win=win, hop=hop, B=B, C=C, F=F, spec_fmt=fmts[0], wave_fmt=fmts[1], **kw)


def _inv_cases():
    fm = [(CF, CF), (CL, CF), (CF, CL), (CL, CL)]
    cases = [icase('plan %d' % n, n, fmts=fm[i % 4], C=1 + i % 3) for i, n in enumerate(PLANS)]
    cases += [icase('bs %d' % n, n, fmts=fm[i % 4], F=5) for i, n in enumerate((4, 6, 126, 128, 130, 254, 258, 510, 514, 1022))]
    cases += [icase('bs 400', 400, mixed_radix=0), icase('400 win 301', 400, win=301), icase('bs 300 win 199', 300, win=199, fmts=(CL, CL)),
              icase('big 4096', 4096, B=1, F=5, fmts=(CL, CF)), icase('big 8192', 8192, B=1, C=1, F=3),
              icase('big 4096 win 4500', 4096, win=4500, B=1, F=2), icase('big 8192 win 8193', 8192, win=8193, B=1, C=2, F=2, fmts=(CL, CL)),
              icase('big 4096 win 3001', 4096, win=3001, B=1, C=1, F=3)]
    cases += [icase('pow2 %d' % n, n, fmts=fm[i % 4], F=5) for i, n in enumerate(FAST)]
    cases += [icase('pow2 256 win 300', 256, win=300), icase('pow2 1024 win 777', 1024, win=777, fmts=(CL, CL))]
    return cases


INV_CASES = _inv_cases()


def multi_trip_cases(cus):
    """(forward, inverse) cases whose launch takes a second trip of the grid-stride loop on a device with `cus` compute units: just
    over one trip's worth of frames, so the second trip is also a partial one"""
    def frames_for(kernel, n_fft, extra):
        la = launch_of(kernel, n_fft, 1 << 40, cus)
        return la['grid'] * la['per_block'] * la['G'] + extra

    fwd = []
    for id, n_fft, hop, kernel, extra, kw in (
            ('trips 160 hop 2', 160, 2, 'k_stft_mr', 37, {}), ('trips 160 hop 1', 160, 1, 'k_stft_mr', 37, dict(mode=MAGNITUDE)),
            ('trips 1000 hop 2', 1000, 2, 'k_stft_mr', 3, {}),
            ('trips bs 6 hop 1', 6, 1, 'k_stft_bs', 21, {}), ('trips big 8192 hop 1', 8192, 1, 'k_stft_big', 3, {}),
            ('trips big 4096 hop 1', 4096, 1, 'k_stft_big', 5, dict(mode=PHASE))):
        f = frames_for(kernel, n_fft, extra)
        fwd.append(fcase(id, n_fft, hop=hop, B=1, C=1, T=n_fft + hop * (f - 1), multi=True, **kw))
    inv = []
    for id, n_fft, kernel, extra in (('trips 160', 160, 'k_irfft_mr', 37), ('trips bs 6', 6, 'k_irfft_bs', 21),
                                     ('trips big 4096', 4096, 'k_irfft_big', 3), ('trips big 8192', 8192, 'k_irfft_big', 1),
                                     ('trips pow2 256', 256, 'k_irfft', 5)):
        inv.append(icase(id, n_fft, hop=max(1, n_fft // 4), B=1, C=1, F=frames_for(kernel, n_fft, extra), multi=True))
    return fwd, inv


def fwd_input(c):
    if c.get('zero'):
        return np.zeros((c['B'], c['C'], c['T']), np.float32)
    return np.random.default_rng(gm.seed_of(c)).standard_normal((c['B'], c['C'], c['T'])).astype(np.float32)


def fwd_window(c):
    return gm.hann(c['win'], 'f32')


def inv_input(c):
    rng = np.random.default_rng(gm.seed_of(c))
    shape = (c['B'], c['C'], c['F'], c['n_fft'] // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def inv_window(c):
    return gm.synth_window(c)


# =================================================================================================================
# mutants: one wrong line each
# =================================================================================================================
FWD_MUTANTS = {
    'li_clamp': 'k_stft_mr: li = min(l, LIN - 1) -> l',
    'has_in': 'k_stft_mr: has_in ignores l < LIN',
    'win_pair': 'window pairs: n + 1 < win -> n < win',
    'lower_bound': 'validity bits: (unsigned)o <= (unsigned)omax -> o <= omax',
    'ob_wrong_trip': 'k_stft_mr: the output base of the trip that was just fetched (ob_next) instead of this trip\'s',
    'o_skip': 'k_stft_mr: the `o < 0` skip dropped',
    'readlane': 'k_stft_mr: readlane at gq instead of gq * L',
    'nyq_guard': 'pairing: `if (2 * k != N)` dropped',
    'dc_imag': 'pairing: the imaginary parts of DC and Nyquist kept',
    'k_le_ncr': 'k_stft_bs: k <= ncr -> k < ncr',
    'ostride1': 'spec_stride 1 on channels_last',
    'gather': 'k_stft_big: n = r + R j -> r * 1024 + j',
    'phase_zero': 'bin_phase: atan2f(y, x + 0.0f) -> atan2f(y, x)',
}
INV_MUTANTS = {
    'inv_dcnyq': 'inverse pre-pairing: the imaginary parts of DC and Nyquist kept',
    'inv_tail': 'the zero tail for win > n_fft dropped',
    'inv_store': 'frame stores: 2 n + 1 < win -> 2 n < win',
    'ostride1': 'spec_stride 1 on channels_last',
}
# mutants that change no output, with the reason
NEUTRAL = {
    'phase_zero': 'the -0 real parts of an all-zero frame come out of the transform core (k_stft_bs at n_fft 400: products of zeros with the '
                  'negative parts of the chirp), which the emulation replaces by an exact DFT whose zeros are +0; the GPU gate pins the '
                  'line: test_zero_input_gives_zero_output[2-bs 400] fails without it (360 of 4020 phases are pi)',
    'has_in': 'pass 1 of TwoPassFft stores only the lanes l < N2 = LIN, the frame is built from those lanes alone, and the easy / slow '
              'decision of a lane l >= LIN is the one of lane LIN - 1 of the same frame (same frame_pos): has_in only spares those '
              'lanes the masks',
    'win_pair': 'the clamped fetch clears the validity bit of every sample n >= win itself, the 8-byte fetch is taken only with '
                'win >= n_fft, and k_stft_big masks with its own comparison: the zeros of the window pairs are a second line of defence',
    'dc_imag': 'at k = 0 both operands of the pairing are Z[0], so e is real and d imaginary by construction and t[0] = (1, 0): the '
               'imaginary parts are exact zeros already (Bluestein at k = NCr: 1.2e-16 |Z|, from sin(pi) in the table).  The line '
               'matters for non-finite frames only; the GPU gate asserts the exact zeros',
    'nyq_guard': 'at 2 k = N the twiddle is -i: xk = e - i t d and xq = conj(e + i t d) are the same number conj(Z[N/2]) up to the '
                 'rounding of the table entry (cos(pi / 2) is 6e-17 in the table), and both are stored to row[N/2]',
}
