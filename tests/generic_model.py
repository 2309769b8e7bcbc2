"""A checker for the size-generic FFT engine of kapre_amd/csrc/kpr_generic_kernels.h (k_stft_gen<T,TWL>, k_irfft_gen<T,TWL> and their
gen_pass* helpers), for k_ola<T> behind it and for k_filterbank_f64, that needs no GPU and does not import the package.  Three parts,
shared by tests/test_generic_model_host.py (CPU) and tests/test_generic_gate.py (GPU):

  branch model   gen_plan / gen_fft_len / gen_lds / gen_fits / gen_grid of kpr_host_fft.h and the predicates of the kernels restated:
                 *_branches(case) returns the ids of BRANCHES a case reaches
  case tables    STFT_CASES, ISTFT_CASES, OLA_CASES, FB64_CASES: the smallest shapes at which each branch exists
  emulations     emulate_stft / emulate_istft / emulate_fb64: index by index in the kernels' own decomposition, in the element type of
                 the case (every intermediate is a numpy float32 or float64: no fused multiply-add, the kernel's order of operations).
                 Passes of radix 2, 3, 4, 5 are the register butterflies of gen_dft, radix 7 and the run-time radices the direct form
                 of gen_pass / gen_output with its float-reciprocal blk / rem / k, the twiddle index stepped modulo N, the clamped and
                 masked groups of four and the U-way clamping.  Every load and store is checked against the extent of its buffer
                 (OutOfBounds).  Each emulation takes a named mutant = one wrong line; a mutant that no table case tells from the
                 reference means the table is too weak.

The bounds (per element, u = 2^-24 or 2^-53, first order in u)
  One pass of radix R computes y = sum_r a_r w_r with |w_r| = 1.  Per term, relative to |a_r|:
    direct form   the table entry w is rounded (u), the complex product costs sqrt(2) * 2u = 2.83u (two products and one
                  addition per component), the term then goes through at most R - 1 additions: R + 2.83
    radix 2, 4    rounded twiddle and product 3.83, then 1 or 2 additions (the multiplication by +-i is exact): 4.83, 5.83
    radix 3       3.83, then through s = v1 + v2, m = v0 - s / 2, m +- d (3 roundings on a coefficient 1/2) and through
                  d = (v1 - v2) h, m +- d (difference, rounded h, product, sum: 4 roundings on sqrt(3)/2): 1.5 + 3.47 + 3.83 = 8.8
    radix 5       3.83, then through a = v0 + c1 t1 + c2 t2, a +- b (6 roundings on |c2| = 0.809) and through
                  b = s1 t3 + s2 t4, a +- b (5 roundings on s2 = 0.588): 4.86 + 2.94 + 3.83 = 11.7
  so every pass is covered by R + 7 (PASS_CONST; the issue proposed R + 4, which the radix 3 and 5 butterflies exceed).  Every
  intermediate value is a unit-modulus combination of a disjoint subset of the inputs, so the errors of the passes add up to
    |Z^ - Z| <= u * C * sum_n |z_n|,  C = sum over passes of (R_p + 7).
  forward   the frame sample x_n w_n is one product (1).  Unpacked sizes: c = C + 5 (the 5 covers the product; the rest is slack so
            that one constant serves both forms).  Packed sizes: X_k = E + W^k (-i D) takes Z_k and Z_{M-k} with total weight 1 EACH (two
            independent errors, each bounded by u C S since sum |z_n| <= sum |x_n w_n| = S), through one sum, an exact halving, for D a
            rounded twiddle and a product (3.83) and the final sum: (2 + 5.83) / 2 = 3.9 <= 4:  c = 2 C + 4 + 1.
            |X^_k - X_k| <= u * c * S,  S = sum_n |w_n x_n|.   Magnitude adds 2u |X_k| (hypot: one ulp), phase is
            asin(that bound / |X_k|) + 4u pi (atan2: two ulp of pi).
  inverse   S_n = (sum over the Hermitian extension of |X_k|, the imaginary parts of DC and Nyquist dropped) / n_fft * |synth_n|.
            Unpacked: c = C + 3 (rounded 1 / M, two products).  Packed: the pre-pairing costs 3.9 <= 4 per X_k as above, sum_k |Z_k|
            is at most the Hermitian sum and 1 / M = 2 / n_fft:  c = 2 (C + 4) + 3.
  k_ola     the frame errors add, plus (overlap - 1) u * sum |terms| for the additions.
  filterbank  n_freq * u * sum_k |x_k| |fb_k| (a product and at most n_freq - 1 additions per term).
Nothing here is fitted to what the kernels return.
"""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
import proto_generic_fft as pg  # noqa: E402

CL, CF = 'channels_last', 'channels_first'
DT = {'f32': np.float32, 'f64': np.float64}
CDT = {'f32': np.complex64, 'f64': np.complex128}
UNIT = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
LD = np.longdouble
COMPLEX, MAGNITUDE, PHASE = 0, 1, 2              # KPR_OUT_*

# ---- constants of the source, restated (tests/test_generic_model_host.py compares them with the source text) ----------------
THREADS = 256                     # kF64Threads
MAX_PASSES = 16                   # kGenMaxPasses
U_OF = {2: 2, 3: 2, 4: 2, 5: 1, 7: 2, 0: 1}     # gen_fft: the U of each switch arm (0 = default, run-time radix)
LDS_LIMIT = 160 * 1024            # gen_lds, gen_grid
LOAD_UNROLL = 8                   # k_stft_gen: samples per thread and trip of the frame load
SPEC_UNROLL = 4                   # k_irfft_gen: bins per thread and trip of the spectrum load
RT_GROUP = 4                      # gen_output: terms per group of the run-time radix
GRID_WGS = 256                    # gen_grid: workgroups = min(frames, 256 * per_cu)
GRID_PER_CU = 8                   # gen_grid: per_cu = clamp(160 KiB / lds, 1, 8)
GRID_1D_CAP = 256 * 16            # grid_1d's default cap (k_ola, k_filterbank_f64), blocks of 256
MAX_RADIX = 64                    # gen_plan: odd primes up to here
PASS_CONST = 7                    # the bound: R + 7 per pass (docstring)
REFUSAL_TEXT = 'does not fit in LDS (limit 10240 even / 5120 odd)'


class OutOfBounds(Exception):
    """an emulation formed an index outside the buffer it addresses"""


def seed_of(case, salt=0):
    return zlib.crc32(case['id'].encode()) + salt


def shape_of(fmt, b, c, *inner):
    return (b, *inner, c) if fmt == CL else (b, c, *inner)


def to_layout(a, fmt):
    """logical (b, c, *inner) -> the memory image of data format `fmt`"""
    return np.ascontiguousarray(np.moveaxis(a, 1, -1)) if fmt == CL else np.ascontiguousarray(a)


def from_layout(a, fmt):
    return np.moveaxis(a, -1, 1) if fmt == CL else a


def shortened(case):
    """the stride cases with their size cut down (same geometry otherwise): what the CPU tests run instead"""
    return dict(case, **case['short'], stride=False) if case.get('stride') else case


# =================================================================================================================
# plan and launch (kpr_host_fft.h)
# =================================================================================================================
def elem_bytes(ty):
    return 8 if ty == 'f32' else 16           # sizeof(float2), sizeof(double2)


def gen_lds(ty, n_fft):
    """gen_lds: (lds bytes, twiddle table in LDS) or None"""
    buf, tab = elem_bytes(ty) * pg.gen_fft_len(n_fft), elem_bytes(ty) * n_fft
    if 2 * buf > LDS_LIMIT:
        return None
    twl = 2 * buf + tab <= LDS_LIMIT
    return 2 * buf + (tab if twl else 0), twl


def gen_fits(ty, n_fft):
    """gen_fits: dict(m, radix, direct, lds, twl) or None.  float64 without a plan: one pass of radix m (a direct DFT)"""
    m = pg.gen_fft_len(n_fft)
    radix, direct = pg.gen_plan(m), False
    if radix is None:
        if ty != 'f64':
            return None
        radix, direct = [m], True
    lds = gen_lds(ty, n_fft)
    if lds is None:
        return None
    return dict(m=m, radix=radix, direct=direct, lds=lds[0], twl=lds[1], packed=m != n_fft)


def gen_grid(total_frames, lds):
    per_cu = max(1, min(GRID_PER_CU, LDS_LIMIT // max(lds, 1)))
    return max(1, min(total_frames, GRID_WGS * per_cu)), per_cu


def bluestein_m(n_fft):
    if n_fft < 4 or n_fft & 1:
        return 0
    m = 128
    while m < n_fft - 1:
        m *= 2
    return m if m <= 1024 else 0


def engine_takes(ty, n_fft, win, inverse=False):
    """does a call of this type and size run the generic engine?  float64: always (a size that does not fit is refused, not sent
    elsewhere).  float32: fft_family -- not a power-of-two size with a tuned kernel, no Bluestein / mixed-radix size, not 4096 /
    8192, win <= n_fft (the forward transform crops first) and a plan that fits."""
    if ty == 'f64':
        return True
    if not inverse:
        win = min(win, n_fft)
    if n_fft in (256, 512, 1024, 2048, 4096, 8192):
        return False
    if bluestein_m(n_fft) > 0 and win <= n_fft:
        return False
    return win <= n_fft and gen_fits('f32', n_fft) is not None


def _edges():
    """per type and parity: the last size with the twiddle table in LDS, the first without, the last that fits and (float64) the
    first refused, among the sizes the engine takes"""
    out = {}
    for ty in DT:
        for par in (0, 1):
            sizes = [n for n in range(2050 + par, 20484, 2) if engine_takes(ty, n, n)]
            fit = [n for n in sizes if gen_fits(ty, n) is not None]
            twl = [n for n in fit if gen_fits(ty, n)['twl']]
            e = {'twl_last': max(twl), 'twg_first': min(n for n in fit if n > max(twl)), 'fit_last': max(fit)}
            if ty == 'f64':
                e['refused'] = max(fit) + 2
            out[ty, par] = e
    return out


EDGES = _edges()
PARITY = ('even', 'odd')

PASS_KINDS = ('bf2', 'bf3', 'bf4', 'bf5', 'r7', 'rt')


def pass_kind(r):
    return {2: 'bf2', 3: 'bf3', 4: 'bf4', 5: 'bf5', 7: 'r7'}.get(r, 'rt')


def pass_items(n, r):
    """(items one thread is given one at a time, U): butterflies for the register form, outputs for the direct form"""
    return (n // r if r in (2, 3, 4, 5) else n), U_OF.get(r, U_OF[0])


def _ids():
    ids = []
    for ty in DT:
        p = ty + '.'
        ids += [p + s for s in ('packed', 'unpacked', 'n_fft=2', 'n_fft=3', 'twl', 'twg', 'grid.per_cu8', 'grid.per_cu1',
                                'grid.stride.per_cu8', 'grid.stride.per_cu1')]
        for par in PARITY:
            ids += [p + 'lds.%s.%s' % (par, e) for e in ('twl_last', 'twg_first', 'fit_last')]
        for kind in PASS_KINDS:
            ids += [p + 'pass.%s.first' % kind, p + 'pass.%s.later' % kind, p + 'inv.pass.%s' % kind]
        ids += [p + s for s in ('pass.rt.nomask', 'pass.rt.mask', 'pass.rt.61', 'pass.items<256', 'pass.steps>=2',
                                'pass.u2.slot2masked', 'pass.partial')]
        ids += [p + 'fwd.' + s for s in ('N<=2048', 'N>2048', 'win<n_fft', 'win>n_fft', 'pad_begin', 'pad_end', 'cf-cf', 'cf-cl',
                                         'cl-cf', 'cl-cl', 'C1', 'complex', 'magnitude', 'phase')]
        ids += [p + 'inv.' + s for s in ('packed', 'unpacked', 'twl', 'twg', 'M<=1024', 'M>1024', 'M%256', 'win<n_fft',
                                         'dcnyq.imag', 'grid.stride')]
        ids += [p + 'ola.' + s for s in ('hop>win', 'hop==win', 'win%hop', 'F1', 'cl', 'stride')]
    ids += ['f64.n_fft=4', 'f64.direct.packed', 'f64.direct.unpacked', 'f64.inv.direct', 'f64.inv.win>n_fft',
            'f64.lds.even.refused', 'f64.lds.odd.refused']
    ids += ['fb64.cf', 'fb64.cl', 'fb64.cl.C1', 'fb64.stride']
    return tuple(ids)


BRANCHES = _ids()
# float32 sizes without a plan or above the LDS limit take the DFT-as-GEMM family (tests/test_fft_family_labels.py), so float32 has
# no refusal, no direct DFT and no win > n_fft inverse: those ids do not exist above.  Nothing that exists is left out.
EXCLUDED = ()


def plan_branches(ty, n_fft, total_frames, fwd):
    """the plan / launch / pass ids of one launch of k_stft_gen (fwd) or k_irfft_gen"""
    p = ty + '.'
    pl = gen_fits(ty, n_fft)
    if pl is None:
        return {p + 'lds.%s.refused' % PARITY[n_fft & 1]}
    br = set()
    n = pl['m']
    if fwd:
        br.add(p + ('packed' if pl['packed'] else 'unpacked'))
        if n_fft in (2, 3, 4):
            br.add(p + 'n_fft=%d' % n_fft)
        br.add(p + ('twl' if pl['twl'] else 'twg'))
        for name, size in EDGES[ty, n_fft & 1].items():
            if size == n_fft:
                br.add(p + 'lds.%s.%s' % (PARITY[n_fft & 1], name))
        if pl['direct']:
            br.add(p + 'direct.' + ('packed' if pl['packed'] else 'unpacked'))
        grid, per_cu = gen_grid(total_frames, pl['lds'])
        if per_cu in (1, GRID_PER_CU):
            br.add(p + 'grid.per_cu%d' % per_cu)
            if total_frames > grid:
                br.add(p + 'grid.stride.per_cu%d' % per_cu)
    else:
        br.add(p + ('inv.packed' if pl['packed'] else 'inv.unpacked'))
        br.add(p + ('inv.twl' if pl['twl'] else 'inv.twg'))
        if pl['direct']:
            br.add(p + 'inv.direct')
        if total_frames > gen_grid(total_frames, pl['lds'])[0]:
            br.add(p + 'inv.grid.stride')
    for i, r in enumerate(pl['radix']):
        kind = pass_kind(r)
        if not fwd:
            br.add(p + 'inv.pass.' + kind)
            continue
        br.add(p + 'pass.%s.%s' % (kind, 'first' if i == 0 else 'later'))
        if kind == 'rt':
            br.add(p + ('pass.rt.nomask' if (r - 1) % RT_GROUP == 0 else 'pass.rt.mask'))
            if r == 61:
                br.add(p + 'pass.rt.61')
        items, u = pass_items(n, r)
        if items < THREADS:
            br.add(p + 'pass.items<256')
        if items > u * THREADS:
            br.add(p + 'pass.steps>=2')
        if u == 2 and 0 < items % (2 * THREADS) <= THREADS:
            br.add(p + 'pass.u2.slot2masked')
        if items % THREADS:
            br.add(p + 'pass.partial')
    return br


# =================================================================================================================
# the engine, element by element
# =================================================================================================================
def twiddles(ty, n_fft):
    """build_twiddles / build_twiddles64: (re, im) of exp(-2 pi i j / n_fft) in the element type"""
    if ty == 'f32':
        a = -2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / np.float64(n_fft)
        return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)
    a = LD(-2.0) * LD('3.14159265358979323846264338327950288') * np.arange(n_fft).astype(LD) / LD(n_fft)
    return np.cos(a).astype(np.float64), np.sin(a).astype(np.float64)


def _check(idx, n):
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise OutOfBounds('index %d .. %d of a buffer of %d' % (idx.min(), idx.max(), n))


def _ld(buf, idx):
    _check(idx, buf[0].shape[-1])
    return buf[0][..., idx], buf[1][..., idx]


def _st(buf, idx, v):
    _check(idx, buf[0].shape[-1])
    buf[0][..., idx], buf[1][..., idx] = v


def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _mul(a, w):
    return a[0] * w[0] - a[1] * w[1], a[0] * w[1] + a[1] * w[0]


def _muli(a, s):
    return (-a[1], a[0]) if s > 0 else (a[1], -a[0])


def gen_dft(r, v, sign, t):
    """gen_dft<R>: the register butterflies, in the kernel's order of operations"""
    if r == 2:
        return [_add(v[0], v[1]), _sub(v[0], v[1])]
    if r == 4:
        t0, t1, t2 = _add(v[0], v[2]), _sub(v[0], v[2]), _add(v[1], v[3])
        t3 = _muli(_sub(v[1], v[3]), sign)
        return [_add(t0, t2), _add(t1, t3), _sub(t0, t2), _sub(t1, t3)]
    if r == 3:
        h, half = t(0.86602540378443864676), t(0.5)
        s, d = _add(v[1], v[2]), _sub(v[1], v[2])
        d = _muli((d[0] * h, d[1] * h), sign)
        m = (v[0][0] - half * s[0], v[0][1] - half * s[1])
        return [_add(v[0], s), _add(m, d), _sub(m, d)]
    assert r == 5
    c1, c2 = t(0.30901699437494742410), t(-0.80901699437494742410)
    s1, s2 = t(0.95105651629515357212), t(0.58778525229247312917)
    t1, t2, t3, t4 = _add(v[1], v[4]), _add(v[2], v[3]), _sub(v[1], v[4]), _sub(v[2], v[3])
    a1 = (v[0][0] + c1 * t1[0] + c2 * t2[0], v[0][1] + c1 * t1[1] + c2 * t2[1])
    a2 = (v[0][0] + c2 * t1[0] + c1 * t2[0], v[0][1] + c2 * t1[1] + c1 * t2[1])
    b1 = _muli((s1 * t3[0] + s2 * t4[0], s1 * t3[1] + s2 * t4[1]), sign)
    b2 = _muli((s2 * t3[0] - s1 * t4[0], s2 * t3[1] - s1 * t4[1]), sign)
    return [_add(v[0], _add(t1, t2)), _add(a1, b1), _add(a2, b2), _sub(a2, b2), _sub(a1, b1)]


def thread_starts(items, u):
    """every first index `threadIdx.x + trip * U * 256 < items` of the pass loops, in thread order per trip"""
    trips = -(-items // (u * THREADS))
    o0 = (np.arange(THREADS)[None, :] + (np.arange(trips) * u * THREADS)[:, None]).ravel()
    return o0[o0 < items]


def _fresh(a):
    return np.full_like(a[0], np.nan), np.full_like(a[1], np.nan)


def gen_pass_bf(a, tw, tws, n, r, ns, sign, t):
    """gen_pass_bf<R, U>"""
    u_ = U_OF[r]
    nr, step = n // r, n // (ns * r)
    b = _fresh(a)
    j0 = thread_starts(nr, u_)
    for u in range(u_):
        tgt = j0 + u * THREADS
        j = np.minimum(tgt, nr - 1)
        k = j - pg.float_div(j, ns) * ns
        ob = (j - k) * r + k
        v = [_ld(a, j + q * nr) for q in range(r)]
        for q in range(1, r):
            w = _ld(tw, (q * k * step) * tws)
            v[q] = _mul(v[q], (w[0], -w[1]) if sign > 0 else w)
        v = gen_dft(r, v, sign, t)
        keep = tgt < nr
        for q in range(r):
            _st(b, ob[keep] + q * ns, (v[q][0][..., keep], v[q][1][..., keep]))
    return b


def gen_output(rc, a, tw, tws, j, nr, idx0, n, r, sign, mutant):
    """gen_output<RC>: one output of the direct form, the terms added in the kernel's order"""
    sr, si = _ld(a, j)
    idx = np.zeros_like(idx0)

    def step():
        nonlocal idx
        idx = idx + idx0
        if mutant != 'idx_mod':
            idx = np.where(idx >= n, idx - n, idx)
        return _ld(tw, idx * tws)

    def term(v, w):
        nonlocal sr, si
        wr, wi = w[0], (w[1] if sign < 0 else -w[1])
        sr = sr + (v[0] * wr - v[1] * wi)
        si = si + (v[0] * wi + v[1] * wr)

    if rc > 0:
        loaded = [(step(), _ld(a, j + q * nr)) for q in range(1, rc)]
        for w, v in loaded:
            term(v, w)
        return sr, si
    for r0 in range(1, r, RT_GROUP):
        loaded = []
        for u in range(RT_GROUP):
            w = step()
            q = min(r0 + u, r if mutant == 'clamp_R' else r - 1)
            loaded.append((w, _ld(a, j + q * nr)))
        for u, (w, v) in enumerate(loaded):
            if r0 + u < r or mutant == 'mask_r':
                term(v, w)
    return sr, si


def gen_pass(a, tw, tws, n, r, ns, sign, mutant):
    """gen_pass<RC, U>: RC = 7 (U = 2) or 0 (U = 1)"""
    rc = 7 if r == 7 else 0
    u_ = U_OF[rc]
    nr, step = n // r, n // (ns * r)
    b = _fresh(a)
    o0 = thread_starts(n, u_)
    for u in range(u_):
        tgt = o0 + u * THREADS
        o = np.minimum(tgt, n - 1)
        blk = pg.float_div(o, ns * r)
        rem = o - blk * (ns * r)
        k = rem - pg.float_div(rem, ns) * ns
        out = gen_output(rc, a, tw, tws, blk * ns + k, nr, rem * step, n, r, sign, mutant)
        keep = np.ones_like(tgt, bool) if mutant == 'store_mask' else tgt < n
        _st(b, tgt[keep], (out[0][..., keep], out[1][..., keep]))
    return b


def gen_fft(a, radix, tw, tws, sign, t, mutant=None):
    """gen_fft: a = (re, im) of shape (frames, N); returns the buffer that holds the result"""
    n, ns = a[0].shape[-1], 1
    for r in radix:
        if r in (2, 3, 4, 5):
            a = gen_pass_bf(a, tw, tws, n, r, ns, sign, t)
        else:
            a = gen_pass(a, tw, tws, n, r, ns, sign, mutant)
        ns *= r
    return a


def frame_index(b_, c_, f_, in_cl, out_cl, t_len, k_):
    """frame_pos / spec_base for every frame gf = (b C + c) F + f: (sig_off, es, spec base, spec stride)"""
    gf = np.arange(b_ * c_ * f_)
    bc, f = gf // f_, gf % f_
    b, c = bc // c_, bc % c_
    sig_off, es = (b * t_len * c_ + c, c_) if in_cl else (bc * t_len, 1)
    base, st = (((b * f_ + f) * k_) * c_ + c, c_) if out_cl else ((bc * f_ + f) * k_, 1)
    return f, sig_off, es, base, st


# =================================================================================================================
# forward: k_stft_gen
# =================================================================================================================
def scase(id, ty, n_fft, win=None, hop=None, B=2, C=2, T=None, pads=(False, False), fmts=(CF, CF), mode=COMPLEX, **kw):
    win = n_fft if win is None else win
    hop = max(1, (2 * n_fft) // 3) if hop is None else hop
    # two to three frames per signal, more at the tiny sizes: at least ~300 bins per signal, so that the largest error of a case is
    # a stable figure (the float64 regression bound compares it with the emulation's)
    T = max(2 * max(win, n_fft) + hop // 2 + 1, win + hop * (300 // (n_fft // 2 + 1))) if T is None else T
    return dict(id='%s %s' % (ty, id), ty=ty, n_fft=n_fft, win=win, hop=hop, B=B, C=C, T=T, pad_begin=pads[0], pad_end=pads[1],
                in_fmt=fmts[0], out_fmt=fmts[1], mode=mode, **kw)


def frames_of(c):
    t = c['T'] + (c['n_fft'] - c['hop'] if c['pad_begin'] else 0)
    if c['pad_end']:
        return -(-t // c['hop'])
    return 0 if t < c['win'] else 1 + (t - c['win']) // c['hop']


def _stft_cases():
    cases = []
    PB, PE = (True, False), (False, True)
    # (id, n_fft, keyword arguments): every (type, size) the engine takes becomes a case
    small = [
        ('2', 2, dict(pads=PB)), ('3', 3, dict(pads=PE, fmts=(CL, CL))), ('4', 4, dict(fmts=(CF, CL))),
        ('6', 6, dict(pads=PE, mode=MAGNITUDE)), ('10', 10, dict(pads=PB, fmts=(CL, CF), mode=PHASE)),
        ('11', 11, dict(fmts=(CL, CF))), ('13', 13, dict(pads=PE, mode=MAGNITUDE)), ('61', 61, dict(pads=PB, fmts=(CF, CL))),
        ('14', 14, dict(fmts=(CL, CL))), ('22', 22, dict(pads=PE)), ('26', 26, dict(pads=PB)), ('122', 122, dict(fmts=(CF, CL))),
        ('15 win 9', 15, dict(win=9, hop=4, pads=PE, C=1, fmts=(CL, CL))), ('15 win 20', 15, dict(win=20, hop=7, pads=PB)),
        ('77', 77, dict(pads=PE, mode=PHASE)), ('67', 67, dict(pads=PB, fmts=(CL, CL))), ('134', 134, dict(pads=PE, mode=MAGNITUDE)),
        ('1001', 1001, dict(pads=PB, fmts=(CL, CF))), ('1200', 1200, dict(win=1000, pads=PE, fmts=(CL, CL), mode=MAGNITUDE)),
        ('2050', 2050, dict(pads=PB, fmts=(CF, CL), mode=PHASE)), ('3003', 3003, dict(pads=PE, fmts=(CL, CF))),
        ('2050 win 2100', 2050, dict(win=2100, pads=PE)),
    ]
    for ty in DT:
        for id, n_fft, kw in small:
            if engine_takes(ty, n_fft, kw.get('win', n_fft)):
                cases.append(scase(id, ty, n_fft, **kw))
        # the LDS edges (and float64's direct DFT at the largest size it can have): one signal, two frames
        sizes = sorted({n for (t_, _), e in EDGES.items() if t_ == ty for n in e.values()} | ({10006} if ty == 'f64' else set()))
        for n_fft in sizes:
            cases.append(scase('edge %d' % n_fft, ty, n_fft, hop=n_fft, B=1, C=1, T=2 * n_fft, refused=gen_fits(ty, n_fft) is None))
        # the frame loop taken twice: 8 workgroups per CU (2048) and 1 per CU (256)
        cases.append(scase('stride 15/4', ty, 15, hop=4, B=1, C=2, T=15 + 4 * 1100, fmts=(CL, CF), stride=True, short=dict(T=15 + 4 * 3)))
        big = EDGES[ty, 0]['twl_last']                                      # 160 KiB of LDS: float64 5120, float32 10240
        cases.append(scase('stride %d' % big, ty, big, hop=big, B=1, C=1, T=big * 259, stride=True, short=dict(T=big * 2)))
    return cases


STFT_CASES = _stft_cases()


def stft_branches(c):
    p = c['ty'] + '.'
    f_ = frames_of(c)
    br = plan_branches(c['ty'], c['n_fft'], c['B'] * c['C'] * f_, True)
    if c.get('refused'):
        return br
    n_fft, win, t_len = c['n_fft'], min(c['win'], c['n_fft']), c['T']
    br.add(p + ('fwd.N<=2048' if n_fft <= LOAD_UNROLL * THREADS else 'fwd.N>2048'))
    if c['win'] < n_fft:
        br.add(p + 'fwd.win<n_fft')
    if c['win'] > n_fft:
        br.add(p + 'fwd.win>n_fft')
    s0 = np.arange(f_) * c['hop'] - (n_fft - c['hop'] if c['pad_begin'] else 0)
    if (s0 < 0).any():
        br.add(p + 'fwd.pad_begin')
    if (s0 + win - 1 >= t_len).any():
        br.add(p + 'fwd.pad_end')
    if c['C'] > 1:
        br.add(p + 'fwd.%s-%s' % ('cl' if c['in_fmt'] == CL else 'cf', 'cl' if c['out_fmt'] == CL else 'cf'))
    else:
        br.add(p + 'fwd.C1')
    br.add(p + 'fwd.' + ('complex', 'magnitude', 'phase')[c['mode']])
    return br


def hann(n, ty):
    """the periodic Hann window, computed in float64"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(DT[ty])


def stft_input(c):
    """logical (B, C, T) Gaussian samples, exact in the case's element type"""
    return np.random.default_rng(seed_of(c)).standard_normal((c['B'], c['C'], c['T'])).astype(DT[c['ty']])


def emulate_stft(c, x, window, mutant=None):
    """k_stft_gen on x (the memory image of c['in_fmt']) with `window` (win values of the element type): the output's memory image"""
    ty, t = c['ty'], DT[c['ty']]
    n, b_, c_, t_len, hop = c['n_fft'], c['B'], c['C'], c['T'], c['hop']
    win, k_, f_ = min(c['win'], n), n // 2 + 1, frames_of(c)
    pl = gen_fits(ty, n)
    m, packed = pl['m'], pl['packed']
    tws = 2 if packed and mutant != 'tws1' else 1
    tw = twiddles(ty, n)
    f, sig_off, es, base, st = frame_index(b_, c_, f_, c['in_fmt'] == CL and c_ > 1, c['out_fmt'] == CL and c_ > 1, t_len, k_)
    xf = np.asarray(x, t).ravel()
    window = np.asarray(window, t)
    # the frame load: clamped addresses, masked values
    s0 = f * hop - (n - hop if c['pad_begin'] else 0)
    nn = np.arange(n)
    tt = s0[:, None] + nn[None, :]
    addr = sig_off[:, None] + np.clip(tt, 0, t_len - 1) * es
    _check(addr, xf.size)
    ok = (tt >= 0) & (tt < t_len)
    if mutant != 'win_mask':
        ok &= (nn < win)[None, :]
    v = np.where(ok, xf[addr] * window[np.minimum(nn, win - 1)][None, :], t(0))
    a = (v[:, 0::2].copy(), v[:, 1::2].copy()) if packed else (v, np.zeros_like(v))
    r = gen_fft(a, pl['radix'], tw, tws, -1, t, mutant)
    k = np.arange(k_)
    if packed:
        half = t(0.5)
        zk = _ld(r, k if mutant == 'k_eq_M' else np.where(k == m, 0, k))
        zm = _ld(r, np.where(k == 0, 0, m - k))
        w = _ld(tw, k)
        e = (half * (zk[0] + zm[0]), half * (zk[1] - zm[1]))
        d = (half * (zk[0] - zm[0]), half * (zk[1] + zm[1]))
        vr, vi = _add(e, _mul((d[1], -d[0]), w))
    else:
        vr, vi = _ld(r, k)
    vi = np.where((k == 0) | (2 * k == n), t(0), vi)
    o = base[:, None] + k[None, :] * st
    if c['mode'] == COMPLEX:
        out = np.full(b_ * c_ * f_ * k_, np.nan, CDT[ty])
        out[o] = vr + 1j * vi
    else:
        out = np.full(b_ * c_ * f_ * k_, np.nan, t)
        out[o] = np.hypot(vr, vi) if c['mode'] == MAGNITUDE else np.arctan2(vi, vr)
    return out.reshape(shape_of(c['out_fmt'], b_, c_, f_, k_))


def ref_stft(c, x_bct, window):
    """longdouble reference with frames built as tests/test_f64.py builds them (tf.signal.stft): (X of shape (B, C, F, K) complex
    longdouble, S = sum_n |w_n x_n| of shape (B, C, F, 1))"""
    n, win, hop = c['n_fft'], c['win'], c['hop']
    x = np.asarray(x_bct, LD)
    if c['pad_begin']:
        x = np.pad(x, ((0, 0), (0, 0), (n - hop, 0)))
    f_ = frames_of(c)
    x = np.pad(x, ((0, 0), (0, 0), (0, max(0, (f_ - 1) * hop + win - x.shape[-1]))))
    idx = np.arange(win)[None, :] + hop * np.arange(f_)[:, None]
    frames = (x[..., idx] * np.asarray(window, LD))[..., :n]               # rfft(n = n_fft) crops win > n_fft
    return np.fft.rfft(frames, n=n, axis=-1), np.abs(frames).sum(-1, keepdims=True).astype(np.float64)


def fft_const(radix):
    return sum(r + PASS_CONST for r in radix)


def stft_bound(c, want, s):
    """per element (docstring): complex and magnitude as absolute errors, phase as an angle"""
    pl = gen_fits(c['ty'], c['n_fft'])
    cc = 2 * fft_const(pl['radix']) + 5 if pl['packed'] else fft_const(pl['radix']) + 5
    u = UNIT[c['ty']]
    bound = u * cc * s * np.ones(want.shape)
    mag = np.abs(want).astype(np.float64)
    if c['mode'] == MAGNITUDE:
        return bound + 2 * u * mag
    if c['mode'] == PHASE:
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.arcsin(np.minimum(bound / mag, 1.0)) + 4 * u * np.pi
    return bound


def stft_want(c, want):
    return want if c['mode'] == COMPLEX else np.abs(want) if c['mode'] == MAGNITUDE else np.angle(want)


PHASE_FLOOR = 1e-2            # phase is compared at bins with |want| >= this share of the largest
PHASE_LEFT_OUT = 0.02         # at most this share of the bins may be left out


def stft_error(c, got, want):
    """(|error| per element, elements compared): phase is compared as angle(exp(i (got - want))) where |want| is large enough"""
    if c['mode'] != PHASE:
        return np.abs(got.astype(want.dtype if c['mode'] == COMPLEX else LD) - stft_want(c, want)).astype(np.float64), np.ones(want.shape, bool)
    use = np.abs(want) >= PHASE_FLOOR * np.abs(want).max()
    d = got.astype(LD) - np.angle(want)
    return np.abs(np.angle(np.exp(1j * d))).astype(np.float64), use


# =================================================================================================================
# inverse: k_irfft_gen + k_ola
# =================================================================================================================
def icase(id, ty, n_fft, win=None, hop=None, B=2, C=2, F=None, fmts=(CF, CF), **kw):
    """fmts: (spectrogram layout, waveform layout); three frames per signal, more at the tiny sizes (see scase)"""
    win = n_fft if win is None else win
    F = max(3, min(64, 300 // n_fft)) if F is None else F
    hop = max(1, win // 3) if hop is None else hop
    return dict(id='%s %s' % (ty, id), ty=ty, n_fft=n_fft, win=win, hop=hop, B=B, C=C, F=F, spec_fmt=fmts[0], wave_fmt=fmts[1], **kw)


def _istft_cases():
    inv, ola = [], []
    sizes = [
        ('3', 3, {}), ('4', 4, dict(fmts=(CL, CF))), ('6', 6, {}), ('10', 10, dict(fmts=(CF, CL))), ('15 win 9', 15, dict(win=9)),
        ('15 win 20', 15, dict(win=20, fmts=(CL, CL))), ('22', 22, {}), ('26', 26, {}), ('122', 122, {}), ('14', 14, {}), ('67', 67, dict(fmts=(CL, CL))),
        ('134', 134, dict(win=100)), ('77', 77, dict(fmts=(CL, CF))), ('1001', 1001, {}), ('1200', 1200, dict(win=1000, fmts=(CF, CL))),
        ('2050', 2050, dict(fmts=(CL, CL))), ('3003', 3003, dict(B=1)),
    ]
    for ty in DT:
        for id, n_fft, kw in sizes:
            if engine_takes(ty, n_fft, kw.get('win', n_fft), inverse=True):
                inv.append(icase(id, ty, n_fft, **kw))
        for par in (0, 1):                                                  # the twiddle table in global memory
            n_fft = EDGES[ty, par]['twg_first']
            inv.append(icase('edge %d' % n_fft, ty, n_fft, hop=n_fft // 2, B=1, C=1, F=2))
        # k_ola<T> behind n_fft 15 (a synthesis window without zeros: hop >= win leaves no overlap to normalise)
        ola += [icase('ola hop 20', ty, 15, hop=20, fmts=(CF, CL)), icase('ola hop 15', ty, 15, hop=15),
                icase('ola hop 4', ty, 15, hop=4, F=7, fmts=(CL, CL)), icase('ola F1', ty, 15, hop=4, F=1, fmts=(CL, CF)),
                icase('ola stride', ty, 15, hop=4, B=1, C=1, F=263000, stride=True, short=dict(F=9))]
    return inv, ola


ISTFT_CASES, OLA_CASES = _istft_cases()


def istft_branches(c):
    p = c['ty'] + '.'
    n_fft, win, hop, f_ = c['n_fft'], c['win'], c['hop'], c['F']
    br = plan_branches(c['ty'], n_fft, c['B'] * c['C'] * f_, False)
    m = pg.gen_fft_len(n_fft)
    br.add(p + ('inv.M<=1024' if m <= SPEC_UNROLL * THREADS else 'inv.M>1024'))
    if m % THREADS:
        br.add(p + 'inv.M%256')
    if win < n_fft:
        br.add(p + 'inv.win<n_fft')
    if win > n_fft:
        br.add(p + 'inv.win>n_fft')
    br.add(p + 'inv.dcnyq.imag')                                           # istft_input: every bin has an imaginary part
    if hop > win:
        br.add(p + 'ola.hop>win')
    if hop == win:
        br.add(p + 'ola.hop==win')
    if hop < win and win % hop:
        br.add(p + 'ola.win%hop')
    if f_ == 1:
        br.add(p + 'ola.F1')
    if c['wave_fmt'] == CL and c['C'] > 1:
        br.add(p + 'ola.cl')
    if c['B'] * c['C'] * ((f_ - 1) * hop + win) > GRID_1D_CAP * THREADS:
        br.add(p + 'ola.stride')
    return br


def synth_window(c):
    """a synthesis window without zeros, exact in the element type"""
    return (0.5 + 0.5 * hann(c['win'], 'f64') + 0.01 * np.arange(c['win']) / c['win']).astype(DT[c['ty']])


def istft_input(c):
    """logical (B, C, F, K) complex Gaussian bins (DC and Nyquist included: their imaginary parts must be ignored)"""
    rng = np.random.default_rng(seed_of(c))
    shape = (c['B'], c['C'], c['F'], c['n_fft'] // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(CDT[c['ty']])


def emulate_irfft(c, spec, synth, mutant=None):
    """k_irfft_gen on `spec` (the memory image of c['spec_fmt']): the [total_frames][win] workspace"""
    ty, t = c['ty'], DT[c['ty']]
    n, b_, c_, f_, win = c['n_fft'], c['B'], c['C'], c['F'], c['win']
    k_ = n // 2 + 1
    pl = gen_fits(ty, n)
    m, packed = pl['m'], pl['packed']
    tws = 2 if packed and mutant != 'tws1' else 1
    tw = twiddles(ty, n)
    _, _, _, base, st = frame_index(b_, c_, f_, False, c['spec_fmt'] == CL and c_ > 1, 0, k_)
    sf = np.asarray(spec, CDT[ty]).ravel()
    sre, sim = sf.real.astype(t), sf.imag.astype(t)

    def bins(kk):
        addr = base[:, None] + kk[None, :] * st
        _check(addr, sf.size)
        return sre[addr], sim[addr]

    k = np.arange(m)
    if packed:
        half = t(0.5)
        xk, xm = bins(k), bins(m - k)
        if mutant != 'dcnyq_imag':
            xk = (xk[0], np.where(k == 0, t(0), xk[1]))
            xm = (xm[0], np.where(k == 0, t(0), xm[1]))
        w = _ld(tw, k)
        e = (half * (xk[0] + xm[0]), half * (xk[1] - xm[1]))
        d = (half * (xk[0] - xm[0]), half * (xk[1] + xm[1]))
        xo = _mul(d, (w[0], w[1] if mutant == 'inv_conj' else -w[1]))
        a = (e[0] - xo[1], e[1] + xo[0])
    else:
        kk = np.where(k < k_, k, n - k)
        vr, vi = bins(kk)
        vi = np.where(k >= k_, -vi, vi)
        if mutant != 'dcnyq_imag':
            vi = np.where((kk == 0) | (2 * kk == n), t(0), vi)
        a = (vr, vi)
    r = gen_fft(a, pl['radix'], tw, tws, +1, t, mutant)
    inv_m = t(1.0 / float(n if mutant == 'inv_m' else m))
    rr = np.stack([r[0], r[1]], -1).reshape(r[0].shape[0], -1) if packed else r[0]      # packed: (x[2m], x[2m+1]) interleaved
    nn = np.arange(win)
    if mutant == 'zero_tail':
        vals = rr[:, np.minimum(nn, n - 1)]
    else:
        _check(nn[nn < n], rr.shape[-1])
        vals = np.where((nn < n)[None, :], rr[:, np.minimum(nn, n - 1)], t(0))
    return vals * inv_m * np.asarray(synth, t)[None, :]


def emulate_ola(c, frames, mutant=None):
    """k_ola<T> on the workspace: the waveform's memory image"""
    t = DT[c['ty']]
    b_, c_, f_, win, hop = c['B'], c['C'], c['F'], c['win'], c['hop']
    t_out = (f_ - 1) * hop + win
    flat = np.asarray(frames, t).ravel()
    i = np.arange(b_ * c_ * t_out)
    bc = i // t_out
    tt = i - bc * t_out
    f_hi = np.minimum(tt // hop, f_ - 1)
    f_lo = (tt - win) // hop if mutant == 'f_lo' else (tt - win + hop) // hop
    f_lo = np.where(tt - win + 1 <= 0, 0, f_lo)
    acc = np.zeros(i.size, t)
    for j in range(int((f_hi - f_lo).max()) + 1):
        f = f_lo + j
        on = f <= f_hi
        addr = ((bc * f_ + f) * win + (tt - f * hop))[on]
        _check(addr, flat.size)
        acc[on] = acc[on] + flat[addr]
    out = np.full(i.size, np.nan, t)
    if c['wave_fmt'] == CL and c_ > 1:
        b = bc // c_
        out[(b * t_out + tt) * c_ + (bc - b * c_)] = acc
    else:
        out[i] = acc
    return out.reshape(shape_of(c['wave_fmt'], b_, c_, t_out))


def emulate_istft(c, spec, synth, mutant=None):
    return emulate_ola(c, emulate_irfft(c, spec, synth, mutant), mutant)


def ref_istft(c, spec_bcfk, synth):
    """longdouble reference (tf.signal.inverse_stft as tests/test_f64.py restates it): (waveform (B, C, t_out), its bound)"""
    n, win, hop, f_ = c['n_fft'], c['win'], c['hop'], c['F']
    spec = np.asarray(spec_bcfk).astype(np.clongdouble)
    synth = np.asarray(synth, LD)
    frames = np.fft.irfft(spec, n=n, axis=-1)[..., :win]
    mag = np.abs(spec)
    edge = [0] + ([n // 2] if n % 2 == 0 else [])
    mag[..., edge] = np.abs(spec[..., edge].real)
    herm = 2 * mag.sum(-1, keepdims=True) - mag[..., edge].sum(-1, keepdims=True)
    if win > n:
        frames = np.pad(frames, [(0, 0)] * 3 + [(0, win - n)])
    frames = frames * synth
    s = herm / n * np.abs(synth) * (np.arange(win) < n)                    # (B, C, F, win)
    pl = gen_fits(c['ty'], n)
    cc = 2 * (fft_const(pl['radix']) + 4) + 3 if pl['packed'] else fft_const(pl['radix']) + 3
    u = UNIT[c['ty']]
    b_, c_ = spec.shape[:2]
    t_out = (f_ - 1) * hop + win
    out, bound, terms, count = (np.zeros((b_, c_, t_out), LD) for _ in range(4))
    for i in range(f_):
        sl = slice(i * hop, i * hop + win)
        out[..., sl] += frames[:, :, i]
        bound[..., sl] += u * cc * s[:, :, i]
        terms[..., sl] += np.abs(frames[:, :, i])
        count[..., sl] += 1
    bound += np.maximum(count - 1, 0) * u * terms
    return out, bound.astype(np.float64)


# =================================================================================================================
# k_filterbank_f64
# =================================================================================================================
def bcase(id, fmt, B, C, F, n_freq, n_filt, **kw):
    return dict(id=id, fmt=fmt, B=B, C=C, F=F, n_freq=n_freq, n_filt=n_filt, **kw)


FB64_CASES = [
    bcase('cf 2x3x5 9->4', CF, 2, 3, 5, 9, 4), bcase('cl 2x3x5 9->4', CL, 2, 3, 5, 9, 4), bcase('cl 2x1x5 9->4', CL, 2, 1, 5, 9, 4),
    # just over 4096 * 256 outputs: every thread takes a second one
    bcase('stride cl 3->7', CL, 1, 2, (GRID_1D_CAP * THREADS) // 14 + 5, 3, 7, stride=True, short=dict(F=11)),
]


def fb64_branches(c):
    br = {'fb64.cf' if c['fmt'] == CF else 'fb64.cl' if c['C'] > 1 else 'fb64.cl.C1'}
    if c['B'] * c['C'] * c['F'] * c['n_filt'] > GRID_1D_CAP * THREADS:
        br.add('fb64.stride')
    return br


def fb64_input(c):
    """(logical (B, C, F, n_freq) input, (n_freq, n_filt) matrix of float32 values: the layer keeps its filterbank in float32)"""
    rng = np.random.default_rng(seed_of(c))
    return rng.standard_normal((c['B'], c['C'], c['F'], c['n_freq'])), rng.standard_normal((c['n_freq'], c['n_filt'])).astype(np.float32)


def emulate_fb64(c, x, fb):
    """k_filterbank_f64 on the memory image x: one thread per output, the bins added in ascending order"""
    b_, c_, f_, n_freq, n_filt = c['B'], c['C'], c['F'], c['n_freq'], c['n_filt']
    xf, fbf = np.asarray(x, np.float64).ravel(), np.asarray(fb, np.float64).ravel()
    i = np.arange(b_ * c_ * f_ * n_filt)
    mm, row = i % n_filt, i // n_filt
    f, bc = row % f_, row // f_
    b = bc // c_
    ch = bc - b * c_
    if c['fmt'] == CL and c_ > 1:
        xin, xo, es = ((b * f_ + f) * n_freq) * c_ + ch, ((b * f_ + f) * n_filt + mm) * c_ + ch, c_
    else:
        xin, xo, es = row * n_freq, row * n_filt + mm, 1
    acc = np.zeros(i.size)
    for k in range(n_freq):
        _check(xin + k * es, xf.size)
        acc = acc + xf[xin + k * es] * fbf[k * n_filt + mm]
    out = np.full(i.size, np.nan)
    out[xo] = acc
    return out.reshape(shape_of(c['fmt'], b_, c_, f_, n_filt))


def ref_fb64(c, x_bcfk, fb):
    """(longdouble product (B, C, F, n_filt), its bound)"""
    x, fb = np.asarray(x_bcfk, LD), np.asarray(fb, LD)
    return x @ fb, (c['n_freq'] * UNIT['f64'] * (np.abs(x) @ np.abs(fb))).astype(np.float64)


# =================================================================================================================
# mutants: one wrong line each
# =================================================================================================================
MUTANTS = {
    # name: (what it breaks, the emulations it applies to)
    'idx_mod': ('gen_output: `if (idx >= N) idx -= N` dropped', ('stft', 'istft')),
    'mask_r': ('gen_output: the `r0 + u < R` mask dropped', ('stft', 'istft')),
    'clamp_R': ('gen_output: min(r0 + u, R - 1) -> min(r0 + u, R)', ('stft', 'istft')),
    'store_mask': ('gen_pass: the `o0 + u * 256 < N` store mask dropped', ('stft', 'istft')),
    'tws1': ('packed sizes: twiddle stride 2 -> 1', ('stft', 'istft')),
    'k_eq_M': ('k_stft_gen: bin k == M reads r[M] instead of r[0]', ('stft',)),
    'win_mask': ('k_stft_gen: the `n < win` mask dropped', ('stft',)),
    'inv_conj': ('k_irfft_gen: the pre-pairing twiddle not conjugated', ('istft',)),
    'dcnyq_imag': ('k_irfft_gen: the imaginary parts of DC and Nyquist kept', ('istft',)),
    'inv_m': ('k_irfft_gen: inv_m = 1 / n_fft for packed sizes', ('istft',)),
    'zero_tail': ('k_irfft_gen: no zero tail for n >= n_fft', ('istft',)),
    'f_lo': ('k_ola: f_lo = (t - win) / hop', ('istft',)),
}
# float32 calls with win > n_fft take the DFT-as-GEMM path, so k_irfft_gen<float> never has a tail to zero
F64_ONLY_MUTANTS = ('zero_tail',)
