"""A checker for the forward kernels of kapre_amd/csrc/kpr_signal_kernels.h (k_frame, k_energy, k_delta, k_thin_gemm) that needs
no GPU and does not import the package.  Three parts, shared by tests/test_signal_model_host.py (CPU) and tests/test_signal_gate.py
(GPU):

  branch model   the predicates of the host dispatch (frame_args, the `vec` tests, part_words, thin_gemm_shape, the grids) and of
                 the kernels (the streaming condition of k_energy, the wave-uniform interior test of k_delta ...) restated in
                 numpy: *_branches(case) returns the ids of BRANCHES a case reaches.  The alignment of the input's base pointer
                 is an input (case['misaligned']: the tensor starts one float past a 16-byte boundary); outputs are fresh
                 allocations and always aligned.
  case tables    FRAME_CASES, ENERGY_CASES, DELTA_CASES, THIN_CASES: the smallest shape at which each branch exists
  emulations     emulate_*(case, ...): float64, index by index in the kernel's own decomposition (hop blocks with full[] / pre[],
                 delta_src_index, row / element -> source index, 16-row blocks of k-groups), NOT the oracle's formulation.  Each takes a
                 named mutant = one wrong line; a mutant that no table case tells from the oracle means the table is too weak.

The 64-bit index branch of k_frame (frame.index64: 2^31 or more output vectors, at least 8.6 GB of output) is in BRANCHES so that
the gap stays visible, and in EXCLUDED: no case reaches it.
"""
import zlib

import numpy as np

CL, CF = 'channels_last', 'channels_first'
U32 = 2.0 ** -24

# ---- constants of the source, restated (tests/test_signal_model_host.py compares them with the source text) ----------------
EN_FRAMES = 64                    # kEnFrames: frames per k_energy workgroup
EN_UNROLL = 12 * 256              # float4s one pass of k_energy's streaming loop takes
BLOCK = 256
GRID_CAP = 1 << 16                # grid_1d cap of k_frame / k_delta, workgroup cap of k_energy
THIN_GRID_CAP = 256 * 8           # workgroups of k_thin_gemm, 64 rows each per pass
THIN_MAX_TILES = 4                # thin_gemm_shape: (n_filt + 15) / 16 <= 4
THIN_MAX_K = 512                  # thin_gemm_shape: n_freq <= 512
LDS_PLAIN = 64 * 1024             # dynamic LDS a launch gets without hipFuncSetAttribute
THIN_BIG_LDS_OPT_IN = True        # kpr_apply_filterbank_f32 launches k_thin_gemm through allow_big_lds above LDS_PLAIN

BRANCHES = (
    'frame.empty', 'frame.vec4', 'frame.vec1', 'frame.cl', 'frame.T<L', 'frame.pad', 'frame.gridstride', 'frame.index64',
    'frame.vec4.load16', 'frame.vec4.dwordload', 'frame.vec4.mixed', 'frame.vec4.straddle',
    'energy.refused', 'energy.cl', 'energy.chunks>=2', 'energy.chunk.partial', 'energy.wgstride',
    'energy.stream', 'energy.stream.passes>=2', 'energy.stream.passes>=3', 'energy.stream.padend', 'energy.stream.ragged',
    'energy.stream.r0', 'energy.stream.r>0',
    'energy.general', 'energy.general.q0', 'energy.general.r0', 'energy.general.r>0', 'energy.general.pad',
    'energy.general.hop%4', 'energy.general.nolds', 'energy.general.es>1', 'energy.general.r%4', 'energy.general.T%4',
    'energy.general.pastend', 'energy.general.misaligned',
    'delta.vec4', 'delta.vec1', 'delta.vec1.misaligned', 'delta.cl', 'delta.interior', 'delta.interior.j0>4',
    'delta.interior.clamp', 'delta.edge', 'delta.mixedwave', 'delta.pad.constant', 'delta.pad.symmetric', 'delta.pad.reflect',
    'delta.pad.wrap', 'delta.T1', 'delta.gridstride',
    'thin.nt1', 'thin.nt2', 'thin.nt3', 'thin.nt4', 'thin.k%16', 'thin.n%16', 'thin.rows%16', 'thin.idlewaves', 'thin.lds=64K',
    'thin.lds>64K', 'thin.rowstride',
    'gemm.k%4', 'gemm.k>512', 'gemm.n>64', 'gemm.cl', 'gemm.misaligned',
)
EXCLUDED = ('frame.index64',)


def seed_of(case, salt=0):
    return zlib.crc32(case['id'].encode()) + salt


def x_offset(case):
    """floats between a 16-byte boundary and the first element of the input"""
    return 1 if case.get('misaligned') else 0


def shape_of(fmt, b, c, *inner):
    return (b, *inner, c) if fmt == CL else (b, c, *inner)


def shortened(case):
    """the stride cases with their size cut down (same geometry otherwise): what the CPU tests run instead"""
    return dict(case, **case['short'], stride=False) if case.get('stride') else case


# =================================================================================================================
# Frame
# =================================================================================================================
def frame_count(T, L, hop, pad_end):
    """kpr_frame_count"""
    if pad_end:
        return -(-T // hop)
    return 0 if T < L else 1 + (T - L) // hop


def fcase(id, L, hop, T, C=1, fmt=CF, batch=2, pad_end=False, pad_value=0.0, **kw):
    return dict(id=id, L=L, hop=hop, T=T, C=C, fmt=fmt, batch=batch, pad_end=pad_end, pad_value=pad_value, **kw)


N_STRIDE = GRID_CAP * BLOCK           # elements one pass of a capped grid covers

FRAME_CASES = [
    fcase('8/4/64', 8, 4, 64),                                              # every float4 aligned: 16-byte loads only
    fcase('8/3/64', 8, 3, 64),                                              # hop 3: every fourth frame aligned, the rest dwords
    fcase('7/3/50', 7, 3, 50),                                              # odd row: VEC 1
    fcase('8/8/64', 8, 8, 64),                                              # no overlap
    fcase('cl2 6/5/50', 6, 5, 50, C=2, fmt=CL),                             # rows of 12 floats across both channels
    fcase('cl3 5/2/33', 5, 2, 33, C=3, fmt=CL),                             # rows of 15: VEC 1
    fcase('cl2 6/5/23 pad', 6, 5, 23, C=2, fmt=CL, pad_end=True, pad_value=1.5),
    fcase('8/4/21 pad', 8, 4, 21, pad_end=True, pad_value=-3.0),            # a float4 with one sample left of the signal
    fcase('8/4/5 pad T<L', 8, 4, 5, pad_end=True, pad_value=2.0),
    fcase('8/4/5 T<L', 8, 4, 5),                                            # no frame: nothing is launched
    fcase('8/4/64 cl1', 8, 4, 64, C=1, fmt=CL),                             # channels_last with one channel: the plain geometry
    fcase('8/4/64 misaligned', 8, 4, 64, misaligned=True),
    # odd row length, just over 65536 * 256 output elements: every thread takes a second element
    fcase('stride 7/3', 7, 3, 3 * (N_STRIDE // 7 + 40) + 7, batch=1, stride=True, short=dict(T=100)),
]


def frame_geometry(case):
    L, hop, T, C = case['L'], case['hop'], case['T'], case['C']
    F = frame_count(T, L, hop, case['pad_end'])
    cl = case['fmt'] == CL and C > 1                                        # frame_args
    rowlen = L * C if cl else L
    nbq = case['batch'] if cl else case['batch'] * C
    vec = rowlen % 4 == 0                                                   # the output is a fresh allocation: aligned
    per_row = rowlen // 4 if vec else rowlen
    return dict(F=F, cl=cl, rowlen=rowlen, nbq=nbq, nrows=nbq * F, vec=vec, per_row=per_row, total=nbq * F * per_row,
                cm=C if cl else 1)


def frame_branches(case):
    g = frame_geometry(case)
    L, hop, T = case['L'], case['hop'], case['T']
    if g['nrows'] == 0:
        return {'frame.empty'}
    br = {'frame.vec4' if g['vec'] else 'frame.vec1'}
    if g['cl']:
        br.add('frame.cl')
    if T < L:
        br.add('frame.T<L')
    if g['total'] > GRID_CAP * BLOCK:
        br.add('frame.gridstride')
    if g['total'] >= 2 ** 31:
        br.add('frame.index64')
    if (T - (g['F'] - 1) * hop) * g['cm'] < g['rowlen']:
        br.add('frame.pad')
    if g['vec']:
        f = np.arange(g['F'])[None, :, None]
        i = np.arange(0, g['rowlen'], 4)[None, None, :]
        bq = np.arange(min(g['nbq'], 4))[:, None, None]
        off = (bq * T + f * hop) * g['cm'] + i + x_offset(case)
        avail = (T - f * hop) * g['cm']
        fits = (i + 3 < avail) & (off >= 0)
        load16 = fits & (off % 4 == 0)
        if load16.any():
            br.add('frame.vec4.load16')
        if (~load16).any():
            br.add('frame.vec4.dwordload')
        if load16.any() and (fits & ~load16).any():
            br.add('frame.vec4.mixed')
        if ((i < avail) & (i + 3 >= avail)).any():
            br.add('frame.vec4.straddle')
    return br


def frame_label(case):
    return '' if frame_geometry(case)['nrows'] == 0 else 'k_frame'


def frame_input(case, dtype=np.float32):
    rng = np.random.default_rng(seed_of(case))
    return rng.uniform(-1, 1, shape_of(case['fmt'], case['batch'], case['C'], case['T'])).astype(dtype)


def emulate_frame(case, x, mutant=None):
    """row = one frame of one batch item (channels_last, C > 1: L * C contiguous floats) or of one signal; element i of the row comes
    from src[i] while i < avail, else it is pad_value"""
    g = frame_geometry(case)
    T, hop = case['T'], case['hop']
    flat = np.asarray(x).reshape(-1)
    rows = np.arange(g['nrows'])
    bq, f = rows // max(g['F'], 1), rows % max(g['F'], 1)
    t0 = f * hop
    base = (bq * T + t0) * g['cm']
    avail = (T - t0) if mutant == 'avail_without_C' else (T - t0) * g['cm']
    i = np.arange(g['rowlen'])[None, :]
    idx = base[:, None] + i
    ok = i < avail[:, None]
    out = np.where(ok, flat[np.clip(idx, 0, max(flat.size - 1, 0))] if flat.size else 0.0, flat.dtype.type(case['pad_value']))
    return out.reshape(shape_of(case['fmt'], case['batch'], case['C'], g['F'], case['L']))


FRAME_MUTANTS = ('avail_without_C',)


# =================================================================================================================
# Energy
# =================================================================================================================
def ecase(id, L, hop, T=None, frames=None, **kw):
    if T is None:
        T = (frames - 1) * hop + L
    c = fcase(id, L, hop, T, **kw)
    c.setdefault('sample_rate', 22050)
    c.setdefault('ref_duration', 0.1)
    return c


ENERGY_CASES = [
    # general path
    ecase('10/3/50', 10, 3, 50),                                            # hop % 4; q = 3, r = 1
    ecase('5/8/50', 5, 8, 50),                                              # q = 0: a frame shorter than the hop
    ecase('8/4/50', 8, 4, 50),                                              # T % 4; r = 0
    ecase('10/8/64', 10, 8, 64),                                            # r % 4
    ecase('10/3 70f', 10, 3, frames=70),                                    # two chunks on the general path
    ecase('8/4/64 pad', 8, 4, 64, pad_end=True, pad_value=3.0),             # the last frame reaches past the end
    ecase('8/4/62 pad', 8, 4, 62, pad_end=True, pad_value=0.5),
    ecase('1024/1024/8f', 1024, 1024, frames=8, batch=1),                   # 66 * 256 partial sums do not fit 64 KiB
    ecase('8/4/64 cl2', 8, 4, 64, C=2, fmt=CL),                             # element stride 2
    ecase('8/4/64 misaligned', 8, 4, 64, misaligned=True),
    # streaming path
    ecase('8/4/64', 8, 4, 64),
    ecase('12/8/128', 12, 8, 128),                                          # r = 4
    ecase('256/256/70f', 256, 256, frames=70, batch=1),                     # 65 * 64 float4s: two passes; two chunks
    ecase('2048/512/70f', 2048, 512, frames=70, batch=1),                   # 68 * 128 float4s: three passes; ragged chunk 2
    ecase('8/8/64 pad', 8, 8, 64, pad_end=True, pad_value=2.0),             # pad_end with nothing to pad
    ecase('8/4/64 cl1', 8, 4, 64, C=1, fmt=CL),
    ecase('8/4/64 cf3', 8, 4, 64, C=3, fmt=CF),
    ecase('8/4 64f', 8, 4, frames=64),
    ecase('8/4 65f', 8, 4, frames=65),
    ecase('8/4 129f', 8, 4, frames=129),
    # 65 537 signals of 16 samples: workgroup 0 takes a second signal
    ecase('stride 8/4/16', 8, 4, 16, batch=GRID_CAP + 1, stride=True, short=dict(batch=5)),
]
ENERGY_REFUSED = ecase('20000/1', 20000, 1, 20010, batch=1)                 # 2 * (64 + 20001) floats of LDS: the library refuses


def energy_scale(case):
    return case['ref_duration'] / (case['L'] / case['sample_rate'])


def energy_plan(case):
    L, hop, T, C = case['L'], case['hop'], case['T'], case['C']
    F = frame_count(T, L, hop, case['pad_end'])
    q = L // hop
    r = L - q * hop
    nblk = EN_FRAMES + q + (1 if r else 0)
    lds = 4 * 2 * (EN_FRAMES + q + 1)
    part_words = 0
    if hop % 4 == 0:
        pw = (EN_FRAMES + q + 1) * (hop // 4)
        if lds + 4 * pw <= LDS_PLAIN:
            part_words = pw
    cl = case['fmt'] == CL                                                  # kpr_energy_f32 overrides frame_args' cl
    es = C if cl else 1
    why = []
    if hop % 4:
        why.append('hop%4')
    elif not part_words:
        why.append('nolds')
    if es != 1:
        why.append('es>1')
    if r % 4:
        why.append('r%4')
    if T % 4:
        why.append('T%4')
    if (F - 1) * hop + L > T:
        why.append('pastend')
    if not why and x_offset(case) % 4:                                      # src + t_lo is as aligned as x once hop, T are multiples of 4
        why.append('misaligned')
    return dict(F=F, q=q, r=r, nblk=nblk, chunks=-(-F // EN_FRAMES), refused=lds > LDS_PLAIN, part_words=part_words, cl=cl,
                es=es, why=why, stream=not why, n4=nblk * (hop // 4), n_sig=case['batch'] * C)


def energy_branches(case):
    p = energy_plan(case)
    if p['refused']:
        return {'energy.refused'}
    br = set()
    if p['cl']:
        br.add('energy.cl')
    if p['chunks'] >= 2:
        br.add('energy.chunks>=2')
    if p['F'] % EN_FRAMES:
        br.add('energy.chunk.partial')
    if p['n_sig'] * p['chunks'] > GRID_CAP:
        br.add('energy.wgstride')
    T, hop = case['T'], case['hop']
    last_t_lo = (p['chunks'] - 1) * EN_FRAMES * hop
    if p['stream']:
        br.add('energy.stream')
        passes = -(-p['n4'] // EN_UNROLL)
        if passes >= 2:
            br.add('energy.stream.passes>=2')
        if passes >= 3:
            br.add('energy.stream.passes>=3')
        if case['pad_end']:
            br.add('energy.stream.padend')
        if (T - last_t_lo) // 4 < p['n4']:
            br.add('energy.stream.ragged')
        br.add('energy.stream.r>0' if p['r'] else 'energy.stream.r0')
    else:
        br.add('energy.general')
        br.update('energy.general.' + w for w in p['why'])
        if p['q'] == 0:
            br.add('energy.general.q0')
        br.add('energy.general.r>0' if p['r'] else 'energy.general.r0')
        if (p['F'] - 1) * hop + case['L'] > T:
            br.add('energy.general.pad')
    return br


def energy_signals(case, x):
    """(n_sig, T): signal b * C + c"""
    b, C, T = case['batch'], case['C'], case['T']
    x = np.asarray(x, np.float64)
    if case['fmt'] == CL:
        x = x.reshape(b, T, C).transpose(0, 2, 1)
    return x.reshape(b * C, T)


def emulate_energy(case, x, mutant=None, internals=None):
    """per workgroup (64 frames of one signal): full[i] = sum of squares of hop block f0 + i, pre[i] = of its first r samples;
    output f = scale * (full[f] + ... + full[f + q - 1] + (r ? pre[f + q] : 0)).  Streaming path: samples past the end count
    as 0 (their partial sums are zeroed); general path: as pad_value.  internals: a list that receives every chunk's full[]."""
    p = energy_plan(case)
    T, hop, q, r, nblk, F = case['T'], case['hop'], p['q'], p['r'], p['nblk'], p['F']
    xs = energy_signals(case, x)
    out = np.zeros((p['n_sig'], F))
    for chunk in range(p['chunks']):
        f0 = chunk * EN_FRAMES
        fb = f0 + (1 if mutant == 'seam_off_by_one' and chunk > 0 else 0)
        t = (fb + np.arange(nblk))[:, None] * hop + np.arange(hop)[None, :]
        w = xs[:, np.minimum(t, T - 1)]                                     # (n_sig, nblk, hop)
        if p['stream']:
            if mutant == 'stale_partials':                                  # the clamped load p4[n4v - 1] is squared, not zeroed
                t_lo = fb * hop
                n4v = min(p['n4'], (T - t_lo) >> 2)
                past = xs[:, t_lo + 4 * (n4v - 1) + (t - t_lo) % 4]
            else:
                past = 0.0
        else:
            past = case['pad_value']
        w = np.where((t < T)[None], w, past)
        sq = w * w
        full, pre = sq.sum(-1), sq[..., :r].sum(-1)
        if internals is not None:
            internals.append(full)
        nf = min(EN_FRAMES, F - f0)
        acc = np.zeros((p['n_sig'], nf))
        for k in range(q):
            acc += full[:, k:k + nf]
        if r and mutant != 'r_as_zero':
            at = max(q - 1, 0) if mutant == 'pre_at_q_minus_1' else q
            acc += pre[:, at:at + nf]
        out[:, f0:f0 + nf] = energy_scale(case) * acc
    out = out.reshape(case['batch'], case['C'], F)
    return out.transpose(0, 2, 1) if case['fmt'] == CL else out


# 'stale_partials' is an equivalent mutant as far as outputs go: the streaming path is only taken when no frame reaches past the
# signal, so no output reads a partial sum beyond n4v.  The host test asserts exactly that (full[] differs, no output does).
ENERGY_MUTANTS = ('pre_at_q_minus_1', 'r_as_zero', 'seam_off_by_one')
ENERGY_EQUIVALENT_MUTANTS = ('stale_partials',)


def energy_bound(case, want):
    """|got - want| per element: every output is scale * a sum of L non-negative squares; each square, the scale and the product
    round once and the additions L - 1 times in any order: (L + 8) * 2^-24 * want to first order"""
    return (case['L'] + 8) * U32 * np.abs(want)


def energy_exact_input(case):
    """integers in [-15, 15]: every square, partial sum and total is an integer (pad_value 0.5: a multiple of 1/4) below 2^24"""
    rng = np.random.default_rng(seed_of(case, 1))
    return rng.integers(-15, 16, shape_of(case['fmt'], case['batch'], case['C'], case['T'])).astype(np.float32)


def energy_exact_magnitude(case):
    """largest intermediate, in units of the spacing 1/4 of the values"""
    return 4 * case['L'] * max(15.0, abs(case['pad_value'])) ** 2


def energy_exact_expected(case, x):
    fr = frame_windows(energy_signals(case, x), case)
    s = (fr * fr).sum(-1)                                                   # exact in float64
    out = (np.float32(energy_scale(case)) * s.astype(np.float32)).astype(np.float32)
    out = out.reshape(case['batch'], case['C'], -1)
    return out.transpose(0, 2, 1) if case['fmt'] == CL else out


def frame_windows(xs, case):
    """(n_sig, T) -> (n_sig, F, L) with pad_value past the end: the definition, for the expected values of the exact inputs"""
    T, L, hop = case['T'], case['L'], case['hop']
    F = frame_count(T, L, hop, case['pad_end'])
    idx = np.arange(F)[:, None] * hop + np.arange(L)[None, :]
    return np.where((idx < T)[None], xs[:, np.minimum(idx, T - 1)], case['pad_value'])


# =================================================================================================================
# Delta
# =================================================================================================================
MODES = ('symmetric', 'reflect', 'constant')


def dcase(id, win, mode, T, f, C=1, fmt=CF, batch=2, **kw):
    return dict(id=id, win=win, mode=mode, T=T, f=f, C=C, fmt=fmt, batch=batch, **kw)


def _delta_cases():
    cases = []
    for win in (3, 5, 9, 11, 101):
        n = (win - 1) // 2
        for mode in MODES:
            for T in sorted({1, 2, n, 2 * n, 2 * n + 1, 200}):
                for f in (1, 13, 256):                                      # 1, 13: waves span rows and items; 256: uniform waves
                    cases.append(dcase('w%d %s T%d f%d' % (win, mode, T, f), win, mode, T, f, group='w%d %s' % (win, mode)))
    for mode in MODES:
        cases.append(dcase('w9 %s cl3' % mode, 9, mode, 23, 8, C=3, fmt=CL, group='layouts'))       # inner 24: VEC 4
        cases.append(dcase('w9 %s cl3 odd' % mode, 9, mode, 23, 5, C=3, fmt=CL, group='layouts'))   # inner 15: VEC 1
        cases.append(dcase('w5 %s misaligned' % mode, 5, mode, 23, 8, misaligned=True, group='layouts'))
        # inner 13, just over 65536 * 256 elements
        cases.append(dcase('stride w5 %s' % mode, 5, mode, N_STRIDE // 13 + 40, 13, batch=1, stride=True, short=dict(T=300),
                           group='stride'))
    return cases


DELTA_CASES = _delta_cases()


def delta_geometry(case):
    b, C, T, f = case['batch'], case['C'], case['T'], case['f']
    cl = case['fmt'] == CL
    outer, inner = (b, f * C) if cl else (b * C, f)
    n = (case['win'] - 1) // 2
    vec = inner % 4 == 0 and x_offset(case) % 4 == 0
    per_row = inner // 4 if vec else inner
    return dict(outer=outer, inner=inner, n=n, vec=vec, V=4 if vec else 1, per_row=per_row, total=outer * T * per_row, cl=cl,
                denom=2 * sum(i * i for i in range(1, n + 1)), shape=shape_of(case['fmt'], b, C, T, f))


def delta_wave_paths(case, limit=None):
    """per element (thread-loop index e): is its wave on the interior path?  A wave = 64 consecutive e (the grid stride is a multiple
    of 64); lanes past `total` are inactive and do not vote.  Returns (interior per element, path per element)."""
    g = delta_geometry(case)
    total = g['total'] if limit is None else min(g['total'], limit)
    e = np.arange(total)
    t = (e // g['per_row']) % case['T']
    interior = (t - g['n'] >= 0) & (t + g['n'] < case['T'])
    padded = np.ones(-(-total // 64) * 64, bool)
    padded[:total] = interior
    path = np.repeat(padded.reshape(-1, 64).all(axis=1), 64)[:total]
    return interior, path


def delta_branches(case):
    g = delta_geometry(case)
    T, n, mode = case['T'], g['n'], case['mode']
    br = {'delta.vec4' if g['vec'] else 'delta.vec1', 'delta.pad.' + mode}  # t = 0 is never interior: the pad is always met
    if not g['vec'] and g['inner'] % 4 == 0:
        br.add('delta.vec1.misaligned')
    if g['cl'] and case['C'] > 1:
        br.add('delta.cl')
    if g['total'] > GRID_CAP * BLOCK:
        br.add('delta.gridstride')
    if T == 1:
        br.add('delta.T1')
    if (mode == 'symmetric' and n > T) or (mode == 'reflect' and n >= T > 1):
        br.add('delta.pad.wrap')
    interior, path = delta_wave_paths(case, limit=1 << 20)                  # a prefix: what it reaches, the whole launch reaches
    pad = -len(interior) % 64
    any_in = np.concatenate([interior, np.zeros(pad, bool)]).reshape(-1, 64).any(axis=1)
    all_in = np.concatenate([path, np.ones(pad, bool)]).reshape(-1, 64).all(axis=1)
    if all_in.any():
        br.add('delta.interior')
        if n > 4:
            br.add('delta.interior.j0>4')
        if n % 4:
            br.add('delta.interior.clamp')
    if (~any_in).any():
        br.add('delta.edge')
    if (any_in & ~all_in).any():
        br.add('delta.mixedwave')
    return br


def delta_src_index(t, T, mode, mutant=None):
    """the kernel's function of the same name, vectorised: row to read for position t, -1 = a zero"""
    t = np.asarray(t, np.int64)
    if mode == 'symmetric' and mutant == 'symmetric_as_reflect':
        mode = 'reflect'
    outside = (t < 0) | (t >= T)
    if mode == 'constant':
        v = np.full_like(t, -1)
    elif T == 1:
        v = np.zeros_like(t)
    elif mode == 'symmetric':
        p = 2 * T
        m = t % p
        v = np.where(m < T, m, p - 1 - m)
    else:
        p = 2 * T - 2
        m = t % p
        v = np.where(m < T, m, p - m)
    return np.where(outside, v, t)


def _delta_rows(X, idx):
    """X (outer, T, inner) at rows idx (T,), zero where idx < 0"""
    return np.where((idx >= 0)[None, :, None], X[:, np.maximum(idx, 0), :], 0.0)


def emulate_delta(case, x, mutant=None):
    g = delta_geometry(case)
    T, n, mode = case['T'], g['n'], case['mode']
    X = np.asarray(x, np.float64).reshape(g['outer'], T, g['inner'])
    t = np.arange(T)
    # the general path: pairs (+j, -j) through delta_src_index
    general = np.zeros_like(X)
    for j in range(1, n + 1):
        general += j * (_delta_rows(X, delta_src_index(t + j, T, mode, mutant)) - _delta_rows(X, delta_src_index(t - j, T, mode, mutant)))
    # the interior path: groups of four j, the loads clamped to n, the weights not
    inside = (t - n >= 0) & (t + n < T)
    fast = np.zeros_like(X)
    for j0 in range(1, n + 1, 4):
        for u in range(4):
            j = min(j0 + u, n)
            d = _delta_rows(X, np.where(inside, t + j, -1)) - _delta_rows(X, np.where(inside, t - j, -1))
            if mutant == 'clamped_weight':
                fast += j * d                                               # the clamped j as weight: no guard, duplicates added
            elif j0 + u <= n:
                fast += (j0 + u) * d
    _, path = delta_wave_paths(case)
    on_fast = np.repeat(path, g['V']).reshape(X.shape)
    return (np.where(on_fast, fast, general) * (1.0 / g['denom'])).reshape(g['shape'])


DELTA_MUTANTS = ('clamped_weight', 'symmetric_as_reflect')


def delta_bound(case, x):
    """(2n + 4) * 2^-24 * inv_denom * sum_j j (|x[t + j]| + |x[t - j]|) over the padded rows: 2n terms, each a difference and a
    product, added in a chain, one final product"""
    g = delta_geometry(case)
    T, n = case['T'], g['n']
    X = np.abs(np.asarray(x, np.float64)).reshape(g['outer'], T, g['inner'])
    t = np.arange(T)
    s = np.zeros_like(X)
    for j in range(1, n + 1):
        s += j * (_delta_rows(X, delta_src_index(t + j, T, case['mode'])) + _delta_rows(X, delta_src_index(t - j, T, case['mode'])))
    return ((2 * n + 4) * U32 / g['denom'] * s).reshape(g['shape'])


def delta_input(case, dtype=np.float32):
    return np.random.default_rng(seed_of(case)).uniform(-1, 1, delta_geometry(case)['shape']).astype(dtype)


def delta_exact_input(case):
    return np.random.default_rng(seed_of(case, 1)).integers(-63, 64, delta_geometry(case)['shape']).astype(np.float32)


def delta_exact_magnitude(case):
    n = (case['win'] - 1) // 2
    return 126 * n * (n + 1) // 2


def delta_exact_expected(case, x):
    g = delta_geometry(case)
    num = emulate_delta(case, x) * g['denom']                               # integers: exact in float64
    num = np.rint(num)
    return (num.astype(np.float32) * np.float32(1.0 / g['denom'])).astype(np.float32)


# =================================================================================================================
# Thin GEMM
# =================================================================================================================
def tcase(K, N, rows, C=1, fmt=CF, **kw):
    id = 'K%d N%d rows%d' % (K, N, rows) + (' cl C%d' % C if fmt == CL else '') + (' misaligned' if kw.get('misaligned') else '')
    return dict(id=id, K=K, N=N, rows=rows, C=C, fmt=fmt, **kw)


THIN_ROWS = (1, 15, 16, 17, 63, 64, 65, 4099)
THIN_ROWSTRIDE = THIN_GRID_CAP * 64 + 17
# (K, N): every K and every N of the lists below at least once, the tile counts 1 - 4 against K below / on / above 16 and the LDS
# boundary: (256, 64) is exactly 64 KiB, (272, 64), (512, 33) and (512, 64) are above
THIN_KN = [(4, 1), (4, 64), (12, 13), (12, 49), (16, 16), (16, 33), (20, 17), (20, 48), (40, 13), (40, 32), (40, 64), (128, 20),
           (128, 49), (256, 1), (256, 48), (256, 64), (272, 17), (272, 64), (512, 16), (512, 32), (512, 33), (512, 64)]
THIN_KS = (4, 12, 16, 20, 40, 128, 256, 272, 512)
THIN_NS = (1, 13, 16, 17, 32, 33, 48, 49, 64)
THIN_CASES = [tcase(K, N, rows) for K, N in THIN_KN for rows in THIN_ROWS] + [
    tcase(20, 17, THIN_ROWSTRIDE),                                          # 8194 row blocks for 8192 waves
    tcase(272, 64, THIN_ROWSTRIDE // 8),
    # not thin
    tcase(10, 13, 65), tcase(516, 16, 65), tcase(40, 65, 65), tcase(40, 13, 22, C=3, fmt=CL), tcase(40, 13, 65, misaligned=True),
    tcase(40, 13, 65, C=1, fmt=CL),                                         # channels_last with one channel is contiguous: thin
]


def thin_plan(case):
    K, N, rows = case['K'], case['N'], case['rows']
    ntiles = -(-N // 16)
    shape = ntiles <= THIN_MAX_TILES and K <= THIN_MAX_K and K % 4 == 0     # thin_gemm_shape
    contiguous = case['fmt'] == CF or case['C'] == 1
    lds = 4 * 4 * 64 * ntiles * (-(-K // 16))
    thin = shape and contiguous and x_offset(case) % 4 == 0 and (lds <= LDS_PLAIN or THIN_BIG_LDS_OPT_IN)
    return dict(thin=thin, ntiles=ntiles, lds=lds, grid=min(-(-rows // 64), THIN_GRID_CAP), nblk=-(-rows // 16),
                contiguous=contiguous)


def thin_branches(case):
    p = thin_plan(case)
    K, N, rows = case['K'], case['N'], case['rows']
    br = set()
    if not p['thin']:
        if K % 4:
            br.add('gemm.k%4')
        if K > THIN_MAX_K:
            br.add('gemm.k>512')
        if p['ntiles'] > THIN_MAX_TILES:
            br.add('gemm.n>64')
        if not p['contiguous']:
            br.add('gemm.cl')
        if x_offset(case) % 4:
            br.add('gemm.misaligned')
        return br
    br.add('thin.nt%d' % p['ntiles'])
    if K % 16:
        br.add('thin.k%16')
    if N % 16:
        br.add('thin.n%16')
    if rows % 16:
        br.add('thin.rows%16')
    if p['nblk'] < 4 * p['grid']:
        br.add('thin.idlewaves')
    if p['lds'] == LDS_PLAIN:
        br.add('thin.lds=64K')
    if p['lds'] > LDS_PLAIN:
        br.add('thin.lds>64K')
    if p['nblk'] > 4 * p['grid']:
        br.add('thin.rowstride')
    return br


def thin_label(case):
    return 'k_thin_gemm' if thin_plan(case)['thin'] else 'k_gemm'


def thin_exact_input(case):
    rng = np.random.default_rng(seed_of(case, 1))
    return (rng.integers(-7, 8, (case['rows'] * case['C'], case['K'])).astype(np.float32),
            rng.integers(-7, 8, (case['K'], case['N'])).astype(np.float32))


def thin_exact_magnitude(case):
    return 49 * case['K']


def emulate_thin(case, a, b, mutant=None):
    """blocks of 16 rows (rows past the end: clamped loads, no store), k-groups of 16 = four float4 lanes of which a lane loads
    only when k0 + 3 < K, B zero-filled to 16 J x 16 NT; unwritten outputs stay NaN"""
    p = thin_plan(case)
    K, N = case['K'], case['N']
    rows = a.shape[0]
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    rb = np.arange(-(-rows // 16))
    if mutant == 'first_grid_pass_only':
        rb = rb[rb < 4 * min(-(-rows // 64), THIN_GRID_CAP)]
    J = K // 16 if mutant == 'partial_kgroup_dropped' else -(-K // 16)
    row = (rb[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
    src = np.minimum(row, rows - 1)
    ap = np.zeros((row.size, 16 * J))
    for k0 in range(0, 16 * J, 4):
        if k0 + 3 < K:
            ap[:, k0:k0 + 4] = a[src, k0:k0 + 4]
    bp = np.zeros((16 * J, 16 * p['ntiles']))
    kk = min(K, 16 * J)
    bp[:kk, :N] = b[:kk]
    d = ap @ bp
    out = np.full((rows, N), np.nan)
    ok = row < rows
    out[row[ok]] = d[ok, :N]
    return out


THIN_MUTANTS = ('partial_kgroup_dropped', 'first_grid_pass_only')
