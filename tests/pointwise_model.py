"""A checker for the stand-alone pointwise layers -- Magnitude, Phase (k_cplx_to_real, k_cplx_to_real_f64) and MagnitudeToDecibel
(k_stats_init, k_db_log<1|4>, k_db_clamp<1|4>, k_db_f64) -- that needs no GPU and does not import the package.  Shared by
tests/test_pointwise_model_host.py (CPU) and tests/test_pointwise_gate.py (GPU):

  plan functions  the host code restated in numpy: db_chunks, the per-block range [g0, g1), db_split, VEC from the two base
                  alignments, the grid_1d cap; db_paths() says in closed form which loop of k_db_log / k_db_clamp touches each
                  element (scalar head, four-in-flight loop, remainder loop, scalar tail)
  emulations      emulate_db() and emulate_c2r(): every workgroup, thread (256 at a time, as an index vector) and loop of the
                  kernels reads and writes the elements the kernel's would; they keep the per-block statistics, the encoded
                  per-item words, the clamp decisions and a write count per element.  Each takes a named mutant = one wrong line.
  expectations    to_db_bound (derived below), fma32 / mag_fma (float32 fused multiply-add emulated exactly), db_checks() -- the
                  assertions of the GPU test as a function of (input, run (a), run (b)), so that the CPU test can apply the very
                  same checks to the emulation and to its mutants
  case tables     DB_CASES, C2R_SIZES, DB_F64_SIZES: the smallest shapes at which each branch exists

MUTANTS are told from the unmutated emulation by db_checks / the write-coverage check on at least one table case.
EQUIVALENT_MUTANTS are wrong lines that change no output and no statistics word -- no test of outputs can see them; the CPU test
proves that (identical outputs, different access counts), so that nobody mistakes their survival for a hole in the tables:
  log.guard_removed      an empty block would issue atomicMax(enc(-inf)) / atomicMin(enc(+inf)); every finite decibel value
                         encodes above / below those, and every item has a non-empty block
  log.inflight_stride3   i += 3 * blockDim after four loads: the fourth vector is processed twice by the same block
  clamp.forced_chunks    db_clamp taking the forced option for BOTH its grid and its argument: another exact cover of the item
  c2r.step_blockdim      i += blockDim.x: every thread walks on through everything behind its first element
"""
import zlib

import numpy as np

U32 = 2.0 ** -24
BLOCK = 256
DB_TARGET_BLOCKS = 2048           # db_chunks: want = ceil(2048 / n_items)
DB_MAX_CHUNKS = 256
DB_MIN_CHUNK = 4096               # floats per chunk at least
GRID_CAP = 256 * 16               # grid_1d's default cap: k_cplx_to_real, k_stats_init
F64_BLOCK = 1024                  # k_db_f64: one workgroup per item
FLT_MIN = np.float32(1.17549435e-38)
C_DB = np.float32(3.01029995663981195)           # the literal in to_db: float32(10 log10 2)

HEAD, INFLIGHT, REMAINDER, TAIL, VECTOR = 0, 1, 2, 3, 4      # path codes (VECTOR: the one vector loop of k_db_clamp)

BRANCHES = (
    'db.chunks=1', 'db.chunks>=2', 'db.chunks.want1', 'db.chunks.cap256', 'db.chunks.forced', 'db.block.empty', 'db.block.short',
    'db.log.vec4', 'db.log.vec1', 'db.log.head', 'db.log.tail', 'db.log.middle.empty', 'db.log.inflight', 'db.log.inflight.partial',
    'db.log.remainder', 'db.log.remainder.only',
    'db.clamp.vec4', 'db.clamp.vec1', 'db.clamp.head', 'db.clamp.tail', 'db.clamp.early_return', 'db.clamp.floor',
    'db.clamp.slots>1', 'db.index>=2^31', 'db.stats_init.gridstride',
    'db.f64.threads>items', 'db.f64.one_pass', 'db.f64.stride',
    'c2r.empty', 'c2r.mag', 'c2r.phase', 'c2r.partial_wave', 'c2r.blocks>=2', 'c2r.gridstride2', 'c2r.gridstride3', 'c2r.misaligned',
    'c2r.f64',
)
EXCLUDED = (
    'db.clamp.slots>1',            # only the fused kernels pass slots > 1: tests/test_db_slots.py
    'db.index>=2^31',              # flat indices of 2^31 and more: at least 8.6 GB each way
    'db.stats_init.gridstride',    # more than 4096 * 256 items: test_decibel_more_than_2_pow_20_items
)

MUTANTS = (
    'log.a0_floor', 'log.a1_not_raised', 'log.tail_dropped', 'log.inflight_le', 'log.per_floor', 'log.item_plus_one',
    'log.hi_unclamped', 'clamp.early_return_swapped', 'clamp.global_max', 'clamp.forced_chunks_arg', 'clamp.per_floor',
    'clamp.tail_dropped', 'clamp.a0_floor', 'c2r.single_pass',
)
EQUIVALENT_MUTANTS = ('log.guard_removed', 'log.inflight_stride3', 'clamp.forced_chunks', 'c2r.step_blockdim')


def seed_of(case, salt=0):
    return zlib.crc32(case['id'].encode()) + salt


# =================================================================================================================
# float32 arithmetic, emulated exactly
# =================================================================================================================
def fma32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding.  The product of two float32 values is exact in float64 (48 bits); its float64 sum
    with c is not (tests/test_fb_pw.py's _fma32 stops there and double-rounds on float32 ties).  Here the sum's rounding error
    comes from TwoSum and the float64 sum is moved to its odd neighbour when the error is non-zero (rounding to odd): a 53-bit
    round-to-odd followed by the 24-bit round-to-nearest is the single rounding (53 >= 24 + 2)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all='ignore'):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        e = np.where(np.isfinite(s) & np.isfinite(e), e, 0.0)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where((e != 0) & even, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def mag_fma(x, y):
    """what k_cplx_to_real returns: float32 sqrt(fma(x, x, fl(y * y)))"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(all='ignore'):
        yy = (y.astype(np.float64) * y.astype(np.float64)).astype(np.float32)       # exact product, one rounding
        return np.sqrt(fma32(x, x, yy))


def enc_f(f):
    """kpr_common.h enc_f: order-preserving float -> unsigned"""
    u = np.asarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dec_f(u):
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


# =================================================================================================================
# decibel: the host's plan
# =================================================================================================================
def db_chunks(n_items, item_size):
    """kpr_host_mel.h db_chunks: blocks per item"""
    want = (DB_TARGET_BLOCKS + n_items - 1) // max(1, n_items)
    return max(1, min(DB_MAX_CHUNKS, want, item_size // DB_MIN_CHUNK))


def db_vec(x_offset, out_offset):
    """(VEC of k_db_log, VEC of k_db_clamp) from the float offsets of the two bases past a 16-byte boundary: the log pass needs
    both aligned, the clamp pass looks at `out` alone"""
    return (4 if (x_offset % 4 == 0 and out_offset % 4 == 0) else 1), (4 if out_offset % 4 == 0 else 1)


def db_block_range(block, item_size, chunks, mutant=None):
    """(item, g0, g1) of a workgroup"""
    item = (block + 1) // chunks if mutant == 'item_plus_one' else block // chunks
    chunk = block % chunks
    per = item_size // chunks if mutant == 'per_floor' else (item_size + chunks - 1) // chunks
    lo = min(item_size, chunk * per)
    hi = lo + per if mutant == 'hi_unclamped' else min(item_size, lo + per)
    return item, item * item_size + lo, item * item_size + hi


def db_split(g0, g1, vec, mutant=None):
    """[g0, a0) scalar head, [a0, a1) 16-byte vectors, [a1, g1) scalar tail"""
    if vec == 1:
        return g1, g1
    a0 = g0 // vec * vec if mutant == 'a0_floor' else min(g1, (g0 + vec - 1) // vec * vec)
    a1 = g1 // vec * vec if mutant == 'a1_not_raised' else max(a0, g1 // vec * vec)
    return a0, a1


def grid_1d(n, block=BLOCK, cap=GRID_CAP):
    return int(min(max((n + block - 1) // block, 1), cap))


def db_paths(n_items, item_size, chunks, vec, clamp=False):
    """closed form: the loop that touches each flat element -- HEAD / INFLIGHT / REMAINDER / TAIL in k_db_log, HEAD / VECTOR / TAIL
    in k_db_clamp -- and the number of empty blocks"""
    path = np.full(n_items * item_size, -1, np.int8)
    empty = 0
    for b in range(n_items * chunks):
        _, g0, g1 = db_block_range(b, item_size, chunks)
        if g1 == g0:
            empty += 1
            continue
        a0, a1 = db_split(g0, g1, vec)
        path[g0:a0] = HEAD
        path[a1:g1] = TAIL
        nv = (a1 - a0) // vec
        if nv <= 0:
            continue
        if clamp:
            path[a0:a1] = VECTOR
            continue
        r = np.arange(nv)
        t, k = r % BLOCK, r // BLOCK
        # thread t is in flight while t + 4 j B + 3 B < nv: n_if(t) = ceil((nv - t - 3 B) / (4 B)) rounds of four vectors
        n_if = np.maximum(0, -(-(nv - t - 3 * BLOCK) // (4 * BLOCK)))
        code = np.where(k < 4 * n_if, INFLIGHT, REMAINDER).astype(np.int8)
        path[a0:a1] = np.repeat(code, vec)
    return path, empty


def db_device_params(ref_value, amin):
    """make_db: the C ABI carries float32 parameters; amin is raised to the smallest normal float, ref_term is computed in double
    from the float32 values and rounded once"""
    ref32, amin32 = np.float32(ref_value), np.float32(amin)
    amin_k = np.maximum(amin32, FLT_MIN)
    ref_term = np.float32(10.0 * np.log10(max(float(amin32), float(ref32))))
    return amin_k, ref_term


def to_db_model(x, amin_k, ref_term):
    """to_db with a correctly rounded log2 in the place of v_log_f32 (which may differ from it by its one ulp)"""
    with np.errstate(all='ignore'):
        m = np.fmax(np.asarray(x, np.float32), amin_k)                       # fmaxf: NaN -> amin
        lg = np.log2(m.astype(np.float64)).astype(np.float32)
        return fma32(np.full(lg.shape, C_DB), lg, np.full(lg.shape, -ref_term, np.float32))


def to_db_bound(x, amin, ref):
    """|kernel - float64 oracle| for one element BEFORE the dynamic-range floor, in dB.  With m = max(x, amin), l = log2 m,
    c = 10 log10 2, r = 10 log10 max(amin, ref) the oracle is y = c l - r and the kernel fl(C L - R) (one fmaf), so
        |err| <= C spacing32(l)        v_log_f32 is off by at most one ulp of its result (the comment in kpr_common.h at to_db says
                                       "1 ulp"; taken from there, not measured here)
               + u c |l|               C = float32(10 log10 2)
               + u |r|                 R = float32(ref_term); the double-precision evaluation behind it adds ~1e-16
               + u (|y| + the above)   the single rounding of the fmaf
               + 2 (10 / ln 10) u      amin and ref_value cross the C ABI as float32: each moves its logarithm by at most u relative
    with u = 2^-24.  Elements at or under amin have m = amin exactly (also 0, negatives, -Inf, denormals, and NaN: fmaxf)."""
    x = np.asarray(x, np.float64)
    amin_k, ref_term = db_device_params(ref, amin)
    with np.errstate(all='ignore'):
        m = np.fmax(x, float(amin_k))
        l = np.log2(m)
        c = 10.0 * np.log10(2.0)
        r = abs(float(ref_term))
        y = c * l - float(ref_term)
        parts = float(C_DB) * np.spacing(np.abs(l).astype(np.float32)).astype(np.float64) + U32 * c * np.abs(l) + U32 * r
        parts = np.where(l == 0, U32 * r, parts)                       # log2(1) = 0 exactly: spacing32(0) is no ulp
        return parts + U32 * (np.abs(y) + parts) + 2 * (10.0 / np.log(10.0)) * U32


# =================================================================================================================
# decibel: the index-level emulation of k_stats_init + k_db_log + k_db_clamp
# =================================================================================================================
def _mut(mutant, kernel):
    return mutant.split('.', 1)[1] if mutant and mutant.startswith(kernel + '.') else None


def emulate_db(x, n_items, item_size, ref_value, amin, dyn, x_offset=0, out_offset=0, forced=0, mutant=None):
    """x: the flat float32 input.  Returns dict(out, writes (log-pass stores per element), path (the loop of the last store),
    clamp_path, clamp_writes, stats (the 2 n_items encoded words), block_stats [(item, max, min, issued)], decisions [(block,
    'return' | 'clamp')], oob (accesses outside the arrays: dropped and counted)).  `out` starts as NaN, as the GPU test poisons
    its allocation."""
    x = np.asarray(x, np.float32).reshape(-1)
    N = n_items * item_size
    assert x.size == N
    amin_k, ref_term = db_device_params(ref_value, amin)
    vec_log, vec_clamp = db_vec(x_offset, out_offset)
    out = np.full(N, np.nan, np.float32)
    writes, path = np.zeros(N, np.int32), np.full(N, -1, np.int8)
    cwrites, cpath = np.zeros(N, np.int32), np.full(N, -1, np.int8)
    tid = np.arange(BLOCK, dtype=np.int64)
    oob = [0]

    def inside(idx):
        ok = (idx >= 0) & (idx < N)
        oob[0] += int(idx.size - ok.sum())
        return idx[ok]

    # ---- k_stats_init --------------------------------------------------------------------------------------------
    stats = np.zeros(2 * n_items, np.uint32)
    grid = grid_1d(n_items)
    i = np.arange(grid * BLOCK, dtype=np.int64)
    while (i < n_items).any():
        sel = i[i < n_items]
        stats[2 * sel], stats[2 * sel + 1] = 0, 0xffffffff
        i = i + grid * BLOCK

    # ---- k_db_log ------------------------------------------------------------------------------------------------
    ml = _mut(mutant, 'log')
    chunks = forced if forced > 0 else db_chunks(n_items, item_size)
    block_stats = []
    for b in range(n_items * chunks):
        item, g0, g1 = db_block_range(b, item_size, chunks, ml)
        a0, a1 = db_split(g0, g1, vec_log, ml)
        ext = [-np.inf, np.inf]

        def visit(idx, code):
            idx = inside(idx)
            if idx.size == 0:
                return
            d = to_db_model(x[idx], amin_k, ref_term)
            out[idx] = d
            np.add.at(writes, idx, 1)
            path[idx] = code
            with np.errstate(all='ignore'):
                ext[0], ext[1] = np.fmax(ext[0], np.fmax.reduce(d)), np.fmin(ext[1], np.fmin.reduce(d))

        for part, (p0, p1) in enumerate(((g0, a0), (a1, g1))):            # scalar head and tail
            if part == 1 and ml == 'tail_dropped':
                continue
            i = p0 + tid
            while (i < p1).any():
                visit(i[i < p1], TAIL if part else HEAD)
                i = i + BLOCK
        lanes = np.arange(vec_log, dtype=np.int64)
        vhi = a1 // vec_log
        i = a0 // vec_log + tid
        while True:                                                        # four loads in flight
            act = (i + 3 * BLOCK <= vhi) if ml == 'inflight_le' else (i + 3 * BLOCK < vhi)
            if not act.any():
                break
            for q in range(4):
                visit(((i[act] + q * BLOCK)[:, None] * vec_log + lanes).reshape(-1), INFLIGHT)
            i = np.where(act, i + (3 if ml == 'inflight_stride3' else 4) * BLOCK, i)
        while (i < vhi).any():                                             # remainder
            visit((i[i < vhi][:, None] * vec_log + lanes).reshape(-1), REMAINDER)
            i = i + BLOCK
        issued = bool(ext[0] >= ext[1]) or ml == 'guard_removed'
        block_stats.append((item, float(ext[0]), float(ext[1]), issued))
        if issued:
            if 0 <= item < n_items:
                stats[2 * item] = max(stats[2 * item], enc_f(np.float32(ext[0])))
                stats[2 * item + 1] = min(stats[2 * item + 1], enc_f(np.float32(ext[1])))
            else:
                oob[0] += 2
    stats_after_log = stats.copy()

    # ---- k_db_clamp (slots = 1) ----------------------------------------------------------------------------------
    mc = _mut(mutant, 'clamp')
    own = db_chunks(n_items, item_size)                                    # db_clamp recomputes its own chunking
    grid_chunks = forced if (mc == 'forced_chunks' and forced > 0) else own
    karg = forced if (mc in ('forced_chunks', 'forced_chunks_arg') and forced > 0) else own
    decisions = []
    dyn32 = np.float32(dyn)
    lanes = np.arange(vec_clamp, dtype=np.int64)
    for b in range(n_items * grid_chunks):
        item, g0, g1 = db_block_range(b, item_size, karg, mc)
        if not 0 <= item < n_items:
            oob[0] += 1
            continue
        umax, umin = (stats[0::2].max() if mc == 'global_max' else stats[2 * item]), stats[2 * item + 1]
        with np.errstate(all='ignore'):
            thr = np.float32(dec_f(umax) - dyn32)
            if (dec_f(umax) if mc == 'early_return_swapped' else dec_f(umin)) >= thr:
                decisions.append((b, 'return'))
                continue
        decisions.append((b, 'clamp'))
        a0, a1 = db_split(g0, g1, vec_clamp, mc)

        def clamp(idx, code):
            idx = inside(idx)
            out[idx] = np.fmax(out[idx], thr)
            np.add.at(cwrites, idx, 1)
            cpath[idx] = code

        for part, (p0, p1) in enumerate(((g0, a0), (a1, g1))):
            if part == 1 and mc == 'tail_dropped':
                continue
            i = p0 + tid
            while (i < p1).any():
                clamp(i[i < p1], TAIL if part else HEAD)
                i = i + BLOCK
        i = a0 // vec_clamp + tid
        while (i < a1 // vec_clamp).any():
            clamp((i[i < a1 // vec_clamp][:, None] * vec_clamp + lanes).reshape(-1), VECTOR)
            i = i + BLOCK
    return dict(out=out.reshape(n_items, item_size), writes=writes, path=path, clamp_path=cpath, clamp_writes=cwrites,
                stats=stats_after_log, block_stats=block_stats, decisions=decisions, oob=oob[0], chunks=chunks)


# =================================================================================================================
# decibel: cases, inputs, checks
# =================================================================================================================
def dbcase(n_items, item_size, forced=0, **kw):
    ident = '%dx%d' % (n_items, item_size) + (' db_chunks %d' % forced if forced else '')
    return dict(id=ident, n_items=n_items, item_size=item_size, forced=forced, **kw)


DB_CASES = [
    dbcase(1, 1), dbcase(5, 3), dbcase(3, 1),                 # scalar only, the vector middle is empty
    dbcase(7, 1027),                                          # one chunk, remainder loop only
    dbcase(3, 3601),                                          # 900 vectors: threads 0..131 in flight, the rest in the remainder loop
    dbcase(3, 5003),                                          # one chunk, in-flight loop once + remainder
    dbcase(3, 8193),                                          # 2 chunks of 4097: odd boundaries
    dbcase(2, 12293),                                         # 3 chunks of 4098
    dbcase(300, 8195, big=True),                              # 2 chunks, many items
    dbcase(2049, 4099, big=True),                             # want = 1: one chunk although the item is large
    dbcase(1, 1050000, big=True),                             # the 256-chunk cap
    dbcase(2, 1000, forced=7), dbcase(2, 5, forced=8),        # tiny unaligned chunks; empty blocks
]
DB_VARIANTS = {'aligned': (0, 0), 'x+1': (1, 0), 'out+1': (0, 1)}     # floats of (x, out) past a 16-byte boundary
DB_PARAMS = [(1.0, 1e-5, 80.0), (0.7, 1e-7, 40.0), (1e-9, 1e-6, 0.5)]  # (ref_value, amin, dynamic_range); the last: ref < amin
DB_DYN_OFF = 1000.0                # run (a): more than the spread of any input here (the palette times the scales spans
#                                    2^-46 .. 2^29 and amin >= 1e-7: under 160 dB), so no floor applies
DB_F64_SIZES = (1, 1023, 1024, 1025, 8193)
PLACES = ('first', 'last', 'head', 'tail', 'inflight', 'remainder', 'lastchunk')
KINDS = ('wide', 'narrow', 'narrow+low')
SCALES = (0, 3, -5, 6, -2, 5, -6, 1, 4, -3, 2, -4, -1)        # item i is scaled by 2^SCALES[...]: neighbouring maxima differ


def db_plan(case):
    chunks = case['forced'] if case['forced'] else db_chunks(case['n_items'], case['item_size'])
    return dict(chunks=chunks, clamp_chunks=db_chunks(case['n_items'], case['item_size']),
                per=(case['item_size'] + chunks - 1) // chunks)


def db_branches(case, variant, early_return=True, floor=True):
    n, sz = case['n_items'], case['item_size']
    p = db_plan(case)
    vl, vc = db_vec(*DB_VARIANTS[variant])
    br = {'db.log.vec%d' % vl, 'db.clamp.vec%d' % vc}
    own = p['clamp_chunks']
    br.add('db.chunks=1' if own == 1 else 'db.chunks>=2')
    if (DB_TARGET_BLOCKS + n - 1) // n == 1 and sz >= DB_MIN_CHUNK:             # the item count, not the item size, says one chunk
        br.add('db.chunks.want1')
    if own == DB_MAX_CHUNKS:
        br.add('db.chunks.cap256')
    if case['forced']:
        br.add('db.chunks.forced')
    path, empty = db_paths(n, sz, p['chunks'], vl)
    if empty:
        br.add('db.block.empty')
    if sz % p['chunks'] and p['chunks'] > 1 and not empty:
        br.add('db.block.short')
    codes = set(np.unique(path).tolist())
    assert -1 not in codes
    br |= {'db.log.head'} if HEAD in codes else set()
    br |= {'db.log.tail'} if TAIL in codes else set()
    if vl == 4:
        if not codes & {INFLIGHT, REMAINDER}:
            br.add('db.log.middle.empty')
        if INFLIGHT in codes:
            br.add('db.log.inflight')
        if REMAINDER in codes:
            br.add('db.log.remainder' if INFLIGHT in codes else 'db.log.remainder.only')
        # some threads of one block in flight, others of the same block not: 768 < vectors of the block's middle < 1024
        for b in range(min(n * p['chunks'], 4)):
            _, g0, g1 = db_block_range(b, sz, p['chunks'])
            a0, a1 = db_split(g0, g1, 4)
            if 3 * BLOCK < (a1 - a0) // 4 < 4 * BLOCK:
                br.add('db.log.inflight.partial')
    cp, _ = db_paths(n, sz, own, vc, clamp=True)
    ccodes = set(np.unique(cp).tolist())
    if floor:
        br.add('db.clamp.floor')
        br |= {'db.clamp.head'} if HEAD in ccodes else set()
        br |= {'db.clamp.tail'} if TAIL in ccodes and vc == 4 else set()
    if early_return:
        br.add('db.clamp.early_return')
    return br


def db_places(case):
    """per item: in-item offsets of the seven places the maximum and the minimum are put at, taken from the aligned launch's
    paths (a place that does not exist at this shape falls back to the previous one in PLACES)"""
    n, sz = case['n_items'], case['item_size']
    p = db_plan(case)
    path, _ = db_paths(n, sz, p['chunks'], 4)
    path = path.reshape(n, sz)
    last_lo = min(sz - 1, (p['chunks'] - 1) * p['per'])
    last_lo = last_lo if last_lo < sz else 0
    places = np.zeros((n, len(PLACES)), np.int64)
    for i in range(n):
        row = path[i]
        pos = [0, sz - 1]
        for code in (HEAD, TAIL, INFLIGHT, REMAINDER):
            at = np.flatnonzero(row == code)
            pos.append(int(at[len(at) // 2]) if at.size else pos[-1])
        # a head / tail element of a LATER chunk where there is one (the first chunk of item 0 starts aligned)
        for k, code in ((2, HEAD), (3, TAIL)):
            at = np.flatnonzero(row == code)
            if at.size:
                pos[k] = int(at[-1] if code == HEAD else at[0])
        pos.append(min(sz - 1, last_lo + (sz - last_lo) // 2))
        places[i] = pos
    return places


def db_palette(kind, amin):
    """float32 values before the item's scale; `specials` are laid in unscaled"""
    j = np.arange(61)
    if kind == 'wide':
        mags = (2.0 ** (j - 40.0)) * (1.0 + (j * 37 % 61) / 64.0)                          # 61 magnitudes over 2^-40 .. 2^21
        specials = np.array([0.0, -0.0, -1.0, -np.inf, 1e-41, float(np.float32(amin))], np.float32)
    else:
        mags = (2.0 ** 20) * (1.0 + j / 1024.0)                                             # 0.25 dB wide
        specials = np.zeros(0, np.float32)
    return mags.astype(np.float32), specials


def db_input(case, params, rnd=0):
    """(x [n_items, item_size] float32, kinds [n_items]).  Item i: kind KINDS[(i + rnd) % 3], scale 2^SCALES[(2 i + rnd) % 13], its
    palette laid out by a seeded permutation; one element above everything else at place (i + rnd + 1) % 7 (the item's only maximum)
    and, for 'narrow+low', one element under amin at place rnd % 7: the only one outside any dynamic range of DB_PARAMS.
      wide        the whole palette and the specials: about half of the item lies under the floor of run (b)
      narrow      0.25 dB wide: run (b) must return early and leave it alone
      narrow+low  early return unless the single low element reached the statistics"""
    n, sz = case['n_items'], case['item_size']
    amin = params[1]
    rng = np.random.default_rng(seed_of(case, rnd))
    places = db_places(case)
    x = np.empty((n, sz), np.float32)
    kinds = []
    for i in range(n):
        kind = KINDS[(i + rnd) % 3]
        kinds.append(kind)
        scale = np.float32(2.0 ** SCALES[(2 * i + rnd) % len(SCALES)])
        mags, specials = db_palette(kind, amin)
        vals = np.concatenate([mags * scale, specials])
        x[i] = vals[np.resize(rng.permutation(vals.size), sz)]
        top = np.float32(2.0 ** 23) * scale
        if kind == 'narrow':
            top = np.float32(2.0 ** 20 * (1.0 + 62.0 / 1024.0)) * scale
        pmax, pmin = places[i][(i + rnd + 1) % 7], places[i][rnd % 7]
        if pmin == pmax:                                               # two places that fell back to one element
            pmin = (pmax + sz // 2) % sz
        if kind == 'narrow+low':
            top = np.float32(2.0 ** 20 * (1.0 + 62.0 / 1024.0)) * scale
            x[i, pmin] = np.float32(2.0 ** -35) * scale
        elif kind == 'wide':
            x[i, pmin] = 0.0                                           # (an item of two or three values has a floor to apply too)
        x[i, pmax] = top
    return x, kinds


def db_runs(case, index=0):
    """the (round, variant, parameter set) triples a case runs with, on the GPU and on the CPU alike: seven rounds (every place for
    the maximum and the low element) x three variants, every variant with every parameter set; the large cases one round"""
    for rnd in range(1 if case.get('big') else 7):
        for k, variant in enumerate(DB_VARIANTS):
            yield rnd, variant, DB_PARAMS[(rnd + (0 if case.get('big') else k) + index) % 3]


def db_expected_b(fa, dyn):
    """run (b) from run (a): the kernel's threshold is ONE float32 subtraction from the item's float32 maximum"""
    fa = np.asarray(fa, np.float32)
    thr = (fa.reshape(fa.shape[0], -1).max(1) - np.float32(dyn)).astype(np.float32)
    return np.maximum(fa, thr.reshape((-1,) + (1,) * (fa.ndim - 1)))


def db_checks(x, fa, fb, params, oracle, stats=None):
    """the assertions of the gate on one case: x the input, fa run (a) (dynamic range DB_DYN_OFF), fb run (b) (the case's),
    oracle = kapre_oracle.magnitude_to_decibel, stats = the 2 n_items statistics words where the caller owns the workspace.
    Returns (failures [str], worst error / bound of run (a), of run (b))."""
    ref, amin, dyn = params
    n = x.shape[0]
    x2, fa, fb = x.reshape(n, -1), np.asarray(fa, np.float32).reshape(n, -1), np.asarray(fb, np.float32).reshape(n, -1)
    fails = []
    if np.isnan(fa).any():
        fails.append('run (a): %d elements were never written (NaN poison)' % int(np.isnan(fa).sum()))
    # one bit pattern per input value, wherever it stands
    xb, fab = x2.reshape(-1).view(np.uint32), fa.reshape(-1).view(np.uint32)
    order = np.argsort(xb, kind='stable')
    same = xb[order][1:] == xb[order][:-1]
    diff = fab[order][1:] != fab[order][:-1]
    if (same & diff).any():
        fails.append('run (a): %d neighbouring pairs of equal inputs with different output bits' % int((same & diff).sum()))
    amin_k, _ = db_device_params(ref, amin)
    under = ~(x2 > amin_k)
    if under.any():
        floor_bits = np.unique(fa[under].view(np.uint32))
        at_amin = fa[x2 == amin_k].view(np.uint32)
        if floor_bits.size != 1 or (at_amin.size and at_amin[0] != floor_bits[0]):
            fails.append('run (a): values <= amin do not all give the bits of amin')
    bound = to_db_bound(x2, amin, ref)
    with np.errstate(all='ignore'):
        ea = np.abs(fa.astype(np.float64) - oracle(x2, ref, amin, DB_DYN_OFF))
        wa = float(np.nan_to_num(ea / bound, nan=np.inf).max())
    if wa > 1.0:
        fails.append('run (a): %.3f of to_db_bound' % wa)
    want_b = db_expected_b(fa, dyn)
    if not np.array_equal(fb.view(np.uint32), want_b.view(np.uint32)):
        bad = np.flatnonzero((fb.view(np.uint32) != want_b.view(np.uint32)).reshape(-1))
        fails.append('run (b): %d elements differ from max(f, item max - dyn), first at flat index %d' % (bad.size, bad[0]))
    # the floor: 1-Lipschitz in the element and in the item's maximum; one more float32 rounding for the subtraction
    top = np.nanargmax(np.where(np.isnan(fa), -np.inf, fa), axis=1)
    ob = oracle(x2, ref, amin, dyn)
    bb = np.maximum(bound, (bound[np.arange(n), top] + U32 * np.abs(ob.min(axis=1)))[:, None])
    with np.errstate(all='ignore'):
        wb = float(np.nan_to_num(np.abs(fb.astype(np.float64) - ob) / bb, nan=np.inf).max())
    if wb > 1.0:
        fails.append('run (b): %.3f of the bound' % wb)
    if stats is not None:
        st = np.asarray(stats, np.uint32)
        if not (np.array_equal(dec_f(st[0::2]), fa.max(1)) and np.array_equal(dec_f(st[1::2]), fa.min(1))):
            fails.append('statistics words are not the items\' maxima / minima')
    return fails, wa, wb


# =================================================================================================================
# k_cplx_to_real
# =================================================================================================================
C2R_SIZES = (0, 1, 63, 64, 65, 257)
C2R_STRIDE_SIZES = (GRID_CAP * BLOCK + 257, 2 * GRID_CAP * BLOCK + 1)          # second and third trip of the grid stride


def c2r_branches(n, phase=False, misaligned=False, f64=False):
    if n == 0:
        return {'c2r.empty'}
    br = {'c2r.phase' if phase else 'c2r.mag'}
    if n % 64:
        br.add('c2r.partial_wave')
    if n > BLOCK:
        br.add('c2r.blocks>=2')
    if n > GRID_CAP * BLOCK:
        br.add('c2r.gridstride2')
    if n > 2 * GRID_CAP * BLOCK:
        br.add('c2r.gridstride3')
    if misaligned:
        br.add('c2r.misaligned')
    if f64:
        br.add('c2r.f64')
    return br


def c2r_trips(n):
    """closed form: the trip of the grid-stride loop that writes each element"""
    return np.arange(n) // (grid_1d(n) * BLOCK)


def emulate_c2r(re, im, fn=mag_fma, mutant=None):
    """every thread of the capped grid walks i = blockIdx * 256 + threadIdx, += gridDim * 256.  Returns (out (NaN where nothing was
    written), writes per element, trip of the last write)."""
    n = re.size
    out, writes, trip = np.full(n, np.nan, np.float32), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    if n == 0:
        return out, writes, trip                                   # run_cplx_to_real launches nothing
    mc = _mut(mutant, 'c2r')
    grid = grid_1d(n)
    start = (np.arange(grid)[:, None] * BLOCK + np.arange(BLOCK)[None, :]).reshape(-1)
    if mc == 'step_blockdim':
        # thread s writes s, s + 256, ...: element e is written by the threads s <= e with s = e (mod 256)
        e = np.arange(n)
        out[:] = fn(re, im)
        writes[:] = np.minimum(e, start[-1]) // BLOCK + 1
        trip[:] = (e - e % BLOCK) // BLOCK
        return out, writes, trip
    i, k = start, 0
    while (i < n).any():
        sel = i[i < n]
        out[sel] = fn(re[sel], im[sel])
        writes[sel] += 1
        trip[sel] = k
        if mc == 'single_pass':
            break
        i, k = i + grid * BLOCK, k + 1
    return out, writes, trip


def db_f64_branches(item_size):
    return {'db.f64.threads>items' if item_size < F64_BLOCK else 'db.f64.one_pass' if item_size == F64_BLOCK else 'db.f64.stride'}


# ---- Phase: inputs of the bound check ---------------------------------------------------------------------------------
PHASE_K_ULP = 6                    # the OpenCL full-profile limit for atan2, which the ROCm device library is written to


def phase_inputs(seed=5, n=40000):
    """(re, im) float32: all four quadrants, |im / re| = 2^U(-40, 40), radii 2^U(-20, 20); a tenth hug an axis
    (|im / re| in 2^-40 .. 2^-30 or 2^30 .. 2^40)"""
    rng = np.random.default_rng(seed)
    e = rng.uniform(-40, 40, n)
    hug = rng.random(n) < 0.1
    e = np.where(hug, np.sign(e) * rng.uniform(30, 40, n), e)
    r = 2.0 ** rng.uniform(-20, 20, n)
    ratio = 2.0 ** e
    re = (r / np.sqrt(1 + ratio * ratio)) * rng.choice([-1.0, 1.0], n)
    im = (r * ratio / np.sqrt(1 + ratio * ratio)) * rng.choice([-1.0, 1.0], n)
    return re.astype(np.float32), im.astype(np.float32)


def ulp_error(got, want64):
    """|got - want| in float32 ulps of want (signed comparison, no modulo)"""
    want64 = np.asarray(want64, np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)


def phase_special_inputs():
    """(re, im) of the IEEE special cases of atan2(im, re): every sign combination of (+-0, +-0), (+-0, +-x), (+-y, +-0),
    (+-Inf, finite), (finite, +-Inf), (+-Inf, +-Inf)"""
    z, f, inf = [0.0, -0.0], [1.5, -1.5, 3e-30, -3e-30, 2e30, -2e30], [np.inf, -np.inf]
    pairs = [(a, b) for a in z for b in z] + [(a, b) for a in z for b in f] + [(a, b) for a in f for b in z]
    pairs += [(a, b) for a in inf for b in f + z] + [(a, b) for a in f + z for b in inf] + [(a, b) for a in inf for b in inf]
    re = np.array([p[0] for p in pairs], np.float32)
    im = np.array([p[1] for p in pairs], np.float32)
    return re, im
