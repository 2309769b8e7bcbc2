"""The pointwise gate's checker is itself checked (no GPU): tests/pointwise_model.py restates the launches of Magnitude, Phase and
MagnitudeToDecibel, so (1) its constants must be the ones in the source text, (2) its case tables must reach every branch it names
outside EXCLUDED, (3) its closed-form plan must agree with its index-level emulation element by element, (4) the emulation must
pass the very checks the GPU test applies (pointwise_model.db_checks), (5) each emulation with one wrong line must fail them on at
least one case -- and the four wrong lines that change no output must be shown to change none -- and (6) mag_fma must be the
correctly rounded float32 sqrt(fma(x, x, fl(y y))), proved against fractions.Fraction.  It also measures the reference of the
Phase bound: float32 np.arctan2 against float64 np.arctan2 on the gate's inputs.
"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import kapre_oracle as o
import pointwise_model as m

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'kapre_amd', 'csrc')


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


# ---- 1. constants ------------------------------------------------------------------------------------------------
def test_constants_are_the_ones_in_the_source():
    mel, host, misc, ops, gen, common = (source(n) for n in ('kpr_host_mel.h', 'kpr_host.h', 'kpr_misc_kernels.h',
                                                             'kpr_host_ops.h', 'kpr_generic_kernels.h', 'kpr_common.h'))
    hip = ops + mel                                      # the decibel bodies (kpr_host_ops.h), the statistics-init helper
    want, cap, per = one(r'const long long want = \((\d+) \+ n_items - 1\) / std::max<long long>\(1, n_items\);\s*'
                         r'return \(int\)std::max<long long>\(1, std::min<long long>\(std::min<long long>\((\d+), want\), item_size / (\d+)\)\);', mel)
    assert (int(want), int(cap), int(per)) == (m.DB_TARGET_BLOCKS, m.DB_MAX_CHUNKS, m.DB_MIN_CHUNK)
    a, b = one(r'static int grid_1d\(long long n, int block, int cap = (\d+) \* (\d+)\)', host)
    assert int(a) * int(b) == m.GRID_CAP
    assert 'const dim3 grid(grid_1d(n, 256));' in ops and 'dim3(grid_1d(n_items, 256)), dim3(256), 0, st, stats' in hip
    assert misc.count('__launch_bounds__(256) void k_db_') == 2
    assert 'i + 3 * (long long)blockDim.x < vhi; i += 4 * (long long)blockDim.x' in misc
    assert 'a0 = min(g1, (g0 + VEC - 1) / VEC * VEC);' in misc and 'a1 = max(a0, g1 / VEC * VEC);' in misc
    assert misc.count('const long long per = (item_size + chunks - 1) / chunks;') == 2
    assert misc.count('const long long lo = min(item_size, chunk * per), hi = min(item_size, lo + per);') == 2
    assert 'if (dec_f(umin) >= thr) return;' in misc and 'if (mx >= mn) {' in misc
    # VEC: the log pass from both bases, the clamp pass from `out`; the forced option moves the log pass alone
    assert 'with_vec<4>(((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0' in hip
    assert 'if ((((uintptr_t)out) & 15) == 0)' in mel and 'const int chunks = db_chunks(n_items, item_size);' in mel
    assert 'if (opt(OPT_DB_CHUNKS) > 0) chunks = opt(OPT_DB_CHUNKS);' in hip and mel.count('OPT_DB_CHUNKS') == 0
    assert np.float32(float(one(r'return fmaf\(([0-9.]+)f, __builtin_amdgcn_logf\(fmaxf\(v, db\.amin\)\), -db\.ref_term\);', common))) == m.C_DB
    assert 'd.amin = std::max(db->amin, 1.17549435e-38f);' in mel
    assert 'dim3((unsigned)n_items), dim3(%d), 0, (hipStream_t)stream, x,' % m.F64_BLOCK in hip and '__launch_bounds__(%d) void k_db_f64' % m.F64_BLOCK in gen
    # one expression for |z| in Magnitude, HPSS and TimeStretch
    expr = r'sqrtf\(fmaf\((\w+)\.x, \1\.x, \1\.y \* \1\.y\)\)'
    assert len(re.findall(expr, misc)) == 1 and len(re.findall(expr, source('kpr_hpss_kernels.h'))) == 1
    assert len(re.findall(expr, source('kpr_time_stretch_kernels.h'))) == 1


# ---- 2. coverage -------------------------------------------------------------------------------------------------
def table_branches():
    reached = {}
    for c in m.DB_CASES:
        for v in m.DB_VARIANTS:
            for b in m.db_branches(c, v):
                reached.setdefault(b, '%s %s' % (c['id'], v))
    for n in m.C2R_SIZES + m.C2R_STRIDE_SIZES:
        for b in m.c2r_branches(n) | m.c2r_branches(n, phase=True) | (m.c2r_branches(n, f64=True) if n == 257 else set()):
            reached.setdefault(b, 'c2r %d' % n)
    reached.setdefault('c2r.misaligned', 'c2r 257 one complex value into its buffer')
    for n in m.DB_F64_SIZES:
        for b in m.db_f64_branches(n):
            reached.setdefault(b, 'f64 %d' % n)
    return reached


def test_every_branch_has_a_case():
    assert len(set(m.BRANCHES)) == len(m.BRANCHES) and set(m.EXCLUDED) <= set(m.BRANCHES)
    reached = table_branches()
    assert set(reached) <= set(m.BRANCHES), set(reached) - set(m.BRANCHES)
    missing = [b for b in m.BRANCHES if b not in reached and b not in m.EXCLUDED]
    assert not missing, missing
    assert not [b for b in m.EXCLUDED if b in reached]


def test_the_cases_the_issue_names_take_the_path_it_says():
    br = {c['id']: m.db_branches(c, 'aligned') for c in m.DB_CASES}
    for cid in ('1x1', '5x3', '3x1'):
        assert 'db.log.middle.empty' in br[cid] and not br[cid] & {'db.log.inflight', 'db.log.remainder', 'db.log.remainder.only'}
    assert 'db.log.remainder.only' in br['7x1027'] and 'db.chunks=1' in br['7x1027']
    assert {'db.log.inflight', 'db.log.remainder', 'db.chunks=1'} <= br['3x5003'] and 'db.log.inflight.partial' not in br['3x5003']
    assert 'db.log.inflight.partial' in br['3x3601']
    by = {c['id']: c for c in m.DB_CASES}
    assert (m.db_plan(by['3x8193'])['chunks'], m.db_plan(by['3x8193'])['per']) == (2, 4097)
    assert (m.db_plan(by['2x12293'])['chunks'], m.db_plan(by['2x12293'])['per']) == (3, 4098)
    assert m.db_plan(by['300x8195'])['chunks'] == 2 and 'db.chunks>=2' in br['300x8195']
    assert m.db_plan(by['2049x4099'])['chunks'] == 1 and m.db_chunks(2048, 4099) == 1 and m.db_chunks(1024, 8192) == 2
    assert 'db.chunks.want1' in br['2049x4099'] and 'db.chunks.want1' not in br['300x8195']
    assert m.db_plan(by['1x1050000'])['chunks'] == 256 and 'db.chunks.cap256' in br['1x1050000']
    assert m.db_chunks(1, 8191) == 1 and m.db_chunks(1, 8192) == 2                     # more than one block per item from 8192 floats
    assert 'db.block.empty' in br['2x5 db_chunks 8'] and 'db.chunks.forced' in br['2x1000 db_chunks 7']
    assert m.db_plan(by['2x1000 db_chunks 7']) == dict(chunks=7, clamp_chunks=1, per=143)
    assert m.db_vec(0, 0) == (4, 4) and m.db_vec(1, 0) == (1, 4) and m.db_vec(0, 1) == (1, 1)
    assert m.c2r_branches(m.C2R_STRIDE_SIZES[0]) >= {'c2r.gridstride2'} and 'c2r.gridstride3' not in m.c2r_branches(m.C2R_STRIDE_SIZES[0])
    assert 'c2r.gridstride3' in m.c2r_branches(m.C2R_STRIDE_SIZES[1])


# ---- 3 + 4. the plan agrees with the emulation; the emulation passes the gate's checks ------------------------------------
def run_pair(c, variant, params, rnd=0, mutant=None):
    x, kinds = m.db_input(c, params, rnd)
    xo, oo = m.DB_VARIANTS[variant]
    kw = dict(x_offset=xo, out_offset=oo, forced=c['forced'], mutant=mutant)
    ea = m.emulate_db(x, c['n_items'], c['item_size'], params[0], params[1], m.DB_DYN_OFF, **kw)
    eb = m.emulate_db(x, c['n_items'], c['item_size'], *params, **kw)
    return x, kinds, ea, eb


@pytest.mark.parametrize('cid', [c['id'] for c in m.DB_CASES])
def test_plan_agrees_with_the_emulation_and_the_emulation_passes_the_checks(cid):
    c = {c['id']: c for c in m.DB_CASES}[cid]
    n, sz = c['n_items'], c['item_size']
    for rnd, variant, params in m.db_runs(c, [k['id'] for k in m.DB_CASES].index(cid)):
        if c.get('big') and variant != 'aligned':
            continue
        x, kinds, ea, eb = run_pair(c, variant, params, rnd)
        vl, vc = m.db_vec(*m.DB_VARIANTS[variant])
        p = m.db_plan(c)
        path, empty = m.db_paths(n, sz, p['chunks'], vl)
        assert ea['oob'] == 0 and eb['oob'] == 0
        np.testing.assert_array_equal(ea['path'], path)
        assert (ea['writes'] == 1).all()                                   # every element once: no overlap between blocks or loops
        assert sum(1 for s in ea['block_stats'] if not s[3]) == empty       # exactly the empty blocks issue no atomics
        fa, fb = ea['out'], eb['out']
        np.testing.assert_array_equal(m.dec_f(ea['stats'][0::2]), fa.max(1))
        np.testing.assert_array_equal(m.dec_f(ea['stats'][1::2]), fa.min(1))
        assert all(d == 'return' for _, d in ea['decisions'])              # run (a): no floor anywhere
        # run (b): the clamp pass covers exactly the items whose minimum lies under the floor, once, along the planned paths
        cpath, _ = m.db_paths(n, sz, p['clamp_chunks'], vc, clamp=True)
        active = fa.min(1) < (fa.max(1) - np.float32(params[2])).astype(np.float32)
        for i, kind in enumerate(kinds):
            assert active[i] == (kind != 'narrow' and not (sz == 1)), (i, kind)
        want_w = np.repeat(active, sz).astype(np.int32)
        np.testing.assert_array_equal(eb['clamp_writes'], want_w)
        np.testing.assert_array_equal(eb['clamp_path'], np.where(want_w == 1, cpath, -1))
        assert [d for _, d in eb['decisions']] == ['clamp' if active[b // p['clamp_chunks']] else 'return' for b in range(n * p['clamp_chunks'])]
        fails, wa, wb = m.db_checks(x, fa, fb, params, o.magnitude_to_decibel, stats=ea['stats'])
        assert not fails, (cid, variant, fails)
        assert wa <= 1.0 and wb <= 1.0


def test_every_place_is_used_for_a_maximum_and_a_minimum():
    """over the rounds the GPU test runs, the maximum and the single low element stand in every one of the seven places"""
    c = {c['id']: c for c in m.DB_CASES}['3x8193']
    path, _ = m.db_paths(3, 8193, 2, 4)
    path = path.reshape(3, -1)
    places = m.db_places(c)
    assert [int(path[1][places[1][k]]) for k in (2, 3, 4, 5)] == [m.HEAD, m.TAIL, m.INFLIGHT, m.REMAINDER]
    assert places[1][0] == 0 and places[1][1] == 8192 and places[1][6] >= 4097
    seen_max, seen_min = set(), set()
    for rnd in range(7):
        x, kinds = m.db_input(c, m.DB_PARAMS[0], rnd)
        for i in range(3):
            seen_max.add(int(np.flatnonzero(places[i] == x[i].argmax())[0]))
            if kinds[i] == 'narrow+low':
                seen_min.add(int(np.flatnonzero(places[i] == x[i].argmin())[0]))
    assert seen_max == set(range(7)) and seen_min == set(range(7))


# ---- 5. mutants --------------------------------------------------------------------------------------------------
SMALL = [c for c in m.DB_CASES if not c.get('big')]


def db_mutant_killed(mutant):
    for rnd in range(7):
        for c in SMALL:
            for k, variant in enumerate(m.DB_VARIANTS):
                params = m.DB_PARAMS[(rnd + k) % 3]
                x, _, ea, eb = run_pair(c, variant, params, rnd, mutant)
                fails, _, _ = m.db_checks(x, ea['out'], eb['out'], params, o.magnitude_to_decibel)
                if fails:
                    return '%s %s round %d: %s' % (c['id'], variant, rnd, fails[0])
    return None


def c2r_mutant_killed(mutant):
    for n in (257, m.GRID_CAP * m.BLOCK + 257):
        rng = np.random.default_rng(n)
        re, im = (rng.integers(-2047, 2048, n).astype(np.float32) for _ in range(2))
        out, _, _ = m.emulate_c2r(re, im, mutant=mutant)
        want = np.sqrt((re * re + im * im).astype(np.float32))
        if not np.array_equal(out.view(np.uint32), want.view(np.uint32)):
            return 'c2r %d: %d elements differ' % (n, int((out.view(np.uint32) != want.view(np.uint32)).sum()))
    return None


@pytest.mark.parametrize('mutant', m.MUTANTS)
def test_each_mutant_fails_the_checks_of_the_gate(mutant):
    how = (c2r_mutant_killed if mutant.startswith('c2r.') else db_mutant_killed)(mutant)
    print('pointwise model: mutant %-28s killed by %s' % (mutant, how))
    assert how is not None, mutant
    KILLED.add(mutant)


KILLED = set()


def test_the_equivalent_mutants_change_no_output():
    """the four wrong lines of EQUIVALENT_MUTANTS: the same outputs and statistics words on every small case, variant and
    parameter set -- only the access counts differ (which no test of outputs can see)"""
    assert len(m.MUTANTS) >= 12 and not set(m.MUTANTS) & set(m.EQUIVALENT_MUTANTS)
    differs = {k: False for k in m.EQUIVALENT_MUTANTS}
    for c in SMALL:
        for k, variant in enumerate(m.DB_VARIANTS):
            params = m.DB_PARAMS[k % 3]
            _, _, ea, eb = run_pair(c, variant, params, k)
            for mutant in m.EQUIVALENT_MUTANTS[:3]:
                _, _, ma, mb = run_pair(c, variant, params, k, mutant)
                for e, f in ((ea, ma), (eb, mb)):
                    np.testing.assert_array_equal(e['out'].view(np.uint32), f['out'].view(np.uint32), err_msg=mutant)
                    np.testing.assert_array_equal(e['stats'], f['stats'], err_msg=mutant)
                    assert f['oob'] == 0
                differs[mutant] |= (not np.array_equal(ea['writes'], ma['writes']) or not np.array_equal(eb['clamp_path'], mb['clamp_path'])
                                    or [s[3] for s in ea['block_stats']] != [s[3] for s in ma['block_stats']])
    n = m.GRID_CAP * m.BLOCK + 257
    re, im = np.arange(n, dtype=np.float32) % 2047, np.ones(n, np.float32)
    out, writes, _ = m.emulate_c2r(re, im)
    mout, mwrites, _ = m.emulate_c2r(re, im, mutant='c2r.step_blockdim')
    np.testing.assert_array_equal(out.view(np.uint32), mout.view(np.uint32))
    assert (writes == 1).all() and mwrites.max() == m.GRID_CAP
    differs['c2r.step_blockdim'] = True
    assert all(differs.values()), differs                         # the emulation does see each of them, in what the GPU cannot show
    print('pointwise model: %d equivalent mutants change no output: %s' % (len(differs), ', '.join(differs)))


def test_mutant_count():
    """runs after the mutant tests: prints the count"""
    if not KILLED:
        pytest.skip('the mutant tests did not run in this session')
    print('pointwise model: %d of %d mutants killed (+ %d proved equivalent)' % (len(KILLED), len(m.MUTANTS), len(m.EQUIVALENT_MUTANTS)))
    assert KILLED == set(m.MUTANTS)


# ---- k_cplx_to_real: plan and emulation ---------------------------------------------------------------------------------
def test_c2r_plan_agrees_with_the_emulation():
    for n in m.C2R_SIZES + m.C2R_STRIDE_SIZES:
        re, im = (np.arange(n) % 4095 - 2047).astype(np.float32), (np.arange(n) % 17 - 8).astype(np.float32)
        out, writes, trip = m.emulate_c2r(re, im)
        assert (writes == 1).all()
        np.testing.assert_array_equal(trip, m.c2r_trips(n))
        np.testing.assert_array_equal(out, np.sqrt((re * re + im * im).astype(np.float32)))       # integers: exact whatever is fused
    assert m.c2r_trips(m.C2R_STRIDE_SIZES[0]).max() == 1 and m.c2r_trips(m.C2R_STRIDE_SIZES[1]).max() == 2
    assert m.grid_1d(m.C2R_STRIDE_SIZES[0]) == 4096 and m.grid_1d(257) == 2 and m.grid_1d(1) == 1


# ---- 6. mag_fma ---------------------------------------------------------------------------------------------------
def round_f32(q):
    """a non-negative Fraction rounded to the nearest float32 (ties to even), exactly"""
    if q == 0:
        return np.float32(0.0)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    scaled = q / Fraction(2) ** (e - 23)                        # the float32 grid at this exponent is the integers
    lo = scaled.numerator // scaled.denominator
    rem = scaled - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2):
        lo += 1
    return np.float32(np.ldexp(float(lo), e - 23))


def test_mag_fma_is_the_exact_float32_fma():
    rng = np.random.default_rng(2024)
    n = 10000
    x = (2.0 ** rng.uniform(-40, 40, n) * rng.choice([-1, 1], n)).astype(np.float32)
    y = (2.0 ** rng.uniform(-40, 40, n) * rng.choice([-1, 1], n)).astype(np.float32)
    y[: n // 2] = (x[: n // 2] * 2.0 ** rng.uniform(-13, 13, n // 2)).astype(np.float32)      # comparable squares: where ties live
    yy = (y.astype(np.float64) ** 2).astype(np.float32)
    got = m.fma32(x, x, yy)
    naive = (x.astype(np.float64) * x.astype(np.float64) + yy.astype(np.float64)).astype(np.float32)
    for i in range(n):
        want = round_f32(Fraction(float(x[i])) ** 2 + Fraction(float(yy[i])))
        assert got[i] == want, (i, x[i], y[i])
        assert round_f32(Fraction(float(y[i])) ** 2) == yy[i]
    np.testing.assert_array_equal(m.mag_fma(x, y), np.sqrt(got))
    # a float64 sum alone double-rounds: x^2 = 1 + 2^-11 + 2^-24 exactly, a float32 tie; adding 2^-60 puts the sum just above the
    # tie, the float64 addition rounds it back onto the tie and the float32 cast then rounds to even -- downwards
    a, c = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    exact = round_f32(Fraction(float(a)) ** 2 + Fraction(float(c)))
    two_step = np.float32(float(a) * float(a) + float(c))
    assert m.fma32(a, a, c) == exact and two_step != exact
    print('mag_fma: %d draws equal the Fraction result; the float64 sum alone differs on %d of them' % (n, int((naive != got).sum())))
    # exact inputs: whatever is fused, integer components give the correctly rounded root of the exact sum
    xi, yi = (rng.integers(-2047, 2048, 5000).astype(np.float32) for _ in range(2))
    np.testing.assert_array_equal(m.mag_fma(xi, yi), np.sqrt((xi * xi + yi * yi).astype(np.float32)))
    with np.errstate(all='ignore'):
        assert m.mag_fma(np.float32(1e20), np.float32(0)) == np.inf and m.mag_fma(np.float32(0), np.float32(1e20)) == np.inf


# ---- to_db_bound ------------------------------------------------------------------------------------------------------
def test_to_db_bound_holds_for_any_log_within_one_ulp():
    """the bound is derived for a log2 off by up to one float32 ulp: push the model's log one ulp each way and stay inside"""
    rng = np.random.default_rng(3)
    x = np.concatenate([(2.0 ** rng.uniform(-45, 30, 20000)).astype(np.float32), np.float32([0, -1, 1, 1e-5, 1e-41, -np.inf, 0.99999994, 1.0000001])])
    for ref, amin, _ in m.DB_PARAMS:
        amin_k, ref_term = m.db_device_params(ref, amin)
        mm = np.fmax(x, amin_k)
        lg = np.log2(mm.astype(np.float64)).astype(np.float32)
        want = o.magnitude_to_decibel(x, ref, amin, m.DB_DYN_OFF)
        bound = m.to_db_bound(x, amin, ref)
        for lgv in (lg, np.nextafter(lg, np.float32(np.inf)), np.nextafter(lg, np.float32(-np.inf))):
            lgv = np.where(lg == 0, lg, lgv)
            got = m.fma32(np.full(lg.shape, m.C_DB), lgv, np.full(lg.shape, -ref_term, np.float32))
            assert (np.abs(got.astype(np.float64) - want) <= bound).all()
        assert bound.max() < 2.5e-5                               # (2^-45 .. 2^30; the golden tests allow 1e-4 / 1e-5)
    assert m.db_device_params(1e-9, 1e-6)[1] == np.float32(10 * np.log10(float(np.float32(1e-6))))      # ref < amin


# ---- the Phase reference --------------------------------------------------------------------------------------------------
def test_float32_arctan2_against_float64_on_the_gate_inputs():
    """the reference alone: float32 np.arctan2 against float64 np.arctan2 on the inputs of the bound check.  One ulp was the
    expectation; numpy 2.2's float32 arctan2 measures 2.633 ulp here (239 of 40 000 points above one ulp), so it is held to the
    limit the kernel is held to, and it serves as the bit-exact reference on the IEEE special cases only.  The GPU test records
    the kernel's figure next to this one; DESIGN.md 4.8.3 quotes both."""
    re, im = m.phase_inputs()
    assert re.size == 40000 and (re > 0).any() and (re < 0).any() and (im > 0).any() and (im < 0).any()
    ratio = np.abs(im.astype(np.float64) / re.astype(np.float64))
    assert ratio.min() < 2.0 ** -39 and ratio.max() > 2.0 ** 39
    want = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    worst = float(m.ulp_error(np.arctan2(im, re), want).max())
    print('phase reference: float32 np.arctan2 is at most %.3f ulp from float64 np.arctan2 (kernel bound: %d ulp)' % (worst, m.PHASE_K_ULP))
    assert worst <= m.PHASE_K_ULP
    sre, sim = m.phase_special_inputs()
    assert sre.size == 4 + 12 + 12 + 16 + 16 + 4
