"""The generic gate's checker is itself checked (no GPU): tests/generic_model.py restates the size-generic FFT engine, k_ola and
k_filterbank_f64, so (1) its constants must be the ones in the source text, (2) its case tables must reach every branch it names,
(3) its emulations must agree with numpy.fft in longdouble within the derived bounds on every case -- float64 and float32 -- and
(4) each emulation with one wrong line must leave its bound, or form an index outside a buffer, on at least one case: else the table
could not tell that kernel bug either.  (5) The float-reciprocal divisions of the pass loops are exact for every pair the cases form.
"""
import os
import re

import numpy as np
import pytest

import generic_model as m
import proto_generic_fft as pg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'kapre_amd', 'csrc')
HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 1e-18


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def product(expr):
    out = 1
    for factor in expr.split('*'):
        out *= int(factor)
    return out


# ---- 1. constants ------------------------------------------------------------------------------------------------
def test_constants_are_the_ones_in_the_source():
    kern, fft, host = source('kpr_generic_kernels.h'), source('kpr_host_fft.h'), source('kpr_host.h')
    assert int(one(r'constexpr int kF64Threads = (\d+);', kern)) == m.THREADS
    assert int(one(r'constexpr int kGenMaxPasses = (\d+);', kern)) == m.MAX_PASSES
    # the U of each gen_fft switch arm, and which form each radix takes
    arms = re.findall(r'case (\d+): (gen_pass_bf|gen_pass)<(\d+), (\d+)>\(a, b, tw, tws, N, (?:R, )?ns, sign\); break;', kern)
    assert {int(r): (fn, int(rc), int(u)) for r, fn, rc, u in arms} == {
        2: ('gen_pass_bf', 2, m.U_OF[2]), 3: ('gen_pass_bf', 3, m.U_OF[3]), 4: ('gen_pass_bf', 4, m.U_OF[4]),
        5: ('gen_pass_bf', 5, m.U_OF[5]), 7: ('gen_pass', 7, m.U_OF[7])}
    assert int(one(r'default: gen_pass<0, (\d+)>\(a, b, tw, tws, N, R, ns, sign\); break;', kern)) == m.U_OF[0]
    assert kern.count('+= U * kF64Threads)') == 2 and kern.count('u * kF64Threads < ') == 2
    # the eight-per-thread frame load, the four-per-thread spectrum load, the groups of four of the run-time radix
    assert int(one(r'n0 < N; n0 \+= (\d+) \* kF64Threads\)', kern)) == m.LOAD_UNROLL
    assert kern.count('for (int u = 0; u < %d; ++u) {' % m.LOAD_UNROLL) == 2 and 'T sv[%d], wv[%d];' % ((m.LOAD_UNROLL,) * 2) in kern
    assert int(one(r'k0 < M; k0 \+= (\d+) \* kF64Threads\)', kern)) == m.SPEC_UNROLL
    assert 'T2 sv[%d], sm[%d];' % ((m.SPEC_UNROLL,) * 2) in kern
    assert int(one(r'for \(int r0 = 1; r0 < R; r0 \+= (\d+)\) \{', kern)) == m.RT_GROUP and 'T2 v[%d], w[%d];' % ((m.RT_GROUP,) * 2) in kern
    # 160 KiB: gen_lds (twice), gen_grid, and what allow_big_lds asks for
    assert 'if (2 * buf > 160 * 1024) return false;' in fft and '*tw_lds = 2 * buf + tab <= 160 * 1024;' in fft
    assert fft.count('160 * 1024') == 3 and product('160 * 1024') == m.LDS_LIMIT
    assert product(one(r'hipFuncAttributeMaxDynamicSharedMemorySize, (\d+ \* \d+)\)', host)) == m.LDS_LIMIT
    per_cu, wgs = one(r'std::min<long long>\((\d+), \(160 \* 1024\) / std::max<size_t>\(lds, 1\)\)\);\n'
                      r'    return \(int\)std::max<long long>\(1, std::min<long long>\(g\.total_frames, (\d+) \* per_cu\)\);', fft)
    assert (int(per_cu), int(wgs)) == (m.GRID_PER_CU, m.GRID_WGS)
    assert product(one(r'static int grid_1d\(long long n, int block, int cap = (\d+ \* \d+)\)', host)) == m.GRID_1D_CAP
    assert int(one(r'for \(int f = 3; f <= (\d+) && m > 1; f \+= 2\)', fft)) == m.MAX_RADIX
    assert m.REFUSAL_TEXT in fft
    # k_ola and k_filterbank_f64 are launched with grid_1d's default cap
    assert 'k_ola<T>, dim3(grid_1d(n_sig * t_out, 256)), dim3(256)' in source('kpr_host_istft.h')
    assert 'k_filterbank_f64, dim3(grid_1d(total, 256)), dim3(256)' in source('kpr_host_ops.h')


def test_a_refused_size_returns_before_any_launch():
    """gen_launch_plan is the first statement of both launchers that can fail: a refused size launches nothing"""
    for name, fn in (('kpr_host_stft.h', 'launch_stft_gen'), ('kpr_host_istft.h', 'launch_irfft_gen')):
        body = source(name).split('static int %s(' % fn)[1]
        first = body.split('GenLaunch l;\n')[1].lstrip().split('\n')[0]
        assert first == 'if (int e = gen_launch_plan(sizeof(T2), g.n_fft, &l)) return e;', first
        assert body.index('gen_launch_plan') < body.index('launch_gen(')


def test_the_plan_model_agrees_with_the_edges_the_issue_names():
    e = m.EDGES
    assert e['f64', 0] == dict(twl_last=5120, twg_first=5122, fit_last=10240, refused=10242)
    assert e['f64', 1] == dict(twl_last=3413, twg_first=3415, fit_last=5119, refused=5121)
    assert e['f32', 0]['twl_last'] == 10240 and e['f32', 0]['fit_last'] == 20480
    assert e['f32', 0]['twg_first'] > 10240 and e['f32', 1]['twl_last'] * 24 <= m.LDS_LIMIT < e['f32', 1]['twg_first'] * 24
    assert e['f32', 1]['fit_last'] * 16 <= m.LDS_LIMIT
    assert m.gen_fits('f64', 10006) == dict(m=5003, radix=[5003], direct=True, lds=16 * 10006, twl=False, packed=True)
    assert m.gen_fits('f64', 67)['radix'] == [67] and m.gen_fits('f64', 134)['radix'] == [67] and m.gen_fits('f32', 67) is None
    assert m.gen_fits('f64', 2050)['radix'] == [5, 5, 41] and m.gen_fits('f64', 1200)['radix'] == [4, 2, 3, 5, 5]
    assert not m.engine_takes('f32', 1000, 1000) and not m.engine_takes('f32', 4, 4) and m.engine_takes('f32', 2, 2)
    assert m.engine_takes('f32', 15, 20) and not m.engine_takes('f32', 15, 20, inverse=True)
    assert m.gen_grid(5000, 15 * 24) == (2048, 8) and m.gen_grid(5000, 160 * 1024) == (256, 1) and m.gen_grid(7, 160 * 1024) == (7, 1)


# ---- 2. coverage -------------------------------------------------------------------------------------------------
TABLES = ((m.STFT_CASES, m.stft_branches), (m.ISTFT_CASES + m.OLA_CASES, m.istft_branches), (m.FB64_CASES, m.fb64_branches))


def test_every_branch_has_a_case():
    assert len(set(m.BRANCHES)) == len(m.BRANCHES)
    reached = {}
    for cases, fn in TABLES:
        assert len({c['id'] for c in cases}) == len(cases)
        for c in cases:
            for b in fn(c):
                assert b in m.BRANCHES, (c['id'], b)
                reached.setdefault(b, c['id'])
    missing = [b for b in m.BRANCHES if b not in reached and b not in m.EXCLUDED]
    assert not missing, missing
    assert not [b for b in m.EXCLUDED if b in reached]


def test_the_cases_are_as_small_as_the_issue_asks():
    for c in m.STFT_CASES:
        if c.get('stride'):
            continue
        frames = m.frames_of(c)
        assert c['B'] * c['C'] <= 4 and frames * c['n_fft'] <= max(4 * c['n_fft'], 3000) and (c['n_fft'] <= 4096 or frames <= 4), c['id']
    for c in m.ISTFT_CASES:
        assert c['B'] * c['C'] <= 4 and c['F'] * c['n_fft'] <= max(3 * c['n_fft'], 300) and (c['n_fft'] <= 4096 or c['F'] <= 4), c['id']
    stride = {c['id']: c for c in m.STFT_CASES + m.OLA_CASES if c.get('stride')}
    assert m.frames_of(stride['f64 stride 15/4']) * 2 > 2048 and m.frames_of(stride['f32 stride 10240']) > 256
    assert m.gen_fits('f32', 10240)['lds'] > 80 * 1024 and m.gen_fits('f64', 5120)['lds'] > 80 * 1024
    assert stride['f64 ola stride']['F'] == 263000


# ---- 3. the emulations against numpy.fft in longdouble --------------------------------------------------------------
def worst(err, bound, use=None):
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    frac = np.nan_to_num(frac, nan=np.inf)
    if use is not None:
        frac = frac[use]
    return float(frac.max()) if frac.size else 0.0


def stft_frac(c, mutant=None):
    c = m.shortened(c)
    x, window = m.stft_input(c), m.hann(c['win'], c['ty'])
    got = m.from_layout(m.emulate_stft(c, m.to_layout(x, c['in_fmt']), window, mutant), c['out_fmt'])
    want, s = m.ref_stft(c, x, window)
    assert got.shape == want.shape
    err, use = m.stft_error(c, got, want)
    if c['mode'] == m.PHASE:
        assert 1.0 - use.mean() <= m.PHASE_LEFT_OUT
    return worst(err, m.stft_bound(c, want, s), use)


def istft_frac(c, mutant=None):
    c = m.shortened(c)
    spec, synth = m.istft_input(c), m.synth_window(c)
    got = m.from_layout(m.emulate_istft(c, m.to_layout(spec, c['spec_fmt']), synth, mutant), c['wave_fmt'])
    want, bound = m.ref_istft(c, spec, synth)
    assert got.shape == want.shape
    return worst(np.abs(got.astype(np.longdouble) - want).astype(np.float64), bound)


def fb64_frac(c):
    c = m.shortened(c)
    x, fb = m.fb64_input(c)
    got = m.from_layout(m.emulate_fb64(c, m.to_layout(x, c['fmt']), fb), c['fmt'])
    want, bound = m.ref_fb64(c, x, fb)
    return worst(np.abs(got.astype(np.longdouble) - want).astype(np.float64), bound)


needs_longdouble = pytest.mark.skipif(not HAVE_LONGDOUBLE, reason='numpy longdouble is no wider than float64 here')


@needs_longdouble
@pytest.mark.parametrize('ty', list(m.DT))
def test_forward_emulation_is_within_its_bound_on_every_case(ty):
    """also: the float64 emulation EQUALS the longdouble rfft to float64 round-off -- a bound of a few thousand u is met with an
    error of a few u, so the share of the bound is small (the issue measured 0.08 against its own, tighter constant)"""
    for c in m.STFT_CASES:
        if c['ty'] == ty and not c.get('refused'):
            frac = stft_frac(c)
            assert frac <= 0.25, (c['id'], frac)


@needs_longdouble
@pytest.mark.parametrize('ty', list(m.DT))
def test_inverse_emulation_is_within_its_bound_on_every_case(ty):
    for c in m.ISTFT_CASES + m.OLA_CASES:
        if c['ty'] == ty:
            frac = istft_frac(c)
            assert frac <= 0.25, (c['id'], frac)


@needs_longdouble
def test_filterbank_emulation_is_within_its_bound_on_every_case():
    for c in m.FB64_CASES:
        assert fb64_frac(c) <= 1.0, c["id"]


def test_refused_cases_are_refused_by_the_model():
    refused = [c for c in m.STFT_CASES if c.get('refused')]
    assert sorted(c['n_fft'] for c in refused) == [5121, 10242] and all(c['ty'] == 'f64' for c in refused)
    for c in refused:
        assert m.gen_fits('f64', c['n_fft']) is None and m.gen_fits('f64', c['n_fft'] - 2) is not None


# ---- 4. mutants ----------------------------------------------------------------------------------------------------
def killed(fn, c, mutant):
    try:
        return fn(c, mutant) > 1.0
    except m.OutOfBounds:
        return True


@needs_longdouble
@pytest.mark.parametrize('mutant', list(m.MUTANTS))
def test_every_mutant_is_killed_by_a_case_of_the_table(mutant):
    """small cases only (n_fft <= 2100, no direct DFT of thousands of points): a mutant a small case cannot tell is not covered"""
    _, where = m.MUTANTS[mutant]
    kills = []
    for ty in m.DT:
        if ty == 'f32' and mutant in m.F64_ONLY_MUTANTS:
            continue
        if 'stft' in where:
            kills += [c['id'] for c in m.STFT_CASES if c['ty'] == ty and c['n_fft'] <= 2100 and not c.get('refused') and killed(stft_frac, c, mutant)]
        if 'istft' in where:
            kills += [c['id'] for c in m.ISTFT_CASES + m.OLA_CASES if c['ty'] == ty and c['n_fft'] <= 2100 and killed(istft_frac, c, mutant)]
        assert [k for k in kills if k.startswith(ty)], (mutant, ty)
    print('%s (%s): killed by %s' % (mutant, m.MUTANTS[mutant][0], ', '.join(kills)))


def test_the_mutant_list_has_what_the_issue_names():
    assert set(m.MUTANTS) >= {'idx_mod', 'mask_r', 'clamp_R', 'store_mask', 'k_eq_M', 'inv_conj', 'dcnyq_imag', 'inv_m', 'win_mask',
                              'zero_tail', 'f_lo', 'tws1'}


# ---- 5. the float-reciprocal divisions -------------------------------------------------------------------------------
def test_float_reciprocal_division_is_exact_for_every_pair_the_cases_form():
    """gen_pass: o / (ns R) for o < N and rem / ns for rem < ns R; gen_pass_bf: j / ns for j < N / R -- for every pass of every plan
    in the tables (tests/test_proto_generic.py stops at the divisors up to 4096 and five more)"""
    pairs = set()
    for c in m.STFT_CASES + m.ISTFT_CASES + m.OLA_CASES:
        pl = m.gen_fits(c['ty'], c['n_fft'])
        if pl is None:
            continue
        ns = 1
        for r in pl['radix']:
            if r in (2, 3, 4, 5):
                pairs.add((pl['m'] // r, ns))
            else:
                pairs |= {(pl['m'], ns * r), (ns * r, ns)}
            ns *= r
    assert max(d for _, d in pairs) > 4096 + 1000 and len(pairs) > 60      # beyond the list of tests/test_proto_generic.py
    for n, d in sorted(pairs):
        o = np.arange(n)
        assert (pg.float_div(o, d) == o // d).all(), (n, d)
