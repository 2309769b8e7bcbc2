"""The forward gate's checker is itself checked (no GPU): tests/signal_model.py restates the dispatch of k_frame, k_energy, k_delta
and k_thin_gemm, so (1) its constants must be the ones in the source text, (2) its case tables must reach every branch it names,
(3) its index-level emulations must equal the oracle (oracle/kapre_oracle.py) on every case and (4) each emulation with one wrong
line must differ from the oracle on at least one case -- else the table could not tell that kernel bug either.
"""
import os
import re

import numpy as np
import pytest

import kapre_oracle as o
import signal_model as m

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'kapre_amd', 'csrc')


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
    kern, mel = source('kpr_signal_kernels.h'), source('kpr_host_mel.h')
    hip = source('kpr_host_ops.h') + mel                 # the Frame / Energy / Delta bodies, the thin-GEMM launch
    assert int(one(r'constexpr int kEnFrames = (\d+);', kern)) == m.EN_FRAMES
    assert product(one(r'i0 < n4; i0 \+= (\d+ \* \d+)\)', kern)) == m.EN_UNROLL
    unroll = int(one(r'f32x4 v\[(\d+)\];', kern))
    assert unroll * m.BLOCK == m.EN_UNROLL and kern.count('k < %d; ++k' % unroll) == 2
    assert kern.count('__launch_bounds__(256)') == 4
    # the grid caps
    assert 1 << int(one(r'k_frame<v>, dim3\(grid_1d\(work, 256, 1 << (\d+)\)\), dim3\(256\)', hip)) == m.GRID_CAP
    assert 1 << int(one(r'k_delta<v>, dim3\(grid_1d\(a\.total / v, 256, 1 << (\d+)\)\), dim3\(256\)', hip)) == m.GRID_CAP
    assert 1 << int(one(r'k_energy, dim3\(\(unsigned\)std::min<long long>\(a\.n_sig \* chunks, 1 << (\d+)\)\), dim3\(256\)', hip)) == m.GRID_CAP
    assert product(one(r'std::min<long long>\(\(rows \+ 63\) / 64, (\d+ \* \d+)\)', hip)) == m.THIN_GRID_CAP
    # the 64 KiB a launch gets without opting in: where the thin GEMM opts in, k_energy's refusal, k_energy's part_words
    assert [product(e) for e in re.findall(r'lds (?:\+ sizeof\(float\) \* pw <=|>) (\d+ \* \d+)\)', hip)] == [m.LDS_PLAIN] * 3
    assert 'size_t lds = sizeof(float) * 2 * (size_t)(kEnFrames + q + 1);' in hip
    assert 'const size_t pw = (size_t)(kEnFrames + q + 1) * (hop_length / 4);' in hip
    # thin_gemm_shape and the thin launch
    tiles, kmax, kmask = one(r'thin_gemm_shape\(int n_freq, int n_filt\) \{ return \(n_filt \+ 15\) / 16 <= (\d+) && n_freq <= (\d+) && '
                             r'\(n_freq & (\d+)\) == 0; \}', mel)
    assert (int(tiles), int(kmax), int(kmask)) == (m.THIN_MAX_TILES, m.THIN_MAX_K, 3)
    assert 'const size_t lds = sizeof(float) * 4 * 64 * (size_t)ntiles * ((n_freq + 15) / 16);' in hip
    assert 'if (contiguous && thin_gemm_shape(n_freq, n_filt) && (((uintptr_t)x) & 15) == 0) {' in hip


def thin_launch_opts_in(hip):
    """the k_thin_gemm launch sets hipFuncAttributeMaxDynamicSharedMemorySize (allow_big_lds) for what it launches"""
    return re.search(r'allow_big_lds\(\w+, reinterpret_cast<const void\*>\(&k_thin_gemm<\w+>\)\)', hip) is not None


def test_thin_gemm_cases_above_64_kib_agree_with_the_dispatch():
    """thin_gemm_shape admits 4 tiles x 32 k-groups = 128 KiB of B fragments; a launch above 64 KiB of dynamic LDS fails unless the
    kernel opted in.  The model calls those cases thin: the launch must go through allow_big_lds."""
    big = [c for c in m.THIN_CASES if m.thin_plan(c)['lds'] > m.LDS_PLAIN and 'thin.lds>64K' in m.thin_branches(c)]
    assert {(c['K'], c['N']) for c in big} >= {(272, 64), (512, 33), (512, 64)}
    assert m.thin_plan(m.tcase(256, 64, 64))['lds'] == m.LDS_PLAIN
    assert m.thin_plan(m.tcase(512, 64, 64))['lds'] == 128 * 1024 <= 160 * 1024
    opts_in = thin_launch_opts_in(source('kpr_host_mel.h'))
    assert opts_in == m.THIN_BIG_LDS_OPT_IN
    for c in big:
        assert opts_in, '%s: %d bytes of dynamic LDS and no opt-in at the launch' % (c['id'], m.thin_plan(c)['lds'])
    assert 'hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024' in source('kpr_host.h')


# ---- 2. coverage -------------------------------------------------------------------------------------------------
TABLES = {'frame': (m.FRAME_CASES, m.frame_branches), 'energy': (m.ENERGY_CASES + [m.ENERGY_REFUSED], m.energy_branches),
          'delta': (m.DELTA_CASES, m.delta_branches), 'thin': (m.THIN_CASES, m.thin_branches)}


def test_every_branch_has_a_case():
    assert len(set(m.BRANCHES)) == len(m.BRANCHES)
    assert m.EXCLUDED == ('frame.index64',)
    reached = {}
    for kernel, (cases, fn) in TABLES.items():
        assert len({c['id'] for c in cases}) == len(cases), kernel
        for c in cases:
            for b in fn(c):
                assert b in m.BRANCHES, (c['id'], b)
                assert b.split('.')[0] == ('thin' if kernel == 'thin' and b.startswith('gemm') else kernel) or b.startswith('gemm')
                reached.setdefault(b, c['id'])
    missing = [b for b in m.BRANCHES if b not in reached and b not in m.EXCLUDED]
    assert not missing, missing
    assert not [b for b in m.EXCLUDED if b in reached]


def test_the_cases_the_issue_names_take_the_path_it_says():
    en = {c['id']: m.energy_branches(c) for c in m.ENERGY_CASES}
    assert {'energy.stream', 'energy.stream.passes>=3', 'energy.chunks>=2', 'energy.chunk.partial', 'energy.stream.ragged'} <= en['2048/512/70f']
    assert 'energy.stream.passes>=2' in en['256/256/70f'] and 'energy.stream.passes>=3' not in en['256/256/70f']
    assert 'energy.stream.passes>=2' not in en['8/4/64']
    assert 'energy.stream.padend' in en['8/8/64 pad']
    assert {'energy.general', 'energy.general.T%4', 'energy.general.pastend'} <= en['8/4/62 pad']
    assert en['1024/1024/8f'] >= {'energy.general', 'energy.general.nolds'}
    assert 'energy.general.q0' in en['5/8/50'] and 'energy.general.hop%4' in en['10/3/50']
    assert en['8/4/64 misaligned'] >= {'energy.general.misaligned'} and en['10/8/64'] >= {'energy.general.r%4'}
    assert 'energy.wgstride' in en['stride 8/4/16']
    assert m.energy_branches(m.ENERGY_REFUSED) == {'energy.refused'}
    fr = {c['id']: m.frame_branches(c) for c in m.FRAME_CASES}
    assert fr['8/4/64'] >= {'frame.vec4.load16'} and 'frame.vec4.dwordload' not in fr['8/4/64']
    assert 'frame.vec4.mixed' in fr['8/3/64'] and 'frame.vec1' in fr['7/3/50']
    assert 'frame.vec4.straddle' in fr['8/4/21 pad'] and fr['8/4/5 T<L'] == {'frame.empty'}
    assert fr['8/4/64 misaligned'] >= {'frame.vec4.dwordload'} and 'frame.vec4.load16' not in fr['8/4/64 misaligned']
    assert fr['stride 7/3'] >= {'frame.gridstride', 'frame.vec1'}
    de = {c['id']: m.delta_branches(c) for c in m.DELTA_CASES}
    assert de['w101 symmetric T200 f256'] >= {'delta.interior.j0>4', 'delta.interior.clamp', 'delta.vec4'}
    assert 'delta.interior' not in de['w101 symmetric T100 f256'] and 'delta.interior' in de['w101 symmetric T101 f256']
    assert 'delta.mixedwave' in de['w9 reflect T200 f13'] and 'delta.mixedwave' not in de['w9 reflect T200 f256']
    assert 'delta.pad.wrap' in de['w101 reflect T2 f1'] and 'delta.T1' in de['w3 symmetric T1 f13']
    assert de['stride w5 constant'] >= {'delta.gridstride', 'delta.vec1'}
    assert 'delta.vec1.misaligned' in de['w5 reflect misaligned']
    assert {c['K'] for c in m.THIN_CASES} >= set(m.THIN_KS) and {c['N'] for c in m.THIN_CASES} >= set(m.THIN_NS)
    assert {c['rows'] for c in m.THIN_CASES} >= set(m.THIN_ROWS) | {m.THIN_ROWSTRIDE}
    labels = {c['id']: m.thin_label(c) for c in m.THIN_CASES}
    for cid in ('K10 N13 rows65', 'K516 N16 rows65', 'K40 N65 rows65', 'K40 N13 rows22 cl C3', 'K40 N13 rows65 misaligned'):
        assert labels[cid] == 'k_gemm', cid
    assert labels['K40 N13 rows65 cl C1'] == 'k_thin_gemm'


# ---- 3. the emulations are the oracle ----------------------------------------------------------------------------
FLOOR = 1e-3      # inputs are of order 1: an output that is zero but for the oracle's round-off (Delta with one frame) is compared on that scale


def same(got, want, what, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size:
        assert np.isfinite(got).all(), what
        err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), FLOOR)
        assert err <= tol, '%s: %.3g of the largest value' % (what, err)


def differs(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not want.size:
        return got.shape != want.shape
    bad = ~np.isfinite(got) | (np.abs(got - want) > 1e-9 * max(float(np.abs(want).max()), FLOOR))
    return bool(bad.any())


def frame_oracle(c, x):
    return o.kapre_frame(x, c['L'], c['hop'], c['pad_end'], c['pad_value'], c['fmt'])


def energy_oracle(c, x):
    return o.kapre_energy(x, c['sample_rate'], c['ref_duration'], c['L'], c['hop'], c['pad_end'], c['pad_value'], c['fmt'])


def delta_oracle(c, x):
    return o.kapre_delta(x, c['win'], c['mode'], c['fmt'])


def thin_inputs(c):
    rng = np.random.default_rng(m.seed_of(c))
    return rng.uniform(-1, 1, (c['rows'] * c['C'], c['K'])), rng.uniform(-1, 1, (c['K'], c['N']))


def test_frame_emulation_is_the_oracle():
    for c in map(m.shortened, m.FRAME_CASES):
        x = m.frame_input(c, np.float64)
        want = frame_oracle(c, x)
        got = m.emulate_frame(c, x)
        assert got.shape == want.shape, c['id']
        np.testing.assert_array_equal(got, want, err_msg=c['id'])


def test_energy_emulation_is_the_oracle():
    for c in map(m.shortened, m.ENERGY_CASES):
        x = m.frame_input(c, np.float64)
        same(m.emulate_energy(c, x), energy_oracle(c, x), c['id'])
        xe = m.energy_exact_input(c)
        same(m.energy_exact_expected(c, xe), energy_oracle(c, xe), c['id'] + ' (exact input)', tol=2.0 ** -22)


def test_delta_emulation_is_the_oracle():
    for c in map(m.shortened, m.DELTA_CASES):
        x = m.delta_input(c, np.float64)
        same(m.emulate_delta(c, x), delta_oracle(c, x), c['id'])
    for c in map(m.shortened, m.DELTA_CASES[::7]):
        xe = m.delta_exact_input(c)
        same(m.delta_exact_expected(c, xe), delta_oracle(c, xe), c['id'] + ' (exact input)', tol=2.0 ** -22)


def test_thin_gemm_emulation_is_the_matrix_product():
    for c in m.THIN_CASES:
        if not m.thin_plan(c)['thin']:
            continue
        a, b = thin_inputs(c)
        same(m.emulate_thin(c, a, b), a @ b, c['id'])


# ---- 4. one wrong line shows -------------------------------------------------------------------------------------
def noticed(cases, emulate, oracle, inputs, mutant):
    return [c['id'] for c in map(m.shortened, cases) for x in [inputs(c)] if differs(emulate(c, x, mutant), oracle(c, x))]


@pytest.mark.parametrize('mutant', m.FRAME_MUTANTS)
def test_frame_mutants_are_noticed(mutant):
    hit = noticed(m.FRAME_CASES, m.emulate_frame, frame_oracle, lambda c: m.frame_input(c, np.float64), mutant)
    assert hit, mutant
    assert all(cid.startswith('cl') for cid in hit)                         # only rows that span channels can tell


@pytest.mark.parametrize('mutant', m.ENERGY_MUTANTS)
def test_energy_mutants_are_noticed(mutant):
    hit = noticed(m.ENERGY_CASES, m.emulate_energy, energy_oracle, lambda c: m.frame_input(c, np.float64), mutant)
    assert hit, mutant
    paths = {('stream' if m.energy_plan(c)['stream'] else 'general') for c in m.ENERGY_CASES if c['id'] in hit}
    assert paths == {'stream', 'general'}, (mutant, hit)                    # noticed on both paths


def test_energy_partial_sums_past_the_signal_reach_no_output():
    """'streaming partials beyond n4v not zeroed' cannot be told from the kernel by any output: the streaming condition asks that no
    frame reaches past the signal, so no output adds a block sum that holds such a partial.  Asserted as that property: on every
    streaming case whose range is ragged, full[] changes and the output does not."""
    ragged = [c for c in map(m.shortened, m.ENERGY_CASES) if 'energy.stream.ragged' in m.energy_branches(c)]
    assert len(ragged) >= 5
    for c in ragged:
        x = m.frame_input(c, np.float64) + 2.0                              # no zero samples: a stale partial sum is not 0
        clean, stale = [], []
        want = m.emulate_energy(c, x, internals=clean)
        got = m.emulate_energy(c, x, 'stale_partials', internals=stale)
        assert any(differs(s, f) for s, f in zip(stale, clean)), c['id']
        np.testing.assert_array_equal(got, want, err_msg=c['id'])
    assert m.ENERGY_EQUIVALENT_MUTANTS == ('stale_partials',)


@pytest.mark.parametrize('mutant', m.DELTA_MUTANTS)
def test_delta_mutants_are_noticed(mutant):
    hit = noticed(m.DELTA_CASES, m.emulate_delta, delta_oracle, lambda c: m.delta_input(c, np.float64), mutant)
    assert hit, mutant
    if mutant == 'clamped_weight':                                          # only where (win - 1) / 2 is no multiple of four
        assert all(((c['win'] - 1) // 2) % 4 for c in m.DELTA_CASES if c['id'] in hit)


@pytest.mark.parametrize('mutant', m.THIN_MUTANTS)
def test_thin_gemm_mutants_are_noticed(mutant):
    thin = [c for c in m.THIN_CASES if m.thin_plan(c)['thin']]
    hit = [c['id'] for c in thin for a, b in [thin_inputs(c)] if differs(m.emulate_thin(c, a, b, mutant), a @ b)]
    assert hit, mutant
    if mutant == 'first_grid_pass_only':
        assert set(hit) == {c['id'] for c in thin if 'thin.rowstride' in m.thin_branches(c)}
    else:
        assert set(hit) == {c['id'] for c in thin if 'thin.k%16' in m.thin_branches(c)}


# ---- 5. exact inputs stay exact ----------------------------------------------------------------------------------
def test_exact_inputs_stay_below_two_to_the_24():
    """every float32 operation on the exact inputs is exact as long as every intermediate is an integer (Energy with pad_value 0.5:
    a multiple of 1/4) of magnitude below 2^24, whatever the order of the additions"""
    for c in m.ENERGY_CASES:
        assert m.energy_exact_magnitude(c) < 2 ** 24, c['id']
        assert float(c['pad_value']) * 2 == int(c['pad_value'] * 2) and abs(c['pad_value']) <= 15, c['id']
        assert int(np.abs(m.energy_exact_input(m.shortened(c))).max()) <= 15
    for c in m.DELTA_CASES:
        assert m.delta_exact_magnitude(c) < 2 ** 24, c['id']
    assert int(np.abs(m.delta_exact_input(m.DELTA_CASES[-5])).max()) <= 63
    for c in m.THIN_CASES:
        assert m.thin_exact_magnitude(c) < 2 ** 24, c['id']
    a, b = m.thin_exact_input(m.THIN_CASES[0])
    assert max(int(np.abs(a).max()), int(np.abs(b).max())) <= 7
