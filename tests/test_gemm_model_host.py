"""CPU only: tests/gemm_model.py against the source text and against itself.

  - the constants the model restates equal the text of kpr_misc_kernels.h / kpr_host.h / kpr_host_mel.h / kpr_mel_kernels.h
  - the case tables reach every id of BRANCHES outside EXCLUDED (the ids of POINTERS are cases of tests/signal_model.py that run on
    this kernel there)
  - the index-level emulation equals the plain float64 oracle of the same operation to 1e-12 on every case, with no load or store
    outside its buffer and no output element left unwritten
  - every one-line mutant of MUTANTS leaves that bound or forms an out-of-range index on some case, except those of EQUIVALENT, which
    change no output element of any case (asserted exactly so)
  - numpy's float32 product of the same float32 tables stays under REG / 2 against numpy's FFT on every DFT case, and inside the
    per-element bounds the GPU gate asserts: the limits are such that the reference alone satisfies them
"""
import os
import re

import numpy as np
import pytest

import gemm_model as m
import generic_model as gm
import signal_model as sm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'kapre_amd', 'csrc')
TOL = 1e-12


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_equal_the_source_text():
    misc, host, mel, melk, fft = src('kpr_misc_kernels.h'), src('kpr_host.h'), src('kpr_host_mel.h'), src('kpr_mel_kernels.h'), src('kpr_host_fft.h')
    assert 'constexpr int TM = %d, TN = %d, KC = %d,' % (m.TM, m.TN, m.KC) in misc
    assert 'enum { A_PLAIN = %d, A_CABS = %d, A_FRAME = %d, A_CPLX = %d };' % (m.A_PLAIN, m.A_CABS, m.A_FRAME, m.A_CPLX) in misc
    assert 'enum { E_PLAIN = %d, E_CPLX = %d, E_WINDOW = %d, E_DB = %d };' % (m.E_PLAIN, m.E_CPLX, m.E_WINDOW, m.E_DB) in misc
    assert 'dim3 grid((unsigned)((ga.in.rows + 63) / 64), (unsigned)((ga.N + 63) / 64));' in host
    assert 'static int grid_1d(long long n, int block, int cap = 256 * 16)' in host and m.GRID_1D_CAP == 256 * 16
    assert 'dim3(grid_1d(g.total_frames * (g.win - g.n_fft), 256))' in src('kpr_host_istft.h')
    assert 'constexpr int kMaxTiles = %d;' % m.MAX_TILES in melk and 'constexpr int kChunkRows = %d;' % m.CHUNK_ROWS in melk
    assert 'if ((M + 15) / 16 > kMaxTiles || K > %d)' % m.SCHED_MAX_ROWS in mel
    assert 'if (ntiles > kMaxTiles || n_freq > %d) fb_kranges_host = nullptr;' % m.SCHED_MAX_ROWS in mel
    # the lines the mutants change
    for line in ('const long long rc = g.ok ? r : 0;', 'const int kc = min(k, ga.Kdim - 1);', 'tc = min(max(t, 0LL), ga.T - 1);',
                 'return (kin && t >= 0 && t < ga.T) ? v : 0.0f;', 'g.t0 = r0 * ga.hop - ga.pad_left;', 'min(ng, ga.N - 1)',
                 'bv[i] = (kg < ga.Kdim && ng < ga.N) ? v : 0.0f;', 't < (col0 + TN) / 16 && t * 16 < ga.N; ++t', 'if (klo > khi) klo = khi;',
                 'for (int kc = klo; kc < khi; kc += KC)', 'if (r >= ga.out.rows) return;', '(long long)(kc >> 1) * ga.in.es) + (kc & 1)]',
                 'out[2 * (ob + (long long)(n >> 1) * ga.out.es) + (n & 1)] = v;', '(n < ga.win) ? v * ga.window[n] : 0.0f;',
                 'atomicMax(&ga.stats[2 * r2], enc_f(mx));'):
        assert line in misc, line
    for line in ('if (g.out_cl) { m.s2 = (long long)g.F * Q * g.C; m.s1 = 1; m.s0 = Q * g.C; m.es = g.C; }',
                 'else { m.s2 = (long long)g.C * g.F * Q; m.s1 = (long long)g.F * Q; m.s0 = Q; m.es = 1; }'):
        assert line in host, line
    assert 'if (g.in_cl) { ga.in.s2 = g.T * g.C; ga.in.s1 = 1; ga.t_es = g.C; }' in src('kpr_host_stft.h')
    assert 'ga.Kdim = 2 * g.K; ga.N = std::min(g.n_fft, g.win); ga.ldb = g.n_fft;' in src('kpr_host_istft.h')
    assert 'ga.in.s2 = (long long)n_freq * channels; ga.in.s1 = 0; ga.in.s0 = 1; ga.in.es = channels;' in mel
    assert 'lo &= ~7;' in mel and 'hi = std::min(cap, lo + need);' in mel
    assert '(2 * kn) % n_fft == 0 ? 0.0f : (float)(-std::sin(a));' in fft
    assert '(edge || (2 * kn) % n_fft == 0) ? 0.0f : (float)(-ck * std::sin(a));' in fft
    assert sorted(int(x) for x in re.findall(r'case (\d+): return f\(FftTag', fft)) == sorted(m.MR_SIZES)


def test_route_predicates():
    for n in (67, 71, 127, 1028, 2049):
        assert m.fft_family(n, n) == 'gemm'
    for n, win in ((6, 9), (67, 80), (400, 500), (6, 506)):
        assert m.fft_family(n, win) == 'gemm'
    assert m.fft_family(400, 400) == 'mr' and m.fft_family(1200, 1200) == 'gen' and m.fft_family(15, 15) == 'gen'
    assert all(m.mel_staged_gemm(c['n_fft']) for c in m.MEL_CASES) and not m.mel_staged_gemm(400) and not m.mel_staged_gemm(300)
    assert {m.mel_stage(c['n_fft']) for c in m.MEL_CASES} == {'gen', 'gemm'}
    assert m.sched_kranges(8, 1025, [(0, 8)] * 65) is None
    assert m.sched_kranges(601, 16, [(4, 40)]) == [(0, 64)] and m.sched_kranges(601, 16, [(596, 604)]) == [(576, 608)]
    assert m.sched_kranges(34, 16, [(12, 36)]) == [(8, 40)]                       # beyond Kdim = 34, inside the cap of 64


def test_the_pointers_name_cases_of_the_signal_gate_that_run_on_this_kernel():
    cases = {c['id']: c for c in sm.THIN_CASES}
    for bid, cid in m.POINTERS.items():
        assert bid in m.BRANCHES and sm.thin_label(cases[cid]) == 'k_gemm'


# ---------------------------------------------------------------------------------------------
# every case: emulation vs oracle, with or without a mutant.  The inputs and oracles are computed once.
# ---------------------------------------------------------------------------------------------
def _prepare():
    runs = []
    for c in m.FWD_CASES:
        x, w = m.stft_input(c), m.hann(c['win'])
        xin, table = m.to_layout(x, c['in_fmt']), m.build_dft_fwd(c['n_fft'])
        want = m.to_layout(m.oracle_stft(c, x, w, table), c['out_fmt'])
        runs.append(('fwd', c, want, lambda mut, c=c, xin=xin, w=w: m.emulate_stft(c, xin, w, mut)))
    for c in m.INV_CASES:
        spec, synth = m.istft_input(c), m.synth_window(c)
        sin, table = m.to_layout(spec, c['spec_fmt']), m.build_dft_inv(c['n_fft'])
        want = m.oracle_istft(c, spec, synth, table)
        runs.append(('inv', c, want, lambda mut, c=c, sin=sin, synth=synth: m.emulate_istft(c, sin, synth, mut)))
    for c in m.FB_CASES:
        x, fb = m.fb_input(c)
        xin = m.to_layout(x, c['fmt'])
        runs.append(('fb', c, m.oracle_fb(c, x, fb), lambda mut, c=c, xin=xin, fb=fb: m.emulate_fb(c, xin, fb, mut)))
    for c in m.MEL_CASES:
        x, w, fb = m.mel_input(c), m.hann(c['win']), m.mel_bank(c)
        spec = np.fft.rfft(m.stft_frames(c, x, w), n=c['n_fft'], axis=-1)
        for db in (None,) + m.DB_RUNS:
            want, st = m.oracle_mel(c, spec, fb, db)

            def run(mut, c=c, spec=spec, fb=fb, db=db, st=st):
                got, stats, tr = m.emulate_mel(c, spec, fb, db, mut)
                if db is not None:                   # the clamp reads the statistics: a wrong word shows in the output
                    if not np.allclose(stats, st, rtol=0, atol=1e-9):
                        tr.violations.append('statistics words are not the items\' maxima / minima')
                    got = m.db_clamp(got, stats[:, 0], db[2])
                return got, tr
            if db is not None:
                want = m.db_clamp(want, st[:, 0], db[2])
            runs.append(('mel', c, want, run))
    return runs


RUNS = _prepare()
CLEAN = {}


def outcome(run, mut=()):
    kind, c, want, fn = run
    got, tr = fn(frozenset(mut))
    assert got.shape == want.shape, (c['id'], got.shape, want.shape)
    with np.errstate(invalid='ignore'):
        err = np.abs(got - want)
    err = float(np.nan_to_num(err, nan=np.inf).max() / max(np.abs(want).max(), 1e-300)) if err.size else 0.0
    return got, err, tr


def clean(i):
    if i not in CLEAN:
        CLEAN[i] = outcome(RUNS[i])
    return CLEAN[i]


def test_the_emulation_equals_the_float64_oracle_on_every_case():
    for i, run in enumerate(RUNS):
        _, err, tr = clean(i)
        assert not tr.violations, (run[1]['id'], tr.violations[:3])
        assert err <= TOL, (run[1]['id'], err)


def test_the_case_tables_reach_every_branch():
    reached = set(m.POINTERS)
    for i in range(len(RUNS)):
        reached |= clean(i)[2].branches
    assert reached <= set(m.BRANCHES), sorted(reached - set(m.BRANCHES))
    assert reached >= set(m.BRANCHES) - set(m.EXCLUDED), sorted(set(m.BRANCHES) - set(m.EXCLUDED) - reached)
    assert not reached & set(m.EXCLUDED)


def applies(mut, kind):
    return {'t>=0': 'fwd', 't<T': 'fwd', 'pad_sign': 'fwd', 't_es1': 'fwd', 'ecplx.n': 'fwd', 'cplx.swap': 'inv', 'ewin': 'inv',
            'inv.edge': 'inv', 'stats.q': 'mel'}.get(mut, kind) == kind


@pytest.mark.parametrize('mut', sorted(m.MUTANTS))
def test_mutant(mut):
    killed, moved = [], []
    for i, run in enumerate(RUNS):
        if not applies(mut, run[0]):
            continue
        got, err, tr = outcome(run, (mut,))
        if tr.violations or err > TOL:
            killed.append(run[1]['id'])
        if tr.violations or not np.array_equal(got, clean(i)[0]):
            moved.append(run[1]['id'])
        if killed and mut not in m.EQUIVALENT:
            break
    if mut in m.EQUIVALENT:
        assert not moved, '%s (%s) changed an output of %s' % (mut, m.EQUIVALENT[mut], moved)
    else:
        assert killed, '%s (%s) survives every case' % (mut, m.MUTANTS[mut])


def test_equivalent_mutants_are_mutants():
    assert set(m.EQUIVALENT) <= set(m.MUTANTS)


# ---------------------------------------------------------------------------------------------
# what the reference alone achieves
# ---------------------------------------------------------------------------------------------
def test_float32_numpy_products_meet_the_limits_the_gate_asserts():
    worst = {}
    for c in m.FWD_CASES:
        x, w, table = m.stft_input(c), m.hann(c['win']), m.build_dft_fwd(c['n_fft'])
        want, _ = gm.ref_stft(c, x, w)
        err = np.abs(m.parts(m.stft_f32_product(c, x, w, table)).astype(np.float64) - m.parts(want).astype(np.float64))
        frac = m.fraction(err, m.stft_bound(c, x, w, table))
        ratio = float(err.max() / np.abs(want).max())
        worst['fwd'] = max(worst.get('fwd', (0, 0)), (frac, ratio))
        assert frac <= 1.0 and ratio <= m.REG / 2, (c['id'], frac, ratio)
    for c in m.INV_CASES:
        spec, synth, table = m.istft_input(c), m.synth_window(c), m.build_dft_inv(c['n_fft'])
        want, bound = m.ref_istft(c, spec, synth, table)
        err = np.abs(m.istft_f32_product(c, spec, synth, table).astype(np.float64) - want.astype(np.float64))
        frac = m.fraction(err, bound)
        ratio = float(err.max() / np.abs(want).max())
        worst['inv'] = max(worst.get('inv', (0, 0)), (frac, ratio))
        assert frac <= 1.0 and ratio <= m.REG / 2, (c['id'], frac, ratio)
    print('float32 numpy products: worst (error / bound, max error / max) forward %s, inverse %s' % (worst['fwd'], worst['inv']))


def test_the_nyquist_column_of_the_table():
    """real input: the float64 product with the table gives exact zeros in the imaginary parts of DC and Nyquist; with the table as it
    was ((float)(-sin(pi)) = -1.22e-16 in the Nyquist column of every odd row) it does not"""
    c = {x['id']: x for x in m.FWD_CASES}[m.NYQUIST_CASE]
    x, w = m.stft_input(c), m.hann(c['win'])
    new, old = m.build_dft_fwd(c['n_fft']), m.build_dft_fwd(c['n_fft'], exact_zeros=False)
    assert np.count_nonzero(new[:, 1]) == 0 and np.count_nonzero(new[:, -1]) == 0 and np.count_nonzero(old[:, -1]) == c['n_fft'] // 2
    diff = np.flatnonzero((new != old).any(0))
    assert np.all(diff % 2 == 1) and np.all(np.abs(old[new != old]) <= 2.0 ** -52)          # sine entries under 2.3e-16 only
    z = m.oracle_stft(c, x, w, new)
    assert np.all(z.imag[..., 0] == 0) and np.all(z.imag[..., -1] == 0)
    zo = m.oracle_stft(c, x, w, old)
    assert 0 < np.abs(zo.imag[..., -1]).max() <= m.TABLE_ABS * np.abs(m.stft_frames(c, x, w)).sum(-1).max()
    inv_new, inv_old = m.build_dft_inv(c['n_fft']), m.build_dft_inv(c['n_fft'], exact_zeros=False)
    assert np.all(np.abs(inv_old[inv_new != inv_old]) <= 2.0 ** -52 * 2 / c['n_fft'])
