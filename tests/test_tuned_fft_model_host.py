"""The tuned-transform gate's checker is itself checked (no GPU): tests/tuned_fft_model.py restates the routes and the code around the
transform cores of k_stft_mr / k_stft_bs / k_stft_big and k_irfft_mr / k_irfft_bs / k_irfft_big / k_irfft, so (1) its constants and the
lines its mutants change must be the ones in the source text, (2) bin over holds must be a bijection for all 18 plans, (3) its tables
must agree with longdouble, (4) its case tables must reach every id outside EXCLUDED, at 64, 256 and 304 compute units for the
multi-trip cases, (5) its emulations must agree with numpy's longdouble rfft / irfft + overlap-add within 1e-12 on every case, (6) every
one-line mutant must be told from the reference by a named case, or change no output for a reason that is written down, and (7) the
reference alone must leave few enough phase bins out.
"""
import os
import re

import numpy as np
import pytest

import generic_model as gm
import tuned_fft_model as m

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'kapre_amd', 'csrc')
AGREE = 1e-12
HOST_CUS = 2                      # the emulations run the table cases as a device with two compute units would


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


# ---- 1. constants and mutated lines ----------------------------------------------------------------------------------
def test_constants_are_the_ones_in_the_source():
    fft, mr, host, hfft = source('kpr_fft.h'), source('kpr_fft_mr.h'), source('kpr_host.h'), source('kpr_host_fft.h')
    assert int(one(r'constexpr int kPts = (\d+);', fft)) == m.K_PTS
    assert int(one(r'constexpr int kMrP = (\d+);', mr)) == m.MR_P
    assert 'return n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048;' in hfft and m.FAST == (256, 512, 1024, 2048)
    assert 'static bool big_nfft(int n_fft) { return n_fft == 4096 || n_fft == 8192; }' in hfft and m.BIG == {4096: 2, 8192: 4}
    assert 'int m = 128;\n    while (m < 2 * ncr - 1) m *= 2;\n    return m <= 1024 ? m : 0;' in hfft
    assert 'return !fast_nfft(s->n_fft) && bluestein_m(s->n_fft) > 0 && s->win_length <= s->n_fft;' in hfft
    assert 'if (bluestein_ok(s)) return mixed_radix_plan(s->n_fft) && opt(OPT_MIXED_RADIX) ? FAM_MR : FAM_BS;' in hfft
    assert hfft.index('if (fast_nfft(s->n_fft)) return FAM_POW2;') < hfft.index('if (bluestein_ok(s))') < hfft.index('if (big_nfft(s->n_fft)) return FAM_BIG;')
    # the 18 typedefs and the switch that selects them
    mrs = {int(n): (int(a), int(b)) for a, b, n in re.findall(r'typedef MrFft<(\d+), (\d+)> Fft(\d+);', hfft)}
    tps = {int(n): (int(a), int(b)) for a, b, n in re.findall(r'typedef TwoPassFft<(\d+), (\d+)> Fft(\d+);', hfft)}
    assert mrs == m.MR_TYPEDEFS and tps == m.TP_TYPEDEFS and len(m.PLANS) == 18
    assert {int(n) for n in re.findall(r'case (\d+): return f\(FftTag<Fft\1>\{\}\);', hfft)} == set(m.PLANS)
    # the members of the two plan templates
    assert 'static constexpr int P = kMrP, L = R2 * R3, N = P * L, Q2 = P / R2, Q3 = P / R3;' in mr
    assert 'static constexpr int RL = (R3 > 1) ? R3 : R2;' in mr and 'static constexpr int PIN = P, LIN = L, ROW = N;' in mr
    assert 'static KPR_DEV int bin(int l, int reg) { return l + L * (reg / RL) + (N / RL) * (reg % RL); }' in mr
    assert 'static constexpr int N = N1 * N2, P = (N1 > N2) ? N1 : N2, L = P;' in mr
    assert 'static constexpr int PIN = N1, LIN = N2, ROW = N2P * N1;' in mr and 'static constexpr int N2P = N2 | 1;' in mr
    assert 'static KPR_DEV int bin(int l, int reg) { return l + N1 * reg; }' in mr
    assert 'static KPR_DEV bool holds(int l, int reg) { return l < N1 && reg < N2; }' in mr
    # the composite register DFTs the bound counts stages of
    comp = {int(n): (int(a), int(b)) for n, a, b in re.findall(r'template <> struct Dft<(\d+)> \{ static KPR_DEV void run\(f2 \(&v\)\[\d+\]\) \{ dft_ab<(\d+), (\d+)>\(v\); \} \};', mr)}
    assert comp == {6: (2, 3), 10: (2, 5), 12: (4, 3), 15: (3, 5), 20: (4, 5), 24: (8, 3)}
    assert all(m.STAGES[n] == m.STAGES[a] + m.STAGES[b] for n, (a, b) in comp.items()) and m.STAGES[16] == (4, 4)
    stft = source('kpr_stft_kernels.h')
    assert 'return ((F::ROW > F::N + 1) ? F::ROW : F::N + 1) | 1; }' in stft
    assert 'return (M + M / 32 + 24 + 3) / 4 * 4 + 2 * ncr + 2 * (ncr + 1) + 2;' in stft
    assert 'return sizeof(float) * 2 * ((size_t)4 * G * mr_row_stride<FF>() + 3 * (size_t)FF::N);' in hfft
    # launch_framewise and every launcher's per_block, per_cu, threads
    assert 'per_cu = std::max(1, std::min(per_cu, (int)(160 * 1024 / lds)));' in host
    assert 'std::min<long long>((groups + per_block - 1) / per_block, (long long)per_cu * cus));' in host
    hs, hi = source('kpr_host_stft.h'), source('kpr_host_istft.h')
    assert 'launch_framewise(&k_stft_big<R>, &lds_opt_in, g.total_frames, NW, 2, 64 * NW, lds, st, "k_stft_big", 0,' in hs
    assert 'const size_t lds = sizeof(float) * 2 * (size_t)NW * (R * 1024 + 1);' in hs
    assert 'launch_framewise(&k_stft_bs<M>, &lds_opt_in, ngroups, 4, 2, 256, lds, st, "k_stft_bs", 0,' in hs
    assert 'sizeof(float) * ((size_t)4 * G * bs_slot_words(M, g.n_fft / 2) + 2 * (size_t)(3 * M + g.n_fft / 2 + 2));' in hs
    assert 'launch_framewise(&k_stft_mr<FF>, &lds_opt_in, ngroups, 4, 3 /*' in hs and '"k_stft_mr", FF::N, x, g, window, tw, mode, out, ngroups);' in hs
    assert 'launch_framewise(&k_irfft_big<R>, &lds_opt_in, g.total_frames, NW, 1 /* 128 KiB of LDS */, 64 * NW, lds, st, "k_irfft_big", 0,' in hi
    assert 'const size_t lds = sizeof(float) * 2 * (size_t)(2 * NW) * (R * 1024 + 1);' in hi
    assert 'launch_framewise(&k_irfft_bs<M>, nullptr, ngroups, 4, 2, 256, lds, st, "k_irfft_bs", 0,' in hi
    assert 'launch_framewise(&k_irfft_mr<FF>, &lds_opt_in, ngroups, 4, 2, 256, lds, st, "k_irfft_mr", 0,' in hi
    assert 'launch_framewise(&k_irfft<NC>, nullptr, nblocks, 1, 2, 256, lds, st, "k_irfft", 0,' in hi
    assert 'const size_t lds = sizeof(float) * (4 * G * NC + 4 * G * (2 * NC + 8));' in hi
    assert 'const long long nblocks = (g.total_frames + 4 * G - 1) / (4 * G);' in hi
    assert hs.count('constexpr int NW = (R == 2) ? 4 : 2;') == 1 and hi.count('constexpr int NW = (R == 2) ? 4 : 2;') == 1


MUTATED_LINES = {
    # mutant: (file, the line it changes)
    'li_clamp': ('kpr_stft_kernels.h', 'const int li = min(l, LIN - 1);'),
    'has_in': ('kpr_stft_kernels.h', 'const bool has_in = active && l < LIN;'),
    'win_pair': ('kpr_common.h', 'winl[i] = f2{(n < win) ? scale_even * a : 0.0f, (n + 1 < win) ? scale_odd * b : 0.0f};'),
    'lower_bound': ('kpr_stft_kernels.h', 'vm |= (valid_ && n_ < g.win && (unsigned)o0_ <= (unsigned)omax_) ? (1ull << (2 * m)) : 0ull;'),
    'ob_wrong_trip': ('kpr_stft_kernels.h', 'const long long ob = ob_next;'),
    'o_skip': ('kpr_stft_kernels.h', 'if (o < 0) continue;'),
    'readlane': ('kpr_stft_kernels.h', '(unsigned)__builtin_amdgcn_readlane((int)ob_lo, gq * L));'),
    'nyq_guard': ('kpr_stft_kernels.h', 'if (2 * k != N) row[N - k] = xq;'),
    'dc_imag': ('kpr_stft_kernels.h', 'if (k == 0) { xk.y = 0.0f; xq.y = 0.0f; }'),
    'k_le_ncr': ('kpr_stft_kernels.h', 'if (k <= ncr) {'),
    'ostride1': ('kpr_common.h', 'KPR_DEV int spec_stride(const Geom& g) { return g.out_cl ? g.C : 1; }'),
    'gather': ('kpr_stft_kernels.h', 'const int n = r + R * (fl + L * m);'),
    'phase_zero': ('kpr_stft_kernels.h', 'KPR_DEV float bin_phase(f2 v) { return atan2f(v.y, v.x + 0.0f); }'),
    'inv_dcnyq': ('kpr_istft_kernels.h', 'if (k == 0) { a.y = 0.0f; b.y = 0.0f; }'),
    'inv_tail': ('kpr_istft_kernels.h', 'for (int n = 2 * NB + lane; n < g.win; n += 64) fo[n] = 0.0f;'),
    'inv_store': ('kpr_istft_kernels.h', 'if (2 * n + 1 < g.win) fo[2 * n + 1] = -z[r].y * w.y;'),
}


def test_the_mutated_lines_are_in_the_source():
    assert set(MUTATED_LINES) == set(m.FWD_MUTANTS) | set(m.INV_MUTANTS)
    for name, (fname, line) in MUTATED_LINES.items():
        assert line in source(fname), name
    ist = source('kpr_istft_kernels.h')
    # the same lines in the sibling kernels the inverse emulation stands for
    assert ist.count('if (2 * n + 1 < g.win) fo[2 * n + 1]') == 3 and ist.count('if (n + 1 < g.win) fo[n + 1]') == 1
    assert ist.count('if (k == 0) { a.y = 0.0f; b.y = 0.0f; }') >= 3 and 'if (kc == 0) { a.y = 0.0f; b.y = 0.0f; }' in ist
    assert 'if (k == 0) { xk.y = 0.0f; xq.y = 0.0f; }' in ist
    assert 'for (int n = 2 * NC + fl; n < g.win; n += L) fo[n] = 0.0f;' in ist
    # the three tuned forward kernels take their phase from bin_phase
    stft = source('kpr_stft_kernels.h')
    tuned = stft[stft.index('KPR_DEV float bin_phase'):]
    assert tuned.count(': bin_phase(') == 3 and tuned.count('atan2f(') == 1


# ---- 2. the plans ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_fft', sorted(m.PLANS))
def test_bin_over_holds_is_a_bijection(n_fft):
    pl = m.PLANS[n_fft]
    assert pl.N == n_fft // 2 and pl.L * pl.G <= 64 and pl.PIN * pl.LIN == pl.N and pl.LIN <= pl.L and pl.PIN <= pl.P
    l, r = np.meshgrid(np.arange(pl.L), np.arange(pl.P), indexing='ij')
    bins = pl.bin(l, r)[pl.holds(l, r)]
    assert sorted(bins.tolist()) == list(range(pl.N))
    assert pl.row_stride() >= pl.N + 1 and pl.row_stride() >= pl.ROW and pl.row_stride() & 1
    assert pl.lds_bytes() <= m.LDS_LIMIT
    prod = 1
    for s in pl.stages:
        prod *= s
    assert prod == pl.N


def test_routes():
    assert [m.bluestein_m(n) for n in (2, 4, 6, 126, 128, 130, 254, 258, 510, 514, 1022, 1024, 1026, 401)] == \
        [0, 128, 128, 128, 128, 256, 256, 512, 512, 1024, 1024, 1024, 0, 0]
    for n in (4, 8, 16, 32, 64, 128):                       # the powers of two below 256 are no "fast" sizes: Bluestein
        assert m.fft_family(n, n) == m.FAM_BS
    assert m.fft_family(400, 400) == m.FAM_MR and m.fft_family(400, 400, mixed_radix=0) == m.FAM_BS
    assert m.fft_family(4096, 5000) == m.FAM_BIG and m.fft_family(512, 600) == m.FAM_POW2
    # the zero-tail loops of k_irfft_mr / k_irfft_bs are unreachable (EXCLUDED): win_length > n_fft leaves both families
    for n in list(m.PLANS) + [4, 6, 126, 300, 1022]:
        c = m.icase('x', n, win=n + 1)
        assert m.inverse_family(c) == m.FAM_OTHER and m.inverse_launches(c, 256) == 'k_gemm + k_fill_cols + k_ola', n
        assert m.forward_family(m.fcase('x', n, win=n + 1)) in (m.FAM_MR, m.FAM_BS)           # forward_geom crops first
    assert m.launch_of('k_stft_mr', 400, 10 ** 9, 256)['grid'] == 3 * 256 and m.launch_of('k_stft_mr', 400, 10, 256)['grid'] == 1
    assert m.launch_of('k_stft_big', 8192, 10 ** 9, 256)['grid'] == 2 * 256 and m.launch_of('k_irfft_big', 4096, 10 ** 9, 256)['grid'] == 256
    assert m.launch_of('k_stft_mr', 160, 10 ** 9, 256)['label'] == 'k_stft_mr<80>'


# ---- 3. tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_fft', [4, 6, 126, 130, 400, 1022])
def test_the_tables_agree_with_longdouble(n_fft):
    pi = m.LD('3.14159265358979323846264338327950288')
    j = np.arange(n_fft).astype(m.LD)
    tw = m.build_twiddles(n_fft)
    assert np.abs(tw - np.exp(-2j * pi * j / n_fft)).max() <= 2.0 ** -24
    w, bt, t = m.build_bluestein(n_fft)
    ncr, mm = n_fft // 2, m.bluestein_m(n_fft)
    n = np.arange(ncr)
    chirp = np.exp(-1j * pi * ((n * n) % (2 * ncr)).astype(m.LD) / ncr)
    assert np.abs(w[:ncr] - chirp).max() <= 2.0 ** -24 and not w[ncr:].any()
    b = np.zeros(mm, np.clongdouble)
    b[:ncr] = np.conj(chirp)
    b[mm - n[1:]] = np.conj(chirp[1:])
    want = np.fft.fft(b) / (2 * mm)
    assert np.abs(bt - want).max() <= 2.0 ** -24 * max(1.0, float(np.abs(want).max()))
    assert np.abs(t - np.exp(-2j * pi * np.arange(ncr + 1).astype(m.LD) / n_fft)).max() <= 2.0 ** -24


# ---- 4. coverage -----------------------------------------------------------------------------------------------------
def run_fwd(c, cus, mutant=None):
    x, w = m.fwd_input(c), m.fwd_window(c)
    ids = set()
    got = gm.from_layout(m.emulate_stft(c, gm.to_layout(x, c['in_fmt']), w, cus, mutant, ids), c['out_fmt'])
    return got, ids | m.static_fwd_ids(c), x, w


def run_inv(c, cus, mutant=None):
    sp, w = m.inv_input(c), m.inv_window(c)
    ids = set()
    got = gm.from_layout(m.emulate_istft(c, gm.to_layout(sp, c['spec_fmt']), w, cus, mutant, ids), c['wave_fmt'])
    return got, ids, sp, w


def fwd_err(c, got, x, w):
    want, _ = gm.ref_stft(c, x, w)
    err, use = gm.stft_error(c, got, want)
    return float(np.nan_to_num(err[use], nan=np.inf).max() / np.abs(want).max())


def inv_err(c, got, sp, w):
    want, _ = m.ref_istft(c, sp, w)
    return float(np.nan_to_num(np.abs(got - want).astype(np.float64), nan=np.inf).max() / np.abs(want).max())


_RESULTS = {}


def results():
    """every table case and the multi-trip cases of a two-CU device, emulated once: id -> (kind, case, error, ids)"""
    if not _RESULTS:
        mf, mi = m.multi_trip_cases(HOST_CUS)
        for c in m.FWD_CASES + mf:
            got, ids, x, w = run_fwd(c, HOST_CUS)
            _RESULTS['fwd ' + c['id']] = ('fwd', c, fwd_err(c, got, x, w), ids)
        for c in m.INV_CASES + mi:
            got, ids, sp, w = run_inv(c, HOST_CUS)
            _RESULTS['inv ' + c['id']] = ('inv', c, inv_err(c, got, sp, w), ids)
    return _RESULTS


def test_the_emulations_agree_with_longdouble():
    for key, (_, c, err, _) in results().items():
        assert err <= AGREE, (key, err)


def test_every_branch_has_a_case():
    assert len(set(m.BRANCHES)) == len(m.BRANCHES) and not set(m.EXCLUDED) & set(m.BRANCHES)
    assert len({c['id'] for c in m.FWD_CASES}) == len(m.FWD_CASES) and len({c['id'] for c in m.INV_CASES}) == len(m.INV_CASES)
    reached = {}
    for key, (_, c, _, ids) in results().items():
        for b in ids:
            assert b in m.BRANCHES, (key, b)
            reached.setdefault(b, key)
    missing = [b for b in m.BRANCHES if b not in reached]
    assert not missing, missing
    # the ids the issue names one case for
    named = {'lanes.idle': 'fwd 1000 two frames per wave', 'lanes.no_input': 'fwd 96 odd T', 'fetch.slow.misaligned': 'fwd 96 odd T',
             'fetch.mixed_wave': 'fwd 160 odd hop', 'T<n_fft': 'fwd 160 T 30', 'fetch.easy': 'fwd 160 easy, last group partial',
             'group.partial': 'fwd 160 easy, last group partial', 'bs.ncr.2': 'fwd bs 4', 'bs.M.exact_fit': 'fwd bs 128',
             'bs.ncr.odd': 'fwd bs 6', 'win.odd': 'fwd 400 win 301', 'fwd.mr.trips>=2': 'fwd trips 160 hop 2'}
    for b, key in named.items():
        assert b in results()[key][3], (b, key)
    assert 'fetch.easy' in results()['fwd trips 160 hop 2'][3] and 'fetch.easy' not in results()['fwd trips 160 hop 1'][3]


@pytest.mark.parametrize('cus', [1, 2, 64, 256, 304])
def test_the_multi_trip_cases_take_a_second_trip_at_any_cu_count(cus):
    """the formula, not the emulation: just over one trip's worth of frames, under 40 MB of output at 256 compute units"""
    fwd, inv = m.multi_trip_cases(cus)
    for c in fwd:
        total = gm.frames_of(c)
        la = m.launch_of(m.FWD_KERNEL[m.forward_family(c)], c['n_fft'], total, cus)
        per_trip = la['grid'] * la['per_block'] * la['G']
        assert la['trips'] == 2 and per_trip < total < per_trip + 64 and la['groups'] % (la['grid'] * la['per_block']), c['id']
        if cus <= 256:
            assert total * (c['n_fft'] // 2 + 1) * 8 <= 41e6, c['id']
    for c in inv:
        la = m.launch_of(m.INV_KERNEL[m.inverse_family(c)], c['n_fft'], c['F'], cus)
        assert la['trips'] == 2 and la['groups'] % (la['grid'] * la['per_block']), c['id']
        if cus <= 256:
            assert c['F'] * max(c['win'], (c['n_fft'] // 2 + 1) * 2) * 4 <= 41e6, c['id']
    # a second trip of k_stft_mr needs more than 4 * 3 * CUs frame groups
    assert m.launch_of('k_stft_mr', 160, 16 * 12 * cus, cus)['trips'] == 1 and m.launch_of('k_stft_mr', 160, 16 * 12 * cus + 1, cus)['trips'] == 2


def test_the_cases_are_small():
    for c in m.FWD_CASES:
        assert c['B'] * c['C'] * gm.frames_of(c) * c['n_fft'] <= 60000, c['id']
    for c in m.INV_CASES:
        assert c['B'] * c['C'] * c['F'] * max(c['n_fft'], c['win']) <= 60000, c['id']


# ---- 5. mutants ------------------------------------------------------------------------------------------------------
# mutant -> the case that tells it from the reference
FWD_KILLERS = {
    'li_clamp': '96 eight signals of one frame', 'lower_bound': 'plan 120', 'ob_wrong_trip': 'trips 160 hop 2',
    'o_skip': '160 easy, last group partial', 'readlane': 'plan 160', 'k_le_ncr': 'bs 6', 'ostride1': 'plan 192',
    'gather': 'big 8192',
}
INV_KILLERS = {'inv_dcnyq': 'plan 96', 'inv_tail': 'big 4096 win 4500', 'inv_store': '400 win 301', 'ostride1': 'plan 120'}
NEUTRAL = m.NEUTRAL


def killed(run, err_of, c, cus, mutant):
    try:
        got, _, a, w = run(c, cus, mutant)
    except (m.OutOfBounds, m.WriteError):
        return True
    return err_of(c, got, a, w) > 1e-6


@pytest.mark.parametrize('mutant', sorted(m.FWD_MUTANTS))
def test_forward_mutants(mutant):
    cases = {c['id']: c for c in m.FWD_CASES + m.multi_trip_cases(HOST_CUS)[0]}
    if mutant in NEUTRAL:
        assert mutant not in FWD_KILLERS and NEUTRAL[mutant]
        for c in cases.values():
            got, _, x, w = run_fwd(c, HOST_CUS, mutant)
            assert fwd_err(c, got, x, w) <= AGREE, (mutant, c['id'])
        return
    c = cases[FWD_KILLERS[mutant]]
    assert not killed(run_fwd, fwd_err, c, HOST_CUS, None)
    assert killed(run_fwd, fwd_err, c, HOST_CUS, mutant), (mutant, c['id'])


@pytest.mark.parametrize('mutant', sorted(m.INV_MUTANTS))
def test_inverse_mutants(mutant):
    cases = {c['id']: c for c in m.INV_CASES}
    c = cases[INV_KILLERS[mutant]]
    assert not killed(run_inv, inv_err, c, HOST_CUS, None)
    assert killed(run_inv, inv_err, c, HOST_CUS, mutant), (mutant, c['id'])


# ---- 6. the reference alone ------------------------------------------------------------------------------------------
def test_the_phase_cases_leave_few_bins_out():
    seen = 0
    for c in m.FWD_CASES + m.multi_trip_cases(256)[0]:
        if c['mode'] != m.PHASE or c.get('multi'):
            continue
        want, _ = gm.ref_stft(c, m.fwd_input(c), m.fwd_window(c))
        left_out = 1.0 - float((np.abs(want) >= m.PHASE_FLOOR * np.abs(want).max()).mean())
        assert left_out <= m.PHASE_LEFT_OUT, (c['id'], left_out)
        seen += 1
    assert seen >= 4


def test_the_bound_constants():
    """the constants the docstring derives, spelled out for one plan of each kind"""
    assert m.PLANS[400].stages == (4, 5, 2, 5) and m.PLANS[400].const() == 11 + 12 + 9 + 12
    assert m.PLANS[1000].stages == (4, 5, 5, 5) and m.PLANS[96].stages == (8, 2, 3) and m.PLANS[960].stages == (4, 5, 8, 3)
    assert m.fft_const(m.FAM_BIG, 4096) == 90 + 9 and m.fft_const(m.FAM_BIG, 8192) == 90 + 11 and m.fft_const(m.FAM_POW2, 512) == 72
    bt = float(np.abs(m.build_bluestein(400)[1]).sum())
    assert abs(m.fft_const(m.FAM_BS, 400) - 2 * (2 * 81 + 11.49) * bt) < 1e-9 and 5 < bt < 0.75 * np.sqrt(400)


# ---- 7. the prototypes in float32 ------------------------------------------------------------------------------------
def frames32(c, x, window):
    """the windowed, cropped frames of signal (0, 0) as the kernels form them: float32 products"""
    n, win, hop = c['n_fft'], c['win'], c['hop']
    sig = np.asarray(x[0, 0], np.float32)
    if c['pad_begin']:
        sig = np.pad(sig, (n - hop, 0))
    f_ = gm.frames_of(c)
    sig = np.pad(sig, (0, max(0, (f_ - 1) * hop + win - sig.size)))
    idx = np.arange(win)[None, :] + hop * np.arange(f_)[:, None]
    fr = (sig[idx] * np.asarray(window, np.float32))[:, :n]
    return np.pad(fr, ((0, 0), (0, n - fr.shape[1])))


def stockham32(a):
    """proto_stockham's lane FFT of a power-of-two length on complex64 values"""
    import proto_stockham as ps
    nc = a.shape[0]
    lanes = nc // ps.P
    regs = np.asarray(a, np.complex64).reshape(ps.P, lanes).T.copy()                     # regs[lane, m] = a[lane + L m]
    return ps.complex_fft_lanes(regs, nc, -1).T.reshape(nc)


def pair32(z, n_fft):
    n = n_fft // 2
    k = np.arange(n + 1)
    zk, zp = z[k % n], np.conj(z[(n - k) % n])
    t = np.exp(-2j * np.pi * k / n_fft).astype(np.complex64)
    return (zk + zp) / 2 - 1j * t * (zk - zp) / 2


def big32(frame):
    """k_stft_big's decomposition on complex64 values: R sub-FFTs of 1024 points (proto_stockham), W_NB^{rk}, the radix-R combine"""
    n_fft = frame.shape[0]
    r_, nb = m.BIG[n_fft], n_fft // 2
    z = (frame[0::2] + 1j * frame[1::2]).astype(np.complex64)
    k = np.arange(1024)
    e = [stockham32(z[r::r_]) * np.exp(-2j * np.pi * r * k / nb).astype(np.complex64) for r in range(r_)]
    out = np.zeros(nb, np.complex64)
    for s in range(r_):
        out[1024 * s + k] = sum(np.complex64(np.exp(-2j * np.pi * r * s / r_)) * e[r] for r in range(r_))
    return pair32(out, n_fft)


@pytest.mark.parametrize('cid', ['plan %d' % n for n in sorted(m.PLANS)] + ['bs 4', 'bs 6', 'bs 126', 'bs 128', 'bs 130', 'bs 510', 'bs 1022',
                                                                           'bs 400', 'big 4096 win 3001', 'big 8192 win 5000'])
def test_a_float32_run_of_the_prototypes_stays_inside_the_bound(cid):
    """the reference alone satisfies limit (a): oracle/proto_mixed_radix.py, proto_bluestein.py and proto_stockham.py follow the
    kernels' passes; run on complex64 values with constants rounded to float32 they stay inside u c S on the gate's inputs"""
    import proto_bluestein as pbs
    import proto_mixed_radix as pmr
    c = dict({c['id']: c for c in m.FWD_CASES}[cid], mode=m.COMPLEX)
    x, w = m.fwd_input(c), m.fwd_window(c)
    want, s = gm.ref_stft(c, x, w)
    bound = m.stft_bound(c, want, s)[0, 0]
    fam = m.forward_family(c)
    fr = frames32(c, x, w)
    worst = 0.0
    for f in np.argsort(s[0, 0, :, 0])[-2:]:                     # the two fullest frames (with padding some are all zeros)
        if fam == m.FAM_MR:
            got = pmr.rfft_mr(fr[f], dtype=np.complex64)
        elif fam == m.FAM_BS:
            got = pbs.rfft_bluestein(fr[f], np.complex64, stockham32)
        else:
            got = big32(fr[f])
        assert got.dtype == np.complex64
        err = np.abs(got.astype(np.clongdouble) - want[0, 0, f]).astype(np.float64)
        assert err.max() > 0                                    # a float32 run, not the reference again
        worst = max(worst, float((err / bound[f]).max()))
    print('float32 prototype, %s: worst error / bound = %.4f' % (cid, worst))
    assert worst <= 1.0
