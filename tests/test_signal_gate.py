"""-m gpu: the forward gate of k_frame, k_energy, k_delta and k_thin_gemm (kapre_amd/csrc/kpr_signal_kernels.h).  The golden
fixtures meet these kernels at one or two workload shapes; here they run on the case tables of tests/signal_model.py, the
smallest shape at which each branch of the host dispatch and of the kernels exists (tests/test_signal_model_host.py proves on the
CPU that the tables reach every branch of signal_model.BRANCHES and tell every one-line mutant of the kernels from the oracle).

Every case runs twice:
  exact inputs    small integers (Energy [-15, 15], Delta [-63, 63], thin GEMM A and B in [-7, 7]; Frame is a copy): every float32
                  operation is exact whatever the order of the additions, so the expected output is known to the bit and compared
                  with assert_array_equal -- one dropped, duplicated or misplaced element is a non-zero difference
  random floats   against the float64 oracle (oracle/kapre_oracle.py) under a bound per element:
                    Energy  (L + 8) * 2^-24 * want            (derived: signal_model.energy_bound; all terms are non-negative)
                            and, for L <= 400, the project's 2e-6 of the largest output (tests/test_gpu_parity.py)
                    Delta   (2n + 4) * 2^-24 * inv_denom * sum_j j (|x[t+j]| + |x[t-j]|)   (derived: signal_model.delta_bound)
                    thin GEMM through LogmelToMFCC / ApplyFilterbank: assert_close of tests/test_gpu_parity.py (REL and REG)
Every case asserts the launch label (k_thin_gemm where the model says thin, k_gemm where it says otherwise), poisons the output
allocation with NaN first, and the misaligned cases hand the library a contiguous view one float into a buffer.  The stride cases
(just over 65536 * 256 elements, 65 537 signals, 2048 * 64 + 17 rows) keep their references on the device or vectorised.

Not covered: the 64-bit index branch of k_frame (2^31 or more output vectors: at least 8.6 GB of output), signal_model.EXCLUDED.
The last test asserts that the cases that ran reached every other branch and prints each kernel's worst error as a fraction of its
bound (DESIGN.md 4.8.2 quotes them).
"""
import numpy as np
import pytest
import torch

import kapre_oracle as o
import signal_model as m
import kapre_amd as kapre
from kapre_amd import ApplyFilterbank, Delta, _ffi
from kapre_amd.signal import Frame, Energy, LogmelToMFCC
from test_gpu_parity import assert_close, REG

pytestmark = pytest.mark.gpu

REACHED = set()           # branch ids of the cases that ran and passed
WORST = {}                # kernel / bound -> worst error as a fraction of the bound


def poison(numel):
    """the next torch.empty of this size is handed this block by the caching allocator: what a kernel leaves unwritten is NaN"""
    t = torch.full((int(numel),), float('nan'), dtype=torch.float32, device='cuda')
    del t


def to_device(x, misaligned=False):
    """a contiguous float32 device tensor; misaligned: a view one float into its buffer (_ffi.as_device passes it through)"""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    if not misaligned:
        d = t.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device='cuda')
    d = buf[1:1 + t.numel()].view(t.shape)
    d.copy_(t)
    assert d.is_contiguous() and d.data_ptr() % 16 == 4
    assert _ffi.as_device(d, torch.float32) is d
    return d


def label():
    return _ffi.last_launches().split(' + ')[-1]


def note(what, frac):
    frac = frac if frac == frac else float('inf')
    WORST[what] = max(WORST.get(what, 0.0), frac)


def within(what, got, want, bound, cid):
    """|got - want| <= bound element by element (NaN fails)"""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(np.nan_to_num(frac, nan=np.inf).max()) if frac.size else 0.0
    print('signal gate [%s] %s: worst error / bound = %.3f' % (what, cid, worst))
    note(what, worst)
    assert worst <= 1.0, '%s %s: %.3g of the bound' % (what, cid, worst)


def by_id(cases):
    return {c['id']: c for c in cases}


# ---------------------------------------------------------------------------------------------
# Frame
# ---------------------------------------------------------------------------------------------
FRAME = by_id(m.FRAME_CASES)


def frame_layer(c):
    return Frame(frame_length=c['L'], hop_length=c['hop'], pad_end=c['pad_end'], pad_value=c['pad_value'], data_format=c['fmt'])


@pytest.mark.parametrize('cid', [cid for cid, c in FRAME.items() if not c.get('stride')])
def test_frame(cid):
    c = FRAME[cid]
    g = m.frame_geometry(c)
    for x in (np.random.default_rng(m.seed_of(c, 1)).integers(-99, 100, m.frame_input(c).shape).astype(np.float32), m.frame_input(c)):
        xd = to_device(x, c.get('misaligned'))
        poison(g['nrows'] * g['rowlen'])
        got = frame_layer(c)(xd)
        assert label() == m.frame_label(c), _ffi.last_launches()
        got = got.cpu().numpy()
        want = o.kapre_frame(x, c['L'], c['hop'], c['pad_end'], c['pad_value'], c['fmt'])
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want.astype(np.float32))
        np.testing.assert_array_equal(got, m.emulate_frame(c, x))
    note('k_frame (copy: exact)', 0.0)
    kapre.check_device()
    REACHED.update(m.frame_branches(c))


def test_frame_past_the_grid_cap():
    """rows of 7 floats (VEC 1) and just over 65536 * 256 output elements: every thread takes a second element; the reference is
    x.unfold on the device"""
    c = FRAME['stride 7/3']
    g = m.frame_geometry(c)
    assert m.N_STRIDE < g['total'] < m.N_STRIDE + 7 * 64 and not g['vec']
    xd = torch.randint(-9999, 10000, (1, 1, c['T']), device='cuda').to(torch.float32)
    poison(g['total'])
    got = frame_layer(c)(xd)
    assert label() == 'k_frame'
    assert tuple(got.shape) == (1, 1, g['F'], c['L'])
    assert torch.equal(got.view(g['F'], c['L']), xd.view(-1).unfold(0, c['L'], c['hop']))
    kapre.check_device()
    REACHED.update(m.frame_branches(c))


# ---------------------------------------------------------------------------------------------
# Energy
# ---------------------------------------------------------------------------------------------
ENERGY = by_id(m.ENERGY_CASES)


def energy_layer(c):
    return Energy(sample_rate=c['sample_rate'], ref_duration=c['ref_duration'], frame_length=c['L'], hop_length=c['hop'],
                  pad_end=c['pad_end'], pad_value=c['pad_value'], data_format=c['fmt'])


def run_energy(c, x):
    p = m.energy_plan(c)
    xd = to_device(x, c.get('misaligned'))
    poison(p['n_sig'] * p['F'])
    got = energy_layer(c)(xd)
    assert label() == 'k_energy', _ffi.last_launches()
    return got.cpu().numpy()


@pytest.mark.parametrize('cid', list(ENERGY))
def test_energy(cid):
    c = ENERGY[cid]
    assert energy_layer(c)._scale() == m.energy_scale(c)
    xe = m.energy_exact_input(c)
    want = m.energy_exact_expected(c, xe)
    got = run_energy(c, xe)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    note('k_energy (exact inputs)', 0.0)

    x = m.frame_input(c)
    want = o.kapre_energy(x, c['sample_rate'], c['ref_duration'], c['L'], c['hop'], c['pad_end'], c['pad_value'], c['fmt'])
    got = run_energy(c, x)
    assert got.shape == want.shape
    within('k_energy (L + 8) u want', got, want, m.energy_bound(c, want), cid)
    if c['L'] <= 400:
        top = np.abs(want).max()
        within('k_energy 2e-6 of max', got, want, np.full(want.shape, 2e-6 * top), cid)
    kapre.check_device()
    REACHED.update(m.energy_branches(c))


def test_energy_refuses_a_hop_ratio_its_lds_cannot_hold():
    c = m.ENERGY_REFUSED
    assert m.energy_plan(c)['refused']
    xd = to_device(m.frame_input(c))
    with pytest.raises(RuntimeError, match='kpr_energy_f32'):
        energy_layer(c)(xd)
    assert _ffi.device_status() == 0
    kapre.check_device()
    REACHED.update(m.energy_branches(c))


# ---------------------------------------------------------------------------------------------
# Delta
# ---------------------------------------------------------------------------------------------
DELTA_GROUPS = {}
for _c in m.DELTA_CASES:
    DELTA_GROUPS.setdefault(_c['group'], []).append(_c)


def run_delta(c, xd):
    poison(xd.numel())
    got = Delta(win_length=c['win'], mode=c['mode'], data_format=c['fmt'])(xd)
    assert label() == 'k_delta', _ffi.last_launches()
    assert got.shape == xd.shape
    return got


@pytest.mark.parametrize('group', [g for g in DELTA_GROUPS if g != 'stride'])
def test_delta(group):
    for c in DELTA_GROUPS[group]:
        xe = m.delta_exact_input(c)
        got = run_delta(c, to_device(xe, c.get('misaligned'))).cpu().numpy()
        np.testing.assert_array_equal(got, m.delta_exact_expected(c, xe), err_msg=c['id'])
        x = m.delta_input(c)
        got = run_delta(c, to_device(x, c.get('misaligned'))).cpu().numpy()
        within('k_delta derived bound', got, o.kapre_delta(x, c['win'], c['mode'], c['fmt']), m.delta_bound(c, x), c['id'])
        REACHED.update(m.delta_branches(c))
    note('k_delta (exact inputs)', 0.0)
    kapre.check_device()


@pytest.mark.parametrize('mode', m.MODES)
def test_delta_past_the_grid_cap(mode):
    """inner = 13 (VEC 1), just over 65536 * 256 elements; the reference is built on the device in float64 from the model's
    delta_src_index: exact for the integer input, under the derived bound for the random one"""
    c = by_id(m.DELTA_CASES)['stride w5 ' + mode]
    g = m.delta_geometry(c)
    T, n = c['T'], g['n']
    assert m.N_STRIDE < g['total'] < m.N_STRIDE + 13 * 64 and not g['vec']
    idx = torch.from_numpy(m.delta_src_index(np.arange(-n, T + n), T, mode)).cuda()
    inv = float(np.float32(1.0 / g['denom']))

    def reference(xd, absolute):
        xp = xd.view(T, 13).to(torch.float64)
        xp = torch.where((idx >= 0)[:, None], (xp.abs() if absolute else xp)[idx.clamp(min=0)], torch.zeros((), dtype=torch.float64, device='cuda'))
        num = torch.zeros((T, 13), dtype=torch.float64, device='cuda')
        for j in range(1, n + 1):
            hi, lo = xp[n + j:n + j + T], xp[n - j:n - j + T]
            num += j * (hi + lo if absolute else hi - lo)
        return num

    xe = torch.randint(-63, 64, g['shape'], device='cuda').to(torch.float32)
    got = run_delta(c, xe)
    assert torch.equal(got.view(T, 13), reference(xe, False).to(torch.float32) * inv)
    x = torch.rand(g['shape'], device='cuda') * 2 - 1
    got = run_delta(c, x)
    err = (got.view(T, 13).to(torch.float64) - reference(x, False) / g['denom']).abs()
    bound = (2 * n + 4) * m.U32 / g['denom'] * reference(x, True)
    worst = float((err / bound.clamp(min=1e-300)).max())
    worst = worst if worst == worst else float('inf')
    print('signal gate [k_delta derived bound] %s: worst error / bound = %.3f' % (c['id'], worst))
    note('k_delta derived bound', worst)
    assert worst <= 1.0
    kapre.check_device()
    REACHED.update(m.delta_branches(c))


# ---------------------------------------------------------------------------------------------
# Thin GEMM
# ---------------------------------------------------------------------------------------------
THIN_GROUPS = {}
for _c in m.THIN_CASES:
    THIN_GROUPS.setdefault(_c['id'].replace(' rows%d' % _c['rows'], ''), []).append(_c)


def matmul_rows(c, a, bd):
    """rows of `a` -> the rank-4 tensor of the case's layout -> _ffi.freq_matmul -> rows"""
    frames, C, K, N = c['rows'], c['C'], c['K'], c['N']
    x = a.reshape(1, frames, C, K).transpose(0, 1, 3, 2) if c['fmt'] == m.CL else a.reshape(1, C, frames, K)
    xd = to_device(x, c.get('misaligned'))
    poison(frames * C * N)
    out = _ffi.freq_matmul(xd, c['fmt'], bd)
    assert label() == m.thin_label(c), (c['id'], _ffi.last_launches())
    out = out.cpu().numpy()
    return (out.transpose(0, 1, 3, 2) if c['fmt'] == m.CL else out).reshape(frames * C, N)


@pytest.mark.parametrize('group', list(THIN_GROUPS))
def test_thin_gemm_exact(group):
    """integer A and B in [-7, 7] through _ffi.freq_matmul with the matrix given directly: the integer product, to the bit; the
    cases the model does not call thin (K % 4, K > 512, N > 64, channels_last with C > 1, misaligned x) must not launch it"""
    for c in THIN_GROUPS[group]:
        a, b = m.thin_exact_input(c)
        got = matmul_rows(c, a, to_device(b))
        np.testing.assert_array_equal(got, (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32), err_msg=c['id'])
        REACHED.update(m.thin_branches(c))
    note('k_thin_gemm (exact inputs)', 0.0)
    kapre.check_device()


def layer_close(what, c, got, want):
    assert label() == m.thin_label(c) == 'k_thin_gemm', _ffi.last_launches()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print('signal gate [k_thin_gemm REG] %s: error %.3g of the largest output = %.3f of REG' % (what, err, err / REG))
    note('k_thin_gemm REG (4e-6 of max)', err / REG)
    assert_close(got, want)
    REACHED.update(m.thin_branches(c))


@pytest.mark.parametrize('n_mfccs', [13, 20, 40])
@pytest.mark.parametrize('n_mels', [40, 64, 128])
def test_thin_gemm_through_logmel_to_mfcc(n_mels, n_mfccs):
    c = m.tcase(n_mels, min(n_mfccs, n_mels), 2 * 131)
    x = np.random.default_rng(n_mels + n_mfccs).uniform(-1, 1, (2, 1, 131, n_mels)).astype(np.float32)
    poison(2 * 131 * c['N'])
    got = LogmelToMFCC(n_mfccs=n_mfccs, data_format=m.CF)(to_device(x)).cpu().numpy()
    layer_close('LogmelToMFCC %d -> %d' % (n_mels, n_mfccs), c, got, o.kapre_logmel_to_mfcc(x, n_mfccs, m.CF))
    kapre.check_device()


@pytest.mark.parametrize('n_mels', [40, 64])
def test_thin_gemm_through_apply_filterbank_above_64_kib(n_mels):
    """512 bins x 40 filters = 96 KiB, x 64 = 128 KiB of B fragments in LDS: the launches that need the opt-in"""
    c = m.tcase(512, n_mels, 2 * 131)
    assert 'thin.lds>64K' in m.thin_branches(c)
    layer = ApplyFilterbank(type='mel', filterbank_kwargs=dict(sample_rate=22050, n_freq=512, n_mels=n_mels), data_format=m.CF)
    x = np.random.default_rng(n_mels).uniform(0, 1, (2, 1, 131, 512)).astype(np.float32)
    poison(2 * 131 * n_mels)
    got = layer(to_device(x)).cpu().numpy()
    layer_close('ApplyFilterbank 512 -> %d' % n_mels, c, got, o.apply_filterbank(x, np.asarray(layer.filterbank), m.CF))
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# what this file reached
# ---------------------------------------------------------------------------------------------
def test_every_branch_was_reached():
    """runs last: the union of the branch ids of the cases above is BRANCHES minus the declared exclusion"""
    if not REACHED:
        pytest.skip('the cases above did not run in this session')
    print('signal gate worst error / bound:')
    for what in sorted(WORST):
        print('  %-40s %.4f' % (what, WORST[what]))
    assert REACHED == set(m.BRANCHES) - set(m.EXCLUDED), (sorted(set(m.BRANCHES) - set(m.EXCLUDED) - REACHED), sorted(REACHED - set(m.BRANCHES)))
