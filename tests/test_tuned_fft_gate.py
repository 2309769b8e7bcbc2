"""-m gpu: the gate of the tuned transforms at the sizes that are not 256 ... 2048 -- k_stft_mr<plan> (18 plans), k_stft_bs<M>,
k_stft_big<R> and the two-kernel inverses k_irfft_mr / k_irfft_bs<M> / k_irfft_big<R> / k_irfft<NC> + k_ola.  The older tests meet
each of them with one shape per size and a tolerance of 2e-5 of the largest output.  Here they run on the case tables of
tests/tuned_fft_model.py: every plan, the idle and input-less lanes, partial groups, both fetch paths and the wave that mixes them,
both layouts on either side, the three epilogues, Bluestein at the edges of M, and -- built from the device's CU count -- launches
that take a second trip of every grid-stride loop (tests/test_tuned_fft_model_host.py proves on the CPU that the tables reach every
id of tuned_fft_model.BRANCHES and disposes of every one-line mutant).

Every case poisons the output allocation with NaN, runs through STFT (STFT._run for magnitude and phase) or _ffi.istft under
istft_path 2, asserts that _ffi.last_launches() EQUALS the expected list, calls kapre.check_device() and compares with numpy.fft on
longdouble frames:
  (a) element by element within u c S, c derived per plan in tuned_fft_model's docstring (NaN fails); phase at the bins with
      |want| >= 1e-2 of the largest (at most 2 % may be left out)
  (b) max |err| / max |want| <= 2e-5 forward (tests/test_gpu_parity.py), 4e-6 inverse (tests/test_fft_family_labels.py)
The multi-trip cases keep their references on the device in float64 and assert the same two limits there.
Exact checks: zero input gives zeros; one NaN sample spoils exactly its own frame; DC and Nyquist are real and their phase is 0 or
pi by the sign; n_fft 400 through k_stft_bs and through k_stft_mr agree within the sum of their bounds.

The last test asserts that the cases that ran reached every id and prints each kernel's worst figures (DESIGN.md 4.8.6 quotes them).
"""
import time

import numpy as np
import pytest
import torch

import generic_model as gm
import tuned_fft_model as m
import kapre_amd as kapre
from kapre_amd import STFT, _ffi, backend

pytestmark = pytest.mark.gpu

HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 1e-18
REACHED = set()
WORST = {}
T0 = [None]


def cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def poison(numel, dtype):
    """the next torch.empty of this size is handed this block by the caching allocator: what a kernel leaves unwritten is NaN"""
    t = torch.full((int(numel),), float('nan'), dtype=dtype, device='cuda')
    del t


def note(kernel, figure, value):
    value = value if value == value else float('inf')
    WORST[kernel, figure] = max(WORST.get((kernel, figure), 0.0), value)


def fraction(err, bound, use=None):
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    frac = np.nan_to_num(frac, nan=np.inf)
    if use is not None:
        frac = frac[use]
    return float(frac.max()) if frac.size else 0.0


def ratio(err, want):
    err = np.nan_to_num(np.asarray(err, np.float64), nan=np.inf)
    return float(err.max() / max(float(np.abs(want).max()), 1e-300)) if err.size else 0.0


def check(kernel, cid, err, bound, want, limit, use=None):
    frac = fraction(err, bound, use)
    got_ratio = ratio(err[use] if use is not None else err, want)
    note(kernel, 'error / bound', frac)
    line = 'tuned gate [%s] %s: worst error / bound = %.4f' % (kernel, cid, frac)
    if limit is not None:
        note(kernel, 'max error / max (limit %.0e)' % limit, got_ratio)
        line += ', max error / max = %.3g' % got_ratio
    print(line)
    assert frac <= 1.0, '%s %s: %.3g of the bound' % (kernel, cid, frac)
    if limit is not None:
        assert got_ratio <= limit, '%s %s: max error / max = %.3g, limit %.3g' % (kernel, cid, got_ratio, limit)


class option:
    """kpr_set_option for the duration of a block"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = _ffi.set_option(self.name, self.value)

    def __exit__(self, *exc):
        _ffi.set_option(self.name, self.old)


def kernel_name(c, fam):
    mode = '' if c.get('mode', m.COMPLEX) == m.COMPLEX else ' magnitude' if c['mode'] == m.MAGNITUDE else ' phase'
    return {m.FAM_MR: 'mr', m.FAM_BS: 'bs', m.FAM_BIG: 'big', m.FAM_POW2: 'pow2'}[fam] + mode


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
FWD_TABLE = {c['id']: c for c in m.FWD_CASES}


def stft_layer(c):
    return STFT(n_fft=c['n_fft'], win_length=c['win'], hop_length=c['hop'], pad_begin=c['pad_begin'], pad_end=c['pad_end'],
                input_data_format=c['in_fmt'], output_data_format=c['out_fmt'])


def run_stft(c, layer, xd):
    if T0[0] is None:
        T0[0] = time.time()
    f_, k_ = gm.frames_of(c), c['n_fft'] // 2 + 1
    dtype = torch.complex64 if c['mode'] == m.COMPLEX else torch.float32
    poison(c['B'] * c['C'] * f_ * k_, dtype)
    with option('mixed_radix', c.get('mixed_radix', 1)):
        got = layer(xd) if c['mode'] == m.COMPLEX else layer._run(xd, c['mode'])
        launches = _ffi.last_launches()
    assert launches == m.forward_launches(c, cus()), launches
    assert tuple(got.shape) == gm.shape_of(c['out_fmt'], c['B'], c['C'], f_, k_) and got.dtype == dtype
    kapre.check_device()
    return got


def forward(c, x):
    """(got in the logical (B, C, F, K) order, window) of one forward case on the host array x (B, C, T)"""
    layer = stft_layer(c)
    window = backend.window_values(layer.window_fn, c['win'], np.float32)
    got = run_stft(c, layer, torch.from_numpy(gm.to_layout(x, c['in_fmt'])).cuda())
    return gm.from_layout(got.cpu().numpy(), c['out_fmt']), window


@pytest.mark.parametrize('cid', list(FWD_TABLE))
def test_stft(cid):
    c = FWD_TABLE[cid]
    x = m.fwd_input(c)
    got, window = forward(c, x)
    want, s = gm.ref_stft(c, x if HAVE_LONGDOUBLE else x.astype(np.float64), window)
    assert got.shape == want.shape
    err, use = gm.stft_error(c, got, want)
    fam = m.forward_family(c)
    if c['mode'] == m.PHASE:
        left_out = 1.0 - float(use.mean())
        print('tuned gate %s: %.2f %% of the bins left out' % (cid, 100 * left_out))
        assert left_out <= m.PHASE_LEFT_OUT
        # the bins left out must still be numbers
        assert np.isfinite(got).all()
    check('k_stft_' + kernel_name(c, fam), cid, err, m.stft_bound(c, want, s), gm.stft_want(c, want),
          None if c['mode'] == m.PHASE else m.REG_FWD, use if c['mode'] == m.PHASE else None)
    if c['mode'] == m.COMPLEX:                                  # real input: DC and Nyquist are real, exactly
        assert not got[..., 0].imag.any() and not got[..., -1].imag.any()
    if c['mode'] == m.PHASE:                                    # ... and their phase is 0 or +pi by the sign of the real part
        for k in (0, -1):
            sure = np.abs(want[..., k].real) > m.stft_bound(dict(c, mode=m.COMPLEX), want, s)[..., k]
            assert np.isin(got[..., k], (np.float32(0.0), np.float32(np.pi))).all()
            assert ((got[..., k] != 0) == (want[..., k].real < 0))[sure].all()
    ids = set()
    m.emulate_stft(c, gm.to_layout(x, c['in_fmt']), window, cus(), None, ids)
    REACHED.update(ids | m.static_fwd_ids(c))


MULTI_FWD = [c['id'] for c in m.multi_trip_cases(256)[0]]


@pytest.mark.parametrize('cid', MULTI_FWD)
def test_stft_with_a_second_trip(cid):
    """just over one trip's worth of frames at THIS device's CU count: k_stft_mr consumes in trip 2 the samples, validity bits and
    output base it fetched in trip 1.  Reference: x.unfold and torch.fft.rfft in float64 on the device, the bound from its frames"""
    c = {c['id']: c for c in m.multi_trip_cases(cus())[0]}[cid]
    fam = m.forward_family(c)
    f_ = gm.frames_of(c)
    la = m.launch_of(m.FWD_KERNEL[fam], c['n_fft'], f_, cus())
    assert la['trips'] == 2 and la['groups'] % (la['grid'] * la['per_block'])
    layer = stft_layer(c)
    gen = torch.Generator(device='cuda').manual_seed(gm.seed_of(c))
    x = torch.randn((1, 1, c['T']), dtype=torch.float32, device='cuda', generator=gen)
    got = run_stft(c, layer, x)[0, 0]
    window = torch.from_numpy(backend.window_values(layer.window_fn, c['win'], np.float32).astype(np.float64)).cuda()
    worst_frac, worst_err, biggest, use_share = 0.0, 0.0, 0.0, 1.0
    cc = 2 * m.fft_const(fam, c['n_fft']) + 5
    for lo in range(0, f_, 4096):                              # in slices: the float64 frames of n_fft 8192 are 64 KiB each
        hi = min(f_, lo + 4096)
        frames = x[0, 0, lo * c['hop']:(hi - 1) * c['hop'] + c['n_fft']].to(torch.float64).unfold(-1, c['n_fft'], c['hop']) * window
        want = torch.fft.rfft(frames, dim=-1)
        bound = m.U32 * cc * frames.abs().sum(-1, keepdim=True)
        g = got[lo:hi]
        if c['mode'] == m.COMPLEX:
            err = (g.to(torch.complex128) - want).abs()
        elif c['mode'] == m.MAGNITUDE:
            err, bound = (g.to(torch.float64) - want.abs()).abs(), bound + 2 * m.U32 * want.abs()
        else:
            d = g.to(torch.float64) - want.angle()
            err = torch.atan2(torch.sin(d), torch.cos(d)).abs()
            bound = torch.asin(torch.clamp(bound / want.abs(), max=1.0)) + 4 * m.U32 * np.pi
            use = want.abs() >= m.PHASE_FLOOR * want.abs().max()
            use_share = min(use_share, float(use.double().mean()))
            err, bound = torch.where(use, err, torch.zeros_like(err)), torch.where(use, bound, torch.ones_like(bound))
        err = torch.nan_to_num(err, nan=float('inf'))
        worst_frac = max(worst_frac, float((err / bound).max()))
        worst_err, biggest = max(worst_err, float(err.max())), max(biggest, float(want.abs().max()))
    kernel = 'k_stft_' + kernel_name(c, fam) + ' second trip'
    note(kernel, 'error / bound', worst_frac)
    print('tuned gate [%s] %s: %d frames, %d per trip, worst error / bound = %.4f, max error / max = %.3g'
          % (kernel, cid, f_, la['grid'] * la['per_block'] * la['G'], worst_frac, worst_err / biggest))
    assert worst_frac <= 1.0
    if c['mode'] != m.PHASE:
        note(kernel, 'max error / max (limit %.0e)' % m.REG_FWD, worst_err / biggest)
        assert worst_err / biggest <= m.REG_FWD
    else:
        assert 1.0 - use_share <= m.PHASE_LEFT_OUT and bool(torch.isfinite(got).all())
    REACHED.update(m.static_fwd_ids(c) | {'trips>=2', 'trips>=2.last_partial', 'fwd.%s.trips>=2' % fam})


# ---------------------------------------------------------------------------------------------
# inverse
# ---------------------------------------------------------------------------------------------
INV_TABLE = {c['id']: c for c in m.INV_CASES}


def run_istft(c, sd, synth):
    if T0[0] is None:
        T0[0] = time.time()
    t_out = (c['F'] - 1) * c['hop'] + c['win']
    poison(c['B'] * c['C'] * t_out, torch.float32)
    with option('istft_path', 2), option('mixed_radix', c.get('mixed_radix', 1)):
        got = _ffi.istft(sd, torch.from_numpy(synth).cuda(), c['n_fft'], c['win'], c['hop'], c['wave_fmt'], c['spec_fmt'])
        launches = _ffi.last_launches()
    assert launches == m.inverse_launches(c, cus()), launches
    assert tuple(got.shape) == gm.shape_of(c['wave_fmt'], c['B'], c['C'], t_out) and got.dtype == torch.float32
    kapre.check_device()
    return got


@pytest.mark.parametrize('cid', list(INV_TABLE))
def test_istft(cid):
    c = INV_TABLE[cid]
    spec, synth = m.inv_input(c), m.inv_window(c)
    sin = gm.to_layout(spec, c['spec_fmt'])
    got = gm.from_layout(run_istft(c, torch.from_numpy(sin).cuda(), synth).cpu().numpy(), c['wave_fmt'])
    want, bound = m.ref_istft(c, spec, synth)
    assert got.shape == want.shape
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    check('k_irfft_' + kernel_name(c, m.inverse_family(c)) + ' + k_ola', cid, err, bound, want, m.REG_INV)
    ids = set()
    m.emulate_irfft(c, sin, synth, cus(), None, ids)
    REACHED.update(ids)


MULTI_INV = [c['id'] for c in m.multi_trip_cases(256)[1]]


@pytest.mark.parametrize('cid', MULTI_INV)
def test_istft_with_a_second_trip(cid):
    """more frame groups than one trip of the inverse FFT kernel takes on this device.  Reference: torch.fft.irfft and strided
    additions in float64 on the device; the bound of tuned_fft_model.ref_istft built there"""
    c = {c['id']: c for c in m.multi_trip_cases(cus())[1]}[cid]
    fam = m.inverse_family(c)
    f_, n, win, hop = c['F'], c['n_fft'], c['win'], c['hop']
    la = m.launch_of(m.INV_KERNEL[fam], n, f_, cus())
    assert la['trips'] == 2 and la['groups'] % (la['grid'] * la['per_block'])
    synth = m.inv_window(c)
    gen = torch.Generator(device='cuda').manual_seed(gm.seed_of(c))
    spec = torch.view_as_complex(torch.randn((1, 1, f_, n // 2 + 1, 2), dtype=torch.float32, device='cuda', generator=gen))
    got = run_istft(c, spec, synth).view(-1).to(torch.float64)
    sw = torch.from_numpy(synth.astype(np.float64)).cuda()
    s64 = spec.to(torch.complex128).view(f_, -1)
    frames = torch.fft.irfft(s64, n=n, dim=-1)[:, :win] * sw
    mag = s64.abs()
    mag[:, 0], mag[:, -1] = s64[:, 0].real.abs(), s64[:, -1].real.abs()
    herm = 2 * mag.sum(-1, keepdim=True) - mag[:, :1] - mag[:, -1:]
    cc = 2 * (m.fft_const(fam, n) + 4) + 3
    fb = m.U32 * cc * herm / n * sw.abs()
    t_out = (f_ - 1) * hop + win
    want, bound, terms, count = (torch.zeros(t_out, dtype=torch.float64, device='cuda') for _ in range(4))
    for j in range(win):
        sl = slice(j, j + (f_ - 1) * hop + 1, hop)
        want[sl] += frames[:, j]
        bound[sl] += fb[:, j]
        terms[sl] += frames[:, j].abs()
        count[sl] += 1
    bound += torch.clamp(count - 1, min=0) * m.U32 * terms
    err = torch.nan_to_num((got - want).abs(), nan=float('inf'))
    frac, rel = float((err / bound).max()), float(err.max() / want.abs().max())
    kernel = 'k_irfft_' + kernel_name(c, fam) + ' + k_ola second trip'
    note(kernel, 'error / bound', frac)
    note(kernel, 'max error / max (limit %.0e)' % m.REG_INV, rel)
    print('tuned gate [%s] %s: %d frames, %d per trip, worst error / bound = %.4f, max error / max = %.3g'
          % (kernel, cid, f_, la['grid'] * la['per_block'] * la['G'], frac, rel))
    assert frac <= 1.0 and rel <= m.REG_INV
    REACHED.update({'trips>=2', 'trips>=2.last_partial', 'inv.%s.trips>=2' % fam})


# ---------------------------------------------------------------------------------------------
# exact checks
# ---------------------------------------------------------------------------------------------
EXACT = ['plan 96', 'plan 1000', '160 odd hop', 'bs 6', 'bs 130', 'bs 400', 'big 4096 win 3001']


@pytest.mark.parametrize('cid', EXACT)
@pytest.mark.parametrize('mode', [m.COMPLEX, m.MAGNITUDE, m.PHASE])
def test_zero_input_gives_zero_output(cid, mode):
    """no NaN from idle or clamped lanes, and atan2(0, 0) = 0"""
    c = dict(FWD_TABLE[cid], mode=mode)
    got, _ = forward(c, np.zeros((c['B'], c['C'], c['T']), np.float32))
    if got.any():
        print('tuned gate, zero input %s: %d of %d outputs are not zero, values %s' % (cid, np.count_nonzero(got), got.size, np.unique(got[got != 0])[:8]))
    assert got.shape[2] == gm.frames_of(c) and not got.any() and np.isfinite(got).all()


@pytest.mark.parametrize('n_fft, kw', [(160, {}), (96, {}), (1000, {}), (400, dict(mixed_radix=0)), (126, {}), (4096, {})])
def test_one_nan_sample_spoils_exactly_its_own_frame(n_fft, kw):
    """hop >= n_fft: the frames do not overlap.  The frames that share the wave (k_stft_mr, k_stft_bs), the LDS rows and the
    clamped loads of the NaN's neighbours stay inside their bounds"""
    frames = 2 * 64 // max(1, n_fft // 32) + 3 if n_fft < 4096 else 6
    c = m.fcase('nan %d' % n_fft, n_fft, hop=n_fft + 2, B=1, C=1, frames=frames, **kw)
    f_ = gm.frames_of(c)
    x = m.fwd_input(c)
    bad = f_ // 2
    x[0, 0, bad * c['hop'] + n_fft // 3] = np.nan
    got, window = forward(c, x)
    finite = np.isfinite(got).all(-1)[0, 0]
    assert not np.isfinite(got[0, 0, bad]).any(), 'the frame with the NaN'
    assert finite[np.arange(f_) != bad].all(), np.nonzero(~finite)[0]
    clean = np.where(np.isnan(x), 0.0, x).astype(np.float32)
    want, s = gm.ref_stft(c, clean, window)
    err, _ = gm.stft_error(c, got, want)
    keep = np.arange(f_) != bad
    assert fraction(err[:, :, keep], m.stft_bound(c, want, s)[:, :, keep]) <= 1.0


def test_n_fft_400_agrees_on_both_kernels():
    """the same frames through k_stft_mr<200> and, with mixed_radix 0, through k_stft_bs: within the sum of their bounds"""
    c_mr = FWD_TABLE['plan 400']
    c_bs = dict(c_mr, mixed_radix=0)
    assert m.forward_launches(c_mr, cus()) == 'k_stft_mr<200>' and m.forward_launches(c_bs, cus()) == 'k_stft_bs'
    x = m.fwd_input(c_mr)
    got_mr, window = forward(c_mr, x)
    got_bs, _ = forward(c_bs, x)
    want, s = gm.ref_stft(c_mr, x, window)
    both = m.stft_bound(c_mr, want, s) + m.stft_bound(c_bs, want, s)
    diff = np.abs(got_mr.astype(np.complex128) - got_bs.astype(np.complex128))
    frac = fraction(diff, both)
    print('tuned gate [n_fft 400, k_stft_mr against k_stft_bs]: worst difference / (sum of bounds) = %.4f, max difference / max = %.3g'
          % (frac, ratio(diff, want)))
    note('k_stft_mr<200> against k_stft_bs', 'difference / sum of bounds', frac)
    assert frac <= 1.0


# ---------------------------------------------------------------------------------------------
# what this file reached
# ---------------------------------------------------------------------------------------------
def test_every_branch_was_reached():
    """runs last: the union of the branch ids of the cases above is BRANCHES"""
    if not REACHED:
        pytest.skip('the cases above did not run in this session')
    print('tuned gate on %d compute units, %.1f s since the first case; worst figures:' % (cus(), time.time() - T0[0]))
    for kernel, figure in sorted(WORST):
        print('  %-44s %-36s %.4g' % (kernel, figure, WORST[kernel, figure]))
    assert REACHED >= set(m.BRANCHES), sorted(set(m.BRANCHES) - REACHED)
    assert REACHED <= set(m.BRANCHES), sorted(REACHED - set(m.BRANCHES))
