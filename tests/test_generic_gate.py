"""-m gpu: the forward gate of the size-generic FFT engine (k_stft_gen<T,TWL>, k_irfft_gen<T,TWL> of
kapre_amd/csrc/kpr_generic_kernels.h), of k_ola<T> behind it and of k_filterbank_f64.  The engine is every float64 layer's only
transform and float32's transform at every size without a tuned plan; the other tests meet it at a dozen sizes that reach radices
2 ... 5 (float64) and 7, 11, 13 (float32).  Here it runs on the case tables of tests/generic_model.py: the smallest shapes that reach
every radix form as a first and as a later pass, the float64 direct DFT, both twiddle placements, every LDS edge, the second trip of
every loop and both precisions of the inverse (tests/test_generic_model_host.py proves on the CPU that the tables reach every id of
generic_model.BRANCHES and tell every one-line mutant of the kernels from the reference).

Every case poisons the output allocation with NaN, runs through the layers (STFT, InverseSTFT, ApplyFilterbank; STFT._run for the
magnitude and phase modes of kpr_stft_f32 / kpr_stft_f64), asserts that _ffi.last_launches() EQUALS the expected list and compares
with numpy.fft on longdouble frames:
  (a) element by element within the bound derived in generic_model's docstring (NaN fails); phase as angle(exp(i (got - want))) at
      the bins with |want| >= 1e-2 of the largest (at most 2 % of the bins may be left out), bound = asin((a) / |want|)
  (b) max |err| / max |want|: float32 <= 4e-6 (REG of tests/test_gpu_parity.py); float64 <= 8 x the same ratio of the model's
      float64 emulation on the same input against the same reference -- measured per case on the host against the reference, never
      against the kernel; the 8 allows for fused multiply-adds and another order inside a pass.  Without an 80-bit longdouble the
      reference is float64 numpy and (b) is skipped for float64 (the output says so).
The stride cases (more frames than workgroups at both gen_grid shapes, k_ola and k_filterbank_f64 past 4096 * 256 outputs) keep their
references on the device in float64 and assert the project's existing tolerances (1e-11 / 4e-6 of the largest output, 1e-14 for the
filterbank).  The refused float64 sizes must raise, name the limit and launch nothing.

The last test asserts that the cases that ran reached every id and prints each kernel's worst error / bound and worst error / the
emulation's error (DESIGN.md 4.8.4 quotes them).
"""
import numpy as np
import pytest
import torch

import generic_model as m
import kapre_amd as kapre
from kapre_amd import STFT, InverseSTFT, ApplyFilterbank, _ffi, backend

pytestmark = pytest.mark.gpu

REG32 = 4e-6              # tests/test_gpu_parity.py REG, tests/test_fuzz_gate.py REGRESSION
TOL64 = 1e-11             # tests/test_f64.py
FB64 = 1e-14              # tests/test_f64.py, ApplyFilterbank
FACTOR64 = 8.0            # float64: times the emulation's own error ratio
HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 1e-18

REACHED = set()           # branch ids of the cases that ran and passed
WORST = {}                # (kernel, figure) -> worst value
TORCH = {'f32': torch.float32, 'f64': torch.float64}
CTORCH = {'f32': torch.complex64, 'f64': torch.complex128}
CNAME = {'f32': 'float', 'f64': 'double'}


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
    return float(err.max() / max(float(np.abs(want).max()), 1e-300))


def check(kernel, c, err, bound, want, emu_err, use=None, regression=True):
    """(a) and (b) of the module docstring; emu_err: the float64 emulation's |error| on the same input (float64 cases)"""
    cid, ty = c['id'], c['ty']
    frac = fraction(err, bound, use)
    note(kernel, 'error / bound', frac)
    line = 'generic gate [%s] %s: worst error / bound = %.4f' % (kernel, cid, frac)
    got_ratio = ratio(err[use] if use is not None else err, want)
    limit = None
    if regression and ty == 'f32':
        limit = REG32
    elif regression and HAVE_LONGDOUBLE:
        emu_ratio = ratio(emu_err, want)
        limit = FACTOR64 * emu_ratio
        over = got_ratio / emu_ratio if emu_ratio > 0 else (0.0 if got_ratio == 0 else float('inf'))
        note(kernel, 'error / emulation error', over)
        line += ', max error / max = %.3g, emulation %.3g (x %.2f)' % (got_ratio, emu_ratio, over)
    elif regression:
        line += ' (no extended longdouble here: the float64 regression bound is skipped)'
    if limit is not None and ty == 'f32':
        note(kernel, 'max error / max (limit 4e-6)', got_ratio)
        line += ', max error / max = %.3g' % got_ratio
    print(line)
    assert frac <= 1.0, '%s %s: %.3g of the bound' % (kernel, cid, frac)
    if limit is not None:
        assert got_ratio <= limit, '%s %s: max error / max = %.3g, limit %.3g' % (kernel, cid, got_ratio, limit)


def by_id(cases):
    return {c['id']: c for c in cases}


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
STFT_TABLE = by_id(m.STFT_CASES)


def stft_layer(c):
    kw = dict(dtype='float64') if c['ty'] == 'f64' else {}
    return STFT(n_fft=c['n_fft'], win_length=c['win'], hop_length=c['hop'], pad_begin=c['pad_begin'], pad_end=c['pad_end'],
                input_data_format=c['in_fmt'], output_data_format=c['out_fmt'], **kw)


def run_stft(c, layer, xd):
    f_, k_ = m.frames_of(c), c['n_fft'] // 2 + 1
    poison(c['B'] * c['C'] * f_ * k_, CTORCH[c['ty']] if c['mode'] == m.COMPLEX else TORCH[c['ty']])
    got = layer(xd) if c['mode'] == m.COMPLEX else layer._run(xd, c['mode'])
    assert _ffi.last_launches() == 'k_stft_gen<%s>' % CNAME[c['ty']], _ffi.last_launches()
    assert tuple(got.shape) == m.shape_of(c['out_fmt'], c['B'], c['C'], f_, k_)
    assert got.dtype == (CTORCH[c['ty']] if c['mode'] == m.COMPLEX else TORCH[c['ty']])
    return got


@pytest.mark.parametrize('cid', [cid for cid, c in STFT_TABLE.items() if not c.get('stride') and not c.get('refused')])
def test_stft(cid):
    c = STFT_TABLE[cid]
    layer = stft_layer(c)
    x = m.stft_input(c)
    window = backend.window_values(layer.window_fn, c['win'], m.DT[c['ty']])           # the values the layer uploads
    xin = m.to_layout(x, c['in_fmt'])
    got = m.from_layout(run_stft(c, layer, torch.from_numpy(xin).cuda()).cpu().numpy(), c['out_fmt'])
    if HAVE_LONGDOUBLE:
        want, s = m.ref_stft(c, x, window)
    else:
        want, s = m.ref_stft(c, x.astype(np.float64), window.astype(np.float64))
    assert got.shape == want.shape
    err, use = m.stft_error(c, got, want)
    kernel = 'k_stft_gen<%s>' % CNAME[c['ty']] + ('' if c['mode'] == m.COMPLEX else ' magnitude' if c['mode'] == m.MAGNITUDE else ' phase')
    emu_err = None
    if c['mode'] == m.PHASE:
        left_out = 1.0 - float(use.mean())
        print('generic gate [%s] %s: %.2f %% of the bins left out' % (kernel, cid, 100 * left_out))
        assert left_out <= m.PHASE_LEFT_OUT
    elif c['ty'] == 'f64' and HAVE_LONGDOUBLE:
        emu = m.from_layout(m.emulate_stft(c, xin, window), c['out_fmt'])
        emu_err, _ = m.stft_error(c, emu, want)
    check(kernel, c, err, m.stft_bound(c, want, s), m.stft_want(c, want), emu_err, use if c['mode'] == m.PHASE else None,
          regression=c['mode'] != m.PHASE)
    kapre.check_device()
    REACHED.update(m.stft_branches(c))


def device_frames(c, xd_bct, window):
    """tf.signal.stft's frames of the logical (B, C, T) float64 device tensor, windowed and cropped: (B, C, F, min(win, n_fft))"""
    f_ = m.frames_of(c)
    if c['pad_begin']:
        xd_bct = torch.nn.functional.pad(xd_bct, (c['n_fft'] - c['hop'], 0))
    need = (f_ - 1) * c['hop'] + c['win']
    xd_bct = torch.nn.functional.pad(xd_bct, (0, max(0, need - xd_bct.shape[-1])))
    frames = xd_bct.unfold(-1, c['win'], c['hop'])[:, :, :f_] * window
    return frames[..., :c['n_fft']]


@pytest.mark.parametrize('cid', [cid for cid, c in STFT_TABLE.items() if c.get('stride')])
def test_stft_with_more_frames_than_workgroups(cid):
    """gen_grid launches at most 256 * per_cu workgroups (per_cu = 8 at n_fft 15, 1 at 160 KiB of LDS): the frame loop with its
    trailing barrier and reused buffers runs a second time.  Reference: x.unfold and torch.fft.rfft in float64 on the device"""
    c = STFT_TABLE[cid]
    pl = m.gen_fits(c['ty'], c['n_fft'])
    total = c['B'] * c['C'] * m.frames_of(c)
    grid, per_cu = m.gen_grid(total, pl['lds'])
    assert grid < total <= 2 * grid and per_cu in (1, m.GRID_PER_CU)
    layer = stft_layer(c)
    gen = torch.Generator(device='cuda').manual_seed(m.seed_of(c))
    x = torch.randn((c['B'], c['C'], c['T']), dtype=TORCH[c['ty']], device='cuda', generator=gen)
    xin = x.transpose(1, 2).contiguous() if c['in_fmt'] == m.CL else x
    got = run_stft(c, layer, xin)
    got = got.movedim(-1, 1) if c['out_fmt'] == m.CL else got
    window = torch.from_numpy(backend.window_values(layer.window_fn, c['win'], m.DT[c['ty']]).astype(np.float64)).cuda()
    want = torch.fft.rfft(device_frames(c, x.to(torch.float64), window), n=c['n_fft'], dim=-1)
    err = float((got.to(torch.complex128) - want).abs().max() / want.abs().max())
    err = err if err == err else float('inf')
    limit = TOL64 if c['ty'] == 'f64' else REG32
    print('generic gate [k_stft_gen<%s> frame loop] %s: %d frames on %d workgroups, max error / max = %.3g (limit %.0e)'
          % (CNAME[c['ty']], cid, total, grid, err, limit))
    note('k_stft_gen<%s> frame loop' % CNAME[c['ty']], 'max error / max (limit %.0e)' % limit, err)
    assert err <= limit
    kapre.check_device()
    REACHED.update(m.stft_branches(c))


@pytest.mark.parametrize('cid', [cid for cid, c in STFT_TABLE.items() if c.get('refused')])
def test_a_size_above_the_lds_limit_is_refused_before_any_launch(cid):
    c = STFT_TABLE[cid]
    assert m.gen_fits('f64', c['n_fft']) is None and m.gen_fits('f64', c['n_fft'] - 2) is not None
    xd = torch.from_numpy(m.to_layout(m.stft_input(c), c['in_fmt'])).cuda()
    with pytest.raises(RuntimeError, match=r'does not fit in LDS \(limit 10240 even / 5120 odd\)'):
        stft_layer(c)(xd)
    assert _ffi.last_launches() == ''
    spec = torch.zeros((1, 1, 2, c['n_fft'] // 2 + 1), dtype=torch.complex128, device='cuda')
    with pytest.raises(RuntimeError, match=r'does not fit in LDS \(limit 10240 even / 5120 odd\)'):
        InverseSTFT(n_fft=c['n_fft'], hop_length=c['n_fft'], input_data_format=m.CF, output_data_format=m.CF, dtype='float64')(spec)
    assert _ffi.last_launches() == ''
    assert _ffi.device_status() == 0
    kapre.check_device()
    REACHED.update(m.stft_branches(c))


# ---------------------------------------------------------------------------------------------
# inverse
# ---------------------------------------------------------------------------------------------
ISTFT_TABLE = by_id(m.ISTFT_CASES + m.OLA_CASES)


def istft_layer(c, synth):
    kw = dict(dtype='float64') if c['ty'] == 'f64' else {}
    layer = InverseSTFT(n_fft=c['n_fft'], win_length=c['win'], hop_length=c['hop'], input_data_format=c['spec_fmt'],
                        output_data_format=c['wave_fmt'], **kw)
    # a synthesis window without zeros (tf's inverse_stft_window_fn divides by the overlapped squares: 0 / 0 at hop >= win)
    layer.window_fn = lambda n, dtype=np.float32: np.asarray(synth, dtype)
    return layer


def run_istft(c, layer, sd):
    t_out = (c['F'] - 1) * c['hop'] + c['win']
    poison(c['B'] * c['C'] * t_out, TORCH[c['ty']])
    got = layer(sd)
    assert _ffi.last_launches() == 'k_irfft_gen<%s> + k_ola' % CNAME[c['ty']], _ffi.last_launches()
    assert tuple(got.shape) == m.shape_of(c['wave_fmt'], c['B'], c['C'], t_out) and got.dtype == TORCH[c['ty']]
    return got


@pytest.mark.parametrize('cid', [cid for cid, c in ISTFT_TABLE.items() if not c.get('stride')])
def test_istft(cid):
    c = ISTFT_TABLE[cid]
    spec, synth = m.istft_input(c), m.synth_window(c)
    sin = m.to_layout(spec, c['spec_fmt'])
    got = m.from_layout(run_istft(c, istft_layer(c, synth), torch.from_numpy(sin).cuda()).cpu().numpy(), c['wave_fmt'])
    want, bound = m.ref_istft(c, spec, synth)
    if not HAVE_LONGDOUBLE:
        want = want.astype(np.float64)
    assert got.shape == want.shape
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    emu_err = None
    if c['ty'] == 'f64' and HAVE_LONGDOUBLE:
        emu = m.from_layout(m.emulate_istft(c, sin, synth), c['wave_fmt'])
        emu_err = np.abs(emu.astype(np.longdouble) - want).astype(np.float64)
    check('k_irfft_gen<%s> + k_ola' % CNAME[c['ty']], c, err, bound, want, emu_err)
    kapre.check_device()
    REACHED.update(m.istft_branches(c))


@pytest.mark.parametrize('cid', [cid for cid, c in ISTFT_TABLE.items() if c.get('stride')])
def test_ola_past_the_grid_cap(cid):
    """263 000 frames of n_fft 15 at hop 4: k_ola takes a second output per thread (just over 4096 * 256 of them) and k_irfft_gen
    takes ~128 frames per workgroup.  Reference: torch.fft.irfft and 15 strided additions in float64 on the device"""
    c = ISTFT_TABLE[cid]
    f_, win, hop = c['F'], c['win'], c['hop']
    t_out = (f_ - 1) * hop + win
    assert m.GRID_1D_CAP * m.THREADS < t_out < m.GRID_1D_CAP * m.THREADS + 4096 and c['B'] * c['C'] == 1
    synth = m.synth_window(c)
    gen = torch.Generator(device='cuda').manual_seed(m.seed_of(c))
    spec = torch.view_as_complex(torch.randn((1, 1, f_, c['n_fft'] // 2 + 1, 2), dtype=TORCH[c['ty']], device='cuda', generator=gen))
    got = run_istft(c, istft_layer(c, synth), spec).view(-1)
    frames = torch.fft.irfft(spec.to(torch.complex128).view(f_, -1), n=c['n_fft'], dim=-1)[:, :win] * torch.from_numpy(synth.astype(np.float64)).cuda()
    want = torch.zeros(t_out, dtype=torch.float64, device='cuda')
    for j in range(win):
        want[j:j + (f_ - 1) * hop + 1:hop] += frames[:, j]
    err = float((got.to(torch.float64) - want).abs().max() / want.abs().max())
    err = err if err == err else float('inf')
    limit = TOL64 if c['ty'] == 'f64' else REG32
    print('generic gate [k_ola<%s> past the grid cap] %s: %d outputs, max error / max = %.3g (limit %.0e)' % (CNAME[c['ty']], cid, t_out, err, limit))
    note('k_irfft_gen<%s> + k_ola past the grid cap' % CNAME[c['ty']], 'max error / max (limit %.0e)' % limit, err)
    assert err <= limit
    kapre.check_device()
    REACHED.update(m.istft_branches(c))


# ---------------------------------------------------------------------------------------------
# float64 filterbank
# ---------------------------------------------------------------------------------------------
FB64_TABLE = by_id(m.FB64_CASES)


def fb64_layer(c, fb):
    layer = ApplyFilterbank('mel', dict(sample_rate=16000, n_freq=c['n_freq'], n_mels=c['n_filt']), data_format=c['fmt'], dtype='float64')
    layer.filterbank = fb                     # (n_freq, n_filt) float32, as the layer keeps it
    return layer


def run_fb64(c, layer, xd):
    poison(c['B'] * c['C'] * c['F'] * c['n_filt'], torch.float64)
    got = layer(xd)
    assert _ffi.last_launches() == 'k_filterbank_f64', _ffi.last_launches()
    assert tuple(got.shape) == m.shape_of(c['fmt'], c['B'], c['C'], c['F'], c['n_filt']) and got.dtype == torch.float64
    return got


@pytest.mark.parametrize('cid', [cid for cid, c in FB64_TABLE.items() if not c.get('stride')])
def test_filterbank_f64(cid):
    c = FB64_TABLE[cid]
    x, fb = m.fb64_input(c)
    got = m.from_layout(run_fb64(c, fb64_layer(c, fb), torch.from_numpy(m.to_layout(x, c['fmt'])).cuda()).cpu().numpy(), c['fmt'])
    want, bound = m.ref_fb64(c, x, fb)
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    frac = fraction(err, bound)
    print('generic gate [k_filterbank_f64] %s: worst error / bound = %.4f' % (cid, frac))
    note('k_filterbank_f64', 'error / bound', frac)
    assert frac <= 1.0
    assert ratio(err, want) <= FB64
    kapre.check_device()
    REACHED.update(m.fb64_branches(c))


def test_filterbank_f64_past_the_grid_cap():
    c = FB64_TABLE['stride cl 3->7']
    total = c['B'] * c['C'] * c['F'] * c['n_filt']
    assert m.GRID_1D_CAP * m.THREADS < total < m.GRID_1D_CAP * m.THREADS + 4096
    _, fb = m.fb64_input(m.shortened(c))
    gen = torch.Generator(device='cuda').manual_seed(m.seed_of(c))
    x = torch.randn(m.shape_of(c['fmt'], c['B'], c['C'], c['F'], c['n_freq']), dtype=torch.float64, device='cuda', generator=gen)
    got = run_fb64(c, fb64_layer(c, fb), x)
    want = torch.einsum('bfkc,km->bfmc', x, torch.from_numpy(fb.astype(np.float64)).cuda())
    err = float((got - want).abs().max() / want.abs().max())
    err = err if err == err else float('inf')
    print('generic gate [k_filterbank_f64 past the grid cap]: %d outputs, max error / max = %.3g (limit %.0e)' % (total, err, FB64))
    note('k_filterbank_f64 past the grid cap', 'max error / max (limit %.0e)' % FB64, err)
    assert err <= FB64
    kapre.check_device()
    REACHED.update(m.fb64_branches(c))


# ---------------------------------------------------------------------------------------------
# what this file reached
# ---------------------------------------------------------------------------------------------
def test_every_branch_was_reached():
    """runs last: the union of the branch ids of the cases above is BRANCHES minus the declared exclusions"""
    if not REACHED:
        pytest.skip('the cases above did not run in this session')
    print('generic gate, worst figures:')
    for kernel, figure in sorted(WORST):
        print('  %-44s %-36s %.4g' % (kernel, figure, WORST[kernel, figure]))
    assert REACHED >= set(m.BRANCHES) - set(m.EXCLUDED), sorted(set(m.BRANCHES) - set(m.EXCLUDED) - REACHED)
    assert REACHED <= set(m.BRANCHES), sorted(REACHED - set(m.BRANCHES))
