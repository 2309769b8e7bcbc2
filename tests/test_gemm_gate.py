"""-m gpu: the forward gate of the generic GEMM k_gemm<AMODE, EPI> (kapre_amd/csrc/kpr_misc_kernels.h) in its five instances, and of
k_fill_cols behind the inverse one.  The kernel is what every family falls back to: the forward and inverse DFT of every float32
size without an FFT plan, the staged mel product, ApplyFilterbank on everything that is not thin.  The cases are the tables of
tests/gemm_model.py: the smallest shapes that cross the 64-row, 64-column and 16-deep tile edges of every instance, both paddings of
the frame accessor, windows shorter and longer than n_fft, k-ranges that differ from tile to tile, a 64-row tile with rows of two
batch items (tests/test_gemm_model_host.py proves on the CPU that the tables reach every id of gemm_model.BRANCHES and tell every
one-line mutant of the kernel from the reference).

Every case poisons the output allocation with NaN, runs through the layers, asserts that _ffi.last_launches() EQUALS the expected
list and holds every element to the bound derived in gemm_model's docstring (NaN fails), next to max |err| / max |want| <= 4e-6 (REG of
tests/test_gpu_parity.py).  References: numpy's FFT on longdouble frames.  The <A_PLAIN, E_PLAIN> cases have integer entries in
[-7, 7] (every partial sum below 2^24) and are compared bit for bit; the <A_CABS, *> instances read a spectrum that the stage
before them wrote into the call's workspace, which no entry point lets a caller fill, so they are held to their bounds.

The last test asserts that the cases that ran reached every id and prints each instance's worst error / bound and worst
max error / max (DESIGN.md 4.8.5 quotes them).
"""
import numpy as np
import pytest
import torch

import gemm_model as m
import generic_model as gm
import pointwise_model as pm
import kapre_amd as kapre
from kapre_amd import STFT, InverseSTFT, ApplyFilterbank, Magnitude, MagnitudeToDecibel, Phase, Sequential, _ffi

pytestmark = pytest.mark.gpu

REACHED = set()           # branch ids of the cases that ran and passed
WORST = {}                # (instance, figure) -> worst value
LD = gm.LD


def poison(numel, dtype):
    """the next torch.empty of this size is handed this block by the caching allocator: what a kernel leaves unwritten is NaN"""
    t = torch.full((int(numel),), float('nan'), dtype=dtype, device='cuda')
    del t


def note(instance, figure, value):
    value = value if value == value else float('inf')
    WORST[instance, figure] = max(WORST.get((instance, figure), 0.0), value)


def check(instance, cid, err, bound, want):
    """every element within its bound, and the project's regression limit"""
    err = np.nan_to_num(np.asarray(err, np.float64), nan=np.inf)
    frac = m.fraction(err, bound)
    ratio = float(err.max() / max(float(np.abs(want).max()), 1e-300))
    note(instance, 'error / bound', frac)
    note(instance, 'max error / max (limit 4e-6)', ratio)
    print('gemm gate [%s] %s: worst error / bound = %.4f, max error / max = %.3g' % (instance, cid, frac, ratio))
    assert frac <= 1.0, '%s %s: %.3g of the bound' % (instance, cid, frac)
    assert ratio <= m.REG, '%s %s: max error / max = %.3g' % (instance, cid, ratio)


def by_id(cases):
    return {c['id']: c for c in cases}


# ---------------------------------------------------------------------------------------------
# <A_FRAME, E_CPLX>: the forward DFT
# ---------------------------------------------------------------------------------------------
FWD = by_id(m.FWD_CASES)


def stft_layer(c):
    return STFT(n_fft=c['n_fft'], win_length=c['win'], hop_length=c['hop'], pad_begin=c['pad_begin'], pad_end=c['pad_end'],
                input_data_format=c['in_fmt'], output_data_format=c['out_fmt'])


def run_stft(c, x):
    f_, k_ = m.frames_of(c), c['n_fft'] // 2 + 1
    layer = stft_layer(c)
    window = np.asarray(layer.window_fn(c['win']), np.float32)                    # the values the layer uploads
    assert np.array_equal(window, m.hann(c['win']))
    poison(c['B'] * c['C'] * f_ * k_, torch.complex64)
    got = layer(torch.from_numpy(m.to_layout(x, c['in_fmt'])).cuda())
    assert _ffi.last_launches() == 'k_gemm', _ffi.last_launches()
    assert tuple(got.shape) == m.shape_of(c['out_fmt'], c['B'], c['C'], f_, k_) and got.dtype == torch.complex64
    return m.from_layout(got.cpu().numpy(), c['out_fmt']), window


@pytest.mark.parametrize('cid', list(FWD))
def test_forward_dft(cid):
    c = FWD[cid]
    x = m.stft_input(c)
    got, window = run_stft(c, x)
    want, _ = gm.ref_stft(c, x, window)
    assert got.shape == want.shape
    err = np.abs(m.parts(got).astype(LD) - m.parts(want)).astype(np.float64)
    check('k_gemm<A_FRAME, E_CPLX>', cid, err, m.stft_bound(c, x, window, m.build_dft_fwd(c['n_fft'])), m.parts(want).astype(np.float64))
    kapre.check_device()
    REACHED.update(m.emulate_stft(c, m.to_layout(x, c['in_fmt']), window)[1].branches)


def test_dc_and_nyquist_bins_of_a_real_frame_have_no_imaginary_part():
    """the sine column of the table holds exact zeros where the sine is zero: imag(X[0]) and imag(X[n_fft / 2]) are exact zeros, as
    numpy.fft.rfft's are, and the phase of a negative Nyquist bin is +pi (it was +pi or -pi by the sign of a 1e-15 residue)"""
    c = FWD[m.NYQUIST_CASE]
    x = m.stft_input(c)
    got, window = run_stft(c, x)
    want = np.fft.rfft(m.stft_frames(c, x, window), n=c['n_fft'], axis=-1)
    assert np.all(want.imag[..., 0] == 0) and np.all(want.imag[..., -1] == 0)
    assert np.all(got.imag[..., 0] == 0) and np.all(got.imag[..., -1] == 0), float(np.abs(got.imag[..., [0, -1]]).max())
    poison(got.size, torch.float32)
    phase = Sequential([stft_layer(c), Phase()])(torch.from_numpy(m.to_layout(x, c['in_fmt'])).cuda())
    assert _ffi.last_launches() == 'k_gemm + k_cplx_to_real', _ffi.last_launches()
    phase = m.from_layout(phase.cpu().numpy(), c['out_fmt'])
    for k in (0, -1):
        neg, pos = got.real[..., k] < 0, got.real[..., k] > 0
        assert neg.any() and pos.any()
        assert np.all(phase[..., k][neg] == np.float32(np.pi)) and np.all(phase[..., k][pos] == 0)
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# <A_CPLX, E_WINDOW>: the inverse DFT, k_fill_cols, k_ola
# ---------------------------------------------------------------------------------------------
INV = by_id(m.INV_CASES)


@pytest.mark.parametrize('cid', list(INV))
def test_inverse_dft(cid):
    c = INV[cid]
    spec, synth = m.istft_input(c), m.synth_window(c)
    layer = InverseSTFT(n_fft=c['n_fft'], win_length=c['win'], hop_length=c['hop'], input_data_format=c['spec_fmt'],
                        output_data_format=c['wave_fmt'])
    layer.window_fn = lambda n, dtype=np.float32: np.asarray(synth, dtype)       # a synthesis window without zeros
    t_out = (c['F'] - 1) * c['hop'] + c['win']
    sin = m.to_layout(spec, c['spec_fmt'])
    poison(c['B'] * c['C'] * t_out, torch.float32)
    got = layer(torch.from_numpy(sin).cuda())
    expected = 'k_gemm + k_fill_cols + k_ola' if c['win'] > c['n_fft'] else 'k_gemm + k_ola'
    assert _ffi.last_launches() == expected, _ffi.last_launches()
    assert tuple(got.shape) == m.shape_of(c['wave_fmt'], c['B'], c['C'], t_out) and got.dtype == torch.float32
    want, bound = m.ref_istft(c, spec, synth, m.build_dft_inv(c['n_fft']))
    err = np.abs(got.cpu().numpy().astype(LD) - want).astype(np.float64)
    check('k_gemm<A_CPLX, E_WINDOW>', cid, err, bound, want.astype(np.float64))
    kapre.check_device()
    REACHED.update(m.emulate_istft(c, sin, synth)[1].branches)


# ---------------------------------------------------------------------------------------------
# <A_PLAIN, E_PLAIN> with the raw k-ranges: exact
# ---------------------------------------------------------------------------------------------
FB = by_id(m.FB_CASES)


@pytest.mark.parametrize('cid', list(FB))
def test_filterbank_with_k_ranges_is_exact(cid):
    c = FB[cid]
    x, fb = m.fb_input(c)
    kr = _ffi.filterbank_kranges(fb)
    assert [tuple(int(v) for v in p) for p in np.asarray(kr).reshape(-1, 2)] == m.raw_kranges(fb)
    xd = torch.from_numpy(m.to_layout(x, c['fmt'])).cuda()
    poison(c['B'] * c['C'] * c['F'] * c['n_filt'], torch.float32)
    if m.thin_gemm_shape(c['n_freq'], c['n_filt']):                  # the layer hands these shapes no packed copy of the matrix
        layer = ApplyFilterbank('mel', dict(sample_rate=16000, n_freq=c['n_freq'], n_mels=c['n_filt']), data_format=c['fmt'])
        layer.filterbank = fb
        got = layer(xd)
    else:                                                             # the layer's call without its packed copy
        got = _ffi.freq_matmul(xd, c['fmt'], torch.from_numpy(fb).cuda(), None, kr)
    assert _ffi.last_launches() == 'k_gemm', _ffi.last_launches()
    want = m.oracle_fb(c, x, fb)
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    bad = int((got != want.astype(np.float32)).sum())                # NaN counts
    note('k_gemm<A_PLAIN, E_PLAIN>', 'elements that differ (exact cases)', bad)
    print('gemm gate [k_gemm<A_PLAIN, E_PLAIN>] %s: %d of %d elements differ' % (cid, bad, got.size))
    assert bad == 0
    kapre.check_device()
    REACHED.update(m.emulate_fb(c, m.to_layout(x, c['fmt']), fb)[1].branches)


# ---------------------------------------------------------------------------------------------
# <A_CABS, E_PLAIN>, <A_CABS, E_DB>: the staged mel product
# ---------------------------------------------------------------------------------------------
MEL = by_id(m.MEL_CASES)
STAGE_LABEL = {'gen': 'k_stft_gen<float>', 'gemm': 'k_gemm'}


def mel_chain(c, fb, db):
    bank = ApplyFilterbank('mel', dict(sample_rate=16000, n_freq=c['n_fft'] // 2 + 1, n_mels=8), data_format=c['out_fmt'])
    bank.filterbank = fb                                              # a bank set by hand
    layers = [stft_layer(c), Magnitude(), bank]
    if db is not None:
        layers.append(MagnitudeToDecibel(ref_value=db[0], amin=db[1], dynamic_range=db[2]))
    return Sequential(layers)


def run_mel(c, xd, fb, db):
    f_ = m.frames_of(c)
    poison(c['B'] * c['C'] * f_ * c['n_filt'], torch.float32)
    got = mel_chain(c, fb, db)(xd)
    label = STAGE_LABEL[m.mel_stage(c['n_fft'])] + ' + k_gemm'
    expected = label if db is None else 'k_stats_init + ' + label + ' + k_db_clamp'
    assert _ffi.last_launches() == expected, _ffi.last_launches()
    assert tuple(got.shape) == m.shape_of(c['out_fmt'], c['B'], c['C'], f_, c['n_filt']) and got.dtype == torch.float32
    return got.cpu().numpy()


@pytest.mark.parametrize('cid', list(MEL))
def test_staged_mel_product(cid):
    c = MEL[cid]
    x, fb = m.mel_input(c), m.mel_bank(c)
    window = m.hann(c['win'])
    xd = torch.from_numpy(m.to_layout(x, c['in_fmt'])).cuda()
    want, bound = m.mel_reference(c, x, window, fb)
    want, bound = m.to_layout(want, c['out_fmt']), m.to_layout(bound, c['out_fmt'])
    got = run_mel(c, xd, fb, None)
    check('k_gemm<A_CABS, E_PLAIN>', cid, np.abs(got.astype(np.float64) - want), bound, want)
    # decibels: run (a) with the floor off against the interval, run (b) from run (a)'s bits
    (ref, amin, _), dyn = m.DB_RUNS[0], m.DB_RUNS[1][2]
    fa = run_mel(c, xd, fb, m.DB_RUNS[0])
    lo, hi = m.db_interval(want, bound, m.DB_RUNS[0])
    frac = m.fraction(np.nan_to_num(np.abs(fa.astype(np.float64) - (lo + hi) / 2), nan=np.inf), (hi - lo) / 2)
    lin = np.abs(10.0 ** (fa.astype(np.float64) / 10.0) - np.maximum(want, float(pm.db_device_params(ref, amin)[0])))
    ratio = float(np.nan_to_num(lin, nan=np.inf).max() / np.abs(want).max())
    note('k_gemm<A_CABS, E_DB>', 'error / bound', frac)
    note('k_gemm<A_CABS, E_DB>', 'max error / max (limit 4e-6)', ratio)
    print('gemm gate [k_gemm<A_CABS, E_DB>] %s: worst error / bound = %.4f, max error / max (linear) = %.3g' % (cid, frac, ratio))
    assert frac <= 1.0 and ratio <= m.REG
    fb_ = run_mel(c, xd, fb, m.DB_RUNS[1])
    want_b = pm.db_expected_b(fa, dyn)
    assert (want_b > fa).any(), 'the floor of run (b) is not active'
    assert np.array_equal(fb_.view(np.uint32), want_b.view(np.uint32)), int((fb_.view(np.uint32) != want_b.view(np.uint32)).sum())
    kapre.check_device()
    spec = np.fft.rfft(m.stft_frames(c, x, window), n=c['n_fft'], axis=-1)
    for db in (None,) + m.DB_RUNS:
        REACHED.update(m.emulate_mel(c, spec, fb, db)[2].branches)


# ---------------------------------------------------------------------------------------------
# what this file reached
# ---------------------------------------------------------------------------------------------
def test_every_branch_was_reached():
    """runs last: the union of the branch ids of the cases above, with the ids whose cases tests/test_signal_gate.py runs
    (gemm_model.POINTERS), is BRANCHES minus the declared exclusion"""
    if not REACHED:
        pytest.skip('the cases above did not run in this session')
    print('gemm gate, worst figures:')
    for instance, figure in sorted(WORST):
        print('  %-28s %-40s %.4g' % (instance, figure, WORST[instance, figure]))
    reached = REACHED | set(m.POINTERS)
    assert reached >= set(m.BRANCHES) - set(m.EXCLUDED), sorted(set(m.BRANCHES) - set(m.EXCLUDED) - reached)
    assert reached <= set(m.BRANCHES), sorted(reached - set(m.BRANCHES))
