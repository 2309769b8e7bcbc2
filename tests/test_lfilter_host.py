"""LFilter without a GPU: the float64 model against scipy's cascades, the error budget on the library's chunked scan written in
numpy, the biquad designs, the carry matrices of kpr_lfilter_carry against an 80-digit recurrence, the plan, the layer surface
and the argument checks of the C entry points."""
import ctypes
import decimal
import os
import re

import numpy as np
import pytest
import scipy.signal

import kapre_amd as kapre
from kapre_amd import _ffi, backend
from conftest import REPO

import lfilter_model as lm

FILTERS = lm.test_filters()
RNG = np.random.default_rng(20261)


# ------------------------------------------------------------------ the model
def test_model_is_sosfilt_for_cascades():
    x = RNG.standard_normal((2, 3000))
    sos = np.concatenate([backend.biquad_sos('highpass', 16000, 80), backend.biquad_sos('peaking', 16000, 2000, 2.0, 6.0),
                          backend.biquad_sos('lowpass', 16000, 4000)])
    y = x
    for row in sos:
        y = lm.lfilter(y, lm.coef_of(row))
    want = scipy.signal.sosfilt(sos, x, axis=-1)
    # both are float64 recurrences over the same sections; sosfilt runs the transposed direct form II: a few roundings per
    # sample and section apart, carried on by filters whose impulse responses sum to less than 100
    assert np.max(np.abs(y - want)) <= 3 * 100 * 8 * 2.0 ** -53 * np.max(np.abs(want))


def test_zero_phase_is_sosfiltfilt_without_padding():
    """zero_phase = the cascade forward, then the cascade in reverse, from zero states.  sosfiltfilt(padtype=None) does the same
    from the steady-state initial conditions of its first sample (zi x[0]); those are linear in that sample, so their response r
    is added here and the comparison is exact up to float64 roundings."""
    x = RNG.standard_normal((2, 2500))
    sos = np.concatenate([backend.biquad_sos('highpass', 16000, 80), backend.biquad_sos('lowpass', 16000, 4000)])
    coefs = [lm.coef_of(row) for row in sos]
    zi = scipy.signal.sosfilt_zi(sos)
    r = scipy.signal.sosfilt(sos, np.zeros(x.shape[-1]), zi=zi)[0]           # the response to the initial state alone
    y = x
    for c in coefs:
        y = lm.lfilter(y, c)
    y = y + x[:, :1] * r
    last = y[:, -1:]
    for c in coefs:
        y = lm.lfilter(y, c, reverse=True)
    y = y + last * r[::-1]
    want = scipy.signal.sosfiltfilt(sos, x, axis=-1, padtype=None)
    # four passes per direction pair, a few roundings per sample each, carried on by impulse responses that sum to less than
    # 100; r itself reaches a few times the signal
    assert np.max(np.abs(y - want)) <= 4 * 100 * 8 * 2.0 ** -53 * np.max(np.abs(want))
    # and the model's own zero-phase cascade is that order of passes, rounded to float32 between launches
    x32 = x.astype(np.float32)
    z = x32
    for c in coefs:
        z = lm.lfilter(z, c).astype(np.float32)
    for c in coefs:
        z = lm.lfilter(z, c, reverse=True).astype(np.float32)
    assert np.array_equal(z, lm.cascade(x32, coefs, zero_phase=True))


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_budget_holds_for_the_chunked_scan_in_numpy(name):
    """the scan of kpr_lfilter_kernels.h in numpy float64 at the library's chunk sizes, carries from a long double recurrence:
    three segments and a ragged tail of unit noise, with and without an offset of 2, both forms, both directions"""
    coef = FILTERS[name]
    lane, wave, step, seg, _ = _ffi.lfilter_plan(1, 1, 100000, 'channels_first')
    n = 3 * seg + 777
    worst = 0.0
    for off in (0.0, 2.0):
        x = (RNG.standard_normal(n) + off).astype(np.float32)
        for segmented in (False, True):
            for reverse in (False, True):
                y = lm.chunked_scan(x, coef, lane, wave // lane, step // wave, seg // step, segmented, reverse)
                worst = max(worst, lm.worst_ratio(y.astype(np.float32), x, coef, reverse))
    print("chunked scan in numpy, %s: worst ratio %.4f" % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["hp5", "hp20", "lp30dbl", "deemph"])
def test_budget_holds_at_the_seams_in_numpy(name):
    """impulses and steps next to the seams, the segmented form included: the case that a scan carrying the direct form's state
    (y[t-1], y[t-2]) misses by a factor of five (an impulse on the last sample of a segment through the 5 Hz high-pass: the
    zero-state scan of the next segment is then 1e7 times the true output and has to cancel against the carried part)"""
    coef = FILTERS[name]
    lane, wave, step, seg, _ = _ffi.lfilter_plan(1, 1, 100000, 'channels_first')
    T = 3 * seg
    worst = 0.0
    for p in (0, 3, wave - 1, step - 1, seg - 2, seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, T - 1):
        for kind in ("impulse", "step"):
            x = np.zeros(T, dtype=np.float32)
            x[p if kind == "impulse" else slice(p, None)] = 1.0
            for segmented in (False, True):
                y = lm.chunked_scan(x, coef, lane, wave // lane, step // wave, seg // step, segmented)
                worst = max(worst, lm.worst_ratio(y.astype(np.float32), x, coef))
    print("chunked scan in numpy at the seams, %s: worst ratio %.4f" % (name, worst))
    assert worst <= 1.0


def test_float32_recurrence_fails_the_rule():
    """what makes the rule discriminating: a sequential float32 loop misses it by orders of magnitude on the 20 Hz high-pass"""
    coef = FILTERS['hp20']
    x = RNG.standard_normal(4000).astype(np.float32)
    b0, b1, b2, a1, a2 = (np.float32(v) for v in coef)
    y = np.zeros(4000, dtype=np.float32)
    for t in range(4000):
        y[t] = (b0 * x[t] + (b1 * x[t - 1] if t >= 1 else 0) + (b2 * x[t - 2] if t >= 2 else 0)
                - (a1 * y[t - 1] if t >= 1 else 0) - (a2 * y[t - 2] if t >= 2 else 0))
    assert lm.worst_ratio(y, x, coef) > 100.0


# ------------------------------------------------------------------ biquad designs
@pytest.mark.parametrize("kind", ["lowpass", "highpass"])
@pytest.mark.parametrize("fs,f", [(48000, 20.0), (16000, 80.0), (44100, 1000.0), (16000, 4000.0)])
def test_biquad_is_butterworth_at_q_sqrt_half(kind, fs, f):
    got = backend.biquad_sos(kind, fs, f, q=1.0 / np.sqrt(2.0))
    want = scipy.signal.butter(2, f, kind, fs=fs, output='sos')
    assert got.shape == (1, 6) and got.dtype == np.float64
    assert np.max(np.abs(got - want)) <= 1e-12


def _gain_db(sos, f, fs):
    w, h = scipy.signal.freqz(sos[0, :3], sos[0, 3:], worN=np.array([f], dtype=np.float64), fs=fs)
    return 20.0 * np.log10(np.abs(h[0]))


def test_biquad_frequency_responses():
    fs, f = 44100.0, 1000.0
    nyq = fs / 2.0
    q = 1.0 / np.sqrt(2.0)
    for kind in ("lowpass", "highpass"):
        assert abs(_gain_db(backend.biquad_sos(kind, fs, f, q), f, fs) - (-3.0103)) < 1e-4
    for g in (6.0, -9.0):
        pk = backend.biquad_sos('peaking', fs, f, 2.0, g)
        assert abs(_gain_db(pk, f, fs) - g) < 1e-9 and abs(_gain_db(pk, 0.0, fs)) < 1e-9 and abs(_gain_db(pk, nyq, fs)) < 1e-9
        assert abs(_gain_db(backend.biquad_sos('lowshelf', fs, f, q, g), 0.0, fs) - g) < 1e-9
        assert abs(_gain_db(backend.biquad_sos('highshelf', fs, f, q, g), nyq, fs) - g) < 1e-9
    assert _gain_db(backend.biquad_sos('notch', fs, f, 4.0), f, fs) < -200.0
    ap = backend.biquad_sos('allpass', fs, f, q)
    w, h = scipy.signal.freqz(ap[0, :3], ap[0, 3:], worN=512, fs=fs)
    assert np.max(np.abs(np.abs(h) - 1.0)) <= 1e-12
    assert abs(_gain_db(backend.biquad_sos('bandpass', fs, f, 3.0), f, fs)) < 1e-9
    for kind in backend.BIQUAD_KINDS:                            # every design is a stable section the layer takes
        backend.lfilter_sections(backend.biquad_sos(kind, fs, f, 0.9, 3.0))


def test_sos_from_ba():
    assert backend.sos_from_ba([1.0, -0.97], [1.0]).tolist() == [[1.0, -0.97, 0.0, 1.0, 0.0, 0.0]]
    assert backend.sos_from_ba(2.0, [1.0, -0.5, 0.25]).tolist() == [[2.0, 0.0, 0.0, 1.0, -0.5, 0.25]]
    for b, a in (([1, 2, 3, 4], [1]), ([1], [1, 2, 3, 4]), ([], [1])):
        with pytest.raises(ValueError, match="order <= 2"):
            backend.sos_from_ba(b, a)
    assert backend.lfilter_sections(backend.sos_from_ba([2.0, 1.0], [2.0, -1.0])) == ((1.0, 0.5, 0.0, -0.5, 0.0),)


# ------------------------------------------------------------------ carry matrices
def _chunk_lengths():
    lane, wave, step, seg, _ = _ffi.lfilter_plan(1, 1, 1 << 20, 'channels_first')
    lanes = wave // lane
    out = {0, 1, 2, lane, wave, step, seg}
    out.update(lane << k for k in range(int(np.log2(lanes))))    # the powers of two of the wave-level combine
    out.update(lane * i for i in range(lanes))                   # what a lane applies to its wave's carry-in
    return sorted(out)


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_carry_matrices_against_80_digits(name):
    """every entry within 2^-44 of the largest entry's magnitude: entries reach about 2^12 and M c cancels against l by up to about
    2^9 on these filters, and the carry's share must stay under 2^-24 / 32.  No plan length goes beyond 8192, where the long
    double recurrence measured <= 2.5e-15."""
    coef = FILTERS[name]
    worst = 0.0
    for n in _chunk_lengths():
        assert n <= 10 ** 4
        got = _ffi.lfilter_carry(coef, n).ravel()
        want = lm.carry_decimal(coef, n)
        with decimal.localcontext() as ctx:
            ctx.prec = 80
            top = max(abs(w) for w in want)
            err = max(abs(decimal.Decimal(float(g)) - w) for g, w in zip(got, want))
            # (a fast filter's M_8192 lies below the smallest float64: one step of the subnormal grid is all a double can do)
            err = max(err - decimal.Decimal(2) ** -1074, decimal.Decimal(0))
            rel = float(err / top) if top else float(err)
        worst = max(worst, rel)
        assert rel <= 2.0 ** -44, (name, n, rel)
    print("carry matrices, %s: worst relative error %.2e" % (name, worst))


def test_carry_matrix_is_the_power_of_the_companion_matrix():
    coef = FILTERS['bs1770']
    comp = np.array([[-coef[3], -coef[4]], [1.0, 0.0]])
    assert np.array_equal(_ffi.lfilter_carry(coef, 0), np.eye(2))
    assert np.array_equal(_ffi.lfilter_carry(coef, 1), comp)
    for n in (2, 5, 16, 64):
        assert np.allclose(_ffi.lfilter_carry(coef, n), np.linalg.matrix_power(comp, n), rtol=1e-12, atol=1e-15)


def test_repeated_squaring_is_not_good_enough():
    """the table of the issue: np.linalg.matrix_power in float64 on the 5 Hz high-pass at n = 8192 is about 1e-7 away"""
    coef = FILTERS['hp5']
    want = [float(v) for v in lm.carry_decimal(coef, 8192)]
    sq = np.linalg.matrix_power(np.array([[-coef[3], -coef[4]], [1.0, 0.0]]), 8192).ravel()
    top = max(abs(v) for v in want)
    assert max(abs(a - b) for a, b in zip(sq, want)) / top > 2.0 ** -44
    assert max(abs(a - b) for a, b in zip(_ffi.lfilter_carry(coef, 8192).ravel(), want)) / top <= 2.0 ** -44


def test_carry_argument_checks():
    L = _ffi.lib()
    m = (ctypes.c_double * 4)()
    ok = (ctypes.c_double * 5)(1.0, 0.0, 0.0, -0.5, 0.1)
    assert L.kpr_lfilter_carry(ok, 16, m) == 0
    assert L.kpr_lfilter_carry(ok, -1, m) == -1 and L.kpr_lfilter_carry(ok, (1 << 20) + 1, m) == -1
    assert L.kpr_lfilter_carry(None, 16, m) == -1 and L.kpr_lfilter_carry(ok, 16, None) == -1
    for a1, a2 in ((0.0, 1.0), (0.0, -1.0), (2.0, 0.999), (-1.5, 0.5), (1.5, 0.5), (float('nan'), 0.0)):
        bad = (ctypes.c_double * 5)(1.0, 0.0, 0.0, a1, a2)
        assert L.kpr_lfilter_carry(bad, 16, m) == -1, (a1, a2)
    assert b"stability triangle" in L.kpr_last_error() or b"finite" in L.kpr_last_error()
    with pytest.raises(ValueError, match="stability triangle"):
        _ffi.lfilter_carry((1.0, 0.0, 0.0, 0.0, 1.0), 4)


# ------------------------------------------------------------------ the plan
def test_plan_is_positive_consistent_and_monotone():
    for fmt in ("channels_first", "channels_last"):
        lane, wave, step, seg, form = _ffi.lfilter_plan(3, 2, 100000, fmt)
        assert min(lane, wave, step, seg) > 0 and form in (_ffi.LFILTER_WHOLE, _ffi.LFILTER_SEGMENTED)
        assert wave == 64 * lane and step % wave == 0 and seg % step == 0 and lane % 4 == 0
        for length in (1, seg, seg + 1, 160000, 1 << 20):
            forms = [_ffi.lfilter_plan(b, c, length, fmt)[4] for b, c in
                     ((1, 1), (2, 1), (2, 2), (3, 3), (16, 1), (16, 2), (64, 1), (127, 1), (64, 2), (128, 1), (256, 1), (512, 2), (4096, 1))]
            assert all(f in (1, 2) for f in forms)
            # segmented (2) for few series, whole-signal (1) from some count on, never back
            assert forms == sorted(forms, reverse=True), (length, forms)
            if length <= seg:
                assert set(forms) == {_ffi.LFILTER_WHOLE}            # one segment: nothing to cut
    assert _ffi.lfilter_plan(8, 1, 160000, 'channels_first')[4] == _ffi.LFILTER_SEGMENTED
    assert _ffi.lfilter_plan(1024, 1, 110250, 'channels_first')[4] == _ffi.LFILTER_WHOLE


def test_plan_follows_the_option():
    old = _ffi.set_option("lfilter_variant", 1)
    try:
        assert _ffi.lfilter_plan(2, 1, 100000, 'channels_first')[4] == _ffi.LFILTER_WHOLE
        _ffi.set_option("lfilter_variant", 2)
        assert _ffi.lfilter_plan(2048, 1, 100000, 'channels_first')[4] == _ffi.LFILTER_SEGMENTED
        assert _ffi.lfilter_plan(2048, 1, 100, 'channels_first')[4] == _ffi.LFILTER_WHOLE
        with pytest.raises(RuntimeError):
            _ffi.set_option("lfilter_variant", 3)
    finally:
        _ffi.set_option("lfilter_variant", old)
    assert old == 0


def test_launch_entry_argument_checks():
    """every call returns before a launch (no device here): the pointers are never dereferenced"""
    L = _ffi.lib()
    fake, dst, wsp, null = (ctypes.c_void_p(v) for v in (0x1000, 0x40000000, 0x80000000, 0))
    ok = (ctypes.c_double * 5)(1.0, -2.0, 1.0, -1.9, 0.95)

    def run(x=fake, batch=2, channels=1, length=100, layout=1, coef=ok, reverse=0, out=dst, ws=wsp, ws_bytes=1 << 20):
        return L.kpr_lfilter_f32(x, batch, channels, length, layout, coef, reverse, out, ws, ws_bytes, null)

    assert run(batch=0) == 0 and run(length=0) == 0 and run(batch=0, x=null, out=null) == 0
    for bad in (dict(x=null), dict(out=null), dict(batch=-1), dict(channels=0), dict(length=-1), dict(layout=2), dict(reverse=2),
                dict(coef=None), dict(out=fake), dict(x=ctypes.c_void_p(0x1002)), dict(out=ctypes.c_void_p(0x1004 + 100)),
                dict(coef=(ctypes.c_double * 5)(1.0, 0.0, 0.0, 0.0, 1.0)), dict(coef=(ctypes.c_double * 5)(1.0, 0.0, 0.0, 2.0, 0.5)),
                dict(coef=(ctypes.c_double * 5)(float('inf'), 0.0, 0.0, 0.0, 0.0))):
        assert run(**bad) == -1, bad
    assert run(length=1 << 30) == -2 and b"2^30" in L.kpr_last_error()
    assert run(length=1 << 29, channels=2) == -2 and run(length=1 << 29, channels=2, layout=0) != -2
    # the segmented form (two series of 100000 samples) needs its workspace
    need = L.kpr_lfilter_workspace_bytes(2, 1, 100000, 1)
    seg = _ffi.lfilter_plan(2, 1, 100000, 'channels_last')[3]
    assert need == 2 * -(-100000 // seg) * 32 and L.kpr_lfilter_workspace_bytes(2, 1, seg, 1) == 0
    assert L.kpr_lfilter_workspace_bytes(-1, 1, 10, 0) == -1
    assert run(length=100000, ws=null) == -4 and run(length=100000, ws_bytes=need - 1) == -4
    assert b"workspace" in L.kpr_last_error()
    assert run(length=100000, ws=ctypes.c_void_p(0x80000004), ws_bytes=need) == -4
    assert run(length=100000, ws=ctypes.c_void_p(0x1000 + 64), ws_bytes=need) == -1 and b"overlaps" in L.kpr_last_error()


# ------------------------------------------------------------------ the layers
@pytest.mark.parametrize("fmt", ["channels_last", "channels_first"])
def test_config_round_trip_and_output_shape(fmt):
    sos = np.concatenate([backend.biquad_sos('highpass', 16000, 80), backend.biquad_sos('highshelf', 16000, 3000, gain_db=4.0)])
    layer = kapre.LFilter(sos, zero_phase=True, data_format=fmt, name="eq")
    config = layer.get_config()
    assert config["sos"] == sos.tolist() and config["zero_phase"] is True and config["data_format"] == fmt and config["name"] == "eq"
    assert all(type(v) is float for row in config["sos"] for v in row)
    import json
    again = kapre.LFilter.from_config(json.loads(json.dumps(config)))
    assert again.get_config() == config
    assert kapre.LFilter(sos[0]).get_config()["sos"] == [sos[0].tolist()]        # (6,) is one section
    from kapre_amd.keras_shim import get_registered_object
    for cls in (kapre.LFilter, kapre.Preemphasis, kapre.Deemphasis):
        assert get_registered_object("Kapre>" + cls.__name__) is cls
    for T in (0, 1, 441, None):
        shape = _ffi.shape_of(fmt, None, 2, T)
        assert layer.compute_output_shape(shape) == shape
    model = kapre.Sequential([kapre.Preemphasis(0.95, input_shape=_ffi.shape_of(fmt, 0, 1, 22050)[1:], data_format=fmt)])
    assert model.output_shape == _ffi.shape_of(fmt, None, 1, 22050)


def test_emphasis_layers():
    pre, de = kapre.Preemphasis(), kapre.Deemphasis(0.9, data_format="channels_first")
    assert pre.sos == [[1.0, -0.97, 0.0, 1.0, 0.0, 0.0]] and de.sos == [[1.0, 0.0, 0.0, 1.0, -0.9, 0.0]]
    c = pre.get_config()
    assert c["coef"] == 0.97 and c["data_format"] == "default" and "sos" not in c
    assert kapre.Preemphasis.from_config(c).get_config() == c
    c = de.get_config()
    assert c["coef"] == 0.9 and kapre.Deemphasis.from_config(c).sos == de.sos
    assert isinstance(pre, kapre.LFilter) and isinstance(de, kapre.LFilter)
    for bad in (1.0, -1.5, "0.97", True, float("nan")):
        with pytest.raises(ValueError, match="coef"):
            kapre.Preemphasis(bad)
        with pytest.raises(ValueError, match="coef"):
            kapre.Deemphasis(bad)


def test_validation_errors():
    good = [1.0, 0.0, 0.0, 1.0, -0.5, 0.0]
    for bad in ([1.0, 0.0, 0.0], np.zeros((2, 5)), np.zeros((0, 6)), np.zeros((2, 2, 6)), [good] * 9, "sos", None):
        with pytest.raises(ValueError, match="sos must"):
            kapre.LFilter(bad)
    with pytest.raises(ValueError, match="a0 = 0"):
        kapre.LFilter([1.0, 0.0, 0.0, 0.0, 0.5, 0.0])
    with pytest.raises(ValueError, match="finite"):
        kapre.LFilter([1.0, float("inf"), 0.0, 1.0, 0.5, 0.0])
    for a1, a2 in ((0.0, 1.0), (0.0, -1.0), (2.0, 0.999), (-1.5, 0.5), (1.5, 0.5), (-2.0, 1.0)):
        with pytest.raises(ValueError, match="not stable"):
            kapre.LFilter([1.0, 0.0, 0.0, 1.0, a1, a2])
        with pytest.raises(ValueError, match="not stable"):
            backend.lfilter(np.zeros((1, 8, 1), dtype=np.float32), [2.0, 0.0, 0.0, 2.0, 2 * a1, 2 * a2])
    with pytest.raises(TypeError, match="float32"):
        kapre.LFilter(good)(np.zeros((1, 8, 1), dtype=np.float64))
    with pytest.raises(TypeError, match="float32"):
        backend.lfilter(np.zeros((1, 8, 1), dtype=np.float64), good)
    with pytest.raises(ValueError, match="rank-3"):
        kapre.LFilter(good)(np.zeros((8, 1), dtype=np.float32))
    with pytest.raises(ValueError, match="data_format must be one of"):
        kapre.LFilter(good, data_format="channels_middle")
    for kw in (dict(freq=0.0), dict(freq=8000.0), dict(freq=9000.0), dict(freq=-1.0), dict(q=0.0), dict(q=-1.0),
               dict(freq=float("nan")), dict(gain_db=float("inf"))):
        with pytest.raises(ValueError, match="biquad_sos"):
            backend.biquad_sos('lowpass', **{**dict(sample_rate=16000, freq=100.0), **kw})
    with pytest.raises(ValueError, match="kind must be one of"):
        backend.biquad_sos('brickwall', 16000, 100.0)


def test_exports():
    for name in ("LFilter", "Preemphasis", "Deemphasis"):
        assert name in kapre.__all__ and name in kapre.signal.__all__
        assert getattr(kapre, name) is getattr(kapre.signal, name)
    for name in ("lfilter", "sos_from_ba", "biquad_sos"):
        assert callable(getattr(backend, name))


def test_install_as_kapre_module_names():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import kapre_amd; kapre_amd.install_as_kapre(); "
            "from kapre.signal import LFilter, Preemphasis, Deemphasis; from kapre import LFilter as L2; "
            "from kapre.backend import lfilter, biquad_sos, sos_from_ba; assert L2 is LFilter; print('ok')" % REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "ok"


def test_header_prototypes_exports_and_documents():
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("kpr_lfilter_plan", "kpr_lfilter_carry", "kpr_lfilter_workspace_bytes", "kpr_lfilter_f32"):
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, code), name
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
    assert _ffi.EXPORTS["kpr_lfilter_f32"][1][-1] is ctypes.c_void_p             # the stream comes last
    assert "lfilter_variant" in text and _ffi.lib().kpr_version() == 120
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "kpr_lfilter_kernels.h" in readme and "lfilter_variant" in readme


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='lfilter expects a rank-3 waveform batch'):
        kapre.LFilter([1.0, 0.0, 0.0, 1.0, 0.5, 0.0])(np.zeros((8, 1), np.float32))
    with pytest.raises(TypeError, match='lfilter takes float32 waveforms'):
        kapre.LFilter([1.0, 0.0, 0.0, 1.0, 0.5, 0.0])(np.zeros((1, 8, 1), np.float64))
    with pytest.raises(ValueError, match='lfilter expects a rank-3 waveform batch'):
        kapre.LFilter([1.0, 0.0, 0.0, 1.0, 0.5, 0.0])(np.zeros((8, 1), np.float64))
    with pytest.raises(ValueError, match='lfilter expects a rank-3 waveform batch'):
        backend.lfilter(np.zeros((8, 1), np.float32), [1.0, 0.0, 0.0, 1.0, 0.5, 0.0])
    with pytest.raises(TypeError, match='lfilter takes float32 waveforms'):
        backend.lfilter(np.zeros((1, 8, 1), np.float64), [1.0, 0.0, 0.0, 1.0, 0.5, 0.0])
    with pytest.raises(ValueError, match='lfilter expects a rank-3 waveform batch'):
        backend.lfilter(np.zeros((8, 1), np.float64), [1.0, 0.0, 0.0, 1.0, 0.5, 0.0])
