"""HPSS on the GPU (kpr_hpss_f32 / kpr_hpss_c64, kapre_amd.HPSS) against tests/hpss_model.py: the medians bit for bit on shapes
around the tile edges and on inputs full of ties, the masks and outputs within the float32 budget of the float64 model, the
complex form, selectors and layouts, NaN, refusals, and the STFT -> HPSS -> InverseSTFT chain on a tone with clicks."""
import ctypes

import numpy as np
import pytest

import hpss_model as hm
import kapre_amd as kapre
from kapre_amd import _ffi, backend

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WINDOWS = [(31, 31), (3, 31), (17, 7), (31, 3)]
KINDS = ["levels", "constant", "ramp", "random"]


def _axes(fmt):
    return (1, 2) if fmt == "channels_last" else (2, 3)


def _input(kind, b, ch, frames, freq, fmt, seed):
    """a (b, ch, frames, freq) float32 array in ``fmt``: 4 levels (nearly everything ties), a constant, a ramp that rises in time
    and falls in frequency, or 2^[-20, 20] with 30 % exact zeros"""
    rng = np.random.default_rng(seed)
    shape = (b, ch, frames, freq)
    if kind == "levels":
        x = rng.integers(0, 4, size=shape).astype(np.float32) * np.float32(0.25)
    elif kind == "constant":
        x = np.full(shape, 1.5, np.float32)
    elif kind == "ramp":
        t = np.arange(frames, dtype=np.float32)[:, None]
        f = np.arange(freq, dtype=np.float32)[None, :]
        x = np.broadcast_to(1.0 + t + (freq - f) * np.float32(2.0 ** -10), shape).astype(np.float32)
        x = x * np.arange(1, b * ch + 1, dtype=np.float32).reshape(b, ch, 1, 1)
    else:
        x = (2.0 ** rng.uniform(-20.0, 20.0, size=shape)).astype(np.float32)
        x[rng.random(shape) < 0.3] = 0.0
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1) if fmt == "channels_last" else x)   # (the ramp's strides are broadcast ones)


def _run(x, fmt, kh, kp, power=2.0, mh=1.0, mp=1.0, mode=_ffi.HPSS_VALUES, output="pair"):
    import torch
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).cuda()
    res = _ffi.hpss(xd, fmt, kh, kp, power, mh, mp, mode, output)
    return tuple(r.cpu().numpy() for r in res) if isinstance(res, tuple) else res.cpu().numpy()


@pytest.fixture(scope="module")
def tile():
    tf, tq = _ffi.hpss_plan(434, 513)
    assert (tf, tq) == (64, 64)                       # the shapes below are written around this tile
    return tf, tq


# frames x freq around the tile edges: {1, 2, 15, tf - 1, tf, tf + 1, tf + 16}, each value three times, 21 pairs
EDGE = [1, 2, 15, 63, 64, 65, 80]
SHAPES = [(EDGE[i], EDGE[(i + s) % 7]) for s in (0, 2, 5) for i in range(7)]


# ---- medians, exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_medians_exact(idx, tile):
    """H and P themselves (the launcher's HPSS_MEDIANS form) equal the model's selection bit for bit, the hard mask of power = inf
    -- which flips when one median is wrong -- and the plain outputs at power 1 follow"""
    frames, freq = SHAPES[idx]
    assert {t for t, _ in SHAPES} == {1, 2, 15, tile[0] - 1, tile[0], tile[0] + 1, tile[0] + 16}
    ch, fmt = 1 + idx % 3, ("channels_first", "channels_last")[idx % 2]
    ta, fa = _axes(fmt)
    for w, (kh, kp) in enumerate(WINDOWS):
        kind = KINDS[(idx + w) % 4]
        x = _input(kind, 2, ch, frames, freq, fmt, 1000 * idx + w)
        H, P = hm.medians(x, kh, kp, ta, fa)
        gh, gp = _run(x, fmt, kh, kp, mode=_ffi.HPSS_MEDIANS)
        assert gh.dtype == np.float32 and gh.shape == x.shape
        assert np.array_equal(gh.view(np.uint32), H.view(np.uint32)), (kind, kh, kp, "H")
        assert np.array_equal(gp.view(np.uint32), P.view(np.uint32)), (kind, kh, kp, "P")
        mh_, mp_ = _run(x, fmt, kh, kp, power=float("inf"), mode=_ffi.HPSS_MASKS)
        assert np.array_equal(mh_, (H > P).astype(np.float32)) and np.array_equal(mp_, (P > H).astype(np.float32)), (kind, kh, kp)
        # power 1, margins 1: where one median is zero and the other is not the mask is exactly 0 / 1, where both are equal and
        # not zero it is exactly 0.5 -- on the tied inputs that is most of the plane
        oh, op = _run(x, fmt, kh, kp, power=1.0)
        wh, wp = hm.hpss_model(x, kh, kp, 1.0, 1.0, 1.0, False, ta, fa)
        sure = (H == P) | (H == 0) | (P == 0)
        assert np.array_equal(oh[sure], wh[sure].astype(np.float32)) and np.array_equal(op[sure], wp[sure].astype(np.float32))
        assert np.all(np.abs(oh - wh) <= 16 * U * np.abs(wh)) and np.all(np.abs(op - wp) <= 16 * U * np.abs(wp))
    assert "k_hpss<" in _ffi.last_launches()


def test_instances_and_labels():
    x = _input("levels", 1, 1, 20, 20, "channels_first", 5)
    _run(x, "channels_first", 31, 3)
    assert _ffi.last_launches() == "k_hpss<31,f32>"
    _run(x, "channels_first", 15, 3)
    assert _ffi.last_launches() == "k_hpss<15,f32>"
    _run(x.astype(np.complex64), "channels_first", 17, 15)
    assert _ffi.last_launches() == "k_hpss<31,c64>"
    for kh, kp in ((15, 15), (3, 5), (7, 15), (13, 9)):                  # the 15-slot instance, against the same model
        for fmt in ("channels_first", "channels_last"):
            x = _input("levels", 2, 2, 70, 67, fmt, kh * kp)
            H, P = hm.medians(x, kh, kp, *_axes(fmt))
            gh, gp = _run(x, fmt, kh, kp, mode=_ffi.HPSS_MEDIANS)
            assert np.array_equal(gh, H) and np.array_equal(gp, P), (kh, kp, fmt)


# ---- values ----------------------------------------------------------------------------------------------------------------
VALUE_SHAPES = [(65, 80), (15, 63), (80, 1)]


def _value_share(power, limit_ulps):
    """the largest |err| / (2^-24 |model|) of harmonic, percussive, Mh and Mp over the inputs of this file"""
    worst = 0.0
    for s, (frames, freq) in enumerate(VALUE_SHAPES):
        for k, kind in enumerate(KINDS):
            fmt = ("channels_first", "channels_last")[(s + k) % 2]
            ta, fa = _axes(fmt)
            x = _input(kind, 2, 2, frames, freq, fmt, 77 + 10 * s + k)
            for kh, kp in ((31, 31), (17, 7)):
                for mh, mp in ((1.0, 1.0), (2.0, 3.0)):
                    for mask in (False, True):
                        want = hm.hpss_model(x, kh, kp, power, mh, mp, mask, ta, fa)
                        got = _run(x, fmt, kh, kp, power, mh, mp, _ffi.HPSS_MASKS if mask else _ffi.HPSS_VALUES)
                        for g, w in zip(got, want):
                            assert np.isfinite(g).all()
                            err = np.abs(g.astype(np.float64) - w)
                            nz = w != 0
                            assert np.all(g[~nz] == 0), (kind, kh, kp, mh, mp, mask)
                            worst = max(worst, float(np.max(err[nz] / (U * np.abs(w[nz])), initial=0.0)))
    print("HPSS power %g: largest error %.3f x 2^-24 |model| = %.3f of the limit %g" % (power, worst, worst / limit_ulps, limit_ulps))
    return worst


@pytest.mark.parametrize("power", [1.0, 2.0])
def test_values_power_1_2(power):
    """within 16 2^-24 |model| of the float64 model: 13 roundings of at most half an ulp from P mh to S M, rounded up to 16; the
    build's float32 division is correctly rounded (hipcc's default, no fast-math flag in build.py).  No value of these inputs
    is below 2^-20 other than exact zeros: nothing underflows, no absolute term."""
    assert _value_share(power, 16.0) <= 16.0


# Measured on an MI355X over these inputs, in units of 2^-24 |model|: 4.206 at power 0.5 and 7.112 at power 3; the limit is twice
# that, rounded up to a power of two -- 16 for both.
POWF_MEASURED = {0.5: 4.206, 3.0: 7.112}
POWF_LIMIT = {0.5: 16.0, 3.0: 16.0}


@pytest.mark.parametrize("power", [0.5, 3.0])
def test_values_other_powers(power):
    """a finite power other than 1 and 2 goes through powf, whose error the library does not own: the limit is twice the largest
    error measured on the GPU over these inputs, rounded up to a power of two"""
    assert _value_share(power, POWF_LIMIT[power]) <= POWF_LIMIT[power]


# ---- complex input ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["channels_first", "channels_last"])
def test_complex_input(fmt):
    import torch
    rng = np.random.default_rng(11)
    shape = (2, 2, 70, 65) if fmt == "channels_first" else (2, 70, 65, 2)
    d = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    d[rng.random(shape) < 0.2] = 0
    dd = torch.from_numpy(d).cuda()
    mag = kapre.Magnitude()(dd)
    for kh, kp, power, margin in ((31, 31, 2.0, 1.0), (17, 7, 1.0, (2.0, 3.0)), (5, 3, 3.0, 1.0)):
        lay = lambda **kw: kapre.HPSS(kernel_size=(kh, kp), power=power, margin=margin, data_format=fmt, **kw)
        # hp_abs forms |D| as k_cplx_to_real does (one fused multiply-add under the root): the medians of D are the medians of
        # Magnitude()(D) bit for bit, and so are the masks
        med_c, med_r = (_run(t, fmt, kh, kp, mode=_ffi.HPSS_MEDIANS) for t in (dd, mag))
        for a, b in zip(med_c, med_r):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        m_c, m_r = lay(mask=True)(dd), lay(mask=True)(mag)
        assert m_c.dtype == torch.float32 and torch.equal(m_c, m_r)
        out = lay()(dd)
        assert out.dtype == torch.complex64
        ax = 1 if fmt == "channels_first" else 3
        m = m_c.cpu().numpy()
        want = np.concatenate([d, d], axis=ax)
        got = out.cpu().numpy()
        assert np.array_equal(got.real, want.real * m) and np.array_equal(got.imag, want.imag * m)


# ---- selectors and layouts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_selectors_and_layouts(cplx):
    import torch
    x = _input("random", 2, 3, 66, 70, "channels_first", 21)
    if cplx:
        x = (x * np.exp(1j * np.random.default_rng(3).uniform(0, 6.28, x.shape))).astype(np.complex64)
    xf = torch.from_numpy(x).cuda()
    xl = xf.permute(0, 2, 3, 1).contiguous()
    args = dict(kernel_size=(17, 31), power=2.0, margin=(1.0, 2.0))
    for mask in (False, True):
        both = kapre.HPSS(output='both', mask=mask, data_format='channels_first', **args)(xf)
        assert both.shape == (2, 6, 66, 70) and both.grad_fn is None
        h = kapre.HPSS(output='harmonic', mask=mask, data_format='channels_first', **args)(xf)
        p = kapre.HPSS(output='percussive', mask=mask, data_format='channels_first', **args)(xf)
        as_bits = lambda t: torch.view_as_real(t) if t.is_complex() else t
        assert torch.equal(as_bits(both[:, :3]), as_bits(h)) and torch.equal(as_bits(both[:, 3:]), as_bits(p))
        bh, bp = backend.hpss(xf, mask=mask, data_format='channels_first', **args)
        assert torch.equal(as_bits(bh), as_bits(h)) and torch.equal(as_bits(bp), as_bits(p))
        last = kapre.HPSS(output='both', mask=mask, data_format='channels_last', **args)(xl)
        assert last.shape == (2, 66, 70, 6)
        assert torch.equal(as_bits(last.permute(0, 3, 1, 2).contiguous()), as_bits(both))
        lh, lp = backend.hpss(xl, mask=mask, data_format='channels_last', **args)
        assert torch.equal(as_bits(lh.permute(0, 3, 1, 2).contiguous()), as_bits(h))
        assert torch.equal(as_bits(lp.permute(0, 3, 1, 2).contiguous()), as_bits(p))
        # the same bits twice
        again = kapre.HPSS(output='both', mask=mask, data_format='channels_first', **args)(xf)
        assert torch.equal(as_bits(again), as_bits(both))
    g = xf.clone().requires_grad_(True) if not cplx else xf
    assert kapre.HPSS()(g).grad_fn is None and not kapre.HPSS()(g).requires_grad
    assert kapre.HPSS()(x).shape == (2, 3, 66, 140) and kapre.HPSS()(np.zeros((0, 4, 5, 1), np.float32)).shape == (0, 4, 5, 2)


def test_behind_a_fused_front_end():
    import torch
    wave = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 8000, 1)).astype(np.float32)).cuda()
    front = kapre.get_stft_magnitude_layer(input_shape=(8000, 1), n_fft=512, hop_length=128)
    model = kapre.Sequential(list(front.layers) + [kapre.HPSS(kernel_size=(17, 31))])
    out = model(wave)
    want = kapre.HPSS(kernel_size=(17, 31))(front(wave))
    assert out.shape == model.output_shape[1:] or tuple(out.shape[1:]) == tuple(model.output_shape[1:])
    assert torch.equal(out, want)


# ---- one NaN bin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["interior", "corner"])
@pytest.mark.parametrize("kh, kp", [(31, 31), (3, 17)])
def test_one_nan_bin(where, kh, kp):
    x = _input("random", 1, 1, 70, 80, "channels_first", 31) + np.float32(2.0 ** -20)
    t, f = (40, 66) if where == "interior" else (0, 0)
    x[0, 0, t, f] = np.nan
    y = x.copy()
    y[0, 0, t, f] = np.inf
    for power in (2.0, 0.5):
        got = _run(x, "channels_first", kh, kp, power)
        ref = _run(y, "channels_first", kh, kp, power)
        for g, r in zip(got, ref):
            nan = np.isnan(g)
            assert nan[0, 0, t, f] and nan.sum() == 1
            keep = np.ones(g.shape, bool)
            keep[0, 0, t, f] = False
            assert np.array_equal(g[keep].view(np.uint32), r[keep].view(np.uint32))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    L = _ffi.lib()
    x = torch.rand((2, 2, 40, 33), device="cuda")
    out = torch.empty((2, 4, 40, 33), device="cuda")
    plane = 40 * 33

    def call(xp, oh, op, out_ch, ch=2):
        return L.kpr_hpss_f32(ctypes.c_void_p(xp), 2, ch, 40, 33, 0, 31, 31, 2.0, 1.0, 1.0, 0, ctypes.c_void_p(oh), ctypes.c_void_p(op),
                              out_ch, None)

    o = out.data_ptr()
    assert call(x.data_ptr(), o, o + 2 * plane * 4, 4) == 0               # the stacked form: channels 0-1 and 2-3 of one tensor
    assert call(x.data_ptr(), o + 2 * plane * 4, o, 4) == 0
    assert call(x.data_ptr(), 0, 0, 2) == -1 and b"both" in L.kpr_last_error()
    assert call(x.data_ptr(), x.data_ptr(), 0, 2) == -1 and b"overlaps x" in L.kpr_last_error()
    assert call(x.data_ptr(), 0, x.data_ptr() + 4 * plane * 4 - 4, 2) == -1
    assert call(x.data_ptr(), o, o, 4) == -1 and b"overlap" in L.kpr_last_error()
    assert call(x.data_ptr(), o, o + plane * 4, 4) == -1                  # channels 0-1 and 1-2
    assert call(x.data_ptr(), o, o + 2 * plane * 4 + 4, 4) == -1          # not a whole number of channels
    assert call(x.data_ptr(), o, o + 3 * plane * 4, 4) == -1              # channels 3-4: past the tensor's four
    assert call(x.data_ptr(), o, o + 4, 2) == -1
    torch.cuda.synchronize()


# ---- past 2^31 elements ----------------------------------------------------------------------------------------------------
def test_offsets_past_two_to_the_31():
    """every offset is 64-bit: the last planes of a tensor of more than 2^31 elements equal the same planes run alone"""
    import torch
    n = 2 ** 31 // (64 * 65) + 3
    x = torch.rand((n, 1, 64, 65), device="cuda")
    assert x.numel() > 2 ** 31
    h = _ffi.hpss(x, "channels_first", 31, 31, 2.0, 1.0, 1.0, _ffi.HPSS_VALUES, "harmonic")
    tail = _ffi.hpss(x[-2:].contiguous(), "channels_first", 31, 31, 2.0, 1.0, 1.0, _ffi.HPSS_VALUES, "harmonic")
    head = _ffi.hpss(x[:2].contiguous(), "channels_first", 31, 31, 2.0, 1.0, 1.0, _ffi.HPSS_VALUES, "harmonic")
    assert torch.equal(h[-2:], tail) and torch.equal(h[:2], head)
    want = hm.hpss_model(x[-1:].cpu().numpy(), 31, 31, 2.0, 1.0, 1.0, False, 2, 3)[0]
    assert np.all(np.abs(tail[-1:].cpu().numpy() - want) <= 16 * U * np.abs(want))


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_tone_and_clicks_end_to_end():
    """one second of a steady tone plus three clicks through STFT -> HPSS -> InverseSTFT: around a click the percussive waveform
    carries more energy than the harmonic one, away from the clicks the harmonic one more than the percussive one; with margins
    1 the two spectrograms add up to S"""
    import torch
    sr, n_fft, hop = 16000, 512, 128
    t = np.arange(sr) / sr
    wave = (0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    clicks = (4000, 8000, 12000)
    for c in clicks:
        wave[c:c + 4] += np.float32(4.0) * np.array([1, -1, 1, -1], np.float32)     # energy 64; the tone has 16 in 128 samples
    w = torch.from_numpy(wave.reshape(1, sr, 1)).cuda()
    model = kapre.get_hpss_layer(n_fft=n_fft, hop_length=hop, output='both', input_shape=(sr, 1))
    out = model(w).cpu().numpy().astype(np.float64)
    assert out.shape[1:] == tuple(model.output_shape[1:]) and out.shape[2] == 2
    harm, perc = out[0, :, 0], out[0, :, 1]
    for c in clicks:
        near = slice(c - hop // 2, c + hop // 2)
        assert np.sum(perc[near] ** 2) > np.sum(harm[near] ** 2), c
    for a, b in ((1000, 3000), (5200, 6800), (9200, 10800), (13200, 15000)):
        assert np.sum(harm[a:b] ** 2) > np.sum(perc[a:b] ** 2), (a, b)
    # the single-output chains are the two halves
    only_h = kapre.get_hpss_layer(n_fft=n_fft, hop_length=hop, output='harmonic', input_shape=(sr, 1))(w).cpu().numpy()
    only_p = kapre.get_hpss_layer(n_fft=n_fft, hop_length=hop, output='percussive', input_shape=(sr, 1))(w).cpu().numpy()
    assert np.array_equal(only_h[0, :, 0], out[0, :, 0].astype(np.float32))
    assert np.array_equal(only_p[0, :, 0], out[0, :, 1].astype(np.float32))
    # harmonic + percussive = S within 2 2^-24 relative (margins 1: Mh + Mp = 1)
    S = kapre.get_stft_magnitude_layer(input_shape=(sr, 1), n_fft=n_fft, hop_length=hop, window_name='hann_window',
                                       pad_begin=False, pad_end=False, return_decibel=False)(w)
    h, p = backend.hpss(S)
    s64 = S.cpu().numpy().astype(np.float64)
    total = h.cpu().numpy().astype(np.float64) + p.cpu().numpy().astype(np.float64)
    share = float(np.max(np.abs(total - s64)[s64 > 0] / (2 * U * s64[s64 > 0])))
    print("harmonic + percussive against S: %.3f of 2 x 2^-24 relative" % share)
    assert np.all(np.abs(total - s64) <= 2 * U * s64)
