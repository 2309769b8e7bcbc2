"""GPU tests of the mu-law kernels and of ConcatenateFrequencyMap (kapre_amd/csrc/kpr_companding_kernels.h) against the float64
value of the reference's formulas and the fixtures tools/make_golden_companding.py wrote from the reference's own code.

ENCODE.  v = the float64 value of (sign(x) log1p(mu |x|) / log1p(mu) + 1) / 2 mu + 0.5, c64 = trunc(v), d = |v - round(v)|:
(a) |code - c64| <= 1 everywhere, (b) code == c64 wherever d >= Q 2^-21 (8 float32 ulps of a value of size Q), (c) x == 0 gives
exactly trunc(mu / 2 + 0.5), (d) codes in 0 .. Q - 1 for |x| <= 1.  What (b) leaves out is capped -- 1 % of the elements for
Q <= 1024, 10 % for Q = 65536 (there the guard is 1/32 of a code width) -- and the cap is asserted on the inputs themselves.

DECODE.  Bound per Q = 4 x the largest deviation of the reference formula evaluated in numpy float32 from float64 over the same
codes (the device's exp differs from numpy's, and the exponent amplifies its error by up to ln Q = 11); every test prints the
measured figures next to the bound (DESIGN 4.10 quotes them).

DECODE BACKWARD.  Relative bound 2^-19: the float32 rounding of k = 2 code - mu moves the exponent |k| log2(Q) / mu <= 16 by up to
16 x 2^-24 (6.6e-7 of the result after the factor ln 2), four more roundings and a 1-ulp exp2 add 3.6e-7; twice the sum.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, speech

pytestmark = pytest.mark.gpu

QS = (2, 16, 256, 1024, 65536)
BADARG = -1


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'companding_cases.npz'))


def _torch():
    import torch
    return torch


def enc_v64(x, q):
    x = np.asarray(x, np.float64)
    mu = q - 1.0
    return (np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu) + 1) / 2.0 * mu + 0.5


def dec_ref(codes, q, dtype):
    """the reference's decoder (backend.py:334-340) with every operation in `dtype`"""
    mu = dtype(q - 1.0)
    s = (codes.astype(dtype) / mu) * dtype(2) - dtype(1)
    return np.sign(s) * (np.exp(np.abs(s) * np.log1p(mu)) - dtype(1)) / mu


def encode_inputs():
    sp = speech(10 ** 9)
    return {'uniform': np.random.default_rng(1234).uniform(-1, 1, 1 << 22).astype(np.float32),
            'speech': sp, 'speech_x4_clipped': np.clip(sp * np.float32(4), -1, 1).astype(np.float32)}


def check_encode(x, code, q, label, capped=True):
    v = enc_v64(x, q)
    c64 = np.trunc(v)
    d = np.abs(v - np.round(v))
    guard = q * 2.0 ** -21
    inside = d < guard
    cap = 0.10 if q == 65536 else 0.01
    print('%s Q=%d: %.4f %% of %d elements inside the guard (cap %.0f %%)' % (label, q, 100 * inside.mean(), x.size, 100 * cap))
    assert not capped or inside.mean() <= cap, 'the inputs leave rule (b) too little to check'
    code = code.astype(np.int64)
    diff = np.abs(code - c64)
    print('%s Q=%d: max |code - c64| = %d, disagreements %d (all inside the guard: %s)'
          % (label, q, diff.max(), int((diff != 0).sum()), bool(inside[diff != 0].all())))
    assert diff.max() <= 1                                                     # (a)
    assert (code[~inside] == c64[~inside]).all()                               # (b)
    assert (code[x == 0] == int(np.trunc((q - 1) / 2.0 + 0.5))).all()          # (c)
    assert code.min() >= 0 and code.max() <= q - 1                             # (d)


@pytest.mark.parametrize('q', QS)
def test_encode_parity(q):
    import kapre_amd as kapre
    for label, x in encode_inputs().items():
        assert np.abs(x).max() <= 1
        code = kapre.backend.mu_law_encoding(x, q)
        assert code.dtype == _torch().int32 and tuple(code.shape) == x.shape
        check_encode(x, code.cpu().numpy(), q, label)
    kapre.check_device()


def test_encode_matches_the_reference_fixture_and_layer(fx):
    import kapre_amd as kapre
    x = fx['speech_x']
    for q in QS:
        want = fx['enc_q%d' % q]
        assert np.array_equal(np.trunc(enc_v64(x, q)).astype(np.int32), want)   # the formula above IS the reference's
        got = kapre.backend.mu_law_encoding(x, q).cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape
        # (a 4000-sample slice with 1.25 % exact zeros, which rule (c) pins: the cap belongs to the inputs of test_encode_parity)
        check_encode(x.ravel(), got.ravel(), q, 'fixture', capped=False)
    y = kapre.MuLawEncoding(256)(x)
    assert np.array_equal(y.cpu().numpy(), kapre.backend.mu_law_encoding(x, 256).cpu().numpy())
    ends = kapre.backend.mu_law_encoding(np.array([-1.0, 1.0, 0.0, -0.0], np.float32), 256).cpu().numpy()
    assert ends.tolist() == [0, 255, 128, 128]


def test_encode_heads_tails_views_empty_nan():
    torch = _torch()
    import kapre_amd as kapre
    from kapre_amd import _ffi
    q = 256
    base = np.random.default_rng(7).uniform(-1, 1, 5000).astype(np.float32)
    dev = torch.from_numpy(base).cuda()
    want_all = np.trunc(enc_v64(base, q))
    d = np.abs(enc_v64(base, q) - np.round(enc_v64(base, q)))
    sure = d >= q * 2.0 ** -21
    for off in (0, 1, 2, 3):
        for n in (0, 1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4093, 4096, 4099, 4997):
            view = dev[off:off + n]                                   # the input starts on any word
            assert n == 0 or view.data_ptr() % 16 == (dev.data_ptr() + 4 * off) % 16
            got = kapre.backend.mu_law_encoding(view, q).cpu().numpy()
            sel = sure[off:off + n]
            assert got.shape == (n,) and (got[sel] == want_all[off:off + n][sel]).all(), (off, n)
            assert (np.abs(got - want_all[off:off + n]) <= 1).all()
            # the OUTPUT starts on any word too (the launcher's own output is always aligned): the raw entry point, and the
            # words around the view stay as they were
            out = torch.full((n + 8,), -7, dtype=torch.int32, device='cuda')
            for ooff in (1, 2, 3):
                out.fill_(-7)
                _ffi._call('kpr_mu_law_encode_f32', dev.device, ctypes.c_void_p(view.data_ptr() if n else dev.data_ptr()), n, q,
                           ctypes.c_void_p(out.data_ptr() + 4 * ooff))
                o = out.cpu().numpy()
                assert (o[:ooff] == -7).all() and (o[ooff + n:] == -7).all(), (off, n, ooff)
                assert np.array_equal(o[ooff:ooff + n], got), (off, n, ooff)
    empty = kapre.backend.mu_law_encoding(np.zeros((0, 3), np.float32), q)
    assert tuple(empty.shape) == (0, 3) and empty.dtype == torch.int32
    assert tuple(kapre.backend.mu_law_decoding(empty, q).shape) == (0, 3)
    x = base[:1001].copy()
    x[[0, 5, 500, 1000]] = np.nan
    got = kapre.backend.mu_law_encoding(x, q).cpu().numpy()
    assert (got[[0, 5, 500, 1000]] == 0).all()
    ok = ~np.isnan(x) & sure[:1001]
    assert (got[ok] == want_all[:1001][ok]).all()
    kapre.check_device()                                              # a NaN is data, not a fault


@pytest.mark.parametrize('q', QS)
def test_decode_parity(q, fx):
    torch = _torch()
    import kapre_amd as kapre
    from kapre_amd import _ffi
    for label, codes, want in (('fixture', fx['enc_q%d' % q], fx['dec_q%d' % q]),
                               ('all codes', np.arange(q, dtype=np.int32), dec_ref(np.arange(q, dtype=np.int32), q, np.float64))):
        assert want.dtype == np.float64
        assert np.abs(dec_ref(codes, q, np.float64) - want).max() <= 1e-15       # the fixture is the float64 formula
        ref32 = dec_ref(codes, q, np.float32)
        assert ref32.dtype == np.float32
        ref_dev = float(np.abs(ref32.astype(np.float64) - want).max())
        bound = 4 * ref_dev
        for form, arg in (('int32', codes), ('float32', codes.astype(np.float32)), ('int64', codes.astype(np.int64)),
                          ('int16 / uint8 via torch', torch.from_numpy(codes.astype(np.int64)).to(torch.int16 if q <= 1024 else torch.int32))):
            got = kapre.backend.mu_law_decoding(arg, q)
            assert got.dtype == torch.float32 and tuple(got.shape) == codes.shape
            assert _ffi.last_launches() == 'k_mu_law_decode'                     # one launch
            dev = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
            print('decode Q=%d %s %s: numpy float32 deviates %.3e, bound %.3e, device deviates %.3e' % (q, label, form, ref_dev, bound, dev))
            assert dev <= bound, (q, label, form, dev, bound)
    y = kapre.MuLawDecoding(q)(fx['enc_q%d' % q])
    assert np.array_equal(y.cpu().numpy(), kapre.backend.mu_law_decoding(fx['enc_q%d' % q], q).cpu().numpy())
    kapre.check_device()


def test_round_trip_within_one_quantisation_step():
    import kapre_amd as kapre
    q, x = 256, speech(10 ** 9)
    codes = kapre.backend.mu_law_encoding(x, q)
    back = kapre.backend.mu_law_decoding(codes, q).cpu().numpy().astype(np.float64)
    c = codes.cpu().numpy().astype(np.int64)
    levels = dec_ref(np.arange(-1, q + 1), q, np.float64)                      # levels[c + 1] = decode(c)
    step = np.maximum(levels[c + 2] - levels[c + 1], levels[c + 1] - levels[c])
    err = np.abs(back - x.astype(np.float64))
    print('round trip Q=256: max error %.3e, largest step %.3e, max error / local step %.3f' % (err.max(), step.max(), (err / step).max()))
    assert (err <= step).all()


CFM_SHAPES = [(256, 83, 128, 1), (8, 42, 1025, 6), (3, 5, 1, 2), (2, 7, 513, 1), (2, 7, 513, 2), (2, 9, 201, 3), (2, 9, 201, 6),
              (1, 1, 2, 1), (5, 3, 7, 2), (1, 40, 1025, 3)]


def check_concat(x, y, fmt):
    b, c, t, f = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if fmt == 'channels_last' else x.shape
    if fmt == 'channels_last':
        assert y.shape == (b, t, f, c + 1)
        kept, fmap = y[..., :c], y[..., c]
    else:
        assert y.shape == (b, c + 1, t, f)
        kept, fmap = y[:, :c], y[:, c]
    assert kept.tobytes() == np.ascontiguousarray(x).tobytes()                  # bit for bit
    want = np.arange(f, dtype=np.float64) / (f - 1) if f > 1 else np.zeros(1)
    assert fmap.shape == (b, t, f)
    assert np.abs(fmap.astype(np.float64) - want).max() <= 2.0 ** -23
    assert (fmap[..., 0] == 0.0).all() and (fmap[..., -1] == (1.0 if f > 1 else 0.0)).all()
    assert (fmap == fmap[0, 0]).all()


@pytest.mark.parametrize('fmt', ['channels_last', 'channels_first'])
@pytest.mark.parametrize('shape', CFM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_concat_frequency_map(shape, fmt):
    import kapre_amd as kapre
    from kapre_amd import _ffi
    b, t, f, c = shape
    x = np.random.default_rng(b * 1000 + f).standard_normal(shape if fmt == 'channels_last' else (b, c, t, f)).astype(np.float32)
    x.ravel()[::97] = np.array([np.nan, np.inf, -0.0, 1e-42], np.float32)[np.arange(x.ravel()[::97].size) % 4]   # copied as bits
    layer = kapre.ConcatenateFrequencyMap(data_format=fmt)
    y = layer(x)
    assert _ffi.last_launches() == 'k_freq_map_concat'
    assert tuple(y.shape) == layer.compute_output_shape(x.shape)
    check_concat(x, y.cpu().numpy(), fmt)
    kapre.check_device()


def test_concat_views_start_on_any_word():
    torch = _torch()
    import kapre_amd as kapre
    from kapre_amd import _ffi
    for fmt, dims in (('channels_last', (3, 5, 7, 2)), ('channels_first', (3, 2, 5, 7))):
        n = int(np.prod(dims))
        b, c, t, f = _ffi.dims_of(dims, fmt)
        flat = torch.randn(n + 8, device='cuda')
        n_out = n // c * (c + 1)
        for off in (0, 1, 2, 3):
            x = flat[off:off + n].view(dims)                                     # a contiguous view that starts on word `off`
            want = kapre.ConcatenateFrequencyMap(data_format=fmt)(x.clone()).cpu().numpy()
            check_concat(x.cpu().numpy(), want, fmt)
            for ooff in (0, 1, 2, 3):
                out = torch.full((n_out + 8,), -7.0, device='cuda')
                _ffi._call('kpr_freq_map_concat_f32', x.device, ctypes.c_void_p(x.data_ptr()), b, c, t, f, _ffi.layout(fmt),
                           ctypes.c_void_p(out.data_ptr() + 4 * ooff))
                o = out.cpu().numpy()
                assert (o[:ooff] == -7).all() and (o[ooff + n_out:] == -7).all()
                assert o[ooff:ooff + n_out].tobytes() == want.tobytes(), (fmt, off, ooff)
                back = torch.full((n + 8,), -7.0, device='cuda')
                _ffi._call('kpr_freq_map_concat_bwd_f32', x.device, ctypes.c_void_p(out.data_ptr() + 4 * ooff), b, c, t, f,
                           _ffi.layout(fmt), ctypes.c_void_p(back.data_ptr() + 4 * off))
                o = back.cpu().numpy()
                assert (o[:off] == -7).all() and (o[off + n:] == -7).all()
                assert o[off:off + n].tobytes() == x.cpu().numpy().tobytes(), (fmt, off, ooff)
    kapre.check_device()


def test_concat_fixtures_and_sequential(fx):
    import kapre_amd as kapre
    from kapre_amd import Sequential, STFT, Magnitude, ConcatenateFrequencyMap
    for name, fmt in (('cfm_cl', 'channels_last'), ('cfm_cf', 'channels_first'), ('cfm_default', 'default'),
                      ('cfm_cl_onebin', 'channels_last')):
        x, want = fx[name + '_x'], fx[name + '_y']
        layer = ConcatenateFrequencyMap(data_format=fmt)
        got = layer(x).cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape
        check_concat(x, got, layer.data_format)
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
    wave = speech(8000).reshape(2, 4000, 1)
    for fmt in ('channels_last', 'channels_first'):
        xin = wave if fmt == 'channels_last' else np.ascontiguousarray(wave.transpose(0, 2, 1))
        kw = dict(n_fft=1024, hop_length=512, input_data_format=fmt, output_data_format=fmt, input_shape=xin.shape[1:])
        model = Sequential([STFT(**kw), Magnitude(), ConcatenateFrequencyMap(data_format=fmt)])
        plain = Sequential([STFT(**kw), Magnitude()])
        y, mag = model.predict(xin), plain.predict(xin)
        assert isinstance(y, np.ndarray) and y.dtype == np.float32
        assert y.shape == tuple(d for d in model.compute_output_shape(xin.shape)) and y.shape[1:] == model.output_shape[1:]
        check_concat(mag, y, fmt)
    kapre.check_device()


def test_decode_backward_matches_the_closed_form():
    torch = _torch()
    import kapre_amd as kapre
    rng = np.random.default_rng(11)
    for q in QS:
        mu = q - 1.0
        codes = np.concatenate([rng.uniform(0, mu, 4099), np.arange(min(q, 4096), dtype=np.float64)]).astype(np.float32)
        g = rng.standard_normal(codes.shape).astype(np.float32)
        x = torch.from_numpy(codes).cuda().requires_grad_(True)
        y = kapre.MuLawDecoding(q)(x)
        assert y.grad_fn is not None and y.dtype == torch.float32
        assert np.array_equal(y.detach().cpu().numpy(), kapre.backend.mu_law_decoding(codes, q).cpu().numpy())
        y.backward(torch.from_numpy(g).cuda())
        s = codes.astype(np.float64) / mu * 2 - 1
        want = g.astype(np.float64) * 2 * np.log1p(mu) / mu ** 2 * np.exp(np.abs(s) * np.log1p(mu))
        rel = np.abs(x.grad.cpu().numpy().astype(np.float64) - want) / np.abs(want)
        print('decode backward Q=%d: max relative deviation %.3e (bound %.3e)' % (q, rel.max(), 2.0 ** -19))
        assert rel.max() <= 2.0 ** -19
        # and the closed form is the derivative: central differences of the float64 formula
        eps = 1e-6
        num = (dec_ref(codes.astype(np.float64) + eps, q, np.float64) - dec_ref(codes.astype(np.float64) - eps, q, np.float64)) / (2 * eps)
        away = np.abs(s) > 1e-3                                              # |s| has a kink at 0
        assert np.allclose(num[away] * g[away], want[away], rtol=1e-5, atol=1e-9)
    kapre.check_device()


@pytest.mark.parametrize('fmt', ['channels_last', 'channels_first'])
def test_concat_backward_drops_the_map_channel(fmt):
    torch = _torch()
    import kapre_amd as kapre
    from kapre_amd import _ffi
    for shape in ((4, 9, 201, 3), (2, 5, 128, 1), (3, 7, 1, 2), (2, 83, 513, 2)):
        b, t, f, c = shape
        dims = shape if fmt == 'channels_last' else (b, c, t, f)
        x = torch.randn(dims, device='cuda', requires_grad=True)
        y = kapre.ConcatenateFrequencyMap(data_format=fmt)(x)
        assert y.grad_fn is not None
        g = torch.randn(y.shape, device='cuda')
        y.backward(g)              # (runs on autograd's thread: kpr_last_launches is per thread, the ABI test reads the name)
        want = g[..., :c] if fmt == 'channels_last' else g[:, :c]
        assert x.grad.shape == x.shape and x.grad.cpu().numpy().tobytes() == want.contiguous().cpu().numpy().tobytes()
    kapre.check_device()


def test_encoding_ends_the_tape():
    torch = _torch()
    import kapre_amd as kapre
    x = torch.rand(2, 1000, 1, device='cuda', requires_grad=True)
    y = kapre.MuLawEncoding(256)(x)
    assert y.dtype == torch.int32 and y.grad_fn is None and not y.requires_grad
    plain = torch.rand(2, 1000, 1, device='cuda')
    assert kapre.MuLawDecoding(256)(y).grad_fn is None
    assert kapre.ConcatenateFrequencyMap()(torch.rand(2, 5, 8, 1, device='cuda')).grad_fn is None
    assert kapre.MuLawDecoding(256)(plain * 255).grad_fn is None


def test_abi_argument_checks_and_launch_names():
    torch = _torch()
    from kapre_amd import _ffi
    L = _ffi.lib()
    buf = torch.zeros(64, device='cuda')
    ibuf = torch.zeros(64, dtype=torch.int32, device='cuda')
    p, ip, null, st = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(ibuf.data_ptr()), ctypes.c_void_p(0), _ffi.current_stream_ptr()
    keep = torch.zeros(128, device='cuda')
    out = ctypes.c_void_p(keep.data_ptr())
    mu_calls = {
        'kpr_mu_law_encode_f32': lambda a, o, q, n=16: L.kpr_mu_law_encode_f32(a, n, q, o, st),
        'kpr_mu_law_decode_i32': lambda a, o, q, n=16: L.kpr_mu_law_decode_i32(a, n, q, o, st),
        'kpr_mu_law_decode_f32': lambda a, o, q, n=16: L.kpr_mu_law_decode_f32(a, n, q, o, st),
        'kpr_mu_law_decode_bwd_f32': lambda a, o, q, n=16: L.kpr_mu_law_decode_bwd_f32(a, p, n, q, o, st),
    }
    names = {'kpr_mu_law_encode_f32': 'k_mu_law_encode', 'kpr_mu_law_decode_i32': 'k_mu_law_decode',
             'kpr_mu_law_decode_f32': 'k_mu_law_decode', 'kpr_mu_law_decode_bwd_f32': 'k_mu_law_decode_bwd'}
    for name, call in mu_calls.items():
        src = ip if name.endswith('_i32') else p
        assert call(null, out, 256) == BADARG and b'NULL' in L.kpr_last_error(), name
        assert call(src, null, 256) == BADARG and b'NULL' in L.kpr_last_error(), name
        for q in (1, 0, -3, 65537):
            assert call(src, out, q) == BADARG and b'quantization_channels' in L.kpr_last_error(), (name, q)
        assert call(src, out, 256, n=-1) == BADARG
        assert call(src, out, 256, n=(1 << 40) + 1) == -2 and b'2^40' in L.kpr_last_error()       # the stated limit, before any launch
        assert call(null, null, 256, n=0) == 0 and _ffi.last_launches() == ''
        assert call(src, out, 256) == 0 and _ffi.last_launches() == names[name], name
    assert L.kpr_mu_law_decode_bwd_f32(p, null, 16, 256, out, st) == BADARG
    for name in ('kpr_freq_map_concat_f32', 'kpr_freq_map_concat_bwd_f32'):
        fn = getattr(L, name)
        assert fn(null, 1, 1, 4, 8, 1, out, st) == BADARG and b'NULL' in L.kpr_last_error()
        assert fn(p, 1, 1, 4, 8, 1, null, st) == BADARG and b'NULL' in L.kpr_last_error()
        assert fn(p, 1, 0, 4, 8, 1, out, st) == BADARG and fn(p, 1, 1, 4, 0, 1, out, st) == BADARG
        assert fn(p, 1, 1, 4, 8, 2, out, st) == BADARG and fn(p, -1, 1, 4, 8, 1, out, st) == BADARG
        assert fn(p, 1, 1, 1 << 20, 1 << 11, 1, out, st) == -2 and b'2^31' in L.kpr_last_error()
        assert fn(p, 1, 1, 4, 8, 1, p, st) == BADARG and b'overlap' in L.kpr_last_error()
        assert fn(null, 0, 1, 4, 8, 1, null, st) == 0 and _ffi.last_launches() == ''
        assert fn(p, 1, 1, 4, 8, 1, out, st) == 0
        assert _ffi.last_launches() == ('k_freq_map_drop' if name.endswith('bwd_f32') else 'k_freq_map_concat')
    torch.cuda.synchronize()
    assert _ffi.device_status(raise_on_error=False) == 0
