"""Convolve / Reverb on the GPU: k_spec_fir alone against the float64 model of tests/convolve_model.py, the whole three-launch
convolution against float64 np.convolve, the gradient, the chain in front of the fused mel launch, and the device draw.

Bounds, derived and not tuned:

* k_spec_fir: every component is a float32 FMA chain over 2 P terms, so
      |re(Y) - re(Y64)| <= (2 P + 1) 2^-24 sum_p (|Xr| |Hr| + |Xi| |Hi|) + 2^-149        (likewise for the imaginary part)
* end to end, per batch item: the figure max |y - y64| / (||h||_1 max |x|) is at most four times the same figure of the float32
  CPU model (convolve_model.overlap_save32: another FFT algorithm, no packed-math twiddles), and never above 1e-4.  The model's
  figure of an item is taken over the item's whole convolution, for every mode (see check_case for why, with the figures).

Measured on an MI355X: kernel, worst ratio to its bound 0.64 (P = 1), 0.15 (P = 16), 0.08 (P = 32); end to end, worst device figure
2.8e-7 against 2.7e-7 for the model, case by case between 0.94 and 2.1 times the model; gradient 4.2e-8 against 3.4e-8.
Every check prints its worst figure.  The seams come from kpr_spec_fir_plan.  Batch 3 unless stated."""
import os

import numpy as np
import pytest

import augment_model as am
import convolve_model as cm

pytestmark = pytest.mark.gpu

BATCH = 3
PARITY_LIMIT = 1e-4
RNG = np.random.default_rng(20263)


def to_np(t):
    return t.detach().cpu().numpy()


def to_layout(x_bct, fmt):
    """(b, c, t) -> the layout of ``fmt``, contiguous"""
    return np.array(np.moveaxis(x_bct, 1, 2) if fmt == "channels_last" else x_bct, order="C", copy=True)


def from_layout(y, fmt):
    return np.moveaxis(y, 2, 1) if fmt == "channels_last" else y


def crandn(*shape):
    return (RNG.standard_normal(shape) + 1j * RNG.standard_normal(shape)).astype(np.complex64)


def plan(P):
    from kapre_amd import _ffi
    return _ffi.spec_fir_plan(100, 129, P)


# (name, layout, channels, bins): inner = 1, 5, 129, 130 (one column; odd; odd; even = the 16-byte form), two channels sharing
# an item's filter, and channels_last with 2 and 3 channels of 129 bins (inner 258 = the 16-byte form with band_div 2, inner 387)
GEOMS = (("i1", "channels_first", 1, 1), ("i5", "channels_first", 1, 5), ("i129", "channels_first", 1, 129),
         ("i130", "channels_first", 1, 130), ("cf2x5", "channels_first", 2, 5), ("cl2x129", "channels_last", 2, 129),
         ("cl3x129", "channels_last", 3, 129))
P_VALUES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)


def run_fir(X4, fmt, H, idx, frames_out):
    """X4: numpy complex64 in the rank-4 layout of ``fmt``; returns numpy"""
    import torch
    from kapre_amd import _ffi
    xt = torch.from_numpy(X4).cuda()
    ht = torch.from_numpy(H).cuda()
    it = None if idx is None else torch.from_numpy(np.asarray(idx, dtype=np.int32)).cuda()
    return to_np(_ffi.spec_fir(xt, fmt, ht, it, frames_out))


def as_model(X4, fmt):
    """the rank-4 array as (items, per_item, frames, inner) and its band_div"""
    if fmt == "channels_last":
        b, t, m, c = X4.shape
        return X4.reshape(b, 1, t, m * c), c
    return X4, 1


def make_x(fmt, c, bins, frames):
    return crandn(BATCH, frames, bins, c) if fmt == "channels_last" else crandn(BATCH, c, frames, bins)


# ------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("P", P_VALUES)
def test_spec_fir_against_the_float64_model(P):
    R, W, _ = plan(P)
    S = R * W
    n_ir = BATCH
    worst = 0.0
    n = 0
    for name, fmt, c, bins in GEOMS:
        H = crandn(n_ir, P, bins)
        for frames_in in sorted({1, P - 1, S - 1, S, S + 1, 2 * S + 3}):
            X4 = make_x(fmt, c, bins, frames_in)
            Xm, band_div = as_model(X4, fmt)
            for frames_out in sorted({frames_in + P - 1, frames_in, frames_in - 1}):
                if frames_out < 1:
                    continue
                for idx in (None, [2, 0, 1], [1, 1, 1]):
                    Y = run_fir(X4, fmt, H, idx, frames_out)
                    Y64, bre, bim = cm.spec_fir64(Xm, H, idx, frames_out, band_div)
                    Ym, _ = as_model(Y, fmt)
                    assert Ym.shape == Y64.shape, (name, frames_in, frames_out)
                    k = (2 * P + 1) * 2.0 ** -24
                    rre = np.abs(Ym.real.astype(np.float64) - Y64.real) / (k * bre + 2.0 ** -149)
                    rim = np.abs(Ym.imag.astype(np.float64) - Y64.imag) / (k * bim + 2.0 ** -149)
                    r = float(max(rre.max(), rim.max()))
                    worst = max(worst, r)
                    n += 1
                    assert r <= 1.0, (name, P, frames_in, frames_out, idx, r)
    print("k_spec_fir P = %d: %d launches, worst |Y - Y64| / bound = %.4f" % (P, n, worst))


@pytest.mark.parametrize("P", (1, 3, 8, 9, 17, 32))
@pytest.mark.parametrize("geom", ("i5", "i130", "cl2x129"))
def test_spec_fir_seams(P, geom):
    """a unit frame 1 + 0i at row r gives the rows of H, bit for bit, at rows r ... r + P - 1 and +0 elsewhere: r at every chunk
    and super-block seam and its two neighbours, every r its own batch item of one launch"""
    _, fmt, c, bins = next(g for g in GEOMS if g[0] == geom)
    R, W, _ = plan(P)
    S = R * W
    frames_in = 2 * S + 3
    rows = sorted({r for s in range(0, frames_in + 1, R) for r in (s - 1, s, s + 1) if 0 <= r < frames_in})
    assert all(s in rows for s in (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, R - 1, R, R + 1))
    b = len(rows)
    H = crandn(1, P, bins)
    assert not np.any(H.real == 0) and not np.any(H.imag == 0)
    shape = (b, frames_in, bins, c) if fmt == "channels_last" else (b, c, frames_in, bins)
    X4 = np.zeros(shape, dtype=np.complex64)
    for i, r in enumerate(rows):
        if fmt == "channels_last":
            X4[i, r] = 1.0
        else:
            X4[i, :, r] = 1.0
    frames_out = frames_in + P - 1
    Y = run_fir(X4, fmt, H, None, frames_out)
    want = np.zeros(Y.shape, dtype=np.complex64)
    for i, r in enumerate(rows):
        if fmt == "channels_last":
            want[i, r:r + P] = H[0][:, :, None]
        else:
            want[i, :, r:r + P] = H[0][None]
    assert np.array_equal(Y.view(np.uint32), want.view(np.uint32))          # bits: the zeros are +0


@pytest.mark.parametrize("P", (1, 5, 16, 17))
def test_spec_fir_nan_stays_in_its_column(P):
    R, W, _ = plan(P)
    S = R * W
    for name, fmt, c, bins in (GEOMS[3], GEOMS[5]):
        frames_in, frames_out = S + 5, S + 5 + P - 1
        H = crandn(BATCH, P, bins)
        X4 = make_x(fmt, c, bins, frames_in)
        k, f = R - 1, bins // 2
        clean = X4.copy()
        pos = (1, k, f, c - 1) if fmt == "channels_last" else (1, c - 1, k, f)
        clean[pos] = 0
        X4[pos] = np.nan
        Y, Y0 = run_fir(X4, fmt, H, [0, 1, 2], frames_out), run_fir(clean, fmt, H, [0, 1, 2], frames_out)
        hit = np.zeros(Y.shape, dtype=bool)
        if fmt == "channels_last":
            hit[1, k:k + P, f, c - 1] = True
        else:
            hit[1, c - 1, k:k + P, f] = True
        assert np.array_equal(np.isnan(Y.real) | np.isnan(Y.imag), hit), name
        assert np.array_equal(Y[~hit].view(np.uint32), Y0[~hit].view(np.uint32)), name


def test_spec_fir_same_bits_and_clamped_index():
    import torch
    from kapre_amd import _ffi
    for P in (3, 16, 32):
        for name, fmt, c, bins in (GEOMS[1], GEOMS[3], GEOMS[6]):
            H = crandn(2, P, bins)
            X4 = make_x(fmt, c, bins, 70)
            a, b = run_fir(X4, fmt, H, [1, 0, 1], 75), run_fir(X4, fmt, H, [1, 0, 1], 75)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            # an index outside the table does not fault and is the clamped call
            wild = run_fir(X4, fmt, H, [-5, 1 << 30, 2], 75)
            assert np.array_equal(wild.view(np.uint32), run_fir(X4, fmt, H, [0, 1, 1], 75).view(np.uint32))
    torch.cuda.synchronize()
    assert _ffi.device_status(raise_on_error=False) == 0


# ------------------------------------------------------------------ end to end
def make_irs(kind, n, rng):
    """(irs for the call, index for the call, the impulse response of every batch item)"""
    if kind == "shared":
        h = rng.standard_normal(n) * np.exp(-np.arange(n) / max(n / 4.0, 1.0))
        return h, None, [h] * BATCH
    if kind == "indexed":
        hs = rng.standard_normal((4, n)) * np.exp(-np.arange(n) / max(n / 4.0, 1.0))
        idx = [3, 0, 3]
        return hs, idx, [hs[i] for i in idx]
    hs = rng.standard_normal((BATCH, n)) * np.exp(-np.arange(n) / max(n / 4.0, 1.0))
    return hs, None, list(hs)


def trim(full, t, n, mode):
    first = {"full": 0, "same": (n - 1) // 2, "valid": n - 1}[mode]
    length = {"full": t + n - 1, "same": t, "valid": t - n + 1}[mode]
    return full[..., first:first + length]


def check_case(L, T, n, fmt, c, kind, modes, rng, misses):
    """one input through every mode of ``modes``: returns (worst device figure, worst model figure) so far over the modes; a case
    beyond the limit is appended to ``misses`` (every figure is printed before anything is asserted).

    The model's figure of an item is taken over the item's whole convolution -- what convolve_model.overlap_save32 computes from
    the same input -- for every mode: 'same' and 'valid' are samples of the very launches that 'full' returns.  The figure of a
    trimmed output can rest on a single sample ('valid' with T == len keeps one), where the model's own error is one random
    draw and its quadruple bounds nothing: measured on an MI355X, that one sample is off by 4.8e-9 on the device and 1.2e-9 in
    the model (L 256, T = len = 257), while over the whole convolutions of the same case the two stand at 1.9e-8 and 1.6e-8."""
    import torch
    from kapre_amd import backend
    x = rng.standard_normal((BATCH, c, T)).astype(np.float32)
    irs, idx, per_item = make_irs(kind, n, rng)
    xt = torch.from_numpy(to_layout(x, fmt)).cuda()
    full64 = np.stack([np.stack([np.convolve(x[i, ch].astype(np.float64), per_item[i]) for ch in range(c)]) for i in range(BATCH)])
    full32 = np.stack([cm.overlap_save32(x[i], per_item[i], L) for i in range(BATCH)])
    worst_dev = worst_model = 0.0
    for mode in modes:
        if mode == "valid" and T < n:
            with pytest.raises(ValueError):
                backend.fftconvolve(xt, irs, mode=mode, index=idx, data_format=fmt, block_size=L)
            continue
        y = from_layout(to_np(backend.fftconvolve(xt, irs, mode=mode, index=idx, data_format=fmt, block_size=L)), fmt)
        want, model = trim(full64, T, n, mode), trim(full32, T, n, mode)
        assert y.shape == want.shape and y.dtype == np.float32, (L, T, n, fmt, c, kind, mode)
        for i in range(BATCH):
            fd, fm = cm.figure(y[i], want[i], per_item[i], x[i]), cm.figure(full32[i], full64[i], per_item[i], x[i])
            worst_dev, worst_model = max(worst_dev, fd), max(worst_model, fm)
            if not fd <= min(4.0 * fm, PARITY_LIMIT):
                misses.append((L, T, n, fmt, c, kind, mode, i, fd, fm, cm.figure(model[i], want[i], per_item[i], x[i])))
        print("L %d T %d len %d %s c%d %s %s: device %.3g, model %.3g" % (L, T, n, fmt, c, kind, mode, worst_dev, worst_model))
    return worst_dev, worst_model


@pytest.mark.parametrize("L", (256, 512, 1024))
def test_fftconvolve_against_float64(L):
    """every T x every impulse-response length at this block size; layout, channel count and the kind of impulse responses
    rotate through the cases so that every layout meets every channel count and every kind, and every case runs the three
    modes on one input"""
    rng = np.random.default_rng(1000 + L)
    lengths = [1, 2, L, L + 1, 4 * L + 1] + ([32 * L] if L == 256 else [])
    kinds = ("shared", "indexed", "itemwise")
    worst = (0.0, 0.0)
    misses = []
    i = 0
    for T in (1, L - 1, L, L + 1, 3 * L + 7):
        for n in lengths:
            if n == 32 * L and T != 3 * L + 7:
                continue                                                   # (once)
            fmt = ("channels_first", "channels_last")[i % 2]
            c = 1 + (i // 2) % 3
            kind = kinds[(i // 6 + i) % 3]
            d, m = check_case(L, T, n, fmt, c, kind, ("full", "same", "valid"), rng, misses)
            worst = (max(worst[0], d), max(worst[1], m))
            i += 1
    print("fftconvolve L = %d: %d cases, worst device figure %.3g, worst float32-model figure %.3g" % (L, i, *worst))
    assert not misses, misses             # (L, T, len, layout, channels, kind, mode, item, device figure, model figure, model figure on the trimmed samples)


@pytest.mark.parametrize("fmt", ("channels_first", "channels_last"))
def test_unit_and_delay_impulse_responses(fmt):
    import torch
    from kapre_amd import backend
    rng = np.random.default_rng(5)
    T, L = 3 * 256 + 7, 256
    x = rng.standard_normal((BATCH, 2, T)).astype(np.float32)
    xt = torch.from_numpy(to_layout(x, fmt)).cuda()
    for n in (1, 300):                                                     # [1.0] and [0, ..., 0, 1]
        h = np.zeros(n)
        h[-1] = 1.0
        y = from_layout(to_np(backend.fftconvolve(xt, h, data_format=fmt, block_size=L)), fmt)
        want = np.concatenate([np.zeros((BATCH, 2, n - 1)), x.astype(np.float64)], axis=-1)
        for i in range(BATCH):
            fd = cm.figure(y[i], want[i], h, x[i])
            fm = cm.figure(cm.overlap_save32(x[i], h, L), want[i], h, x[i])
            print("delay %d, %s, item %d: device %.3g, model %.3g" % (n - 1, fmt, i, fd, fm))
            assert fd <= min(4.0 * fm, PARITY_LIMIT)


# ------------------------------------------------------------------ gradient
def conv64_torch(x_bct, per_item, mode):
    """the same convolution with torch.nn.functional.conv1d in float64 on the host, differentiable in x"""
    import torch
    out = []
    for i, h in enumerate(per_item):
        n = len(h)
        w = torch.from_numpy(np.ascontiguousarray(h[::-1])).reshape(1, 1, n)
        full = torch.nn.functional.conv1d(x_bct[i].unsqueeze(1), w, padding=n - 1).squeeze(1)          # (c, T + n - 1)
        first = {"full": 0, "same": (n - 1) // 2, "valid": n - 1}[mode]
        length = {"full": x_bct.shape[-1] + n - 1, "same": x_bct.shape[-1], "valid": x_bct.shape[-1] - n + 1}[mode]
        out.append(full[:, first:first + length])
    return torch.stack(out)


@pytest.mark.parametrize("fmt", ("channels_first", "channels_last"))
@pytest.mark.parametrize("mode", ("full", "same", "valid"))
def test_gradient(fmt, mode):
    import torch
    from kapre_amd import backend
    L = 256
    rng = np.random.default_rng(77)
    worst = (0.0, 0.0)
    for T, n, kind in ((L + 1, 37, "shared"), (L + 1, L + 1, "indexed"), (3 * L + 7, 2 * L + 5, "itemwise"), (3 * L + 7, L + 1, "shared")):
        c = 2
        x = rng.standard_normal((BATCH, c, T)).astype(np.float32)
        irs, idx, per_item = make_irs(kind, n, rng)
        xg = torch.from_numpy(to_layout(x, fmt)).cuda().requires_grad_(True)
        y = backend.fftconvolve(xg, irs, mode=mode, index=idx, data_format=fmt, block_size=L)
        g = rng.standard_normal(from_layout(to_np(y), fmt).shape).astype(np.float32)
        y.backward(torch.from_numpy(to_layout(g, fmt)).cuda())
        gx = from_layout(to_np(xg.grad), fmt)
        x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        y64 = conv64_torch(x64, per_item, mode)
        y64.backward(torch.from_numpy(g.astype(np.float64)))
        gx64 = x64.grad.numpy()
        assert gx.shape == x.shape
        # the float32 CPU model of the same adjoint: the cotangent zero-extended to the full length, convolved with the
        # time-reversed impulse response, read at [n - 1, n - 1 + T)
        first = {"full": 0, "same": (n - 1) // 2, "valid": n - 1}[mode]
        gfull = np.zeros((BATCH, c, T + n - 1), dtype=np.float32)
        gfull[..., first:first + g.shape[-1]] = g
        for i in range(BATCH):
            model = cm.overlap_save32(gfull[i], per_item[i][::-1], L)[..., n - 1:n - 1 + T]
            fd, fm = cm.figure(gx[i], gx64[i], per_item[i], g[i]), cm.figure(model, gx64[i], per_item[i], g[i])
            worst = (max(worst[0], fd), max(worst[1], fm))
            assert fd <= min(4.0 * fm, PARITY_LIMIT), (T, n, kind, i, fd, fm)
        # <conv(x), g> = <x, conv^T(g)>
        lhs = float(np.sum(from_layout(to_np(y), fmt).astype(np.float64) * g))
        rhs = float(np.sum(x.astype(np.float64) * gx))
        scale = float(np.sqrt(np.sum(from_layout(to_np(y), fmt).astype(np.float64) ** 2) * np.sum(g.astype(np.float64) ** 2)))
        assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, scale)
    print("gradient %s %s: worst device figure %.3g, model %.3g" % (fmt, mode, *worst))


def test_impulse_response_gets_no_gradient():
    import torch
    from kapre_amd import backend
    h = torch.randn(40, requires_grad=True)
    x = torch.randn(2, 300, 1).cuda().requires_grad_(True)
    backend.fftconvolve(x, h).sum().backward()
    assert h.grad is None and x.grad is not None


# ------------------------------------------------------------------ in front of the fused mel launch
def test_chain_convolve_mel(tmp_path):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, keras_shim
    from conftest import speech

    rng = np.random.default_rng(3)
    ir = rng.standard_normal(700) * np.exp(-np.arange(700) / 150.0)
    kw = dict(n_fft=512, hop_length=128, sample_rate=16000, n_mels=40, return_decibel=False)
    mel = kapre.get_melspectrogram_layer(input_shape=(None, 1), **kw)
    conv = kapre.Convolve(ir, mode="same", input_shape=(6000, 1))
    model = kapre.Sequential([conv, mel])
    assert model.output_shape == mel.compute_output_shape((None, 6000, 1))
    x = np.stack([speech(6000, 0), speech(6000, 1000)])[:, :, None]
    xt = torch.from_numpy(x).cuda()
    out = model(xt)
    launches = _ffi.last_launches()
    mid = conv(xt)
    assert torch.equal(out, mel(mid))                                      # the two calls made separately, bit for bit
    assert _ffi.last_launches() == launches and launches.startswith("k_mel")                 # the unchanged fused mel launch
    xg = xt.clone().requires_grad_(True)
    model(xg).sum().backward()
    assert xg.grad.shape == xt.shape and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    path = os.path.join(str(tmp_path), "convolve_mel.keras")
    model.save(path)
    again = keras_shim.load_model(path)
    assert [type(l).__name__ for l in again.layers][0] == "Convolve" and again.output_shape == model.output_shape
    assert torch.equal(again(xt), out)
    kapre.check_device()


def test_spec_fir_is_the_middle_launch():
    import torch
    from kapre_amd import _ffi, backend
    x = torch.randn(2, 1000, 1).cuda()
    seen = []
    real = _ffi._call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)

    _ffi._call = spy
    try:
        backend.fftconvolve(x, np.ones(300), mode="full")
    finally:
        _ffi._call = real
    assert seen == ["kpr_stft_f32", "kpr_spec_fir_c64", "kpr_istft_f32"]    # exactly three launches (and the trim)


# ------------------------------------------------------------------ Reverb and the draw
@pytest.mark.parametrize("n_items", (1, 7, 4096))
@pytest.mark.parametrize("n_choices", (1, 7, 1000))
def test_index_draw_is_its_numpy_restatement(n_items, n_choices):
    import torch
    from kapre_amd import _ffi
    state = torch.tensor([0x1234567 + n_items, 5], dtype=torch.int64).cuda()
    got = to_np(_ffi.index_draw(state, n_items, n_choices))
    assert got.dtype == np.int32
    assert np.array_equal(got, cm.index_draw(0x1234567 + n_items, 5, n_items, n_choices))
    assert am.state_of(state) == (0x1234567 + n_items, 6)
    if (n_items, n_choices) == (4096, 7):
        sigma = np.sqrt(4096 * (1 / 7) * (6 / 7))
        counts = np.bincount(got, minlength=7)
        print("index_draw counts", counts.tolist(), "expected %.1f, 6 sigma %.1f" % (4096 / 7, 6 * sigma))
        assert np.all(np.abs(counts - 4096 / 7) <= 6 * sigma)


@pytest.mark.parametrize("fmt", ("channels_first", "channels_last"))
def test_reverb(fmt):
    import torch
    import kapre_amd as kapre
    from kapre_amd import augmentation, backend
    rng = np.random.default_rng(11)
    irs = rng.standard_normal((5, 400)) * np.exp(-np.arange(400) / 80.0)
    layer = kapre.Reverb(irs, input_data_format=fmt)
    unit = irs / np.sqrt(np.sum(irs ** 2, axis=1, keepdims=True))
    b, c, T = 6, 2, 1500
    x = rng.standard_normal((b, c, T)).astype(np.float32)
    xt = torch.from_numpy(to_layout(x, fmt)).cuda()
    assert layer(xt) is xt
    augmentation.set_seed(4242)
    seed, calls = am.state_of(augmentation.device_state(xt.device))
    y1 = layer(xt, training=True)
    drawn = cm.index_draw(seed, calls, b, 5)
    assert np.array_equal(to_np(layer.last_index), drawn)
    assert tuple(y1.shape) == tuple(xt.shape)
    want = backend.fftconvolve(xt, unit, index=drawn, data_format=fmt).narrow(1 if fmt == "channels_last" else 2, 0, T)
    assert torch.equal(y1, want)
    y2 = layer(xt, training=True)
    assert not np.array_equal(to_np(layer.last_index), drawn) or not torch.equal(y1, y2)      # two calls draw differently
    assert am.state_of(augmentation.device_state(xt.device)) == (seed, calls + 2)
    augmentation.set_seed(4242)
    assert torch.equal(layer(xt, training=True), y1)                       # the same run again, bit for bit
    assert torch.equal(layer(xt, training=True), y2)
    # causal: the output up to t does not depend on the input after t
    x2 = x.copy()
    x2[..., 900:] = 0
    augmentation.set_seed(4242)
    y3 = from_layout(to_np(layer(torch.from_numpy(to_layout(x2, fmt)).cuda(), training=True)), fmt)
    y64 = np.stack([np.stack([np.convolve(x[i, ch].astype(np.float64), unit[drawn[i]])[:T] for ch in range(c)]) for i in range(b)])
    assert max(cm.figure(from_layout(to_np(y1), fmt)[i], y64[i], unit[drawn[i]], x[i]) for i in range(b)) <= PARITY_LIMIT
    assert max(cm.figure(y3[i, :, :900], y64[i, :, :900], unit[drawn[i]], x[i]) for i in range(b)) <= PARITY_LIMIT
    # gradients flow to the waveform
    xg = xt.clone().requires_grad_(True)
    augmentation.set_seed(4242)
    layer(xg, training=True).sum().backward()
    assert xg.grad.shape == xt.shape and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    kapre.check_device()
