"""LFilter on the GPU (kapre_amd.LFilter / backend.lfilter, kpr_lfilter_f32) against the float64 model of tests/lfilter_model.py
(scipy.signal.lfilter on the float64 copy of the input).

Parity rule, derived and not tuned, for every element:

    |y - y64| <= 2^-24 |y64| + K 2^-53 bud + 2^-149,   K = 32,   bud = |g| * loc   (lfilter_model.budget)

one rounding to float32, and K float64 roundings relative to the magnitudes of one step, each carried on by 1 / A(z).  Every
check prints its worst ratio |y - y64| / bound.  The seams -- samples per lane, wave, workgroup step and segment -- come from
kpr_lfilter_plan.  Batch 3; the longest signals are three segments and a ragged tail."""
import ctypes
import functools
import os

import numpy as np
import pytest

import lfilter_model as lm
from conftest import speech

pytestmark = pytest.mark.gpu

FILTERS = lm.test_filters()
NAMES = sorted(FILTERS)
BATCH, CH = 3, 3
VARIANTS = (0, 1, 2)                                              # automatic, whole-signal, segmented


def plan():
    from kapre_amd import _ffi
    return _ffi.lfilter_plan(BATCH, CH, 100000, "channels_first")[:4]


def to_layout(x_bct, fmt):
    """(b, c, t) -> the layout of ``fmt``, contiguous"""
    return np.array(np.moveaxis(x_bct, 1, 2) if fmt == "channels_last" else x_bct, order="C", copy=True)


def from_layout(y, fmt):
    return np.moveaxis(y, 2, 1) if fmt == "channels_last" else y


def to_np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def signals(kind, T):
    """(BATCH, CH, T) float32, different data per series; not to be written to"""
    if kind == "speech":
        x = np.stack([speech(T, offset=11000 * i) for i in range(BATCH * CH)]).astype(np.float32)
    else:
        x = np.random.default_rng(T + 17).standard_normal((BATCH * CH, T)).astype(np.float32)
        if kind == "noise+2":
            x = x + np.float32(2.0)
    x = x.reshape(BATCH, CH, T)
    x.setflags(write=False)
    return x


def bound_of(x, coef, reverse=False):
    """(y64, bound) of the model on x along the last axis"""
    y64 = lm.lfilter(x, coef, reverse)
    return y64, 2.0 ** -24 * np.abs(y64) + lm.K * 2.0 ** -53 * lm.budget(x, y64, coef, reverse) + 2.0 ** -149


@functools.lru_cache(maxsize=None)
def reference(name, kind, T, reverse=False):
    y64, bound = bound_of(signals(kind, T), FILTERS[name], reverse)
    y64.setflags(write=False)
    bound.setflags(write=False)
    return y64, bound


def ratio(y, y64, bound):
    assert y.dtype == np.float32 and y.shape == y64.shape
    r = np.abs(y.astype(np.float64) - y64) / bound
    return float(np.max(np.where(np.isfinite(r), r, np.inf))) if r.size else 0.0


def sos_of(coef):
    b0, b1, b2, a1, a2 = coef
    return [b0, b1, b2, 1.0, a1, a2]


class variant:
    """``with variant(v):`` -- lfilter_variant = v inside, the old value restored on the way out"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from kapre_amd import _ffi
        self.old = _ffi.set_option("lfilter_variant", self.v)

    def __exit__(self, *exc):
        from kapre_amd import _ffi
        _ffi.set_option("lfilter_variant", self.old)


def lengths():
    lane, wave, step, seg = plan()
    out = [1, 2, 3]
    for n in (lane, wave, step, seg):
        out += [n - 1, n, n + 1]
    out += [3 * seg + seg // 3 + 1, 3 * seg + seg // 3 + 2]         # three segments and a ragged tail: 4-byte and 16-byte accesses
    return out


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", NAMES)
def test_forward_parity(name):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, backend

    coef = FILTERS[name]
    worst, forms = 0.0, set()
    for kind in ("speech", "noise", "noise+2"):
        for T in lengths():
            x = signals(kind, T)
            y64, bound = reference(name, kind, T)
            for fmt in ("channels_first", "channels_last"):
                for C in (1, 2, 3):
                    xt = torch.from_numpy(to_layout(x[:, :C], fmt)).cuda()
                    for v in VARIANTS:
                        with variant(v):
                            forms.add(_ffi.lfilter_plan(BATCH, C, T, fmt)[4])
                            y = backend.lfilter(xt, sos_of(coef), data_format=fmt)
                        assert y.shape == xt.shape and y.data_ptr() != xt.data_ptr()
                        r = ratio(from_layout(to_np(y), fmt), y64[:, :C], bound[:, :C])
                        assert r <= 1.0, (name, kind, T, fmt, C, v, r)
                        worst = max(worst, r)
    assert forms == {_ffi.LFILTER_WHOLE, _ffi.LFILTER_SEGMENTED}
    print("lfilter forward %s: worst ratio %.4f" % (name, worst))
    kapre.check_device()


# ------------------------------------------------------------------ seams
@pytest.mark.parametrize("name", ["hp5", "deemph"])
@pytest.mark.parametrize("v", [1, 2])
def test_seams(name, v):
    """one series per seam position: a unit impulse and a unit step starting (in scan order) at every position within 3 samples
    of every lane boundary of a three-segment signal -- which takes in every wave, step and segment boundary and both ends.
    A signal that is zero before its start gives exact zeros there, so the model of the series that starts at p is the model of
    the one that starts at 0, shifted: two references per direction, compared on the device in float64."""
    import torch
    import kapre_amd as kapre
    from kapre_amd import backend

    lane, wave, step, seg = plan()
    T = 3 * seg
    coef = FILTERS[name]
    t = np.arange(T)
    starts = t[(t % lane <= 3) | (t % lane >= lane - 3)]
    assert {0, 3, lane - 3, wave - 1, wave, step + 3, seg - 3, seg, 2 * seg - 1, T - 1} <= set(starts.tolist())
    dev = torch.device("cuda")
    p = torch.from_numpy(starts).to(dev)
    tt = torch.arange(T, device=dev)
    worst = 0.0
    for reverse in (False, True):
        # series 2 i: the impulse at starts[i]; series 2 i + 1: the step that starts there and runs on in scan order
        x = torch.zeros((2 * len(starts), 1, T), dtype=torch.float32, device=dev)
        x[0::2, 0, :] = (tt[None, :] == p[:, None]).float()
        x[1::2, 0, :] = ((tt[None, :] <= p[:, None]) if reverse else (tt[None, :] >= p[:, None])).float()
        with variant(v):
            y = backend.lfilter(x, sos_of(coef), data_format="channels_first", reverse=reverse)
        if reverse:                                               # in scan order: the start p becomes T - 1 - p
            y = torch.flip(y, dims=(2,))
        q = (T - 1 - p) if reverse else p
        for kind in (0, 1):
            x0 = np.zeros(T, dtype=np.float32)
            if kind == 0:
                x0[0] = 1.0
            else:
                x0[:] = 1.0
            y64, bound = bound_of(x0, coef)
            ref, bnd = torch.from_numpy(y64).to(dev), torch.from_numpy(bound).to(dev)
            for lo in range(0, len(starts), 1024):
                rows = y[kind::2, 0][lo:lo + 1024].double()
                idx = tt[None, :] - q[lo:lo + 1024, None]
                live = idx >= 0
                idx = idx.clamp(min=0)
                want = torch.where(live, ref[idx], torch.zeros((), dtype=torch.float64, device=dev))
                lim = torch.where(live, bnd[idx], torch.full((), 2.0 ** -149, dtype=torch.float64, device=dev))
                r = torch.nan_to_num((rows - want).abs() / lim, nan=float("inf"))
                worst = max(worst, float(r.max()))
        assert worst <= 1.0, (name, v, reverse, worst)
    print("lfilter seams %s, variant %d, %d series: worst ratio %.4f" % (name, v, 2 * len(starts), worst))
    kapre.check_device()


# ------------------------------------------------------------------ reverse mode, gradient, zero phase
@pytest.mark.parametrize("name", ["hp5", "hp20", "bs1770", "preemph", "deemph"])
def test_reverse_parity(name):
    import torch
    import kapre_amd as kapre
    from kapre_amd import backend

    lane, wave, step, seg = plan()
    coef = FILTERS[name]
    worst = 0.0
    for T in (1, 3, lane + 1, wave - 1, step + 1, seg + 1, 3 * seg + seg // 3 + 1, 3 * seg + seg // 3 + 2):
        x = signals("noise+2", T)
        y64, bound = reference(name, "noise+2", T, True)
        for fmt in ("channels_first", "channels_last"):
            xt = torch.from_numpy(to_layout(x, fmt)).cuda()
            for v in VARIANTS:
                with variant(v):
                    y = backend.lfilter(xt, sos_of(coef), data_format=fmt, reverse=True)
                r = ratio(from_layout(to_np(y), fmt), y64, bound)
                assert r <= 1.0, (name, T, fmt, v, r)
                worst = max(worst, r)
    print("lfilter reverse %s: worst ratio %.4f" % (name, worst))
    kapre.check_device()


@pytest.mark.parametrize("sections", [("hp20",), ("hp80", "bs1770", "preemph")], ids=["one", "three"])
@pytest.mark.parametrize("fmt", ["channels_first", "channels_last"])
def test_gradient(sections, fmt):
    """the cotangent equals the model's adjoint (the sections in reverse order, each in reverse time), section by section under the
    rule with the kernel's own previous output as the input; <F x, g> = <x, F^T g> in float64 to 2^-20 relative"""
    import torch
    import kapre_amd as kapre

    lane, wave, step, seg = plan()
    coefs = [FILTERS[n] for n in sections]
    layer = kapre.LFilter([sos_of(c) for c in coefs], data_format=fmt)
    worst = 0.0
    for T in (step + 5, 3 * seg + 101):
        x = signals("noise", T)
        g = np.random.default_rng(T).standard_normal(x.shape).astype(np.float32)
        xt = torch.from_numpy(to_layout(x, fmt)).cuda().requires_grad_(True)
        gt = torch.from_numpy(to_layout(g, fmt)).cuda()
        for v in VARIANTS:
            with variant(v):
                y = layer(xt)
                gx, = torch.autograd.grad(y, xt, gt)
                # the same chain by hand, to hold every launch of the backward pass to the rule with its own input
                cur = gt
                for c in reversed(coefs):
                    nxt = kapre.backend.lfilter(cur, sos_of(c), data_format=fmt, reverse=True)
                    y64, bound = bound_of(from_layout(to_np(cur), fmt), c, True)
                    r = ratio(from_layout(to_np(nxt), fmt), y64, bound)
                    assert r <= 1.0, (sections, fmt, T, v, r)
                    worst = max(worst, r)
                    cur = nxt
            assert torch.equal(gx, cur) and gx.shape == xt.shape and gx.data_ptr() != cur.data_ptr()
            lhs = float(np.sum(to_np(y).astype(np.float64) * to_np(gt).astype(np.float64)))
            rhs = float(np.sum(to_np(xt).astype(np.float64) * to_np(gx).astype(np.float64)))
            rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
            print("lfilter %s %s T=%d variant %d: <F x, g> = %.9e, <x, F^T g> = %.9e, relative difference %.2e" % (
                "+".join(sections), fmt, T, v, lhs, rhs, rel))
            assert rel <= 2.0 ** -20
    print("lfilter backward %s: worst ratio %.4f" % ("+".join(sections), worst))
    kapre.check_device()


def test_cascade_and_zero_phase():
    """a cascade is checked section by section with the kernel's own previous output as the input, and equals bit for bit the
    hand-made composition of single-section calls; zero_phase = the cascade forward, then the cascade in reverse"""
    import torch
    import kapre_amd as kapre
    from kapre_amd import backend

    lane, wave, step, seg = plan()
    names = ("hp80", "lp4000", "bs1770", "deemph")
    coefs = [FILTERS[n] for n in names]
    sos = [sos_of(c) for c in coefs]
    x = signals("speech", 2 * seg + 345)
    worst = 0.0
    for fmt in ("channels_first", "channels_last"):
        xt = torch.from_numpy(to_layout(x, fmt)).cuda()
        cur = xt
        for c in coefs:
            nxt = backend.lfilter(cur, sos_of(c), data_format=fmt)
            y64, bound = bound_of(from_layout(to_np(cur), fmt), c)
            worst = max(worst, ratio(from_layout(to_np(nxt), fmt), y64, bound))
            cur = nxt
        assert worst <= 1.0
        assert torch.equal(kapre.LFilter(sos, data_format=fmt)(xt), cur)
        assert torch.equal(backend.lfilter(xt, sos, data_format=fmt), cur)
        back = cur
        for c in coefs:
            back = backend.lfilter(back, sos_of(c), data_format=fmt, reverse=True)
        zp = kapre.LFilter(sos, zero_phase=True, data_format=fmt)(xt)
        assert torch.equal(zp, back)
        assert torch.equal(zp, backend.lfilter(backend.lfilter(xt, sos, data_format=fmt), sos, data_format=fmt, reverse=True))
        # close to the float32-rounded model of the whole chain (every section's input differs by earlier roundings)
        want = lm.cascade(x, coefs, zero_phase=True)
        assert np.max(np.abs(from_layout(to_np(zp), fmt) - want)) <= 1e-4 * np.max(np.abs(want))
    print("lfilter cascade %s: worst ratio %.4f" % ("+".join(names), worst))
    kapre.check_device()


def test_emphasis_layers_are_inverse_to_each_other():
    import torch
    import kapre_amd as kapre

    x = signals("speech", 5000)[:, :1]
    xt = torch.from_numpy(to_layout(x, "channels_last")).cuda()
    pre = kapre.Preemphasis(0.97)(xt)
    want = x.astype(np.float64).copy()
    want[..., 1:] -= 0.97 * x[..., :-1].astype(np.float64)
    y64, bound = bound_of(x, lm.PREEMPHASIS)
    assert np.max(np.abs(want - y64)) <= 2.0 ** -52 * np.max(np.abs(x))                          # the model is the textbook formula
    assert ratio(from_layout(to_np(pre), "channels_last"), y64, bound) <= 1.0
    back = kapre.Deemphasis(0.97)(pre)
    assert float((back - xt).abs().max()) <= 2.0 ** -22 * float(xt.abs().max()) * 34                # sum |0.97^k| < 34 roundings of pre
    kapre.check_device()


# ------------------------------------------------------------------ same bits
@pytest.mark.parametrize("v", [1, 2])
def test_same_bits(v):
    import torch
    import kapre_amd as kapre

    lane, wave, step, seg = plan()
    x = signals("noise", 3 * seg + 101)
    layer = kapre.LFilter([sos_of(FILTERS["hp5"]), sos_of(FILTERS["lp100q8"])], data_format="channels_first")
    xt = torch.from_numpy(x.copy()).cuda().requires_grad_(True)
    gt = torch.from_numpy(np.random.default_rng(5).standard_normal(x.shape).astype(np.float32)).cuda()
    with variant(v):
        y1 = layer(xt)
        g1, = torch.autograd.grad(y1, xt, gt)
        y2 = layer(xt)
        g2, = torch.autograd.grad(y2, xt, gt)
    assert y1.data_ptr() != y2.data_ptr() and g1.data_ptr() != g2.data_ptr()
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    kapre.check_device()


# ------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("name", ["hp20", "preemph", "delay"])
def test_non_finite_input(name, v):
    """with t0 the first non-finite sample of a series: every output before t0 (after it in reverse) equals bit for bit the run in
    which that sample is 0, other series are untouched, and a pure FIR section is affected at t0 ... t0 + 2 only"""
    import torch
    import kapre_amd as kapre
    from kapre_amd import backend

    lane, wave, step, seg = plan()
    T = 2 * seg + 99
    fir = FILTERS[name][3] == 0.0 and FILTERS[name][4] == 0.0
    base = signals("noise", T)[:, :2].copy()
    places = [0, lane // 2, wave - 1, wave, seg - 1, seg, T - 1]
    for reverse in (False, True):
        for bad in (np.nan, np.inf):
            clean, dirty = [], []
            for p in places:
                z = base.copy()
                z[1, 0, p] = 0.0
                clean.append(z)
                d = z.copy()
                d[1, 0, p] = bad
                dirty.append(d)
            clean, dirty = np.concatenate(clean), np.concatenate(dirty)              # (3 places, 2, T)
            with variant(v):
                yc = to_np(backend.lfilter(torch.from_numpy(clean).cuda(), sos_of(FILTERS[name]), 'channels_first', reverse))
                yd = to_np(backend.lfilter(torch.from_numpy(dirty).cuda(), sos_of(FILTERS[name]), 'channels_first', reverse))
            for i, p in enumerate(places):
                row = 3 * i + 1
                others = [r for r in range(3 * i, 3 * i + 3) if r != row]
                assert np.array_equal(yc[others], yd[others]) and np.array_equal(yc[row, 1], yd[row, 1])       # untouched
                before = slice(p + 1, T) if reverse else slice(0, p)
                assert np.array_equal(yc[row, 0, before].view(np.uint32), yd[row, 0, before].view(np.uint32)), (name, v, reverse, p)
                if fir:
                    after = slice(0, max(p - 2, 0)) if reverse else slice(p + 3, T)
                    assert np.array_equal(yc[row, 0, after].view(np.uint32), yd[row, 0, after].view(np.uint32)), (name, v, reverse, p)
            assert np.all(np.isfinite(yc))
    kapre.check_device()


# ------------------------------------------------------------------ in front of the fused mel launch
def test_chain_preemphasis_mel(tmp_path):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, keras_shim

    kw = dict(n_fft=512, hop_length=128, sample_rate=16000, n_mels=40, return_decibel=False)
    mel = kapre.get_melspectrogram_layer(input_shape=(None, 1), **kw)
    model = kapre.Sequential([kapre.Preemphasis(0.97, input_shape=(6000, 1)), mel])
    assert model.output_shape == mel.compute_output_shape((None, 6000, 1))
    x = signals("speech", 6000)[:2, :1]
    xt = torch.from_numpy(to_layout(x, "channels_last")).cuda()
    out = model(xt)
    launches = _ffi.last_launches()
    pre = lm.cascade(x, [lm.PREEMPHASIS])
    assert torch.equal(out, mel(torch.from_numpy(to_layout(pre, "channels_last")).cuda()))       # model-then-layer
    assert _ffi.last_launches() == launches and launches.startswith("k_mel")                   # the unchanged fused mel launch
    assert tuple(out.shape)[1:] == tuple(model.output_shape)[1:]
    xg = xt.clone().requires_grad_(True)
    model(xg).sum().backward()
    assert xg.grad.shape == xt.shape and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    path = os.path.join(str(tmp_path), "preemph_mel.keras")
    model.save(path)
    again = keras_shim.load_model(path)
    assert [type(l).__name__ for l in again.layers][0] == "Preemphasis" and again.output_shape == model.output_shape
    assert torch.equal(again(xt), out)
    kapre.check_device()


def test_chain_resample_highpass_mel(tmp_path):
    import torch
    import kapre_amd as kapre
    from kapre_amd import keras_shim
    from kapre_amd.backend import biquad_sos

    sos = biquad_sos('highpass', 16000, 80)
    mel = kapre.get_melspectrogram_layer(n_fft=400, hop_length=160, sample_rate=16000, n_mels=80, input_shape=(None, 1))
    model = kapre.Sequential([kapre.Resample(44100, 16000, input_shape=(22050, 1)), kapre.LFilter(sos), mel])
    assert model.output_shape == mel.compute_output_shape((None, 8000, 1))
    x = signals("speech", 22050)[:2, :1]
    xt = torch.from_numpy(to_layout(x, "channels_last")).cuda()
    out = model(xt)
    assert tuple(out.shape)[1:] == tuple(model.output_shape)[1:]
    res = kapre.Resample(44100, 16000)(xt)
    filt = lm.cascade(from_layout(to_np(res), "channels_last"), [lm.coef_of(sos[0])])             # the model on the kernel's input
    got = kapre.LFilter(sos)(res)
    y64, bound = bound_of(from_layout(to_np(res), "channels_last"), lm.coef_of(sos[0]))
    r = ratio(from_layout(to_np(got), "channels_last"), y64, bound)
    print("lfilter in the chain: worst ratio %.4f, %d of %d samples equal the float32-rounded model" % (
        r, int(np.sum(from_layout(to_np(got), "channels_last") == filt)), filt.size))
    assert r <= 1.0 and torch.equal(out, mel(got))
    xg = xt.clone().requires_grad_(True)
    model(xg).sum().backward()
    assert xg.grad.shape == xt.shape and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    path = os.path.join(str(tmp_path), "front_end.keras")
    model.save(path)
    again = keras_shim.load_model(path)
    assert [type(l).__name__ for l in again.layers][:2] == ["Resample", "LFilter"] and again.output_shape == model.output_shape
    assert again.layers[1].get_config()["sos"] == sos.tolist()
    assert torch.equal(again(xt), out)
    kapre.check_device()


# ------------------------------------------------------------------ errors that need the library and a device
def test_errors():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, backend

    lane, wave, step, seg = plan()
    x = torch.zeros((2, 1, 3 * seg), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="not stable"):
        backend.lfilter(x, [1.0, 0.0, 0.0, 1.0, -2.0, 1.0], data_format="channels_first")
    with pytest.raises(ValueError, match="a0 = 0"):
        backend.lfilter(x, [1.0, 0.0, 0.0, 0.0, 0.5, 0.0], data_format="channels_first")
    with pytest.raises(TypeError, match="float32"):
        kapre.LFilter([1.0, 0.0, 0.0, 1.0, -0.5, 0.0])(x.double())
    # the raw ABI: a short workspace for the segmented form, overlapping x / out
    L = _ffi.lib()
    coef = (ctypes.c_double * 5)(*FILTERS["hp20"])
    out = torch.full_like(x, 7.0)
    need = int(L.kpr_lfilter_workspace_bytes(2, 1, 3 * seg, 0))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = _ffi.current_stream_ptr()
    with variant(2):
        assert L.kpr_lfilter_f32(_ffi.ptr(x), 2, 1, 3 * seg, 0, coef, 0, _ffi.ptr(out), _ffi.ptr(ws), need - 1, stream) == -4
        assert L.kpr_lfilter_f32(_ffi.ptr(x), 2, 1, 3 * seg, 0, coef, 0, _ffi.ptr(out), None, 0, stream) == -4
        assert L.kpr_lfilter_f32(_ffi.ptr(x), 2, 1, 3 * seg, 0, coef, 0, _ffi.ptr(x), _ffi.ptr(ws), need, stream) == -1
        assert b"overlap" in L.kpr_last_error()
        shifted = ctypes.c_void_p(x.data_ptr() + 4 * seg)
        assert L.kpr_lfilter_f32(_ffi.ptr(x), 1, 1, 3 * seg, 0, coef, 0, shifted, _ffi.ptr(ws), need, stream) == -1
        assert L.kpr_lfilter_f32(_ffi.ptr(x), 2, 1, 3 * seg, 0, coef, 0, _ffi.ptr(out), _ffi.ptr(ws), need, stream) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                          # the refused calls wrote nothing, the last one filtered zeros
    with variant(1):                                              # the whole-signal form reads no workspace
        assert L.kpr_lfilter_f32(_ffi.ptr(x), 2, 1, 3 * seg, 0, coef, 1, _ffi.ptr(out), None, 0, stream) == 0
    assert L.kpr_lfilter_f32(_ffi.ptr(x), 0, 1, 3 * seg, 0, coef, 0, _ffi.ptr(out), None, 0, stream) == 0
    assert _ffi.last_launches() == ""                             # batch == 0 launches nothing
    kapre.check_device()
