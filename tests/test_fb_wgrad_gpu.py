"""kpr_filterbank_wgrad_f32 / TrainableFilterbank on the GPU against the float64 model of tests/fb_wgrad_model.py.

Every element: |gW - gW64| <= gamma_K sum |x||g|, K = S c' + n_slabs + 1.  The worst ratio is printed per case;
measured on an MI355X: at most 0.216 with one-chunk slabs ((130, 129), channels_last x 1; 0.200 at (257, 40); 0.167 with three
interleaved channels), 0.021 at (1025, 128) with automatic slabs."""
import numpy as np
import pytest

import fb_wgrad_model as model
from kapre_amd import _ffi

pytestmark = pytest.mark.gpu

LAYOUTS = [("channels_first", 2), ("channels_last", 1), ("channels_last", 3)]
# one partial tile in both directions; exact tile edges (+ 1 bin); several f-tiles; a second column pass
SHAPES = [(1, 1), (17, 5), (65, 16), (257, 40), (130, 129)]


def rows_of(x, fmt):
    b, c, t, _ = x.shape
    return b * t * (1 if fmt == "channels_last" else c)


def run(x, g, fmt):
    """x, g: (b, c, t, .) numpy -> (gW as numpy, the launch label)"""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, 1, 3) if fmt == "channels_last" else a)).cuda()
    gw = _ffi.filterbank_wgrad(dev(x), dev(g), fmt)
    return gw.cpu().numpy(), _ffi.last_launches()


def limit(x, g, fmt):
    """(gW64, the bound per element, n_slabs) under the current options"""
    _, S, n_slabs, _ = _ffi.filterbank_wgrad_plan(rows_of(x, fmt), x.shape[3], g.shape[3], x.shape[1], fmt)
    want, mass = model.fb_wgrad(x, g)
    return want, model.bound(mass, S, n_slabs, x.shape[1] if fmt == "channels_last" else 1), n_slabs


def within_bound(x, g, fmt, keep=None):
    """worst error / bound over the elements of ``keep`` (default: all); asserts the bound and the label"""
    want, lim, n_slabs = limit(x, g, fmt)
    got, label = run(x, g, fmt)
    assert label.startswith("k_fb_wgrad<") and label.endswith("+ k_fb_wgrad_reduce") == (n_slabs > 1), (label, n_slabs)
    keep = np.ones(want.shape, bool) if keep is None else keep
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)[keep]
    assert (err <= lim[keep]).all(), float((err / lim[keep]).max())
    return float((err / lim[keep]).max()), got


def pair(rng, c, t, n_freq, n_filt, b=1):
    return (rng.standard_normal((b, c, t, n)).astype(np.float32) for n in (n_freq, n_filt))


@pytest.mark.parametrize("fmt,c", LAYOUTS)
@pytest.mark.parametrize("n_freq,n_filt", SHAPES)
def test_against_the_model(n_freq, n_filt, fmt, c):
    """frames 1, 3, S - 1, S, S + 1, 2 S + 1 of one item with the smallest slab (one chunk): one slab, the seam, the reduce launch"""
    old = _ffi.set_option("fb_wgrad_rows", 1)
    try:
        S = _ffi.filterbank_wgrad_plan(1, n_freq, n_filt, c, fmt)[1]
        rng, worst = np.random.default_rng(n_freq * 131 + n_filt), 0.0
        for t in (1, 3, S - 1, S, S + 1, 2 * S + 1):
            x, g = pair(rng, c, t, n_freq, n_filt)
            worst = max(worst, within_bound(x, g, fmt)[0])
    finally:
        _ffi.set_option("fb_wgrad_rows", old)
    print("worst error / bound (%d, %d) %s x %d, S = %d: %.4f" % (n_freq, n_filt, fmt, c, S, worst))


@pytest.mark.parametrize("fmt,c", LAYOUTS)
def test_full_width_automatic_slabs(fmt, c):
    rng = np.random.default_rng(7)
    x, g = pair(rng, c, 150, 1025, 128, b=2)
    assert limit(x, g, fmt)[2] >= 2
    print("worst error / bound (1025, 128) %s x %d: %.4f" % (fmt, c, within_bound(x, g, fmt)[0]))


def test_same_bits_and_non_finite_containment():
    """37 rows in slabs of 16: row 35 lies in the tail chunk.  NaN in x[35, 70]: row 70 of gW is NaN; Inf in g[3, 128]: column 128
    (the one filter of the second pass) is non-finite; every other element is what it is without them: no pad lane reads them."""
    x, g = pair(np.random.default_rng(3), 1, 37, 130, 129)
    old = _ffi.set_option("fb_wgrad_rows", 16)
    try:
        assert np.array_equal(run(x, g, "channels_last")[0].view(np.uint32), run(x, g, "channels_last")[0].view(np.uint32))
        x[0, 0, 35, 70], g[0, 0, 3, 128] = np.nan, np.inf
        keep = np.ones((130, 129), bool)
        keep[70, :], keep[:, 128] = False, False
        got = within_bound(x, g, "channels_last", keep)[1]
    finally:
        _ffi.set_option("fb_wgrad_rows", old)
    assert np.isnan(got[70]).all() and not np.isfinite(got[:, 128]).any()


@pytest.mark.parametrize("fmt,c", [("channels_first", 2), ("channels_last", 3)])
def test_layer_through_autograd(fmt, c, monkeypatch):
    """l = sum(a y): gW = x^T a and gx = a W^T exactly, so both are held to their kernels' bounds (gx: a chain of n_filt products)"""
    import torch
    import kapre_amd as kapre
    rng = np.random.default_rng(11)
    x, a = pair(rng, c, 45, 65, 16, b=2)
    w0 = rng.standard_normal((65, 16)).astype(np.float32)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(np.moveaxis(v, 1, 3) if fmt == "channels_last" else v)).cuda()
    layer = kapre.TrainableFilterbank(filterbank=w0, data_format=fmt)
    xt = dev(x).requires_grad_(True)
    y = layer(xt)
    (dev(a) * y).sum().backward()
    (w,) = layer.parameters()
    want, lim, _ = limit(x, a, fmt)
    assert (np.abs(w.grad.cpu().numpy() - want) <= lim).all()
    gx = xt.grad.cpu().numpy()
    gx = np.moveaxis(gx, 3, 1) if fmt == "channels_last" else gx
    assert (np.abs(gx - a.astype(np.float64) @ w0.T.astype(np.float64)) <= model.bound(np.abs(a) @ np.abs(w0.T), 16, 1, 1)).all()
    # an input without a gradient: the output is still on the tape, and backward is the gW launch alone
    calls = []
    matmul = _ffi.freq_matmul
    y = layer(dev(x))
    monkeypatch.setattr(_ffi, "freq_matmul", lambda *args, **kw: calls.append(1) or matmul(*args, **kw))
    w.grad = None
    assert y.grad_fn is not None
    (dev(a) * y).sum().backward()
    # (the launch log is per thread and backward runs on autograd's: the GEMM launcher is counted instead)
    assert calls == [] and (np.abs(w.grad.cpu().numpy() - want) <= lim).all()


def test_an_optimiser_step_is_seen_by_the_next_forward():
    import torch
    import kapre_amd as kapre
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((2, 1000, 1)).astype(np.float32)).cuda()
    w0 = rng.uniform(0, 1, (65, 24)).astype(np.float32)
    front, layer = kapre.Sequential([kapre.STFT(n_fft=128, hop_length=64), kapre.Magnitude()]), kapre.TrainableFilterbank(filterbank=w0)
    chain = kapre.Sequential(front.layers + [layer])
    opt = torch.optim.SGD(chain.parameters(), lr=0.5)
    chain(x).sum().backward()
    opt.step()
    w1 = layer.filterbank
    assert not np.array_equal(w1, w0)
    got = chain(x).detach().cpu().numpy()
    label = _ffi.last_launches()
    assert "mel" not in label and label.startswith(("k_gemm", "k_thin_gemm")), label
    mag = front(x).cpu().numpy().astype(np.float64)                        # (b, frames, 65, 1)
    want, mass = np.einsum("btfc,fm->btmc", mag, w1.astype(np.float64)), np.einsum("btfc,fm->btmc", mag, np.abs(w1))
    assert (np.abs(got - want) <= model.bound(mass, 65, 1, 1)).all()


def test_melspectrogram_layer_trains_saves_and_loads(tmp_path):
    import torch
    import kapre_amd as kapre
    from kapre_amd import keras_shim
    args = dict(n_fft=256, hop_length=128, sample_rate=8000, n_mels=20, input_shape=(2000, 1))
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 2000, 1)).astype(np.float32)).cuda()
    chain = kapre.get_melspectrogram_layer(trainable_fb=True, **args)
    w0 = chain.layers[2].filterbank
    opt = torch.optim.SGD(chain.parameters(), lr=0.1)
    chain(x).sum().backward()
    opt.step()
    chain.layers[2].constrain_()
    w1 = chain.layers[2].filterbank
    assert not np.array_equal(w1, w0) and (w1 >= 0).all()
    path = str(tmp_path / "trained.keras")
    chain.save(path)
    loaded = keras_shim.load_model(path)
    assert type(loaded.layers[2]) is kapre.TrainableFilterbank and np.array_equal(loaded.layers[2].filterbank, w1)
    assert torch.equal(loaded(x), chain(x))
    labels = []
    for kw in ({}, {"trainable_fb": False}):                              # the default chain is the fused launch it was
        kapre.get_melspectrogram_layer(**args, **kw)(x)
        labels.append(_ffi.last_launches())
    assert labels[0] == labels[1] and "mel" in labels[0], labels
