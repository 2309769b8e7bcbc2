"""Resample on the GPU (kapre_amd.Resample / backend.resample, kpr_resample_f32) against the float64 numpy model of
tests/resample_model.py.

Parity rule, derived and not tuned: |y - y64| <= (n_taps + 3) * 2^-24 * budget + 1e-37 for every element, budget = sum_k |tab_k x_k|
of that output (resample_model.abs_budget): the n_taps float32 FMAs of an output each add at most 2^-24 of the running
magnitude, the rounding of the table to float32 and one unit in the last place between the C library's and numpy's sine and
cosine are the + 3.  The backward pass is held to the same formula with the adjoint table's n_taps and budget.  Every check
prints its worst |y - y64| / bound.

Lengths: 1; 5 (shorter than the support); 3 orig + 7; three tiles and a ragged tail, the tile being what kpr_resample_plan
reports for the table of that direction."""
import os

import numpy as np
import pytest

import resample_model as rm
from conftest import rel_err, speech

pytestmark = pytest.mark.gpu

RATIOS = [(44100, 16000), (16000, 44100), (48000, 44100), (3, 2), (2, 3), (1, 2), (2, 1), (48000, 8000)]
IDS = ["%dto%d" % r for r in RATIOS]
BATCH = 3


def shape_of(fmt, b, c, t):
    return (b, t, c) if fmt == "channels_last" else (b, c, t)


def to_layout(x_bct, fmt):
    """(b, c, t) -> the layout of ``fmt``, contiguous"""
    return np.ascontiguousarray(np.moveaxis(x_bct, 1, 2)) if fmt == "channels_last" else np.ascontiguousarray(x_bct)


def from_layout(y, fmt):
    return np.moveaxis(y, 2, 1) if fmt == "channels_last" else y


def table_shape(orig, new, adjoint):
    from kapre_amd import _ffi
    n_phases, n_taps, step = _ffi.resample_table_size(orig, new, 6, 0.99, adjoint)
    return n_phases, n_taps, step, _ffi.resample_plan(n_phases, n_taps, step)


def three_tiles(orig, new, adjoint):
    """an input length T whose pass in that direction writes three whole tiles and a ragged tail"""
    _, _, _, tile = table_shape(orig, new, adjoint)
    want = 3 * tile + tile // 3 + 1                                   # outputs of that direction
    if adjoint:
        return want                                                   # the adjoint writes T samples
    ro, rn = rm.reduced(orig, new)
    T = -(-want * ro // rn)
    assert rm.out_length(T, orig, new) >= want
    return T


def signals(kind, n, T, seed):
    """(n, T) float32: different data per row"""
    if kind == "noise":
        return np.random.default_rng(seed).standard_normal((n, T)).astype(np.float32)
    return np.stack([speech(T, offset=12000 * i) for i in range(n)]).astype(np.float32)


def check(y, y64, budget, n_taps, label):
    bound = (n_taps + 3) * 2.0 ** -24 * budget + 1e-37
    err = np.abs(y.astype(np.float64) - y64)
    worst = float(np.max(err / bound)) if err.size else 0.0
    print("resample %s: worst |y - y64| / bound = %.3f (n_taps %d)" % (label, worst, n_taps))
    assert y.dtype == np.float32 and y.shape == y64.shape
    assert np.all(err <= bound), (label, worst)
    return worst


def to_np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("orig,new", RATIOS, ids=IDS)
def test_forward_parity(orig, new):
    import kapre_amd as kapre

    ro, _ = rm.reduced(orig, new)
    n_taps = table_shape(orig, new, False)[1]
    worst = 0.0
    for T in (1, 5, 3 * ro + 7, three_tiles(orig, new, False)):
        for kind in ("speech", "noise"):
            x = signals(kind, BATCH * 3, T, seed=T).reshape(BATCH, 3, T)
            y64, budget = rm.resample(x, orig, new), rm.abs_budget(x, orig, new)        # once, shared by the shapes below
            for fmt in ("channels_last", "channels_first"):
                layer = kapre.Resample(orig, new, data_format=fmt)
                for C in (1, 2, 3):
                    y = to_np(layer(to_layout(x[:, :C], fmt)))
                    assert y.shape == shape_of(fmt, BATCH, C, rm.out_length(T, orig, new))
                    worst = max(worst, check(from_layout(y, fmt), y64[:, :C], budget[:, :C], n_taps,
                                             "%d->%d T=%d %s %s C=%d" % (orig, new, T, kind, fmt, C)))
    print("resample forward %d->%d: worst ratio %.3f" % (orig, new, worst))
    kapre.check_device()


@pytest.mark.parametrize("orig,new", RATIOS, ids=IDS)
def test_tile_seams(orig, new):
    """one impulse per signal, at every input position within n_taps of a tile boundary, of the signal's start and of its end"""
    import kapre_amd as kapre

    n_phases, n_taps, step, tile = table_shape(orig, new, False)
    T = three_tiles(orig, new, False)
    spots = set(range(0, n_taps + 1)) | set(range(T - n_taps - 1, T))
    for m in (tile, 2 * tile, 3 * tile):
        centre = m * step // n_phases
        spots |= set(range(centre - n_taps - 1, centre + n_taps + 2))
    spots = sorted(s for s in spots if 0 <= s < T)
    if len(spots) % 2:
        spots.append(T // 2)
    x = np.zeros((len(spots), T), dtype=np.float32)
    x[np.arange(len(spots)), spots] = np.float32(0.7) * (1 + np.arange(len(spots)) % 3)
    y64, budget = rm.resample(x, orig, new), rm.abs_budget(x, orig, new)
    y = to_np(kapre.Resample(orig, new, data_format="channels_first")(x[:, None, :]))[:, 0]
    check(y, y64, budget, n_taps, "%d->%d seams, channels_first" % (orig, new))
    pairs = x.reshape(-1, 2, T)                                                # two impulses per item, interleaved
    y = to_np(kapre.Resample(orig, new, data_format="channels_last")(to_layout(pairs, "channels_last")))
    check(from_layout(y, "channels_last").reshape(len(spots), -1), y64, budget, n_taps, "%d->%d seams, channels_last" % (orig, new))
    kapre.check_device()


def test_same_call_same_bits():
    import torch
    import kapre_amd as kapre

    x = torch.from_numpy(signals("noise", 6, three_tiles(44100, 16000, False), 5).reshape(3, -1, 2)).cuda()
    layer = kapre.Resample(44100, 16000, data_format="channels_last")
    a, b = layer(x), layer(x)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    xr = x.clone().requires_grad_(True)
    g = torch.from_numpy(signals("noise", 6, a.shape[1], 6).reshape(3, -1, 2)).cuda()
    (g1,) = torch.autograd.grad(layer(xr), xr, g)
    (g2,) = torch.autograd.grad(layer(xr), xr, g)
    assert torch.equal(g1, g2)


def test_identity_returns_the_input_and_launches_nothing():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, backend

    x = torch.zeros((2, 64, 1), device="cuda")
    plan = _ffi.resample_plans(2, 1, 6, 0.99, x.device)[0]
    assert _ffi.resample(x[:0], "channels_last", plan, 0).shape == (0, 0, 1)       # an empty call: the launch log restarts
    assert _ffi.last_launches() == ""
    assert kapre.Resample(16000, 16000)(x) is x and backend.resample(x, 48000, 48000) is x
    xg = x.clone().requires_grad_(True)
    assert kapre.Resample(44100, 44100)(xg) is xg
    assert _ffi.last_launches() == ""
    kapre.Resample(2, 1)(x)
    assert _ffi.last_launches() == "k_resample<1>"
    kapre.Resample(2, 1)(torch.zeros((2, 64, 2), device="cuda"))
    assert _ffi.last_launches() == "k_resample<2>"


def test_one_forward_launch_without_grad_and_one_more_for_backward():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi

    layer = kapre.Resample(3, 2)
    x = torch.randn((2, 90, 1), device="cuda")
    y = layer(x)
    assert y.grad_fn is None and _ffi.last_launches() == "k_resample<1>"
    xg = x.clone().requires_grad_(True)
    y = layer(xg)
    assert y.grad_fn is not None and _ffi.last_launches() == "k_resample<1>"
    y.sum().backward()
    assert _ffi.last_launches() == "k_resample<1>" and xg.grad.shape == x.shape


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("orig,new", RATIOS, ids=IDS)
def test_backward_parity(orig, new):
    import torch
    import kapre_amd as kapre

    ro, _ = rm.reduced(orig, new)
    n_taps = table_shape(orig, new, True)[1]
    worst = 0.0
    for T in (3 * ro + 7, three_tiles(orig, new, True)):
        x = signals("noise", BATCH * 2, T, seed=T + 1).reshape(BATCH, 2, T)
        T_out = rm.out_length(T, orig, new)
        gy = signals("noise", BATCH * 2, T_out, seed=T + 2).reshape(BATCH, 2, T_out)
        gx64 = rm.adjoint(gy, T, orig, new)
        budget = rm.abs_budget(gy, orig, new, adjoint=True, T=T)
        for fmt in ("channels_last", "channels_first"):
            layer = kapre.Resample(orig, new, data_format=fmt)
            for C in (1, 2):
                xt = torch.from_numpy(to_layout(x[:, :C], fmt)).cuda().requires_grad_(True)
                gt = torch.from_numpy(to_layout(gy[:, :C], fmt)).cuda()
                y = layer(xt)
                (y * gt).sum().backward()
                gx = to_np(xt.grad)
                assert gx.shape == xt.shape
                label = "%d->%d backward T=%d %s C=%d" % (orig, new, T, fmt, C)
                worst = max(worst, check(from_layout(gx, fmt), gx64[:, :C], budget[:, :C], n_taps, label))
                lhs = float(np.sum(to_np(y).astype(np.float64) * to_np(gt).astype(np.float64)))
                rhs = float(np.sum(to_np(xt).astype(np.float64) * gx.astype(np.float64)))
                print("resample %s: <y, gy> = %.9e, <x, gx> = %.9e" % (label, lhs, rhs))
                assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (label, lhs, rhs)
    print("resample backward %d->%d: worst ratio %.3f" % (orig, new, worst))
    kapre.check_device()


# ------------------------------------------------------------------ in front of the fused mel launch
def test_chain_with_the_mel_front_end(tmp_path):
    import torch
    import kapre_amd as kapre
    import kapre_oracle as o
    from kapre_amd import _ffi, keras_shim

    kw = dict(n_fft=400, hop_length=160, sample_rate=16000, n_mels=80, return_decibel=False)
    mel = kapre.get_melspectrogram_layer(input_shape=(None, 1), **kw)
    model = kapre.Sequential([kapre.Resample(44100, 16000, input_shape=(22050, 1)), mel])
    assert model.output_shape == mel.compute_output_shape((None, 8000, 1))
    x = signals("speech", 2, 22050, 0)[:, :, None]
    xt = torch.from_numpy(x).cuda()
    out = model(xt)
    launches = _ffi.last_launches()
    alone = kapre.Resample(44100, 16000)(xt)
    assert alone.shape == (2, 8000, 1)
    assert torch.equal(out, mel(alone)) and _ffi.last_launches() == launches       # the unchanged fused mel launch
    assert launches.startswith("k_mel")
    want = o.kapre_melspectrogram(rm.resample(x, 44100, 16000, axis=1), **kw)
    err = rel_err(to_np(out), want)
    print("resample + mel: rel_err %.3e against the oracle's mel of the float64 model" % err)
    assert out.shape == want.shape and err <= 1e-4

    xg = xt.clone().requires_grad_(True)
    model(xg).sum().backward()
    assert xg.grad.shape == xt.shape and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0

    path = os.path.join(str(tmp_path), "front_end.keras")
    model.save(path)
    again = keras_shim.load_model(path)
    assert [type(l).__name__ for l in again.layers][0] == "Resample" and again.output_shape == model.output_shape
    assert torch.equal(again(xt), out)
    kapre.check_device()
