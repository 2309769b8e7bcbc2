"""The adjoint of CQT without a GPU: the model against the transpose of cqt_model.cqt, the adjoint packer, kpr_cqt_adjoint_plan and
kpr_cqt_adjoint_f32's refusals, the layer's ``differentiable`` argument."""
import ctypes
import os

import numpy as np
import pytest

import cqt_adj_model
import cqt_model

BANKS = [(22050,), (1000, 50, 20, 6), (1000, 60, 9, 3), (1000, 60, 1, 3)]


@pytest.mark.parametrize("center,pad_end", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("bank", BANKS)
def test_model_is_the_transpose_of_the_forward_model(bank, center, pad_end):
    """<CQT(x), G> = <x, CQT^T(G)> over (Re, Im) as a pair of real coordinates, to 1e-12 relative in float64"""
    from kapre_amd import backend
    lengths, _, kernels = backend.cqt_kernels(*bank)
    L = int(lengths[0])
    hop = 512 if L > 1000 else 20
    time, rng = L + 2 * hop + hop // 2, np.random.default_rng(L)
    x = rng.standard_normal(time)
    C, _ = cqt_model.cqt(x, lengths, kernels, hop, center, pad_end)
    G = rng.standard_normal(C.shape) + 1j * rng.standard_normal(C.shape)
    gx, bound, covered = cqt_adj_model.cqt_adjoint(G, time, lengths, kernels, hop, center)
    lhs, rhs = (C.real * G.real + C.imag * G.imag).sum(), (x * gx).sum()
    scale = np.abs(C.real * G.real).sum() + np.abs(C.imag * G.imag).sum()
    assert gx.shape == (time,) and abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)
    assert (bound[~covered] == 0).all() and (gx[~covered] == 0).all() and (np.abs(gx) <= bound / (5 * cqt_adj_model.U)).all()


@pytest.mark.parametrize("hop", [32, 20, 7, "L+3"])
@pytest.mark.parametrize("bank", BANKS[1:])
def test_adjoint_packer_round_trip(bank, hop):
    """every B[tau][c] exactly once at the documented place, zeros elsewhere; the header indexes the fragments in order"""
    from kapre_amd import _ffi, backend
    lengths, offsets, kernels = backend.cqt_kernels(*bank)
    L = int(lengths[0])
    hop = L + 3 if hop == "L+3" else hop
    tiles = _ffi.cqt_tiles(lengths)
    B = np.zeros((L + 16 * hop + 32, 16 * len(tiles)), np.float32)
    for k in range(len(lengths)):
        B[offsets[k]:offsets[k] + lengths[k], 2 * k] = kernels[k].real
        B[offsets[k]:offsets[k] + lengths[k], 2 * k + 1] = -kernels[k].imag
    table = _ffi.cqt_pack_adjoint(lengths, kernels, hop)
    Rt = -(-min(hop, L) // 16)
    header = table[:4 * Rt * len(tiles)].view(np.int32).reshape(Rt, len(tiles), 4)
    frags = table[4 * Rt * len(tiles):].reshape(-1, 4, 16, 4)            # [fragment][kq][n][e]
    seen, at = np.zeros_like(B), 0
    for rt in range(Rt):
        for j, (lo, hi) in enumerate(tiles):
            first, d_lo, n_d, zero = header[rt, j]
            assert first == at and zero == 0 and d_lo >= 0 and (d_lo + n_d - 1) * hop + 16 * rt < L
            for d in range(d_lo, d_lo + n_d):
                t0 = d * hop + 16 * rt
                want = B[t0:t0 + 16, 16 * j:16 * j + 16].copy()           # [n][column of the tile]
                want[max(0, hop - 16 * rt):] = 0                          # those offsets belong to d + 1
                assert np.array_equal(frags[at].transpose(1, 0, 2).reshape(16, 16), want), (rt, j, d)
                assert t0 + 15 >= lo and t0 < hi                          # it meets the tile's range
                seen[t0:t0 + 16, 16 * j:16 * j + 16] += want != 0
                at += 1
    assert at == len(frags) and np.array_equal(seen, (B != 0).astype(np.float32))


def test_plan_and_abi_refusals():
    from kapre_amd import _ffi, backend
    plan = _ffi.cqt_adjoint_plan
    default = backend.cqt_kernels(22050)[0]                              # L = 11339, 11 tiles: rows of 176 floats
    assert plan(default, 512) == (64, 64 + 23 - 1, 32)                   # 32 r-tiles x one group of four row tiles
    assert plan(default, 256) == (64, 64 + 45 - 1, 16)
    assert plan(default, 32) == (64, 232, 8)                             # D = 355 in chunks of 169: 2 r-tiles x 4 row groups
    small, _, kernels = backend.cqt_kernels(1000, 50, 20, 6)
    old = _ffi.set_option("cqt_adjoint_rows", 65)
    try:
        assert plan(default, 512) == (64, 65, 32) and plan(small, 7) == (64, 65, 4)
        _ffi.set_option("cqt_adjoint_rows", 3)                            # at least a run: one d at a time
        assert plan(small, 32) == (64, 64, 8)
    finally:
        _ffi.set_option("cqt_adjoint_rows", old)
    assert plan(small, 167) == (64, 64, 11)                              # D = 1; 11 r-tiles, the last of 7 offsets
    for bad in ([1], [4, 5], [70000], []):
        with pytest.raises(ValueError):
            plan(bad, 32)
    with pytest.raises(ValueError):
        plan(small, 0)
    n = np.ascontiguousarray(small, np.int32)
    floats = _ffi.cqt_pack_adjoint(small, kernels, 32).size
    assert _ffi.cqt_pack_adjoint(small, kernels, 20).size != floats      # the table depends on the hop
    good = dict(batch=1, ch=1, time=900, layout=0, K=len(n), floats=floats, hop=32, g_layout=0)

    def call(**kw):
        a = {**good, **kw}
        return _ffi.lib().kpr_cqt_adjoint_f32(None, a["batch"], a["ch"], a["time"], a["layout"], n.ctypes.data_as(ctypes.c_void_p),
                                              a["K"], None, a["floats"], a["hop"], 0, 0, a["g_layout"], None, None)
    for bad in (dict(floats=floats - 256), dict(hop=0), dict(hop=20), dict(layout=2), dict(g_layout=-1), dict(batch=-1), dict(K=0),
                dict(K=12), dict(), dict(time=163)):                       # hop 20, K = 12: another table size; the last two: NULL
        assert call(**bad) == _ffi.E_BADARG, bad
    assert call(time=2 ** 31) == _ffi.E_UNSUPPORTED
    assert call(batch=0) == 0 and call(ch=0) == 0 and call(time=0) == 0  # nothing to do, nothing launched


def test_layer_argument_config_and_save_load(tmp_path):
    import kapre_amd as kapre
    from kapre_amd import keras_shim
    layer = kapre.CQT(22050, hop_length=256, n_bins=60, differentiable=True)
    assert layer.differentiable and layer.get_config()["differentiable"] is True
    assert kapre.CQT(22050).get_config()["differentiable"] is False and callable(kapre.backend.cqt_adjoint)
    again = kapre.CQT.from_config(layer.get_config())
    assert again.differentiable and again.get_config() == layer.get_config()
    model = kapre.get_cqt_layer(22050, hop_length=256, differentiable=True, input_shape=(22050, 1))
    path = os.path.join(str(tmp_path), "cqt_adj.keras")
    model.save(path)
    loaded = keras_shim.load_model(path)
    assert loaded.layers[0].differentiable and [l.get_config() for l in loaded.layers] == [l.get_config() for l in model.layers]
