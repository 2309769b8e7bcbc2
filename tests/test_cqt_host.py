"""CQT without a GPU: the model on a hand-worked bank, the default bank's lengths, the layer's config, shapes and refusals, the
packer, kpr_cqt_plan and kpr_cqt_f32's refusals."""
import ctypes
import os

import numpy as np
import pytest

import cqt_model


def test_model_on_a_two_bin_bank_and_a_ramp():
    """kernels (1, i, -1, -i) and (1/2, i/2) centred in it, x = 0 ... 7, hop 2: C[t, 0] = (x0 - x2) + i (x3 - x1) = -2 + 2i at
    every frame, C[t, 1] = (x[2t + 1] - i x[2t + 2]) / 2"""
    lengths, kernels = [4, 2], [np.array([1, 1j, -1, -1j]), np.array([0.5, 0.5j])]
    C, bound = cqt_model.cqt(np.arange(8.0), lengths, kernels, 2)
    assert C.shape == (3, 2) and (C[:, 0] == -2 + 2j).all()
    assert (C[:, 1] == [0.5 - 1j, 1.5 - 2j, 2.5 - 3j]).all()
    assert bound[1, 0] == 8 * cqt_model.U * (2 + 3 + 4 + 5) and bound[1, 1] == 6 * cqt_model.U * 3.5
    Cc, _ = cqt_model.cqt(np.arange(8.0), lengths, kernels, 2, center=True)         # frame 0 starts at sample -2
    assert Cc.shape == (5, 2) and Cc[0, 0] == -0 + 1j and Cc[1, 0] == -2 + 2j and Cc[4, 0] == 6 - 7j
    assert cqt_model.cqt(np.arange(7.0), lengths, kernels, 2, pad_end=True)[0][3, 1] == 0
    mag, mb = cqt_model.magnitude_bound(C, bound)
    assert mag[0, 0] == abs(-2 + 2j) and mb[0, 0] == np.sqrt(2.0) * bound[0, 0] + 3 * cqt_model.U * mag[0, 0]


def test_default_bank_lengths_and_kernels():
    from kapre_amd import backend
    lengths, offsets, kernels = backend.cqt_kernels(22050)
    assert (lengths[0], lengths[83], int(lengths.sum())) == (11339, 94, 200481)
    assert (offsets == (11339 - lengths) // 2).all() and all(len(w) == n and w.dtype == np.complex64 for w, n in zip(kernels, lengths))
    assert abs(backend.cqt_frequencies()[45] - 440.0) < 1e-6
    for k in (0, 45, 83):                                                  # norm 1, scaled by sqrt(N_k)
        assert abs(np.abs(kernels[k].astype(np.complex128)).sum() - np.sqrt(lengths[k])) < 1e-4 * np.sqrt(lengths[k])
    w2 = backend.cqt_kernels(22050, norm=2, scale=False)[2][45].astype(np.complex128)
    assert abs((np.abs(w2) ** 2).sum() - 1.0) < 1e-5


def test_layer_config_shapes_and_refusals(tmp_path):
    import kapre_amd as kapre
    from kapre_amd import keras_shim
    assert "CQT" in kapre.__all__ and "get_cqt_layer" in kapre.__all__
    layer = kapre.CQT(22050, hop_length=256, n_bins=60, center=True, output="magnitude", input_data_format="channels_first",
                      output_data_format="channels_last")
    again = kapre.CQT.from_config(layer.get_config())
    assert again.get_config() == layer.get_config() and (again._lengths == layer._lengths).all()
    assert layer.frame_length == 11339 and layer.compute_output_shape((4, 2, 5000)) == (4, 20, 60, 2)
    assert kapre.CQT(22050).compute_output_shape((None, 11339 + 4 * 512, 1)) == (None, 5, 84, 1)
    assert kapre.CQT(22050, pad_end=True, output_data_format="channels_first").compute_output_shape((2, 1000, 3)) == (2, 3, 2, 84)
    for bad in (dict(n_bins=110), dict(fmin=0.25), dict(fmin=11000.0, n_bins=1), dict(hop_length=0), dict(norm=3),
                dict(output="power"), dict(n_bins=0), dict(filter_scale=0), dict(sample_rate=-1)):
        with pytest.raises(ValueError):                                    # Nyquist, L > 65536, N < 2, ...
            kapre.CQT(**{**dict(sample_rate=22050), **bad})
    with pytest.raises(NotImplementedError):
        kapre.CQT(22050, window_name="boxcar")
    with pytest.raises(TypeError):
        kapre.backend.cqt(np.zeros((1, 20000, 1), np.float64), 22050)
    model = kapre.get_cqt_layer(22050, hop_length=256, return_decibel=True, input_shape=(22050, 1))
    assert [type(l).__name__ for l in model.layers] == ["CQT", "MagnitudeToDecibel"] and model.output_shape == (None, 42, 84, 1)
    path = os.path.join(str(tmp_path), "cqt.keras")
    model.save(path)
    loaded = keras_shim.load_model(path)
    assert [l.get_config() for l in loaded.layers] == [l.get_config() for l in model.layers]


@pytest.mark.parametrize("bank", [(22050,), (1000, 50, 20, 6), (1000, 60, 9, 3), (1000, 60, 1, 3)])
def test_packer_round_trip(bank):
    from kapre_amd import _ffi, backend
    lengths, offsets, kernels = backend.cqt_kernels(*bank)
    table, at = _ffi.cqt_pack(lengths, kernels), 0
    for j, (lo, hi) in enumerate(_ffi.cqt_tiles(lengths)):
        steps = -(-(hi - lo) // 16)
        assert lo % 16 == 0 and 0 <= lo < hi <= lengths[0] and lo <= offsets[8 * j] and offsets[8 * j] + lengths[8 * j] <= hi
        dense = table[at:at + steps * 256].reshape(steps, 4, 16, 4).transpose(0, 1, 3, 2).reshape(steps * 16, 16)
        at += steps * 256
        for b in range(8):
            k, col = 8 * j + b, dense[:, 2 * b] - 1j * dense[:, 2 * b + 1]
            want = np.zeros(steps * 16, np.complex64)
            if k < len(lengths):
                want[offsets[k] - lo:offsets[k] - lo + lengths[k]] = kernels[k]
            assert np.array_equal(col, want), (j, b)
    assert at == table.size


def test_plan_and_abi_refusals():
    from kapre_amd import _ffi, backend
    default = backend.cqt_kernels(22050)[0]
    assert _ffi.cqt_plan(default, 512)[:2] == (32, 11344) and _ffi.cqt_plan(default, 256)[:2] == (64, 11344)
    wide = _ffi.cqt_plan(backend.cqt_kernels(48000, n_bins=216, bins_per_octave=24)[0], 512)       # L = 50090: chunks
    assert wide[0] == 32 and 2048 <= wide[1] < 50090 and wide[1] % 16 == 0
    assert _ffi.cqt_plan(default, 4096)[0] == 32 and _ffi.cqt_plan(default, 4096)[1] < 4096        # frames on rows of their own
    small = backend.cqt_kernels(1000, 50, 20, 6)[0]
    old = _ffi.set_option("cqt_chunk", 40)
    try:
        assert _ffi.cqt_plan(small, 32)[1] == 48 and _ffi.cqt_plan(small, 200)[1] == 48             # rounded up to a step
    finally:
        _ffi.set_option("cqt_chunk", old)
    for bad in ([1], [4, 5], [70000], []):
        with pytest.raises(ValueError):
            _ffi.cqt_plan(bad, 32)
    with pytest.raises(ValueError):
        _ffi.cqt_plan(small, 0)
    n = np.ascontiguousarray(small, np.int32)
    floats = _ffi.cqt_pack(small, backend.cqt_kernels(1000, 50, 20, 6)[2]).size
    good = dict(batch=1, ch=1, time=900, layout=0, K=len(n), floats=floats, hop=32, out_layout=0)

    def call(**kw):
        a = {**good, **kw}
        return _ffi.lib().kpr_cqt_f32(None, a["batch"], a["ch"], a["time"], a["layout"], n.ctypes.data_as(ctypes.c_void_p), a["K"],
                                      None, a["floats"], a["hop"], 0, 0, a["out_layout"], 0, None, None)
    for bad in (dict(floats=floats - 256), dict(hop=0), dict(layout=2), dict(out_layout=-1), dict(batch=-1), dict(K=0),
                dict(K=12), dict()):                                       # K = 12: another table size; the last one: NULL pointers
        assert call(**bad) == _ffi.E_BADARG, bad
    assert call(time=2 ** 31) == _ffi.E_UNSUPPORTED
    assert call(batch=0) == 0 and call(ch=0) == 0 and call(time=163) == 0  # nothing to do, nothing launched
