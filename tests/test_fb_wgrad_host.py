"""The filterbank weight gradient without a GPU: kpr_filterbank_wgrad_plan's invariants and refusals, the entry point's refusals,
the TrainableFilterbank layer's config round trip, and the model against a double loop."""
import os

import numpy as np
import pytest

import fb_wgrad_model as model


def test_model_against_a_double_loop():
    rng = np.random.default_rng(0)
    x, g = rng.standard_normal((2, 3, 4, 5)), rng.standard_normal((2, 3, 4, 2))
    want = np.zeros((5, 2))
    for f in range(5):
        for m in range(2):
            want[f, m] = (x[..., f] * g[..., m]).sum()
    got, mass = model.fb_wgrad(x, g)
    assert np.allclose(got, want, rtol=1e-13, atol=0) and (np.abs(got) <= mass).all()
    assert np.allclose(model.bound(mass, 16, 3, 2), 36 * model.U / (1 - 36 * model.U) * mass, rtol=1e-15)


@pytest.mark.parametrize("fmt,c", [("channels_first", 2), ("channels_last", 1), ("channels_last", 3), ("channels_last", 8)])
@pytest.mark.parametrize("n_freq,n_filt", [(1, 1), (130, 129), (1025, 128)])
def test_plan_invariants_and_the_option(n_freq, n_filt, fmt, c):
    from kapre_amd import _ffi
    plan = lambda rows: _ffi.filterbank_wgrad_plan(rows, n_freq, n_filt, c, fmt)
    for rows in (0, 1, 100, 21248, 2_000_000):
        tf, S, n_slabs, passes = plan(rows)
        assert tf == 64 and passes == -(-n_filt // 128) and S * n_slabs >= rows and (n_slabs - 1) * S < max(rows, 1)
        assert (n_slabs == 0) == (rows == 0) and plan(rows) == (tf, S, n_slabs, passes)           # a function of the shape
    chunk = plan(1)[1]                                                     # one chunk: the smallest slab
    assert chunk in (4, 8, 16)
    old = _ffi.set_option("fb_wgrad_rows", chunk + 1)
    try:
        assert plan(10 * chunk + 1)[1:3] == (2 * chunk, 6)                 # at most n rows, rounded up to the chunk
        _ffi.set_option("fb_wgrad_rows", 1)
        assert plan(10 * chunk + 1)[1:3] == (chunk, 11)
    finally:
        _ffi.set_option("fb_wgrad_rows", old)
    assert _ffi.filterbank_wgrad_plan(21248, 1025, 128, 1, "channels_first") == (64, 688, 31, 1)


def test_bad_arguments():
    from kapre_amd import _ffi
    for bad in ((-1, 4, 4, 1, 0), (8, 0, 4, 1, 0), (8, 4, 0, 1, 0), (8, 4, 4, 0, 1), (8, 4, 4, 1, 2), (8, 64, 128, 9, 1)):
        with pytest.raises(ValueError):
            _ffi.filterbank_wgrad_plan(*bad)
    L = _ffi.lib()
    assert L.kpr_filterbank_wgrad_workspace_bytes(8, 0, 4, 1, 0) < 0
    assert L.kpr_filterbank_wgrad_workspace_bytes(16, 4, 4, 1, 0) == 0 and L.kpr_filterbank_wgrad_workspace_bytes(4096, 4, 4, 1, 0) > 0
    call = lambda batch=1, ch=1, frames=8, n_freq=4, n_filt=4, layout=0: L.kpr_filterbank_wgrad_f32(
        None, None, batch, ch, frames, n_freq, n_filt, layout, None, 0, None, None)
    for bad in (dict(), dict(batch=-1), dict(frames=-1), dict(ch=0), dict(n_freq=0), dict(n_filt=0), dict(layout=3), dict(frames=0)):
        assert call(**bad) == _ffi.E_BADARG, bad                           # (the first and the last: NULL pointers)
        assert L.kpr_last_error()
    assert call(ch=9, n_filt=128, layout=1) == _ffi.E_UNSUPPORTED


def test_layer_config_round_trip_and_refusals(tmp_path):
    import kapre_amd as kapre
    from kapre_amd import keras_shim
    mel = dict(sample_rate=8000, n_freq=65, n_mels=12)
    layer = kapre.TrainableFilterbank("mel", mel, data_format="channels_first")
    assert not isinstance(layer, kapre.ApplyFilterbank) and "TrainableFilterbank" in kapre.__all__
    assert np.array_equal(layer.filterbank, kapre.ApplyFilterbank("mel", mel).filterbank.astype(np.float32))
    assert layer.compute_output_shape((None, 2, 7, 65)) == (None, 2, 7, 12) and layer.count_params() == 65 * 12
    (w,) = layer.parameters()
    assert tuple(w.shape) == (65, 12) and w.requires_grad and layer.parameters()[0] is w
    w.data[3, 4] = -0.8125                                                 # "learned"
    assert layer.get_config()["filterbank"][3][4] == -0.8125
    again = kapre.TrainableFilterbank.from_config(layer.get_config())
    assert np.array_equal(again.filterbank, layer.filterbank) and again.get_config() == layer.get_config()
    chain = kapre.Sequential([kapre.Magnitude(), layer])
    assert chain.parameters()[0] is w and chain.count_params() == 65 * 12
    path = os.path.join(str(tmp_path), "fb.keras")
    chain.save(path)
    assert np.array_equal(keras_shim.load_model(path).layers[1].filterbank, layer.filterbank)
    assert layer.constrain_().filterbank.min() == 0.0
    explicit = kapre.TrainableFilterbank(filterbank=np.ones((5, 3)))
    assert explicit.filterbank.dtype == np.float32 and explicit.compute_output_shape((1, 9, 5, 2)) == (1, 9, 3, 2)
    with pytest.raises(NotImplementedError):
        kapre.TrainableFilterbank("mel", mel, dtype="float64")(np.zeros((1, 4, 65, 1)))
    for bad in (dict(type="bark", filterbank_kwargs={}), dict(filterbank=np.ones(4)), dict(type="mel", filterbank_kwargs=mel, data_format="x")):
        with pytest.raises(ValueError):
            kapre.TrainableFilterbank(**bad)
    with pytest.raises(ValueError):
        layer(np.zeros((1, 4, 64, 1), np.float32))                         # 64 bins for a bank of 65
    assert type(kapre.get_melspectrogram_layer(n_fft=128, n_mels=12, trainable_fb=True).layers[2]) is kapre.TrainableFilterbank
    assert type(kapre.get_log_frequency_spectrogram_layer(n_fft=128, trainable_fb=True).layers[2]) is kapre.TrainableFilterbank
    assert type(kapre.get_melspectrogram_layer(n_fft=128, n_mels=12).layers[2]) is kapre.ApplyFilterbank
