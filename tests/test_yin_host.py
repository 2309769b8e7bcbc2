"""YIN without a GPU: the model on hand-worked frames, the layer's config and shapes, kpr_yin_plan, kpr_yin_f32's refusals."""
import numpy as np
import pytest

import yin_model


def test_model_on_a_square_wave_and_a_constant():
    """x = 1, 1, -1, -1, ...: d = (0, 2W, 4W, 2W, 0, 2W, ...), so y(2) = 4/3, y(3) = 3/4, y(4) = 0, y(5) = 1: tau* = 4 and the
    parabola through (3/4, 0, 1) shifts it by -0.125 / 1.75"""
    x = np.tile([1.0, 1.0, -1.0, -1.0], 16)
    y = yin_model.curve(x, 32, 16, 8, 9)
    assert np.allclose(y[0, :6], [1.0, 1.0, 4.0 / 3.0, 0.75, 0.0, 1.0], rtol=1e-15, atol=0)
    f0, cmnd, tau = yin_model.decide(y[0], 8000.0, 2, 9, 0.1)
    assert tau == 4 and cmnd == 0.0 and f0 == 8000.0 / (4.0 - 0.125 / 1.75)
    flat = yin_model.curve(np.full(40, 0.5), 32, 16, 8, 9)
    assert (flat == 1.0).all() and yin_model.decide(flat[0], 8000.0, 2, 9, 0.1) == (4000.0, 1.0, 2)
    assert np.isnan(yin_model.curve(np.r_[np.ones(20), np.inf, np.ones(19)], 32, 16, 8, 9)[0]).all()


def test_layer_config_shapes_and_refusals():
    import kapre_amd as kapre
    assert "YIN" in kapre.__all__ and "YIN" in kapre.signal.__all__
    layer = kapre.YIN(65, 2000, 22050, pad_end=True, return_cmnd=True, data_format="channels_first")
    assert (layer.frame_length, layer.win_length, layer.hop_length) == (2048, 1024, 512) and layer._params[4:6] == (11, 340)
    again = kapre.YIN.from_config(layer.get_config())
    assert again.get_config() == layer.get_config() and again._params == layer._params
    assert layer.compute_output_shape((4, 2, 5000)) == (4, 2, 2, 10)
    assert kapre.YIN(80, 1000, 16000, frame_length=1024).compute_output_shape((1, 5805, 1)) == (1, 19, 1)
    for bad in (dict(fmin=500, fmax=400), dict(fmin=9000, fmax=10000), dict(frame_length=8192), dict(win_length=2046),
                dict(win_length=1), dict(hop_length=0), dict(trough_threshold=0.0), dict(sample_rate=-1)):
        with pytest.raises(ValueError):
            kapre.YIN(**{**dict(fmin=65, fmax=2000, sample_rate=22050), **bad})
    with pytest.raises(TypeError):
        kapre.backend.yin(np.zeros((1, 4096, 1), np.float64), 65, 2000, 22050)


def test_plan_and_abi_refusals():
    from kapre_amd import _ffi
    runs = {g: _ffi.yin_plan(*g, 2, min(340, g[0] - g[1] - 1)) for g in
            [(2048, 1024, 512), (512, 256, 64), (64, 32, 8), (400, 200, 160), (67, 30, 7), (4096, 2000, 3), (2048, 1024, 1)]}
    assert [v[1] for v in runs.values()] == [_ffi.YIN_SHARED] * 3 + [_ffi.YIN_DIRECT] * 4
    assert all(1 <= f <= 8 for f, _ in runs.values()) and runs[(2048, 1024, 512)][0] == 8 and runs[(67, 30, 7)][0] == 8
    assert _ffi.yin_plan(4096, 2, 4096, 1, 4093)[0] == 1                   # a row of 4094 lags, a hop as long as the frame
    old = _ffi.set_option("yin_variant", 1)
    try:
        assert _ffi.yin_plan(2048, 1024, 512, 11, 340)[1] == _ffi.YIN_DIRECT
    finally:
        _ffi.set_option("yin_variant", old)
    good = dict(batch=1, ch=1, time=9000, layout=0, sr=22050.0, fl=2048, W=1024, hop=512, lo=11, hi=340, thr=0.1)

    def call(**kw):
        a = {**good, **kw}
        return _ffi.lib().kpr_yin_f32(None, a["batch"], a["ch"], a["time"], a["layout"], a["sr"], a["fl"], a["W"], a["hop"], a["lo"],
                                      a["hi"], a["thr"], 0, None, None, None, None)
    for bad in (dict(fl=4097), dict(W=1), dict(W=2046), dict(hi=1024), dict(lo=339), dict(lo=0), dict(hop=0), dict(thr=0.0),
                dict(sr=0.0), dict(layout=2), dict(batch=-1), dict()):         # the last one: NULL pointers
        assert call(**bad) == _ffi.E_BADARG, bad
    assert call(time=2 ** 31) == _ffi.E_UNSUPPORTED
    assert call(batch=0) == 0 and call(ch=0) == 0 and call(time=2047) == 0   # nothing to do, nothing launched
    with pytest.raises(ValueError):
        _ffi.yin_plan(2048, 1024, 512, 11, 12)
