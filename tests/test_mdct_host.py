"""MDCT / InverseMDCT without a device: the float64 model (tests/mdct_model.py) against the fast form the kernels implement and
against itself (perfect reconstruction), the layers' host side, kpr_mdct_plan, option mdct_run, and the refusals of the two entry
points with fabricated pointers that are never dereferenced (codes: 0 nothing to do, -1 KPR_E_BADARG, -2 KPR_E_UNSUPPORTED)."""
import numpy as np
import pytest

import kapre_amd
import mdct_model as mm
from kapre_amd import _ffi, backend
from kapre_amd.keras_shim import Sequential


@pytest.mark.parametrize("N", [16, 512])
@pytest.mark.parametrize("norm", [None, "ortho"])
@pytest.mark.parametrize("window", sorted(mm.WINDOWS))
def test_model_fast_form_and_reconstruction(N, norm, window):
    x = np.random.default_rng(1).standard_normal((2, 5 * N + 3))
    w, (s, si) = mm.WINDOWS[window](N), mm.scales(N, norm)
    if N == 16:
        assert np.abs(mm.mdct_fast(x[0, :N], w, s) - mm.mdct(x[0, :N], N, w, s)[0]).max() < 1e-13
    y = mm.inverse_mdct(mm.mdct(x, N, w, s, True, True), N, w, si, True)
    assert np.abs(y[..., :x.shape[-1]] - x).max() < 1e-11
    assert np.abs(getattr(backend, window + "_window")(N, np.float64) - w).max() < 1e-15


def test_layers_host_side():
    fwd = kapre_amd.MDCT(frame_length=512, window_name="sine_window", norm="ortho", pad_begin=True, pad_end=True,
                         input_data_format="channels_first", output_data_format="channels_last")
    inv = kapre_amd.InverseMDCT(window_name="sine_window", norm="ortho", pad_begin=True, length=1000)
    for layer in (fwd, inv):
        again = type(layer).from_config(layer.get_config())
        assert again.get_config() == layer.get_config()
    assert fwd.compute_output_shape((3, 2, 1000)) == (3, mm.frame_count(1000, 512, True, True), 256, 2)
    assert kapre_amd.MDCT(512).compute_output_shape((3, 1000, 2)) == (3, 2, 256, 2)
    assert kapre_amd.MDCT(512).compute_output_shape((3, 500, 2)) == (3, 0, 256, 2)
    assert inv.compute_output_shape((3, 5, 256, 2)) == (3, 1000, 2)
    assert kapre_amd.InverseMDCT(pad_begin=True).compute_output_shape((3, 5, 256, 2)) == (3, 5 * 256, 2)
    seq = Sequential([fwd, kapre_amd.InverseMDCT(input_data_format="channels_last")])
    assert [l.get_config() for l in Sequential.from_config(seq.get_config()).layers] == [l.get_config() for l in seq.layers]
    assert {"MDCT", "InverseMDCT"} <= set(kapre_amd.__all__) & set(kapre_amd.time_frequency.__all__)
    with pytest.raises(TypeError):
        kapre_amd.MDCT(512)(np.zeros((1, 1000, 1), np.float64))
    with pytest.raises(TypeError):
        kapre_amd.InverseMDCT()(np.zeros((1, 3, 256, 1), np.float64))
    for bad in (dict(frame_length=1000), dict(norm="backward"), dict(window_name=np.ones(100))):
        with pytest.raises(ValueError):
            kapre_amd.MDCT(**{"frame_length": 512, **bad})


def test_plan_and_run_option():
    assert [_ffi.mdct_plan(N)[1] for N in (512, 1024, 2048, 4096)] == [8, 16, 32, 64]
    old = _ffi.set_option("mdct_run", 3)
    try:
        assert _ffi.set_option("mdct_run", 3) == 3 and _ffi.mdct_plan(2048)[0] == 3
    finally:
        _ffi.set_option("mdct_run", old)
    assert _ffi.mdct_plan(2048)[0] >= 8
    with pytest.raises(ValueError):
        _ffi.mdct_plan(1000)


X, W, OUT = 0x10000000, 0x30000000, 0x20000000
ORDER = {"kpr_mdct_f32": "x batch ch n layout N w norm adjoint pad_begin pad_end out_layout out stream",
         "kpr_imdct_f32": "x batch ch n layout N w norm adjoint pad_begin out_len out_layout out stream"}
# two series of 2000 samples: 6 frames of 256 coefficients; the inverse: 6 frames -> 1792 samples
GOOD = {"kpr_mdct_f32": dict(x=X, batch=1, ch=2, n=2000, layout=0, N=512, w=W, norm=0, adjoint=0, pad_begin=0, pad_end=0, out_layout=0,
                             out=OUT, stream=None),
        "kpr_imdct_f32": dict(x=X, batch=1, ch=2, n=6, layout=0, N=512, w=W, norm=0, adjoint=0, pad_begin=0, out_len=1792, out_layout=0,
                              out=OUT, stream=None)}
SHARED = [(dict(batch=-1), -1), (dict(ch=-1), -1), (dict(n=-1), -1), (dict(layout=2), -1), (dict(out_layout=2), -1), (dict(norm=2), -1),
          (dict(adjoint=2), -1), (dict(pad_begin=2), -1), (dict(N=1000), -2), (dict(N=256), -2), (dict(N=8192), -2),
          (dict(ch=0), 0), (dict(batch=0), 0),
          (dict(x=None), -1), (dict(w=None), -1), (dict(out=None), -1), (dict(x=X + 2), -1), (dict(w=W + 1), -1), (dict(out=OUT + 2), -1),
          (dict(out=W + 2044), -1), (dict(out=W - 4), -1)]
ROWS = {"kpr_mdct_f32": SHARED + [(dict(pad_end=2), -1), (dict(n=1 << 31), -2), (dict(n=500), 0), (dict(out=X + 15996), -1),
                                  (dict(x=OUT + 12284), -1)],
        "kpr_imdct_f32": SHARED + [(dict(out_len=-1), -1), (dict(out_len=1 << 31), -2), (dict(out_len=0), 0), (dict(out=X + 12284), -1),
                                   (dict(x=OUT + 14332), -1), (dict(n=0, out_len=0), 0)]}


@pytest.mark.parametrize("name", sorted(ORDER))
def test_return_codes(name):
    L, order, good = _ffi.lib(), ORDER[name].split(), GOOD[name]
    got = [(change, getattr(L, name)(*[{**good, **change}[k] for k in order])) for change, _ in ROWS[name]]
    assert got == ROWS[name]
    getattr(L, name)(*[{**good, "N": 1000}[k] for k in order])
    assert all(size in L.kpr_last_error() for size in (b"512", b"1024", b"2048", b"4096"))
