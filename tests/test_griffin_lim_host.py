"""GriffinLim without a GPU: the CPU model's own conditioning (why the GPU tests compare convergence traces and not spectra),
the layer's constructor, config, shapes and exports, the host-only plan call, and the Philox phase model."""
import ctypes

import numpy as np
import pytest

import griffin_lim_model as glm
import kapre_amd as kapre
from kapre_amd import _ffi, backend

CASES = [(geo, mom) for geo in glm.GEOMETRIES for mom in (0.0, 0.99)]


@pytest.fixture(scope="module")
def traces():
    """(float64 sc, float32 sc) of 32 iterations from zero phase, per case: computed once"""
    out = {}
    for geo, mom in CASES:
        M = glm.speech_magnitude(geo, batch=2)
        _, sc64 = glm.griffin_lim(M, *geo[:3], n_iter=32, momentum=mom)
        _, sc32 = glm.griffin_lim_f32(M, *geo[:3], n_iter=32, momentum=mom)
        out[geo, mom] = (sc64, sc32)
    return out


@pytest.mark.parametrize("geo,mom", CASES)
def test_float32_trace_follows_float64(traces, geo, mom):
    """the convergence trace is well conditioned: a float32 run stays within 1e-5 relative of float64 over 32 iterations"""
    sc64, sc32 = traces[geo, mom]
    dev = float(np.max(np.abs(sc32 / sc64 - 1.0)))
    print("float32 trace deviates by %.2e" % dev)
    assert dev <= 1e-5


@pytest.mark.parametrize("geo,mom", CASES)
def test_the_iteration_converges(traces, geo, mom):
    sc64, _ = traces[geo, mom]
    print("sc_32 / sc_1 =", sc64[-1] / sc64[0])
    assert (sc64[-1] < 0.6 * sc64[0]).all()


def test_model_composes():
    """n_iter = 0 is one synthesis of S_0; three runs of one classical iteration chained through S equal one run of three"""
    geo = glm.GEOMETRIES[0]
    M = glm.speech_magnitude(geo, batch=1)
    y0, sc0 = glm.griffin_lim(M, *geo[:3], n_iter=0)
    assert sc0.shape == (0, 1)
    np.testing.assert_allclose(y0, glm.synthesis(M.astype(np.complex128), *geo[:3], None, 'channels_last', 'channels_last'))
    y3, sc3 = glm.griffin_lim(M, *geo[:3], n_iter=3, momentum=0.0)
    S = M.astype(np.complex128)
    for n in range(3):
        R = glm.analysis(glm.synthesis(S, *geo[:3], None, 'channels_last', 'channels_last'), *geo[:3], None, 'channels_last',
                         'channels_last')
        np.testing.assert_allclose(glm.sc_of(R, M), sc3[n], rtol=1e-12)
        S = glm.project(R, None, M, 0.0)
    np.testing.assert_allclose(glm.synthesis(S, *geo[:3], None, 'channels_last', 'channels_last'), y3, atol=1e-12)


def test_projection_model_edges():
    R = np.array([3 + 4j, 0j, 1 + 0j, 2 - 2j])
    T = np.array([1 + 1j, 0j, 2 + 0j, 0j])
    mag = np.array([2.0, 5.0, 0.0, 1.0])
    S = glm.project(R, T, mag, 0.5)
    assert S[1] == 0 and S[2] == 0                                   # a == 0 and mag == 0
    np.testing.assert_allclose(np.abs(S[[0, 3]]), mag[[0, 3]], rtol=1e-12)
    np.testing.assert_allclose(glm.project(R, None, mag, 0.0)[0], 2.0 * (3 + 4j) / 5.0, rtol=1e-15)
    b = glm.project_bound(R, T, mag, 0.5)
    assert b[2] == 0 and b[1] == 2 * glm.U32 * 5.0 * 6.0 and (b[[0, 3]] > 0).all()


# ---- the layer ------------------------------------------------------------------------------------------------------------
def test_exports():
    assert "GriffinLim" in kapre.__all__ and "GriffinLim" in kapre.time_frequency.__all__
    assert kapre.GriffinLim is kapre.time_frequency.GriffinLim
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("kpr_griffin_lim_plan", "kpr_gl_project_f32", "kpr_gl_init_f32", "kpr_griffin_lim_workspace_bytes",
                 "kpr_griffin_lim_f32"):
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
    for name in ("kpr_gl_project_f32", "kpr_gl_init_f32", "kpr_griffin_lim_f32"):
        assert _ffi.EXPORTS[name][1][-1] is ctypes.c_void_p          # the stream comes last
    for fn in ("griffin_lim", "gl_project", "gl_init", "griffin_lim_plan"):
        assert callable(getattr(_ffi, fn))
    assert callable(backend.griffin_lim)
    assert _ffi.lib().kpr_version() == 120


def test_defaults_and_config_round_trip():
    layer = kapre.GriffinLim()
    cfg = layer.get_config()
    assert {k: cfg[k] for k in ('n_fft', 'win_length', 'hop_length', 'window_name', 'n_iter', 'momentum', 'power', 'rand_init',
                                'length', 'input_data_format', 'output_data_format')} == dict(
        n_fft=2048, win_length=2048, hop_length=512, window_name=None, n_iter=32, momentum=0.99, power=1.0, rand_init=True,
        length=None, input_data_format='default', output_data_format='default')
    layer = kapre.GriffinLim(n_fft=512, win_length=400, hop_length=100, window_name='hamming_window', n_iter=7, momentum=0.5,
                             power=2.0, rand_init=False, length=1234, input_data_format='channels_first',
                             output_data_format='channels_last', name='gl')
    again = kapre.GriffinLim.from_config(layer.get_config())
    assert again.get_config() == layer.get_config() and again.name == 'gl'
    assert again.input_data_format == 'channels_first' and again.output_data_format == 'channels_last'
    import json
    json.dumps(layer.get_config())
    assert kapre.keras_shim.get_registered_object('Kapre>GriffinLim') is kapre.GriffinLim


@pytest.mark.parametrize("kw", [dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=float('nan')), dict(n_iter=-1),
                                dict(n_iter=2.5), dict(power=0.0), dict(power=-1.0), dict(power=float('inf')), dict(length=-1)])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        kapre.GriffinLim(n_fft=256, **kw)


def test_constructor_refuses_names():
    with pytest.raises(NotImplementedError):
        kapre.GriffinLim(window_name='no_such_window')
    with pytest.raises(ValueError):
        kapre.GriffinLim(input_data_format='channels_middle')
    with pytest.raises(ValueError):
        backend.griffin_lim(np.zeros((1, 2, 129, 1), np.float32), n_fft=256, momentum=1.5)
    assert kapre.GriffinLim(n_fft=256, momentum=0, n_iter=0).momentum == 0.0


def test_output_shapes():
    layer = kapre.GriffinLim(n_fft=512, win_length=400, hop_length=100)
    assert layer.compute_output_shape((None, 7, 257, 2)) == (None, 1000, 2)
    assert layer.compute_output_shape((4, None, 257, 1)) == (4, None, 1)
    assert layer.compute_output_shape((4, 0, 257, 1)) == (4, 0, 1)
    layer = kapre.GriffinLim(n_fft=512, win_length=400, hop_length=100, input_data_format='channels_first',
                             output_data_format='channels_first', length=777)
    assert layer.compute_output_shape((None, 2, 7, 257)) == (None, 2, 777)
    assert layer.compute_output_shape((None, 2, None, 257)) == (None, 2, 777)
    mixed = kapre.GriffinLim(n_fft=256, input_data_format='channels_first', output_data_format='channels_last')
    assert mixed.compute_output_shape((3, 2, 9, 129)) == (3, 8 * 64 + 256, 2)
    # behind the magnitude front end the frame count round-trips: the natural length never exceeds the input's
    model = kapre.Sequential([kapre.get_stft_magnitude_layer(input_shape=(4000, 1), n_fft=256, hop_length=64, return_decibel=False),
                              kapre.GriffinLim(n_fft=256, hop_length=64)])
    assert model.output_shape == (None, 3968, 1)


def test_inputs_are_checked_before_the_device():
    layer = kapre.GriffinLim(n_fft=256, hop_length=64)
    with pytest.raises(TypeError):
        layer(np.zeros((1, 9, 129, 1), np.float64))
    with pytest.raises(ValueError):
        layer(np.zeros((9, 129, 1), np.float32))
    with pytest.raises(TypeError):
        kapre.GriffinLim(n_fft=256, dtype='float64')(np.zeros((1, 9, 129, 1), np.float32))


def test_plan_reports_the_tiling():
    ch, n = _ffi.griffin_lim_plan(1)
    assert ch >= 256 and ch % 4 == 0 and n == 1
    assert _ffi.griffin_lim_plan(ch) == (ch, 1) and _ffi.griffin_lim_plan(ch + 1) == (ch, 2)
    assert _ffi.griffin_lim_plan(2 * ch + 3) == (ch, 3) and _ffi.griffin_lim_plan(0) == (ch, 0)
    L = _ffi.lib()
    assert L.kpr_griffin_lim_plan(-1, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) != 0
    g = _ffi.StftGeom(3, 2, 0, 512, 400, 100, 0, 0, 1, 1)
    with_mom = L.kpr_griffin_lim_workspace_bytes(ctypes.byref(g), 7, 1, 0)
    without = L.kpr_griffin_lim_workspace_bytes(ctypes.byref(g), 7, 0, 0)
    n_bytes = 3 * 2 * 7 * 257 * 8
    assert with_mom - without >= n_bytes and without >= 2 * n_bytes           # S and one R; the second R / T with momentum
    assert L.kpr_griffin_lim_workspace_bytes(ctypes.byref(g), 7, 0, 1) - without >= n_bytes // 2     # mag
    padded = _ffi.StftGeom(3, 2, 0, 512, 400, 100, 1, 0, 1, 1)
    assert L.kpr_griffin_lim_workspace_bytes(ctypes.byref(padded), 7, 0, 0) == -1 and b"pad" in L.kpr_last_error()


# ---- the initial phase -------------------------------------------------------------------------------------------------------
def test_philox_phase_is_independent_of_the_layout():
    last = glm.philox_phase(2 ** 63 + 11, 3, (2, 5, 7, 3), 'channels_last')
    first = glm.philox_phase(2 ** 63 + 11, 3, (2, 3, 5, 7), 'channels_first')
    assert last.shape == (2, 5, 7, 3) and np.array_equal(last, np.transpose(first, (0, 2, 3, 1)))
    assert 0.0 <= first.min() and first.max() < 2 * np.pi
    # one Philox block serves four consecutive elements; calls and seed both change the stream
    assert not np.array_equal(first, glm.philox_phase(2 ** 63 + 11, 4, (2, 3, 5, 7), 'channels_first'))
    assert not np.array_equal(first, glm.philox_phase(2 ** 63 + 12, 3, (2, 3, 5, 7), 'channels_first'))
    # a longer tensor starts with the same draws: the draw of an element depends on its index alone
    longer = glm.philox_phase(2 ** 63 + 11, 3, (1, 1, 40, 7), 'channels_first').ravel()
    assert np.array_equal(longer[:first[0].size], first[0].ravel())
    # uniform enough: 16 sectors of 210 draws, none empty and none with a third of them
    hist = np.histogram(first, bins=16, range=(0, 2 * np.pi))[0]
    assert hist.min() > 0 and hist.max() < first.size // 3


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='GriffinLim expects a rank-4 input'):
        kapre.GriffinLim(n_fft=256, hop_length=64)(np.zeros((9, 129, 1), np.float32))
    with pytest.raises(TypeError, match='GriffinLim has float32 kernels only; got a float64 input'):
        kapre.GriffinLim(n_fft=256, hop_length=64)(np.zeros((1, 9, 129, 1), np.float64))
    with pytest.raises(ValueError, match='GriffinLim expects a rank-4 input'):
        kapre.GriffinLim(n_fft=256, hop_length=64)(np.zeros((9, 129, 1), np.float64))
    with pytest.raises(ValueError, match='GriffinLim expects a rank-4 input'):
        backend.griffin_lim(np.zeros((9, 129, 1), np.float32), n_fft=256, hop_length=64)
    with pytest.raises(TypeError, match='GriffinLim has float32 kernels only; got a float64 input'):
        backend.griffin_lim(np.zeros((1, 9, 129, 1), np.float64), n_fft=256, hop_length=64)
    with pytest.raises(ValueError, match='GriffinLim expects a rank-4 input'):
        backend.griffin_lim(np.zeros((9, 129, 1), np.float64), n_fft=256, hop_length=64)
