"""The table-free resampler on the host: the float64 model of tests/resample_direct_model.py against resample_model.py, the
dense matrix and torch's float64 autograd; the float32 restatement of the kernel's arithmetic against the error rule with the
derived constant C_of(L) -- and the float32-position variant violating it, which shows that the rule catches that
mistake; kpr_resample_direct_plan; the header, the exports and the Python surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import resample_direct_model as dm
import resample_model as rm
from conftest import REPO

PAIRS = [(25427, 24000), (24000, 25427), (10079, 8000), (55, 49), (48000, 47999), (2147483647, 2147483629), (44100, 16000)]
IDS = ["%dto%d" % p for p in PAIRS]


def same_window_as_the_library(orig, new):
    """the model's window is the library's: n_taps of kpr_resample_direct_plan in both directions"""
    from kapre_amd import _ffi

    for adjoint in (False, True):
        assert _ffi.resample_direct_plan(orig, new, 6, 0.99, adjoint)[0] == dm.shape(orig, new, 6, 0.99, adjoint)[3]


# ------------------------------------------------------------------ the float64 model
@pytest.mark.parametrize("orig,new", [(44100, 16000), (16000, 44100), (48000, 44100), (55, 49), (3, 2), (2, 3), (1, 2), (2, 1)])
def test_model_equals_the_table_model(orig, new):
    same_window_as_the_library(orig, new)
    rng = np.random.default_rng(orig + new)
    for T in (1, 5, 257, 1500):
        x = rng.standard_normal((2, T))
        y = dm.resample(x, orig, new)
        want = rm.resample(x, orig, new)
        assert y.shape == want.shape and np.max(np.abs(y - want)) <= 1e-12
        gy = rng.standard_normal(want.shape)
        gx = dm.adjoint(gy, T, orig, new)
        assert np.max(np.abs(gx - rm.adjoint(gy, T, orig, new))) <= 1e-12


@pytest.mark.parametrize("orig,new", [(3, 2), (2, 3), (55, 49), (7, 1), (1, 7), (25427, 24000), (2147483647, 2147483629)])
def test_model_equals_the_dense_matrix_and_its_adjoint_torch_autograd(orig, new):
    same_window_as_the_library(orig, new)
    import torch

    rng = np.random.default_rng(7)
    T = 61
    natural = rm.out_length(T, orig, new)
    for length in (None, natural // 2, natural + 40):
        D = dm.dense(T, orig, new, length=length)
        x = rng.standard_normal((3, T))
        y = dm.resample(x, orig, new, length=length)
        assert y.shape == (3, D.shape[0]) and np.max(np.abs(y - x @ D.T)) <= 1e-12
        gy = rng.standard_normal(y.shape)
        xt = torch.from_numpy(x).requires_grad_(True)
        (xt @ torch.from_numpy(D).T * torch.from_numpy(gy)).sum().backward()
        assert np.max(np.abs(dm.adjoint(gy, T, orig, new) - xt.grad.numpy())) <= 1e-12
    # past the filter's tail (H inputs = H P / Q outputs) the outputs are exact zeros
    P, Q, H = dm.shape(orig, new)[:3]
    tail = dm.resample(rng.standard_normal((1, T)), orig, new, length=natural + 200)[0, natural + H * P // Q + 2:]
    assert tail.size and not tail.any()


def test_model_builds_nothing_per_phase():
    """P = 2^31 - 1 phases: resample_model.bands would allocate arange(P)"""
    same_window_as_the_library(2147483647, 2147483629)
    x = np.random.default_rng(0).standard_normal(400)
    y = dm.resample(x, 2147483647, 2147483629)
    assert y.shape == (400,) and np.max(np.abs(y - 0.99 * x)) < 0.2            # nearly the identity


# ------------------------------------------------------------------ the float32 restatement and the rule
@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
@pytest.mark.parametrize("orig,new", PAIRS, ids=IDS)
def test_restatement_meets_the_rule_and_a_float_position_does_not(orig, new, adjoint):
    same_window_as_the_library(orig, new)
    assert dm.C_of(6) <= 32.0
    rng = np.random.default_rng(orig % 1000 + adjoint)
    T = 3000
    n_in = rm.out_length(T, orig, new) if adjoint else T
    n_out = T if adjoint else rm.out_length(T, orig, new)
    x = rng.standard_normal((2, n_in)).astype(np.float32)
    y64 = dm._gather(x, n_out, orig, new, 6, 0.99, adjoint, 'sum')
    bound = dm.bound(x, n_out, orig, new, adjoint=adjoint)
    worst = float(np.max(np.abs(dm.resample_f32(x, n_out, orig, new, adjoint=adjoint) - y64) / bound))
    wrong = float(np.max(np.abs(dm.resample_f32(x, n_out, orig, new, adjoint=adjoint, float_position=True) - y64) / bound))
    print("restatement %d->%d%s: worst |y - y64| / bound = %.3f; with a float32 position %.1f"
          % (orig, new, " adjoint" if adjoint else "", worst, wrong))
    assert worst <= 1.0
    assert wrong > 1.0                                                   # even 3000 samples show the mistake


def test_float_position_violates_the_rule_on_the_long_tone():
    """300 000 samples at 0.45 cycles per sample, 25427 -> 24000: a float32 position is wrong by 2^-24 i samples"""
    same_window_as_the_library(25427, 24000)
    T = 300000
    x = np.sin(2.0 * np.pi * 0.45 * np.arange(T)).astype(np.float32)[None]
    n_out = rm.out_length(T, 25427, 24000)
    y64 = dm.resample(x, 25427, 24000)
    bound = dm.bound(x, n_out, 25427, 24000)
    worst = float(np.max(np.abs(dm.resample_f32(x, n_out, 25427, 24000) - y64) / bound))
    wrong = float(np.max(np.abs(dm.resample_f32(x, n_out, 25427, 24000, float_position=True) - y64) / bound))
    print("long tone: restatement %.3f of the bound, float32 position %.0f times the bound" % (worst, wrong))
    assert worst <= 1.0 and wrong > 100.0


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("orig,new", PAIRS + [(2, 1), (1, 2), (48000, 8000), (8000, 48000), (50854, 48000), (16000, 16000)])
def test_plan_tap_counts_equal_the_models(orig, new):
    from kapre_amd import _ffi

    for adjoint in (False, True):
        n_taps, tile = _ffi.resample_direct_plan(orig, new, 6, 0.99, adjoint)
        P, Q, H, want, _, _ = dm.shape(orig, new, 6, 0.99, adjoint)
        assert n_taps == want == 2 * H and 64 <= tile <= 1024
        # the window holds the support of every output of a stretch
        a, r = dm.positions(2000, P, Q)
        U = 6 * max(rm.reduced(orig, new)) / 0.99
        assert np.all(np.abs(np.int64(-H) * P - r) >= U) and np.all(np.abs(np.int64(H + 1) * P - r) >= U)
    for L, rolloff in ((1, 1.0), (2, 0.9)):
        assert _ffi.resample_direct_plan(orig, new, L, rolloff, False)[0] == dm.shape(orig, new, L, rolloff, False)[3]


def test_plan_refusals():
    from kapre_amd import _ffi

    L = _ffi.lib()
    n, t = ctypes.c_int(0), ctypes.c_int(0)

    def text(*args):
        rc = L.kpr_resample_direct_plan(*args)
        return rc, L.kpr_last_error().decode()

    ok = (ctypes.byref(n), ctypes.byref(t))
    assert text(0, 1, 6, 0.99, 0, *ok) == (_ffi.E_BADARG, "orig_freq and new_freq must be positive, got 0 and 1")
    assert text(2, -1, 6, 0.99, 0, *ok) == (_ffi.E_BADARG, "orig_freq and new_freq must be positive, got 2 and -1")
    assert text(2, 1, 0, 0.99, 0, *ok) == (_ffi.E_BADARG, "lowpass_filter_width must be at least 1, got 0")
    assert text(2, 1, 6, 1.5, 0, *ok) == (_ffi.E_BADARG, "rolloff must lie in (0, 1], got 1.5")
    assert text(2, 1, 6, 0.99, 2, *ok) == (_ffi.E_BADARG, "adjoint must be 0 or 1, got 2")
    assert text(2, 1, 6, 0.99, 0, None, ctypes.byref(t)) == (_ffi.E_BADARG, "n_taps / outputs_per_tile must not be NULL")
    rc, msg = text(48000, 4000, 6, 0.99, 0, *ok)                          # 2 ceil(6 * 12 / 0.99) = 146 taps
    assert rc == _ffi.E_UNSUPPORTED and "a support of 146 taps; supported are at most 128 taps" in msg, msg
    assert text(48000, 4000, 6, 0.99, 1, *ok)[0] == 0                     # its adjoint has 14
    with pytest.raises(ValueError, match="a support of 146 taps"):
        _ffi.resample_direct_plan(48000, 4000, 6, 0.99, False)
    # no limit on the number of phases: the pairs the table route refuses
    with pytest.raises(ValueError, match="phases"):
        _ffi.resample_table_size(50854, 48000, 6, 0.99, False)
    assert _ffi.resample_direct_plan(50854, 48000, 6, 0.99, False)[0] == 14


def test_launcher_refusals_touch_no_device():
    """the argument checks of kpr_resample_direct_f32 come before the first HIP call of a launch"""
    from kapre_amd import _ffi

    L = _ffi.lib()
    P = ctypes.c_void_p(4096)

    def text(*args):
        rc = L.kpr_resample_direct_f32(*args)
        return rc, L.kpr_last_error().decode()

    assert text(P, -1, 1, 8, 0, 2, 1, 6, 0.99, 0, 4, P, None) == (_ffi.E_BADARG, "bad batch/channels/in_len/out_len/layout")
    assert text(P, 1, 1, 8, 0, 2, 1, 6, 0.99, 0, -4, P, None)[0] == _ffi.E_BADARG
    assert text(P, 1, 1, 8, 0, 0, 1, 6, 0.99, 0, 4, P, None)[1] == "orig_freq and new_freq must be positive, got 0 and 1"
    rc, msg = text(P, 1, 1, 8, 0, 48000, 4000, 6, 0.99, 0, 4, P, None)
    assert rc == _ffi.E_UNSUPPORTED and "146 taps" in msg
    rc, msg = text(P, 1, 2, 1 << 29, 1, 2, 1, 6, 0.99, 0, 4, P, None)
    assert rc == _ffi.E_UNSUPPORTED and "2^30 elements or more per signal" in msg
    for in_len, out_len in ((1 << 62, 4), (8, 1 << 62), ((1 << 63) - 1, (1 << 63) - 1)):      # no product that could overflow
        rc, msg = text(P, 1, 3, in_len, 1, 2, 1, 6, 0.99, 0, out_len, P, None)
        assert rc == _ffi.E_UNSUPPORTED and "2^30 elements or more per signal" in msg
    assert text(P, 1, 2, (1 << 29) - 1, 1, 2, 1, 6, 0.99, 0, 0, P, None)[0] == 0                # the largest signal, nothing to write
    assert text(P, 0, 1, 8, 0, 2, 1, 6, 0.99, 0, 4, P, None)[0] == 0      # batch == 0: nothing to do
    assert text(P, 1, 1, 8, 0, 2, 1, 6, 0.99, 0, 0, P, None)[0] == 0      # out_len == 0
    assert text(None, 1, 1, 8, 0, 2, 1, 6, 0.99, 0, 4, P, None) == (_ffi.E_BADARG, "x / out must not be NULL")
    assert text(ctypes.c_void_p(4097), 1, 1, 8, 0, 2, 1, 6, 0.99, 0, 4, P, None) == (_ffi.E_BADARG, "the pointers must be 4-byte aligned")
    assert text(P, 1, 1, 8, 0, 2, 1, 6, 0.99, 0, 4, ctypes.c_void_p(4100), None) == (_ffi.E_BADARG, "x and out overlap")


# ------------------------------------------------------------------ the surface
def test_header_exports_and_python_names():
    import kapre_amd
    from kapre_amd import _ffi, autograd, backend, signal

    header = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    for name in ("kpr_resample_direct_plan", "kpr_resample_direct_f32"):
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _ffi.EXPORTS
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    assert "getenv" not in open(os.path.join(REPO, "kapre_amd", "csrc", "kpr_resample_direct_kernels.h")).read()
    assert _ffi.lib().kpr_version() == 120
    assert callable(_ffi.resample_direct) and callable(_ffi.resample_direct_plan) and callable(autograd.resample_direct)
    assert "PitchShift" in kapre_amd.__all__ and "PitchShift" in signal.__all__ and kapre_amd.PitchShift is signal.PitchShift
    assert backend.RESAMPLE_METHODS == ('polyphase', 'direct')


def test_resample_method_and_length_arguments():
    import kapre_amd as kapre
    from kapre_amd import backend

    x = np.zeros((1, 16, 1), dtype=np.float32)
    with pytest.raises(ValueError, match="method must be 'polyphase' or 'direct'"):
        backend.resample(x, 2, 1, method='table')
    with pytest.raises(ValueError, match="length is for method='direct' only"):
        backend.resample(x, 2, 1, length=8)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="length must be None or an integer >= 0"):
            backend.resample(x, 2, 1, method='direct', length=bad)
    with pytest.raises(ValueError, match="method must be"):
        kapre.Resample(2, 1, method='fast')
    with pytest.raises(ValueError, match="1 MiB"):
        kapre.Resample(50854, 48000)                                   # today's path keeps its refusal
    with pytest.raises(ValueError, match="a support of 146 taps"):
        kapre.Resample(48000, 4000, method='direct')
    with pytest.raises(TypeError, match="float32 kernels only"):
        backend.resample(x.astype(np.float64), 2, 1, method='direct')
    layer = kapre.Resample(50854, 48000, method='direct', input_shape=(50854, 2))
    assert layer.output_shape == (None, 48000, 2)
    cfg = layer.get_config()
    assert cfg['method'] == 'direct' and kapre.Resample(2, 1).get_config()['method'] == 'polyphase'
    again = kapre.Resample.from_config(cfg)
    assert again.get_config() == cfg
    # equal rates return the input itself, with length None or the input's
    assert backend.resample(x, 5, 5, method='direct') is x and backend.resample(x, 5, 5, method='direct', length=16) is x
    assert kapre.Resample(7, 7, method='direct')(x) is x
