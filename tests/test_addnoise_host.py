"""AddNoise without a GPU: the models of tests/mix_model.py against a direct loop, the achieved signal-to-noise ratio, the draw's
restatement, ``backend.noise_bank``, the argument checks of the C entry points through ctypes (fake pointers: every call fails its
checks before anything is launched), the workspace and plan queries, the layer surface, and the records."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import kapre_amd as kapre
from kapre_amd import _ffi, backend
from conftest import REPO

import mix_model as mm

RNG = np.random.default_rng(20263)
NULL = ctypes.c_void_p(0)


def P(addr):
    return ctypes.c_void_p(addr)                # never dereferenced


# ------------------------------------------------------------------ the models
@pytest.mark.parametrize("C,T,L,o,snr", [(1, 1, 1, 0, 0.0), (1, 7, 3, 2, 20.0), (2, 5, 5, 4, -5.0), (3, 9, 37, 36, 10.0), (2, 11, 4, 1, 3.5)])
def test_model_against_a_direct_loop(C, T, L, o, snr):
    bank, lengths = backend.noise_bank([RNG.standard_normal(L), RNG.standard_normal(L + 2)])
    x = RNG.standard_normal((2, C, T)).astype(np.float32)
    index, offset, snrs = [0, 1], [o, min(o, L + 1)], np.array([snr, snr + 1.0], dtype=np.float32)
    seg = mm.segments(bank, lengths, index, offset, T)
    y, stats = mm.forward64(x, seg, snrs)
    for b in range(2):
        n = bank[index[b]].astype(np.float64)
        Lb = int(lengths[index[b]])
        Sx = Sn = 0.0
        for t in range(T):
            assert seg[b, t] == n[(offset[b] + t) % Lb]
            Sn += seg[b, t] ** 2
            for c in range(C):
                Sx += float(x[b, c, t]) ** 2
        g = math.sqrt((Sx / (C * T)) / (Sn / T)) * 10.0 ** (-float(snrs[b]) / 20.0)
        assert abs(stats[b, 0] - Sx) <= 1e-14 * Sx and abs(stats[b, 1] - Sn) <= 1e-14 * Sn and abs(stats[b, 2] - g) <= 1e-14 * g
        for c in range(C):
            for t in range(T):
                assert abs(y[b, c, t] - (float(x[b, c, t]) + g * seg[b, t])) <= 1e-14 * (abs(y[b, c, t]) + 1.0)
    # backward: gx = gy + (<gy, seg> g / Sx) x, against central differences of the float64 forward
    gy = RNG.standard_normal(x.shape)
    gx, D, coef = mm.backward64(x, gy, seg, stats)
    x64 = x.astype(np.float64)
    d = RNG.standard_normal(x.shape)
    eps = 1e-6
    yp, _ = mm.forward64(x64 + eps * d, seg, snrs)
    ym, _ = mm.forward64(x64 - eps * d, seg, snrs)
    lhs, rhs = float(np.sum(gx * d)), float(np.sum((yp - ym) * gy)) / (2 * eps)
    assert abs(lhs - rhs) <= 1e-7 * max(abs(rhs), 1.0)
    for b in range(2):
        assert abs(D[b] - sum(gy[b, c, t] * seg[b, t] for c in range(C) for t in range(T))) <= 1e-12 * (abs(D[b]) + 1.0)


def test_achieved_snr_is_the_request():
    bank, lengths = backend.noise_bank([RNG.standard_normal(4099), RNG.standard_normal(37)])
    for C, T in ((1, 20000), (2, 5000), (3, 11)):
        x = RNG.standard_normal((4, C, T)).astype(np.float32)
        snr = np.array([-5.0, 0.0, 20.0, 40.0], dtype=np.float32)
        seg = mm.segments(bank, lengths, [0, 1, 0, 1], [0, 36, 4098, 5], T)
        y, stats = mm.forward64(x, seg, snr)
        got = mm.achieved_snr_db(x, y)
        print("achieved - requested dB:", (got - snr).tolist())
        assert np.max(np.abs(got - snr)) <= 1e-9


def test_zero_energy_in_the_model_and_the_float32_restatement():
    bank, lengths = backend.noise_bank([[0.0, 0.0, 1.0], [0.0, 0.0]])
    x = RNG.standard_normal((3, 2, 2)).astype(np.float32)
    x[1] = 0.0
    seg = mm.segments(bank, lengths, [0, 0, 1], [0, 2, 0], 2)               # item 0: a silent stretch of noise 0; item 2: a silent noise
    y64, stats = mm.forward64(x, seg, np.zeros(3, np.float32))
    assert stats[0, 2] == 0.0 and stats[1, 2] == 0.0 and stats[2, 2] == 0.0
    assert np.array_equal(y64, x.astype(np.float64)) and np.array_equal(mm.forward32(x, seg, np.zeros(3, np.float32)), x)
    gx, D, coef = mm.backward64(x, np.ones_like(x), seg, stats)
    assert np.array_equal(gx, np.ones(x.shape))


def test_float32_restatement_obeys_the_forward_bound():
    worst = 0.0
    for T, L, snr in ((1, 1, 0.0), (5, 3, -5.0), (777, 37, 20.0), (20000, 4099, 40.0), (8193, 5, 3.0)):
        bank, lengths = backend.noise_bank(RNG.standard_normal(L))
        x = RNG.standard_normal((2, 1, T)).astype(np.float32)
        seg = mm.segments(bank, lengths, [0, 0], [0, L - 1], T)
        s = np.full(2, snr, np.float32)
        y64, stats = mm.forward64(x, seg, s)
        ratio = np.max(np.abs(mm.forward32(x, seg, s).astype(np.float64) - y64) / mm.forward_bound(y64, stats, seg))
        worst = max(worst, float(ratio))
    print("float32 restatement, worst |y - y64| / bound = %.4f" % worst)
    assert worst <= 1.0


def test_noise_draw_model():
    lengths = [1, 7, 4099]
    a = mm.noise_draw(1234, 0, 4096, lengths, 5.0, 20.0)
    assert a.dtype == np.int32 and a.shape == (4096, 4)
    assert a[:, 0].min() >= 0 and a[:, 0].max() <= 2 and np.all(a[:, 3] == 0)
    assert np.all(a[:, 1] >= 0) and np.all(a[:, 1] < np.asarray(lengths)[a[:, 0]])
    snr = a[:, 2].copy().view(np.float32)
    assert snr.min() >= 5.0 and snr.max() <= 20.0 and 12.0 < snr.mean() < 13.0
    assert np.array_equal(a, mm.noise_draw(1234, 0, 4096, lengths, 5.0, 20.0))
    assert not np.array_equal(a, mm.noise_draw(1234, 1, 4096, lengths, 5.0, 20.0))
    assert np.array_equal(a[:7], mm.noise_draw(1234, 0, 7, lengths, 5.0, 20.0))         # an entry does not depend on the item count
    fixed = mm.noise_draw(99, 5, 100, [3], 7.25, 7.25)
    assert np.all(fixed[:, 0] == 0) and np.all(fixed[:, 2].copy().view(np.float32) == np.float32(7.25))
    sigma = np.sqrt(4096 * (1 / 3) * (2 / 3))
    assert np.all(np.abs(np.bincount(a[:, 0], minlength=3) - 4096 / 3) <= 6 * sigma)
    # the snr formula: one float64 fma, one rounding to float32
    assert mm.snr_value(5.0, 20.0, 0) == np.float32(5.0)
    assert mm.snr_value(5.0, 20.0, 1 << 31) == np.float32(12.5)
    assert mm.snr_value(-5.0, 40.0, (1 << 32) - 1) <= np.float32(40.0)


# ------------------------------------------------------------------ the bank
def test_noise_bank_shapes():
    bank, lengths = backend.noise_bank(np.arange(1, 6))
    assert bank.dtype == np.float32 and bank.shape == (1, 5) and lengths.dtype == np.int32 and lengths.tolist() == [5]
    bank, lengths = backend.noise_bank(np.ones((3, 4)))
    assert bank.shape == (3, 4) and lengths.tolist() == [4, 4, 4]
    bank, lengths = backend.noise_bank([np.ones(2), np.arange(1, 8), [3.0]])
    assert bank.shape == (3, 7) and lengths.tolist() == [2, 7, 1]
    assert bank[0].tolist() == [1, 1, 0, 0, 0, 0, 0] and bank[2].tolist() == [3, 0, 0, 0, 0, 0, 0]
    assert bank[1].tolist() == list(range(1, 8))
    bank, lengths = backend.noise_bank([[1.0, 2.0], [3.0, 4.0]])                   # nested lists of equal length: (n, L)
    assert bank.tolist() == [[1.0, 2.0], [3.0, 4.0]] and lengths.tolist() == [2, 2]


def test_noise_bank_errors():
    for bad in ([], np.zeros((0, 4)), np.zeros((2, 0)), [np.ones(3), np.zeros(0)], np.zeros((2, 2, 2)), [1.0, np.nan],
                [np.ones(3), np.array([1.0, np.inf])], 3.0, [np.ones(3), np.ones((2, 2))], "noise"):
        with pytest.raises(ValueError):
            backend.noise_bank(bad)


# ------------------------------------------------------------------ the C entry points, argument errors only
def _fwd(x=P(0x100000), batch=2, channels=1, time=100, layout=0, noise=P(0x200000), n_noise=2, stride=50, lengths=P(0x300000),
         table=P(0x400000), out=P(0x500000), stats=P(0x600000), ws=P(0x700000), ws_bytes=1 << 20):
    return _ffi.lib().kpr_add_noise_f32(x, batch, channels, time, layout, noise, n_noise, stride, lengths, table, out, stats, ws,
                                        ws_bytes, NULL)


def _bwd(gy=P(0x800000), x=P(0x100000), batch=2, channels=1, time=100, layout=0, noise=P(0x200000), n_noise=2, stride=50,
         lengths=P(0x300000), table=P(0x400000), stats=P(0x600000), gx=P(0x500000), stats_out=NULL, ws=P(0x700000), ws_bytes=1 << 20):
    return _ffi.lib().kpr_add_noise_bwd_f32(gy, x, batch, channels, time, layout, noise, n_noise, stride, lengths, table, stats, gx,
                                            stats_out, ws, ws_bytes, NULL)


def _err():
    return _ffi.lib().kpr_last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_add_noise_argument_errors(call):
    out_name = "out" if call is _fwd else "gx"
    for kw in (dict(x=NULL), {out_name: NULL}, dict(noise=NULL), dict(lengths=NULL), dict(table=NULL), dict(stats=NULL)):
        assert call(**kw) == -1 and b"NULL" in _err(), kw
    assert call(n_noise=0) == -1 and b"n_noise" in _err()
    assert call(stride=0) == -1 and b"stride" in _err()
    assert call(time=0) == -1 and b"time" in _err()
    assert call(channels=0) == -1 and call(batch=-1) == -1 and call(layout=2) == -1
    assert call(time=1 << 30) == -2 and b"2^30" in _err()
    assert call(time=1 << 29, channels=2) == -2 and b"2^30" in _err()
    assert call(**{out_name: P(0x100000)}) == -1 and b"overlap" in _err()               # in place
    assert call(**{out_name: P(0x100000 + 4 * 150)}) == -1 and b"overlap" in _err()       # out starts inside x
    assert call(**{out_name: P(0x200000)}) == -1 and b"overlap" in _err()               # out on the bank
    assert call(x=P(0x100002)) == -1 and b"aligned" in _err()
    assert call(stats=P(0x600004)) == -1 and b"aligned" in _err()
    # the workspace: only the streamed form asks for it
    old = _ffi.set_option("addnoise_variant", 1)
    try:
        need = _ffi.add_noise_workspace_bytes(2, 1, 100, 0)
        assert call(ws=NULL) == -4 and b"workspace" in _err()
        assert call(ws_bytes=need - 1) == -4 and b"workspace" in _err() and str(need).encode() in _err()
        assert call(ws=P(0x500000)) == -1 and b"workspace overlaps" in _err()
    finally:
        _ffi.set_option("addnoise_variant", old)
    assert call(batch=0) == 0                                                         # nothing to do, nothing launched
    if call is _bwd:
        assert call(gy=NULL) == -1 and b"NULL" in _err()
        assert call(gx=P(0x800000)) == -1 and b"overlap" in _err()                    # gx on gy


def test_noise_draw_argument_errors():
    L = _ffi.lib()

    def draw(table=P(0x10000), n_items=4, n_noise=3, lengths=P(0x20000), lo=5.0, hi=20.0, state=P(0x30000)):
        return L.kpr_noise_draw(table, n_items, n_noise, lengths, lo, hi, state, NULL)

    assert draw(n_noise=0) == -1 and b"n_noise" in _err()
    assert draw(n_items=-1) == -1
    assert draw(lo=20.0, hi=5.0) == -1 and b"snr" in _err()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert draw(lo=bad) == -1 and b"snr" in _err()
        assert draw(hi=bad) == -1 and b"snr" in _err()
    assert draw(state=NULL) == -1 and b"state" in _err()
    assert draw(lengths=NULL) == -1 and b"lengths" in _err()
    assert draw(table=NULL) == -1 and b"table" in _err()
    assert draw(table=P(0x10004)) == -1 and b"aligned" in _err()
    assert draw(table=P(0x30000 - 16)) == -1 and b"overlaps" in _err()                # the table runs into the state
    assert draw(n_items=(1 << 20) + 1, state=P(0x8000000), lengths=P(0x9000000)) == -2 and b"2^20" in _err()


def test_plan_and_workspace_queries():
    K, chunks, limit, form = _ffi.add_noise_plan(256, 1, 44100, "channels_last")
    assert K == 8192 and chunks == 6 and limit >= 44100 and form == _ffi.ADDNOISE_RESIDENT      # the headline item is resident
    assert _ffi.add_noise_workspace_bytes(256, 1, 44100, "channels_last") == 256 * 6 * 16
    assert _ffi.add_noise_plan(256, 1, limit, 0)[3] == _ffi.ADDNOISE_RESIDENT
    assert _ffi.add_noise_plan(256, 1, limit + 1, 0)[3] == _ffi.ADDNOISE_STREAMED
    assert _ffi.add_noise_plan(256, 2, limit // 2 + 1, 1)[3] == _ffi.ADDNOISE_STREAMED
    # the automatic rule (profiles/addnoise_times.md): resident needs a workgroup per compute unit, 256 items
    assert _ffi.add_noise_plan(255, 1, 44100, 0)[3] == _ffi.ADDNOISE_STREAMED
    assert _ffi.add_noise_plan(8, 1, 5, 0)[3] == _ffi.ADDNOISE_STREAMED
    assert _ffi.add_noise_plan(3, 2, 5, 1)[:2] == (K, 1) and _ffi.add_noise_plan(3, 1, K + 1, 1)[1] == 2
    assert _ffi.add_noise_workspace_bytes(0, 1, 5, 0) == 0
    old = _ffi.set_option("addnoise_variant", 1)
    try:
        assert _ffi.add_noise_plan(256, 1, 44100, 1)[3] == _ffi.ADDNOISE_STREAMED
        _ffi.set_option("addnoise_variant", 2)
        assert _ffi.add_noise_plan(256, 1, 44100, 1)[3] == _ffi.ADDNOISE_RESIDENT
        assert _ffi.add_noise_plan(8, 1, limit, 0)[3] == _ffi.ADDNOISE_RESIDENT
        assert _ffi.add_noise_plan(8, 1, limit + 1, 0)[3] == _ffi.ADDNOISE_STREAMED
        with pytest.raises(RuntimeError, match="outside"):
            _ffi.set_option("addnoise_variant", 3)
    finally:
        _ffi.set_option("addnoise_variant", old)
    L = _ffi.lib()
    assert L.kpr_add_noise_workspace_bytes(1, 0, 5, 0) == -1 and L.kpr_add_noise_workspace_bytes(1, 1, 0, 0) == -1
    assert L.kpr_add_noise_workspace_bytes(1, 1, 1 << 30, 0) == -1
    out = (ctypes.c_int * 4)()
    assert L.kpr_add_noise_plan(1, 1, 5, 0, None) == -1 and L.kpr_add_noise_plan(1, 1, 5, 3, out) == -1


# ------------------------------------------------------------------ the layer surface
def test_layer_config_round_trip(tmp_path):
    noises = [RNG.standard_normal(5), RNG.standard_normal(9)]
    layer = kapre.AddNoise(noises, snr_db=(0.0, 15.0), input_data_format='channels_first', name='musan')
    cfg = layer.get_config()
    assert cfg['snr_db'] == [0.0, 15.0] and cfg['input_data_format'] == 'channels_first' and cfg['name'] == 'musan'
    assert [len(n) for n in cfg['noises']] == [5, 9]
    assert np.array_equal(np.asarray(cfg['noises'][1], dtype=np.float32), noises[1].astype(np.float32))
    again = kapre.AddNoise.from_config(cfg)
    assert again.get_config() == cfg
    assert np.array_equal(again._plan.bank, layer._plan.bank) and np.array_equal(again._plan.lengths, layer._plan.lengths)
    fixed = kapre.AddNoise(np.ones(4), snr_db=10)
    assert fixed.get_config()['snr_db'] == 10.0 and fixed._snr == (10.0, 10.0)
    assert kapre.AddNoise.from_config(fixed.get_config()).get_config() == fixed.get_config()
    assert kapre.AddNoise(np.ones(4)).get_config()['snr_db'] == [5.0, 20.0]
    from kapre_amd.keras_shim import Sequential, get_registered_object, load_model
    assert get_registered_object('Kapre>AddNoise') is kapre.AddNoise
    assert kapre.augmentation.AddNoise is kapre.AddNoise
    model = Sequential([kapre.AddNoise(noises, snr_db=(0.0, 15.0), input_shape=(100, 1))])
    path = str(tmp_path / "noisy")
    model.save(path)
    loaded = load_model(path)
    assert loaded.layers[-1].get_config()['noises'] == model.layers[-1].get_config()['noises']
    assert loaded.layers[-1].get_config()['snr_db'] == [0.0, 15.0]
    assert layer.compute_output_shape((None, 2, 100)) == (None, 2, 100)


def test_layer_argument_errors():
    for bad in ((5.0, 1.0), (1.0, 2.0, 3.0), float("nan"), (0.0, float("inf")), ()):
        with pytest.raises(ValueError):
            kapre.AddNoise(np.ones(4), snr_db=bad)
    with pytest.raises(ValueError):
        kapre.AddNoise([])
    with pytest.raises(ValueError):
        kapre.AddNoise(np.ones(4), input_data_format='weird')
    layer = kapre.AddNoise(np.ones(4))
    with pytest.raises(ValueError):
        layer(np.zeros((2, 100), np.float32), training=True)
    with pytest.raises(TypeError):
        layer(np.zeros((2, 100, 1), np.float64), training=True)
    with pytest.raises(TypeError):
        backend.add_noise(np.zeros((2, 100, 1), np.float64), np.ones(4), 10.0)
    with pytest.raises(ValueError):
        backend.add_noise(np.zeros((2, 100), np.float32), np.ones(4), 10.0)


def test_without_training_the_layer_returns_its_input():
    layer = kapre.AddNoise(RNG.standard_normal((3, 50)))
    x = np.zeros((2, 100, 1), dtype=np.float32)
    assert layer(x) is x and layer(x, training=False) is x and layer(x, training=None) is x
    assert layer.last_draw is None and layer.last_stats is None


def test_training_without_a_gpu_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    layer = kapre.AddNoise(RNG.standard_normal((3, 50)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(np.zeros((2, 100, 1), dtype=np.float32), training=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        backend.add_noise(np.zeros((2, 100, 1), dtype=np.float32), np.ones(4), 10.0)


def test_noise_table_host_checks():
    lengths = np.array([3, 7], dtype=np.int32)
    for kw in (dict(index=[0, 2]), dict(index=[-1, 0]), dict(index=[0, 1], offset=[3, 0]), dict(offset=[0, -1]),
               dict(index=[0, 1, 1]), dict(offset=[0.5, 1.0])):
        with pytest.raises(ValueError):
            backend.noise_table(2, "cpu", lengths, 10.0, **kw)
    with pytest.raises(ValueError):
        backend.noise_table(2, "cpu", lengths, [1.0, float("nan")])
    t = backend.noise_table(2, "cpu", lengths, [1.0, 2.5], index=[1, 0], offset=[6, 2]).numpy()
    assert t.dtype == np.int32 and t[:, :2].tolist() == [[1, 6], [0, 2]] and np.all(t[:, 3] == 0)
    assert t[:, 2].copy().view(np.float32).tolist() == [1.0, 2.5]


# ------------------------------------------------------------------ records
def test_exports_and_names():
    assert "AddNoise" in kapre.__all__ and "AddNoise" in kapre.augmentation.__all__
    text = open(os.path.join(REPO, "include", "kapre_hip.h")).read()
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("kpr_noise_draw", "kpr_add_noise_plan", "kpr_add_noise_workspace_bytes", "kpr_add_noise_f32", "kpr_add_noise_bwd_f32"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _ffi.EXPORTS and hasattr(handle, name), name
    for name in ("kpr_noise_draw", "kpr_add_noise_f32", "kpr_add_noise_bwd_f32"):
        assert _ffi.EXPORTS[name][1][-1] is ctypes.c_void_p                           # the stream comes last
    assert re.search(r"#define KPR_VERSION 120\b", text) and _ffi.lib().kpr_version() == 120
    assert "addnoise_variant" in text
    hip = open(os.path.join(REPO, "kapre_amd", "csrc", "kapre_hip.hip")).read()
    assert "kpr_mix_kernels.h" in hip and "kpr_host_mix.h" in hip


def test_documents_name_the_new_kernels():
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "kpr_mix_kernels.h" in readme and "AddNoise" in readme and "addnoise_variant" in readme
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "4.19" in design and "k_mix_res" in design and "k_mix_sums" in design
    assert "kpr_add_noise_f32" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(REPO, "tools", "kbench_addnoise.py"))
    assert os.path.exists(os.path.join(REPO, "profiles", "addnoise_times.md"))


def test_install_as_kapre_reaches_the_layer():
    import subprocess
    import sys
    code = ("import kapre_amd; kapre_amd.install_as_kapre(); from kapre.augmentation import AddNoise; import kapre; "
            "assert AddNoise is kapre_amd.AddNoise and kapre.AddNoise is AddNoise")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


def test_refusal_table_rank_first_then_64_bit():
    """each intake of this operation: the rank error, the 64-bit refusal with its exception class, and the rank error when both
    apply -- all raised on the input as given, before a device is looked for"""
    with pytest.raises(ValueError, match='add_noise expects a rank-3 waveform batch'):
        backend.add_noise(np.zeros((2, 100), np.float32), np.ones(4), 10.0)
    with pytest.raises(TypeError, match='add_noise has float32 kernels only; got a float64 input'):
        backend.add_noise(np.zeros((2, 100, 1), np.float64), np.ones(4), 10.0)
    with pytest.raises(ValueError, match='add_noise expects a rank-3 waveform batch'):
        backend.add_noise(np.zeros((2, 100), np.float64), np.ones(4), 10.0)
    with pytest.raises(ValueError, match='AddNoise expects a rank-3 waveform batch'):
        kapre.AddNoise(np.ones(4))(np.zeros((2, 100), np.float32), training=True)
    with pytest.raises(TypeError, match='AddNoise has float32 kernels only; got a float64 input'):
        kapre.AddNoise(np.ones(4))(np.zeros((2, 100, 1), np.float64), training=True)
    with pytest.raises(ValueError, match='AddNoise expects a rank-3 waveform batch'):
        kapre.AddNoise(np.ones(4))(np.zeros((2, 100), np.float64), training=True)
