"""GriffinLim on the GPU (kapre_amd.GriffinLim / backend.griffin_lim, kpr_griffin_lim_f32, kpr_gl_project_f32, kpr_gl_init_f32)
against the float64 model of tests/griffin_lim_model.py.

Why no sup-norm parity of S or y after several iterations: the projection divides by |a|, so an error d on a becomes
mag d / |a| on S.  On the CPU (golden speech clip, the geometries below) a torch-float32 run strays 3e-7 from float64 after one
iteration; relative noise of 1e-6 behind each transform gives 2e-5 ... 6e-5 after one and more than 1e-4 after four; with momentum
0.99 a float32 run is 8e-4 away after 32.  Such a check would fail correct code.  What is checked instead:
 1. the step alone, elementwise: |S_dev - S_64| <= 2 u mag (6 + 2 (|R| + c |T|) / |a|), u = 2^-24 (griffin_lim_model.project_bound);
 2. the loop is bit for bit the composition of this package's own InverseSTFT, STFT and the step (buffer rotation, T_0 = 0);
 3. the convergence trace, which is well conditioned (tests/test_griffin_lim_host.py: float32 within 1e-5 of float64): every sc_n
    within 1e-4 relative of the float64 model's, and so the sc of the returned waveform recomputed by the oracle;
 4. the initial spectrum against the Philox model;
 5. the edges.
Every check prints its figures.

Measured on an MI355X: the step uses at most 0.19 of the elementwise bound and its sc is within 1.7e-7 of float64;
the traces deviate by 6e-8 ... 1.1e-6 with momentum 0 and by at most 9.2e-6 with momentum 0.99, the sc of A(y) by at most 3.9e-6;
|S_0| is within 0.72 ulp of mag, its angle within 1.5e-7 rad of the Philox model."""
import ctypes
import os

import numpy as np
import pytest

import griffin_lim_model as glm
from augment_model import state_of
from conftest import rel_err

pytestmark = pytest.mark.gpu

FORMATS = [("channels_last", "channels_last"), ("channels_last", "channels_first"), ("channels_first", "channels_last"),
           ("channels_first", "channels_first")]                       # (spectrogram, waveform)
C99 = 0.99 / 1.99


def CH():
    from kapre_amd import _ffi
    return _ffi.griffin_lim_plan(1)[0]


SIZES = {"1": lambda ch: 1, "3": lambda ch: 3, "4": lambda ch: 4, "5": lambda ch: 5, "129": lambda ch: 129,
         "CH-1": lambda ch: ch - 1, "CH": lambda ch: ch, "CH+1": lambda ch: ch + 1, "2CH+3": lambda ch: 2 * ch + 3}


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def random_s0(M, seed):
    """mag e^{i phi} with phi uniform, complex64, in M's layout"""
    phi = np.random.default_rng(seed).uniform(0, 2 * np.pi, M.shape)
    return (M * np.exp(1j * phi)).astype(np.complex64)


# ---- 1. the step alone ---------------------------------------------------------------------------------------------------
def step_inputs(n_items, item, seed):
    rng = np.random.default_rng(seed)
    R = (rng.normal(size=(n_items, item)) + 1j * rng.normal(size=(n_items, item))).astype(np.complex64)
    T = (rng.normal(size=(n_items, item)) + 1j * rng.normal(size=(n_items, item))).astype(np.complex64)
    mag = rng.random((n_items, item)).astype(np.float32)
    if item >= 4:                       # planted zeros: mag == 0, and a == 0 (R and T both 0, whatever c is)
        mag[:, 1] = 0.0
        R[:, 2] = 0.0
        T[:, 2] = 0.0
    return R, T, mag


def offset_view(x, off):
    """x on the device, its base ``off`` elements behind an aligned allocation"""
    import torch
    host = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.empty(x.size + off, dtype=host.dtype, device="cuda")
    view = buf[off:].view(x.shape)
    view.copy_(host)
    return view


@pytest.mark.parametrize("n_items", [1, 3])
@pytest.mark.parametrize("size", list(SIZES))
def test_projection_step(size, n_items):
    from kapre_amd import _ffi
    item = SIZES[size](CH())
    R, T, mag = step_inputs(n_items, item, seed=item + n_items)
    worst = 0.0
    for off in (0, 1):
        Rd, Td, md = offset_view(R, off), offset_view(T, off), offset_view(mag, off)
        for c in (0.0, C99):
            c32 = float(np.float32(c))
            S, sc = _ffi.gl_project(Rd, Td if c else None, md, c, want_sc=True)
            label = _ffi.last_launches()
            assert label == "k_gl_project<%d,%s> + k_gl_finish" % (1 if off else 4, "mom" if c else "plain"), label
            S2, sc2 = _ffi.gl_project(Rd, Td if c else None, md, c, want_sc=True)
            S_only = _ffi.gl_project(Rd, Td if c else None, md, c)
            S, sc, S2, sc2, S_only = (t.cpu().numpy() for t in (S, sc, S2, sc2, S_only))
            assert S.tobytes() == S2.tobytes() == S_only.tobytes() and sc.tobytes() == sc2.tobytes()      # the same bits
            want = glm.project(R, T if c else None, mag, c32)
            bound = glm.project_bound(R, T if c else None, mag, c32)
            err = np.abs(S.astype(np.complex128) - want)
            assert (err <= bound).all(), (size, off, c, float(np.max(err - bound)))
            share = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
            worst = max(worst, share)
            assert (S[mag == 0] == 0).all()                                          # zeros stay exact zeros
            if item >= 4:
                assert (S[:, 2] == 0).all() and (S[:, 1] == 0).all()
            sc64 = glm.sc_of(R, mag)
            sc_dev = float(np.max(np.abs(sc / sc64 - 1.0)))
            print("step %s x %d, offset %d, c %.3f: share of the bound %.3f, sc deviates by %.2e" % (size, n_items, off, c, share, sc_dev))
            assert sc_dev <= 1e-5
    print("step %s x %d: largest share of the elementwise bound %.3f" % (size, n_items, worst))


def test_projection_step_arguments():
    import torch
    from kapre_amd import _ffi
    R = torch.zeros((2, 8), dtype=torch.complex64, device="cuda")
    mag = torch.ones((2, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="T must not be NULL"):
        _ffi.gl_project(R, None, mag, 0.25)
    with pytest.raises(RuntimeError, match=r"\[0, 1\)"):
        _ffi.gl_project(R, R.clone(), mag, 1.0)
    L = _ffi.lib()
    st = _ffi.current_stream_ptr()
    assert L.kpr_gl_project_f32(_ffi.ptr(R), None, _ffi.ptr(mag), 2, 8, 0.0, _ffi.ptr(R), None, None, 0, st) == -1       # S == R
    sc = torch.zeros(2, device="cuda")
    assert L.kpr_gl_project_f32(_ffi.ptr(R), None, _ffi.ptr(mag), 2, 8, 0.0, _ffi.ptr(torch.empty_like(R)), _ffi.ptr(sc), None, 0,
                                st) == -4                                            # sc_out needs the workspace
    empty = _ffi.gl_project(R[:0], None, mag[:0], 0.0)
    assert empty.shape == (0, 8)


# ---- 2. the loop is the composition ------------------------------------------------------------------------------------------
def compose(M, S0, geo, fmts, momentum, n_iter):
    """The Python loop from this package's own layers and the step: (y, sc, [S_0, S_1, ...])"""
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi
    n_fft, win, hop, _ = geo
    inv = kapre.InverseSTFT(n_fft, win, hop, input_data_format=fmts[0], output_data_format=fmts[1])
    fwd = kapre.STFT(n_fft, win, hop, input_data_format=fmts[1], output_data_format=fmts[0])
    c = glm.momentum_c(momentum)
    S, T, scs, states = S0, torch.zeros_like(S0), [], [S0]
    for _ in range(n_iter):
        R = fwd(inv(S))
        S, sc = _ffi.gl_project(R, T if momentum else None, M, c, want_sc=True)
        T = R
        scs.append(sc)
        states.append(S)
    sc = torch.stack(scs) if scs else torch.zeros((0, M.shape[0]), device=M.device)
    return inv(S), sc, states


@pytest.mark.parametrize("fmts", FORMATS, ids=lambda f: f[0][9:] + "-" + f[1][9:])
@pytest.mark.parametrize("geo", glm.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_loop_is_the_composition(geo, fmts):
    from kapre_amd import backend
    kw = dict(n_fft=geo[0], win_length=geo[1], hop_length=geo[2], input_data_format=fmts[0], output_data_format=fmts[1],
              return_convergence=True)
    for batch in (1, 3):
        for ch in (1, 2):
            Mh = glm.speech_magnitude(geo, batch, ch, fmts[0])
            M, S0 = dev(Mh), dev(random_s0(Mh, seed=batch * 10 + ch))
            for momentum in (0.0, 0.99):
                for n_iter in (0, 1, 3):
                    y, sc = backend.griffin_lim(M, n_iter=n_iter, momentum=momentum, init=S0, **kw)
                    y_c, sc_c, states = compose(M, S0, geo, fmts, momentum, n_iter)
                    assert y.shape == y_c.shape and sc.shape == (n_iter, batch)
                    assert y.cpu().numpy().tobytes() == y_c.cpu().numpy().tobytes(), (batch, ch, momentum, n_iter)
                    assert sc.cpu().numpy().tobytes() == sc_c.cpu().numpy().tobytes(), (batch, ch, momentum, n_iter)
            # three chained classical calls of one iteration, each started from the state the step leaves, are one call of three
            y3, sc3 = backend.griffin_lim(M, n_iter=3, momentum=0.0, init=S0, **kw)
            states = compose(M, S0, geo, fmts, 0.0, 3)[2]
            for k in range(3):
                y1, sc1 = backend.griffin_lim(M, n_iter=1, momentum=0.0, init=states[k], **kw)
                assert sc1.cpu().numpy().tobytes() == sc3[k:k + 1].cpu().numpy().tobytes(), (batch, ch, k)
            assert y1.cpu().numpy().tobytes() == y3.cpu().numpy().tobytes()


# ---- 3. against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmts", FORMATS, ids=lambda f: f[0][9:] + "-" + f[1][9:])
@pytest.mark.parametrize("geo", glm.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_convergence_trace_against_the_model(geo, fmts):
    from kapre_amd import backend
    n_fft, win, hop, _ = geo
    worst = [0.0, 0.0]
    for batch, ch in ((1, 2), (3, 1)):
        Mh = glm.speech_magnitude(geo, batch, ch, fmts[0])
        for momentum in (0.0, 0.99):
            for given in (False, True):
                S0 = random_s0(Mh, seed=7 + batch) if given else None
                y, sc = backend.griffin_lim(dev(Mh), n_fft=n_fft, win_length=win, hop_length=hop, n_iter=32, momentum=momentum,
                                            rand_init=False, init=None if S0 is None else dev(S0), input_data_format=fmts[0],
                                            output_data_format=fmts[1], return_convergence=True)
                y64, sc64 = glm.griffin_lim(Mh, n_fft, win, hop, n_iter=32, momentum=momentum, S0=S0, spec_fmt=fmts[0],
                                            wave_fmt=fmts[1])
                trace = float(np.max(np.abs(sc.cpu().numpy() / sc64 - 1.0)))
                final = glm.sc_of(glm.analysis(y.cpu().numpy(), n_fft, win, hop, None, fmts[1], fmts[0]), Mh)
                final64 = glm.sc_of(glm.analysis(y64, n_fft, win, hop, None, fmts[1], fmts[0]), Mh)
                last = float(np.max(np.abs(final / final64 - 1.0)))
                print("b%d c%d momentum %.2f %s: trace deviates by %.2e, sc of A(y) by %.2e (sc_1 %.3f -> sc_32 %.3f)"
                      % (batch, ch, momentum, "given S_0" if given else "zero phase", trace, last, sc64[0].max(), sc64[-1].max()))
                worst = [max(worst[0], trace), max(worst[1], last)]
                assert y.shape == y64.shape
                assert trace <= 1e-4 and last <= 1e-4
    print("worst: trace %.2e, sc of A(y) %.2e" % tuple(worst))


# ---- 4. the initial spectrum ------------------------------------------------------------------------------------------------
def test_random_init_is_the_philox_model():
    import torch
    from kapre_amd import _ffi, augmentation
    rng = np.random.default_rng(4)
    seed = 2 ** 63 + 12345
    ch_plain = CH()
    for fmt, shape in (("channels_first", (2, 3, 5, 129)), ("channels_last", (2, 5, 129, 3)), ("channels_last", (1, 7, 33, 1)),
                       ("channels_first", (1, 1, 3, ch_plain // 3 + 1))):
        M = (0.1 + rng.random(shape)).astype(np.float32)
        for off in (0, 1):                                               # the 16-byte and the scalar instance
            augmentation.set_seed(seed)
            state = augmentation.device_state(torch.device("cuda", torch.cuda.current_device()))
            assert state_of(state) == (seed, 0)
            mag, S0 = _ffi.gl_init(offset_view(M, off), fmt, 1.0, _ffi.GL_INIT_RANDOM, state)
            assert _ffi.last_launches() == "k_gl_init<%d,rand> + k_gl_advance" % (1 if off else 4)
            assert state_of(state) == (seed, 1)                          # calls advances by exactly one
            S0 = S0.cpu().numpy().astype(np.complex128)
            ulp = float(np.max(np.abs(np.abs(S0) - M) / (M * 2.0 ** -23)))
            ang = float(np.max(np.abs(glm.wrap(np.angle(S0) - glm.philox_phase(seed, 0, shape, fmt)))))
            print("init %s %s offset %d: |S_0| within %.2f ulp of mag, angle within %.2e rad" % (fmt, shape, off, ulp, ang))
            assert ulp <= 4.0 and ang <= 1e-6
            _, again = _ffi.gl_init(offset_view(M, off), fmt, 1.0, _ffi.GL_INIT_RANDOM, state)          # calls == 1 now
            ang1 = np.abs(glm.wrap(np.angle(again.cpu().numpy().astype(np.complex128)) - glm.philox_phase(seed, 1, shape, fmt)))
            assert float(ang1.max()) <= 1e-6 and state_of(state) == (seed, 2)


def test_draw_is_identical_in_both_layouts():
    import torch
    from kapre_amd import _ffi, augmentation
    ones = torch.ones((2, 3, 5, 129), dtype=torch.float32, device="cuda")             # channels_first; S_0 is then the unit phase
    augmentation.set_seed(99)
    state = augmentation.device_state(ones.device)
    first = _ffi.gl_init(ones, "channels_first", 1.0, _ffi.GL_INIT_RANDOM, state)[1]
    augmentation.set_seed(99)
    last = _ffi.gl_init(ones.permute(0, 2, 3, 1).contiguous(), "channels_last", 1.0, _ffi.GL_INIT_RANDOM, state)[1]
    assert torch.equal(last.permute(0, 3, 1, 2), first)
    zero = _ffi.gl_init(ones, "channels_first", 1.0, _ffi.GL_INIT_ZERO)[1]
    assert torch.equal(zero, torch.complex(ones, torch.zeros_like(ones))) and state_of(state) == (99, 1)


def test_seed_reproduces_a_run():
    import kapre_amd as kapre
    from kapre_amd import augmentation
    geo = glm.GEOMETRIES[2]
    M = dev(glm.speech_magnitude(geo, 2, 2))
    layer = kapre.GriffinLim(geo[0], geo[1], geo[2], n_iter=4)
    augmentation.set_seed(5)
    a, sc_a = layer(M).cpu().numpy(), layer.last_convergence.cpu().numpy()
    b = layer(M).cpu().numpy()                                            # the generator has moved on
    augmentation.set_seed(5)
    c, sc_c = layer(M).cpu().numpy(), layer.last_convergence.cpu().numpy()
    assert a.tobytes() == c.tobytes() and sc_a.tobytes() == sc_c.tobytes() and a.tobytes() != b.tobytes()
    assert sc_a.shape == (4, 2) and layer.last_convergence.is_cuda


def test_power():
    from kapre_amd import _ffi, backend
    geo = glm.GEOMETRIES[1]
    Mh = glm.speech_magnitude(geo, 3, 1)
    M2 = (Mh * Mh).astype(np.float32)
    want = np.sqrt(M2.astype(np.float64))
    for off in (0, 1):
        mag, S0 = _ffi.gl_init(offset_view(M2, off), "channels_last", 2.0, _ffi.GL_INIT_ZERO)
        err, limit = rel_err(mag.cpu().numpy(), want), 8 * rel_err(glm.root_f32(M2, 2.0), want)
        print("power 2, offset %d: mag strays %.2e, limit 8 x float32 model = %.2e" % (off, err, limit))
        assert err <= limit
        assert np.array_equal(S0.cpu().numpy(), mag.cpu().numpy().astype(np.complex64))
    Md = dev(Mh)
    assert _ffi.gl_init(Md, "channels_last", 1.0, _ffi.GL_INIT_ZERO)[0] is Md                     # power 1: M itself
    kw = dict(n_fft=geo[0], win_length=geo[1], hop_length=geo[2], n_iter=8, rand_init=False, return_convergence=True)
    _, sc1 = backend.griffin_lim(dev(Mh), power=1.0, **kw)
    _, sc2 = backend.griffin_lim(dev(M2), power=2.0, **kw)
    dev_sc = float(np.max(np.abs(sc2.cpu().numpy() / sc1.cpu().numpy() - 1.0)))
    print("power 2 on M^2 against power 1 on M: traces differ by %.2e" % dev_sc)
    assert dev_sc <= 1e-4


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_nan_stays_in_its_item(momentum):
    from kapre_amd import backend
    geo = glm.GEOMETRIES[0]
    Mh = glm.speech_magnitude(geo, 3, 2)
    bad = Mh.copy()
    bad[1, 4, 17, 1] = np.nan
    kw = dict(n_fft=geo[0], win_length=geo[1], hop_length=geo[2], n_iter=5, momentum=momentum, rand_init=False,
              return_convergence=True)
    y, sc = (t.cpu().numpy() for t in backend.griffin_lim(dev(Mh), **kw))
    yb, scb = (t.cpu().numpy() for t in backend.griffin_lim(dev(bad), **kw))
    for item in (0, 2):
        assert y[item].tobytes() == yb[item].tobytes() and sc[:, item].tobytes() == scb[:, item].tobytes()
    assert np.isnan(scb[:, 1]).all() and np.isfinite(sc).all()


def test_length_dtype_and_grad():
    import torch
    import kapre_amd as kapre
    geo = glm.GEOMETRIES[3]
    n_fft, win, hop, frames = geo
    natural = glm.natural_length(frames, win, hop)
    M = dev(glm.speech_magnitude(geo, 2, 1, "channels_first"))
    kw = dict(n_fft=n_fft, hop_length=hop, n_iter=2, rand_init=False, input_data_format="channels_first")
    full = kapre.GriffinLim(output_data_format="channels_first", **kw)(M)
    assert full.shape == (2, 1, natural)
    for fmt in ("channels_first", "channels_last"):
        ref = full if fmt == "channels_first" else full.permute(0, 2, 1)
        axis = 2 if fmt == "channels_first" else 1
        short = kapre.GriffinLim(length=natural - 100, output_data_format=fmt, **kw)(M)
        longer = kapre.GriffinLim(length=natural + 37, output_data_format=fmt, **kw)(M)
        assert short.shape[axis] == natural - 100 and longer.shape[axis] == natural + 37 and short.is_contiguous()
        assert torch.equal(short, ref.narrow(axis, 0, natural - 100))
        assert torch.equal(longer.narrow(axis, 0, natural), ref) and not longer.narrow(axis, natural, 37).any()
    with pytest.raises(TypeError):
        kapre.GriffinLim(**kw)(M.double())
    with pytest.raises(ValueError):
        kapre.GriffinLim(**kw)(M[..., :-1])
    x = M.clone().requires_grad_(True)
    out = kapre.GriffinLim(output_data_format="channels_first", **kw)(x)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, full)
    empty = kapre.GriffinLim(output_data_format="channels_first", **kw)(M[:, :, :0])
    assert empty.shape == (2, 1, 0)


def test_c_abi_refuses_bad_arguments():
    import torch
    from kapre_amd import _ffi
    geo = glm.GEOMETRIES[0]
    M = dev(glm.speech_magnitude(geo, 1, 1))
    win = torch.ones(geo[1], device="cuda")
    g = _ffi.StftGeom(1, 1, 0, geo[0], geo[1], geo[2], 0, 0, 1, 1)
    n = int(_ffi.lib().kpr_griffin_lim_workspace_bytes(ctypes.byref(g), geo[3], 1, 1))
    ws = _ffi.workspace(n, M.device)
    out = torch.empty((1, glm.natural_length(geo[3], geo[1], geo[2]), 1), device="cuda")

    def call(n_iter=1, momentum=0.5, power=1.0, mode=0, init=None, state=None, geom=g, nbytes=n):
        return _ffi.lib().kpr_griffin_lim_f32(_ffi.ptr(M), ctypes.byref(geom), geo[3], _ffi.ptr(win), _ffi.ptr(win), n_iter, momentum,
                                              power, mode, init, state, _ffi.ptr(out), None, _ffi.ptr(ws), nbytes,
                                              _ffi.current_stream_ptr())

    assert call() == 0
    for kw in (dict(n_iter=-1), dict(momentum=1.0), dict(momentum=-0.5), dict(power=0.0), dict(mode=3), dict(mode=2), dict(mode=1),
               dict(geom=_ffi.StftGeom(1, 1, 0, geo[0], geo[1], geo[2], 0, 1, 1, 1)), dict(geom=_ffi.StftGeom(1, 0, 0, 256, 256, 64, 0, 0, 1, 1))):
        assert call(**kw) == -1, kw
    assert call(nbytes=n // 2) == -4
    torch.cuda.synchronize()


def test_sequential_runs_saves_and_loads(tmp_path):
    import torch
    import kapre_amd as kapre
    from conftest import speech
    from kapre_amd import augmentation
    from kapre_amd.keras_shim import load_model
    x = np.stack([speech(4000, 500), speech(4000, 9000)])[:, :, None]
    model = kapre.Sequential([kapre.get_stft_magnitude_layer(input_shape=(4000, 1), n_fft=256, hop_length=64, return_decibel=False),
                              kapre.GriffinLim(n_fft=256, hop_length=64, n_iter=16, rand_init=True)])
    assert model.output_shape == (None, 3968, 1)
    augmentation.set_seed(1)
    y = model.predict(x)
    assert y.shape == (2, 3968, 1) and np.isfinite(y).all()
    sc = model.layers[-1].last_convergence.cpu().numpy()
    print("Sequential: sc_1 %s -> sc_16 %s" % (sc[0], sc[-1]))
    assert sc.shape == (16, 2) and (sc[-1] < sc[0]).all()
    path = os.path.join(tmp_path, "gl.keras")
    model.save(path)
    loaded = load_model(path)
    assert loaded.output_shape == (None, 3968, 1) and loaded.layers[-1].get_config() == model.layers[-1].get_config()
    augmentation.set_seed(1)
    assert loaded.predict(x).tobytes() == y.tobytes()
    kapre.check_device()
