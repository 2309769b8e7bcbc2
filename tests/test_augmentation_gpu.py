"""-m gpu: SpecAugment and ChannelSwap on the device (kapre_amd/augmentation.py, csrc/kpr_augment_kernels.h).

Checker: tests/augment_model.py -- the draw rule (Philox4x32-10, pinned to published vectors in test_augmentation_host.py) and
the reference's masks (kapre/augmentation.py:211-214, :264) in numpy.  The device table must equal the model entry for entry,
the outputs must equal `np.where(mask, mask_value, x)` bit for bit.  Gradients: torch float64 autograd of the same arithmetic on
the CPU with the table / permutation fixed, in the style and with the tolerances of tests/test_autograd.py.
"""
import numpy as np
import pytest
import torch

import augment_model as am
from test_autograd import CL, CF, ref_stft, ref_db, to_bct, loss_of, cotangent, check, wave

import kapre_amd as kapre
from kapre_amd import SpecAugment, ChannelSwap, Sequential, _ffi, augmentation, backend
from kapre_amd.composed import get_melspectrogram_layer

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _state(seed, calls):
    return torch.tensor([augmentation._as_int64(seed), augmentation._as_int64(calls)], dtype=torch.int64).to(_dev())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _special_values(shape, seed):
    """float32 data with NaN (two payloads), +-Inf, -0.0 and denormals sprinkled in"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 30 - 40).astype(np.float32)
    flat = _bits(x).reshape(-1)
    specials = np.array([0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000],
                        np.uint32)
    idx = rng.choice(flat.size, size=min(flat.size // 3, 4000), replace=False)
    flat[idx] = specials[np.arange(idx.size) % specials.size]
    return x


def _expected(x_btf, table, n_tm, mask_value):
    """np.where(mask, mask_value, x) on the bit patterns"""
    b, t, f = x_btf.shape
    mask = am.mask_from_table(table, n_tm, t, f)
    return np.where(mask, _bits(np.float32(mask_value).reshape(1))[0], _bits(x_btf)), mask


# ---------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------
DRAW_CASES = [
    # items, n_time, n_freq, n_time_masks, time_param, n_freq_masks, freq_param
    (4, 256, 128, 3, 10, 4, 5),          # the reference's own test shape
    (256, 83, 128, 3, 10, 4, 5),
    (16, 83, 1025, 3, 10, 4, 5),
    (2048, 998, 80, 3, 10, 4, 5),
    (64, 16, 8, 2, 16, 3, 8),            # parameters equal to the axis lengths
    (32, 83, 128, 0, 10, 4, 5),          # no time masks
    (32, 83, 128, 3, 10, 0, 5),          # no frequency masks
    (5, 83, 128, 32, 83, 32, 128),       # the cap: 32 masks per axis
]


@pytest.mark.parametrize('items,n_time,n_freq,n_tm,tp,n_fm,fp', DRAW_CASES)
def test_device_table_equals_the_model(items, n_time, n_freq, n_tm, tp, n_fm, fp):
    seed, calls = 0xfedcba9876543210, (1 << 32) - 2           # the counter crosses a 32-bit boundary on the way
    state = _state(seed, calls)
    for k in range(3):
        table = _ffi.spec_augment_draw(state, items, n_tm, n_fm, n_time, n_freq, tp, fp)
        assert table.shape == (items, n_tm + n_fm, 2) and table.dtype == torch.int32
        assert _ffi.last_launches() == 'k_specaug_draw'
        want = am.draw_table(seed, calls + k, items, n_tm, n_fm, n_time, n_freq, tp, fp)
        got = table.cpu().numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert am.state_of(state) == (seed, calls + k + 1)           # one launch, one step
        first, last = got[..., 0], got[..., 1]
        limit = np.where(np.arange(n_tm + n_fm) < n_tm, n_time, n_freq)[None, :]
        assert (first >= 0).all() and (first <= last).all() and (last < limit).all()


def test_draw_rejects_what_the_reference_rejects():
    state = _state(1, 0)
    with pytest.raises(RuntimeError, match='time_mask_param'):
        _ffi.spec_augment_draw(state, 2, 1, 1, 9, 128, 10, 5)
    with pytest.raises(RuntimeError, match='freq_mask_param'):
        _ffi.spec_augment_draw(state, 2, 1, 1, 83, 4, 10, 5)
    with pytest.raises(RuntimeError, match='mask counts'):
        _ffi.spec_augment_draw(state, 2, 33, 1, 83, 128, 10, 5)
    assert am.state_of(state) == (1, 0)                              # a refused call draws nothing


def test_set_seed_makes_runs_identical():
    x = torch.from_numpy(_special_values((6, 83, 128, 1), 3)).to(_dev())
    layer = SpecAugment(5, 10, n_freq_masks=4, n_time_masks=3, mask_value=-80.0)
    runs = []
    for _ in range(2):
        augmentation.set_seed(20240607)
        assert am.state_of(augmentation.device_state(x.device)) == (20240607, 0)
        ys, ts = [], []
        for _ in range(3):
            ys.append(_bits(layer(x, training=True).cpu().numpy()))
            ts.append(layer.last_mask_table.cpu().numpy())
        runs.append((ys, ts))
        assert am.state_of(augmentation.device_state(x.device)) == (20240607, 3)
    for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]):
        assert np.array_equal(a, b)
    assert not np.array_equal(runs[0][1][0], runs[0][1][1])          # call after call: new masks
    for k in range(3):
        assert np.array_equal(runs[0][1][k], am.draw_table(20240607, k, 6, 3, 4, 83, 128, 10, 5))
    augmentation.set_seed(1)
    layer(x, training=True)
    assert not np.array_equal(layer.last_mask_table.cpu().numpy(), runs[0][1][0])


# ---------------------------------------------------------------------------------------------
# the masks
# ---------------------------------------------------------------------------------------------
APPLY_SHAPES = [(6, 83, 128), (5, 37, 1025), (4, 50, 201), (3, 998, 80), (7, 16, 3), (2, 300, 8192)]


@pytest.mark.parametrize('batch,n_time,n_freq', APPLY_SHAPES)
@pytest.mark.parametrize('fmt', [CL, CF])
@pytest.mark.parametrize('mask_value', [0.0, -80.0])
def test_layer_output_is_where_of_the_table_bit_for_bit(batch, n_time, n_freq, fmt, mask_value):
    x_btf = _special_values((batch, n_time, n_freq), seed=n_freq)
    x_np = x_btf[..., None] if fmt == CL else x_btf[:, None]
    x = torch.from_numpy(x_np).to(_dev())
    keep = x.clone()
    tp, fp = min(10, n_time), min(5, n_freq)
    layer = SpecAugment(freq_mask_param=fp, time_mask_param=tp, n_freq_masks=4, n_time_masks=3, mask_value=mask_value,
                        data_format=fmt)
    augmentation.set_seed(n_time * 1000 + n_freq)
    seed, calls = am.state_of(augmentation.device_state(x.device))
    y = layer(x, training=True)
    assert y is not x and y.shape == x.shape and y.dtype == torch.float32
    assert _ffi.last_launches() == 'k_specaug_apply'
    assert torch.equal(x.view(torch.int32), keep.view(torch.int32))              # the stand-alone layer leaves its input alone
    table = layer.last_mask_table.cpu().numpy()
    assert np.array_equal(table, am.draw_table(seed, calls, batch, 3, 4, n_time, n_freq, tp, fp))
    want, mask = _expected(x_btf, table, 3, mask_value)
    got = _bits(y.cpu().numpy()).reshape(batch, n_time, n_freq)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert mask.any()
    # in place (out == x): the same bits
    z = x.clone()
    assert _ffi.spec_augment_apply(z, layer.last_mask_table, 3, 4, n_time, n_freq, mask_value, inplace=True) is z
    assert _ffi.last_launches() == 'k_specaug_apply'
    assert np.array_equal(_bits(z.cpu().numpy()).reshape(batch, n_time, n_freq), want)


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_bases_that_are_not_16_byte_aligned(offset):
    batch, n_time, n_freq = 3, 41, 201
    n = batch * n_time * n_freq
    x_btf = _special_values((batch, n_time, n_freq), seed=offset)
    buf = torch.zeros(n + 8, dtype=torch.float32, device=_dev())
    x = buf[offset:offset + n].view(batch, n_time, n_freq, 1)
    x.copy_(torch.from_numpy(x_btf[..., None]))
    obuf = torch.full((n + 8,), 7.0, dtype=torch.float32, device=_dev())
    table_np = am.draw_table(5, offset, batch, 3, 4, n_time, n_freq, 10, 5)
    table = torch.from_numpy(table_np).to(_dev())
    want, _ = _expected(x_btf, table_np, 3, -80.0)
    for o_off in (0, offset):
        out = obuf[o_off:o_off + n].view(batch, n_time, n_freq, 1)
        _ffi._call('kpr_spec_augment_apply_f32', x.device, _ffi.ptr(x), _ffi.ptr(out), _ffi.ptr(table), batch, 3, 4, n_time, n_freq,
                   -80.0)
        assert np.array_equal(_bits(out.cpu().numpy()).reshape(batch, n_time, n_freq), want)
        assert (obuf[:o_off] == 7.0).all() and (obuf[o_off + n:] == 7.0).all()      # nothing outside the block
        obuf.fill_(7.0)
    _ffi.spec_augment_apply(x, table, 3, 4, n_time, n_freq, -80.0, inplace=True)          # in place, on the unaligned view
    assert np.array_equal(_bits(x.cpu().numpy()).reshape(batch, n_time, n_freq), want)
    assert (buf[:offset] == 0).all() and (buf[offset + n:] == 0).all()


def test_apply_refuses_overlap_and_long_rows():
    x = torch.zeros(4 * 10 * 12 + 4, dtype=torch.float32, device=_dev())
    table = torch.zeros((4, 2, 2), dtype=torch.int32, device=_dev())
    args = (_ffi.ptr(table), 4, 1, 1, 10, 12, 0.0)
    with pytest.raises(RuntimeError, match='overlap'):
        _ffi._call('kpr_spec_augment_apply_f32', x.device, _ffi.ptr(x), _ffi.ptr(x[4:]), *args)
    with pytest.raises(RuntimeError, match='65536'):
        _ffi._call('kpr_spec_augment_apply_f32', x.device, _ffi.ptr(x), _ffi.ptr(x[4:]), _ffi.ptr(table), 1, 1, 1, 1, 65537, 0.0)


def test_float64_and_numpy_inputs_compute_in_float32():
    x_btf = _special_values((3, 40, 64), seed=11)
    finite = np.nan_to_num(x_btf, nan=1.0, posinf=2.0, neginf=-2.0)
    layer = SpecAugment(5, 10, n_freq_masks=2, n_time_masks=2, mask_value=-1.0, dtype='float64')
    y = layer(finite[..., None].astype(np.float64), training=True)
    assert y.dtype == torch.float32 and y.is_cuda
    want, _ = _expected(finite, layer.last_mask_table.cpu().numpy(), 2, -1.0)
    assert np.array_equal(_bits(y.cpu().numpy()).reshape(3, 40, 64), want)


# ---------------------------------------------------------------------------------------------
# behind the fused mel chain
# ---------------------------------------------------------------------------------------------
def _mel_layers(fmt=CL, ch=1, t=22050, n_fft=1024, hop=256, n_mels=80, decibel=True):
    return get_melspectrogram_layer(input_shape=(t, ch) if fmt == CL else (ch, t), n_fft=n_fft, hop_length=hop, sample_rate=22050,
                                    n_mels=n_mels, return_decibel=decibel, input_data_format=fmt, output_data_format=fmt,
                                    pad_end=True)


@pytest.mark.parametrize('fmt', [CL, CF])
def test_sequential_masks_the_fused_output_in_place(fmt):
    x = wave(5, 1, 22050, fmt, seed=5).to(_dev())
    keep = x.clone()
    plain = Sequential([_mel_layers(fmt)])
    aug = SpecAugment(freq_mask_param=5, time_mask_param=10, n_freq_masks=4, n_time_masks=3, mask_value=-80.0, data_format=fmt)
    model = Sequential([_mel_layers(fmt), aug])
    base = plain(x)
    base_launches = _ffi.last_launches()
    assert base_launches
    # inference: the model without the layer, bit for bit and launch for launch
    for training in (None, False):
        y = model(x, training=training) if training is not None else model(x)
        assert _ffi.last_launches() == base_launches
        assert torch.equal(y.view(torch.int32), base.view(torch.int32))
    # training: that output, masked with the table of the call -- in place on the fused kernel's output
    augmentation.set_seed(99)
    live = torch.cuda.memory_allocated()
    y = model(x, training=True)
    assert _ffi.last_launches() == 'k_specaug_apply'
    assert torch.cuda.memory_allocated() - live < 1.5 * base.numel() * 4          # one block: the fused output, masked in place
    b, n_time, n_freq = (base.shape[0], base.shape[1], base.shape[2]) if fmt == CL else (base.shape[0], base.shape[2], base.shape[3])
    table = aug.last_mask_table.cpu().numpy()
    assert np.array_equal(table, am.draw_table(99, 0, b, 3, 4, n_time, n_freq, 10, 5))
    want, mask = _expected(base.cpu().numpy().reshape(b, n_time, n_freq), table, 3, -80.0)
    assert np.array_equal(_bits(y.cpu().numpy()).reshape(b, n_time, n_freq), want)
    assert mask.any() and torch.equal(x, keep)
    assert torch.equal(plain(x).view(torch.int32), base.view(torch.int32))       # (nothing of the other model was touched)


def test_the_chains_own_input_is_never_masked_in_place():
    spec = torch.from_numpy(_special_values((4, 83, 128, 1), 8)).to(_dev())
    keep = spec.clone()
    aug = SpecAugment(5, 10, n_freq_masks=4, n_time_masks=3)
    y = Sequential([aug])(spec, training=True)
    assert _ffi.last_launches() == 'k_specaug_apply' and y is not spec
    assert torch.equal(spec.view(torch.int32), keep.view(torch.int32))
    # two augmentation layers in a row: the second one owns what the first produced
    aug2 = SpecAugment(5, 10, n_freq_masks=1, n_time_masks=1, mask_value=3.0)
    y2 = Sequential([aug, aug2])(spec, training=True)
    assert _ffi.last_launches() == 'k_specaug_apply'
    assert torch.equal(spec.view(torch.int32), keep.view(torch.int32))
    w1, _ = _expected(keep.cpu().numpy().reshape(4, 83, 128), aug.last_mask_table.cpu().numpy(), 3, 0.0)
    w2, _ = _expected(w1.view(np.float32), aug2.last_mask_table.cpu().numpy(), 1, 3.0)
    assert np.array_equal(_bits(y2.cpu().numpy()).reshape(4, 83, 128), w2)


def test_a_view_of_the_chains_input_is_not_masked_in_place():
    """fuse_and_run's ownership rule (keras_shim.Layer): a layer of the package that hands back a view of its input has not
    produced a tensor of its own -- SpecAugment behind it runs out of place and the caller's data stay as they are."""
    from kapre_amd import keras_shim

    class Window(keras_shim.Layer):                      # stands for a layer of the package: the rule goes by the module
        def call(self, x):
            return x[:, :, :, :]

    Window.__module__ = 'kapre_amd.time_frequency'
    spec = torch.from_numpy(_special_values((4, 83, 128, 1), 9)).to(_dev())
    keep = spec.clone()
    aug = SpecAugment(5, 10, n_freq_masks=4, n_time_masks=3, mask_value=-80.0)
    y = Sequential([Window(), aug])(spec, training=True)
    assert torch.equal(spec.view(torch.int32), keep.view(torch.int32))
    assert y.untyped_storage().data_ptr() != spec.untyped_storage().data_ptr()
    want, mask = _expected(keep.cpu().numpy().reshape(4, 83, 128), aug.last_mask_table.cpu().numpy(), 3, -80.0)
    assert mask.any() and np.array_equal(_bits(y.cpu().numpy()).reshape(4, 83, 128), want)


def test_captured_graph_draws_new_masks_at_every_replay():
    x = wave(4, 1, 22050, CL, seed=6).to(_dev())
    aug = SpecAugment(freq_mask_param=5, time_mask_param=10, n_freq_masks=4, n_time_masks=3, mask_value=-80.0)
    model = Sequential([_mel_layers(CL), aug])
    base = Sequential([_mel_layers(CL)])(x).cpu().numpy()
    b, n_time, n_freq = base.shape[:3]
    augmentation.set_seed(4242)
    model(x, training=True)                                  # warm-up: the device state exists before the capture
    torch.cuda.synchronize()
    state = augmentation.device_state(x.device)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        model(x, training=True)                              # the plans and workspaces of this stream
        torch.cuda.synchronize()
        seed, calls = am.state_of(state)
        with torch.cuda.graph(graph, stream=side):
            y = model(x, training=True)
    torch.cuda.synchronize()
    assert (seed, calls) == (4242, 2) and am.state_of(state) == (4242, 2)      # capturing runs nothing
    table_t = aug.last_mask_table
    tables = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        table = table_t.cpu().numpy().copy()
        assert np.array_equal(table, am.draw_table(seed, calls + k, b, 3, 4, n_time, n_freq, 10, 5)), k
        want, _ = _expected(base.reshape(b, n_time, n_freq), table, 3, -80.0)
        assert np.array_equal(_bits(y.cpu().numpy()).reshape(b, n_time, n_freq), want), k
        tables.append(table)
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])
    assert am.state_of(state) == (4242, 5)


# ---------------------------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------------------------
def _ref_mask(yr, table, n_tm, mask_value, fmt):
    """torch float64 where(mask, mask_value, y) with the table fixed"""
    n_time, n_freq = (yr.shape[1], yr.shape[2]) if fmt == CL else (yr.shape[2], yr.shape[3])
    mask = torch.from_numpy(am.mask_from_table(table, n_tm, n_time, n_freq))
    mask = mask[..., None] if fmt == CL else mask[:, None]
    return torch.where(mask, torch.tensor(mask_value, dtype=torch.float64), yr)


@pytest.mark.parametrize('fmt', [CL, CF])
def test_spec_augment_backward(fmt):
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn((4, 83, 201, 1) if fmt == CL else (4, 1, 83, 201), generator=g, dtype=torch.float32)
    layer = SpecAugment(freq_mask_param=20, time_mask_param=10, n_freq_masks=4, n_time_masks=3, mask_value=-3.0, data_format=fmt)
    xg = x0.to(_dev()).requires_grad_(True)
    y = layer(xg, training=True)
    assert y.grad_fn is not None and _ffi.last_launches() == 'k_specaug_apply'
    r = cotangent(y.shape, False, seed=32)
    loss_of(y, r).backward()
    xr = x0.to(torch.float64).requires_grad_(True)
    yr = _ref_mask(xr, layer.last_mask_table.cpu().numpy(), 3, -3.0, fmt)
    np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().numpy(), atol=1e-6)
    loss_of(yr, r).backward()
    check(xg.grad, xr.grad, 2e-4, 'dL/dx through SpecAugment')
    assert (xg.grad == 0).any() and (xg.grad != 0).any()
    assert layer(xg, training=False) is xg                       # inference: the tensor itself, graph and all


@pytest.mark.parametrize('fmt,decibel', [(CL, True), (CF, False)])
def test_spec_augment_backward_behind_the_fused_mel_chain(fmt, decibel):
    n_fft, hop, n_mels, t = 1024, 256, 80, 6 * 1024
    mel = get_melspectrogram_layer(input_shape=(t, 1) if fmt == CL else (1, t), n_fft=n_fft, hop_length=hop, sample_rate=22050,
                                   n_mels=n_mels, return_decibel=decibel, db_dynamic_range=60.0, input_data_format=fmt,
                                   output_data_format=fmt, pad_end=True)
    aug = SpecAugment(freq_mask_param=8, time_mask_param=5, n_freq_masks=2, n_time_masks=2, mask_value=-60.0 if decibel else 0.0,
                      data_format=fmt)
    model = Sequential([mel, aug])
    x0 = wave(3, 1, t, fmt, seed=41)
    xg = x0.to(_dev()).requires_grad_(True)
    y = model(xg, training=True)
    assert y.grad_fn is not None and _ffi.last_launches() == 'k_specaug_apply'       # out of place under the tape
    r = cotangent(y.shape, False, seed=42)
    loss_of(y, r).backward()

    xr = x0.to(torch.float64).requires_grad_(True)
    window = backend.get_window_fn(None)(n_fft).astype(np.float64)
    fb = torch.as_tensor(np.asarray(mel.layers[2].filterbank, np.float64))
    m = ref_stft(to_bct(xr, fmt), n_fft, n_fft, hop, window, False, True).abs() @ fb
    m = m.permute(0, 2, 3, 1) if fmt == CL else m
    yr = ref_db(m, 1.0, 1e-5, 60.0) if decibel else m
    yr = _ref_mask(yr, aug.last_mask_table.cpu().numpy(), 2, aug.mask_value, fmt)
    assert tuple(yr.shape) == tuple(y.shape)
    loss_of(yr, r).backward()
    check(xg.grad, xr.grad, 3e-4, 'dL/dx through the fused mel chain and SpecAugment')


# ---------------------------------------------------------------------------------------------
# ChannelSwap
# ---------------------------------------------------------------------------------------------
def _swap_input(shape, complex_, seed):
    rng = np.random.default_rng(seed)
    if complex_:
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return _special_values(shape, seed)


SWAP_SHAPES = [
    # rank-3 signals and rank-4 spectrograms; the channel count goes where the format puts it
    ((3, 1000), False), ((3, 1001), False), ((5, 7), False), ((3, 40, 128), False), ((2, 37, 201), False), ((2, 3, 5), False),
    ((2, 37, 201), True), ((3, 6, 7), True), ((3, 1000), True),
]


@pytest.mark.parametrize('rest,complex_', SWAP_SHAPES)
@pytest.mark.parametrize('fmt', [CL, CF])
@pytest.mark.parametrize('n_ch', [1, 2, 3, 4, 6])
def test_channel_swap_is_take_along_the_channel_axis(rest, complex_, fmt, n_ch):
    shape = (rest[0],) + ((rest[1:] + (n_ch,)) if fmt == CL else ((n_ch,) + rest[1:]))
    axis = len(shape) - 1 if fmt == CL else 1
    x_np = _swap_input(shape, complex_, seed=n_ch)
    x = torch.from_numpy(x_np).to(_dev())
    keep = x.clone()
    layer = ChannelSwap(data_format=fmt)
    seed = 1000 + n_ch
    np.random.seed(seed)
    perm = np.random.permutation(n_ch) if n_ch > 1 else np.arange(1)
    np.random.seed(seed)
    y = layer(x, training=True)
    if n_ch == 1:
        assert y is x
        return
    assert layer.last_permutation == perm.tolist()
    assert y is not x and y.dtype == x.dtype and y.shape == x.shape
    word = np.uint64 if complex_ else np.uint32
    assert np.array_equal(np.ascontiguousarray(y.cpu().numpy()).view(word), np.take(x_np, perm, axis=axis).view(word))
    assert torch.equal(torch.view_as_real(x) if complex_ else x.view(torch.int32),
                       torch.view_as_real(keep) if complex_ else keep.view(torch.int32))
    back = _ffi.channel_gather(y, axis, np.argsort(perm).tolist())
    assert np.array_equal(np.ascontiguousarray(back.cpu().numpy()).view(word), x_np.view(word))
    assert layer(x, training=False) is x and layer(x) is x


def test_channel_swap_draws_from_numpys_global_generator():
    x = torch.arange(2 * 6 * 50, dtype=torch.float32, device=_dev()).reshape(2, 6, 50)
    layer = ChannelSwap(data_format=CF)
    np.random.seed(7)
    seen = set()
    for _ in range(20):
        layer(x, training=True)
        seen.add(tuple(layer.last_permutation))
    assert len(seen) > 10
    np.random.seed(7)
    layer(x, training=True)
    np.random.seed(7)
    assert layer.last_permutation == np.random.permutation(6).tolist()


def test_channel_gather_limits():
    x = torch.zeros(2, 65, 64, device=_dev())
    with pytest.raises(RuntimeError, match='at most 64'):
        ChannelSwap(data_format=CF)(x, training=True)
    x64 = torch.randn(2, 64, 100, device=_dev())
    np.random.seed(3)
    perm = np.random.permutation(64)
    np.random.seed(3)
    y = ChannelSwap(data_format=CF)(x64, training=True)
    assert torch.equal(y, x64[:, torch.from_numpy(perm).to(_dev())])
    with pytest.raises(RuntimeError, match='outside'):
        _ffi.channel_gather(x64, 1, [64] * 64)


@pytest.mark.parametrize('fmt,complex_', [(CL, False), (CF, False), (CF, True)])
def test_channel_swap_backward(fmt, complex_):
    g = torch.Generator().manual_seed(51)
    shape = (3, 20, 33, 4) if fmt == CL else (3, 4, 20, 33)
    x0 = torch.randn(shape + ((2,) if complex_ else ()), generator=g, dtype=torch.float64)
    x0 = torch.view_as_complex(x0) if complex_ else x0
    layer = ChannelSwap(data_format=fmt)
    xg = x0.to(torch.complex64 if complex_ else torch.float32).to(_dev()).requires_grad_(True)
    np.random.seed(52)
    y = layer(xg, training=True)
    assert y.grad_fn is not None
    r = cotangent(y.shape, complex_, seed=53)
    loss_of(y, r).backward()
    xr = x0.clone().requires_grad_(True)
    yr = xr.index_select(3 if fmt == CL else 1, torch.tensor(layer.last_permutation))
    loss_of(yr, r).backward()
    check(xg.grad, xr.grad, 2e-4, 'dL/dx through ChannelSwap')


def test_channel_swap_backward_behind_the_fused_mel_chain():
    n_fft, hop, n_mels, t = 512, 128, 40, 6 * 512
    mel = get_melspectrogram_layer(input_shape=(t, 2), n_fft=n_fft, hop_length=hop, sample_rate=22050, n_mels=n_mels,
                                   return_decibel=True, db_dynamic_range=60.0, input_data_format=CL, output_data_format=CL,
                                   pad_end=True)
    swap = ChannelSwap(data_format=CL)
    model = Sequential([mel, swap])
    x0 = wave(3, 2, t, CL, seed=61)
    xg = x0.to(_dev()).requires_grad_(True)
    for seed in range(100):                                       # a seed whose permutation of two channels is the swap
        np.random.seed(seed)
        if np.random.permutation(2).tolist() == [1, 0]:
            break
    np.random.seed(seed)
    y = model(xg, training=True)
    assert swap.last_permutation == [1, 0] and y.grad_fn is not None
    r = cotangent(y.shape, False, seed=62)
    loss_of(y, r).backward()
    xr = x0.to(torch.float64).requires_grad_(True)
    window = backend.get_window_fn(None)(n_fft).astype(np.float64)
    fb = torch.as_tensor(np.asarray(mel.layers[2].filterbank, np.float64))
    m = (ref_stft(to_bct(xr, CL), n_fft, n_fft, hop, window, False, True).abs() @ fb).permute(0, 2, 3, 1)
    yr = ref_db(m, 1.0, 1e-5, 60.0).flip(-1)
    loss_of(yr, r).backward()
    check(xg.grad, xr.grad, 3e-4, 'dL/dx through the fused mel chain and ChannelSwap')
    # inference: the model without the layer, same launches
    plain = Sequential([mel])(x0.to(_dev()))
    launches = _ffi.last_launches()
    assert torch.equal(model(x0.to(_dev()), training=False), plain) and _ffi.last_launches() == launches
