"""CPU tests of the augmentation layers (kapre_amd/augmentation.py): the checker itself (tests/augment_model.py: Philox4x32-10
against the published known-answer vectors, the draw rule's range and distribution), API parity with the reference's
kapre/augmentation.py (config keys, exception types, the `training` switch), persistence, and the `training` plumbing of
keras_shim.  Nothing here touches a GPU: with `training` in (None, False) the layers return their input object."""
import os

import numpy as np
import pytest

import augment_model as am

import kapre_amd as kapre
from kapre_amd import SpecAugment, ChannelSwap, Sequential, Input, augmentation, keras_shim

BASE_KEYS = {'name', 'trainable', 'dtype'}
# the reference's get_config lists (kapre/augmentation.py:312-326, :103-112)
SPEC_AUGMENT_KEYS = {'freq_mask_param', 'time_mask_param', 'n_freq_masks', 'n_time_masks', 'mask_value', 'data_format'}
CHANNEL_SWAP_KEYS = {'data_format'}


# ------------------------------------------------------------------ the checker
@pytest.mark.parametrize('counter,key,want', [
    # Random123 known-answer vectors of philox4x32-10 (kat_vectors)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = tuple(int(v) for v in am.philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_draw_rule_range_and_distribution():
    """100 000 (item, mask) pairs, param 10 on an axis of 83: every interval inside the axis, 1 .. 10 elements wide, every width
    with a frequency within 10 % of 1/10 (one standard deviation of a bin is about 1 %)."""
    table = am.draw_table(seed=0x1234567887654321, calls=5, n_items=50000, n_time_masks=2, n_freq_masks=0, n_time=83, n_freq=128,
                          time_mask_param=10, freq_mask_param=5)
    assert table.shape == (50000, 2, 2)
    first, last = table[..., 0].ravel().astype(np.int64), table[..., 1].ravel().astype(np.int64)
    assert (first >= 0).all() and (first <= last).all() and (last <= 82).all()
    width = last - first
    assert (width < 10).all()
    freq = np.bincount(width, minlength=10) / width.size
    assert freq.shape == (10,)
    assert (np.abs(freq - 0.1) <= 0.01).all(), freq
    # the start is spread over what the width leaves: both ends of the axis are reached
    assert first.min() == 0 and last.max() == 82
    # counter based: another call count, another table; the same (seed, calls), the same table
    again = am.draw_table(0x1234567887654321, 5, 50000, 2, 0, 83, 128, 10, 5)
    other = am.draw_table(0x1234567887654321, 6, 50000, 2, 0, 83, 128, 10, 5)
    assert np.array_equal(table, again) and not np.array_equal(table, other)


def test_mask_model_is_inclusive():
    table = np.array([[[2, 4], [0, 0], [1, 1], [5, 6]]], np.int32)          # two time masks, two frequency masks
    mask = am.mask_from_table(table, 2, 6, 8)[0]
    assert mask[:, [1, 5, 6]].all() and mask[[0, 2, 3, 4]].all()
    assert not mask[np.ix_([1, 5], [0, 2, 3, 4, 7])].any()


# ------------------------------------------------------------------ API parity
def test_exports():
    assert kapre.SpecAugment is augmentation.SpecAugment and kapre.ChannelSwap is augmentation.ChannelSwap
    assert {'SpecAugment', 'ChannelSwap'} <= set(kapre.__all__)
    assert callable(kapre.augmentation.set_seed)


@pytest.mark.parametrize('data_format', ['default', 'channels_first', 'channels_last'])
def test_config_keys_and_round_trip(data_format):
    sa = SpecAugment(freq_mask_param=5, time_mask_param=10, n_freq_masks=4, n_time_masks=3, mask_value=-80.0,
                     data_format=data_format, name='sa')
    cfg = sa.get_config()
    assert set(cfg) == BASE_KEYS | SPEC_AUGMENT_KEYS
    resolved = 'channels_last' if data_format == 'default' else data_format      # the reference stores the resolved format
    assert cfg == {'name': 'sa', 'trainable': True, 'dtype': 'float32', 'freq_mask_param': 5, 'time_mask_param': 10,
                   'n_freq_masks': 4, 'n_time_masks': 3, 'mask_value': -80.0, 'data_format': resolved}
    assert SpecAugment.from_config(cfg).get_config() == cfg
    cs = ChannelSwap(data_format=data_format, name='cs')
    cfg = cs.get_config()
    assert set(cfg) == BASE_KEYS | CHANNEL_SWAP_KEYS and cfg['data_format'] == resolved
    assert ChannelSwap.from_config(cfg).get_config() == cfg


def test_defaults_are_the_references():
    sa = SpecAugment(5, 10)
    assert (sa.freq_mask_param, sa.time_mask_param, sa.n_freq_masks, sa.n_time_masks, sa.mask_value) == (5, 10, 1, 1, 0.0)
    assert sa.data_format == ChannelSwap().data_format == 'channels_last'
    with pytest.raises(TypeError):
        SpecAugment(5, 10, seed=1)                      # no seed argument: the config stays the reference's


@pytest.mark.parametrize('kw', [dict(freq_mask_param=0, time_mask_param=10), dict(freq_mask_param=5, time_mask_param=0),
                                dict(freq_mask_param=None, time_mask_param=10), dict(freq_mask_param=5, time_mask_param=None)])
def test_constructor_runtime_error(kw):
    with pytest.raises(RuntimeError):
        SpecAugment(**kw)
    with pytest.raises(ValueError):
        SpecAugment(5, 10, data_format='weird')
    with pytest.raises(ValueError):
        ChannelSwap(data_format='weird')


def test_call_errors_come_before_any_gpu_work():
    sa = SpecAugment(freq_mask_param=5, time_mask_param=10, n_freq_masks=4, n_time_masks=3)
    with pytest.raises(ValueError, match='ndim'):
        sa(np.zeros((2, 83, 128), np.float32), training=True)
    with pytest.raises(RuntimeError, match='depth'):
        sa(np.zeros((2, 83, 128, 4), np.float32), training=True)
    with pytest.raises(ValueError, match='time_mask_param'):
        sa(np.zeros((2, 9, 128, 1), np.float32), training=True)            # 9 frames < time_mask_param
    with pytest.raises(ValueError, match='freq_mask_param'):
        sa(np.zeros((2, 83, 4, 1), np.float32), training=True)             # 4 bins < freq_mask_param
    with pytest.raises(ValueError, match='freq_mask_param'):
        SpecAugment(5, 10, data_format='channels_first')(np.zeros((2, 1, 83, 4), np.float32), training=True)
    # an axis without masks is not checked (the reference only visits an axis whose mask count is >= 1)
    assert SpecAugment(5, 10, n_time_masks=0)._check((2, 9, 128, 1)) == (9, 128)
    assert SpecAugment(5, 10, n_freq_masks=0)._check((2, 83, 4, 1)) == (83, 4)
    with pytest.raises(ValueError, match='freq_mask_param'):
        SpecAugment(5, 10, n_time_masks=0)._check((2, 9, 4, 1))
    with pytest.raises(ValueError, match='ndim'):
        ChannelSwap()(np.zeros((4, 2), np.float32), training=True)
    with pytest.raises(ValueError, match='ndim'):
        ChannelSwap()(np.zeros((1, 2, 3, 4, 5), np.float32), training=True)


@pytest.mark.parametrize('training', [None, False])
def test_inference_returns_the_input_object(training):
    import torch
    for x in (np.zeros((2, 83, 128, 1), np.float32), torch.zeros(2, 83, 128, 1), np.zeros((2, 83, 128, 4), np.float64)):
        assert SpecAugment(5, 10)(x, training=training) is x
        assert ChannelSwap()(x, training=training) is x
    x = np.zeros((3, 5), np.float32)                    # not even the rank is looked at
    assert SpecAugment(5, 10)(x) is x and ChannelSwap()(x) is x
    # one channel: nothing to swap, in training too
    x = np.zeros((2, 100, 1), np.float32)
    assert ChannelSwap()(x, training=True) is x
    x = np.zeros((2, 1, 83, 128), np.float32)
    assert ChannelSwap(data_format='channels_first')(x, training=True) is x


# ------------------------------------------------------------------ keras_shim: training reaches the layers that take it
def test_sequential_forwards_training():
    x = np.zeros((2, 83, 128, 4), np.float32)
    model = Sequential([Input(shape=(83, 128, 4)), keras_shim.Layer(), SpecAugment(5, 10), ChannelSwap()])
    assert model(x) is x and model(x, training=False) is x and model(x, training=None) is x
    with pytest.raises(RuntimeError, match='depth'):                   # training=True reached SpecAugment.call
        model(x, training=True)
    nested = Sequential([Sequential([SpecAugment(5, 10)])])
    with pytest.raises(RuntimeError, match='depth'):
        nested(x, training=True)
    assert nested(x, training=False) is x

    class Plain(keras_shim.Layer):                                      # a layer without the parameter is called as before
        def call(self, x):
            return x

    class Takes(keras_shim.Layer):
        def call(self, x, training=None):
            self.seen = training
            return x

    t = Takes()
    assert Sequential([Plain(), t])(x, training=True) is x and t.seen is True
    assert t(x) is x and t.seen is None
    assert Plain()(x, training=True) is x
    assert model.predict(x) is not None


def test_set_seed_records_the_seed():
    """The device states are created lazily (first training call on a device): without one set_seed only records the seed."""
    try:
        augmentation.set_seed(2 ** 64 - 1)
        assert augmentation._seed == 2 ** 64 - 1
        assert augmentation._as_int64(2 ** 64 - 1) == -1 and augmentation._as_int64(5) == 5
        assert augmentation._as_int64(2 ** 63) == -2 ** 63
    finally:
        augmentation._seed = None


# ------------------------------------------------------------------ persistence (the reference's tests/test_augmentation.py:142-179)
@pytest.mark.parametrize('data_format', ['default', 'channels_first', 'channels_last'])
@pytest.mark.parametrize('ext', ['.keras', '.h5'])
def test_save_load(tmp_path, data_format, ext):
    shape = (1, 83, 128) if data_format == 'channels_first' else (83, 128, 1)
    layers = {
        'SpecAugment': SpecAugment(freq_mask_param=5, time_mask_param=10, n_freq_masks=4, n_time_masks=3, mask_value=0.0,
                                   data_format=data_format),
        'ChannelSwap': ChannelSwap(data_format=data_format),
    }
    x = np.random.default_rng(0).standard_normal((2,) + shape).astype(np.float32)
    for name, layer in layers.items():
        model = Sequential([Input(shape=shape), layer])
        path = os.path.join(str(tmp_path), name + ext)
        model.save(path)
        for custom in (None, {name: type(layer)}):
            loaded = keras_shim.load_model(path, custom_objects=custom)
            assert type(loaded.layers[0]) is type(layer)
            assert loaded.layers[0].get_config() == layer.get_config()
            assert loaded.input_shape == model.input_shape == (None,) + shape
            assert loaded.output_shape == (None,) + shape
            np.testing.assert_allclose(loaded(x, training=None), model(x, training=None))
            assert loaded(x, training=None) is x
