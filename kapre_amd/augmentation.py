"""Augmentation layers -- the training-only layers of the reference's ``kapre/augmentation.py``: ``SpecAugment``
(:115-326) and ``ChannelSwap`` (:17-112).  Constructor signatures, defaults, ``get_config`` keys and raised exception
types are the reference's; with ``training`` in ``(None, False)`` both return their input OBJECT and launch nothing.

``SpecAugment`` draws its masks on the device (``kpr_spec_augment_draw``: Philox4x32-10 over a 16-byte device state
``(seed, calls)``), so a training step copies nothing from the host and a captured graph draws new masks at every
replay.  The stream is this package's own: TensorFlow's generator is not reproduced (and could not be).  ``set_seed``
makes runs repeatable; the layer's config carries no seed, as upstream.

``Reverb`` has no counterpart in the reference: room-impulse-response augmentation of the waveform, one impulse response per
batch item drawn from the same device generator (``kpr_index_draw``), applied by ``backend.fftconvolve``'s three launches.

``AddNoise`` has none either: additive noise at a random signal-to-noise ratio (MUSAN-style), the noise, its starting point and
the ratio of every batch item drawn from that generator (``kpr_noise_draw``), mixed by ``kpr_add_noise_f32``.
"""
from __future__ import annotations

import os

import numpy as np

from . import _ffi, autograd, backend
from .backend import _CH_FIRST_STR, _CH_LAST_STR
from .keras_shim import Layer, register_keras_serializable

__all__ = ['SpecAugment', 'ChannelSwap', 'Reverb', 'AddNoise', 'set_seed']

_seed = None          # what set_seed gave; None: OS entropy at the first use of a device
_states = {}          # device index -> int64[2] on that device: (seed, calls) as kpr_spec_augment_draw reads them


def _as_int64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def set_seed(seed: int) -> None:
    """Seed SpecAugment's device generator: every device's state becomes ``(seed, calls = 0)`` -- the states that exist are
    rewritten where they are (a captured graph keeps drawing from the address it recorded), the others start there."""
    global _seed
    import torch

    _seed = int(seed)
    for state in _states.values():
        state.copy_(torch.tensor([_as_int64(_seed), 0], dtype=torch.int64))


def device_state(device):
    """The generator state of ``device`` (created on first use; not inside a graph capture: it is a host-to-device copy)."""
    import torch

    state = _states.get(device.index)
    if state is None:
        seed = _seed if _seed is not None else int.from_bytes(os.urandom(8), 'little')
        state = _states[device.index] = torch.tensor([_as_int64(seed), 0], dtype=torch.int64).to(device)
    return state


def _resolve_format(data_format):
    backend.validate_data_format_str(data_format)
    if isinstance(data_format, dict):           # (the reference's workaround for a Keras deserialisation bug)
        data_format = data_format['config']
    return backend.resolve_data_format(data_format)


def _config_format(data_format):
    return data_format if data_format in (_CH_FIRST_STR, _CH_LAST_STR) else 'default'


@register_keras_serializable(package='Kapre')
class ChannelSwap(Layer):
    """Randomly permute the channels of a batch of signals (rank 3) or spectrograms (rank 4); reference :17-112.

    ONE permutation per call, drawn with ``np.random.permutation`` as upstream, so ``np.random.seed`` governs it.  It travels
    in the kernel's arguments: a captured graph replays the permutation it was captured with (a traced TensorFlow function
    does the same).  float32 and complex64 data, at most 64 channels.  ``last_permutation`` is that of the last training call.
    """

    def __init__(self, data_format='default', **kwargs):
        super(ChannelSwap, self).__init__(**kwargs)
        self.data_format = _resolve_format(data_format)
        self.last_permutation = None

    def call(self, x, training=None):
        if training in (None, False):
            return x
        ndim = len(x.shape)
        if ndim not in (3, 4):
            raise ValueError(
                'ndim of input tensor x should be 3 (batch signal) or 4 (batch spectrogram),'
                'but it is %d' % ndim
            )
        ch_axis = ndim - 1 if self.data_format == _CH_LAST_STR else 1
        n_ch = int(x.shape[ch_axis])
        if n_ch == 1:
            return x
        perm = np.random.permutation(n_ch).tolist()
        self.last_permutation = perm
        if autograd.needs_grad(x):
            dtype = 'complex64' if x.is_complex() else 'float32'
            return autograd.channel_gather(autograd.prep(x, dtype), ch_axis, perm)
        return self._forward(x, ch_axis, perm)

    @staticmethod
    def _forward(x, ch_axis, perm):
        import torch

        complex_in = np.iscomplexobj(x) if isinstance(x, np.ndarray) else (isinstance(x, torch.Tensor) and x.is_complex())
        return _ffi.channel_gather(_ffi.as_device(x, torch.complex64 if complex_in else torch.float32), ch_axis, perm)

    def get_config(self):
        config = super(ChannelSwap, self).get_config()
        config.update({'data_format': _config_format(self.data_format)})
        return config


@register_keras_serializable(package='Kapre')
class SpecAugment(Layer):
    """SpecAugment (Park et al. 2019, https://arxiv.org/abs/1904.08779) of a one-channel spectrogram batch; reference :115-326.

    Args are the reference's: ``freq_mask_param`` (F of the paper), ``time_mask_param`` (T), ``n_freq_masks=1`` (mF),
    ``n_time_masks=1`` (mT), ``mask_value=0.0``, ``data_format='default'``.  Every batch item gets its own masks; a mask
    covers ``width + 1`` frames / bins, ``width`` uniform in ``0 .. param - 1`` (the reference's ``<=``, :211-214).
    At most 32 masks per axis.  After a training call ``last_mask_table`` is the device table of that call: int32
    ``(batch, n_time_masks + n_freq_masks, 2)`` of inclusive ``(first, last)``, time masks first.
    """

    def __init__(
        self,
        freq_mask_param,
        time_mask_param,
        n_freq_masks=1,
        n_time_masks=1,
        mask_value=0.0,
        data_format='default',
        **kwargs,
    ):
        super(SpecAugment, self).__init__(**kwargs)
        data_format = _resolve_format(data_format)
        self.freq_mask_param = freq_mask_param
        self.time_mask_param = time_mask_param
        self.n_freq_masks = n_freq_masks
        self.n_time_masks = n_time_masks
        self.mask_value = mask_value
        if not self.freq_mask_param or not self.time_mask_param:
            raise RuntimeError(
                "Both freq_mask_param and time_mask_param must be defined and different "
                "than zero"
            )
        self.data_format = data_format
        self.last_mask_table = None

    def _mask_counts(self):
        """(time masks, frequency masks): the reference applies an axis' masks when its count is >= 1"""
        return max(int(self.n_time_masks), 0), max(int(self.n_freq_masks), 0)

    def _check(self, shape):
        """The reference's checks, in its order (:296-306, :245); returns (n_time, n_freq)."""
        if len(shape) != 4:
            raise ValueError(
                'ndim of input tensor x should be 4 (batch spectrogram),' 'but it is %d' % len(shape)
            )
        ch_axis = 1 if self.data_format == 'channels_first' else 3
        if shape[ch_axis] != 1:
            raise RuntimeError(
                'SpecAugment does not support spectrograms with depth greater than 1'
            )
        n_time, n_freq = (shape[1], shape[2]) if ch_axis == 3 else (shape[2], shape[3])
        n_tm, n_fm = self._mask_counts()
        if (n_tm and n_time < self.time_mask_param) or (n_fm and n_freq < self.freq_mask_param):
            raise ValueError(
                "Time and freq axis shapes must be greater than time_mask_param "
                "and freq_mask_param respectively"
            )
        return int(n_time), int(n_freq)

    def call(self, x, training=None, **kwargs):
        if training in (None, False):
            return x
        if autograd.needs_grad(x):
            return autograd.spec_augment(self, autograd.prep(x, 'float32'))       # (its forward is _forward)
        return self._forward(x)

    def _forward(self, x, inplace=False):
        """The training pass: the reference's checks, a fresh table, then the masks.  ``inplace`` (fuse_and_run, on a tensor
        nobody else holds) masks ``x`` itself; otherwise ``x`` is left as it is."""
        import torch

        n_time, n_freq = self._check(tuple(x.shape))
        x = _ffi.as_device(x, torch.float32)
        n_tm, n_fm = self._mask_counts()
        table = _ffi.spec_augment_draw(device_state(x.device), x.shape[0], n_tm, n_fm, n_time, n_freq,
                                       self.time_mask_param, self.freq_mask_param)
        self.last_mask_table = table
        return self._apply(x, table, self.mask_value, inplace)

    def _apply(self, x, table, mask_value, inplace=False):
        n_tm, n_fm = self._mask_counts()
        n_time, n_freq = (x.shape[1], x.shape[2]) if self.data_format == _CH_LAST_STR else (x.shape[2], x.shape[3])
        return _ffi.spec_augment_apply(x, table, n_tm, n_fm, n_time, n_freq, mask_value, inplace=inplace)

    def get_config(self):
        config = super(SpecAugment, self).get_config()
        config.update(
            {
                'freq_mask_param': self.freq_mask_param,
                'time_mask_param': self.time_mask_param,
                'n_freq_masks': self.n_freq_masks,
                'n_time_masks': self.n_time_masks,
                'mask_value': self.mask_value,
                'data_format': _config_format(self.data_format),
            }
        )
        return config


@register_keras_serializable(package='Kapre')
class Reverb(Layer):
    """Room-impulse-response augmentation of a waveform batch: in training every batch item is convolved with one of the
    impulse responses ``irs`` (array-like (n_ir, len) or (len,)), drawn on the device by ``kpr_index_draw`` from the generator
    that ``SpecAugment`` uses (``set_seed`` makes a run repeatable bit for bit; a captured graph draws anew at every replay).
    The output has the input's shape: the first ``time`` samples of the full convolution, causally aligned (sample t depends on
    the input up to t).  ``normalize`` scales every impulse response to unit energy, once, on the host.  The channels of an
    item share its impulse response.  With ``training`` in ``(None, False)`` the layer returns its input OBJECT and launches
    nothing.  float32; differentiable with respect to the waveform.  ``last_index`` is the device int32 vector drawn by the
    last training call."""

    def __init__(self, irs, normalize=True, input_data_format='default', **kwargs):
        super(Reverb, self).__init__(**kwargs)
        self.input_data_format = _resolve_format(input_data_format)
        h = backend.convolve_irs(irs)
        self.irs = h.tolist()
        self.normalize = bool(normalize)
        if self.normalize:
            energy = np.sqrt(np.sum(h * h, axis=1, keepdims=True))
            if np.any(energy == 0.0):
                raise ValueError('Reverb: an impulse response of zero energy cannot be normalised')
            h = h / energy
        self._plan = backend.ConvolvePlan(h)
        self.last_index = None

    def compute_output_shape(self, input_shape):
        """the input's shape"""
        return tuple(input_shape)

    def call(self, x, training=None):
        if training in (None, False):
            return x
        x, _ = autograd.intake(x, 3, 'float32', 'Reverb expects a rank-3 waveform batch, got shape %s', TypeError,
                               'Reverb has float32 kernels only; got a float64 input (cast it to float32)')
        t = _ffi.dims_of(x.shape, self.input_data_format)[2]
        self.last_index = _ffi.index_draw(device_state(x.device), x.shape[0], self._plan.n_ir)
        return backend._convolve_run(x, self._plan, self.input_data_format, 'full', index=self.last_index, out_len=t)

    def get_config(self):
        config = super(Reverb, self).get_config()
        config.update({'irs': self.irs, 'normalize': self.normalize,
                       'input_data_format': _config_format(self.input_data_format)})
        return config


@register_keras_serializable(package='Kapre')
class AddNoise(Layer):
    """Additive-noise augmentation of a waveform batch: in training every batch item gets one of the mono ``noises`` (what
    ``backend.noise_bank`` takes: (L,), (n, L) or a list of 1-D arrays of different lengths), read circularly from a random
    offset and scaled so that the ratio of the item's mean power to the mean power of the added noise is a signal-to-noise ratio
    drawn uniformly from ``snr_db = (low, high)`` in dB; a scalar ``snr_db`` fixes it.  The channels of an item share its noise
    and its gain; a silent item, or a silent stretch of noise, leaves the item as it is.  Everything is drawn on the device by
    ``kpr_noise_draw`` from the generator that ``SpecAugment`` and ``Reverb`` use (``set_seed`` makes a run repeatable bit for
    bit; a captured graph draws anew at every replay, nothing is copied from the host per call).  With ``training`` in
    ``(None, False)`` the layer returns its input OBJECT and launches nothing.  float32; differentiable with respect to the
    waveform (exactly: the gain depends on it).  After a training call ``last_draw`` is the device int32 (batch, 4) table of
    (index, offset, snr as float32 bits, 0) and ``last_stats`` the device float64 (batch, 4) rows (signal energy, noise
    energy, gain, 0)."""

    def __init__(self, noises, snr_db=(5.0, 20.0), input_data_format='default', **kwargs):
        super(AddNoise, self).__init__(**kwargs)
        self.input_data_format = _resolve_format(input_data_format)
        self._plan = backend.NoisePlan(noises)
        self.noises = [self._plan.bank[k, :n].astype(np.float64).tolist() for k, n in enumerate(self._plan.lengths)]
        if np.ndim(snr_db) == 0:
            lo = hi = float(snr_db)
            self.snr_db = lo
        else:
            if len(snr_db) != 2:
                raise ValueError('AddNoise: snr_db must be a number or (low, high), got %r' % (snr_db,))
            lo, hi = float(snr_db[0]), float(snr_db[1])
            self.snr_db = [lo, hi]
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError('AddNoise: snr_db must be finite with low <= high, got %r' % (snr_db,))
        self._snr = (lo, hi)
        self.last_draw = None
        self.last_stats = None

    def compute_output_shape(self, input_shape):
        """the input's shape"""
        return tuple(input_shape)

    def call(self, x, training=None):
        if training in (None, False):
            return x
        x, _ = autograd.intake(x, 3, 'float32', 'AddNoise expects a rank-3 waveform batch, got shape %s', TypeError,
                               'AddNoise has float32 kernels only; got a float64 input (cast it to float32)')
        _, lengths = self._plan.device(x.device)
        self.last_draw = _ffi.noise_draw(device_state(x.device), x.shape[0], lengths, *self._snr)
        y, self.last_stats = backend._add_noise_run(x, self._plan, self.last_draw, self.input_data_format)
        return y

    def get_config(self):
        config = super(AddNoise, self).get_config()
        config.update({'noises': self.noises, 'snr_db': self.snr_db,
                       'input_data_format': _config_format(self.input_data_format)})
        return config
