"""Time-frequency layers -- MI355X implementation behind Kapre's own layer API.

Mirror of /root/reference/kapre/time_frequency.py for the hot path: ``STFT`` (:61-203),
``InverseSTFT`` (:207-333), ``Magnitude`` (:337-359), ``Phase`` (:363-411),
``MagnitudeToDecibel`` (:415-465), ``ApplyFilterbank`` (:469-559), ``Delta`` (:561-644),
``ConcatenateFrequencyMap`` (:647-744); ``PCEN``, ``CMVN``, ``GriffinLim``, ``TimeStretch`` and ``HPSS`` are this package's own.  Constructor signatures,
defaults, ``get_config`` keys and raised exception types are the reference's; ``call`` runs the
hand-written gfx950 kernels of libkapre_hip.so through ``kapre_amd._ffi`` (ctypes).  Inputs may be
numpy arrays or torch tensors; outputs are torch tensors on the GPU (complex64 / float32).

``fuse_and_run`` is the peephole optimiser used by ``Sequential``: the chains
``STFT -> Magnitude -> ApplyFilterbank [-> MagnitudeToDecibel]``, ``STFT -> Magnitude
[-> MagnitudeToDecibel]`` and ``STFT -> Phase`` each become one kernel launch (plus the clamp
pass when decibel scaling is on).
"""
from __future__ import annotations

import ctypes
import weakref

import numpy as np

from . import _ffi, autograd, backend
from .augmentation import SpecAugment
from .backend import _CH_FIRST_STR, _CH_LAST_STR
from .keras_shim import Layer, register_keras_serializable

__all__ = [
    'STFT',
    'InverseSTFT',
    'Magnitude',
    'Phase',
    'MagnitudeToDecibel',
    'ApplyFilterbank',
    'Delta',
    'ConcatenateFrequencyMap',
    'PCEN',
    'CMVN',
    'GriffinLim',
    'TimeStretch',
    'HPSS',
]


def _forget_packed(ptr):
    try:
        _ffi.filterbank_forget(ptr)
    except Exception:        # interpreter shutdown: the library may be gone already
        pass


class _WorkspacePool:
    """Scratch buffers of the cached (plan-based) calls: one per (device, stream), grown
    geometrically and NEVER freed -- a captured hipGraph keeps replaying the pointer it recorded, so
    a buffer that was ever handed out stays alive (outgrown ones are parked in ``_retired``; total
    memory stays below twice the largest request).  Calls on one stream are ordered, so sharing the
    buffer between plans of that stream is safe."""

    def __init__(self):
        self._live = {}
        self._retired = []

    def get(self, nbytes: int, device, stream_ptr: int):
        key = (str(device), int(stream_ptr))
        buf = self._live.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None:
                self._retired.append(buf)
            grow = 0 if buf is None else 2 * buf.numel()
            buf = self._live[key] = _ffi.workspace(max(int(nbytes), grow, 4096), device)
        return buf


_PLAN_WORKSPACES = _WorkspacePool()


@register_keras_serializable(package='Kapre')
class STFT(Layer):
    """Short-time Fourier transform layer (reference: time_frequency.py:61-203).

    ``output_data_format == 'channels_last'`` -> (batch, time, freq, channel);
    ``'channels_first'`` -> (batch, channel, time, freq); dtype complex64.

    Args are the reference's: ``n_fft=2048, win_length=None (-> n_fft), hop_length=None
    (-> win_length // 4), window_name=None (-> hann), pad_begin=False, pad_end=False,
    input_data_format='default', output_data_format='default', **kwargs``.
    ``pad_begin`` pads ``n_fft - hop_length`` zeros on the left (code at :169-172).
    """

    def __init__(
        self,
        n_fft=2048,
        win_length=None,
        hop_length=None,
        window_name=None,
        pad_begin=False,
        pad_end=False,
        input_data_format='default',
        output_data_format='default',
        **kwargs,
    ):
        super(STFT, self).__init__(**kwargs)

        for data_format in (input_data_format, output_data_format):
            backend.validate_data_format_str(data_format)   # reference order: validate first (:115-116)
        if isinstance(input_data_format, dict):
            input_data_format = input_data_format['config']
        if isinstance(output_data_format, dict):
            output_data_format = output_data_format['config']

        if win_length is None:
            win_length = n_fft
        if hop_length is None:
            hop_length = win_length // 4

        self.n_fft = n_fft
        self.win_length = win_length
        self.hop_length = hop_length
        self.window_name = window_name
        self.window_fn = backend.get_window_fn(window_name)   # NotImplementedError if unknown
        self.pad_begin = pad_begin
        self.pad_end = pad_end

        self.input_data_format_original = input_data_format
        self.output_data_format_original = output_data_format
        self.output_data_format = backend.resolve_data_format(output_data_format)
        self.input_data_format = backend.resolve_data_format(input_data_format)
        self._consts = _ffi.DeviceConstants()

    # -- helpers -----------------------------------------------------------------------------
    def _geom(self, x) -> _ffi.StftGeom:
        if x.dim() != 3:
            raise ValueError('STFT expects a rank-3 input (batch, time, ch) / (batch, ch, time), '
                             'got shape %s' % (tuple(x.shape),))
        b, c, t = _ffi.dims_of(x.shape, self.input_data_format)
        return _ffi.StftGeom(b, c, t, int(self.n_fft), int(self.win_length), int(self.hop_length),
                             int(bool(self.pad_begin)), int(bool(self.pad_end)),
                             _ffi.layout(self.input_data_format),
                             _ffi.layout(self.output_data_format))

    def _window(self, device, f64=False):
        # float32 uses window_fn's own values; float64 recomputes them in float64 (backend.window_values)
        if f64:
            return self._consts.get(('window64', int(self.win_length), id(self.window_fn)), device,
                                    lambda: backend.window_values(self.window_fn, int(self.win_length), np.float64))
        return self._consts.get(('window', int(self.win_length), id(self.window_fn)), device,
                                lambda: self.window_fn(int(self.win_length)))

    def _plan_version(self):
        """Everything of the layer a cached fused-call plan depends on (attributes are plain and
        may be reassigned by the caller, as with any Keras layer)."""
        return (int(self.n_fft), int(self.win_length), int(self.hop_length), bool(self.pad_begin),
                bool(self.pad_end), self.input_data_format, self.output_data_format,
                id(self.window_fn))

    def _run(self, x, mode: int):
        """float32 STFT, or float64 for a dtype='float64' layer (reference :155): complex or real output by ``mode``."""
        import torch

        x = _ffi.as_device(x, torch.float64 if self._f64 else torch.float32)
        g = self._geom(x)
        n_frames = _ffi.num_frames(g)
        return _ffi.stft(x, g, n_frames, self._window(x.device, self._f64), mode)

    def compute_output_shape(self, input_shape):
        """(b, t, ch) / (b, ch, t) -> (b, frame, n_fft // 2 + 1, ch) / (b, ch, frame, n_fft // 2 + 1); frames as tf.signal.stft counts
        them after the left padding of n_fft - hop_length (reference: time_frequency.py:164-185)"""
        b, c, t = _ffi.dims_of(input_shape, self.input_data_format)
        frames = None
        if t is not None:
            t = int(t) + (int(self.n_fft) - int(self.hop_length) if self.pad_begin else 0)
            frames = -(-t // int(self.hop_length)) if self.pad_end else max(0, 1 + (t - int(self.win_length)) // int(self.hop_length))
        return _ffi.shape_of(self.output_data_format, b, c, frames, int(self.n_fft) // 2 + 1)

    def call(self, x):
        """(batch, time, ch) or (batch, ch, time) float -> complex64 STFT (reference :146-187).
        Differentiable when ``x`` is a torch tensor that requires grad (kapre_amd/autograd.py)."""
        if autograd.needs_grad(x):
            return autograd.stft(self, autograd.prep(x, 'float64' if self._f64 else 'float32'))
        return self._run(x, _ffi.OUT_COMPLEX)

    def get_config(self):
        config = super(STFT, self).get_config()
        config.update(
            {
                'n_fft': self.n_fft,
                'win_length': self.win_length,
                'hop_length': self.hop_length,
                'window_name': self.window_name,
                'pad_begin': self.pad_begin,
                'pad_end': self.pad_end,
                'input_data_format': self.input_data_format_original,
                'output_data_format': self.output_data_format_original,
            }
        )
        return config


def _complex_f64(x, layer_f64: bool) -> bool:
    """Compute precision for a layer that consumes a complex tensor: the INPUT's.  Keras autocasting only touches
    floating-point tensors, so the reference's ``tf.abs`` / ``tf.math.angle`` / ``tf.signal.inverse_stft`` run in the
    precision of the complex input whatever the layer's own dtype is (complex128 -> float64 out, complex64 -> float32
    out).  Non-complex inputs follow the layer dtype."""
    name = str(getattr(x, 'dtype', '')).replace('torch.', '')
    if name == 'complex128':
        return True
    if name == 'complex64':
        return False
    return layer_f64


def _as_device_complex(x, layer_f64: bool):
    import torch

    return _ffi.as_device(x, torch.complex128 if _complex_f64(x, layer_f64) else torch.complex64)


@register_keras_serializable(package='Kapre')
class InverseSTFT(Layer):
    """Inverse STFT layer (reference: time_frequency.py:207-333).

    Input (batch, time, freq, ch) / (batch, ch, time, freq) complex64; output
    (batch, time, ch) / (batch, ch, time) float32 of length ``(n_frames-1)*hop + win_length``
    (the caller trims, as the reference notes at :213-214).
    """

    def __init__(
        self,
        n_fft=2048,
        win_length=None,
        hop_length=None,
        forward_window_name=None,
        input_data_format='default',
        output_data_format='default',
        **kwargs,
    ):
        super(InverseSTFT, self).__init__(**kwargs)

        for data_format in (input_data_format, output_data_format):
            backend.validate_data_format_str(data_format)
        if isinstance(input_data_format, dict):
            input_data_format = input_data_format['config']
        if isinstance(output_data_format, dict):
            output_data_format = output_data_format['config']

        if win_length is None:
            win_length = n_fft
        if hop_length is None:
            hop_length = win_length // 4

        self.n_fft = n_fft
        self.win_length = win_length
        self.hop_length = hop_length
        self.forward_window_name = forward_window_name
        self.window_fn = backend.inverse_stft_window_fn(
            frame_step=hop_length, forward_window_fn=backend.get_window_fn(forward_window_name)
        )

        self.input_data_format_original = input_data_format
        self.output_data_format_original = output_data_format
        self.output_data_format = backend.resolve_data_format(output_data_format)
        self.input_data_format = backend.resolve_data_format(input_data_format)
        self._consts = _ffi.DeviceConstants()

    def compute_output_shape(self, input_shape):
        """(b, frame, freq, ch) / (b, ch, frame, freq) -> (b, (frame - 1) hop + win, ch) / (b, ch, ...): untrimmed, as upstream"""
        b, c, f, _ = _ffi.dims_of(input_shape, self.input_data_format)
        t = None if f is None else ((int(f) - 1) * int(self.hop_length) + int(self.win_length) if int(f) > 0 else 0)
        return _ffi.shape_of(self.output_data_format, b, c, t)

    def call(self, x):
        if autograd.needs_grad(x):
            return autograd.istft(self, autograd.prep(x, 'complex128' if _complex_f64(x, self._f64) else 'complex64'))
        return self._forward(x)

    def _forward(self, x):
        import torch

        x = _as_device_complex(x, self._f64)
        if x.dim() != 4:
            raise ValueError('InverseSTFT expects a rank-4 input, got shape %s' % (tuple(x.shape),))
        k = _ffi.dims_of(x.shape, self.input_data_format)[3]
        k_need = int(self.n_fft) // 2 + 1
        if k != k_need:
            # tf.signal.irfft crops / zero-pads the frequency axis to n_fft//2+1
            axis = 2 if self.input_data_format == _CH_LAST_STR else 3
            if k > k_need:
                x = x.narrow(axis, 0, k_need).contiguous()
            else:
                pad = [0, 0] * (x.dim() - 1 - axis) + [0, k_need - k]
                x = torch.nn.functional.pad(torch.view_as_real(x), [0, 0] + pad)
                x = torch.view_as_complex(x.contiguous())
        # float32 uses window_fn's own values; float64 recomputes them in float64 (backend.window_values)
        if x.dtype == torch.complex128:
            win = self._consts.get('synth64', x.device,
                                   lambda: backend.window_values(self.window_fn, int(self.win_length), np.float64))
        else:
            win = self._consts.get('synth', x.device, lambda: self.window_fn(int(self.win_length)))
        return _ffi.istft(x, win, self.n_fft, self.win_length, self.hop_length, self.output_data_format,
                          self.input_data_format)

    def get_config(self):
        config = super(InverseSTFT, self).get_config()
        config.update(
            {
                'n_fft': self.n_fft,
                'win_length': self.win_length,
                'hop_length': self.hop_length,
                'forward_window_name': self.forward_window_name,
                'input_data_format': self.input_data_format_original,
                'output_data_format': self.output_data_format_original,
            }
        )
        return config


@register_keras_serializable(package='Kapre')
class Magnitude(Layer):
    """Magnitude of a complex input -> float32 (reference: time_frequency.py:337-359)."""

    def call(self, x):
        if autograd.needs_grad(x):
            return autograd.magnitude(self, autograd.prep(x, 'complex128' if _complex_f64(x, self._f64) else 'complex64'))
        return self._forward(x)

    def _forward(self, x):
        return _ffi.cplx_to_real(_as_device_complex(x, self._f64), phase=False)


@register_keras_serializable(package='Kapre')
class Phase(Layer):
    """Phase (radian) of a complex input (reference: time_frequency.py:363-411).

    ``approx_atan_accuracy`` is kept for config compatibility; the TFLite continued-fraction
    approximation it selects upstream is a TFLite deployment feature and is not reproduced:
    the accurate ``atan2`` is always used.
    """

    def __init__(self, approx_atan_accuracy=None, **kwargs):
        super(Phase, self).__init__(**kwargs)
        self.approx_atan_accuracy = approx_atan_accuracy

    def call(self, x):
        if autograd.needs_grad(x):
            return autograd.phase(self, autograd.prep(x, 'complex128' if _complex_f64(x, self._f64) else 'complex64'))
        return self._forward(x)

    def _forward(self, x):
        return _ffi.cplx_to_real(_as_device_complex(x, self._f64), phase=True)

    def get_config(self):
        config = super(Phase, self).get_config()
        config.update({'approx_atan_accuracy': self.approx_atan_accuracy})
        return config


@register_keras_serializable(package='Kapre')
class MagnitudeToDecibel(Layer):
    """Decibel scaling layer wrapping ``backend.magnitude_to_decibel``
    (reference: time_frequency.py:415-465)."""

    def __init__(self, ref_value=1.0, amin=1e-5, dynamic_range=80.0, **kwargs):
        super(MagnitudeToDecibel, self).__init__(**kwargs)
        self.ref_value = ref_value
        self.amin = amin
        self.dynamic_range = dynamic_range

    def call(self, x):
        if autograd.needs_grad(x):
            self._db_params()          # parameter validation before anything is recorded
            return autograd.decibel(self, autograd.prep(x, 'float64' if self._f64 else 'float32'))
        return self._forward(x)

    def _forward(self, x):
        import torch

        # Keras autocast: the layer dtype decides the compute dtype, then the backend follows its input
        x = _ffi.as_device(x, torch.float64 if self._f64 else torch.float32)
        return backend.magnitude_to_decibel(
            x, ref_value=self.ref_value, amin=self.amin, dynamic_range=self.dynamic_range
        )

    def _db_params(self) -> _ffi.DbParams:
        # same validation (and order) as backend.magnitude_to_decibel, backend.py:168-173
        if self.ref_value <= 0:
            raise ValueError(f'ref_value must be positive, got: {self.ref_value}')
        if self.amin <= 0:
            raise ValueError(f'amin must be positive, got: {self.amin}')
        if self.dynamic_range <= 0:
            raise ValueError(f'dynamic_range must be positive, got: {self.dynamic_range}')
        return _ffi.DbParams(1, float(self.ref_value), float(self.amin), float(self.dynamic_range))

    def get_config(self):
        config = super(MagnitudeToDecibel, self).get_config()
        config.update(
            {
                'amin': self.amin,
                'dynamic_range': self.dynamic_range,
                'ref_value': self.ref_value,
            }
        )
        return config


@register_keras_serializable(package='Kapre')
class ApplyFilterbank(Layer):
    """Apply a (n_freq, n_filterbanks) filterbank along the frequency axis
    (reference: time_frequency.py:469-559).

    ``type`` is ``'mel'`` or ``'log'``; ``filterbank_kwargs`` go to ``backend.filterbank_mel`` /
    ``backend.filterbank_log``.  As upstream, any other ``type`` leaves ``self.filterbank``
    unset (AttributeError on use).
    """

    def __init__(
        self,
        type,
        filterbank_kwargs,
        data_format='default',
        **kwargs,
    ):
        super(ApplyFilterbank, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        if isinstance(data_format, dict):
            data_format = data_format['config']

        self.type = type
        self.filterbank_kwargs = filterbank_kwargs
        self._consts = _ffi.DeviceConstants()
        self._kranges = None
        self._fb_version = 0

        if type == 'log':
            self.filterbank = _log_filterbank = backend.filterbank_log(**filterbank_kwargs)
        elif type == 'mel':
            self.filterbank = _mel_filterbank = backend.filterbank_mel(**filterbank_kwargs)

        self.data_format_original = data_format
        self.data_format = backend.resolve_data_format(data_format)

        if self.data_format == _CH_FIRST_STR:
            self.freq_axis = 3
        else:
            self.freq_axis = 2

    @property
    def filterbank(self):
        """The (n_freq, n_filterbanks) float32 matrix.  ASSIGNING a new array (what
        ``dist.broadcast_constants`` does) bumps ``_fb_version`` and drops every device copy,
        packed copy and k-range table derived from the old one, here and in the fused-call plans
        (they are keyed on the version).  Mutating the array in place is not tracked.  As upstream,
        a ``type`` other than 'mel' / 'log' leaves the attribute unset (AttributeError on use)."""
        try:
            return self.__dict__['_filterbank']
        except KeyError:
            raise AttributeError("'ApplyFilterbank' object has no attribute 'filterbank'") from None

    @filterbank.setter
    def filterbank(self, value):
        self.__dict__['_filterbank'] = value
        self._fb_version += 1
        self._kranges = None
        self._consts.clear()

    def _fb_device(self, device):
        return self._consts.get('fb', device, lambda: np.asarray(self.filterbank, np.float32))

    def _fb_packed_device(self, device):
        """Filterbank in MFMA-fragment order (kpr_filterbank_pack), built once per device.  When the tensor is released
        (layer dropped, filterbank replaced) the library is told to forget the address: its header check is cached per
        address, and the allocator hands freed addresses out again."""
        return self._consts.get('fb_packed', device,
                                lambda: _ffi.filterbank_pack(np.asarray(self.filterbank, np.float32), self._fb_kranges()),
                                on_new=lambda t: weakref.finalize(t, _forget_packed, t.data_ptr()))

    def _fb_kranges(self):
        """Host int32 [lo, hi) row ranges per 16-filter tile (exact zeros outside)."""
        if self._kranges is None:
            self._kranges = _ffi.filterbank_kranges(np.asarray(self.filterbank, np.float32))
        return self._kranges

    def _fb_transposed_device(self, device, f64: bool):
        """(n_filt, n_freq) copy of the matrix: the backward pass is the same GEMM with it."""
        return self._consts.get('fbT64' if f64 else 'fbT', device,
                                lambda: np.ascontiguousarray(
                                    np.asarray(self.filterbank, np.float64 if f64 else np.float32).T))

    def compute_output_shape(self, input_shape):
        """the frequency axis (3 for channels_first, 2 for channels_last) becomes the number of filters"""
        shape = list(input_shape)
        shape[self.freq_axis] = int(self.filterbank.shape[1])
        return tuple(shape)

    def call(self, x):
        if autograd.needs_grad(x):
            x = autograd.prep(x, 'float64' if self._f64 else 'float32')
            return autograd.matrix(self, x, self._fb_transposed_device(x.device, self._f64), self.data_format)
        return self._forward(x)

    def _forward(self, x):
        import torch

        x = _ffi.as_device(x, torch.float64 if self._f64 else torch.float32)
        if x.dim() != 4:
            raise ValueError('ApplyFilterbank expects a rank-4 input, got shape %s'
                             % (tuple(x.shape),))
        k = _ffi.dims_of(x.shape, self.data_format)[3]
        n_freq, n_filt = self.filterbank.shape
        if k != n_freq:
            raise ValueError('frequency axis has %d bins but the filterbank expects %d'
                             % (k, n_freq))
        if self._f64:
            # the filterbank itself is floatx (float32) upstream as well (backend.py:231, :296); cast like TF does
            fb64 = self._consts.get('fb64', x.device, lambda: np.asarray(self.filterbank, np.float64))
            return _ffi.freq_matmul(x, self.data_format, fb64)
        kr = self._fb_kranges()
        packed = None
        thin = n_filt <= 64 and n_freq <= 512 and n_freq % 4 == 0          # the thin GEMM takes these
        if not thin and n_freq <= 1025:
            try:
                packed = self._fb_packed_device(x.device)      # wide banded matrix: MFMA consumer path
            except RuntimeError:
                packed = None                                   # band too wide to pack: generic GEMM
        return _ffi.freq_matmul(x, self.data_format, self._fb_device(x.device), packed, kr)

    def get_config(self):
        config = super(ApplyFilterbank, self).get_config()
        config.update(
            {
                'type': self.type,
                'filterbank_kwargs': self.filterbank_kwargs,
                'data_format': self.data_format_original,
            }
        )
        return config


@register_keras_serializable(package='Kapre')
class Delta(Layer):
    """Delta: a local estimate of the derivative along the time axis
    (reference: time_frequency.py:561-644).  ``tf.pad(mode)`` of ``(win_length - 1) // 2`` frames
    on both sides, correlation with ``[-n .. n]``, division by ``2 * sum(i^2)`` -- one kernel.
    Input / output: (b, t, f, ch) for ``channels_last``, (b, ch, t, f) for ``channels_first``."""

    def __init__(self, win_length=5, mode='symmetric', data_format='default', **kwargs):
        super(Delta, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        if isinstance(data_format, dict):
            data_format = data_format['config']
        if not win_length >= 3:
            raise ValueError(
                'win_length should be equal or bigger than 3, but it is %d' % win_length)
        if win_length % 2 != 1:
            raise ValueError('win_length should be an odd number, but it is %d' % win_length)
        if mode.lower() not in ('symmetric', 'reflect', 'constant'):
            raise ValueError(
                'mode.lower() should be one of {}'.format(str(('symmetric', 'reflect', 'constant')))
                + 'but it is {}'.format(mode))
        self.data_format_original = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self.win_length = win_length
        self.mode = mode
        self.n = (self.win_length - 1) // 2
        self.denom = 2 * sum([_n ** 2 for _n in range(1, self.n + 1, 1)])

    def call(self, x):
        if autograd.needs_grad(x):
            return autograd.delta(self, autograd.prep(x, 'float32'))
        return self._forward(x)

    def _forward(self, x):
        import torch

        x = _ffi.as_device(x, torch.float32)
        if x.dim() != 4:
            raise ValueError('Delta expects a rank-4 input, got shape %s' % (tuple(x.shape),))
        return _ffi.delta(x, self.data_format, self.win_length, self.mode)

    def get_config(self):
        config = super(Delta, self).get_config()
        config.update({'win_length': self.win_length, 'mode': self.mode,
                       'data_format': self.data_format_original})
        return config


@register_keras_serializable(package='Kapre')
class ConcatenateFrequencyMap(Layer):
    """Adds a frequency-information channel to a batch of spectrograms or feature maps (reference: time_frequency.py:647-744;
    with a following ``Conv2D``: frequency-aware convolution, Koutini et al. 2019).  The new last channel holds
    ``f / (n_freq - 1)`` for bin ``f``: 0.0 at the lowest bin, exactly 1.0 at the highest (0.0 when there is one bin).
    (b, t, f, ch) -> (b, t, f, ch + 1) for ``channels_last``, (b, ch, t, f) -> (b, ch + 1, t, f) for ``channels_first``;
    float32; one kernel writes the whole output in one pass (kpr_freq_map_concat_f32)."""

    def __init__(self, data_format='default', **kwargs):
        super(ConcatenateFrequencyMap, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        if isinstance(data_format, dict):           # (the reference's workaround for a Keras deserialisation bug)
            data_format = data_format['config']
        self.data_format_original = data_format
        self.data_format = backend.resolve_data_format(data_format)

    def compute_output_shape(self, input_shape):
        shape = list(input_shape)
        ch_axis = 3 if self.data_format == _CH_LAST_STR else 1
        if shape[ch_axis] is not None:
            shape[ch_axis] = int(shape[ch_axis]) + 1
        return tuple(shape)

    @staticmethod
    def _check(x):
        """float32 and rank 4, asked before anything reaches the device"""
        import torch

        if isinstance(x, torch.Tensor):
            dtype, ok = x.dtype, x.dtype == torch.float32
        else:
            x = x if isinstance(x, np.ndarray) else np.asarray(x)
            dtype, ok = x.dtype, x.dtype == np.float32
        if not ok:
            raise TypeError('ConcatenateFrequencyMap expects a float32 input, got %s' % (dtype,))
        if len(x.shape) != 4:
            raise ValueError('ConcatenateFrequencyMap expects a rank-4 input, got shape %s' % (tuple(x.shape),))

    def call(self, x):
        self._check(x)
        if autograd.needs_grad(x):
            return autograd.freq_map_concat(autograd.prep(x, 'float32'), self.data_format)
        return self._forward(x)

    def _forward(self, x):
        import torch

        return _ffi.freq_map_concat(_ffi.as_device(x, torch.float32), self.data_format)

    def get_config(self):
        config = super(ConcatenateFrequencyMap, self).get_config()
        config.update({'data_format': self.data_format_original})
        return config


@register_keras_serializable(package='Kapre')
class PCEN(Layer):
    """Per-channel energy normalisation (Wang et al. 2017, "Trainable frontend for robust and far-field keyword spotting"):
    the normalisation used in place of ``MagnitudeToDecibel`` behind a (mel) magnitude spectrogram.  Per batch item, channel
    and frequency band, along time:

        S[0] = x[0], S[t] = (1 - smooth_coef) S[t-1] + smooth_coef x[t]
        y[t] = (x[t] (eps + S[t])^-alpha + delta)^r - delta^r

    ``smooth_coef``, ``alpha``, ``delta``, ``r``: a scalar or a 1-D array with one value per band (0 < smooth_coef <= 1,
    alpha >= 0, delta > 0, r > 0, eps > 0: ``ValueError`` at construction; a vector's length is checked against the input at
    call time).  By default they are constants: the layer is differentiable with respect to its input only.
    (b, t, f, ch) for ``channels_last``, (b, ch, t, f) for ``channels_first``, same shape out; float32 (a float64 layer raises
    ``NotImplementedError``); one kernel, one pass (kpr_pcen_f32).  No frames: an empty tensor, nothing is launched.

    ``trainable_params``: ``True``, or a subset of ``('smooth_coef', 'alpha', 'delta', 'r')``, makes the named ones learned.
    ``build(input_shape)``, or the first call, creates one float32 ``torch.nn.Parameter`` of ``n_bands`` values for each (the
    constructor's value, a scalar broadcast), moved to the input's device by the first call there; ``parameters()`` lists them
    for a torch optimiser (``weights`` too; ``count_params()`` counts them).  The output then has a ``grad_fn`` also for an
    input that carries none, and ``backward()`` fills their ``.grad`` (kpr_pcen_bwd_params_f32; no input gradient is computed
    when the input needs none).  With the Keras keyword ``trainable=False`` the parameters exist but do not require grad.
    The kernels do not check the values: call ``constrain_()`` after an optimiser step to clamp them into the domain.
    ``get_config()`` carries the current (learned) values as lists, so a saved model reloads with them."""

    PARAM_NAMES = ('smooth_coef', 'alpha', 'delta', 'r')

    def __init__(self, smooth_coef=0.025, alpha=0.98, delta=2.0, r=0.5, eps=1e-6, data_format='default',
                 trainable_params=False, **kwargs):
        super(PCEN, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        if isinstance(data_format, dict):
            data_format = data_format['config']
        *self._params, self.eps = backend.pcen_parameters(smooth_coef, alpha, delta, r, eps)
        self.smooth_coef, self.alpha, self.delta, self.r = (
            np.asarray(v, dtype=np.float64).tolist() for v in (smooth_coef, alpha, delta, r))     # JSON-ready
        self.data_format_original = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self._consts = _ffi.DeviceConstants()
        if isinstance(trainable_params, bool):
            names = self.PARAM_NAMES if trainable_params else ()
        elif isinstance(trainable_params, (list, tuple)) and all(isinstance(n, str) for n in trainable_params):
            unknown = sorted(set(trainable_params) - set(self.PARAM_NAMES))
            if unknown or len(set(trainable_params)) != len(trainable_params):
                raise ValueError('PCEN: trainable_params must name each of %s at most once, got %r'
                                 % (self.PARAM_NAMES, trainable_params))
            names = tuple(n for n in self.PARAM_NAMES if n in trainable_params)
        else:
            raise ValueError('PCEN: trainable_params must be True, False or a list of names out of %s, got %r'
                             % (self.PARAM_NAMES, trainable_params))
        self.trainable_params = trainable_params if isinstance(trainable_params, bool) else list(names)
        self._trainable_names = names
        self._weights = None                                  # name -> torch.nn.Parameter, made by build() / the first call

    def compute_output_shape(self, input_shape):
        return tuple(input_shape)

    def build(self, input_shape, device=None):
        """Create the learned parameters for an input of ``input_shape`` (with the batch axis) on ``device`` (default: the CPU;
        the first call moves them to its input's device).  Nothing to do for a layer without learned parameters."""
        if not self._trainable_names or self._weights is not None:
            return
        import torch

        if len(input_shape) != 4:
            raise ValueError('PCEN expects a rank-4 input, got shape %s' % (tuple(input_shape),))
        n_bands = input_shape[2] if self.data_format == 'channels_last' else input_shape[3]
        if n_bands is None or int(n_bands) <= 0:
            raise ValueError('PCEN: the learned parameters need a known, positive number of bands, got input shape %s'
                             % (tuple(input_shape),))
        table = backend.pcen_band_table(self._params, int(n_bands))
        self._weights = {
            name: torch.nn.Parameter(torch.from_numpy(table[self.PARAM_NAMES.index(name)].copy()).to(device or 'cpu'),
                                     requires_grad=bool(self.trainable))
            for name in self._trainable_names}

    def parameters(self):
        """The learned parameters (``torch.nn.Parameter``, one value per band) in the order smooth_coef, alpha, delta, r: what a
        torch optimiser takes.  ``RuntimeError`` before ``build`` / the first call of a layer that has some."""
        if self._trainable_names and self._weights is None:
            if self._input_shape_arg is None:
                raise RuntimeError('PCEN: the parameters are created by build(input_shape) or the first call')
            self.build((None,) + tuple(self._input_shape_arg))
        return [self._weights[n] for n in self._trainable_names]

    @property
    def weights(self):
        return [self._weights[n] for n in self._trainable_names] if self._weights is not None else []

    def count_params(self) -> int:
        return sum(int(w.numel()) for w in self.weights)

    def constrain_(self):
        """Clamp the learned parameters in place into the domain of the definition: smooth_coef into [2^-10, 1], alpha >= 0,
        delta and r at least the smallest positive normal float32.  For use after an optimiser step."""
        import torch

        tiny = float(np.finfo(np.float32).tiny)
        bounds = {'smooth_coef': (2.0 ** -10, 1.0), 'alpha': (0.0, None), 'delta': (tiny, None), 'r': (tiny, None)}
        with torch.no_grad():
            for name, w in zip(self._trainable_names, self.weights):
                w.clamp_(min=bounds[name][0], max=bounds[name][1])
        return self

    def call(self, x):
        if self._f64:
            raise NotImplementedError('PCEN has float32 kernels only; build the layer with dtype float32')
        tensors = None
        if self._trainable_names:
            import torch

            if len(x.shape) != 4:
                raise ValueError('PCEN expects a rank-4 input, got shape %s' % (tuple(x.shape),))
            _ffi.require_gpu()
            device = x.device if isinstance(x, torch.Tensor) and x.is_cuda else torch.device('cuda', torch.cuda.current_device())
            self.build(tuple(x.shape), device)
            for w in self._weights.values():
                if w.device != device:
                    w.data = w.data.to(device)                # (the Parameter an optimiser holds stays the same object)
                w.requires_grad_(bool(self.trainable))
            tensors = [self._weights.get(n) for n in self.PARAM_NAMES]
        return backend._pcen_run(
            x, lambda n, device: self._consts.get(('pcen', n), device, lambda: backend.pcen_band_table(self._params, n)),
            self.eps, self.data_format, tensors)

    def get_config(self):
        config = super(PCEN, self).get_config()
        values = {'smooth_coef': self.smooth_coef, 'alpha': self.alpha, 'delta': self.delta, 'r': self.r}
        for name, w in zip(self._trainable_names, self.weights):
            values[name] = w.detach().cpu().numpy().astype(np.float64).tolist()       # the learned values
        config.update(values)
        config.update({'eps': self.eps, 'data_format': self.data_format_original})
        if self._trainable_names:
            config['trainable_params'] = self.trainable_params
        return config


@register_keras_serializable(package='Kapre')
class CMVN(Layer):
    """Per-utterance mean and variance normalisation along time (Kaldi's ``apply-cmvn --norm-vars``, ESPnet's
    ``UtteranceMVN``; instance normalisation over time), the step behind a log-mel spectrogram.  Per batch item, channel and
    frequency band, over its n frames:

        d[t] = x[t] - x[0];  m = mean(d);  c[t] = d[t] - m
        y[t] = c[t] / sqrt(mean(c^2) + eps)    (``norm_vars=True``: population variance)
        y[t] = c[t]                            (``norm_vars=False``: mean normalisation only)

    ``norm_vars`` must be a bool and ``eps`` a finite number >= 0 (``ValueError`` at construction).  A constant series -- a band
    clamped to the decibel floor -- gives exactly +0.0.  (b, t, f, ch) for ``channels_last``, (b, ch, t, f) for
    ``channels_first``, same shape out; float32 (a float64 layer raises ``NotImplementedError``); one kernel
    (kpr_cmvn_f32), one pass up to 128 frames, two reads of the input beyond.  No frames: an empty tensor, nothing is
    launched.  No parameters; differentiable with respect to its input (one backward launch, kpr_cmvn_bwd_f32)."""

    def __init__(self, norm_vars=True, eps=1e-5, data_format='default', **kwargs):
        super(CMVN, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        if isinstance(data_format, dict):
            data_format = data_format['config']
        self.norm_vars, self.eps = backend.cmvn_parameters(norm_vars, eps)
        self.data_format_original = data_format
        self.data_format = backend.resolve_data_format(data_format)

    def compute_output_shape(self, input_shape):
        return tuple(input_shape)

    def call(self, x):
        if self._f64:
            raise NotImplementedError('CMVN has float32 kernels only; build the layer with dtype float32')
        return backend._cmvn_run(x, self.norm_vars, self.eps, self.data_format)

    def get_config(self):
        config = super(CMVN, self).get_config()
        config.update({'norm_vars': self.norm_vars, 'eps': self.eps, 'data_format': self.data_format_original})
        return config


_GL_CONSTS = _ffi.DeviceConstants()          # the windows of backend.griffin_lim (the layer keeps its own)


def _griffin_lim_run(x, consts, n_fft, win_length, hop_length, window_name, window_fn, n_iter, momentum, power, rand_init,
                     length, spec_fmt, wave_fmt, init=None):
    """(waveform, sc) of one Griffin-Lim run on ``x`` in resolved data formats; the windows come from ``consts`` and the
    scratch from the workspace pool of the current stream."""
    import torch

    from .augmentation import device_state
    x, _ = autograd.intake(x.detach() if isinstance(x, torch.Tensor) else x, 4, 'float32',
                           'GriffinLim expects a rank-4 input, got shape %s', TypeError,
                           'GriffinLim has float32 kernels only; got a float64 input (cast it to float32)')
    k = _ffi.dims_of(x.shape, spec_fmt)[3]
    if k != n_fft // 2 + 1:
        raise ValueError('GriffinLim: the frequency axis has %d bins, n_fft = %d needs %d' % (k, n_fft, n_fft // 2 + 1))
    if init is not None:
        if isinstance(init, torch.Tensor):
            init = init.detach()
        init = _ffi.as_device(init, torch.complex64)
        if tuple(init.shape) != tuple(x.shape) or init.device != x.device:
            raise ValueError('GriffinLim: init must have the shape %s of the magnitude and live on its device, got %s on %s'
                             % (tuple(x.shape), tuple(init.shape), init.device))
    synth_fn = backend.inverse_stft_window_fn(frame_step=hop_length, forward_window_fn=window_fn)
    key = (window_name if isinstance(window_name, str) or window_name is None else id(window_fn), win_length, hop_length)
    win = consts.get(('gl_window',) + key, x.device, lambda: window_fn(win_length))
    synth = consts.get(('gl_synth',) + key, x.device, lambda: synth_fn(win_length))
    mode = _ffi.GL_INIT_GIVEN if init is not None else _ffi.GL_INIT_RANDOM if rand_init else _ffi.GL_INIT_ZERO
    state = device_state(x.device) if mode == _ffi.GL_INIT_RANDOM and x.numel() > 0 else None
    b, c, f, _ = _ffi.dims_of(x.shape, spec_fmt)
    g = _ffi.StftGeom(b, c, 0, n_fft, win_length, hop_length, 0, 0, _ffi.layout(wave_fmt), _ffi.layout(spec_fmt))
    ws_bytes = _ffi.griffin_lim_workspace_bytes(g, f, momentum, power)
    ws = _PLAN_WORKSPACES.get(ws_bytes, x.device, torch.cuda.current_stream(x.device).cuda_stream)
    wave, sc = _ffi.griffin_lim(x, win, synth, n_fft, win_length, hop_length, wave_fmt, spec_fmt, n_iter, momentum, power, mode,
                                init, state, True, ws)
    if length is not None:
        axis = 1 if wave_fmt == _CH_LAST_STR else 2
        t = wave.shape[axis]
        if length < t:
            wave = wave.narrow(axis, 0, int(length)).contiguous()
        elif length > t:
            wave = torch.nn.functional.pad(wave, [0, 0, 0, int(length) - t] if axis == 1 else [0, int(length) - t])
    return wave, sc


@register_keras_serializable(package='Kapre')
class GriffinLim(Layer):
    """Griffin-Lim phase reconstruction: a magnitude spectrogram back to a waveform (Griffin & Lim 1984, with the momentum
    term of Perraudin, Balazs & Sondergaard 2013 -- the algorithm of ``librosa.griffinlim`` and torchaudio's ``GriffinLim``),
    the inverse direction behind ``get_stft_magnitude_layer(return_decibel=False)``.  With A this package's ``STFT(n_fft,
    win_length, hop_length, window_name)`` without padding, A+ its ``InverseSTFT(..., forward_window_name=window_name)`` and
    c = momentum / (1 + momentum):

        mag = x ** (1 / power);  S_0 = mag e^{i phi}  (phi random with ``rand_init``, else 0);  T_0 = 0
        n = 1 .. n_iter:  R = A(A+(S));  a = R - c T;  S = mag a / (|a| + 1e-16);  T = R
        y = A+(S)

    Framing is tf.signal's (not centred), as in the two transforms.  Input (b, frame, n_fft // 2 + 1, ch) for
    ``channels_last``, (b, ch, frame, n_fft // 2 + 1) for ``channels_first``, float32 and not negative; output (b, time, ch) /
    (b, ch, time) with (frame - 1) hop + win samples, or exactly ``length`` (trimmed, or padded with zeros).  ``momentum = 0``
    is the classical algorithm; ``n_iter = 0`` is one inverse transform of S_0.  ``n_iter < 0``, ``momentum`` outside [0, 1)
    and ``power <= 0`` raise ``ValueError``, a float64 input ``TypeError``.

    The whole run stays on the device: one call of kpr_griffin_lim_f32 queues every launch on the current stream, waits for
    nothing and copies nothing to the host.  The random phase comes from SpecAugment's device generator
    (``augmentation.set_seed`` makes runs repeatable; every call with ``rand_init`` advances it by one).  After a call
    ``last_convergence`` is the device tensor (n_iter, batch) of || |R_n| - mag || / || mag || per batch item.

    The output carries no ``grad_fn``: the layer is not differentiable, and an input that requires grad is detached."""

    def __init__(self, n_fft=2048, win_length=None, hop_length=None, window_name=None, n_iter=32, momentum=0.99, power=1.0,
                 rand_init=True, length=None, input_data_format='default', output_data_format='default', **kwargs):
        super(GriffinLim, self).__init__(**kwargs)
        for data_format in (input_data_format, output_data_format):
            backend.validate_data_format_str(data_format)
        if isinstance(input_data_format, dict):
            input_data_format = input_data_format['config']
        if isinstance(output_data_format, dict):
            output_data_format = output_data_format['config']
        if win_length is None:
            win_length = n_fft
        if hop_length is None:
            hop_length = win_length // 4
        self.n_iter, self.momentum, self.power = backend.griffin_lim_parameters(n_iter, momentum, power)
        if length is not None and (isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 0):
            raise ValueError('GriffinLim: length must be None or an integer >= 0, got %r' % (length,))
        self.n_fft = n_fft
        self.win_length = win_length
        self.hop_length = hop_length
        self.window_name = window_name
        self.window_fn = backend.get_window_fn(window_name)   # NotImplementedError if unknown
        self.rand_init = bool(rand_init)
        self.length = None if length is None else int(length)
        self.input_data_format_original = input_data_format
        self.output_data_format_original = output_data_format
        self.input_data_format = backend.resolve_data_format(input_data_format)
        self.output_data_format = backend.resolve_data_format(output_data_format)
        self._consts = _ffi.DeviceConstants()
        self.last_convergence = None

    def compute_output_shape(self, input_shape):
        """(b, frame, freq, ch) / (b, ch, frame, freq) -> (b, t, ch) / (b, ch, t), t = ``length`` or (frame - 1) hop + win"""
        b, c, f, _ = _ffi.dims_of(input_shape, self.input_data_format)
        if self.length is not None:
            t = self.length
        else:
            t = None if f is None else ((int(f) - 1) * int(self.hop_length) + int(self.win_length) if int(f) > 0 else 0)
        return _ffi.shape_of(self.output_data_format, b, c, t)

    def call(self, x):
        if self._f64:
            raise TypeError('GriffinLim has float32 kernels only; build the layer with dtype float32')
        wave, self.last_convergence = _griffin_lim_run(
            x, self._consts, int(self.n_fft), int(self.win_length), int(self.hop_length), self.window_name, self.window_fn,
            self.n_iter, self.momentum, self.power, self.rand_init, self.length, self.input_data_format, self.output_data_format)
        return wave

    def get_config(self):
        config = super(GriffinLim, self).get_config()
        config.update(
            {
                'n_fft': self.n_fft,
                'win_length': self.win_length,
                'hop_length': self.hop_length,
                'window_name': self.window_name,
                'n_iter': self.n_iter,
                'momentum': self.momentum,
                'power': self.power,
                'rand_init': self.rand_init,
                'length': self.length,
                'input_data_format': self.input_data_format_original,
                'output_data_format': self.output_data_format_original,
            }
        )
        return config


_TS_CONSTS = _ffi.DeviceConstants()          # the tables of backend.phase_vocoder (the layer keeps its own)


def _time_stretch_run(x, rate, fmt, consts):
    """``x`` through the phase vocoder at the validated ``rate`` in the resolved data format ``fmt``; the tables come from
    ``consts``, one pair per (frames, rate, device)."""
    import torch

    cplx = x.is_complex() if isinstance(x, torch.Tensor) else np.iscomplexobj(x)
    if len(x.shape) == 4 and not cplx:                   # (behind the rank refusal, ahead of the 64-bit one)
        raise TypeError('TimeStretch expects a complex spectrogram (the output of STFT), got dtype %s' % (x.dtype,))
    x, _ = autograd.intake(x.detach() if isinstance(x, torch.Tensor) else x, 4, 'complex64',
                           'TimeStretch expects a rank-4 input, got shape %s', TypeError,
                           'TimeStretch has float32 kernels only; got a complex128 input (cast it to complex64)')
    frames = int(_ffi.dims_of(x.shape, fmt)[2])
    frames_out = backend.time_stretch_length(frames, rate)
    table = lambda which: (lambda: backend.time_stretch_table(frames, rate)[which])
    idx = consts.get(('ts_idx', frames, rate), x.device, table(0))
    alpha = consts.get(('ts_alpha', frames, rate), x.device, table(1))
    return _ffi.time_stretch(x, fmt, idx, alpha, frames_out)


@register_keras_serializable(package='Kapre')
class TimeStretch(Layer):
    """Phase-vocoder time stretching of a complex spectrogram: the speed of the signal changes, its pitch does not
    (``torchaudio.transforms.TimeStretch``, ``librosa.phase_vocoder``).  It sits between ``STFT`` and ``InverseSTFT``
    (``composed.get_time_stretch_layer``).  ``rate`` < 1 slows the signal down, ``rate`` > 1 speeds it up: T input frames give
    T' = ceil(T / rate) output frames.  For output frame t, with s = t * rate (float64), i = floor(s), a = s - i, and the frames
    X[T] and X[T + 1] taken as zero, per bin:

        Theta(x) = 2 rint(atan2f(im, re) c) as a uint32 word, 2^32 = one turn, c = float32(2^30 / pi);
                   0 for a bin that is zero (whatever the signs of the zeros) or not finite
        P[0] = Theta(X[0]);   P[t + 1] = P[t] + Theta(X[i + 1]) - Theta(X[i])     (uint32 arithmetic)
        m[t] = a |X[i + 1]| + (1 - a) |X[i]|
        Y[t] = m[t] (cos, sin)(pi h),   h = (float)(int32)P[t] 2^-31

    There is no ``hop_length`` argument.  The textbook recurrence adds wrap(angle X[i + 1] - angle X[i] - adv) + adv per step,
    adv being the phase a bin's centre frequency advances in one hop; wrap() changes its argument by a whole number of turns, so
    the accumulated phase equals angle X[0] + sum (angle X[i + 1] - angle X[i]) modulo 2 pi, and Y depends on it only modulo
    2 pi: adv, and with it the hop length, drops out.  Kept as 32-bit fixed-point words the sum is integer addition -- it wraps by
    itself and loses no precision however long the clip, where a float32 running sum of radians drifts.

    ``rate = 1`` gives P[t] = Theta(X[t]) and returns the input up to rounding.  A non-finite bin makes non-finite only the
    output frames that read it; every other frame is bit for bit what it would be with that bin set to 0.  The same inputs give
    the same bits.  (b, frame, freq, ch) for ``channels_last``, (b, ch, frame, freq) for ``channels_first``; complex64 in and
    out, one kernel launch (kpr_time_stretch_c64); the index tables are computed on the host in float64 once per
    (frames, device) and kept.  ``rate`` must be a finite number > 0 and not a bool (``ValueError``), the input rank 4
    (``ValueError``) and complex (``TypeError``); a complex128 input or a float64 layer raises ``TypeError``.

    The output carries no ``grad_fn``: the layer is not differentiable, and an input that requires grad is detached."""

    def __init__(self, rate, data_format='default', **kwargs):
        super(TimeStretch, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        if isinstance(data_format, dict):
            data_format = data_format['config']
        self.rate = backend.time_stretch_parameters(rate)
        self.data_format_original = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self._consts = _ffi.DeviceConstants()

    def compute_output_shape(self, input_shape):
        """frames -> ceil(frames / rate); ``None`` stays ``None``"""
        b, c, f, k = _ffi.dims_of(input_shape, self.data_format)
        return _ffi.shape_of(self.data_format, b, c, backend.time_stretch_length(f, self.rate), k)

    def call(self, x):
        if self._f64:
            raise TypeError('TimeStretch has float32 kernels only; build the layer with dtype float32')
        return _time_stretch_run(x, self.rate, self.data_format, self._consts)

    def get_config(self):
        config = super(TimeStretch, self).get_config()
        config.update({'rate': self.rate, 'data_format': self.data_format_original})
        return config


def _hpss_run(x, sizes, power, margins, mask, fmt, output):
    """``x`` through the separation with validated parameters in the resolved data format ``fmt``; ``output`` as in
    ``_ffi.hpss``."""
    import torch

    cplx = x.is_complex() if isinstance(x, torch.Tensor) else np.iscomplexobj(x)
    x, _ = autograd.intake(x.detach() if isinstance(x, torch.Tensor) else x, 4, 'complex64' if cplx else 'float32',
                           'HPSS expects a rank-4 input, got shape %s', TypeError,
                           'HPSS has float32 kernels only; got a %s input (cast it to float32 / complex64)' % (x.dtype,))
    return _ffi.hpss(x, fmt, sizes[0], sizes[1], power, margins[0], margins[1], _ffi.HPSS_MASKS if mask else _ffi.HPSS_VALUES, output)


@register_keras_serializable(package='Kapre')
class HPSS(Layer):
    """Median-filter harmonic-percussive source separation of a spectrogram (Fitzgerald 2010 with Driedger's margins;
    ``librosa.decompose.hpss``, ``librosa.effects.harmonic`` / ``percussive``).  Per (batch item, channel) plane S of T frames
    and F bins, with the window lengths (kh, kp) = ``kernel_size`` and the margins (mh, mp) = ``margin``:

        H[t, f] = median of S[r(t + d, T), f], |d| <= (kh - 1) / 2          (along time: what is steady is harmonic)
        P[t, f] = median of S[t, r(f + d, F)], |d| <= (kp - 1) / 2          (along frequency: what is broadband is percussive)
        r(i, n): j = i mod 2n; j if j < n else 2n - 1 - j                   (the edge repeats: d c b a | a b c d | d c b a)
        soft(X, R) = (X / Z)^power / ((X / Z)^power + (R / Z)^power), Z = max(X, R);  where Z < 2^-126: 0.5 if both margins are 1,
                     else 0;  power = inf: 1 where X > R, else 0
        Mh = soft(H, P mh),  Mp = soft(P, H mp);   harmonic = S Mh,  percussive = S Mp

    The median is a selection -- it equals one of its inputs bit for bit -- and NaN orders above +Inf as in ``numpy.sort``, so a
    single NaN bin makes NaN only its own bin of the outputs; everything else is what it would be with +Inf there.  The same
    inputs give the same bits.  A complex64 input (the output of ``STFT``) is separated by the masks of its magnitude: the
    outputs are complex64 and go straight into ``InverseSTFT`` (``composed.get_hpss_layer``).

    ``output``: 'harmonic', 'percussive', or 'both' -- one tensor with the channel axis doubled, the harmonic channels first,
    then the percussive ones: two input planes for a CNN, twice the waveform channels behind ``InverseSTFT``.  ``mask=True``
    returns the float32 masks instead.  ``kernel_size`` and ``margin`` are a scalar or a (harmonic, percussive) pair: sizes odd
    and in 3 ... 31, margins >= 1, ``power`` > 0 or ``inf`` (``ValueError`` otherwise).  (b, frame, freq, ch) for
    ``channels_last``, (b, ch, frame, freq) for ``channels_first``; one kernel launch (kpr_hpss_f32 / kpr_hpss_c64).  The input
    must have rank 4 (``ValueError``); a float64 / complex128 input or a float64 layer raises ``TypeError``.

    The output carries no ``grad_fn``: the layer is not differentiable (a median has no useful gradient), and an input that
    requires grad is detached."""

    def __init__(self, kernel_size=31, power=2.0, margin=1.0, output='both', mask=False, data_format='default', **kwargs):
        super(HPSS, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        if isinstance(data_format, dict):
            data_format = data_format['config']
        if output not in ('harmonic', 'percussive', 'both'):
            raise ValueError("HPSS: output must be 'harmonic', 'percussive' or 'both', got %r" % (output,))
        self.kernel_size, self.power, self.margin = backend.hpss_parameters(kernel_size, power, margin)
        self.output = output
        self.mask = bool(mask)
        self.data_format_original = data_format
        self.data_format = backend.resolve_data_format(data_format)

    def compute_output_shape(self, input_shape):
        """the input's shape; 'both' doubles the channel axis (``None`` stays ``None``)"""
        b, c, f, k = _ffi.dims_of(input_shape, self.data_format)
        if self.output == 'both' and c is not None:
            c = 2 * c
        return _ffi.shape_of(self.data_format, b, c, f, k)

    def call(self, x):
        if self._f64:
            raise TypeError('HPSS has float32 kernels only; build the layer with dtype float32')
        return _hpss_run(x, self.kernel_size, self.power, self.margin, self.mask, self.data_format, self.output)

    def get_config(self):
        config = super(HPSS, self).get_config()
        config.update({'kernel_size': list(self.kernel_size), 'power': self.power, 'margin': list(self.margin),
                       'output': self.output, 'mask': self.mask, 'data_format': self.data_format_original})
        return config


# --------------------------------------------------------------------------------------------
# fused execution
# --------------------------------------------------------------------------------------------
class _MelPlan:
    """Everything of one fused call that does not depend on the data: geometry, output shape,
    workspace and the ctypes argument objects.  Cached per (input shape, device, stream, dB)."""

    __slots__ = ('g', 'g_ref', 'out_shape', 'n_filt', 'db', 'db_ref', 'ws', 'ws_ptr', 'ws_bytes',
                 'win', 'win_ptr', 'fb', 'fb_ptr', 'fbp', 'fbp_ptr', 'kr', 'kr_ptr', 'stream',
                 'fb_layer', 'db_layer')


def _mel_plan(stft, fb_layer, db_layer, x, stream_ptr):
    import torch

    plan = _MelPlan()
    plan.g = stft._geom(x)
    plan.g_ref = ctypes.byref(plan.g)
    n_frames = _ffi.num_frames(plan.g)
    n_freq, n_filt = fb_layer.filterbank.shape
    if n_freq != int(stft.n_fft) // 2 + 1:
        raise ValueError('filterbank has %d frequency rows but the STFT produces %d bins'
                         % (n_freq, int(stft.n_fft) // 2 + 1))
    plan.n_filt = n_filt
    plan.db = db_layer._db_params() if db_layer is not None else _ffi.DbParams(0, 1.0, 1e-5, 80.0)
    plan.db_ref = ctypes.byref(plan.db)
    plan.out_shape = _ffi.shape_of(plan.g.out_layout, plan.g.batch, plan.g.channels, n_frames, n_filt)
    plan.fb_layer, plan.db_layer = fb_layer, db_layer       # keep the key's objects alive (no id() reuse)
    plan.win = stft._window(x.device)
    plan.win_ptr = _ffi.ptr(plan.win)
    plan.fb = fb_layer._fb_device(x.device)
    plan.fb_ptr = _ffi.ptr(plan.fb)
    try:
        plan.fbp = fb_layer._fb_packed_device(x.device)
    except RuntimeError:
        plan.fbp = None                 # more filter tiles than the packed schedule holds: generic product
    plan.fbp_ptr = _ffi.ptr(plan.fbp)
    plan.ws_bytes = _ffi.mel_workspace_bytes(plan.g_ref, n_filt, plan.db_ref, plan.fbp is not None)
    plan.ws = _PLAN_WORKSPACES.get(plan.ws_bytes, x.device, stream_ptr)
    plan.ws_ptr = _ffi.ptr(plan.ws)
    plan.kr = fb_layer._fb_kranges()
    plan.kr_ptr = plan.kr.ctypes.data_as(ctypes.c_void_p)
    plan.stream = ctypes.c_void_p(stream_ptr)
    return plan


def fused_melspectrogram(stft: STFT, fb_layer: ApplyFilterbank, db_layer, x):
    """STFT -> Magnitude -> ApplyFilterbank [-> MagnitudeToDecibel] in one launch (kpr_mel_f32)."""
    import torch

    x = _ffi.as_device(x, torch.float32)
    dev = x.device
    stream_ptr = torch.cuda.current_stream(dev).cuda_stream
    db_key = None if db_layer is None else (db_layer.ref_value, db_layer.amin, db_layer.dynamic_range)
    key = (tuple(x.shape), dev.index, stream_ptr, db_key, id(fb_layer), fb_layer._fb_version,
           stft._plan_version())
    cache = stft.__dict__.setdefault('_mel_plans', {})
    plan = cache.get(key)
    if plan is None or plan.fb_layer is not fb_layer:
        if len(cache) >= 64:
            cache.pop(next(iter(cache)))        # oldest plan; its scratch lives in the pool, not in the plan
        plan = cache[key] = _mel_plan(stft, fb_layer, db_layer, x, stream_ptr)
    out = torch.empty(plan.out_shape, dtype=torch.float32, device=dev)
    L = _ffi.lib()

    def launch():
        return L.kpr_mel_f32(x.data_ptr(), plan.g_ref, plan.win_ptr, plan.fb_ptr, plan.fbp_ptr, plan.n_filt,
                             plan.kr_ptr, plan.db_ref, out.data_ptr(), plan.ws_ptr, plan.ws_bytes, plan.stream)

    if torch.cuda.current_device() != dev.index:
        with torch.cuda.device(dev):
            rc = launch()
    else:
        rc = launch()
    if rc == _ffi.E_WORKSPACE and plan.fbp is not None:
        # KPR_E_WORKSPACE: a bank whose schedule none of the fused kernels holds (dense matrices): the two-launch path stages the
        # spectrum and needs the unpacked workspace -- the plan is upgraded once and keeps the larger workspace
        ws_bytes = _ffi.mel_workspace_bytes(plan.g_ref, plan.n_filt, plan.db_ref, False)
        if ws_bytes > plan.ws_bytes:
            plan.ws_bytes = ws_bytes
            plan.ws = _PLAN_WORKSPACES.get(plan.ws_bytes, dev, stream_ptr)
            plan.ws_ptr = _ffi.ptr(plan.ws)
            with torch.cuda.device(dev):
                rc = launch()
    if rc:
        _ffi.check(rc, 'kpr_mel_f32')
    return out


def _run_mel_group(group, x):
    db_layer = group[3] if len(group) == 4 else None
    return fused_melspectrogram(group[0], group[2], db_layer, x)


def _run_stft_mag(group, x):
    return group[0]._run(x, _ffi.OUT_MAGNITUDE)


def _run_stft_phase(group, x):
    return group[0]._run(x, _ffi.OUT_PHASE)


def _chain_owns(layer, x, y, owned: bool) -> bool:
    """True when ``y = layer(x)`` is a tensor only this chain holds: the owned ``x`` handed through, or the output of one of
    this package's layers that does not share ``x``'s storage (keras_shim.Layer: the layers of this package return fresh
    tensors and keep no reference to them; a view of the input is recognised here and counts as the input)."""
    import torch

    if y is x:
        return owned
    if (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.device == y.device
            and x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr()):
        return owned
    return type(layer).__module__.startswith(__package__ + '.')


def fuse_and_run(layers, x, training=None):
    """Run a flat list of layers, fusing the Kapre chains that have a single-kernel form.  When ``x`` carries gradient
    a fused group runs as one autograd node (forward = the fused launch, backward = recomputation through the
    individual layers, kapre_amd/autograd.py).  ``training`` goes to the layers whose ``call`` takes it; when it is true a
    ``SpecAugment`` masks IN PLACE a float32 tensor that a kernel of this chain produced, that nobody else holds and that
    carries no gradient (no second buffer) -- the chain's own input is never modified."""
    import torch

    i, n = 0, len(layers)
    owned = False                    # x is an output of this chain that nobody else holds
    while i < n:
        layer = layers[i]
        group, runner = None, None
        # (layers of different compute dtypes are never fused; the single-kernel mel chain is float32 only)
        if type(layer) is STFT and i + 1 < n and layers[i + 1]._f64 == layer._f64:
            nxt = layers[i + 1]
            if type(nxt) is Magnitude:
                # STFT -> Magnitude -> ApplyFilterbank [-> MagnitudeToDecibel]
                if (not layer._f64 and i + 2 < n and type(layers[i + 2]) is ApplyFilterbank
                        and not layers[i + 2]._f64
                        and not (i + 3 < n and type(layers[i + 3]) is MagnitudeToDecibel and layers[i + 3]._f64)
                        and hasattr(layers[i + 2], 'filterbank')
                        and layers[i + 2].data_format == layer.output_data_format):
                    step = 4 if i + 3 < n and type(layers[i + 3]) is MagnitudeToDecibel else 3
                    group, runner = layers[i:i + step], _run_mel_group
                else:
                    # STFT -> Magnitude (magnitude written straight from the FFT kernel)
                    group, runner = layers[i:i + 2], _run_stft_mag
            elif type(nxt) is Phase:
                group, runner = layers[i:i + 2], _run_stft_phase
        if group is not None:
            x = autograd.chain(group, x, runner) if autograd.needs_grad(x) else runner(group, x)
            owned = True
            i += len(group)
            continue
        if (type(layer) is SpecAugment and training not in (None, False) and owned and isinstance(x, torch.Tensor)
                and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and not x.requires_grad):
            x = layer._forward(x, inplace=True)
        else:
            y = layer(x, training=training)
            owned = _chain_owns(layer, x, y, owned)
            x = y
        i += 1
    return x
