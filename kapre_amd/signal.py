"""Signal layers: the consumers / neighbours of the time-frequency path that SURVEY 8f row 4 names
(reference: /root/reference/kapre/signal.py).  Frame, Energy and LogmelToMFCC keep the reference's
constructor signatures, validation, get_config() keys and output shapes; the arithmetic runs in
libkapre_hip.so (kpr_frame_f32 / kpr_energy_f32 / kpr_apply_filterbank_f32 with a DCT-II matrix).
MuLawEncoding / MuLawDecoding (signal.py:236-361) are thin layers over backend.mu_law_encoding / mu_law_decoding
(kpr_mu_law_encode_f32 / kpr_mu_law_decode_i32 / kpr_mu_law_decode_f32).  Resample has no counterpart in the reference: it is
the step in front of every front end (kpr_resample_f32).  Neither have LFilter, Preemphasis and Deemphasis: biquad filtering of
the waveform itself (kpr_lfilter_f32), Convolve: convolution with a fixed impulse response (kpr_stft_f32, kpr_spec_fir_c64,
kpr_istft_f32), and PitchShift: a time stretch and the table-free resampler (kpr_resample_direct_f32)."""
import math

import numpy as np

from . import _ffi, autograd, backend
from .backend import _CH_FIRST_STR, _CH_LAST_STR
from .keras_shim import Layer, register_keras_serializable

__all__ = ['Frame', 'Energy', 'MuLawEncoding', 'MuLawDecoding', 'LogmelToMFCC', 'Resample', 'LFilter', 'Preemphasis',
           'Deemphasis', 'Convolve', 'PitchShift']


def _as_waveform(x):
    import torch

    x = _ffi.as_device(x, torch.float32)
    if x.dim() != 3:
        raise ValueError('expected a rank-3 waveform batch, got shape %s' % (tuple(x.shape),))
    return x


@register_keras_serializable(package='Kapre')
class Frame(Layer):
    """Frame the input audio signal -- ``tf.signal.frame`` (reference: signal.py:22-119).

    (batch, time, ch) -> (batch, n_frame, frame_length, ch) for ``channels_last``;
    (batch, ch, time) -> (batch, ch, n_frame, frame_length) for ``channels_first``."""

    def __init__(self, frame_length, hop_length, pad_end=False, pad_value=0, data_format='default',
                 **kwargs):
        super(Frame, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        if frame_length <= 0:
            raise ValueError(f'frame_length must be positive, got: {frame_length}')
        if hop_length <= 0:
            raise ValueError(f'hop_length must be positive, got: {hop_length}')
        if frame_length < hop_length:
            raise ValueError(f'frame_length ({frame_length}) must be >= hop_length ({hop_length})')
        self.frame_length = frame_length
        self.hop_length = hop_length
        self.pad_end = pad_end
        self.pad_value = pad_value
        self.data_format_str = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self.time_axis = 2 if self.data_format == _CH_FIRST_STR else 1

    def compute_output_shape(self, input_shape):
        """(b, t, ch) -> (b, frame, frame_length, ch); (b, ch, t) -> (b, ch, frame, frame_length) (tf.signal.frame)"""
        b, c, t = _ffi.dims_of(input_shape, self.data_format)
        n = None
        if t is not None:
            t, fl, hop = int(t), int(self.frame_length), int(self.hop_length)
            n = -(-t // hop) if self.pad_end else max(0, 1 + (t - fl) // hop)
        return _ffi.shape_of(self.data_format, b, c, n, int(self.frame_length))

    def call(self, x):
        if autograd.needs_grad(x):
            return autograd.frame(self, autograd.prep(x, 'float32'))
        return self._forward(x)

    def _forward(self, x):
        return _ffi.frame(_as_waveform(x), self.data_format, self.frame_length, self.hop_length, self.pad_end,
                          self.pad_value)

    def get_config(self):
        config = super(Frame, self).get_config()
        config.update({'frame_length': self.frame_length, 'hop_length': self.hop_length,
                       'pad_end': self.pad_end, 'pad_value': self.pad_value,
                       'data_format': self.data_format_str})
        return config


@register_keras_serializable(package='Kapre')
class Energy(Layer):
    """Energy of each frame, normalised to ``ref_duration`` (reference: signal.py:122-240).

    (batch, time, ch) -> (batch, n_frame, ch); (batch, ch, time) -> (batch, ch, n_frame).  The
    frames are never materialised: one kernel sums the squares of each frame's samples."""

    def __init__(self, sample_rate=22050, ref_duration=0.1, frame_length=2205, hop_length=1102,
                 pad_end=False, pad_value=0, data_format='default', **kwargs):
        super(Energy, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        self.sample_rate = sample_rate
        self.ref_duration = ref_duration
        self.frame_length = frame_length
        self.hop_length = hop_length
        self.pad_end = pad_end
        self.pad_value = pad_value
        self.data_format_str = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self.time_axis = 2 if self.data_format == _CH_FIRST_STR else 1

    def compute_output_shape(self, input_shape):
        """(b, t, ch) -> (b, frame, ch); (b, ch, t) -> (b, ch, frame)"""
        b, c, t = _ffi.dims_of(input_shape, self.data_format)
        n = None
        if t is not None:
            t, fl, hop = int(t), int(self.frame_length), int(self.hop_length)
            n = -(-t // hop) if self.pad_end else max(0, 1 + (t - fl) // hop)
        return _ffi.shape_of(self.data_format, b, c, n)

    def call(self, x):
        if autograd.needs_grad(x):
            return autograd.energy(self, autograd.prep(x, 'float32'))
        return self._forward(x)

    def _scale(self):
        return self.ref_duration / (self.frame_length / self.sample_rate)

    def _forward(self, x):
        return _ffi.energy(_as_waveform(x), self.data_format, self.frame_length, self.hop_length, self.pad_end,
                           self.pad_value, self._scale())

    def get_config(self):
        config = super(Energy, self).get_config()
        config.update({'sample_rate': self.sample_rate, 'ref_duration': self.ref_duration,
                       'frame_length': self.frame_length, 'hop_length': self.hop_length,
                       'pad_end': self.pad_end, 'pad_value': self.pad_value,
                       'data_format': self.data_format_str})
        return config


@register_keras_serializable(package='Kapre')
class MuLawEncoding(Layer):
    """Mu-law encoding (compression) of an audio signal in [-1, 1] to int32 codes in ``0 .. quantization_channels - 1``
    (reference: signal.py:236-306).  Any shape; the shape does not change.  ``quantization_channels``: 256 for 8 bits.
    Values outside [-1, 1] are not clipped; a NaN sample gives code 0.  The output is an integer tensor without ``grad_fn``."""

    def __init__(self, quantization_channels, **kwargs):
        super(MuLawEncoding, self).__init__(**kwargs)
        if quantization_channels < 2:
            raise ValueError(
                f'quantization_channels must be at least 2, got: {quantization_channels}'
            )
        if quantization_channels > 65536:
            raise ValueError(
                f'quantization_channels must be <= 65536, got: {quantization_channels}'
            )
        self.quantization_channels = quantization_channels

    def compute_output_shape(self, input_shape):
        return tuple(input_shape)

    def call(self, x):
        return backend.mu_law_encoding(x, self.quantization_channels)

    def get_config(self):
        config = super(MuLawEncoding, self).get_config()
        config.update({'quantization_channels': self.quantization_channels})
        return config


@register_keras_serializable(package='Kapre')
class MuLawDecoding(Layer):
    """Mu-law decoding (expansion) of mu-law codes to float32 in [-1, 1] (reference: signal.py:309-361).  Any shape; int32
    or float32 codes (other dtypes are converted first).  As upstream the constructor validates nothing; a value outside
    ``2 .. 65536`` is refused by the library at call time.  Float codes that ``requires_grad`` are differentiable."""

    def __init__(self, quantization_channels, **kwargs):
        super(MuLawDecoding, self).__init__(**kwargs)
        self.quantization_channels = quantization_channels

    def compute_output_shape(self, input_shape):
        return tuple(input_shape)

    def call(self, x):
        return backend.mu_law_decoding(x, self.quantization_channels)

    def get_config(self):
        config = super(MuLawDecoding, self).get_config()
        config.update({'quantization_channels': self.quantization_channels})
        return config


def mfcc_matrix(n_mels: int, n_mfccs: int) -> np.ndarray:
    """(n_mels, n_mfccs) float32 matrix of ``tf.signal.mfccs_from_log_mel_spectrograms``:
    unnormalised DCT-II ``2 cos(pi (2n+1) k / (2N))`` scaled by ``rsqrt(2N)`` (HTK convention; the
    reference notes the sqrt(2) difference to librosa's orthonormal DCT in bin 0, signal.py:370-377).
    Built in float64, stored as floatx."""
    n = np.arange(n_mels, dtype=np.float64)
    k = np.arange(min(n_mfccs, n_mels), dtype=np.float64)
    m = 2.0 * np.cos(np.pi * np.outer(2.0 * n + 1.0, k) / (2.0 * n_mels)) / math.sqrt(2.0 * n_mels)
    return m.astype(np.float32)


@register_keras_serializable(package='Kapre')
class LogmelToMFCC(Layer):
    """MFCC from a log-melspectrogram (reference: signal.py:364-447): DCT-II over the mel axis,
    first ``n_mfccs`` coefficients.  (b, time, mel, ch) -> (b, time, n_mfccs, ch) or
    (b, ch, time, mel) -> (b, ch, time, n_mfccs).  The DCT is a (n_mels x n_mfccs) matrix applied
    by the same MFMA GEMM kernel as ApplyFilterbank."""

    def __init__(self, n_mfccs=20, data_format='default', **kwargs):
        super(LogmelToMFCC, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        self.n_mfccs = n_mfccs
        self.data_format_str = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self.permutation = (0, 1, 3, 2) if self.data_format == _CH_LAST_STR else None
        self._consts = _ffi.DeviceConstants()

    def _matrix(self, n_mels, device):
        return self._consts.get(n_mels, device, lambda: mfcc_matrix(n_mels, self.n_mfccs))

    def compute_output_shape(self, input_shape):
        """the mel axis (3 for channels_first, 2 for channels_last) becomes n_mfccs"""
        shape = list(input_shape)
        shape[3 if self.data_format == _CH_FIRST_STR else 2] = int(self.n_mfccs)
        return tuple(shape)

    def call(self, log_melgrams):
        if autograd.needs_grad(log_melgrams):
            x = autograd.prep(log_melgrams, 'float32')
            n_mels = int(_ffi.dims_of(x.shape, self.data_format)[3]) if x.dim() == 4 else 0
            if n_mels:
                mat_t = self._matrix(n_mels, x.device).t().contiguous()      # (n_mfccs, n_mels): the backward GEMM
                return autograd.matrix(self, x, mat_t, self.data_format)
        return self._forward(log_melgrams)

    def _forward(self, log_melgrams):
        import torch

        x = _ffi.as_device(log_melgrams, torch.float32)
        if x.dim() != 4:
            raise ValueError('LogmelToMFCC expects a rank-4 input, got shape %s' % (tuple(x.shape),))
        n_mels = int(_ffi.dims_of(x.shape, self.data_format)[3])
        # (n_mels, min(n_mfccs, n_mels)): the first n_mfccs coefficients, as the slice upstream
        return _ffi.freq_matmul(x, self.data_format, self._matrix(n_mels, x.device))

    def get_config(self):
        config = super(LogmelToMFCC, self).get_config()
        config.update({'n_mfccs': self.n_mfccs, 'data_format': self.data_format_str})
        return config


@register_keras_serializable(package='Kapre')
class Resample(Layer):
    """Sample-rate conversion from ``orig_freq`` to ``new_freq`` (positive integers): band-limited interpolation with a
    Hann-windowed sinc of ``lowpass_filter_width`` zero crossings a side and cutoff ``rolloff`` times the lower Nyquist
    frequency (``backend.resample``).  ``method='polyphase'`` reads a table: any rational ratio whose polyphase table has at
    most 128 taps and 1 MiB -- every pair among 8, 11.025, 16, 22.05, 24, 32, 44.1 and 48 kHz does.  ``method='direct'``
    computes the taps on the device: any pair of rates below 2^31 whose support is at most 128 taps, the same outputs up to
    float32 rounding, at several times the arithmetic.

    (batch, time, ch) -> (batch, ceil(new_freq time / orig_freq), ch) for ``channels_last``;
    (batch, ch, time) -> (batch, ch, ceil(new_freq time / orig_freq)) for ``channels_first``.  numpy or torch, float32 (a
    float64 input raises ``TypeError``).  One launch; differentiable (one more launch of the same kernel).  ``orig_freq ==
    new_freq`` returns its input."""

    def __init__(self, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, data_format='default', method='polyphase',
                 **kwargs):
        super(Resample, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        self._params = backend.resample_parameters(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff = self._params
        self.method, _ = backend.resample_method(method)
        backend.resample_supported(self._params, self.method)        # ValueError for a conversion the library does not support
        self.data_format_str = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self.time_axis = 2 if self.data_format == _CH_FIRST_STR else 1

    def compute_output_shape(self, input_shape):
        """(b, t, ch) -> (b, ceil(new t / orig), ch); (b, ch, t) -> (b, ch, ceil(new t / orig))"""
        b, c, t = _ffi.dims_of(input_shape, self.data_format)
        return _ffi.shape_of(self.data_format, b, c, backend.resample_length(t, self.orig_freq, self.new_freq))

    def call(self, x):
        return backend._resample_run(x, self._params, self.data_format, self.method)

    def get_config(self):
        config = super(Resample, self).get_config()
        config.update({'orig_freq': self.orig_freq, 'new_freq': self.new_freq,
                       'lowpass_filter_width': self.lowpass_filter_width, 'rolloff': self.rolloff,
                       'data_format': self.data_format_str, 'method': self.method})
        return config


@register_keras_serializable(package='Kapre')
class PitchShift(Layer):
    """Pitch shift by ``n_steps`` steps of 1 / ``bins_per_octave`` octave without a change of duration
    (``torchaudio.transforms.PitchShift``, ``librosa.effects.pitch_shift``): ``get_time_stretch_layer(rate, n_fft,
    hop_length)`` with rate = 2 ** (-n_steps / bins_per_octave) -- its windows, its edges --, then a resample from
    orig_freq = int(sample_rate / rate) to ``sample_rate`` with the table-free kernel, cut or zero-extended to the input's
    length inside that launch (``backend.pitch_shift``).  ``n_steps`` is any finite number, positive up, negative down; there
    is one path and no step that raises for the size of a table.  ``hop_length`` defaults to ``n_fft // 4``.

    (batch, time, ch) for ``channels_last``, (batch, ch, time) for ``channels_first``, any channel count; the output has the
    input's shape.  numpy or torch, float32 (a float64 input raises ``TypeError``); fewer than ``n_fft`` samples raise
    ``ValueError``.  ``n_steps = 0`` returns its input and launches nothing.  No gradient: ``TimeStretch`` carries none, so the
    output is detached.  One step for the whole batch; a step drawn per item on the device would need per-item rates and
    ragged lengths through the time stretch and the inverse STFT."""

    def __init__(self, sample_rate, n_steps, bins_per_octave=12, n_fft=2048, hop_length=None, data_format='default', **kwargs):
        from .composed import get_time_stretch_layer
        super(PitchShift, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        self.rate, self.orig_freq = backend.pitch_shift_parameters(sample_rate, n_steps, bins_per_octave)
        self.sample_rate, self.n_steps, self.bins_per_octave = int(sample_rate), n_steps, int(bins_per_octave)
        self._params = None
        if float(n_steps) != 0.0:
            self._params = backend.resample_parameters(self.orig_freq, self.sample_rate, 6, 0.99)
            backend.resample_supported(self._params, 'direct')
        self.n_fft, self.hop_length = n_fft, hop_length
        self._stretch = get_time_stretch_layer(self.rate, n_fft=n_fft, hop_length=hop_length, input_data_format=data_format,
                                               name=self.name + '_stretch')
        self.data_format_str = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self.time_axis = 2 if self.data_format == _CH_FIRST_STR else 1

    def compute_output_shape(self, input_shape):
        """the input's shape"""
        return tuple(input_shape)

    def call(self, x):
        return backend._pitch_shift_run(x, self._stretch, self.n_fft, self._params, self.data_format)

    def get_config(self):
        config = super(PitchShift, self).get_config()
        config.update({'sample_rate': self.sample_rate, 'n_steps': self.n_steps, 'bins_per_octave': self.bins_per_octave,
                       'n_fft': self.n_fft, 'hop_length': self.hop_length, 'data_format': self.data_format_str})
        return config


@register_keras_serializable(package='Kapre')
class LFilter(Layer):
    """A cascade of biquad IIR sections along time over the waveform (``backend.lfilter``): pre-emphasis, DC blockers,
    de-emphasis, shelving and peaking equalisers (``backend.biquad_sos``), loudness weighting.  ``sos``: array-like (n, 6) or
    (6,) in ``scipy.signal``'s row convention (b0, b1, b2, a0, a1, a2), 1 <= n <= 8, every section stable (``ValueError``
    otherwise).  ``zero_phase`` runs every section forward and then every section from the last sample to the
    first, from zero states: ``scipy.signal.sosfiltfilt`` with ``padlen=0`` without its steady-state initial conditions.

    (batch, time, ch) for ``channels_last``, (batch, ch, time) for ``channels_first``; the output has the input's shape.
    numpy or torch, float32 (a float64 input raises ``TypeError``).  The arithmetic is float64 inside the kernel with the
    float64 coefficients: each section's output is the float32 rounding of ``scipy.signal.lfilter`` on the float64 copy of
    its input.  Differentiable with respect to the waveform (the sections in reverse order in the other direction).

    Non-finite input: with t0 the first NaN / Inf sample of a series, every output before t0 (after it, for a pass in
    reverse) equals bit for bit the output of the call in which that sample is 0; from t0 on that series is unspecified when
    a1 or a2 is non-zero (a recurrence does not forget), a pure FIR section is affected at t0 ... t0 + 2 only, and other series
    are never touched."""

    def __init__(self, sos, zero_phase=False, data_format='default', **kwargs):
        super(LFilter, self).__init__(**kwargs)
        backend.validate_data_format_str(data_format)
        self._sections = backend.lfilter_sections(sos)
        rows = np.array(sos, dtype=np.float64)
        self.sos = [[float(v) for v in row] for row in (rows[None, :] if rows.ndim == 1 else rows)]
        self.zero_phase = bool(zero_phase)
        # zero_phase: the whole cascade forward, then the whole cascade from the last sample to the first
        self._plan = tuple((c, r) for r in ((False, True) if self.zero_phase else (False,)) for c in self._sections)
        self.data_format_str = data_format
        self.data_format = backend.resolve_data_format(data_format)
        self.time_axis = 2 if self.data_format == _CH_FIRST_STR else 1

    def compute_output_shape(self, input_shape):
        """the input's shape"""
        return tuple(input_shape)

    def call(self, x):
        return backend._lfilter_run(x, self._plan, self.data_format)

    def get_config(self):
        config = super(LFilter, self).get_config()
        config.update({'sos': [list(row) for row in self.sos], 'zero_phase': self.zero_phase,
                       'data_format': self.data_format_str})
        return config


def _emphasis_coef(coef):
    if isinstance(coef, bool) or np.ndim(coef) != 0 or not isinstance(coef, (int, float, np.integer, np.floating)):
        raise ValueError('coef must be a number, got %r' % (coef,))
    if not abs(float(coef)) < 1.0:
        raise ValueError('|coef| < 1 is required, got %r' % (coef,))
    return float(coef)


@register_keras_serializable(package='Kapre')
class Preemphasis(LFilter):
    """y[t] = x[t] - coef x[t-1] along time (``LFilter`` with the section [1, -coef, 0, 1, 0, 0]: a pure FIR launch)."""

    def __init__(self, coef=0.97, data_format='default', **kwargs):
        self.coef = _emphasis_coef(coef)
        super(Preemphasis, self).__init__([1.0, -self.coef, 0.0, 1.0, 0.0, 0.0], data_format=data_format, **kwargs)

    def get_config(self):
        config = Layer.get_config(self)
        config.update({'coef': self.coef, 'data_format': self.data_format_str})
        return config


@register_keras_serializable(package='Kapre')
class Deemphasis(LFilter):
    """y[t] = x[t] + coef y[t-1] along time, the inverse of ``Preemphasis`` (``LFilter`` with the section
    [1, 0, 0, 1, -coef, 0])."""

    def __init__(self, coef=0.97, data_format='default', **kwargs):
        self.coef = _emphasis_coef(coef)
        super(Deemphasis, self).__init__([1.0, 0.0, 0.0, 1.0, -self.coef, 0.0], data_format=data_format, **kwargs)

    def get_config(self):
        config = Layer.get_config(self)
        config.update({'coef': self.coef, 'data_format': self.data_format_str})
        return config


@register_keras_serializable(package='Kapre')
class Convolve(Layer):
    """Convolution of the waveform with a fixed impulse response along time (``backend.fftconvolve``;
    ``torchaudio.transforms.Convolve``): room, microphone and channel responses, FIR filters of up to 32768 taps.  ``ir``:
    array-like (len,), shared by every item and channel, or (n, len) for batches of exactly n items, item i with ir[i].
    ``mode``: 'full', 'same' (scipy's centring) or 'valid'.  ``block_size``: None for ``backend.convolve_block``'s rule, or one of
    256, 512, 1024.

    (batch, time, ch) -> (batch, time', ch) for ``channels_last``, (batch, ch, time) -> (batch, ch, time') for
    ``channels_first``, time' = time + len - 1, time or time - len + 1.  numpy or torch, float32 (a float64 input raises
    ``TypeError``).  Three launches and a trim; differentiable with respect to the waveform (the same three launches with the
    time-reversed impulse response).  The impulse response is a constant of the layer: it travels in the config and gets no
    gradient."""

    def __init__(self, ir, mode='full', block_size=None, input_data_format='default', **kwargs):
        super(Convolve, self).__init__(**kwargs)
        backend.validate_data_format_str(input_data_format)
        backend.convolve_length(None, 1, mode)                      # ValueError for an unknown mode
        self._plan = backend.ConvolvePlan(ir, block_size)
        self.ir = self._plan.h[0].tolist() if np.ndim(ir) == 1 else self._plan.h.tolist()
        self.mode = mode
        self.block_size = None if block_size is None else int(block_size)
        self.input_data_format_str = input_data_format
        self.input_data_format = backend.resolve_data_format(input_data_format)
        self.time_axis = 2 if self.input_data_format == _CH_FIRST_STR else 1

    def compute_output_shape(self, input_shape):
        """(b, t, ch) -> (b, t', ch); (b, ch, t) -> (b, ch, t') with t' the length ``mode`` keeps"""
        b, c, t = _ffi.dims_of(input_shape, self.input_data_format)
        return _ffi.shape_of(self.input_data_format, b, c, backend.convolve_length(t, self._plan.ir_len, self.mode))

    def call(self, x):
        return backend._convolve_run(x, self._plan, self.input_data_format, self.mode)

    def get_config(self):
        config = super(Convolve, self).get_config()
        config.update({'ir': self.ir, 'mode': self.mode, 'block_size': self.block_size,
                       'input_data_format': self.input_data_format_str})
        return config
