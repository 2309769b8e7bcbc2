"""Backend operations -- host-side mirror of /root/reference/kapre/backend.py for the hot path.

Same names, argument meaning and error behaviour as the reference:
``get_window_fn`` (backend.py:58-100), ``validate_data_format_str`` (:103-123),
``magnitude_to_decibel`` (:126-194), ``filterbank_mel`` (:197-231), ``filterbank_log`` (:234-299),
``mu_law_encoding`` (:302-319), ``mu_law_decoding`` (:322-341).  ``pcen``, ``cmvn``, ``resample``, ``lfilter``, ``fftconvolve`` and ``griffin_lim`` have no counterpart there.

Constants that the reference builds once on the host through TensorFlow/librosa (windows, the mel
and log filterbanks) are built here once on the host in numpy (float64 arithmetic, float32
result, following the published tf.signal / librosa definitions); everything that touches the
signal itself runs in the HIP kernels behind ``kapre_amd._ffi``.
"""
from __future__ import annotations

from typing import Callable, Optional, Union

import numpy as np

from . import _ffi

_CH_FIRST_STR = 'channels_first'
_CH_LAST_STR = 'channels_last'
_CH_DEFAULT_STR = 'default'

# Keras' global image_data_format(); the reference resolves 'default' through it
# (time_frequency.py:142-144) and itself falls back to 'channels_last' (backend.py:36-37).
_IMAGE_DATA_FORMAT = _CH_LAST_STR


def image_data_format() -> str:
    return _IMAGE_DATA_FORMAT


def set_image_data_format(data_format: str) -> None:
    global _IMAGE_DATA_FORMAT
    if data_format not in (_CH_FIRST_STR, _CH_LAST_STR):
        raise ValueError('Unknown data_format: %r' % (data_format,))
    _IMAGE_DATA_FORMAT = data_format


def _get_image_data_format() -> str:
    return image_data_format()


def resolve_data_format(data_format):
    """``'default'`` becomes the global ``image_data_format()``; anything else is returned as it is."""
    return image_data_format() if data_format == _CH_DEFAULT_STR else data_format


def _get_floatx() -> str:
    return 'float32'


# --------------------------------------------------------------------------------------
# windows: tf.signal.*_window(window_length, periodic=True, dtype=float32)
# --------------------------------------------------------------------------------------
# (``dtype``: tf.signal window functions take the dtype of the framed signal; float64 layers ask for float64)
def _raised_cosine_window(window_length: int, a: float, b: float, dtype=np.float32) -> np.ndarray:
    # tf.signal: n = window_length + periodic*even - 1 (periodic only affects even lengths)
    if window_length == 1:
        return np.ones(1, dtype=dtype)
    even = 1 - window_length % 2
    n = float(window_length + even - 1)
    count = np.arange(window_length, dtype=np.float64)
    return (a - b * np.cos(2.0 * np.pi * count / n)).astype(dtype)


def hann_window(window_length: int, dtype=np.float32) -> np.ndarray:
    return _raised_cosine_window(int(window_length), 0.5, 0.5, dtype)


def hamming_window(window_length: int, dtype=np.float32) -> np.ndarray:
    return _raised_cosine_window(int(window_length), 0.54, 0.46, dtype)


def kaiser_window(window_length: int, beta: float = 12.0, dtype=np.float32) -> np.ndarray:
    window_length = int(window_length)
    if window_length == 1:
        return np.ones(1, dtype=dtype)
    halflen = (window_length - 1) / 2.0
    arg = np.arange(window_length, dtype=np.float64) - halflen
    arg = beta * np.sqrt(np.maximum(0.0, 1.0 - (arg / halflen) ** 2))
    return (np.i0(arg) / np.i0(beta)).astype(dtype)


def kaiser_bessel_derived_window(window_length: int, beta: float = 12.0, dtype=np.float32) -> np.ndarray:
    window_length = int(window_length)
    halflen = window_length // 2
    kw = kaiser_window(halflen + 1, beta, dtype=dtype).astype(np.float64)
    csum = np.cumsum(kw)
    half = np.sqrt(csum[:-1] / csum[-1])
    return np.concatenate([half, half[::-1]]).astype(dtype)


def vorbis_window(window_length: int, dtype=np.float32) -> np.ndarray:
    window_length = int(window_length)
    arg = np.arange(window_length, dtype=np.float64) + 0.5
    return np.sin(np.pi / 2.0 * np.sin(np.pi / window_length * arg) ** 2).astype(dtype)


_AVAILABLE_WINDOWS = {
    'hamming_window': hamming_window,
    'hann_window': hann_window,
    'kaiser_bessel_derived_window': kaiser_bessel_derived_window,
    'kaiser_window': kaiser_window,
    'vorbis_window': vorbis_window,
}


def get_window_fn(window_name: Optional[str] = None) -> Callable[[int], np.ndarray]:
    """Return a window function given its name (reference: backend.py:58-100).

    ``None`` -> hann.  Unknown names raise ``NotImplementedError`` like the reference.
    The returned callable maps a window length to a float32 numpy array.
    """
    if window_name is None:
        return hann_window
    if window_name not in _AVAILABLE_WINDOWS:
        raise NotImplementedError(
            'Window name %s is not supported now. Currently, %d windows are'
            'supported - %s'
            % (window_name, len(_AVAILABLE_WINDOWS), ', '.join(_AVAILABLE_WINDOWS.keys()))
        )
    return _AVAILABLE_WINDOWS[window_name]


def window_values(window_fn, length: int, dtype=np.float32) -> np.ndarray:
    """``window_fn(length)`` in ``dtype``: the built-in windows take the dtype (as tf.signal's do); a user
    callable that only accepts the length is evaluated as is and cast."""
    if dtype == np.float32:
        return np.asarray(window_fn(length), dtype=np.float32)
    try:
        return np.asarray(window_fn(length, dtype=dtype), dtype=dtype)
    except TypeError:
        return np.asarray(window_fn(length), dtype=dtype)


def inverse_stft_window_fn(frame_step: int, forward_window_fn: Callable[[int], np.ndarray]):
    """tf.signal.inverse_stft_window_fn (used at time_frequency.py:278-280)."""

    def _fn(frame_length: int, dtype=np.float32) -> np.ndarray:
        fw = np.asarray(window_values(forward_window_fn, frame_length, dtype), dtype=dtype)
        denom = np.square(fw)
        overlaps = -(-frame_length // frame_step)
        denom = np.pad(denom, (0, overlaps * frame_step - frame_length))
        denom = denom.reshape(overlaps, frame_step).sum(0, keepdims=True)
        denom = np.tile(denom, (overlaps, 1)).reshape(overlaps * frame_step)
        with np.errstate(divide='ignore', invalid='ignore'):
            return (fw / denom[:frame_length]).astype(dtype)

    return _fn


def validate_data_format_str(data_format: str) -> None:
    """Reference: backend.py:103-123 (TypeError for non-str, ValueError for unknown values)."""
    if not isinstance(data_format, str):
        raise TypeError(
            f'data_format must be a string, got {type(data_format).__name__}: {data_format}'
        )
    if data_format not in (_CH_DEFAULT_STR, _CH_FIRST_STR, _CH_LAST_STR):
        raise ValueError(
            f'data_format must be one of {[_CH_FIRST_STR, _CH_LAST_STR, _CH_DEFAULT_STR]}, '
            f'got: {data_format!r}'
        )


# --------------------------------------------------------------------------------------
# decibel
# --------------------------------------------------------------------------------------
def magnitude_to_decibel(x, ref_value: float = 1.0, amin: float = 1e-5,
                         dynamic_range: float = 80.0):
    """Decibel scaling on the GPU (reference: backend.py:126-194).

    ``10*log10(max(x, amin)) - 10*log10(max(amin, ref_value))`` clamped from below at
    (per batch item max) - dynamic_range; a rank-1 input is one item.  Raises ``ValueError`` for
    non-positive parameters exactly like the reference (:168-173).
    Accepts a numpy array or torch tensor; returns a float32 torch tensor on the GPU (float64 for a
    float64 input: the TF ops of the reference follow the dtype of their argument).
    """
    if ref_value <= 0:
        raise ValueError(f'ref_value must be positive, got: {ref_value}')
    if amin <= 0:
        raise ValueError(f'amin must be positive, got: {amin}')
    if dynamic_range <= 0:
        raise ValueError(f'dynamic_range must be positive, got: {dynamic_range}')
    import torch

    f64 = _ffi.is_f64(x)            # tf ops compute in the dtype of their input (float64 layers hand in float64)
    xt = _ffi.as_device(x, torch.float64 if f64 else torch.float32)
    return _ffi.mag_to_db(xt, ref_value, amin, dynamic_range)


# --------------------------------------------------------------------------------------
# filterbanks (host constants)
# --------------------------------------------------------------------------------------
def _hz_to_mel(frequencies, htk: bool):
    frequencies = np.asanyarray(frequencies, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + frequencies / 700.0)
    f_sp = 200.0 / 3
    mels = frequencies / f_sp
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    if frequencies.ndim:
        log_t = frequencies >= min_log_hz
        mels[log_t] = min_log_mel + np.log(frequencies[log_t] / min_log_hz) / logstep
    elif frequencies >= min_log_hz:
        mels = min_log_mel + np.log(frequencies / min_log_hz) / logstep
    return mels


def _mel_to_hz(mels, htk: bool):
    mels = np.asanyarray(mels, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (mels / 2595.0) - 1.0)
    f_sp = 200.0 / 3
    freqs = f_sp * mels
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    if mels.ndim:
        log_t = mels >= min_log_mel
        freqs[log_t] = min_log_hz * np.exp(logstep * (mels[log_t] - min_log_mel))
    elif mels >= min_log_mel:
        freqs = min_log_hz * np.exp(logstep * (mels - min_log_mel))
    return freqs


def filterbank_mel(sample_rate: int, n_freq: int, n_mels: int = 128, f_min: float = 0.0,
                   f_max: Optional[float] = None, htk: bool = False,
                   norm: Union[str, int, float, None] = 'slaney') -> np.ndarray:
    """Mel filterbank, shape (n_freq, n_mels), float32 (reference: backend.py:197-231, which
    wraps ``librosa.filters.mel(sr, n_fft=(n_freq-1)*2, ...).astype(floatx).T``)."""
    n_fft = (n_freq - 1) * 2
    if f_max is None:
        f_max = float(sample_rate) / 2
    n_mels = int(n_mels)
    weights = np.zeros((n_mels, int(1 + n_fft // 2)), dtype=np.float32)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sample_rate)
    mel_pts = np.linspace(_hz_to_mel(f_min, htk), _hz_to_mel(f_max, htk), n_mels + 2)
    mel_f = _mel_to_hz(mel_pts, htk)
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    if isinstance(norm, str):
        if norm == 'slaney':
            enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
            weights *= enorm[:, np.newaxis]
        else:
            raise ValueError(f'Unsupported norm={norm}')
    elif norm is not None:
        weights = _normalize(weights, norm=norm, axis=-1)
    return np.ascontiguousarray(weights.astype(_get_floatx()).T)


def _normalize(S: np.ndarray, norm, axis: int) -> np.ndarray:
    """librosa.util.normalize (fill=None): rows with norm below `tiny` are left unscaled."""
    mag = np.abs(S).astype(float)          # librosa computes the norm in float64
    if norm == np.inf:
        length = np.max(mag, axis=axis, keepdims=True)
    elif norm > 0:
        length = np.sum(mag ** norm, axis=axis, keepdims=True) ** (1.0 / norm)
    else:
        raise ValueError(f'Unsupported norm: {norm!r}')
    length = np.where(length < np.finfo(S.dtype).tiny, 1.0, length)
    return (S / length).astype(S.dtype)    # Snorm = np.empty_like(S); Snorm[:] = S / length


def filterbank_log(sample_rate: int, n_freq: int, n_bins: int = 84, bins_per_octave: int = 12,
                   f_min: Optional[float] = None, spread: float = 0.125) -> np.ndarray:
    """Log-frequency filterbank, shape (n_freq, n_bins), float32 (reference: backend.py:234-299)."""
    if f_min is None:
        f_min = 32.70319566
    f_max = f_min * 2 ** (n_bins / bins_per_octave)
    if f_max > sample_rate // 2:
        raise RuntimeError(
            'Maximum frequency of log filterbank should be lower or equal to the maximum'
            'frequency of the input (defined by its sample rate), '
            'but f_max=%f and maximum frequency is %f. \n'
            'Fix it by reducing n_bins, increasing bins_per_octave and/or reducing f_min.\n'
            'You can also do it by increasing sample_rate but it means you need to upsample'
            'the input audio data, too.' % (f_max, sample_rate)
        )
    sigma = float(spread) / bins_per_octave
    basis = np.zeros((n_bins, n_freq))
    fft_freqs = np.fft.rfftfreq(n=(n_freq - 1) * 2, d=1.0 / sample_rate)
    log_freqs = np.log2(fft_freqs[1:])
    for i in range(n_bins):
        c_freq = f_min * (2.0 ** (float(i) / bins_per_octave))
        basis[i, 1:] = np.exp(
            -0.5 * ((log_freqs - np.log2(c_freq)) / sigma) ** 2 - np.log2(sigma) - log_freqs
        )
    basis = _normalize(basis, norm=1, axis=1)
    return np.ascontiguousarray(basis.astype(_get_floatx()).T)


# --------------------------------------------------------------------------------------
# mu-law companding
# --------------------------------------------------------------------------------------
def _is_float(x) -> bool:
    import torch

    if isinstance(x, torch.Tensor):
        return x.is_floating_point()
    return np.issubdtype(np.asarray(x).dtype, np.floating)


def mu_law_encoding(signal, quantization_channels: int):
    """Mu-law compression on the GPU (reference: backend.py:302-319): a signal scaled to [-1, 1] becomes int32 codes in
    ``0 .. quantization_channels - 1``.  Any shape, numpy array or torch tensor; computed in float32.  Values outside
    [-1, 1] are not clipped (the formula as it stands, as TensorFlow); a NaN gives code 0.  The result carries no gradient."""
    import torch

    x = signal.detach() if isinstance(signal, torch.Tensor) else signal
    return _ffi.mu_law_encode(_ffi.as_device(x, torch.float32), quantization_channels)


def mu_law_decoding(signal_mu, quantization_channels: int):
    """Mu-law expansion on the GPU (reference: backend.py:322-341): float32 of the shape of ``signal_mu``.  int32 and
    float32 codes have kernels of their own; other integer dtypes are converted to int32, other float dtypes to float32,
    first.  A float tensor that ``requires_grad`` gets a ``grad_fn`` (kapre_amd/autograd.py)."""
    import torch

    from . import autograd
    if autograd.needs_grad(signal_mu):
        return autograd.mu_law_decode(autograd.prep(signal_mu, 'float32'), quantization_channels)
    dtype = torch.float32 if _is_float(signal_mu) else torch.int32
    return _ffi.mu_law_decode(_ffi.as_device(signal_mu, dtype), quantization_channels)


# --------------------------------------------------------------------------------------
# PCEN
# --------------------------------------------------------------------------------------
def pcen_parameters(s, alpha, delta, r, eps):
    """Validated PCEN parameters: ``s``, ``alpha``, ``delta``, ``r`` as float32 arrays of shape () or (n,), ``eps`` as a
    float.  ``ValueError`` unless 0 < s <= 1, alpha >= 0, delta > 0, r > 0, eps > 0 (and each is a scalar or 1-D)."""
    out = []
    for name, value, ok, rule in (('s', s, lambda v: (v > 0) & (v <= 1), '0 < s <= 1'),
                                  ('alpha', alpha, lambda v: v >= 0, 'alpha >= 0'),
                                  ('delta', delta, lambda v: v > 0, 'delta > 0'),
                                  ('r', r, lambda v: v > 0, 'r > 0')):
        v = np.asarray(value, dtype=np.float64)
        if v.ndim > 1 or v.size == 0:
            raise ValueError('PCEN: %s must be a scalar or a 1-D array with one value per band, got shape %s' % (name, v.shape))
        v32 = v.astype(np.float32)
        if not (np.all(ok(v)) and np.all(ok(v32))):          # (NaN fails every rule; so does a value float32 rounds out of range)
            raise ValueError('PCEN: %s is required, got %s = %r' % (rule, name, value))
        out.append(v32)
    if np.ndim(eps) != 0 or not float(np.float32(eps)) > 0:
        raise ValueError('PCEN: eps must be a positive scalar, got %r' % (eps,))
    return out[0], out[1], out[2], out[3], float(eps)


def pcen_band_table(params, n_bands: int) -> np.ndarray:
    """The (4, n_bands) float32 table (rows s, alpha, delta, r) the kernel reads: scalars repeated, vectors checked against
    ``n_bands`` (``ValueError``)."""
    table = np.empty((4, n_bands), dtype=np.float32)
    for row, (name, v) in enumerate(zip(('s', 'alpha', 'delta', 'r'), params)):
        if v.ndim == 1 and v.shape[0] != n_bands:
            raise ValueError('PCEN: %s has %d values, the input has %d bands' % (name, v.shape[0], n_bands))
        table[row] = v
    return table


def _pcen_run(x, table_of, eps, data_format, tensors=None):
    """PCEN of ``x`` (rank 4); ``table_of(n_bands, device)``: the device copy of ``pcen_band_table``.  ``tensors``: for each of
    s, alpha, delta, r either None or a float32 torch tensor of shape () or (n_bands,) that takes the table row's place; the
    call is recorded for autograd when ``x`` or one of them requires grad."""
    import torch

    from . import autograd
    x, grad = autograd.intake(x, 4, 'float32', 'PCEN expects a rank-4 input, got shape %s', NotImplementedError,
                              'PCEN has float32 kernels only; got a float64 input (cast it to float32)')
    tensors = tuple(tensors) if tensors is not None else (None,) * 4
    grad = grad or any(autograd.needs_grad(t) for t in tensors)
    n_bands = int(x.shape[2] if data_format == _CH_LAST_STR else x.shape[3])
    params = list(table_of(n_bands, x.device)) if n_bands > 0 else [None] * 4
    for i, (name, t) in enumerate(zip(('s', 'alpha', 'delta', 'r'), tensors)):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.dim() > 1 or (t.dim() == 1 and t.shape[0] != n_bands):
            raise ValueError('PCEN: the tensor %s must be float32 of shape () or (%d,), got %s of shape %s'
                             % (name, n_bands, t.dtype, tuple(t.shape)))
        if t.device != x.device:
            raise ValueError('PCEN: the tensor %s is on %s, the input on %s' % (name, t.device, x.device))
        # (torch ops, recorded: the gradient of a 0-d tensor arrives summed over the bands)
        params[i] = (t.expand(n_bands) if t.dim() == 0 else t).contiguous() if n_bands > 0 else None
    if grad:
        return autograd.pcen(x, data_format, tuple(params), eps)
    return _ffi.pcen(x, data_format, tuple(params), eps)


def pcen(x, s=0.025, alpha=0.98, delta=2.0, r=0.5, eps=1e-6, data_format='default'):
    """Per-channel energy normalisation (Wang et al. 2017) of a non-negative spectrogram batch on the GPU:
    (b, time, freq, ch) for ``channels_last``, (b, ch, time, freq) for ``channels_first``; float32 out, same shape.

        S[0] = x[0], S[t] = (1 - s) S[t-1] + s x[t];   y[t] = (x[t] (eps + S[t])^-alpha + delta)^r - delta^r

    ``s``, ``alpha``, ``delta``, ``r``: a scalar or one value per frequency band.  One kernel, one pass over ``x``.  A tensor
    that ``requires_grad`` gets a ``grad_fn``.

    Each of the four may also be a float32 torch tensor on ``x``'s device, of shape () or (n_bands,): a learned parameter.  If it
    requires grad, the output has a ``grad_fn`` (also when ``x`` does not) and ``backward()`` fills its ``.grad`` -- summed over
    the bands for a 0-d tensor -- with one more launch pair (kpr_pcen_bwd_params_f32), which skips the input gradient when ``x``
    needs none.  The shapes of tensors are checked, their values are not (that would read device memory on the host): the
    caller keeps 0 < s <= 1, alpha >= 0, delta > 0, r > 0, e.g. by clamping after each optimiser step (``PCEN.constrain_``)."""
    import torch

    validate_data_format_str(data_format)
    given = (s, alpha, delta, r)
    tensors = tuple(v if isinstance(v, torch.Tensor) else None for v in given)
    # (a tensor's place in the table is overwritten: any valid number stands in for it in the validation)
    numbers = [d if t is not None else v for v, t, d in zip(given, tensors, (0.025, 0.98, 2.0, 0.5))]
    *params, eps = pcen_parameters(*numbers, eps)
    fmt = resolve_data_format(data_format)
    return _pcen_run(x, lambda n, device: torch.from_numpy(pcen_band_table(params, n)).to(device), eps, fmt,
                     tensors if any(t is not None for t in tensors) else None)


# --------------------------------------------------------------------------------------
# CMVN
# --------------------------------------------------------------------------------------
def cmvn_parameters(norm_vars, eps):
    """Validated (norm_vars, eps): a bool and a finite float >= 0 (``ValueError``)."""
    if not isinstance(norm_vars, (bool, np.bool_)):
        raise ValueError('CMVN: norm_vars must be a bool, got %r' % (norm_vars,))
    if isinstance(eps, bool) or np.ndim(eps) != 0 or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise ValueError('CMVN: eps must be a scalar >= 0, got %r' % (eps,))
    e32 = float(np.float32(eps))
    if not (np.isfinite(e32) and e32 >= 0 and float(eps) >= 0):
        raise ValueError('CMVN: eps must be finite and >= 0, got %r' % (eps,))
    return bool(norm_vars), float(eps)


def _cmvn_run(x, norm_vars, eps, data_format):
    """CMVN of ``x`` (rank 4) in the resolved ``data_format``; recorded for autograd when ``x`` requires grad."""
    from . import autograd
    x, grad = autograd.intake(x, 4, 'float32', 'CMVN expects a rank-4 input, got shape %s', NotImplementedError,
                              'CMVN has float32 kernels only; got a float64 input (cast it to float32)')
    return (autograd.cmvn if grad else _ffi.cmvn)(x, data_format, norm_vars, eps)


def cmvn(x, norm_vars=True, eps=1e-5, data_format='default'):
    """Per-utterance mean and variance normalisation along time (Kaldi's ``apply-cmvn --norm-vars``, ESPnet's ``UtteranceMVN``)
    of a spectrogram batch on the GPU: (b, time, freq, ch) for ``channels_last``, (b, ch, time, freq) for ``channels_first``;
    float32 out, same shape.  For every (batch item, channel, band), over its n frames:

        d[t] = x[t] - x[0];  m = mean(d);  c[t] = d[t] - m;  y[t] = c[t] / sqrt(mean(c^2) + eps)    (``norm_vars``)
                                                                y[t] = c[t]                            (else)

    The variance is the population variance.  A constant series gives exactly +0.0.  One kernel, one pass over ``x`` up to
    ``_ffi.cmvn_plan``'s resident frame count (128), two reads beyond.  A tensor that ``requires_grad`` gets a ``grad_fn``."""
    validate_data_format_str(data_format)
    norm_vars, eps = cmvn_parameters(norm_vars, eps)
    fmt = resolve_data_format(data_format)
    return _cmvn_run(x, norm_vars, eps, fmt)


# --------------------------------------------------------------------------------------
# sample-rate conversion
# --------------------------------------------------------------------------------------
def resample_parameters(orig_freq, new_freq, lowpass_filter_width, rolloff):
    """Validated (orig_freq, new_freq, lowpass_filter_width, rolloff): positive integer rates, lowpass_filter_width >= 1,
    0 < rolloff <= 1 (``ValueError``)."""
    for name, v in (('orig_freq', orig_freq), ('new_freq', new_freq)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
            raise ValueError('resample: %s must be a positive integer, got %r' % (name, v))
    if (isinstance(lowpass_filter_width, bool) or not isinstance(lowpass_filter_width, (int, np.integer))
            or lowpass_filter_width < 1):
        raise ValueError('resample: lowpass_filter_width must be an integer >= 1, got %r' % (lowpass_filter_width,))
    if np.ndim(rolloff) != 0 or not 0.0 < float(rolloff) <= 1.0:
        raise ValueError('resample: 0 < rolloff <= 1 is required, got %r' % (rolloff,))
    if max(int(orig_freq), int(new_freq)) >= 2 ** 31:
        raise ValueError('resample: the rates must be below 2^31, got %r and %r' % (orig_freq, new_freq))
    return int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff)


def resample_length(t, orig_freq: int, new_freq: int):
    """ceil(new t / orig) with the rates reduced by their gcd; ``None`` stays ``None``."""
    if t is None:
        return None
    g = int(np.gcd(orig_freq, new_freq))
    orig, new = orig_freq // g, new_freq // g
    return -(-new * int(t) // orig)


_RESAMPLE_SUPPORTED = set()          # parameter tuples whose tables kpr_resample_table_size has accepted
_RESAMPLE_DIRECT_SUPPORTED = set()   # parameter tuples whose tap counts kpr_resample_direct_plan has accepted
RESAMPLE_METHODS = ('polyphase', 'direct')


def resample_method(method, length=None):
    """Validated (method, length): ``method`` is 'polyphase' (the table kernel) or 'direct' (taps computed on the device, any
    pair of rates); ``length``, for 'direct' only, is ``None`` or an integer >= 0 that replaces the natural output length
    (``ValueError``)."""
    if method not in RESAMPLE_METHODS:
        raise ValueError("resample: method must be 'polyphase' or 'direct', got %r" % (method,))
    if length is not None:
        if method != 'direct':
            raise ValueError("resample: length is for method='direct' only, got method=%r" % (method,))
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 0:
            raise ValueError('resample: length must be None or an integer >= 0, got %r' % (length,))
        length = int(length)
    return method, length


def resample_supported(params, method):
    """``ValueError`` for a conversion that ``method`` does not support (an O(n_phases) walk on the host for 'polyphase', a
    formula for 'direct'): once per conversion."""
    seen = _RESAMPLE_DIRECT_SUPPORTED if method == 'direct' else _RESAMPLE_SUPPORTED
    if params in seen or (method != 'direct' and params[0] == params[1]):
        return
    for adjoint in (False, True):
        if method == 'direct':
            _ffi.resample_direct_plan(*params, adjoint)
        else:
            _ffi.resample_table_size(*params, adjoint)
    seen.add(params)


def _resample_run(x, params, fmt, method='polyphase', length=None):
    """``x`` (rank 3) through the conversion ``params`` = resample_parameters(...); ``fmt`` is resolved, ``method`` and
    ``length`` are validated."""
    from . import autograd
    autograd.refuse(x, 3, 'resample expects a rank-3 waveform batch, got shape %s', TypeError,
                    'resample has float32 kernels only; got a float64 input (cast it to float32)')
    t = _ffi.dims_of(x.shape, fmt)[2]
    if params[0] == params[1] and (length is None or length == t):
        return x                                                     # nothing to convert, nothing launched
    x, grad = autograd.to_device(x, 'float32')
    out_len = resample_length(t, params[0], params[1]) if length is None else length
    if method == 'direct':
        if grad:
            return autograd.resample_direct(x, fmt, params, out_len)
        return _ffi.resample_direct(x, fmt, params, False, out_len)
    forward, adjoint = _ffi.resample_plans(*params, x.device)
    if grad:
        return autograd.resample(x, fmt, forward, adjoint, out_len)
    return _ffi.resample(x, fmt, forward, out_len)


def resample(x, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, data_format='default', method='polyphase',
             length=None):
    """Sample-rate conversion of a waveform batch on the GPU by the rational ratio new_freq / orig_freq: band-limited
    interpolation with a Hann-windowed sinc (the "sinc_interp_hann" method).  (b, time, ch) for ``channels_last``,
    (b, ch, time) for ``channels_first``; float32 out with ceil(new_freq time / orig_freq) samples.

        h(tau) = (base / orig) sinc(base tau) cos^2(pi base tau / (2 L)) for |base tau| < L,   y[m] = sum_n x[n] h(n / orig - m / new)

    with the rates reduced by their gcd, base = rolloff min(orig, new), L = lowpass_filter_width.  One kernel launch; a
    tensor that ``requires_grad`` gets a ``grad_fn`` whose backward is one launch of the same kernel in its adjoint form.
    ``orig_freq == new_freq`` returns ``x`` itself (with ``length`` None or the input's).  ``TypeError`` for a float64 input.

    ``method='polyphase'`` reads a table of new / gcd rows: ``ValueError`` for a ratio whose table the library does not
    support (more than 128 taps or 1 MiB).  ``method='direct'`` computes the taps on the device from an exact integer
    position: any pair of rates below 2^31 whose support is at most 128 taps, the same outputs up to float32 rounding
    (DESIGN 4.20), at several times the arithmetic.  ``length`` (``'direct'`` only) replaces the natural output length:
    an index past it is the same sum -- the filter's tail, then exact zeros."""
    validate_data_format_str(data_format)
    params = resample_parameters(orig_freq, new_freq, lowpass_filter_width, rolloff)
    method, length = resample_method(method, length)
    resample_supported(params, method)
    fmt = resolve_data_format(data_format)
    return _resample_run(x, params, fmt, method, length)


# --------------------------------------------------------------------------------------
# pitch shifting
# --------------------------------------------------------------------------------------
def pitch_shift_parameters(sample_rate, n_steps, bins_per_octave=12):
    """(rate, orig_freq) of a shift by ``n_steps`` steps of 1 / ``bins_per_octave`` octave at ``sample_rate``:
    rate = 2 ** (-n_steps / bins_per_octave) in float64, the factor of the time stretch, and orig_freq =
    int(sample_rate / rate), the rate the stretched signal is resampled from (``torchaudio``'s truncation).  ``n_steps`` is a
    finite number (a float is allowed, a bool is not); ``n_steps != 0`` with orig_freq == sample_rate is a ``ValueError``: the
    shift is too small to represent at that rate."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or sample_rate <= 0:
        raise ValueError('PitchShift: sample_rate must be a positive integer, got %r' % (sample_rate,))
    if (isinstance(bins_per_octave, bool) or not isinstance(bins_per_octave, (int, np.integer)) or bins_per_octave < 1):
        raise ValueError('PitchShift: bins_per_octave must be an integer >= 1, got %r' % (bins_per_octave,))
    if (isinstance(n_steps, (bool, np.bool_)) or not isinstance(n_steps, (int, float, np.integer, np.floating))
            or not np.isfinite(float(n_steps))):
        raise ValueError('PitchShift: n_steps must be a finite number, got %r' % (n_steps,))
    rate = 2.0 ** (-float(n_steps) / int(bins_per_octave))
    if not (np.isfinite(rate) and rate > 0.0 and int(sample_rate) / rate < 2.0 ** 31):
        raise ValueError('PitchShift: n_steps = %r at %d Hz gives no rate below 2^31' % (n_steps, sample_rate))
    orig_freq = int(int(sample_rate) / rate)
    if orig_freq < 1:
        raise ValueError('PitchShift: n_steps = %r at %d Hz gives no positive rate' % (n_steps, sample_rate))
    if float(n_steps) != 0.0 and orig_freq == int(sample_rate):
        raise ValueError('PitchShift: n_steps = %r is too small a shift to represent at %d Hz' % (n_steps, sample_rate))
    return rate, orig_freq


def _pitch_shift_run(x, stretch, n_fft, params, fmt):
    """``x`` through the time stretch ``stretch`` (``get_time_stretch_layer`` of ``n_fft``; a callable that returns it is
    called when it is needed) and the table-free resampler ``params`` back to the input's length; ``params`` None is the shift
    by zero steps."""
    import torch
    from . import autograd
    autograd.refuse(x, 3, 'PitchShift expects a rank-3 waveform batch, got shape %s', TypeError,
                    'PitchShift has float32 kernels only; got a float64 input (cast it to float32)')
    if params is None:
        return x                                                     # nothing to shift, nothing launched
    t = _ffi.dims_of(x.shape, fmt)[2]
    if t < n_fft:
        raise ValueError('PitchShift: %d samples give no frame of n_fft = %d' % (t, n_fft))
    x = _ffi.as_device(x.detach() if isinstance(x, torch.Tensor) else x, torch.float32)
    from .keras_shim import Layer
    if not isinstance(stretch, Layer):
        stretch = stretch()
    return _ffi.resample_direct(stretch(x).detach().contiguous(), fmt, params, False, t)


_PITCH_SHIFT_CHAINS = {}             # (rate, n_fft, hop_length, data_format) -> get_time_stretch_layer(...), the last 16 used


def _pitch_shift_chain(rate, n_fft, hop_length, data_format):
    """the time-stretch chain of ``pitch_shift``, built once per parameter set (its layers keep their device constants)"""
    from . import composed
    key = (rate, n_fft, hop_length, data_format)
    chain = _PITCH_SHIFT_CHAINS.pop(key, None)
    if chain is None:
        chain = composed.get_time_stretch_layer(rate, n_fft=n_fft, hop_length=hop_length, input_data_format=data_format)
        while len(_PITCH_SHIFT_CHAINS) >= 16:
            _PITCH_SHIFT_CHAINS.pop(next(iter(_PITCH_SHIFT_CHAINS)))
    _PITCH_SHIFT_CHAINS[key] = chain                                 # (most recently used last)
    return chain


def pitch_shift(x, sample_rate, n_steps, bins_per_octave=12, n_fft=2048, hop_length=None, data_format='default'):
    """Pitch shift of a waveform batch by ``n_steps`` steps of 1 / ``bins_per_octave`` octave without a change of duration
    (``kapre_amd.PitchShift`` as a function; ``torchaudio.transforms.PitchShift``, ``librosa.effects.pitch_shift``):
    ``get_time_stretch_layer(rate, n_fft, hop_length)`` with rate = 2 ** (-n_steps / bins_per_octave), then
    ``resample(orig_freq -> sample_rate, method='direct', length=time)`` with orig_freq = int(sample_rate / rate).  The
    output has the input's shape and carries no ``grad_fn`` (the time stretch has none).  ``n_steps = 0`` returns ``x``
    itself.  ``ValueError`` for fewer than ``n_fft`` samples, ``TypeError`` for a float64 input."""
    validate_data_format_str(data_format)
    rate, orig_freq = pitch_shift_parameters(sample_rate, n_steps, bins_per_octave)
    fmt = resolve_data_format(data_format)
    params = None
    if float(n_steps) != 0.0:
        params = resample_parameters(orig_freq, int(sample_rate), 6, 0.99)
        resample_supported(params, 'direct')
    if isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or n_fft < 1:
        raise ValueError('PitchShift: n_fft must be a positive integer, got %r' % (n_fft,))
    return _pitch_shift_run(x, lambda: _pitch_shift_chain(rate, int(n_fft), hop_length, data_format), int(n_fft), params, fmt)


# --------------------------------------------------------------------------------------
# biquad IIR filtering
# --------------------------------------------------------------------------------------
LFILTER_MAX_SECTIONS = 8
BIQUAD_KINDS = ('lowpass', 'highpass', 'bandpass', 'notch', 'allpass', 'peaking', 'lowshelf', 'highshelf')


def lfilter_sections(sos):
    """Validated second-order sections: ``sos`` is array-like (n, 6) or (6,) in scipy's row convention (b0, b1, b2, a0, a1, a2)
    with 1 <= n <= 8 -> a tuple of n tuples (b0, b1, b2, a1, a2) of Python floats, divided by a0 in float64.  ``ValueError``
    for another shape, a value that is not finite, a0 == 0, or (a1, a2) outside the stability triangle |a2| < 1,
    |a1| < 1 + a2."""
    try:
        s = np.array(sos, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('lfilter: sos must be array-like of shape (n, 6) or (6,), got %r' % (sos,))
    if s.ndim == 1:
        s = s[None, :]
    if s.ndim != 2 or s.shape[1] != 6 or not 1 <= s.shape[0] <= LFILTER_MAX_SECTIONS:
        raise ValueError('lfilter: sos must have shape (n, 6) or (6,) with 1 <= n <= %d, got shape %s'
                         % (LFILTER_MAX_SECTIONS, tuple(np.shape(sos))))
    if not np.all(np.isfinite(s)):
        raise ValueError('lfilter: every coefficient must be finite, got %r' % (s.tolist(),))
    out = []
    for i, row in enumerate(s):
        if row[3] == 0.0:
            raise ValueError('lfilter: section %d has a0 = 0' % i)
        b0, b1, b2, a1, a2 = (float(v) for v in np.concatenate([row[:3], row[4:]]) / row[3])
        if not (abs(a2) < 1.0 and abs(a1) < 1.0 + a2):
            raise ValueError('lfilter: section %d is not stable: a1 = %r, a2 = %r lie outside the triangle |a2| < 1, '
                             '|a1| < 1 + a2' % (i, a1, a2))
        out.append((b0, b1, b2, a1, a2))
    return tuple(out)


def sos_from_ba(b, a):
    """One section (1, 6) in scipy's convention from transfer-function coefficients of order <= 2 (``b`` and ``a`` of one to
    three values, padded with zeros), float64."""
    b, a = np.atleast_1d(np.asarray(b, dtype=np.float64)), np.atleast_1d(np.asarray(a, dtype=np.float64))
    if b.ndim != 1 or a.ndim != 1 or not 1 <= b.size <= 3 or not 1 <= a.size <= 3:
        raise ValueError('sos_from_ba: b and a hold one to three coefficients each (order <= 2), got %d and %d'
                         % (b.size, a.size))
    row = np.zeros((1, 6), dtype=np.float64)
    row[0, :b.size] = b
    row[0, 3:3 + a.size] = a
    return row


def biquad_sos(kind, sample_rate, freq, q=0.7071067811865476, gain_db=0.0):
    """One biquad section (1, 6) in scipy's convention, normalised to a0 = 1, from the RBJ audio-EQ-cookbook formulas, in float64 -- the formulas
    behind ``torchaudio.functional.*_biquad``.  ``kind``: 'lowpass', 'highpass', 'bandpass' (constant 0 dB peak gain), 'notch',
    'allpass', 'peaking', 'lowshelf', 'highshelf'; ``gain_db`` is read by the last three.  0 < freq < sample_rate / 2 and
    q > 0 (``ValueError``)."""
    if kind not in BIQUAD_KINDS:
        raise ValueError('biquad_sos: kind must be one of %s, got %r' % (', '.join(BIQUAD_KINDS), kind))
    for name, v in (('sample_rate', sample_rate), ('freq', freq), ('q', q), ('gain_db', gain_db)):
        if isinstance(v, bool) or np.ndim(v) != 0 or not np.isfinite(float(v)):
            raise ValueError('biquad_sos: %s must be a finite number, got %r' % (name, v))
    fs, f, q, gain_db = float(sample_rate), float(freq), float(q), float(gain_db)
    if not (fs > 0.0 and 0.0 < f < 0.5 * fs):
        raise ValueError('biquad_sos: 0 < freq < sample_rate / 2 is required, got freq %r at %r' % (freq, sample_rate))
    if not q > 0.0:
        raise ValueError('biquad_sos: q must be positive, got %r' % (q,))
    w0 = 2.0 * np.pi * f / fs
    cw, alpha = float(np.cos(w0)), float(np.sin(w0)) / (2.0 * q)
    A = 10.0 ** (gain_db / 40.0)
    if kind == 'lowpass':
        b, a = [(1 - cw) / 2, 1 - cw, (1 - cw) / 2], [1 + alpha, -2 * cw, 1 - alpha]
    elif kind == 'highpass':
        b, a = [(1 + cw) / 2, -(1 + cw), (1 + cw) / 2], [1 + alpha, -2 * cw, 1 - alpha]
    elif kind == 'bandpass':
        b, a = [alpha, 0.0, -alpha], [1 + alpha, -2 * cw, 1 - alpha]
    elif kind == 'notch':
        b, a = [1.0, -2 * cw, 1.0], [1 + alpha, -2 * cw, 1 - alpha]
    elif kind == 'allpass':
        b, a = [1 - alpha, -2 * cw, 1 + alpha], [1 + alpha, -2 * cw, 1 - alpha]
    elif kind == 'peaking':
        b, a = [1 + alpha * A, -2 * cw, 1 - alpha * A], [1 + alpha / A, -2 * cw, 1 - alpha / A]
    else:
        r = 2.0 * np.sqrt(A) * alpha
        if kind == 'lowshelf':
            b = [A * ((A + 1) - (A - 1) * cw + r), 2 * A * ((A - 1) - (A + 1) * cw), A * ((A + 1) - (A - 1) * cw - r)]
            a = [(A + 1) + (A - 1) * cw + r, -2 * ((A - 1) + (A + 1) * cw), (A + 1) + (A - 1) * cw - r]
        else:
            b = [A * ((A + 1) + (A - 1) * cw + r), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - r)]
            a = [(A + 1) - (A - 1) * cw + r, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - r]
    return np.array([b + a], dtype=np.float64) / a[0]                  # a0 = 1, as scipy.signal's designs


def _lfilter_run(x, plan, fmt):
    """``x`` (rank 3) through the launches ``plan`` = ((coef, reverse), ...); ``fmt`` is resolved."""
    from . import autograd
    x, grad = autograd.intake(x, 3, 'float32', 'lfilter expects a rank-3 waveform batch, got shape %s', TypeError,
                              'lfilter takes float32 waveforms (its arithmetic is float64 inside); got a float64 input '
                              '(cast it to float32)')
    if grad:
        return autograd.lfilter(x, fmt, plan)
    for coef, reverse in plan:
        x = _ffi.lfilter(x, fmt, coef, reverse)
    return x


def lfilter(x, sos, data_format='default', reverse=False):
    """A cascade of biquad sections along time over a waveform batch on the GPU.  (b, time, ch) for ``channels_last``,
    (b, ch, time) for ``channels_first``; float32 in and out, the same shape.  ``sos``: (n, 6) or (6,) rows
    (b0, b1, b2, a0, a1, a2) as in ``scipy.signal``, 1 <= n <= 8; every section, with zero initial state,

        y[t] = (b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2]) / a0

    in float64 arithmetic with the float64 coefficients, rounded to float32 once per section -- the float32 rounding of
    ``scipy.signal.lfilter`` on the float64 copy of the input, section by section.  ``reverse`` runs every section from the
    last sample to the first (the adjoint; forward then reverse is zero-phase filtering).  A tensor that ``requires_grad``
    gets a ``grad_fn`` whose backward is the sections in reverse order in the other direction.  ``ValueError`` for a
    malformed or unstable ``sos`` (``lfilter_sections``), ``TypeError`` for a float64 input."""
    validate_data_format_str(data_format)
    sections = lfilter_sections(sos)
    fmt = resolve_data_format(data_format)
    return _lfilter_run(x, tuple((c, bool(reverse)) for c in sections), fmt)


# --------------------------------------------------------------------------------------
# convolution with an impulse response (partitioned overlap-save)
# --------------------------------------------------------------------------------------
CONVOLVE_BLOCKS = (256, 512, 1024)
CONVOLVE_PREFERRED_PARTITIONS = 16        # the block rule: the smallest block with at most this many partitions
CONVOLVE_MAX_PARTITIONS = 32              # what kpr_spec_fir_c64 takes
CONVOLVE_MAX_IR = CONVOLVE_MAX_PARTITIONS * CONVOLVE_BLOCKS[-1]
CONVOLVE_TABLE_MAX_BYTES = 256 << 20
CONVOLVE_MODES = ('full', 'same', 'valid')


def convolve_block(ir_len, block_size=None):
    """The block length L of the partitioned convolution with an impulse response of ``ir_len`` samples: the smallest of
    256, 512, 1024 that cuts it into at most 16 partitions, else 1024.  ``block_size`` overrides the rule with one of the
    three.  ``ValueError`` for an impulse response longer than 32 * 1024 = 32768 samples, for one that a given
    ``block_size`` cuts into more than 32 partitions, and for any other ``block_size``."""
    n = int(ir_len)
    if n < 1:
        raise ValueError('convolve: the impulse response must hold at least one sample, got %d' % n)
    if n > CONVOLVE_MAX_IR:
        raise ValueError('convolve: an impulse response of %d samples is beyond the limit of %d (%d partitions of %d samples)'
                         % (n, CONVOLVE_MAX_IR, CONVOLVE_MAX_PARTITIONS, CONVOLVE_BLOCKS[-1]))
    if block_size is not None:
        if isinstance(block_size, bool) or not isinstance(block_size, (int, np.integer)) or int(block_size) not in CONVOLVE_BLOCKS:
            raise ValueError('convolve: block_size must be one of %s, got %r' % (CONVOLVE_BLOCKS, block_size))
        L = int(block_size)
        if -(-n // L) > CONVOLVE_MAX_PARTITIONS:
            raise ValueError('convolve: block_size %d cuts an impulse response of %d samples into %d partitions, beyond the '
                             'limit of %d' % (L, n, -(-n // L), CONVOLVE_MAX_PARTITIONS))
        return L
    for L in CONVOLVE_BLOCKS:
        if -(-n // L) <= CONVOLVE_PREFERRED_PARTITIONS:
            return L
    return CONVOLVE_BLOCKS[-1]


def convolve_irs(ir):
    """The impulse responses as a float64 (n_ir, len) host array: ``ir`` is array-like (len,) or (n_ir, len), finite, with
    n_ir >= 1 and len >= 1 (``ValueError``).  They are constants: a torch tensor is read once, on the host, and gets no
    gradient."""
    if hasattr(ir, 'detach'):
        ir = ir.detach().cpu().numpy()
    try:
        h = np.array(ir, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('convolve: ir must be array-like of shape (len,) or (n_ir, len), got %r' % (ir,))
    if h.ndim == 1:
        h = h[None, :]
    if h.ndim != 2 or h.shape[0] < 1 or h.shape[1] < 1:
        raise ValueError('convolve: ir must have shape (len,) or (n_ir, len) with n_ir, len >= 1, got shape %s'
                         % (tuple(np.shape(ir)),))
    if not np.all(np.isfinite(h)):
        raise ValueError('convolve: every sample of ir must be finite')
    return np.ascontiguousarray(h)


def _convolve_table_bytes(n_ir, n_part, L):
    nbytes = n_ir * n_part * (L + 1) * 8
    if nbytes > CONVOLVE_TABLE_MAX_BYTES:
        raise ValueError('convolve: the filter table of %d impulse responses x %d partitions x %d bins takes %d bytes '
                         '(%.1f MiB), beyond the limit of %d MiB' % (n_ir, n_part, L + 1, nbytes, nbytes / 2.0 ** 20,
                                                                     CONVOLVE_TABLE_MAX_BYTES >> 20))
    return nbytes


def convolve_table(ir, L, adjoint=False):
    """The filter table of the partitioned convolution with block length ``L``: complex64 (n_ir, P, L + 1) with
    P = ceil(len / L) and row p of filter i being rfft(ir[i, p L : (p + 1) L], n = 2 L), computed in float64 and rounded
    once.  ``adjoint``: the table of the time-reversed impulse responses (the backward pass).  ``ValueError`` naming the
    size for a table above 256 MiB."""
    L = int(L)
    shape = tuple(np.shape(ir))
    if len(shape) in (1, 2) and all(shape):                            # (refused by its size before anything is copied)
        _convolve_table_bytes(shape[0] if len(shape) == 2 else 1, -(-shape[-1] // L), L)
    h = convolve_irs(ir)
    n_ir, n = h.shape
    P = -(-n // L)
    if adjoint:
        h = h[:, ::-1]
    padded = np.zeros((n_ir, P * L), dtype=np.float64)
    padded[:, :n] = h
    return np.fft.rfft(padded.reshape(n_ir, P, L), n=2 * L, axis=-1).astype(np.complex64)


# the tables, windows and index vectors of every convolution: 32 kept per process (a plan holds on to its own tables)
_CONVOLVE_CONSTS = _ffi.DeviceConstants(max_entries=32)


class ConvolvePlan:
    """What a convolution with fixed impulse responses needs beyond the signal: the float64 host copy of the impulse
    responses, the block length, and the device tables (forward and adjoint), built on first use per device and kept."""

    def __init__(self, ir, block_size=None):
        import hashlib

        self.h = convolve_irs(ir)
        self.n_ir, self.ir_len = self.h.shape
        self.L = convolve_block(self.ir_len, block_size)
        self.n_part = -(-self.ir_len // self.L)
        _convolve_table_bytes(self.n_ir, self.n_part, self.L)
        self._digest = hashlib.sha1(self.h.tobytes()).hexdigest()
        self._tables = _ffi.DeviceConstants()

    def table(self, device, adjoint=False):
        # (the process-wide copy, shared by the plans of equal impulse responses, may be evicted; this plan's stays)
        return self._tables.get(bool(adjoint), device, lambda: _CONVOLVE_CONSTS.get(
            ('table', self._digest, self.h.shape, self.L, bool(adjoint)), device, lambda: convolve_table(self.h, self.L, adjoint)))

    def windows(self, device):
        """(analysis, synthesis): ones(2 L) and [0] * L + [1] * L"""
        L = self.L
        return (_CONVOLVE_CONSTS.get(('ones', L), device, lambda: np.ones(2 * L, dtype=np.float32)),
                _CONVOLVE_CONSTS.get(('tail', L), device, lambda: np.concatenate([np.zeros(L, np.float32), np.ones(L, np.float32)])))


def convolve_length(t, ir_len, mode):
    """Output length of a convolution of ``t`` samples with ``ir_len``: 'full' t + ir_len - 1, 'same' t, 'valid'
    t - ir_len + 1 (``ValueError`` below 1); ``None`` stays ``None``."""
    if mode not in CONVOLVE_MODES:
        raise ValueError("convolve: mode must be one of 'full', 'same', 'valid', got %r" % (mode,))
    if t is None:
        return None
    t = int(t)
    if mode == 'full':
        return t + ir_len - 1
    if mode == 'same':
        return t
    if t - ir_len + 1 < 1:
        raise ValueError("convolve: mode 'valid' needs a signal at least as long as the impulse response, got %d < %d"
                         % (t, ir_len))
    return t - ir_len + 1


def _convolve_offset(ir_len, mode):
    """First sample of the full convolution that ``mode`` keeps ('same': scipy's centring)."""
    return {'full': 0, 'same': (ir_len - 1) // 2, 'valid': ir_len - 1}[mode]


def _convolve_full(x, fmt, plan, idx, adjoint=False):
    """The three launches: every sample of the full convolution of the float32 device waveform ``x`` (or, with ``adjoint``,
    of its convolution with the time-reversed impulse responses) as a view of the inverse launch's output."""
    b, c, t = _ffi.dims_of(x.shape, fmt)
    L = plan.L
    ones, tail = plan.windows(x.device)
    lay = _ffi.layout(fmt)
    geom = _ffi.StftGeom(b, c, t, 2 * L, 2 * L, L, 1, 1, lay, lay)
    k_in = _ffi.num_frames(geom)                                   # ceil((t + L) / L)
    n_full = t + plan.ir_len - 1
    k_out = -(-n_full // L)
    spec = _ffi.stft(x, geom, k_in, ones, _ffi.OUT_COMPLEX)
    spec = _ffi.spec_fir(spec, fmt, plan.table(x.device, adjoint), idx, k_out)
    wave = _ffi.istft(spec, tail, 2 * L, 2 * L, L, fmt, fmt)        # (k_out + 1) L samples; sample n of the convolution is n + L
    return wave.narrow(1 if fmt == _CH_LAST_STR else 2, L, n_full)


def _convolve_index(plan, index, batch, device):
    """The int32 device vector of one filter number per batch item, or None for the one shared impulse response."""
    import torch

    if index is None:
        if plan.n_ir == 1:
            return None
        if plan.n_ir != batch:
            raise ValueError('convolve: %d impulse responses for a batch of %d: without index there must be one, or one per '
                             'batch item' % (plan.n_ir, batch))
        return _CONVOLVE_CONSTS.get(('arange', batch), device, lambda: np.arange(batch, dtype=np.int32))
    if isinstance(index, torch.Tensor) and index.is_cuda:
        if index.dtype != torch.int32 or tuple(index.shape) != (batch,):
            raise ValueError('convolve: a device index must be an int32 tensor of shape (%d,), got %s %s'
                             % (batch, index.dtype, tuple(index.shape)))
        return index.contiguous()
    idx = np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index)
    if idx.shape != (batch,) or idx.dtype.kind not in 'iu':
        raise ValueError('convolve: index must hold one integer per batch item (%d), got shape %s, dtype %s'
                         % (batch, idx.shape, idx.dtype))
    if idx.size and (idx.min() < 0 or idx.max() >= plan.n_ir):
        raise ValueError('convolve: index values must lie in [0, %d), got %d ... %d' % (plan.n_ir, idx.min(), idx.max()))
    return torch.from_numpy(idx.astype(np.int32)).to(device)


def _convolve_run(x, plan, fmt, mode, index=None, out_len=None):
    """``x`` (rank 3) convolved along time through ``plan``; ``fmt`` is resolved.  ``out_len``: keep that many samples from
    the mode's first one (Reverb: the first T of 'full')."""
    from . import autograd
    autograd.refuse(x, 3, 'convolve expects a rank-3 waveform batch, got shape %s', TypeError,
                    'convolve has float32 kernels only; got a float64 input (cast it to float32)')
    b, _, t = _ffi.dims_of(x.shape, fmt)
    n_out = convolve_length(t, plan.ir_len, mode) if out_len is None else int(out_len)
    first = _convolve_offset(plan.ir_len, mode)
    x, grad = autograd.to_device(x, 'float32')
    idx = _convolve_index(plan, index, b, x.device)
    if grad:
        return autograd.convolve(x, fmt, plan, idx, first, n_out)
    return _convolve_full(x, fmt, plan, idx).narrow(1 if fmt == _CH_LAST_STR else 2, first, n_out).contiguous()


def fftconvolve(x, ir, mode='full', index=None, data_format='default', block_size=None):
    """Convolution of a waveform batch with impulse responses on the GPU (``scipy.signal.fftconvolve`` along time,
    ``torchaudio.functional.fftconvolve``): room impulse responses, microphone and channel responses, long FIR filters.
    (b, time, ch) for ``channels_last``, (b, ch, time) for ``channels_first``; float32 in and out.

    ``ir``: (len,), one impulse response for everything; (n_ir, len) with ``index``, one filter number per batch item (host
    integers are validated, an int32 device tensor is taken as it is and clamped by the kernel); or (batch, len) without
    ``index``, item i with ir[i].  The channels of an item share its impulse response.  ``mode``: 'full' (time + len - 1
    samples), 'same' (time samples, scipy's centring: from sample (len - 1) // 2 of 'full') or 'valid' (time - len + 1,
    ``ValueError`` below 1).

    Partitioned overlap-save with block length L = ``convolve_block(len, block_size)``: one STFT launch (n_fft 2 L, hop L,
    rectangular window), the spectral FIR ``kpr_spec_fir_c64`` with the ``convolve_table`` of the impulse responses, one
    inverse-STFT launch, and the trim; nothing is copied to the host.  The impulse responses are constants (no gradient); a
    waveform that ``requires_grad`` gets a ``grad_fn`` whose backward is the same three launches with the table of the
    time-reversed impulse responses.  ``ValueError`` for an impulse response longer than 32768 samples or a table above
    256 MiB, ``TypeError`` for a float64 input."""
    validate_data_format_str(data_format)
    if mode not in CONVOLVE_MODES:
        raise ValueError("convolve: mode must be one of 'full', 'same', 'valid', got %r" % (mode,))
    fmt = resolve_data_format(data_format)
    return _convolve_run(x, ConvolvePlan(ir, block_size), fmt, mode, index)


# --------------------------------------------------------------------------------------
# additive noise at a signal-to-noise ratio
# --------------------------------------------------------------------------------------
def noise_bank(noises):
    """``(bank, lengths)`` of a set of mono noise signals: float32 (n_noise, Lmax), every row zero-padded behind its own
    samples, and int32 (n_noise,).  ``noises``: array-like (L,), (n, L), or a list of 1-D arrays of different lengths.
    ``ValueError`` for an empty set, an empty noise, anything that is not 1-D per noise, and non-finite samples."""
    if hasattr(noises, 'detach'):
        noises = noises.detach().cpu().numpy()
    rows = None
    if not isinstance(noises, np.ndarray):
        try:
            seq = list(noises)
        except TypeError:
            raise ValueError('noise_bank: noises must be array-like, got %r' % (noises,))
        if seq and all(np.ndim(r) == 1 for r in seq):            # a list of signals, each of its own length
            rows = [r.detach().cpu().numpy() if hasattr(r, 'detach') else r for r in seq]
    if rows is None:
        try:
            arr = np.asarray(noises, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('noise_bank: noises must be (L,), (n, L) or a list of 1-D arrays')
        if arr.ndim == 1:
            arr = arr[None, :]
        if arr.ndim != 2:
            raise ValueError('noise_bank: noises must be (L,), (n, L) or a list of 1-D arrays, got shape %s' % (arr.shape,))
        rows = list(arr)
    try:
        rows = [np.asarray(r, dtype=np.float64) for r in rows]
    except (TypeError, ValueError):
        raise ValueError('noise_bank: every noise must be a 1-D array of numbers')
    if not rows or any(r.ndim != 1 or r.size < 1 for r in rows):
        raise ValueError('noise_bank: at least one noise, and at least one sample in every noise, are required')
    if not all(np.all(np.isfinite(r)) for r in rows):
        raise ValueError('noise_bank: every noise sample must be finite')
    lengths = np.array([r.size for r in rows], dtype=np.int32)
    bank = np.zeros((len(rows), int(lengths.max())), dtype=np.float32)
    for k, r in enumerate(rows):
        bank[k, :r.size] = r.astype(np.float32)
    return bank, lengths


class NoisePlan:
    """The host copy of a noise bank and its device copies, made on first use per device and kept."""

    def __init__(self, noises):
        self.bank, self.lengths = noise_bank(noises)
        self.n_noise = int(self.bank.shape[0])
        self._consts = _ffi.DeviceConstants()

    def device(self, device):
        return self._consts.get('bank', device, lambda: (self.bank, self.lengths))


def _noise_column(v, batch, device, what, dtype, np_dtype):
    """One table column: a scalar, a host sequence of ``batch`` values, or a device tensor (batch,) of ``dtype``."""
    import torch

    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dtype != dtype or tuple(v.shape) != (batch,):
            raise ValueError('add_noise: a device %s must be a %s tensor of shape (%d,), got %s %s'
                             % (what, dtype, batch, v.dtype, tuple(v.shape)))
        return v
    a = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
    if a.ndim == 0:
        a = np.full((batch,), a)
    if a.shape != (batch,) or a.dtype.kind not in ('iu' if np_dtype == np.int32 else 'iuf'):
        raise ValueError('add_noise: %s must be a scalar or hold one value per batch item (%d), got shape %s, dtype %s'
                         % (what, batch, a.shape, a.dtype))
    return a.astype(np_dtype)


def noise_table(batch, device, lengths_host, snr_db, index=None, offset=None):
    """The int32 (batch, 4) device table ``kpr_add_noise_f32`` reads -- (index, offset, snr as float32 bits, 0) per item -- from
    scalars, host sequences or device tensors (int32 index / offset, float32 snr).  Host values are validated (``ValueError``:
    an index outside the bank, an offset outside its noise, a non-finite snr); device values are clamped by the kernel."""
    import torch

    idx = _noise_column(0 if index is None else index, batch, device, 'index', torch.int32, np.int32)
    off = _noise_column(0 if offset is None else offset, batch, device, 'offset', torch.int32, np.int32)
    snr = _noise_column(snr_db, batch, device, 'snr_db', torch.float32, np.float32)
    n_noise = len(lengths_host)
    if isinstance(idx, np.ndarray) and idx.size and (idx.min() < 0 or idx.max() >= n_noise):
        raise ValueError('add_noise: index values must lie in [0, %d), got %d ... %d' % (n_noise, idx.min(), idx.max()))
    if isinstance(off, np.ndarray) and off.size:
        limit = np.asarray(lengths_host)[idx] if isinstance(idx, np.ndarray) else np.full((batch,), int(np.max(lengths_host)))
        if off.min() < 0 or np.any(off >= limit):
            raise ValueError('add_noise: every offset must lie in [0, length of its noise)')
    if isinstance(snr, np.ndarray) and not np.all(np.isfinite(snr)):
        raise ValueError('add_noise: snr_db must be finite')
    if all(isinstance(c, np.ndarray) for c in (idx, off, snr)):
        host = np.zeros((batch, 4), dtype=np.int32)
        host[:, 0], host[:, 1], host[:, 2] = idx, off, snr.view(np.int32)
        return torch.from_numpy(host).to(device)
    cols = [torch.from_numpy(c).to(device) if isinstance(c, np.ndarray) else c for c in (idx, off, snr)]
    return torch.stack([cols[0], cols[1], cols[2].view(torch.int32), torch.zeros_like(cols[0])], dim=1).contiguous()


def _add_noise_run(x, plan, table, fmt):
    """(y, stats): ``x`` (float32 device tensor, rank 3) plus the noise that ``table`` names, and the float64 (batch, 4) rows
    (Sx, Sn, g, 0); y is differentiable when ``x`` asks for it."""
    from . import autograd

    bank, lengths = plan.device(x.device)
    if autograd.needs_grad(x):
        return autograd.add_noise(x, fmt, bank, lengths, table)
    return _ffi.add_noise(x, fmt, bank, lengths, table)


def add_noise(x, noise, snr_db, index=None, offset=None, data_format='default'):
    """Noise added to a waveform batch at a signal-to-noise ratio on the GPU (``torchaudio.functional.add_noise`` with a noise
    that tiles circularly).  ``x``: (b, time, ch) for ``channels_last``, (b, ch, time) for ``channels_first``, float32 in and
    out.  ``noise``: what ``noise_bank`` takes, (L,), (n, L) or a list of 1-D arrays.  Item b gets
    ``seg[t] = noise[index[b]][(offset[b] + t) mod L]`` scaled by one gain, so that the ratio of the item's mean power (over
    all its channels) to the mean power of the added noise is ``snr_db[b]`` dB; its channels share the noise and the gain.  A
    silent item or a silent segment is returned as it is.  ``snr_db``: a scalar, a host sequence or a float32 device tensor
    (batch,); ``index`` / ``offset``: host integers, host sequences or int32 device tensors, 0 by default.  Noise and snr are
    constants; a waveform that ``requires_grad`` gets a ``grad_fn`` whose backward is exact (the gain depends on ``x``).
    ``TypeError`` for a float64 input, ``ValueError`` for a rank other than 3."""
    from . import autograd
    validate_data_format_str(data_format)
    fmt = resolve_data_format(data_format)
    autograd.refuse(x, 3, 'add_noise expects a rank-3 waveform batch, got shape %s', TypeError,
                    'add_noise has float32 kernels only; got a float64 input (cast it to float32)')
    plan = noise if isinstance(noise, NoisePlan) else NoisePlan(noise)
    x, _ = autograd.to_device(x, 'float32')
    table = noise_table(int(x.shape[0]), x.device, plan.lengths, snr_db, index, offset)
    return _add_noise_run(x, plan, table, fmt)[0]


# --------------------------------------------------------------------------------------
# Griffin-Lim
# --------------------------------------------------------------------------------------
def griffin_lim_parameters(n_iter, momentum, power):
    """Validated (n_iter, momentum, power): an integer >= 0, 0 <= momentum < 1, power > 0 and finite (``ValueError``)."""
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
        raise ValueError('GriffinLim: n_iter must be an integer >= 0, got %r' % (n_iter,))
    for name, v in (('momentum', momentum), ('power', power)):
        if isinstance(v, bool) or np.ndim(v) != 0 or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError('GriffinLim: %s must be a number, got %r' % (name, v))
    if not 0.0 <= float(momentum) < 1.0:
        raise ValueError('GriffinLim: 0 <= momentum < 1 is required, got %r' % (momentum,))
    if not (float(power) > 0.0 and np.isfinite(float(power))):
        raise ValueError('GriffinLim: power must be positive and finite, got %r' % (power,))
    return int(n_iter), float(momentum), float(power)


def griffin_lim(mag, n_fft=2048, win_length=None, hop_length=None, window_name=None, n_iter=32, momentum=0.99, power=1.0,
                rand_init=True, length=None, input_data_format='default', output_data_format='default', init=None,
                return_convergence=False):
    """Griffin-Lim phase reconstruction of a magnitude spectrogram batch on the GPU (``kapre_amd.GriffinLim`` as a function):
    (b, frame, n_fft // 2 + 1, ch) for ``channels_last``, (b, ch, frame, n_fft // 2 + 1) for ``channels_first``, float32 ->
    the waveform (b, time, ch) / (b, ch, time) of (frame - 1) hop + win samples, or of ``length``.

    ``init``: a complex64 spectrogram in ``mag``'s layout to start from instead of the zero or random phase (it is used as it
    is, not projected).  With ``return_convergence`` returns (waveform, sc), sc being the (n_iter, batch) device tensor of
    || |R_n| - mag || / || mag ||.  The result carries no ``grad_fn``: an input that requires grad is detached."""
    from . import time_frequency

    for data_format in (input_data_format, output_data_format):
        validate_data_format_str(data_format)
    n_iter, momentum, power = griffin_lim_parameters(n_iter, momentum, power)
    if win_length is None:
        win_length = n_fft
    if hop_length is None:
        hop_length = win_length // 4
    wave, sc = time_frequency._griffin_lim_run(
        mag, time_frequency._GL_CONSTS, int(n_fft), int(win_length), int(hop_length), window_name, get_window_fn(window_name),
        n_iter, momentum, power, bool(rand_init), length, resolve_data_format(input_data_format),
        resolve_data_format(output_data_format), init)
    return (wave, sc) if return_convergence else wave


# --------------------------------------------------------------------------------------
# time stretching (phase vocoder)
# --------------------------------------------------------------------------------------
def time_stretch_parameters(rate):
    """Validated rate: a finite number > 0, not a bool (``ValueError``); returned as a float."""
    if isinstance(rate, (bool, np.bool_)) or np.ndim(rate) != 0 or not isinstance(rate, (int, float, np.integer, np.floating)):
        raise ValueError('TimeStretch: rate must be a number > 0, got %r' % (rate,))
    if not (np.isfinite(float(rate)) and float(rate) > 0.0):
        raise ValueError('TimeStretch: rate must be finite and > 0, got %r' % (rate,))
    return float(rate)


def time_stretch_length(frames, rate: float):
    """Output frames of ``frames`` input frames at ``rate``: ceil(frames / rate), taken as the number of t >= 0 whose float64
    product t * rate is below ``frames`` -- the last output frame then starts at an input frame that exists, whatever the
    division would round to.  ``None`` stays ``None``."""
    if frames is None:
        return None
    frames, rate = int(frames), float(rate)
    if frames <= 0:
        return 0
    n = max(int(np.ceil(frames / rate)), 1)
    while n > 1 and np.floor((n - 1) * rate) > frames - 1:
        n -= 1
    while np.floor(n * rate) <= frames - 1:
        n += 1
    return n


def time_stretch_table(frames, rate):
    """(idx, alpha) of a time stretch of ``frames`` input frames: for output frame t, s = t * float64(rate), idx[t] = floor(s)
    (int32) and alpha[t] = s - idx[t] (float32, kept below 1); ``time_stretch_length(frames, rate)`` entries."""
    rate = time_stretch_parameters(rate)
    n = time_stretch_length(frames, rate)
    s = np.arange(n, dtype=np.float64) * rate
    fl = np.floor(s)
    if n and fl[-1] >= 2.0 ** 31 - 2:
        raise ValueError('TimeStretch: %d frames at rate %r: frame indices of 2^31 and more are not supported' % (frames, rate))
    alpha = np.minimum((s - fl).astype(np.float32), np.nextafter(np.float32(1.0), np.float32(0.0)))
    return fl.astype(np.int32), alpha


def phase_vocoder(x, rate, data_format='default'):
    """Phase-vocoder time stretch of a complex spectrogram batch on the GPU (``kapre_amd.TimeStretch`` as a function; the
    operation of ``torchaudio.functional.phase_vocoder`` and ``librosa.phase_vocoder``): (b, frame, freq, ch) for
    ``channels_last``, (b, ch, frame, freq) for ``channels_first``, complex64 in and out, ceil(frame / rate) frames.  ``rate`` < 1
    slows the signal down, > 1 speeds it up.  There is no ``hop_length``: the expected phase advance of a bin changes the
    accumulated phase by whole turns only (see ``TimeStretch``).  One kernel launch.  The result carries no ``grad_fn``: an
    input that requires grad is detached."""
    from . import time_frequency

    validate_data_format_str(data_format)
    rate = time_stretch_parameters(rate)
    fmt = resolve_data_format(data_format)
    return time_frequency._time_stretch_run(x, rate, fmt, time_frequency._TS_CONSTS)


# --------------------------------------------------------------------------------------
# harmonic-percussive separation
# --------------------------------------------------------------------------------------
def _hpss_pair(value, what):
    """A scalar, or a (harmonic, percussive) pair of scalars, as a pair of plain numbers (no bools, no arrays)."""
    pair = tuple(value) if isinstance(value, (tuple, list)) else (value, value)
    if len(pair) != 2:
        raise ValueError('HPSS: %s must be a number or a (harmonic, percussive) pair, got %r' % (what, value))
    for v in pair:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError('HPSS: %s must be a number or a (harmonic, percussive) pair of numbers, got %r' % (what, value))
    return pair


def hpss_parameters(kernel_size=31, power=2.0, margin=1.0):
    """Validated ((kh, kp), power, (mh, mp)) of an HPSS: the window lengths odd integers in 3 ... 31, ``power`` > 0 (``inf``
    allowed), the margins finite and >= 1; each of ``kernel_size`` and ``margin`` a scalar or a (harmonic, percussive) pair.
    A bool, an even or out-of-range size, a margin < 1 or a power <= 0 raises ``ValueError``."""
    sizes = _hpss_pair(kernel_size, 'kernel_size')
    for k in sizes:
        if float(k) != int(k) or int(k) % 2 == 0 or not 3 <= int(k) <= 31:
            raise ValueError('HPSS: kernel_size must be odd and in 3 ... 31, got %r' % (kernel_size,))
    margins = _hpss_pair(margin, 'margin')
    for m in margins:
        if not (np.isfinite(float(m)) and float(m) >= 1.0):
            raise ValueError('HPSS: margin must be finite and >= 1, got %r' % (margin,))
    if isinstance(power, (bool, np.bool_)) or np.ndim(power) != 0 or not isinstance(power, (int, float, np.integer, np.floating)) \
            or not float(power) > 0.0:
        raise ValueError('HPSS: power must be a number > 0 (inf for a hard mask), got %r' % (power,))
    return (int(sizes[0]), int(sizes[1])), float(power), (float(margins[0]), float(margins[1]))


def hpss(x, kernel_size=31, power=2.0, margin=1.0, mask=False, data_format='default'):
    """Median-filter harmonic-percussive separation of a spectrogram batch on the GPU (``kapre_amd.HPSS`` as a function; the
    operation of ``librosa.decompose.hpss``): returns ``(harmonic, percussive)``, each of x's shape -- (b, frame, freq, ch) for
    ``channels_last``, (b, ch, frame, freq) for ``channels_first``.  ``x`` is a float32 spectrogram or the complex64 output of
    ``STFT``, whose magnitude makes the masks, which then multiply it.  ``mask=True`` returns the two float32 masks.  One kernel
    launch.  The results carry no ``grad_fn``: an input that requires grad is detached."""
    from . import time_frequency

    validate_data_format_str(data_format)
    sizes, power, margins = hpss_parameters(kernel_size, power, margin)
    fmt = resolve_data_format(data_format)
    return time_frequency._hpss_run(x, sizes, power, margins, bool(mask), fmt, 'pair')
