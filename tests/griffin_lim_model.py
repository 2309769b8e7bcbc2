"""CPU model of kapre_amd.GriffinLim (test infrastructure: the checker of tests/test_griffin_lim_*.py).

The definition of include/kapre_hip.h, restated on the oracle's transforms: A = oracle.kapre_stft without padding,
A+ = oracle.kapre_istft (untrimmed), c = momentum / (1 + momentum):

    mag = M ** (1 / power);  S_0 = mag e^{i phi} (or given);  T_0 = 0
    n = 1 .. n_iter:  R_n = A(A+(S_{n-1}));  sc_n = || |R_n| - mag || / || mag || per batch item
                      a = R_n - c T_{n-1};  S_n = mag a / (|a| + 1e-16);  T_n = R_n
    y = A+(S_{n_iter})

``griffin_lim`` runs it in float64; ``griffin_lim_f32`` is the same loop in float32 on torch's CPU FFTs (what a float32
implementation can be expected to reach); ``philox_phase`` is the initial phase the device draws; ``project_bound`` the
elementwise limit of one projection in float32.
"""
import numpy as np

import kapre_oracle as o
from augment_model import philox4x32_10

TINY = 1e-16
U32 = 2.0 ** -24          # unit roundoff of float32

# (n_fft, win_length, hop_length, frames): power-of-two and mixed-radix transforms, win < n_fft, hop that does not divide win
GEOMETRIES = [(256, 256, 64, 9), (400, 400, 160, 11), (512, 400, 100, 7), (1024, 1024, 256, 6)]


def natural_length(frames, win, hop):
    return (frames - 1) * hop + win if frames > 0 else 0


def momentum_c(momentum):
    return momentum / (1.0 + momentum)


def sc_of(R, mag):
    """|| |R| - mag ||_2 / || mag ||_2 per item of the leading axis (float64)"""
    R = np.asarray(R, dtype=np.complex128)
    mag = np.asarray(mag, dtype=np.float64)
    axes = tuple(range(1, R.ndim))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.sqrt(np.sum((np.abs(R) - mag) ** 2, axis=axes) / np.sum(mag ** 2, axis=axes))


def project(R, T, mag, c):
    """S = mag a / (|a| + 1e-16), a = R - c T (``T`` None: a = R), float64"""
    R = np.asarray(R, dtype=np.complex128)
    a = R if T is None else R - c * np.asarray(T, dtype=np.complex128)
    return np.asarray(mag, dtype=np.float64) * a / (np.abs(a) + TINY)


def project_bound(R, T, mag, c):
    """Elementwise limit of |S_float32 - S_float64|: 2 u mag (6 + 2 (|R| + c |T|) / |a|).  Six roundings on the quotient path
    (|a|^2 in two, the root, the guard, the quotient, the product), two on a scaled by its cancellation, the whole doubled for
    the hardware's reciprocal and square root (the practice of tests/test_pcen_gpu.py)."""
    R = np.asarray(R, dtype=np.complex128)
    Tm = np.zeros_like(R) if T is None else np.asarray(T, dtype=np.complex128)
    a = R - c * Tm
    with np.errstate(divide='ignore', invalid='ignore'):
        cancel = np.where(np.abs(a) > 0, (np.abs(R) + c * np.abs(Tm)) / np.abs(a), 0.0)
    return 2.0 * U32 * np.asarray(mag, dtype=np.float64) * (6.0 + 2.0 * cancel)


def analysis(y, n_fft, win, hop, window_name, wave_fmt, spec_fmt):
    return o.kapre_stft(y, n_fft, win, hop, window_name, False, False, wave_fmt, spec_fmt)


def synthesis(S, n_fft, win, hop, window_name, spec_fmt, wave_fmt):
    return o.kapre_istft(S, n_fft, win, hop, window_name, spec_fmt, wave_fmt)


def griffin_lim(M, n_fft, win, hop, window_name=None, n_iter=32, momentum=0.99, power=1.0, S0=None, phase=None,
                spec_fmt='channels_last', wave_fmt='channels_last'):
    """float64: (y, sc) with sc of shape (n_iter, batch).  ``S0`` (complex) or ``phase`` (radian) in M's layout; neither:
    zero phase."""
    mag = np.asarray(M, dtype=np.float64)
    if power != 1.0:
        mag = mag ** (1.0 / power)
    if S0 is not None:
        S = np.asarray(S0, dtype=np.complex128)
    elif phase is not None:
        S = mag * np.exp(1j * np.asarray(phase, dtype=np.float64))
    else:
        S = mag.astype(np.complex128)
    c = momentum_c(momentum)
    T = None
    sc = np.zeros((n_iter, mag.shape[0]))
    for n in range(n_iter):
        R = analysis(synthesis(S, n_fft, win, hop, window_name, spec_fmt, wave_fmt), n_fft, win, hop, window_name, wave_fmt, spec_fmt)
        sc[n] = sc_of(R, mag)
        S = project(R, T if momentum != 0 else None, mag, c)
        T = R
    return synthesis(S, n_fft, win, hop, window_name, spec_fmt, wave_fmt), sc


# ---- the same loop in float32 on torch's CPU FFTs (canonical layout (batch, ch, frame, bin) inside) ----------------------
def _to_first(x, fmt, rank):
    import torch
    if fmt == 'channels_last':
        return x.permute(0, rank - 1, *range(1, rank - 1)).contiguous()
    return x


def _from_first(x, fmt, rank):
    if fmt == 'channels_last':
        return x.permute(0, *range(2, rank), 1).contiguous()
    return x


def griffin_lim_f32(M, n_fft, win, hop, window_name=None, n_iter=32, momentum=0.99, power=1.0, S0=None, phase=None,
                    spec_fmt='channels_last', wave_fmt='channels_last', noise=0.0, seed=0):
    """float32 on the CPU: (y, sc) as numpy arrays, sc float64 computed from the float32 R.  ``noise``: relative Gaussian noise
    injected behind each transform (the conditioning experiment of the issue; 0 = none)."""
    import torch

    w = torch.from_numpy(o.get_window(window_name, win).astype(np.float32))
    ws = torch.from_numpy(o.inverse_stft_window(win, hop, o.get_window(window_name, win)).astype(np.float32))
    gen = torch.Generator().manual_seed(seed)

    def noisy(t):
        if noise == 0.0:
            return t
        scale = noise * float(t.abs().max())
        if t.is_complex():
            return t + scale * torch.view_as_complex(torch.randn(t.shape + (2,), generator=gen))
        return t + scale * torch.randn(t.shape, generator=gen)

    def synth(S):                      # (b, c, f, k) complex64 -> (b, c, t) float32
        fr = torch.fft.irfft(S, n=n_fft, dim=-1)
        fr = fr[..., :win] if n_fft >= win else torch.nn.functional.pad(fr, (0, win - n_fft))
        fr = fr * ws
        f = fr.shape[-2]
        out = torch.zeros(fr.shape[:-2] + (natural_length(f, win, hop),), dtype=torch.float32)
        for i in range(f):
            out[..., i * hop:i * hop + win] += fr[..., i, :]
        return noisy(out)

    def ana(y):                        # (b, c, t) -> (b, c, f, k)
        fr = y.unfold(-1, win, hop) * w
        fr = fr[..., :n_fft] if win >= n_fft else torch.nn.functional.pad(fr, (0, n_fft - win))
        return noisy(torch.fft.rfft(fr, n=n_fft, dim=-1))

    mag = _to_first(torch.from_numpy(np.asarray(M, dtype=np.float32)), spec_fmt, 4)
    if power != 1.0:
        mag = mag ** torch.tensor(1.0 / power, dtype=torch.float32)
    if S0 is not None:
        S = _to_first(torch.from_numpy(np.asarray(S0, dtype=np.complex64)), spec_fmt, 4)
    elif phase is not None:
        ph = _to_first(torch.from_numpy(np.asarray(phase, dtype=np.float32)), spec_fmt, 4)
        S = torch.polar(mag, ph)
    else:
        S = torch.complex(mag, torch.zeros_like(mag))
    c = np.float32(momentum_c(momentum))
    T = None
    sc = np.zeros((n_iter, mag.shape[0]))
    for n in range(n_iter):
        R = ana(synth(S))
        sc[n] = sc_of(R.numpy(), mag.numpy())
        a = R if (T is None or momentum == 0) else R - c * T
        S = mag * a / (a.abs() + np.float32(TINY))
        T = R
    return _from_first(synth(S), wave_fmt, 3).numpy(), sc


def root_f32(M2, power):
    """mag = M2 ** (1 / power) as a float32 implementation computes it"""
    return np.power(np.asarray(M2, dtype=np.float32), np.float32(1.0 / power), dtype=np.float32)


# ---- the initial phase of the device ------------------------------------------------------------------------------------
def philox_phase(seed, calls, shape, fmt):
    """phi = 2 pi r 2^-32 (float64, in [0, 2 pi)) for a spectrogram of ``shape`` in the layout ``fmt``: r is word (e mod 4) of
    Philox4x32-10 with key ``seed`` and counter (e div 4, calls), e being the element's index in the channels_first order
    (batch, ch, frame, bin) -- so the draw of an element does not depend on the layout."""
    seed, calls = int(seed) & (2 ** 64 - 1), int(calls) & (2 ** 64 - 1)
    if fmt == 'channels_last':
        b, f, k, ch = shape
    else:
        b, ch, f, k = shape
    e = np.arange(b * ch * f * k, dtype=np.uint64)
    g = e >> np.uint64(2)
    r4 = philox4x32_10((g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), calls & 0xFFFFFFFF, calls >> 32),
                       (seed & 0xFFFFFFFF, seed >> 32))
    r = np.choose((e & np.uint64(3)).astype(np.int64), r4).astype(np.float64)
    phi = (2.0 * np.pi * r * 2.0 ** -32).reshape(b, ch, f, k)
    return np.transpose(phi, (0, 2, 3, 1)) if fmt == 'channels_last' else phi


def wrap(d):
    """an angle difference wrapped into [-pi, pi)"""
    return (np.asarray(d) + np.pi) % (2.0 * np.pi) - np.pi


# ---- inputs --------------------------------------------------------------------------------------------------------------
def speech_magnitude(geometry, batch=1, channels=1, spec_fmt='channels_last', window_name=None):
    """|A(x)| of golden speech clips (one offset per batch item and channel) with exactly ``frames`` frames: float32"""
    from conftest import speech
    n_fft, win, hop, frames = geometry
    t = natural_length(frames, win, hop)
    x = np.stack([np.stack([speech(t, 1000 + 3000 * (bi * channels + ci)) for ci in range(channels)]) for bi in range(batch)])
    M = np.abs(o.kapre_stft(x, n_fft, win, hop, window_name, False, False, 'channels_first', spec_fmt))
    return M.astype(np.float32)
