"""The two-kernel inverse STFT and the forward DFT-GEMM family, one case per FFT family, with the exact launch list asserted.

istft_path 2 keeps kpr_istft_f32 off its one-launch kernels: every call is an inverse FFT of its family into the workspace, then
k_ola.  tests/test_fuzz_gate.py looks for the substring "k_irfft", which k_irfft_mr, k_irfft_bs, k_irfft_big and k_irfft_gen satisfy
as well; here the list of kpr_last_launches() must EQUAL the expected one.  Reference: numpy in float64 -- irfft(n=n_fft), cropped
or zero-extended to win_length, times the window, overlap-added untrimmed; rfft of the windowed frames for the forward cases.
Limits: those of assert_close in tests/test_gpu_parity.py (REL, the contract, and REG, the regression bound of the float32 kernels);
1e-11 for complex128 as in tests/test_win_gt_nfft.py."""
import numpy as np
import pytest

from conftest import rel_err

REL = 1e-4           # tests/test_gpu_parity.py
REG = 4e-6
F64 = 1e-11          # tests/test_win_gt_nfft.py

CL, CF = "channels_last", "channels_first"
B, C, F = 2, 2, 9

# (n_fft, win_length, hop, kpr_fft_plan code of (n_fft, n_fft), launches of the inverse under istft_path 2)
INVERSE = [
    (512, 512, 128, "FFT_POW2", ["k_irfft", "k_ola"]),
    (400, 400, 100, "FFT_MIXED_RADIX", ["k_irfft_mr", "k_ola"]),
    (300, 300, 75, "FFT_BLUESTEIN", ["k_irfft_bs", "k_ola"]),
    (4096, 4096, 1024, "FFT_SUB_FFT", ["k_irfft_big", "k_ola"]),
    (1200, 1200, 300, "FFT_GENERIC", ["k_irfft_gen<float>", "k_ola"]),
    (67, 67, 16, "FFT_DFT_GEMM", ["k_gemm", "k_ola"]),
    # win_length > n_fft: no inverse FFT family takes zero-extended frames, whatever the family of n_fft
    (400, 500, 100, "FFT_MIXED_RADIX", ["k_gemm", "k_fill_cols", "k_ola"]),
]


def test_fft_plan_names_the_families_of_the_table():
    """CPU: the sizes above belong to the families the expected labels assume"""
    from kapre_amd import _ffi
    L = _ffi.lib()
    for n_fft, _, _, code, _ in INVERSE:
        assert L.kpr_fft_plan(n_fft, n_fft) == getattr(_ffi, code), n_fft


def _spectrogram(rng, n_fft, fmt, dtype):
    k = n_fft // 2 + 1
    shape = (B, F, k, C) if fmt == CL else (B, C, F, k)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def _istft_reference(spec, window, n_fft, win, hop, fmt):
    """float64; spec (B, F, K, C) or (B, C, F, K) -> waveform (B, T, C) or (B, C, T), T = (F - 1) hop + win"""
    s = spec.astype(np.complex128)
    if fmt == CL:
        s = s.transpose(0, 3, 1, 2)
    frames = np.fft.irfft(s, n=n_fft, axis=-1)
    if win <= n_fft:
        frames = frames[..., :win]
    else:
        frames = np.concatenate([frames, np.zeros(frames.shape[:-1] + (win - n_fft,))], axis=-1)
    frames = frames * window.astype(np.float64)
    out = np.zeros((B, C, (F - 1) * hop + win))
    for f in range(F):
        out[..., f * hop:f * hop + win] += frames[:, :, f, :]
    return out.transpose(0, 2, 1) if fmt == CL else out


def _check(got, want, f64=False):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    e = rel_err(got, want)
    print("relative error %.3g" % e)
    if f64:
        assert e <= F64, e
    else:
        assert e <= REL and e <= REG, e


def _run_istft(n_fft, win, hop, fmt, dtype, expected):
    import torch
    from kapre_amd import _ffi
    rng = np.random.default_rng(n_fft + win + hop)
    spec = _spectrogram(rng, n_fft, fmt, dtype)
    window = rng.uniform(0.2, 1.0, win).astype(np.float64 if dtype == np.complex128 else np.float32)
    old = _ffi.set_option("istft_path", 2)
    try:
        got = _ffi.istft(torch.from_numpy(spec).cuda(), torch.from_numpy(window).cuda(), n_fft, win, hop, fmt, fmt)
        launches = _ffi.last_launches().split(" + ")
    finally:
        _ffi.set_option("istft_path", old)
    assert launches == expected, launches
    _check(got.cpu().numpy(), _istft_reference(spec, window, n_fft, win, hop, fmt), f64=dtype == np.complex128)


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft, win, hop, code, expected", INVERSE)
@pytest.mark.parametrize("fmt", [CL, CF])
def test_two_kernel_inverse_launches_its_family(n_fft, win, hop, code, expected, fmt):
    _run_istft(n_fft, win, hop, fmt, np.complex64, expected)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [CL, CF])
def test_two_kernel_inverse_float64(fmt):
    _run_istft(400, 400, 100, fmt, np.complex128, ["k_irfft_gen<double>", "k_ola"])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [CL, CF])
@pytest.mark.parametrize("mode, expected", [("OUT_COMPLEX", ["k_gemm"]), ("OUT_MAGNITUDE", ["k_gemm", "k_cplx_to_real"])])
def test_forward_dft_gemm_family(mode, expected, fmt):
    """n_fft 67 (a prime above 64): the DFT as a GEMM; a real-valued output stages the complex spectrum and adds the magnitude pass"""
    import torch
    from kapre_amd import _ffi
    n_fft, hop = 67, 16
    t = (F - 1) * hop + n_fft
    rng = np.random.default_rng(67)
    x = rng.standard_normal((B, t, C) if fmt == CL else (B, C, t)).astype(np.float32)
    window = rng.uniform(0.2, 1.0, n_fft).astype(np.float32)
    geom = _ffi.StftGeom(B, C, t, n_fft, n_fft, hop, 0, 0, _ffi.layout(fmt), _ffi.layout(fmt))
    assert _ffi.num_frames(geom) == F
    got = _ffi.stft(torch.from_numpy(x).cuda(), geom, F, torch.from_numpy(window).cuda(), getattr(_ffi, mode))
    assert _ffi.last_launches().split(" + ") == expected, _ffi.last_launches()
    xs = (x.transpose(0, 2, 1) if fmt == CL else x).astype(np.float64)                      # (B, C, T)
    idx = np.arange(n_fft)[None, :] + hop * np.arange(F)[:, None]
    want = np.fft.rfft(xs[..., idx] * window.astype(np.float64), axis=-1)                   # (B, C, F, K)
    if mode == "OUT_MAGNITUDE":
        want = np.abs(want)
    _check(got.cpu().numpy(), want.transpose(0, 2, 3, 1) if fmt == CL else want)
