"""kapre_amd.PitchShift / backend.pitch_shift on the GPU: bit-equal to the composition of the public pieces
(get_time_stretch_layer, then backend.resample(method='direct', length=T)), the pitch of a tone, and the layer in a
Sequential in front of the fused mel launch."""
import numpy as np
import pytest

from conftest import speech

pytestmark = pytest.mark.gpu


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("n_steps", [4, -3])
def test_composition_of_the_public_pieces(n_steps):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, backend

    sr, n_fft, hop, T = 16000, 256, 64, 4000
    rate, orig_freq = backend.pitch_shift_parameters(sr, n_steps)
    rng = np.random.default_rng(n_steps + 20)
    for fmt in ("channels_last", "channels_first"):
        for C in (1, 2, 3):
            x = np.stack([speech(T, offset=9000 * i) for i in range(3 * C)]).astype(np.float32).reshape(3, C, T)
            x = x + np.float32(0.01) * rng.standard_normal(x.shape).astype(np.float32)
            xt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 1, 2)) if fmt == "channels_last" else x).cuda()
            layer = kapre.PitchShift(sr, n_steps, n_fft=n_fft, hop_length=hop, data_format=fmt)
            y = layer(xt)
            assert _ffi.last_launches() == "k_resample_direct<%d>" % (2 if fmt == "channels_last" and C == 2 else 1)
            assert y.shape == xt.shape and y.dtype == torch.float32 and y.grad_fn is None and not y.requires_grad
            stretched = kapre.get_time_stretch_layer(rate, n_fft=n_fft, hop_length=hop, input_data_format=fmt)(xt)
            want = backend.resample(stretched, orig_freq, sr, data_format=fmt, method='direct', length=T)
            assert torch.equal(y, want)
            assert torch.equal(backend.pitch_shift(xt, sr, n_steps, n_fft=n_fft, hop_length=hop, data_format=fmt), y)
            assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
            # an input that asks for a gradient gets none: the time stretch carries none
            yg = layer(xt.clone().requires_grad_(True))
            assert yg.grad_fn is None and not yg.requires_grad and torch.equal(yg, y)
    assert torch.equal(layer(to_np(xt)), y)                                   # numpy in
    kapre.check_device()


def test_zero_steps_returns_the_same_object_and_launches_nothing():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, backend

    x = torch.zeros((2, 3000, 1), device="cuda")
    _ffi.resample_direct(x[:0], "channels_last", (2, 1, 6, 0.99), False, 0)      # an empty call: the launch log restarts
    assert kapre.PitchShift(16000, 0, n_fft=256)(x) is x and backend.pitch_shift(x, 16000, 0.0) is x
    assert _ffi.last_launches() == ""


@pytest.mark.parametrize("n_steps", [4, -5])
def test_tone_moves_to_the_shifted_pitch(n_steps):
    import kapre_amd as kapre
    from kapre_amd import backend

    sr, n_fft, f0 = 16000, 512, 1000.0
    x = np.sin(2.0 * np.pi * f0 * np.arange(sr) / sr).astype(np.float32).reshape(1, sr, 1)
    y = to_np(kapre.PitchShift(sr, n_steps, n_fft=n_fft)(x))
    assert y.shape == x.shape and np.isfinite(y).all()
    orig_freq = backend.pitch_shift_parameters(sr, n_steps)[1]
    want = f0 * orig_freq / sr
    mid = y[0, n_fft:-n_fft, 0].astype(np.float64)                            # away from the ramps of the first and last windows
    amp = np.abs(np.fft.rfft(mid * np.hanning(len(mid))))
    peak = np.argmax(amp) * sr / len(mid)
    print("n_steps %+d: peak at %.2f Hz, 1000 * orig_freq / sr = %.2f Hz (2^(n/12): %.2f Hz)" % (n_steps, peak, want, f0 * 2.0 ** (n_steps / 12)))
    assert abs(peak - want) <= sr / len(mid)                                  # one bin of this estimate
    kapre.check_device()


def test_eval_mode_in_front_of_the_fused_mel_launch():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi

    kw = dict(n_fft=400, hop_length=160, sample_rate=16000, n_mels=80, return_decibel=False)
    mel = kapre.get_melspectrogram_layer(input_shape=(None, 1), **kw)
    shift = kapre.PitchShift(16000, 2, n_fft=512, input_shape=(8000, 1))
    model = kapre.Sequential([shift, mel])
    assert model.output_shape == mel.compute_output_shape((None, 8000, 1))
    x = torch.from_numpy(np.stack([speech(8000), speech(8000, offset=8000)])[:, :, None].astype(np.float32)).cuda()
    out = model(x, training=False)
    launches = _ffi.last_launches()
    alone = shift(x)
    assert alone.shape == x.shape
    assert torch.equal(out, mel(alone)) and _ffi.last_launches() == launches       # the unchanged fused mel launch
    assert launches.startswith("k_mel")
    assert torch.equal(model(x), out)
    kapre.check_device()
