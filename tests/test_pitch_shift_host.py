"""kapre_amd.PitchShift / backend.pitch_shift on the host: the parameters against hand values, the refusals, the config round
trip, the output shape, and the Sequential in front of a mel front end building, saving and loading."""
import os

import numpy as np
import pytest


def test_parameters_against_hand_values():
    from kapre_amd import backend

    # rate = 2^(-n / 12); orig_freq = int(sample_rate / rate): 16000 * 2^(4/12) = 20158.7..., 48000 * 2^(1/12) = 50854.2...,
    # 44100 * 2^(2/12) = 49500.5...
    assert backend.pitch_shift_parameters(16000, 4, 12)[1] == 20158
    assert backend.pitch_shift_parameters(48000, 1, 12)[1] == 50854
    assert backend.pitch_shift_parameters(44100, 2, 12)[1] == 49500
    rate, orig = backend.pitch_shift_parameters(16000, -12)
    assert rate == 2.0 and orig == 8000
    rate, orig = backend.pitch_shift_parameters(22050, 0)
    assert rate == 1.0 and orig == 22050
    rate, orig = backend.pitch_shift_parameters(16000, 0.5, 24)              # a float step, quarter tones
    assert rate == 2.0 ** (-0.5 / 24) and orig == int(16000 / rate)
    assert backend.pitch_shift_parameters(16000, np.float32(2.0), 12) == backend.pitch_shift_parameters(16000, 2, 12)
    # every semitone step of +-12 at the usual rates is supported: one path, no step that raises
    from kapre_amd import _ffi
    for sr in (16000, 22050, 32000, 44100, 48000):
        for n in list(range(-12, 0)) + list(range(1, 13)):
            orig = backend.pitch_shift_parameters(sr, n)[1]
            for adjoint in (False, True):
                assert _ffi.resample_direct_plan(orig, sr, 6, 0.99, adjoint)[0] <= 128


def test_refusals():
    import kapre_amd as kapre
    from kapre_amd import backend

    for bad in (True, False, None, "2", float("nan"), float("inf"), [1]):
        with pytest.raises(ValueError, match="n_steps must be a finite number"):
            backend.pitch_shift_parameters(16000, bad)
    for bad in (0, -16000, 16000.0, True):
        with pytest.raises(ValueError, match="sample_rate must be a positive integer"):
            backend.pitch_shift_parameters(bad, 2)
    for bad in (0, 12.0, True):
        with pytest.raises(ValueError, match="bins_per_octave must be an integer >= 1"):
            backend.pitch_shift_parameters(16000, 2, bad)
    with pytest.raises(ValueError, match="too small a shift to represent at 16000 Hz"):
        backend.pitch_shift_parameters(16000, 1e-6)
    with pytest.raises(ValueError, match="too small a shift"):
        kapre.PitchShift(8000, 1e-7)
    assert backend.pitch_shift_parameters(8000, -1e-7)[1] == 7999            # (the truncation: a tiny step down is a rate of its own)
    with pytest.raises(ValueError, match="below 2\\^31"):
        backend.pitch_shift_parameters(48000, 400)
    with pytest.raises(ValueError):
        kapre.PitchShift(16000, 2, data_format='weird')
    layer = kapre.PitchShift(16000, 4, n_fft=256, hop_length=64)
    with pytest.raises(ValueError, match="255 samples give no frame of n_fft = 256"):
        layer(np.zeros((1, 255, 1), dtype=np.float32))
    with pytest.raises(ValueError, match="rank-3"):
        layer(np.zeros((1, 4000), dtype=np.float32))
    with pytest.raises(TypeError, match="float32 kernels only"):
        layer(np.zeros((1, 4000, 1), dtype=np.float64))
    with pytest.raises(TypeError, match="float32 kernels only"):
        backend.pitch_shift(np.zeros((1, 4000, 1), dtype=np.float64), 16000, 4, n_fft=256)
    for bad in (0, 256.0, True):
        with pytest.raises(ValueError, match="n_fft must be a positive integer"):
            backend.pitch_shift(np.zeros((1, 4000, 1), dtype=np.float32), 16000, 4, n_fft=bad)
    with pytest.raises(ValueError, match="255 samples give no frame of n_fft = 256"):
        backend.pitch_shift(np.zeros((1, 255, 1), dtype=np.float32), 16000, 4, n_fft=256)


def test_zero_steps_returns_the_input_object():
    import kapre_amd as kapre
    from kapre_amd import backend

    x = np.zeros((2, 300, 1), dtype=np.float32)
    assert kapre.PitchShift(16000, 0)(x) is x and kapre.PitchShift(16000, 0.0, n_fft=256)(x) is x
    assert backend.pitch_shift(x, 44100, 0) is x


def test_config_round_trip_and_shapes():
    import kapre_amd as kapre
    from kapre_amd import keras_shim

    layer = kapre.PitchShift(44100, -3, bins_per_octave=12, n_fft=1024, hop_length=128, data_format='channels_first',
                             input_shape=(2, 22050), name='shift')
    cfg = layer.get_config()
    assert {k: cfg[k] for k in ('sample_rate', 'n_steps', 'bins_per_octave', 'n_fft', 'hop_length', 'data_format', 'name')} == \
        dict(sample_rate=44100, n_steps=-3, bins_per_octave=12, n_fft=1024, hop_length=128, data_format='channels_first', name='shift')
    again = kapre.PitchShift.from_config(cfg)
    assert again.get_config() == cfg and again.orig_freq == layer.orig_freq == int(44100 / 2.0 ** (3 / 12))
    assert again.rate == layer.rate == 2.0 ** (3 / 12)
    assert layer.output_shape == (None, 2, 22050)
    assert layer.compute_output_shape((None, 3, None)) == (None, 3, None)
    assert keras_shim.get_registered_object('Kapre>PitchShift') is kapre.PitchShift
    assert "No gradient" in kapre.PitchShift.__doc__


def test_sequential_with_a_mel_front_end_builds_saves_and_loads(tmp_path):
    import kapre_amd as kapre
    from kapre_amd import keras_shim

    kw = dict(n_fft=400, hop_length=160, sample_rate=16000, n_mels=80, return_decibel=False)
    mel = kapre.get_melspectrogram_layer(input_shape=(None, 1), **kw)
    model = kapre.Sequential([kapre.PitchShift(16000, 4, n_fft=512, input_shape=(16000, 1)), mel])
    assert model.output_shape == mel.compute_output_shape((None, 16000, 1))
    path = os.path.join(str(tmp_path), "shifted_front_end.keras")
    model.save(path)
    again = keras_shim.load_model(path)
    first = again.layers[0]
    assert type(first).__name__ == "PitchShift" and first.orig_freq == 20158 and first.n_fft == 512
    assert again.output_shape == model.output_shape
