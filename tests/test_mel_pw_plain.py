"""The plain-output instance of the per-wave mel kernel (k_mel_plain_pw, kapre_amd/csrc/kpr_mel_pw_kernels.h): n_fft 2048 without
decibels on contiguous input rows with a linear output, band plan (NR, CMQ) = (2, 1).  It specialises k_mel_pw<1024, W, false>
and changes no floating-point operation, so it must give the general kernel's BITS ("mel_pw_plain" 0 = the general kernel), match
the float64 oracle at the tolerance tests/test_gpu_parity.py uses for the fused mel, and every launch outside its conditions
must stay on the general kernels.  The launch label is the general kernel's with ",plain" behind it.

The stale-plan refusal of the plain route is tests/test_gpu_parity.py::test_packed_filterbank_of_another_matrix_is_refused: it
runs on the default route, which is this kernel (the header comparison sits in front of the first access through pl.sec)."""
import numpy as np
import pytest

import kapre_oracle as o
from test_gpu_parity import assert_close, assert_db_close, to_np

from kapre_amd import _ffi, backend, composed

pytestmark = pytest.mark.gpu

T = 2048 + 512 * 9 + 17                      # ten frames per signal; with pad_end the last frames take the zero-filling fetch
BASE = dict(n_fft=2048, hop_length=512, sample_rate=44100)
# (batch, channels, data format in and out, pad_end): 30 frames with edge handling at the item ends; the same with padded last
# frames; the linear output with C > 1
SHAPES = [(3, 1, "channels_last", False), (3, 1, "channels_last", True), (2, 2, "channels_first", False)]
IDS = ["b3c1", "b3c1_pad_end", "b2c2_channels_first"]
_CACHE = {}


def _x(batch, ch, fmt, t=T):
    """float32 uniform(-1, 1), one array per shape (shared by the tests, never written)"""
    key = (batch, ch, fmt, t)
    if key not in _CACHE:
        shape = (batch, t, ch) if fmt == "channels_last" else (batch, ch, t)
        x = np.random.default_rng(20261019 + 7 * batch + ch).uniform(-1, 1, shape).astype(np.float32)
        _CACHE[key] = x
    return _CACHE[key]


def _want(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _run(layer, x, plain=1, variant=0):
    """(output, launch label) under "mel_pw_plain" / "mel_variant" """
    old_p, old_v = _ffi.set_option("mel_pw_plain", plain), _ffi.set_option("mel_variant", variant)
    try:
        out = to_np(layer(x))
        label = _ffi.last_launches()
    finally:
        _ffi.set_option("mel_pw_plain", old_p)
        _ffi.set_option("mel_variant", old_v)
    return out, label


@pytest.mark.parametrize("variant", [6, 5, 7])          # W = 4, 8, 16 (sixteen waves: some get no ticket at all)
@pytest.mark.parametrize("batch, ch, fmt, pad_end", SHAPES, ids=IDS)
def test_plain_gives_the_general_kernels_bits(batch, ch, fmt, pad_end, variant):
    x = _x(batch, ch, fmt)
    layer = composed.get_melspectrogram_layer(n_mels=128, pad_end=pad_end, input_data_format=fmt, output_data_format=fmt, **BASE)
    got, label = _run(layer, x, 1, variant)
    ref, label0 = _run(layer, x, 0, variant)
    w = {6: 4, 5: 8, 7: 16}[variant]
    assert label == "k_mel_pw<1024,w%d>,plain" % w, label
    assert label0 == "k_mel_pw<1024,w%d>" % w, label0
    assert label.startswith("k_mel_pw<1024") and ",plain" in label and ",plain" not in label0
    assert got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("batch, ch, fmt, pad_end", SHAPES, ids=IDS)
def test_plain_against_the_oracle(batch, ch, fmt, pad_end):
    x = _x(batch, ch, fmt)
    kw = dict(n_mels=128, pad_end=pad_end, input_data_format=fmt, output_data_format=fmt, **BASE)
    got, label = _run(composed.get_melspectrogram_layer(**kw), x)
    assert ",plain" in label, label
    assert_close(got, _want(("mel", batch, ch, fmt, pad_end), lambda: o.kapre_melspectrogram(x, **kw)))


def test_default_is_on():
    assert _ffi.set_option("mel_pw_plain", 1) == 1     # (returns the previous value)


# launches outside the plain instance's conditions: (name, channels, format in, format out, layer keywords)
OTHERS = [
    ("decibel", 1, "channels_last", "channels_last", dict(n_mels=128, return_decibel=True)),
    ("channels_last_c2", 2, "channels_last", "channels_last", dict(n_mels=128)),
    ("mels40_nr1", 1, "channels_last", "channels_last", dict(n_mels=40)),
    ("mels200_nr4", 1, "channels_last", "channels_last", dict(n_mels=200)),
    ("mels96_cmq2", 1, "channels_last", "channels_last", dict(n_mels=96)),
]


@pytest.mark.parametrize("name, ch, fi, fo, extra", OTHERS, ids=[c[0] for c in OTHERS])
def test_routes_that_do_not_take_it(name, ch, fi, fo, extra):
    x = _x(2, ch, fi)
    kw = dict(input_data_format=fi, output_data_format=fo, **BASE, **extra)
    got, label = _run(composed.get_melspectrogram_layer(**kw), x)
    assert "k_mel_pw" in label and ",plain" not in label, label
    want = o.kapre_melspectrogram(x, **kw)
    (assert_db_close if extra.get("return_decibel") else assert_close)(got, want)


def test_plan_fields_of_the_routed_banks():
    """what sends the three n_mels cases above to the general kernel, read from the packed header (host only): (NR, CMQ) is
    (2, 1) for the headline's bank alone"""
    def nr_cmq(n_mels):
        fb = np.ascontiguousarray(np.asarray(backend.filterbank_mel(44100, 1025, n_mels), np.float32))
        h = _ffi.filterbank_pack(fb, _ffi.filterbank_kranges(fb))[:64].view(np.uint32)
        assert h[6] != 0 and h[7] == 64
        return int(h[8]), int(h[9])
    assert nr_cmq(128) == (2, 1)
    assert nr_cmq(40)[0] == 1 and nr_cmq(200)[0] == 4
    assert nr_cmq(96) == (2, 2)                         # a triangular bank with two offset quads per round exists at 1025 bins


def test_log_frequency_bank_has_no_band_plan_route():
    x = _x(2, 1, "channels_last")
    kw = dict(input_data_format="channels_last", output_data_format="channels_last", **BASE)
    got, label = _run(composed.get_log_frequency_spectrogram_layer(**kw), x)
    assert "k_mel_pw" not in label and ",plain" not in label, label
    mag = np.abs(o.kapre_stft(x, n_fft=2048, hop_length=512, input_data_format="channels_last", output_data_format="channels_last"))
    assert_close(got, o.apply_filterbank(mag, o.filterbank_log(44100, 1025), "channels_last"))
