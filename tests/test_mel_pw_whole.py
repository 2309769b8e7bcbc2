"""The whole-frames instance of the plain per-wave mel kernel (k_mel_whole_pw, kapre_amd/csrc/kpr_mel_pw_kernels.h): the plain
route's launches without padding (no pad_begin, no frame past the end of its item) and with exactly 128 filters.  It is
k_mel_plain_pw without the edge fetch and the per-store tests and changes no floating-point operation, so it must give the BITS of
the plain kernel ("mel_pw_plain" 2) and of the general kernel ("mel_pw_plain" 0), match the float64 oracle at the tolerance
tests/test_gpu_parity.py uses for the fused mel, and every launch outside its conditions must stay where it was.

The launch label does not tell the whole-frames kernel from the plain one (both are "k_mel_pw<1024,wN>,plain"); the library's
"verbose" line does: "k_mel_pw<1024,N,whole>" / "k_mel_pw<1024,N,plain>" / "k_mel_pw<1024,N>" on stderr, read here through capfd."""
import re

import numpy as np
import pytest

import kapre_oracle as o
from test_gpu_parity import assert_close, assert_db_close, to_np

from kapre_amd import _ffi, composed

pytestmark = pytest.mark.gpu

T10 = 2048 + 512 * 9                         # exactly ten whole frames
BASE = dict(n_fft=2048, hop_length=512, sample_rate=44100)
W_OF = {6: 4, 5: 8, 7: 16}                   # mel_variant -> waves per workgroup
# (batch, channels, data format in and out, samples, mel_variant)
CASES = [(3, 1, "channels_last", T10, v) for v in (6, 5, 7)]
CASES += [(3, 1, "channels_last", T10 + 17, v) for v in (6, 5, 7)]          # a ragged remainder that must not be read
CASES += [(2, 2, "channels_first", T10 + 17, v) for v in (6, 5, 7)]
CASES += [(1, 1, "channels_last", 2048 + 512 * 2, 7)]                       # three frames, sixteen waves: most never get a ticket
IDS = ["b%dc%d_%s_t%d_w%d" % (b, c, f.split("_")[1], t, W_OF[v]) for b, c, f, t, v in CASES]
_CACHE = {}


def _x(batch, ch, fmt, t):
    """float32 uniform(-1, 1), one array per shape (shared by the tests, never written)"""
    key = (batch, ch, fmt, t)
    if key not in _CACHE:
        shape = (batch, t, ch) if fmt == "channels_last" else (batch, ch, t)
        _CACHE[key] = np.random.default_rng(20261126 + 7 * batch + ch).uniform(-1, 1, shape).astype(np.float32)
    return _CACHE[key]


def _run(capfd, layer, x, plain=1, variant=0):
    """(output, launch label, kernel form of the verbose line: "whole" / "plain" / "" for the general kernel)"""
    old = [_ffi.set_option("mel_pw_plain", plain), _ffi.set_option("mel_variant", variant), _ffi.set_option("verbose", 1)]
    try:
        capfd.readouterr()
        out = to_np(layer(x))
        label = _ffi.last_launches()
        err = capfd.readouterr().err
    finally:
        for name, value in zip(("mel_pw_plain", "mel_variant", "verbose"), old):
            _ffi.set_option(name, value)
    lines = re.findall(r"\[kapre_hip\] k_mel_pw<1024,\d+(?:,(\w+))?>:", err)
    assert len(lines) == 1, err
    return out, label, lines[0]


@pytest.mark.parametrize("batch, ch, fmt, t, variant", CASES, ids=IDS)
def test_whole_gives_the_plain_and_the_general_kernels_bits(capfd, batch, ch, fmt, t, variant):
    x = _x(batch, ch, fmt, t)
    kw = dict(n_mels=128, input_data_format=fmt, output_data_format=fmt, **BASE)
    layer = composed.get_melspectrogram_layer(**kw)
    got, label, form = _run(capfd, layer, x, 1, variant)
    ref2, label2, form2 = _run(capfd, layer, x, 2, variant)
    ref0, label0, form0 = _run(capfd, layer, x, 0, variant)
    assert (form, form2, form0) == ("whole", "plain", ""), (form, form2, form0)
    w = W_OF[variant]
    assert label == label2 == "k_mel_pw<1024,w%d>,plain" % w, (label, label2)
    assert label0 == "k_mel_pw<1024,w%d>" % w, label0
    assert got.shape == ref2.shape == ref0.shape
    assert np.array_equal(got, ref2) and np.array_equal(got, ref0)
    if variant == 7:                                               # once per shape
        assert_close(got, o.kapre_melspectrogram(x, **kw))


# launches outside the whole-frames conditions under the default "mel_pw_plain" 1: (name, kernel form, layer keywords)
OTHERS = [
    ("pad_end", "plain", dict(n_mels=128, pad_end=True)),
    ("pad_begin", "plain", dict(n_mels=128, pad_begin=True)),
    ("mels96", "", dict(n_mels=96)),
    ("mels40", "", dict(n_mels=40)),
    ("mels200", "", dict(n_mels=200)),
    ("decibel", "", dict(n_mels=128, return_decibel=True)),
]


@pytest.mark.parametrize("name, form, extra", OTHERS, ids=[c[0] for c in OTHERS])
def test_routes_that_do_not_take_it(capfd, name, form, extra):
    x = _x(3, 1, "channels_last", T10 + 17)
    kw = dict(input_data_format="channels_last", output_data_format="channels_last", **BASE, **extra)
    got, label, got_form = _run(capfd, composed.get_melspectrogram_layer(**kw), x)
    assert got_form == form, (got_form, label)
    assert "k_mel_pw<1024" in label and (",plain" in label) == (form == "plain"), label
    want = o.kapre_melspectrogram(x, **kw)
    (assert_db_close if extra.get("return_decibel") else assert_close)(got, want)


def test_value_two_is_accepted_and_one_stays_the_default():
    assert _ffi.set_option("mel_pw_plain", 2) == 1                 # (returns the previous value)
    assert _ffi.set_option("mel_pw_plain", 1) == 2
