"""The fused mel kernel (k_mel_pw, n_fft 2048: one frame per wave and ticket) gives the same bits for a waveform wherever it
sits in the batch.  Moving an item between batch positions and batch sizes moves its frames between "first ticket of a wave"
(prologue fetch), "later ticket" (fetch in the frame loop), and interior / edge frames, and covers runs shorter than the
sixteen waves of a workgroup (batch 1)."""
import numpy as np
import pytest

import kapre_amd as kapre

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 17, 64, 256)
N_WAVES = 5
T = 22050


def _pool(ch):
    rng = np.random.default_rng(7 + ch)
    return rng.uniform(-1, 1, (N_WAVES, T, ch)).astype(np.float32)


def _run(layer, batch_tl, fmt):
    x = batch_tl if fmt == "channels_last" else np.ascontiguousarray(batch_tl.transpose(0, 2, 1))
    return layer(x).cpu().numpy()


@pytest.mark.parametrize("fmt,ch,db,pad", [
    ("channels_last", 1, False, False),
    ("channels_last", 1, False, True),
    ("channels_first", 1, True, True),
    ("channels_first", 3, False, True),
    ("channels_last", 2, True, False),
    ("channels_last", 3, False, True),
])
def test_rows_independent_of_batch_position(fmt, ch, db, pad):
    kw = dict(n_fft=2048, hop_length=512, sample_rate=44100, n_mels=128, return_decibel=db, pad_end=pad,
              input_data_format=fmt, output_data_format=fmt)
    layer = kapre.get_melspectrogram_layer(**kw)
    pool = _pool(ch)
    ref = [_run(layer, pool[i:i + 1], fmt)[0] for i in range(N_WAVES)]
    filler = np.random.default_rng(99).uniform(-1, 1, (1, T, ch)).astype(np.float32)
    for b in BATCHES:
        batch = np.repeat(filler, b, axis=0)
        where = {}
        for i in range(min(N_WAVES, b)):
            pos = (i * 37 + b // 2) % b
            while pos in where.values():
                pos = (pos + 1) % b
            where[i] = pos
            batch[pos] = pool[i]
        out = _run(layer, batch, fmt)
        for i, pos in where.items():
            assert np.array_equal(out[pos], ref[i]), "batch %d, waveform %d at position %d" % (b, i, pos)
