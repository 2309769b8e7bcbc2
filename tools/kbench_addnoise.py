#!/usr/bin/env python3
"""Kernel times of AddNoise (kapre_amd/csrc/kpr_mix_kernels.h) on an MI355X -> profiles/addnoise_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; beside every variant, alternating with it inside every timed round, a plain
device-to-device copy (Tensor.copy_) of the waveform: the same bytes as one read and one write of the batch.  Both forms
(option ``addnoise_variant`` 1 streamed, 2 resident where the item fits), forward and backward, and the draw.

    python tools/kbench_addnoise.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from kapre_amd import _ffi, backend  # noqa: E402
from kbench_companding import measure  # noqa: E402

# (label, batch, samples, channels, layout, launches per graph)
BLOCKS = [("1024 x 40000 x 1 (2.5 s at 16 kHz; 164 MB, exceeds the Infinity Cache)", 1024, 40000, 1, "channels_last", 5),
          ("256 x 44100 x 1, the headline waveform batch (45 MB, stays in the Infinity Cache)", 256, 44100, 1, "channels_last", 10),
          ("128 x 44100 x 1", 128, 44100, 1, "channels_last", 20),
          ("64 x 44100 x 1", 64, 44100, 1, "channels_last", 20),
          ("32 x 44100 x 1", 32, 44100, 1, "channels_last", 50),
          ("16 x 44100 x 1", 16, 44100, 1, "channels_last", 50),
          ("8 x 44100 x 1 (few items)", 8, 44100, 1, "channels_last", 50),
          ("8 x 160000 x 1 (10 s at 16 kHz: above the resident limit)", 8, 160000, 1, "channels_last", 50),
          ("256 x 22050 x 2, channels_last stereo", 256, 22050, 2, "channels_last", 10),
          ("64 x 80000 x 2, channels_last stereo above the resident limit", 64, 80000, 2, "channels_last", 10)]
NOISE_SAMPLES = (160000, 48000, 4099)                   # the bank: three noises of different lengths


def rows_for(batch, t, c, fmt, steps, dev):
    rng = np.random.default_rng(1)
    plan = backend.NoisePlan([rng.standard_normal(n) for n in NOISE_SAMPLES])
    bank, lengths = plan.device(dev)
    state = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    table = _ffi.noise_draw(state, batch, lengths, 5.0, 20.0)
    x = torch.randn(_ffi.shape_of(fmt, batch, c, t), device=dev)
    gy = torch.randn_like(x)
    out = torch.empty_like(x)
    stats = torch.empty((batch, 4), dtype=torch.float64, device=dev)
    stats2 = torch.empty_like(stats)
    ws_bytes = _ffi.add_noise_workspace_bytes(batch, c, t, fmt)
    ws = _ffi.workspace(ws_bytes, dev)
    lay = _ffi.layout(fmt)
    bankargs = (_ffi.ptr(bank), int(bank.shape[0]), int(bank.shape[1]), _ffi.ptr(lengths), _ffi.ptr(table))
    fwd = lambda: _ffi._call("kpr_add_noise_f32", dev, _ffi.ptr(x), batch, c, t, lay, *bankargs, _ffi.ptr(out), _ffi.ptr(stats),
                             _ffi.ptr(ws), ws_bytes)
    bwd = lambda: _ffi._call("kpr_add_noise_bwd_f32", dev, _ffi.ptr(gy), _ffi.ptr(x), batch, c, t, lay, *bankargs, _ffi.ptr(stats),
                             _ffi.ptr(out), _ffi.ptr(stats2), _ffi.ptr(ws), ws_bytes)
    copy = lambda: out.copy_(x)
    limit = _ffi.add_noise_plan(batch, c, t, fmt)[2]
    rows = []
    for v, name in ((1, "streamed"), (2, "resident")):
        if v == 2 and c * t > limit:
            continue
        old = _ffi.set_option("addnoise_variant", v)             # read at launch (here: at capture) time
        try:
            fwd()
            label = _ffi.last_launches()
            res = measure({"fwd": fwd, "bwd": bwd, "copy": copy}, steps)
        finally:
            _ffi.set_option("addnoise_variant", old)
        nbytes = 8.0 * batch * c * t
        row = "| %s | %s | %.1f | %.1f (%.2f ×) | %.1f (%.2f ×) | %.1f | %.0f |" % (
            name, label, nbytes / 1e6, res["fwd"], res["fwd"] / res["copy"], res["bwd"], res["bwd"] / res["copy"], res["copy"],
            nbytes / res["copy"] / 1e3)
        print(row, flush=True)
        rows.append(row)
    draw = measure({"draw": lambda: _ffi._call("kpr_noise_draw", dev, _ffi.ptr(table), batch, int(lengths.shape[0]), _ffi.ptr(lengths),
                                               5.0, 20.0, _ffi.ptr(state))}, steps)["draw"]
    rows.append("")
    rows.append("k_noise_draw of %d items: %.1f µs." % (batch, draw))
    print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "addnoise_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    K, _, limit, _ = _ffi.add_noise_plan(1, 1, 1, 0)
    head = "| form | launches | waveform MB read + written once | forward µs (× copy) | backward µs (× copy) | copy µs | copy GB/s |"
    rule = "|---|---|---|---|---|---|---|"
    lines = ["# AddNoise kernel times (tools/kbench_addnoise.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per call.  "
             "Forward: `kpr_add_noise_f32`; backward: `kpr_add_noise_bwd_f32` (which reads the cotangent AND the input); copy: "
             "`Tensor.copy_` of the waveform, the bytes of one read and one write.  By construction the streamed form reads the "
             "waveform twice (1.5 × the copy's bytes forward, 2 × backward) and the resident form once (1 × forward, 1.5 × "
             "backward); the noise comes from a bank of %s samples that stays in the caches.  Streamed chunk: %d floats; "
             "resident limit: %d floats per item.  A shape above the limit has no resident row.  No counter run was made."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)",
                " + ".join(str(n) for n in NOISE_SAMPLES), K, limit), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, batch, t, c, fmt, steps in BLOCKS:
        lines += ["## %s; %d launches per graph" % (label, steps), "", head, rule]
        lines += rows_for(batch, t, c, fmt, steps, dev)
        lines.append("")
        torch.cuda.empty_cache()
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
