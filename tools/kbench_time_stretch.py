#!/usr/bin/env python3
"""Kernel times of the phase vocoder (kapre_amd/csrc/kpr_time_stretch_kernels.h) on an MI355X -> profiles/time_stretch_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; beside each kernel, alternating with it inside every timed round, a plain
device-to-device copy (Tensor.copy_) of the bytes the operation has to move: 8 (frames_in + frames_out) columns, the input read
once and the output written once.  The span form reads every input row once; the general form reads two rows per output frame
(at rate 1.25: 1.6 input rows per row of the input) -- its ratio to the copy carries that by construction.
Blocks: the complex spectrogram of the cfg4 shape of bench.py (n_fft 1024: 434 frames of 513 bins, one channel), 128 clips
(from DRAM) and 8 clips (stays in the Infinity Cache), rates 0.8 and 1.25, both layouts with one channel, and channels_last
with two channels (inner = 1026: the 16-byte accesses).

    python tools/kbench_time_stretch.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from kapre_amd import _ffi, backend  # noqa: E402
from kbench_companding import measure  # noqa: E402

FRAMES, BINS = 434, 513
RATES = (0.8, 1.25)
SHARES_HEADING = "## Error shares"
# (label, clips, launches per graph)
BLOCKS = [("the cfg4 spectrogram, from DRAM", 128, 10), ("stays in the Infinity Cache", 8, 100)]
# (name, data format, channels)
LAYOUTS = [("channels_first, 1 channel (inner 513: 8-byte accesses)", "channels_first", 1),
           ("channels_last, 1 channel (inner 513: 8-byte accesses)", "channels_last", 1),
           ("channels_last, 2 channels (inner 1026: 16-byte accesses)", "channels_last", 2)]


def make_step(fmt, b, c, rate, dev):
    """(step, tensors kept alive, bytes of input + output)"""
    x = torch.view_as_complex(torch.randn(_ffi.shape_of(fmt, b, c, FRAMES, BINS) + (2,), device=dev))
    idx, alpha = backend.time_stretch_table(FRAMES, rate)
    idx_d, alpha_d = torch.from_numpy(idx).to(dev), torch.from_numpy(alpha).to(dev)
    outer, inner = (b, BINS * c) if fmt == "channels_last" else (b * c, BINS)
    out = torch.empty(_ffi.shape_of(fmt, b, c, len(idx), BINS), dtype=torch.complex64, device=dev)
    args = (_ffi.ptr(x), outer, FRAMES, len(idx), inner, _ffi.ptr(idx_d), _ffi.ptr(alpha_d), _ffi.ptr(out), _ffi.ptr(None))
    return (lambda: _ffi._call("kpr_time_stretch_c64", dev, *args)), (x, out, idx_d, alpha_d), 8 * (FRAMES + len(idx)) * outer * inner


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "time_stretch_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    rows_per_wave, waves = _ffi.time_stretch_plan(FRAMES, BINS)
    lines = ["# TimeStretch kernel times (tools/kbench_time_stretch.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per launch; "
             "the copy is `Tensor.copy_` of 8 (frames_in + frames_out) columns bytes, captured and timed alternately with the "
             "kernel.  %d input frames of %d bins, standard normal bins; time tiling: %d output frames per wave, %d waves per "
             "workgroup.  Rate 0.8 runs the span form (every input row converted once), rate 1.25 the general form (two rows "
             "per output frame)."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)", FRAMES, BINS, rows_per_wave,
                waves), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, clips, steps in BLOCKS:
        lines += ["## %d clips (%s), %d launches per graph" % (clips, label, steps), "",
                  "| layout | rate | frames out | launched | copy MB | kernel µs | copy MB / kernel µs, GB/s | copy µs | GB/s | kernel / copy |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for name, fmt, c in LAYOUTS:
            for rate in RATES:
                step, keep, nbytes = make_step(fmt, clips, c, rate, dev)
                step()
                launched = _ffi.last_launches()
                src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
                dst = torch.empty_like(src)
                res = measure({"kernel": step, "copy": lambda: dst.copy_(src)}, steps)
                row = "| %s | %g | %d | `%s` | %.1f | %.1f | %.0f | %.1f | %.0f | %.2f |" % (
                    name, rate, keep[1].shape[2 if fmt == "channels_first" else 1], launched, nbytes / 1e6, res["kernel"],
                    nbytes / res["kernel"] / 1e3, res["copy"], nbytes / res["copy"] / 1e3, res["kernel"] / res["copy"])
                lines.append(row)
                print(row, flush=True)
                del step, keep, src, dst
                torch.cuda.empty_cache()
        lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if os.path.exists(args.out):                         # the error shares below the tables come from the GPU tests: kept
        old = open(args.out).read()
        if SHARES_HEADING in old:
            lines.append(old[old.index(SHARES_HEADING):].rstrip("\n"))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
