#!/usr/bin/env python3
"""Kernel times of the harmonic-percussive separation (kapre_amd/csrc/kpr_hpss_kernels.h) on an MI355X -> profiles/hpss_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; beside each kernel, alternating with it inside every timed round, a plain
device-to-device copy (Tensor.copy_) of the bytes the operation has to move: the spectrogram read once and both outputs
written once (three times the spectrogram's bytes).
Blocks: the spectrogram of the cfg4 shape of bench.py (n_fft 1024: 434 frames of 513 bins), 128 clips (from DRAM) and 8 clips
(stays in the Infinity Cache); windows (31, 31) and (17, 17), power 2, output 'both' (one tensor of twice the channels), as a
float32 magnitude and as complex64, one channel in both layouts and two interleaved channels in channels_last.

    python tools/kbench_hpss.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
import argparse
import ctypes
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from kapre_amd import _ffi  # noqa: E402
from kbench_companding import measure  # noqa: E402

FRAMES, BINS = 434, 513
WINDOWS = ((31, 31), (17, 17))
NOTES_HEADING = "## From the final ISA"
# (label, clips, launches per graph)
BLOCKS = [("the cfg4 spectrogram, from DRAM", 128, 10), ("stays in the Infinity Cache", 8, 100)]
# (name, data format, channels, complex)
LAYOUTS = [("channels_first, 1 channel, float32", "channels_first", 1, False),
           ("channels_last, 1 channel, float32", "channels_last", 1, False),
           ("channels_first, 1 channel, complex64", "channels_first", 1, True),
           ("channels_last, 2 interleaved channels, float32", "channels_last", 2, False),
           ("channels_last, 2 interleaved channels, complex64", "channels_last", 2, True)]


def make_step(fmt, b, c, cplx, kh, kp, dev):
    """(step, tensors kept alive, bytes of input + both outputs)"""
    shape = _ffi.shape_of(fmt, b, c, FRAMES, BINS)
    x = torch.view_as_complex(torch.randn(shape + (2,), device=dev)) if cplx else torch.randn(shape, device=dev).abs()
    out = torch.empty(_ffi.shape_of(fmt, b, 2 * c, FRAMES, BINS), dtype=x.dtype, device=dev)
    off = (c if fmt == "channels_last" else c * FRAMES * BINS) * out.element_size()
    args = (_ffi.ptr(x), b, c, FRAMES, BINS, _ffi.layout(fmt), kh, kp, 2.0, 1.0, 1.0, 0, _ffi.ptr(out),
            ctypes.c_void_p(out.data_ptr() + off), 2 * c)
    name = "kpr_hpss_c64" if cplx else "kpr_hpss_f32"
    return (lambda: _ffi._call(name, dev, *args)), (x, out), 3 * x.numel() * x.element_size()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hpss_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    tf, tq = _ffi.hpss_plan(FRAMES, BINS)
    lines = ["# HPSS kernel times (tools/kbench_hpss.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per launch; "
             "the copy is `Tensor.copy_` of three times the spectrogram's bytes (read once, two outputs written), captured and "
             "timed alternately with the kernel.  %d frames of %d bins per plane, power 2, margins 1, output 'both'; tile: %d "
             "frames x %d bins per workgroup (%d x %d tiles per plane)."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)", FRAMES, BINS, tf, tq,
                -(-FRAMES // tf), -(-BINS // tq)), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, clips, steps in BLOCKS:
        lines += ["## %d clips (%s), %d launches per graph" % (clips, label, steps), "",
                  "| layout | windows | launched | copy MB | kernel µs | ns per 1000 bins | copy µs | GB/s | kernel / copy |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for name, fmt, c, cplx in LAYOUTS:
            for kh, kp in WINDOWS:
                step, keep, nbytes = make_step(fmt, clips, c, cplx, kh, kp, dev)
                step()
                launched = _ffi.last_launches()
                src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
                dst = torch.empty_like(src)
                res = measure({"kernel": step, "copy": lambda: dst.copy_(src)}, steps)
                row = "| %s | (%d, %d) | `%s` | %.1f | %.1f | %.2f | %.1f | %.0f | %.2f |" % (
                    name, kh, kp, launched, nbytes / 1e6, res["kernel"], res["kernel"] * 1e6 / keep[0].numel(), res["copy"],
                    nbytes / res["copy"] / 1e3, res["kernel"] / res["copy"])
                lines.append(row)
                print(row, flush=True)
                del step, keep, src, dst
                torch.cuda.empty_cache()
        lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if os.path.exists(args.out):                         # the notes below the tables are written by hand: kept
        old = open(args.out).read()
        if NOTES_HEADING in old:
            lines.append(old[old.index(NOTES_HEADING):].rstrip("\n"))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
