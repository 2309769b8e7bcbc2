#!/usr/bin/env python3
"""Kernel times of Resample forward and backward (kapre_amd/csrc/kpr_resample_kernels.h) on an MI355X -> profiles/resample_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; beside each kernel, alternating with it inside every timed round, a plain
device-to-device copy (Tensor.copy_) that moves the SAME number of bytes (input read + output written).  44100 -> 16000 and
16000 -> 44100, forward and backward (the same kernel with the adjoint table: reads the cotangent of the output, writes that
of the input), mono and channels_last stereo, on a block that stays in the Infinity Cache (64 signals of one second at the
higher rate) and on one of several hundred MB (1024 signals of 2.5 s).

    python tools/kbench_resample.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
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

# (label, signals, seconds, launches per graph)
BLOCKS = [("fits the Infinity Cache", 64, 1.0, 100), ("exceeds it", 1024, 2.5, 10)]
RATES = [(44100, 16000), (16000, 44100)]
FMT = "channels_last"


def variant(orig, new, batch, seconds, channels, backward, dev):
    """(step, buffers kept alive, bytes moved, launch plan line)"""
    fwd, adj = _ffi.resample_plans(orig, new, 6, 0.99, dev)
    t_in = int(round(orig * seconds))
    t_out = backend.resample_length(t_in, orig, new)
    plan, n_src, n_dst = (adj, t_out, t_in) if backward else (fwd, t_in, t_out)
    src = torch.randn((batch, n_src, channels), device=dev)
    dst = torch.empty((batch, n_dst, channels), device=dev)
    args = (_ffi.ptr(src), batch, channels, n_src, _ffi.layout(FMT), _ffi.ptr(plan.table), _ffi.ptr(plan.first), plan.n_phases,
            plan.n_taps, plan.step, n_dst, _ffi.ptr(dst))
    shape = "%d phases × %d taps, tile %d outputs" % (plan.n_phases, plan.n_taps, _ffi.resample_plan(plan.n_phases, plan.n_taps, plan.step))
    return (lambda: _ffi._call("kpr_resample_f32", dev, *args)), (src, dst), 4 * batch * channels * (n_src + n_dst), shape


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lines = ["# Resample kernel times (tools/kbench_resample.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per launch; "
             "the copy is `Tensor.copy_` of the same number of bytes (input read + output written), captured and timed alternately "
             "with the kernel.  channels_last; lowpass_filter_width 6, rolloff 0.99.  The backward pass is the same kernel with the "
             "adjoint table (reads the output's cotangent, writes the input's).  No counter run was made."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)"), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, batch, seconds, steps in BLOCKS:
        lines += ["## %d signals of %.1f s (%s), %d launches per graph" % (batch, seconds, label, steps), "",
                  "| conversion | pass | channels | table | MB moved | kernel µs | GB/s | copy µs | GB/s | kernel / copy |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for orig, new in RATES:
            for backward in (False, True):
                for channels in (1, 2):
                    step, keep, nbytes, shape = variant(orig, new, batch, seconds, channels, backward, dev)
                    a = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
                    b = torch.empty_like(a)
                    res = measure({"kernel": step, "copy": lambda: b.copy_(a)}, steps)
                    row = "| %d → %d | %s | %d | %s | %.1f | %.1f | %.0f | %.1f | %.0f | %.2f |" % (
                        orig, new, "backward" if backward else "forward", channels, shape, nbytes / 1e6, res["kernel"],
                        nbytes / res["kernel"] / 1e3, res["copy"], nbytes / res["copy"] / 1e3, res["kernel"] / res["copy"])
                    lines.append(row)
                    print(row, flush=True)
                    del step, keep, a, b
                    torch.cuda.empty_cache()
        lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
