#!/usr/bin/env python3
"""Kernel times of the YIN pitch tracker (kapre_amd/csrc/kpr_yin_kernels.h) on an MI355X -> profiles/yin_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay.  The automatic dispatch (the shared form at these geometries) and the direct
form (option ``yin_variant`` 1, read at capture time) alternate inside every timed round.  Shapes: the headline batch
256 x 44100 x 1, 1024 signals of 2.5 s and 8 clips (stays in the Infinity Cache), at 2048/1024/512 and 1024/512/256
(frame_length / win_length / hop), sr 22050, lags 11 ... 340.  Arithmetic: W (tau_hi + 1) (sample, lag) pairs per frame, one
subtraction and one FMA each = 3 flops; the vector peak is the float32 rate at the run's own shader clock: CUs x 128 lanes x
2 (FMA) flops per clock, what packed fp32 on 64 lanes reaches too.  The report's last section is read from the ISA and kept by hand.

    python tools/kbench_yin.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from kapre_amd import _ffi  # noqa: E402
from kbench_companding import measure  # noqa: E402

SR, TAU_MIN, TAU_HI = 22050.0, 11, 340
NOTES_HEADING = "## From the final ISA"
GEOMETRIES = [(2048, 1024, 512), (1024, 512, 256)]
# (label, batch, samples, launches per graph)
SHAPES = [("256 × 44100 × 1 (headline batch)", 256, 44100, 4), ("1024 signals of 2.5 s", 1024, 55125, 2),
          ("8 clips of 44100 (Infinity Cache)", 8, 44100, 50)]


def make_step(batch, n, geometry, variant, dev):
    """(step, tensors kept alive, frames per signal): the launch under ``yin_variant`` = variant (read when the step runs)"""
    fl, W, hop = geometry
    x = torch.randn((batch, n, 1), device=dev)
    frames = _ffi._frame_count(n, fl, hop, False)
    f0 = torch.empty((batch, frames, 1), device=dev)
    cmnd = torch.empty_like(f0)
    args = (_ffi.ptr(x), batch, 1, n, _ffi.layout("channels_last"), SR, fl, W, hop, TAU_MIN, TAU_HI, 0.1, 0, _ffi.ptr(f0),
            _ffi.ptr(cmnd), None)

    def step():
        old = _ffi.set_option("yin_variant", variant)
        try:
            _ffi._call("kpr_yin_f32", dev, *args)
        finally:
            _ffi.set_option("yin_variant", old)
    return step, (x, f0, cmnd), frames


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "yin_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    dev = torch.device("cuda", torch.cuda.current_device())
    sclk = _ffi.sclk_mhz()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    peak = cus * 128 * 2 * sclk * 1e6                             # float32 FMA flops per second
    lines = ["# YIN kernel times (tools/kbench_yin.py)", "",
             "%s (%d CUs), torch %s, shader clock %.0f MHz under load: float32 vector peak %.1f Tflop/s; commit %s.  Every row: "
             "a hipGraph of repeated launches into buffers that exist, HIP events on the launch stream, median of 3 after about "
             "0.5 s of continuous replay, in µs per launch; the automatic dispatch and the direct form (`yin_variant` 1) are "
             "captured and timed alternately.  sr 22050, lags %d … %d, one channel; a (sample, lag) pair counts 3 flops.  All times "
             "are measured; no counter run was made."
             % (torch.cuda.get_device_name(), cus, torch.__version__, sclk, peak / 1e12, commit or "(unknown)", TAU_MIN, TAU_HI), "",
             "| shape | frame / win / hop | frames | launched | µs | ns per frame | direct µs | direct / automatic | Gpairs/s | "
             "share of vector peak | direct: share |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for label, batch, n, steps in SHAPES:
        for geometry in GEOMETRIES:
            auto, keep_a, frames = make_step(batch, n, geometry, 0, dev)
            direct, keep_d, _ = make_step(batch, n, geometry, 1, dev)
            auto()
            launched = _ffi.last_launches()
            res = measure({"auto": auto, "direct": direct}, steps)
            pairs = batch * frames * geometry[1] * (TAU_HI + 1)
            row = "| %s | %d / %d / %d | %d | `%s` | %.1f | %.1f | %.1f | %.2f | %.0f | %.3f | %.3f |" % (
                label, *geometry, frames, launched, res["auto"], res["auto"] * 1e3 / (batch * frames), res["direct"],
                res["direct"] / res["auto"], pairs / res["auto"] / 1e3, 3 * pairs / (res["auto"] * 1e-6) / peak,
                3 * pairs / (res["direct"] * 1e-6) / peak)
            lines.append(row)
            print(row, flush=True)
            del auto, direct, keep_a, keep_d
            torch.cuda.empty_cache()
    lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for kept in (args.out, os.path.join(REPO, "profiles", "yin_times.md")):      # the notes below the table are written by hand: kept
        if os.path.exists(kept) and NOTES_HEADING in open(kept).read():
            old = open(kept).read()
            lines.append(old[old.index(NOTES_HEADING):].rstrip("\n"))
            lines.append("")
            break
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
