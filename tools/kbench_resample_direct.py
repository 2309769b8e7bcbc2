#!/usr/bin/env python3
"""Kernel times of the table-free resampler (kapre_amd/csrc/kpr_resample_direct_kernels.h) beside the table kernel and a copy,
and of a whole PitchShift call, on an MI355X -> profiles/resample_direct_times.md.

Method: that of tools/kbench_resample.py (kbench_companding's capture / replay / measure are used as they are) -- every variant
is a hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; the direct kernel, the table kernel (where the pair has a table) and a plain
device-to-device copy (Tensor.copy_) of the SAME number of bytes (input read + output written) alternate inside every timed
round.  1024 signals of 2.5 s, mono and channels_last stereo, forward and backward.  The PitchShift row is the whole eager call
(STFT, TimeStretch, InverseSTFT, resample) between two events, the median of 5 after 2 warm-up calls.  The report's last section,
"Static instruction mix", is read from the ISA and kept by hand: a run carries it over unchanged from the report it replaces.

    python tools/kbench_resample_direct.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import kapre_amd as kapre  # noqa: E402
from kapre_amd import _ffi, backend  # noqa: E402
from kbench_companding import measure  # noqa: E402

BATCH, SECONDS, STEPS = 1024, 2.5, 4
# (orig, new, has a table)
RATES = [(44100, 16000, True), (49500, 44100, True), (46722, 44100, True), (50854, 48000, False)]
FMT = "channels_last"
STATIC_HEADING = "## Static instruction mix"          # from here on the report is not written by this tool and survives a run


def variants(orig, new, table, channels, backward, dev):
    """({name: step}, buffers kept alive, bytes moved, shape text)"""
    params = (orig, new, 6, 0.99)
    t_in = int(round(orig * SECONDS))
    t_out = backend.resample_length(t_in, orig, new)
    n_src, n_dst = (t_out, t_in) if backward else (t_in, t_out)
    src = torch.randn((BATCH, n_src, channels), device=dev)
    dst = torch.empty((BATCH, n_dst, channels), device=dev)
    dargs = (_ffi.ptr(src), BATCH, channels, n_src, _ffi.layout(FMT), orig, new, 6, 0.99, int(backward), n_dst, _ffi.ptr(dst))
    steps = {"direct": lambda: _ffi._call("kpr_resample_direct_f32", dev, *dargs)}
    n_taps, tile = _ffi.resample_direct_plan(*params, backward)
    shape = "%d taps, tile %d" % (n_taps, tile)
    keep = [src, dst]
    if table:
        plan = _ffi.resample_plans(*params, dev)[1 if backward else 0]
        targs = (_ffi.ptr(src), BATCH, channels, n_src, _ffi.layout(FMT), _ffi.ptr(plan.table), _ffi.ptr(plan.first), plan.n_phases,
                 plan.n_taps, plan.step, n_dst, _ffi.ptr(dst))
        steps["table"] = lambda: _ffi._call("kpr_resample_f32", dev, *targs)
        shape += "; table %d phases × %d taps = %d KB" % (plan.n_phases, plan.n_taps, plan.n_phases * plan.n_taps * 4 // 1000)
        keep.append(plan)
    return steps, keep, 4 * BATCH * channels * (n_src + n_dst), shape


def pitch_shift_row(dev):
    layer = kapre.PitchShift(44100, 2)
    x = torch.randn((128, 110250, 1), device=dev)
    times = []
    for it in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        layer(x)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            times.append(e0.elapsed_time(e1) * 1e3)
    return "PitchShift(44100, +2), n_fft 2048, 128 × 110 250 × 1: %.0f µs per call (min %.0f, max %.0f), last launch %s" % (
        statistics.median(times), min(times), max(times), _ffi.last_launches())


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_direct_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lines = ["# Table-free resampler kernel times (tools/kbench_resample_direct.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of %d launches into buffers that "
             "exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per launch; the "
             "copy is `Tensor.copy_` of the same number of bytes (input read + output written); direct kernel, table kernel and copy "
             "are captured and timed alternately.  %d signals of %.1f s, channels_last; lowpass_filter_width 6, rolloff 0.99.  The "
             "backward pass is the same kernel with adjoint = 1 (reads the output's cotangent, writes the input's).  All times are "
             "measured; no counter run was made."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)", STEPS, BATCH, SECONDS), "",
             "| conversion | pass | channels | shape | MB moved | direct µs | table µs | copy µs | direct / table | direct / copy |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    dev = torch.device("cuda", torch.cuda.current_device())
    for orig, new, table in RATES:
        for backward in (False, True):
            for channels in (1, 2):
                steps, keep, nbytes, shape = variants(orig, new, table, channels, backward, dev)
                a = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
                b = torch.empty_like(a)
                steps["copy"] = lambda: b.copy_(a)
                res = measure(steps, STEPS)
                row = "| %d → %d | %s | %d | %s | %.1f | %.1f | %s | %.1f | %s | %.2f |" % (
                    orig, new, "backward" if backward else "forward", channels, shape, nbytes / 1e6, res["direct"],
                    "%.1f" % res["table"] if table else "—", res["copy"],
                    "%.2f" % (res["direct"] / res["table"]) if table else "—", res["direct"] / res["copy"])
                lines.append(row)
                print(row, flush=True)
                del steps, keep, a, b
                torch.cuda.empty_cache()
    lines += ["", "## The whole PitchShift call", "", pitch_shift_row(dev), ""]
    print(lines[-2], flush=True)
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    # the section read from the ISA is kept by hand behind the measured ones: carry it over from the file being replaced
    for kept in (args.out, os.path.join(REPO, "profiles", "resample_direct_times.md")):
        if os.path.exists(kept):
            old = open(kept).read()
            if STATIC_HEADING in old:
                lines.append(old[old.index(STATIC_HEADING):].rstrip("\n"))
                lines.append("")
                break
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
