#!/usr/bin/env python3
"""Kernel times of CMVN forward and backward (kapre_amd/csrc/kpr_cmvn_kernels.h) on an MI355X -> profiles/cmvn_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; beside each kernel, alternating with it inside every timed round, a plain
device-to-device copy (Tensor.copy_) that moves the bytes of the block ONCE per stream the operation has (forward: x in, y
out = 2 streams; backward with norm_vars: y and gy in, gx out = 3).  The resident form moves exactly those bytes; the streamed
form reads its inputs twice (forward 3 block moves against the copy's 2, backward 5 against 3) -- its ratio to the copy
carries that factor by construction.  Blocks, channels_first, one channel:
  16384 x 124 x 80   650 MB per stream, from DRAM, F <= resident_frames: the resident form
  2048 x 998 x 80    654 MB per stream, from DRAM (the block of profiles/pcen_times.md): the streamed form, and k_pcen's
                     forward in the same process for comparison
  256 x 83 x 128     the headline output, 10.9 MB per stream, stays in the Infinity Cache: resident

    python tools/kbench_cmvn.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
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

FMT = "channels_first"
EPS = 1e-5
# (label, shape, launches per graph, rows): a row = (name, kind, norm_vars, want_rstd)
BLOCKS = [
    ("from DRAM, resident", (16384, 124, 80), 10,
     [("forward (x -> y)", "fwd", True, False), ("forward keeping rstd (x -> y, rstd)", "fwd", True, True),
      ("forward, norm_vars off (x -> y)", "fwd", False, False), ("backward (y, rstd, gy -> gx)", "bwd", True, False),
      ("backward, norm_vars off (gy -> gx)", "bwd", False, False)]),
    ("from DRAM, streamed", (2048, 998, 80), 10,
     [("forward (x -> y)", "fwd", True, False), ("backward (y, rstd, gy -> gx)", "bwd", True, False),
      ("k_pcen forward, for comparison (E -> y)", "pcen", True, False)]),
    ("the headline output, in the Infinity Cache, resident", (256, 83, 128), 100,
     [("forward (x -> y)", "fwd", True, False), ("backward (y, rstd, gy -> gx)", "bwd", True, False)]),
]


def make_step(kind, norm_vars, want_rstd, b, t, m, dev):
    """(step, tensors kept alive, streams of block size the operation has)"""
    x = torch.rand((b, 1, t, m), device=dev) * 6 - 60
    geom, stats = _ffi._time_geometry(x.shape, FMT)[:3], (b, 1, m)
    if kind == "pcen":
        x = torch.rand((b, 1, t, m), device=dev)
        params = tuple(torch.from_numpy(backend.pcen_band_table(backend.pcen_parameters(0.025, 0.98, 2.0, 0.5, 1e-6)[:4], m)).to(dev))
        out = torch.empty_like(x)
        args = (_ffi.ptr(x), *_ffi._time_geometry(x.shape, FMT), *(_ffi.ptr(p) for p in params), 1e-6, _ffi.ptr(out), _ffi.ptr(None))
        return (lambda: _ffi._call("kpr_pcen_f32", dev, *args)), (x, out, params), 2
    if kind == "fwd":
        out = torch.empty_like(x)
        rstd = torch.empty(stats, device=dev) if want_rstd else None
        args = (_ffi.ptr(x), *geom, int(norm_vars), EPS, _ffi.ptr(out), _ffi.ptr(rstd))
        return (lambda: _ffi._call("kpr_cmvn_f32", dev, *args)), (x, out, rstd), 2
    gy, gx = torch.randn_like(x), torch.empty_like(x)
    if norm_vars:
        y, rstd = _ffi.cmvn(x, FMT, True, EPS, want_rstd=True)
    else:
        y, rstd = None, None
    del x
    args = (_ffi.ptr(y), _ffi.ptr(rstd), _ffi.ptr(gy), *geom, int(norm_vars), _ffi.ptr(gx))
    return (lambda: _ffi._call("kpr_cmvn_bwd_f32", dev, *args)), (y, rstd, gy, gx), 3 if norm_vars else 2


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cmvn_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    rows_per_wave, waves, resident = _ffi.cmvn_plan(83, 128)
    lines = ["# CMVN kernel times (tools/kbench_cmvn.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per launch; "
             "the copy is `Tensor.copy_` of the block's bytes once per stream of the operation (forward 2, backward 3, backward "
             "without norm_vars 2), captured and timed alternately with the kernel.  `moves` is what the kernel itself reads and "
             "writes in units of one stream: the streamed form reads its inputs twice.  channels_first, one channel, eps 1e-5, "
             "input -60 ± 3; time tiling: %d rows per wave, %d waves per workgroup, resident up to %d frames."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)", rows_per_wave, waves, resident),
             ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, (b, t, m), steps, rows in BLOCKS:
        lines += ["## %d × %d × %d elements (%.1f MB per stream; %s), %d launches per graph" % (b, t, m, 4e-6 * b * t * m, label, steps),
                  "", "| kernel | launched | moves | copy MB | kernel µs | copy MB / kernel µs, GB/s | copy µs | GB/s | kernel / copy |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for name, kind, norm_vars, want_rstd in rows:
            step, keep, streams = make_step(kind, norm_vars, want_rstd, b, t, m, dev)
            step()
            launched = _ffi.last_launches()
            moves = streams if ("res" in launched or kind == "pcen") else 2 * streams - 1
            nbytes = 4 * b * t * m * streams
            src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
            dst = torch.empty_like(src)
            res = measure({"kernel": step, "copy": lambda: dst.copy_(src)}, steps)
            row = "| %s | `%s` | %d | %.1f | %.1f | %.0f | %.1f | %.0f | %.2f |" % (
                name, launched, moves, nbytes / 1e6, res["kernel"], nbytes / res["kernel"] / 1e3, res["copy"],
                nbytes / res["copy"] / 1e3, res["kernel"] / res["copy"])
            lines.append(row)
            print(row, flush=True)
            del step, keep, src, dst
            torch.cuda.empty_cache()
        lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
