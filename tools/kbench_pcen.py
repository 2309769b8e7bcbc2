#!/usr/bin/env python3
"""Kernel times of PCEN forward and backward (kapre_amd/csrc/kpr_pcen_kernels.h) on an MI355X -> profiles/pcen_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; beside each kernel, alternating with it inside every timed round, a plain
device-to-device copy (Tensor.copy_) that moves the SAME number of bytes (read + written).  Two blocks, channels_first:
the headline output 256 x 83 x 128 (10.9 MB per stream, stays in the Infinity Cache) and 2048 x 998 x 80 (654 MB per
stream, does not).  Forward reads E and writes y (with the smoother kept for a backward pass: writes S too); backward reads
E, S and gy and writes gE; the backward pass of a learned PCEN (kpr_pcen_bwd_params_f32: two launches, the second reduces
4 / frames of a block) reads the same and writes gE and the (4, bands) parameter gradients, or the latter alone.

    python tools/kbench_pcen.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
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

BLOCKS = [("fits the Infinity Cache", (256, 83, 128), 100), ("exceeds it", (2048, 998, 80), 10)]
FMT = "channels_first"


def variants(b, t, m, dev):
    params = tuple(torch.from_numpy(backend.pcen_band_table(backend.pcen_parameters(0.025, 0.98, 2.0, 0.5, 1e-6)[:4], m)).to(dev))

    def forward(want_smooth):
        def make():
            x = torch.rand((b, 1, t, m), device=dev)
            out, smooth = torch.empty_like(x), (torch.empty_like(x) if want_smooth else None)
            args = (_ffi.ptr(x), *_ffi._time_geometry(x.shape, FMT), *(_ffi.ptr(p) for p in params), 1e-6, _ffi.ptr(out), _ffi.ptr(smooth))
            return (lambda: _ffi._call("kpr_pcen_f32", dev, *args)), (x, out, smooth)
        return make, 3 if want_smooth else 2

    def backward():
        def make():
            x = torch.rand((b, 1, t, m), device=dev)
            _, smooth = _ffi.pcen(x, FMT, params, 1e-6, want_smooth=True)
            gy, gx = torch.randn_like(x), torch.empty_like(x)
            args = (_ffi.ptr(x), _ffi.ptr(smooth), _ffi.ptr(gy), *_ffi._time_geometry(x.shape, FMT), *(_ffi.ptr(p) for p in params), 1e-6,
                    _ffi.ptr(gx))
            return (lambda: _ffi._call("kpr_pcen_bwd_f32", dev, *args)), (x, smooth, gy, gx)
        return make, 4

    def backward_params(want_gx):
        def make():
            x = torch.rand((b, 1, t, m), device=dev)
            _, smooth = _ffi.pcen(x, FMT, params, 1e-6, want_smooth=True)
            gy, gx = torch.randn_like(x), (torch.empty_like(x) if want_gx else None)
            geom = _ffi._time_geometry(x.shape, FMT)
            gp = torch.empty((4, m), device=dev)
            ws_bytes = int(_ffi.lib().kpr_pcen_bwd_params_workspace_bytes(*geom[:3]))
            ws = _ffi.workspace(ws_bytes, dev)
            args = (_ffi.ptr(x), _ffi.ptr(smooth), _ffi.ptr(gy), *geom, *(_ffi.ptr(p) for p in params), 1e-6, _ffi.ptr(gx),
                    _ffi.ptr(gp), _ffi.ptr(ws), ws_bytes)
            return (lambda: _ffi._call("kpr_pcen_bwd_params_f32", dev, *args)), (x, smooth, gy, gx, gp, ws)
        return make, 4 if want_gx else 3

    return {"forward (E -> y)": forward(False), "forward keeping the smoother (E -> y, S)": forward(True),
            "backward (E, S, gy -> gE)": backward(),
            "backward with parameter gradients (E, S, gy -> gE, g)": backward_params(True),
            "parameter gradients alone (E, S, gy -> g)": backward_params(False)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pcen_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    rows, waves = _ffi.pcen_plan(83, 128)
    lines = ["# PCEN kernel times (tools/kbench_pcen.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per launch; "
             "the copy is `Tensor.copy_` of the same number of bytes (read + written), captured and timed alternately with the "
             "kernel.  channels_first, one channel, default parameters; time tiling: %d rows per wave, %d waves per workgroup."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)", rows, waves), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, (b, t, m), steps in BLOCKS:
        lines += ["## %d × %d × %d elements (%.1f MB per stream; %s), %d launches per graph" % (b, t, m, 4e-6 * b * t * m, label, steps),
                  "", "| kernel | MB moved | kernel µs | GB/s | copy µs | GB/s | kernel / copy |", "|---|---|---|---|---|---|---|"]
        for name, (make, streams) in variants(b, t, m, dev).items():
            nbytes = 4 * b * t * m * streams
            step, keep = make()
            src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
            dst = torch.empty_like(src)
            res = measure({"kernel": step, "copy": lambda: dst.copy_(src)}, steps)
            row = "| %s | %.1f | %.1f | %.0f | %.1f | %.0f | %.2f |" % (
                name, nbytes / 1e6, res["kernel"], nbytes / res["kernel"] / 1e3, res["copy"], nbytes / res["copy"] / 1e3,
                res["kernel"] / res["copy"])
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
