"""Kernel times of the filterbank weight gradient (kapre_amd/csrc/kpr_fb_wgrad_kernels.h) -> profiles/fb_wgrad_times.md.

gW = x^T g for the magnitude block of the headline mel launch (256 items x 83 frames = 21 248 rows of 1025 bins -> 128 filters)
and for 1024 clips of 2.5 s (104 frames each), channels_first with one channel and channels_last stereo.  Beside every time, from
the same run and alternating with it inside every timed round: a device copy of the bytes of x and g read once; the forward
plain GEMM (kpr_apply_filterbank_f32, the same dense matrix); torch.matmul(x2d.T, g2d) on the same tensors (channels_first: a
view; channels_last: the views of both channels, added), the path a user has without this kernel.  Arithmetic: useful =
2 rows c n_freq n_filt flop; executed = what the MFMAs multiply, whole chunks of rows x tiles of 64 bins x tiles of 16 filters;
both over the float32 matrix peak at the run's own shader clock, CUs x 256 flop per clock.

    python tools/kbench_fb_wgrad.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
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

N_FREQ, N_FILT = 1025, 128
NOTES_HEADING = "## From the final ISA"
# (label, batch, frames, channels, layout, launches per graph)
SHAPES = [("headline block, 256 × 83 frames", 256, 83, 1, "channels_first", 8),
          ("headline block, stereo", 256, 83, 2, "channels_last", 4),
          ("1024 clips of 2.5 s", 1024, 104, 1, "channels_first", 2),
          ("1024 clips of 2.5 s, stereo", 1024, 104, 2, "channels_last", 1)]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fb_wgrad_times.md"))
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
    peak = cus * 256 * sclk * 1e6                                 # float32 MFMA flops per second
    lines = ["# Filterbank weight gradient: kernel times (tools/kbench_fb_wgrad.py)", "",
             "%s (%d CUs), torch %s, shader clock %.0f MHz under load: float32 matrix peak %.1f Tflop/s; commit %s.  Every row: a "
             "hipGraph of repeated launches into buffers that exist, HIP events on the launch stream, median of 3 after about 0.5 s "
             "of continuous replay, in µs per call; the weight gradient, a device copy of the bytes of x and g, the forward GEMM "
             "(`kpr_apply_filterbank_f32`, dense) and `torch.matmul(x2d.T, g2d)` are captured and timed alternately.  %d bins -> %d "
             "filters.  All times are measured; no counter run was made."
             % (torch.cuda.get_device_name(), cus, torch.__version__, sclk, peak / 1e12, commit or "(unknown)", N_FREQ, N_FILT), "",
             "| shape | layout | rows × c | launched | plan: S, slabs | wgrad µs | copy µs | forward µs | torch.matmul µs | "
             "wgrad / copy | wgrad / torch | useful / peak | executed / peak |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for label, b, t, c, fmt, steps in SHAPES:
        cl = fmt == "channels_last"
        x = torch.randn(_ffi.shape_of(fmt, b, c, t, N_FREQ), device=dev)
        g = torch.randn(_ffi.shape_of(fmt, b, c, t, N_FILT), device=dev)
        w = torch.rand((N_FREQ, N_FILT), device=dev)
        rows = b * t * (1 if cl else c)
        tf, S, n_slabs, passes = _ffi.filterbank_wgrad_plan(rows, N_FREQ, N_FILT, c, fmt)
        ws_bytes = int(_ffi.lib().kpr_filterbank_wgrad_workspace_bytes(rows, N_FREQ, N_FILT, c, _ffi.layout(fmt)))
        ws, gw, y = _ffi.workspace(ws_bytes, dev), torch.empty_like(w), torch.empty_like(g)
        wg_args = (_ffi.ptr(x), _ffi.ptr(g), b, c, t, N_FREQ, N_FILT, _ffi.layout(fmt), _ffi.ptr(ws), ws_bytes, _ffi.ptr(gw))
        fw_args = (_ffi.ptr(x), b, c, t, N_FREQ, _ffi.layout(fmt), _ffi.ptr(w), N_FILT, None, _ffi.ptr(y))
        wgrad = lambda: _ffi._call("kpr_filterbank_wgrad_f32", dev, *wg_args)
        fwd = lambda: _ffi._call("kpr_apply_filterbank_f32", dev, *fw_args)
        if cl:                                                    # (rows, n, c): one strided view per channel
            x3, g3, ref = x.view(rows, N_FREQ, c), g.view(rows, N_FILT, c), torch.empty_like(w)
            mm = lambda: sum(torch.matmul(x3[:, :, k].t(), g3[:, :, k]) for k in range(c))
        else:
            x2, g2, ref = x.view(rows, N_FREQ), g.view(rows, N_FILT), torch.empty_like(w)
            mm = lambda: torch.matmul(x2.t(), g2, out=ref)
        wgrad()
        launched = _ffi.last_launches()
        torch.cuda.synchronize()
        rel = float((gw - mm()).abs().max() / mm().abs().max())
        assert rel < 1e-4, rel                                    # the two paths compute the same matrix
        src = torch.empty((x.numel() + g.numel()), dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        res = measure({"wgrad": wgrad, "copy": lambda: dst.copy_(src), "fwd": fwd, "mm": mm}, steps)
        fold = c if cl else 1                                     # products a row contributes per (f, m)
        useful = 2.0 * rows * fold * N_FREQ * N_FILT
        rows_exec = -(-rows // 16) * 16                           # whole chunks of 16 rows (c <= 2)
        executed = 2.0 * rows_exec * fold * (-(-N_FREQ // tf) * tf) * (-(-N_FILT // 16) * 16)
        row = "| %s | %s | %d × %d | `%s` | %d, %d | %.1f | %.1f | %.1f | %.1f | %.2f | %.2f | %.3f | %.3f |" % (
            label, fmt, rows, c if cl else 1, launched, S, n_slabs, res["wgrad"], res["copy"], res["fwd"], res["mm"],
            res["wgrad"] / res["copy"], res["wgrad"] / res["mm"], useful / (res["wgrad"] * 1e-6) / peak,
            executed / (res["wgrad"] * 1e-6) / peak)
        lines.append(row)
        print(row, flush=True)
        del x, g, w, ws, gw, y, src, dst, ref
        torch.cuda.empty_cache()
    lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for kept in (args.out, os.path.join(REPO, "profiles", "fb_wgrad_times.md")):   # the notes below the table are written by hand: kept
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
