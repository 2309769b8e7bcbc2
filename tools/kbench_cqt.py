#!/usr/bin/env python3
"""Kernel times of the constant-Q transform (kapre_amd/csrc/kpr_cqt_kernels.h) on an MI355X -> profiles/cqt_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay.  The complex output, the magnitude output and a device copy of as many
bytes as the complex launch moves (waveform read + spectrum written) alternate inside every timed round.  Shapes: the default
bank (84 bins from C1 at 22.05 kHz, L = 11339) at hop 512 on the headline batch 256 x 44100 x 1, on 1024 signals of 2.5 s and
on 8 signals.  Arithmetic: useful = 4 sum N_k flop per frame (a real sample times a complex tap, multiply and add); padded =
what the kernel executes, 2 x 16 columns x the taps of every 8-bin tile; both over the float32 matrix peak at the run's own
shader clock, CUs x 256 flop per clock.  The report's last section is read from the ISA and kept by hand.

--adjoint: the backward pass instead (kapre_amd/csrc/kpr_cqt_adj_kernels.h).  The adjoint launch and the forward complex launch
of the same shape alternate inside every timed round, at hop 512 on the three shapes and at hop 256 on the headline batch; the
section "## Adjoint" of the report is written (or replaced), everything else in it is kept.  Executed arithmetic of the adjoint:
2 x 16 x 16 flop per fragment and hop block.

    python tools/kbench_cqt.py [--adjoint] [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
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

SR, HOP = 22050, 512
NOTES_HEADING = "## From the final ISA"
ADJOINT_HEADING = "## Adjoint"
# (label, batch, samples, launches per graph)
SHAPES = [("256 × 44100 × 1 (headline batch)", 256, 44100, 4), ("1024 signals of 2.5 s", 1024, 55125, 2),
          ("8 signals of 44100", 8, 44100, 20)]


def make_step(x, lengths, table, magnitude, dev):
    b, n, _ = x.shape
    frames = _ffi.cqt_frames(n, lengths[0], HOP, False, False)
    out = torch.empty((b, frames, len(lengths), 1), dtype=torch.float32 if magnitude else torch.complex64, device=dev)
    args = (_ffi.ptr(x), b, 1, n, 0, lengths.ctypes.data, len(lengths), _ffi.ptr(table), int(table.numel()), HOP, 0, 0, 0,
            int(magnitude), _ffi.ptr(out))
    return (lambda: _ffi._call("kpr_cqt_f32", dev, *args)), out, frames


def adjoint_section(dev, peak, lengths, kernels):
    """the lines of the report's adjoint section: the adjoint against the forward complex launch of the same shape"""
    useful = 4 * int(lengths.sum())
    lines = [ADJOINT_HEADING + " (`kpr_cqt_adjoint_f32`, tools/kbench_cqt.py --adjoint)", "",
             "The adjoint launch and the forward complex launch of the same shape, captured and timed alternately as above; useful "
             "arithmetic as the forward's, %d flop per frame; executed: 512 flop per fragment and hop block.  All times are measured; "
             "no counter run was made." % useful, "",
             "| shape | hop | frames | hop blocks | launched | plan: blocks per run, rows, items | fragments | table MB | adjoint µs | "
             "forward µs | adjoint / forward | useful / peak | executed / peak |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    fwd_table = torch.from_numpy(_ffi.cqt_pack(lengths, kernels)).to(dev)
    for hop, shapes in ((512, SHAPES), (256, SHAPES[:1])):
        table = torch.from_numpy(_ffi.cqt_pack_adjoint(lengths, kernels, hop)).to(dev)
        nfrag = sum(n for row in _ffi.cqt_adjoint_ranges(lengths, hop) for _, n in row)
        plan = _ffi.cqt_adjoint_plan(lengths, hop)
        for label, batch, n, steps in shapes:
            x = torch.randn((batch, n, 1), device=dev)
            frames = _ffi.cqt_frames(n, lengths[0], hop, False, False)
            g = torch.randn((batch, frames, len(lengths), 1), dtype=torch.complex64, device=dev)
            out, gx = torch.empty_like(g), torch.empty_like(x)
            fwd_args = (_ffi.ptr(x), batch, 1, n, 0, lengths.ctypes.data, len(lengths), _ffi.ptr(fwd_table), int(fwd_table.numel()),
                        hop, 0, 0, 0, 0, _ffi.ptr(out))
            adj_args = (_ffi.ptr(g), batch, 1, n, 0, lengths.ctypes.data, len(lengths), _ffi.ptr(table), int(table.numel()), hop,
                        0, 0, 0, _ffi.ptr(gx))
            fwd = lambda: _ffi._call("kpr_cqt_f32", dev, *fwd_args)
            adj = lambda: _ffi._call("kpr_cqt_adjoint_f32", dev, *adj_args)
            adj()
            launched = _ffi.last_launches()
            res = measure({"adj": adj, "fwd": fwd}, steps)
            blocks = -(-n // hop)
            executed = 512.0 * nfrag * batch * (-(-blocks // plan[0]) * plan[0])          # whole runs are multiplied
            row = "| %s | %d | %d | %d | `%s` | %d, %d, %d | %d | %.2f | %.1f | %.1f | %.2f | %.3f | %.3f |" % (
                label, hop, frames, blocks, launched, plan[0], plan[1], plan[2], nfrag, table.numel() * 4 / 1e6, res["adj"],
                res["fwd"], res["adj"] / res["fwd"], useful * batch * frames / (res["adj"] * 1e-6) / peak,
                executed / (res["adj"] * 1e-6) / peak)
            lines.append(row)
            print(row, flush=True)
            del x, g, out, gx
            torch.cuda.empty_cache()
    return lines + [""]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cqt_times.md"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--adjoint", action="store_true")
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
    lengths, _, kernels = backend.cqt_kernels(SR)
    if args.adjoint:                                              # the section alone: the rest of the report is kept as it is
        section = adjoint_section(dev, peak, lengths, kernels)
        assert _ffi.device_status(raise_on_error=False) == 0
        old = open(os.path.join(REPO, "profiles", "cqt_times.md")).read()
        head, notes = old[:old.index(NOTES_HEADING)], old[old.index(NOTES_HEADING):]
        if ADJOINT_HEADING in head:
            head = head[:head.index(ADJOINT_HEADING)]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(head.rstrip("\n") + "\n\n" + "\n".join(section) + "\n" + notes)
        print("wrote", args.out)
        return
    table = torch.from_numpy(_ffi.cqt_pack(lengths, kernels)).to(dev)
    useful = 4 * int(lengths.sum())
    padded = sum(2 * 16 * -(-(hi - lo) // 16) * 16 for lo, hi in _ffi.cqt_tiles(lengths))
    F, chunk, items = _ffi.cqt_plan(lengths, HOP)
    lines = ["# CQT kernel times (tools/kbench_cqt.py)", "",
             "%s (%d CUs), torch %s, shader clock %.0f MHz under load: float32 matrix peak %.1f Tflop/s; commit %s.  Every row: a "
             "hipGraph of repeated launches into buffers that exist, HIP events on the launch stream, median of 3 after about 0.5 s "
             "of continuous replay, in µs per launch; the complex launch, the magnitude launch and a device copy of the bytes the "
             "complex launch moves are captured and timed alternately.  Default bank (84 bins, L = %d, ΣN = %d), hop %d, one "
             "channel: %d useful and %d executed flop per frame (ratio %.3f), table %.2f MB.  Plan: runs of %d frames, chunk %d, %d "
             "work items.  All times are measured; no counter run was made."
             % (torch.cuda.get_device_name(), cus, torch.__version__, sclk, peak / 1e12, commit or "(unknown)", lengths[0],
                lengths.sum(), HOP, useful, padded, padded / useful, table.numel() * 4 / 1e6, F, chunk, items), "",
             "| shape | frames | launched | complex µs | magnitude µs | copy µs | ns per frame | useful / peak | executed / peak | "
             "magnitude: useful / peak | complex / copy |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for label, batch, n, steps in SHAPES:
        x = torch.randn((batch, n, 1), device=dev)
        cplx, out_c, frames = make_step(x, lengths, table, False, dev)
        mag, out_m, _ = make_step(x, lengths, table, True, dev)
        moved = x.numel() * 4 + out_c.numel() * 8
        src = torch.empty(moved // 8, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        cplx()
        launched = _ffi.last_launches()
        res = measure({"cplx": cplx, "mag": mag, "copy": lambda: dst.copy_(src)}, steps)
        nf = batch * frames
        row = "| %s | %d | `%s` | %.1f | %.1f | %.1f | %.1f | %.3f | %.3f | %.3f | %.1f |" % (
            label, frames, launched, res["cplx"], res["mag"], res["copy"], res["cplx"] * 1e3 / nf,
            useful * nf / (res["cplx"] * 1e-6) / peak, padded * nf / (res["cplx"] * 1e-6) / peak,
            useful * nf / (res["mag"] * 1e-6) / peak, res["cplx"] / res["copy"])
        lines.append(row)
        print(row, flush=True)
        del cplx, mag, out_c, out_m, x, src, dst
        torch.cuda.empty_cache()
    lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for kept in (args.out, os.path.join(REPO, "profiles", "cqt_times.md")):      # the notes below the table are written by hand: kept
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
