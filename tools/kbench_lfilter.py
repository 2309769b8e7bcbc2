#!/usr/bin/env python3
"""Kernel times of LFilter (kapre_amd/csrc/kpr_lfilter_kernels.h) on an MI355X -> profiles/lfilter_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; beside the forms of the kernel, alternating with them inside every timed
round, a plain device-to-device copy (Tensor.copy_) that moves the SAME number of bytes (input read + output written once).
The 5 Hz high-pass at 48 kHz (a full biquad) and pre-emphasis 0.97 (a pure FIR section, one form), forward and reverse, the
whole-signal form forced, the segmented form forced and the automatic dispatch, on the blocks of the issue; then the sweep over
the number of series that the dispatch threshold (kLfSegmentedBelow, kpr_host_lfilter.h) is read from.

    python tools/kbench_lfilter.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
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

HP5 = backend.lfilter_sections(backend.biquad_sos('highpass', 48000, 5, 0.7071))[0]
PRE = (1.0, -0.97, 0.0, 0.0, 0.0)
# (label, series, samples, channels, layout, launches per graph)
BLOCKS = [("1024 series of 2.5 s at 44.1 kHz (exceeds the Infinity Cache)", 1024, 110250, 1, "channels_first", 5),
          ("the same block as channels_last stereo (exceeds the Infinity Cache)", 1024, 110250, 2, "channels_last", 3),
          ("256 series of 44100 samples, the headline waveform batch (fits the Infinity Cache)", 256, 44100, 1, "channels_first", 50),
          ("16 series of 160000 samples (fits the Infinity Cache)", 16, 160000, 1, "channels_first", 50),
          ("8 series of 160000 samples (fits the Infinity Cache)", 8, 160000, 1, "channels_first", 50)]
SWEEP = [4, 8, 16, 32, 48, 64, 96, 128, 192, 256, 512]          # series of 160000 samples
FORMS = {"whole": 1, "segmented": 2, "automatic": 0}


def make_step(batch, channels, length, fmt, coef, reverse, variant, dev):
    x = torch.randn(_ffi.shape_of(fmt, batch, channels, length), device=dev)
    out = torch.empty_like(x)
    ws_bytes = int(_ffi.lib().kpr_lfilter_workspace_bytes(batch, channels, length, _ffi.layout(fmt)))
    ws = _ffi.workspace(ws_bytes, dev)
    c5 = _ffi._coef5(coef)
    args = (_ffi.ptr(x), batch, channels, length, _ffi.layout(fmt), c5, int(reverse), _ffi.ptr(out), _ffi.ptr(ws), ws_bytes)

    def step():
        old = _ffi.set_option("lfilter_variant", variant)        # read at launch (here: at capture) time
        try:
            _ffi._call("kpr_lfilter_f32", dev, *args)
        finally:
            _ffi.set_option("lfilter_variant", old)
    return step, (x, out, ws, c5)


def rows_for(batch, channels, length, fmt, steps, dev, filters, directions=(False, True)):
    nbytes = 8 * batch * channels * length
    out = []
    for fname, coef in filters:
        fir = coef[3] == 0.0 and coef[4] == 0.0
        for reverse in directions:
            pair, keep = {}, []
            for form, v in FORMS.items():
                if fir and form != "automatic":
                    continue
                pair[form], k = make_step(batch, channels, length, fmt, coef, reverse, v, dev)
                keep.append(k)
            a = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
            b = torch.empty_like(a)
            pair["copy"] = lambda: b.copy_(a)
            res = measure(pair, steps)
            chosen = "fir" if fir else {1: "whole", 2: "segmented"}[_ffi.lfilter_plan(batch, channels, length, fmt)[4]]
            cell = lambda k: "%.1f (%.2f ×)" % (res[k], res[k] / res["copy"]) if k in res else "—"
            row = "| %s | %s | %.1f | %s | %s | %s | %s | %.1f | %.0f |" % (
                fname, "reverse" if reverse else "forward", nbytes / 1e6, cell("whole"), cell("segmented"), cell("automatic"), chosen,
                res["copy"], nbytes / res["copy"] / 1e3)
            out.append((row, res, chosen))
            print(row, flush=True)
            del pair, keep, a, b
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lfilter_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lane, wave, step, seg, _ = _ffi.lfilter_plan(1, 1, 1 << 20, "channels_first")
    head = "| filter | pass | MB moved once | whole µs (× copy) | segmented µs (× copy) | automatic µs (× copy) | automatic runs | copy µs | copy GB/s |"
    rule = "|---|---|---|---|---|---|---|---|---|"
    lines = ["# LFilter kernel times (tools/kbench_lfilter.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per call "
             "(the segmented form's three launches together); the copy is `Tensor.copy_` of the input's bytes read and written once "
             "(what the whole-signal form moves; the segmented form reads the input twice: 1.5 × by construction), captured and "
             "timed alternately with the kernels.  %d samples per lane, %d per wave, %d per workgroup step, %d per segment.  "
             "hp5: the RBJ high-pass at 5 Hz / 48 kHz, Q 0.7071; preemph: y[t] = x[t] - 0.97 x[t-1], a pure FIR section (one form: "
             "no scan).  No counter run was made."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)", lane, wave, step, seg), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, batch, length, channels, fmt, steps in BLOCKS:
        lines += ["## %s, %s, %d launches per graph" % (label, fmt, steps), "", head, rule]
        lines += [r[0] for r in rows_for(batch, channels, length, fmt, steps, dev, (("hp5", HP5), ("preemph", PRE)))]
        lines.append("")
    lines += ["## The threshold: series of 160000 samples, hp5 forward, channels_first, 50 launches per graph", "", head, rule]
    for n in SWEEP:
        for row, res, chosen in rows_for(n, 1, 160000, "channels_first", 50, dev, (("hp5, %d series" % n, HP5),), (False,)):
            lines.append(row)
    lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
