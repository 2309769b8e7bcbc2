"""Kernel times of the MDCT and its inverse (kapre_amd/csrc/kpr_mdct_kernels.h) -> profiles/mdct_times.md.

Forward and inverse at frame lengths 2048 and 512 on the headline batch (256 x 44100 x 1) and on 1024 signals of 2.5 s, Vorbis
window, norm=None, pad_begin and pad_end.  Beside every time, from the same run and alternating with it inside every timed round:
a device copy that reads and writes the same bytes (the waveform's plus the coefficients'), and k_stft at n_fft = N / 2, hop N / 2
on the same waveform -- the same FFT core size, the nearest existing launch (it writes a complex spectrum: twice the bytes).
Every step of a graph works on its own set of buffers, enough sets that a replay walks through more than 512 MB: the figures are
DRAM figures, not Infinity Cache figures.

    python tools/kbench_mdct.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
import argparse
import itertools
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import kapre_amd  # noqa: E402
from kapre_amd import _ffi, backend  # noqa: E402
from kbench_companding import measure  # noqa: E402

NOTES_HEADING = "## From the final ISA"
SHAPES = [("headline batch, 256 × 44100", 256, 44100), ("1024 signals of 2.5 s", 1024, 110250)]
FMT = "channels_first"


def rotating(make_step, sets):
    """step() that takes the next of `sets` buffer sets at every call"""
    steps = itertools.cycle([make_step(i) for i in range(sets)])
    return lambda: next(steps)()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mdct_times.md"))
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
    lines = ["# MDCT / inverse MDCT: kernel times (tools/kbench_mdct.py)", "",
             "%s (%d CUs), torch %s, shader clock %.0f MHz under load; commit %s.  Every row: a hipGraph of launches, each on its own "
             "set of buffers (more than 512 MB per replay), HIP events on the launch stream, median of 3 after about 0.5 s of "
             "continuous replay, in µs per call; the transform, a device copy of the same bytes and `k_stft` at n_fft = N / 2, "
             "hop N / 2 on the same waveform (complex output) are captured and timed alternately.  One channel, Vorbis window, "
             "norm=None, pad_begin and pad_end.  GB/s: the waveform's and the coefficients' bytes over the time.  All times are "
             "measured; no counter run was made."
             % (torch.cuda.get_device_name(), torch.cuda.get_device_properties(dev).multi_processor_count, torch.__version__, sclk,
                commit or "(unknown)"), "",
             "| shape | N | direction | launched | run, lanes | frames | µs | GB/s | copy µs | k_stft µs | / copy | / k_stft |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for (label, b, t), N in itertools.product(SHAPES, (2048, 512)):
        M = N // 2
        frames = _ffi.mdct_frames(t, N, True, True)
        nbytes = 4 * b * (t + frames * M)
        sets = max(2, -(-(512 << 20) // nbytes) + 1)
        w = torch.from_numpy(backend.vorbis_window(N)).to(dev)
        xs = [torch.rand((b, 1, t), device=dev) * 2 - 1 for _ in range(sets)]
        Xs = [torch.empty((b, 1, frames, M), device=dev) for _ in range(sets)]
        ys = [torch.empty((b, 1, t), device=dev) for _ in range(sets)]
        flat = [torch.empty(nbytes // 8, device=dev) for _ in range(2 * sets)]
        stft = kapre_amd.STFT(n_fft=M, hop_length=M, pad_end=True, input_data_format=FMT, output_data_format=FMT)

        def fwd(i):
            a = (_ffi.ptr(xs[i]), b, 1, t, _ffi.layout(FMT), N, _ffi.ptr(w), 0, 0, 1, 1, _ffi.layout(FMT), _ffi.ptr(Xs[i]))
            return lambda: _ffi._call("kpr_mdct_f32", dev, *a)

        def inv(i):
            a = (_ffi.ptr(Xs[i]), b, 1, frames, _ffi.layout(FMT), N, _ffi.ptr(w), 0, 0, 1, t, _ffi.layout(FMT), _ffi.ptr(ys[i]))
            return lambda: _ffi._call("kpr_imdct_f32", dev, *a)

        fwd(0)()
        launched_f = _ffi.last_launches()
        inv(0)()
        launched_i = _ffi.last_launches()
        torch.cuda.synchronize()
        err = float((ys[0] - xs[0]).abs().max())
        assert err < 1e-5, err                                     # the pair reconstructs the waveform
        res = measure({"fwd": rotating(fwd, sets), "inv": rotating(inv, sets),
                       "copy": rotating(lambda i: (lambda: flat[2 * i].copy_(flat[2 * i + 1])), sets),
                       "stft": rotating(lambda i: (lambda: stft(xs[i])), sets)}, sets)
        run, lanes = _ffi.mdct_plan(N)
        for what, launched in (("fwd", launched_f), ("inv", launched_i)):
            row = "| %s | %d | %s | `%s` | %d, %d | %d | %.1f | %.0f | %.1f | %.1f | %.2f | %.2f |" % (
                label, N, "forward" if what == "fwd" else "inverse", launched, run, lanes, frames, res[what],
                nbytes / res[what] / 1e3, res["copy"], res["stft"], res[what] / res["copy"], res[what] / res["stft"])
            lines.append(row)
            print(row, flush=True)
        del xs, Xs, ys, flat
        torch.cuda.empty_cache()
    lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for kept in (args.out, os.path.join(REPO, "profiles", "mdct_times.md")):   # the notes below the table are written by hand: kept
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
