#!/usr/bin/env python3
"""Kernel and call times of Griffin-Lim (kapre_amd/csrc/kpr_griffin_lim_kernels.h) on an MI355X -> profiles/griffin_lim_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay.  Per block:
  * the projection step k_gl_project with momentum (R, T, mag -> S: 28 bytes per bin) and without (R, mag -> S: 20), alone and
    with the convergence figure (+ k_gl_finish), each alternating with a plain device-to-device copy (Tensor.copy_) that reads
    and writes the same number of bytes;
  * the two transforms alone, kpr_istft_f32 (S -> y) and kpr_stft_f32 (y -> R), on the tensors of the run;
  * whole runs of kpr_griffin_lim_f32 from a given S_0 with n_iter = 0 and n_iter = 8: one iteration is their difference / 8,
    set against the sum of the two stand-alone transforms (the rest is the step, the convergence figure and what the launches
    cost each other);
  * one GriffinLim layer call of 32 iterations (momentum 0.99, random phase) by the wall clock, synchronised, median of 5.
Blocks: n_fft 1024, hop 256, 434 frames of 513 bins, one channel (the cfg4 shape of bench.py), batches 128 (cfg4 itself:
28.5 M bins, from DRAM), 16 (a 16-clip batch) and 8 (1.8 M bins: the step's 50 MB stay in the Infinity Cache).

    python tools/kbench_griffin_lim.py [--out FILE] [--commit HASH] [--batches 128,16,8]        needs a GPU: there is no fallback."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import kapre_amd as kapre  # noqa: E402
from kapre_amd import _ffi, backend  # noqa: E402
from kbench_companding import measure  # noqa: E402

N_FFT, HOP, FRAMES = 1024, 256, 434
K = N_FFT // 2 + 1
FMT = "channels_last"
LABELS = {128: "the cfg4 shape, from DRAM", 16: "a 16-clip batch", 8: "stays in the Infinity Cache"}


def copy_step(nbytes, dev):
    src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    return (lambda: dst.copy_(src)), (src, dst)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "griffin_lim_times.md"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--batches", default="128,16,8")
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    chunk = _ffi.griffin_lim_plan(FRAMES * K)
    lines = ["# Griffin-Lim kernel and call times (tools/kbench_griffin_lim.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Kernel rows: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per launch; "
             "the copy is `Tensor.copy_` of the same number of bytes (read + written), captured and timed alternately with the "
             "kernel.  n_fft %d, hop %d, %d frames x %d bins, one channel, hann window; the step cuts an item into %d chunks of at "
             "most %d bins.  Magnitudes of uniform noise, S_0 with a random phase."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)", N_FFT, HOP, FRAMES, K,
                chunk[1], chunk[0]), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    win = torch.from_numpy(backend.hann_window(N_FFT)).to(dev)
    synth = torch.from_numpy(backend.inverse_stft_window_fn(HOP, backend.hann_window)(N_FFT)).to(dev)
    for batch in [int(b) for b in args.batches.split(",")]:
        n = batch * FRAMES * K
        steps = 4 if n > 8e6 else 20
        x = torch.rand((batch, (FRAMES - 1) * HOP + N_FFT, 1), device=dev) * 2 - 1
        M = kapre.get_stft_magnitude_layer(n_fft=N_FFT, hop_length=HOP, return_decibel=False)(x).contiguous()
        assert tuple(M.shape) == (batch, FRAMES, K, 1)
        _, S0 = _ffi.gl_init(M, FMT, 1.0, _ffi.GL_INIT_RANDOM, kapre.augmentation.device_state(dev))
        T = torch.view_as_complex(torch.randn((batch, FRAMES, K, 1, 2), device=dev))
        R = torch.empty_like(S0)
        S = torch.empty_like(S0)
        sc = torch.empty((batch,), device=dev)
        part = _ffi.workspace(8 * batch * chunk[1], dev)
        wave = torch.empty_like(x)
        g = _ffi.StftGeom(batch, 1, 0, N_FFT, N_FFT, HOP, 0, 0, _ffi.layout(FMT), _ffi.layout(FMT))
        gf = _ffi.StftGeom(batch, 1, x.shape[1], N_FFT, N_FFT, HOP, 0, 0, _ffi.layout(FMT), _ffi.layout(FMT))
        wsi_bytes = int(_ffi.lib().kpr_istft_workspace_bytes(ctypes.byref(g), FRAMES))
        wsi = _ffi.workspace(wsi_bytes, dev)
        ws_bytes = _ffi.griffin_lim_workspace_bytes(g, FRAMES, 0.99, 1.0)
        ws = _ffi.workspace(ws_bytes, dev)
        sc8 = torch.empty((8, batch), device=dev)
        c = 0.99 / 1.99

        def project(mom, with_sc):
            a = (_ffi.ptr(S0), _ffi.ptr(T) if mom else None, _ffi.ptr(M), batch, FRAMES * K, c if mom else 0.0, _ffi.ptr(S),
                 _ffi.ptr(sc) if with_sc else None, _ffi.ptr(part), part.numel())
            return lambda: _ffi._call("kpr_gl_project_f32", dev, *a)

        def run(n_iter):
            a = (_ffi.ptr(M), ctypes.byref(g), FRAMES, _ffi.ptr(win), _ffi.ptr(synth), n_iter, 0.99, 1.0, _ffi.GL_INIT_GIVEN,
                 _ffi.ptr(S0), None, _ffi.ptr(wave), _ffi.ptr(sc8) if n_iter else None, _ffi.ptr(ws), ws.numel())
            return lambda: _ffi._call("kpr_griffin_lim_f32", dev, *a)

        istft = lambda: _ffi._call("kpr_istft_f32", dev, _ffi.ptr(S0), ctypes.byref(g), FRAMES, _ffi.ptr(synth), _ffi.ptr(wave),
                                   _ffi.ptr(wsi), wsi_bytes)
        stft = lambda: _ffi._call("kpr_stft_f32", dev, _ffi.ptr(wave), ctypes.byref(gf), _ffi.ptr(win), _ffi.ptr(R), _ffi.OUT_COMPLEX,
                                  None, 0)
        lines += ["## batch %d: %.2f M bins (%s), %d launches per graph" % (batch, n / 1e6, LABELS.get(batch, ""), steps), "",
                  "| kernel | launched | MB moved | kernel µs | GB/s | copy µs | GB/s | kernel / copy |", "|---|---|---|---|---|---|---|---|"]
        for name, mom, with_sc in (("step with momentum", True, False), ("step with momentum + convergence", True, True),
                                   ("step without momentum", False, False), ("step without momentum + convergence", False, True)):
            nbytes = (28 if mom else 20) * n
            step = project(mom, with_sc)
            step()
            launched = _ffi.last_launches()
            cp, keep = copy_step(nbytes, dev)
            res = measure({"kernel": step, "copy": cp}, steps)
            row = "| %s | `%s` | %.1f | %.1f | %.0f | %.1f | %.0f | %.2f |" % (
                name, launched, nbytes / 1e6, res["kernel"], nbytes / res["kernel"] / 1e3, res["copy"], nbytes / res["copy"] / 1e3,
                res["kernel"] / res["copy"])
            lines.append(row)
            print(row, flush=True)
            del cp, keep
            torch.cuda.empty_cache()
        istft()
        l_istft = _ffi.last_launches()
        stft()
        l_stft = _ffi.last_launches()
        res = measure({"istft": istft, "stft": stft, "run0": run(0), "run8": run(8)}, steps)
        iteration = (res["run8"] - res["run0"]) / 8
        lines += ["", "| per launch / per call | µs |", "|---|---|",
                  "| kpr_istft_f32 alone (`%s`) | %.1f |" % (l_istft, res["istft"]),
                  "| kpr_stft_f32 alone (`%s`) | %.1f |" % (l_stft, res["stft"]),
                  "| kpr_griffin_lim_f32, n_iter 0 (one inverse) | %.1f |" % res["run0"],
                  "| kpr_griffin_lim_f32, n_iter 8, momentum 0.99 | %.1f |" % res["run8"],
                  "| one iteration = (n_iter 8 - n_iter 0) / 8 | %.1f |" % iteration,
                  "| the two transforms alone, summed | %.1f |" % (res["istft"] + res["stft"]),
                  "| iteration / transforms | %.2f |" % (iteration / (res["istft"] + res["stft"]))]
        layer = kapre.GriffinLim(n_fft=N_FFT, hop_length=HOP, n_iter=32, momentum=0.99)
        walls = []
        for i in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            layer(M)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        lines += ["| GriffinLim layer call, 32 iterations, wall clock, median of the last 5 | %.2f ms |" % statistics.median(walls[2:]), ""]
        print("\n".join(lines[-11:]), flush=True)
        del x, M, S0, T, R, S, wave, ws, wsi, part, layer
        torch.cuda.empty_cache()
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
