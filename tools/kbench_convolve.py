#!/usr/bin/env python3
"""Kernel times of Convolve (kapre_amd/csrc/kpr_spec_fir_kernels.h and the three-launch call) on an MI355X ->
profiles/convolve_times.md.

Method: that of tools/kbench_companding.py (its capture / replay / measure are used as they are) -- every variant is a
hipGraph of repeated launches into buffers that exist, timed with HIP events on the launch stream, the median of 3 replays
after about half a second of continuous replay; beside every variant, alternating with it inside every timed round, a plain
device-to-device copy (Tensor.copy_) that moves the SAME number of bytes: for k_spec_fir the input spectrogram read and the
output spectrogram written once, for the whole call (backend.fftconvolve: STFT launch, k_spec_fir, inverse-STFT launch, trim)
the waveform read and the convolved waveform written once.  Impulse responses of 0.5 s and 1 s at 16 kHz at every block length
that takes them, on the blocks of the issue.

    python tools/kbench_convolve.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from kapre_amd import _ffi, backend  # noqa: E402
from kbench_companding import measure  # noqa: E402

# (label, signals, samples, launches per graph of the kernel, of the whole call)
BLOCKS = [("1024 signals of 2.5 s at 16 kHz (exceeds the Infinity Cache)", 1024, 40000, 5, 3),
          ("256 signals of 44100 samples, the headline waveform batch", 256, 44100, 10, 5),
          ("8 signals of 2.5 s at 16 kHz (stays in the Infinity Cache)", 8, 40000, 50, 20)]
IR_LENGTHS = (8000, 16000)                       # 0.5 s and 1 s at 16 kHz


def copy_step(nbytes, dev):
    a = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    return (lambda: b.copy_(a)), (a, b)


def rows_for(batch, t, n, L, steps_k, steps_all, dev, rule_L):
    P = -(-n // L)
    k_in, k_out = -(-(t + L) // L), -(-(t + n - 1) // L)
    rng = np.random.default_rng(1)
    ir = rng.standard_normal(n) * np.exp(-np.arange(n) / (n / 6.0))
    plan = backend.ConvolvePlan(ir, L)
    H = plan.table(dev)
    X = torch.randn((batch, 1, k_in, L + 1), dtype=torch.complex64, device=dev)
    Y = torch.empty((batch, 1, k_out, L + 1), dtype=torch.complex64, device=dev)
    args = (_ffi.ptr(X), batch, k_in, L + 1, 1, _ffi.ptr(H), 1, P, _ffi.ptr(None), batch, _ffi.ptr(Y), k_out)
    kbytes = 8 * batch * (k_in + k_out) * (L + 1)
    kcopy, keep_k = copy_step(kbytes, dev)
    res_k = measure({"fir": lambda: _ffi._call("kpr_spec_fir_c64", dev, *args), "copy": kcopy}, steps_k)
    del X, Y, keep_k
    torch.cuda.empty_cache()
    x = torch.randn((batch, 1, t), device=dev)
    abytes = 4 * batch * (2 * t + n - 1)
    acopy, keep_a = copy_step(abytes, dev)
    res_a = measure({"all": lambda: backend._convolve_run(x, plan, "channels_first", "full"), "copy": acopy}, steps_all)
    del x, keep_a
    torch.cuda.empty_cache()
    flops = 8.0 * batch * k_out * (L + 1) * P                      # 4 FMAs per term
    row = "| %d | %d%s | %d | %d | %.1f | %.1f (%.2f ×) | %.1f | %.1f | %.1f | %.1f (%.2f ×) | %.1f |" % (
        n, L, " (rule)" if L == rule_L else "", P, _ffi.spec_fir_plan(k_out, L + 1, P)[2], kbytes / 1e6, res_k["fir"],
        res_k["fir"] / res_k["copy"], res_k["copy"], flops / res_k["fir"] / 1e6, abytes / 1e6, res_a["all"],
        res_a["all"] / res_a["copy"], res_a["copy"])
    print(row, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "convolve_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    rows, waves, _ = _ffi.spec_fir_plan(1, 1, 1)
    head = ("| IR samples | L | P | bucket | spectrogram MB moved once | k_spec_fir µs (× copy) | copy µs | k_spec_fir TFLOP/s | "
            "waveform MB moved once | whole call µs (× copy) | copy µs |")
    rule = "|---|---|---|---|---|---|---|---|---|---|---|"
    lines = ["# Convolve kernel times (tools/kbench_convolve.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per call.  "
             "k_spec_fir: the middle launch alone on a random spectrogram of the call's shape, against `Tensor.copy_` of its "
             "input read and output written once.  Whole call: `backend.fftconvolve(mode='full')` on one channel, channels_first "
             "-- the STFT launch, k_spec_fir, the inverse-STFT launch and the trim -- against `Tensor.copy_` of the waveform read "
             "and the result written once; its two intermediate spectrograms (complex64, L + 1 bins per L samples, each written and read "
             "again) are about eight times those bytes.  %d output rows per wave, %d waves per workgroup.  (rule): the block length "
             "`backend.convolve_block` picks.  An impulse response that a block length would cut into more than 32 partitions "
             "has no row.  No counter run was made."
             % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(), commit or "(unknown)", rows, waves), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, batch, t, steps_k, steps_all in BLOCKS:
        lines += ["## %s; %d / %d launches per graph" % (label, steps_k, steps_all), "", head, rule]
        for n in IR_LENGTHS:
            for L in backend.CONVOLVE_BLOCKS:
                if -(-n // L) > backend.CONVOLVE_MAX_PARTITIONS:
                    continue
                lines.append(rows_for(batch, t, n, L, steps_k, steps_all, dev, backend.convolve_block(n)))
        lines.append("")
    assert _ffi.device_status(raise_on_error=False) == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
