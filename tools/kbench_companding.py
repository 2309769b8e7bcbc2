#!/usr/bin/env python3
"""Kernel times of the mu-law kernels and of ConcatenateFrequencyMap (kapre_amd/csrc/kpr_companding_kernels.h) on an MI355X
-> profiles/companding_times.md.

Method: every variant is a hipGraph of repeated launches into buffers that exist, timed with HIP events on
the launch stream; the median of 3 replays after about half a second of continuous replay.  Two block sizes: one that stays in
the Infinity Cache (256 x 83 x 128 elements, 10.9 MB per stream) and one that does not (2048 x 998 x 80, 654 MB per stream).
Beside each kernel, in the same process and alternating with it inside every timed round: a plain device-to-device copy
(Tensor.copy_) that moves the SAME number of bytes (read + written), the yardstick.

    python tools/kbench_companding.py [--out FILE] [--commit HASH]        needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from kapre_amd import _ffi  # noqa: E402

Q = 256
BLOCKS = [("fits the Infinity Cache", (256, 83, 128), 100), ("exceeds it", (2048, 998, 80), 10)]


def capture(step, steps):
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        step()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(steps):
                step()
    torch.cuda.synchronize()
    return graph, stream


def replay_us(graph, stream, steps):
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        graph.replay()
        e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def measure(pair, steps, settle_s=0.5, rounds=3):
    """pair: {name: step} -> {name: us per step}; the entries alternate inside every round"""
    graphs = {k: capture(f, steps) for k, f in pair.items()}
    first = max(replay_us(*g, steps) for g in graphs.values())
    for g in graphs.values():
        for _ in range(max(2, int(settle_s * 1e6 / max(first * steps, 1.0) / len(graphs)))):
            g[0].replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(replay_us(*g, steps))
    return {k: statistics.median(v) for k, v in times.items()}


def variants(b, t, f):
    """name -> (kernel step, bytes moved per step); buffers are created by the caller of the returned factory"""
    dev = torch.device("cuda", torch.cuda.current_device())
    n = b * t * f

    def mu(name, src_dtype, out_dtype, with_g=False):
        def make():
            src = (torch.rand(n, device=dev) * 2 - 1) if name == "kpr_mu_law_encode_f32" else \
                torch.randint(0, Q, (n,), device=dev, dtype=torch.int32).to(src_dtype)
            out = torch.empty(n, dtype=out_dtype, device=dev)
            g = torch.randn(n, device=dev) if with_g else None
            args = (_ffi.ptr(src),) + ((_ffi.ptr(g),) if with_g else ()) + (n, Q, _ffi.ptr(out))
            return (lambda: _ffi._call(name, dev, *args)), (src, out, g)
        return make, (12 if with_g else 8) * n

    def fmap(c, fmt, backward=False):
        def make():
            cin, cout = (c + 1, c) if backward else (c, c + 1)
            x = torch.randn(_ffi.shape_of(fmt, b, cin, t, f), device=dev)
            out = torch.empty(_ffi.shape_of(fmt, b, cout, t, f), device=dev)
            name = "kpr_freq_map_concat_bwd_f32" if backward else "kpr_freq_map_concat_f32"
            args = (_ffi.ptr(x), b, c, t, f, _ffi.layout(fmt), _ffi.ptr(out))
            return (lambda: _ffi._call(name, dev, *args)), (x, out)
        return make, 4 * n * (2 * c + 1)

    return {
        "mu-law encode (f32 -> i32)": mu("kpr_mu_law_encode_f32", torch.float32, torch.int32),
        "mu-law decode (i32 -> f32)": mu("kpr_mu_law_decode_i32", torch.int32, torch.float32),
        "mu-law decode (f32 -> f32)": mu("kpr_mu_law_decode_f32", torch.float32, torch.float32),
        "mu-law decode backward": mu("kpr_mu_law_decode_bwd_f32", torch.float32, torch.float32, with_g=True),
        "frequency map, channels_last, C = 1": fmap(1, "channels_last"),
        "frequency map, channels_last, C = 3": fmap(3, "channels_last"),
        "frequency map, channels_first, C = 1": fmap(1, "channels_first"),
        "frequency map, channels_first, C = 3": fmap(3, "channels_first"),
        "frequency map backward, channels_last, C = 1": fmap(1, "channels_last", backward=True),
        "frequency map backward, channels_first, C = 1": fmap(1, "channels_first", backward=True),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "companding_times.md"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    _ffi.require_gpu()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    lines = ["# Companding / frequency-map kernel times (tools/kbench_companding.py)", "",
             "%s, torch %s, shader clock %.0f MHz under load, commit %s.  Every row: a hipGraph of repeated launches into buffers "
             "that exist, HIP events on the launch stream, median of 3 after about 0.5 s of continuous replay, in µs per launch; "
             "the copy is `Tensor.copy_` of the same number of bytes (read + written), captured and timed alternately with the "
             "kernel.  quantization_channels = %d." % (torch.cuda.get_device_name(), torch.__version__, _ffi.sclk_mhz(),
                                                      commit or "(unknown)", Q), ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    for label, (b, t, f), steps in BLOCKS:
        lines += ["## %d × %d × %d elements (%.1f MB per stream; %s), %d launches per graph" % (b, t, f, 4e-6 * b * t * f, label, steps),
                  "", "| kernel | MB moved | kernel µs | GB/s | copy µs | GB/s | kernel / copy |", "|---|---|---|---|---|---|---|"]
        for name, (make, nbytes) in variants(b, t, f).items():
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
