#!/usr/bin/env python3
"""Kernel times of the augmentation layers (kapre_amd/augmentation.py) on an MI355X -> profiles/augment_times.md.

Method: DESIGN section 6 (`kernel_us`): a hipGraph of 100 steps, HIP events on the launch stream, the median of 3 replays after
about 1 s of continuous replay, a same-buffer and a rotating figure (consecutive steps on 5 distinct input and output buffers).
Per block (items x frames x bins), in one process, the variants alternating inside every timed round:
  (a) SpecAugment out of place (k_specaug_apply)          (b) in place (the same kernel with out == x)
  (c) a plain copy of the block (Tensor.copy_ into a buffer that exists: the kernel Tensor.clone() runs) -- the yardstick
  (d) the fused log-mel step that produces the block       (e) the same with the in-place mask behind it (draw + apply)
and the draw kernel alone.  Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np, torch
import kapre_amd as kapre
from kapre_amd import _ffi, augmentation

STEPS, NBUF = 100, 5
MASKS = dict(n_time_masks=3, time_mask_param=10, n_freq_masks=4, freq_mask_param=5)
# items, frames, bins, and the front end whose fused launch writes such a block (waveform length, n_fft, hop, sample rate)
BLOCKS = [(256, 83, 128, (44100, 2048, 512, 44100)),
          (256, 998, 80, (160000, 400, 160, 16000)),
          (2048, 998, 80, (160000, 400, 160, 16000))]


def capture(step, rotating):
    """hipGraph of STEPS calls of step(i); i walks the NBUF buffer sets when `rotating`, stays 0 otherwise"""
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        for i in range(NBUF):
            step(i)                                      # every buffer set once: plans, workspaces, code objects
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            for k in range(STEPS):
                step(k % NBUF if rotating else 0)
    torch.cuda.synchronize()
    return graph, stream


def replay_us(graph, stream):
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        graph.replay()
        e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / STEPS


def measure(variants, settle_s=1.0, rounds=3):
    """variants: {name: step(i)} -> {name: (same-buffer us, rotating us)}; the variants alternate inside every round"""
    graphs = {(name, rot): capture(step, rot) for name, step in variants.items() for rot in (False, True)}
    first = replay_us(*next(iter(graphs.values())))
    for g in graphs.values():                            # about settle_s of continuous replay in all
        for _ in range(max(2, int(settle_s * 1e6 / max(first * STEPS, 1.0) / len(graphs)))):
            g[0].replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(replay_us(*g))
    return {name: (statistics.median(times[(name, False)]), statistics.median(times[(name, True)])) for name in variants}


def block_rows(items, frames, bins, front):
    dev = torch.device('cuda', torch.cuda.current_device())
    nm = dict(n_tm=MASKS['n_time_masks'], n_fm=MASKS['n_freq_masks'])
    gen = torch.Generator(device=dev).manual_seed(items + frames)
    xs = [torch.randn((items, frames, bins, 1), generator=gen, device=dev) * 20 - 40 for _ in range(NBUF)]
    outs = [torch.empty_like(xs[0]) for _ in range(NBUF)]
    state = augmentation.device_state(dev)
    table = _ffi.spec_augment_draw(state, items, nm['n_tm'], nm['n_fm'], frames, bins, MASKS['time_mask_param'],
                                   MASKS['freq_mask_param'])
    t = table.cpu().numpy()
    tmask = np.zeros((items, frames), bool)
    fmask = np.zeros((items, bins), bool)
    for k in range(nm['n_tm'] + nm['n_fm']):
        for it in range(items):
            (tmask if k < nm['n_tm'] else fmask)[it, t[it, k, 0]:t[it, k, 1] + 1] = True
    masked = float((tmask[:, :, None] | fmask[:, None, :]).mean())

    def apply(x, out):
        _ffi._call('kpr_spec_augment_apply_f32', dev, _ffi.ptr(x), _ffi.ptr(out), _ffi.ptr(table), items, nm['n_tm'], nm['n_fm'],
                   frames, bins, -80.0)

    res = measure({
        'a': lambda i: apply(xs[i], outs[i]),
        'b': lambda i: apply(outs[i], outs[i]),
        'c': lambda i: outs[i].copy_(xs[i]),
        'draw': lambda i: _ffi.spec_augment_draw(state, items, nm['n_tm'], nm['n_fm'], frames, bins, MASKS['time_mask_param'],
                                                 MASKS['freq_mask_param']),
    })
    del xs, outs
    torch.cuda.empty_cache()

    t_len, n_fft, hop, sr = front
    mel = lambda: kapre.get_melspectrogram_layer(input_shape=(t_len, 1), n_fft=n_fft, hop_length=hop, sample_rate=sr, n_mels=bins,
                                                 return_decibel=True)
    plain = kapre.Sequential([mel()])
    aug = kapre.Sequential([mel(), kapre.SpecAugment(freq_mask_param=MASKS['freq_mask_param'],
                                                    time_mask_param=MASKS['time_mask_param'],
                                                    n_freq_masks=MASKS['n_freq_masks'], n_time_masks=MASKS['n_time_masks'],
                                                    mask_value=-80.0)])
    ws = [torch.rand((items, t_len, 1), generator=gen, device=dev) * 2 - 1 for _ in range(NBUF)]
    assert tuple(plain(ws[0]).shape) == (items, frames, bins, 1)
    ring_d, ring_e = [None] * NBUF, [None] * NBUF          # the outputs of NBUF consecutive steps stay alive: distinct buffers

    def step_d(i):
        ring_d[i] = plain(ws[i])

    def step_e(i):
        ring_e[i] = aug(ws[i], training=True)

    res.update(measure({'d': step_d, 'e': step_e}))
    return res, masked


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'augment_times.md'))
    args = ap.parse_args()
    _ffi.require_gpu()
    augmentation.set_seed(1)
    lines = ['# SpecAugment kernel times (tools/augment_times.py)', '',
             '%s, torch %s.  hipGraph of %d steps, HIP events on the launch stream, median of 3 after about 1 s of continuous replay; '
             'per cell: same buffers / rotating over %d buffer sets, in µs per step.  Masks: %d x %d frames, %d x %d bins, one table '
             'per block.  GB/s: 8 bytes per element over the rotating time.' % (torch.cuda.get_device_name(), torch.__version__, STEPS, NBUF, MASKS['n_time_masks'],
                                 MASKS['time_mask_param'], MASKS['n_freq_masks'], MASKS['freq_mask_param']), '']
    lines += ['| block | MB | masked | (a) out of place | (b) in place | (c) plain copy | (a)/(c) rot. | (b)/(a) rot. | draw | '
              '(d) log-mel | (e) log-mel + mask | (e) − (d) |', '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for items, frames, bins, front in BLOCKS:
        res, masked = block_rows(items, frames, bins, front)
        nbytes = 4 * items * frames * bins
        cell = lambda k, b=None: '%.1f / %.1f%s' % (res[k][0], res[k][1], '' if b is None else ' (%.0f GB/s)' % (b / res[k][1] / 1e3))
        lines.append('| %d × %d × %d | %.1f | %.1f %% | %s | %s | %s | %.2f | %.2f | %s | %s | %s | %.1f / %.1f |' % (
            items, frames, bins, nbytes / 1e6, 100 * masked, cell('a', 2 * nbytes), cell('b', 2 * nbytes), cell('c', 2 * nbytes),
            res['a'][1] / res['c'][1], res['b'][1] / res['a'][1], cell('draw'), cell('d'), cell('e'),
            res['e'][0] - res['d'][0], res['e'][1] - res['d'][1]))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
