// kpr_resample_kernels.h -- rational sample-rate conversion (kapre_amd.signal.Resample) as a polyphase gather, forward and
// adjoint in one kernel.  Part of the single translation unit kapre_hip.hip.
//
//   out[i] = sum_{k < n_taps} tab[i mod P][k] * in[(i div P) * Q + first[i mod P] + k],   in[.] = 0 outside 0 .. in_len - 1
//
// P = n_phases, Q = step.  Forward: (P, Q) = (new, orig); adjoint: (orig, new) with the adjoint's table (kpr_resample_table in
// kapre_hip.hip, resample_support in kpr_host_ops.h).  Output i = b P + p is "block b, phase p"; all outputs of one phase share a row of the table.
//
// A workgroup of 128 .. 512 lanes (the plan picks the count that leaves the fewest lanes without a work item) owns, for one
// signal (or NCH = 2 interleaved channels of one), `nb` consecutive blocks x `pt` consecutive phases.  It stages the one contiguous input span those outputs read into LDS -- coalesced loads, interleaved
// channels taken apart on the way, zeros outside the signal -- and after the one barrier a lane takes work items
// (phase p, block group bg): the blocks bg, bg + ng, ..., bg + 7 ng of phase p, eight accumulators per channel.  Consecutive
// lanes hold consecutive phases (then consecutive block groups), so with pt == P the eight stores of a wave are each one
// run of consecutive outputs, whatever P is -- P = 1, 2, 3 included, where the lanes of a wave differ in the block alone.
// The taps go by in chunks of eight coefficients held in registers (the row of the table is read once per EIGHT outputs per
// channel, from L2 / L1), the inner step is one LDS read and one FMA; the sum of one output runs over k in ascending order
// from 0.0f, whichever lane and tile it falls in: the same inputs give the same bits.  No atomics, no spin waits, nothing
// crosses workgroups; every loop bound is a launch constant.
//
// What it costs, by the static instruction mix: per eight taps of a work item 64 LDS words (32 ds_read2_b32, 128 bytes per
// clock and CU) against 32 v_pk_fma_f32 and about 40 register moves: the LDS pipe is the one that fills first.  A lane's eight
// coefficients are eight consecutive floats of ITS row, so a wave's table loads are n_taps floats apart -- not coalesced, served
// by L1 / L2 and paid once per eight outputs -- and when down-sampling the LDS words of neighbouring lanes lie Q / P apart
// (2.76 for 44100 -> 16000): the 32 lanes of a read group then spread over about three bank rows, a two-way conflict on some
// banks.  A table of few phases and a long step (48000 -> 8000: one phase, step 6, 73 taps) gets a small tile -- 83 work items
// on 128 lanes, 664 outputs -- because the 4096-word span is the limit; it is correct and not tuned.
#pragma once

namespace kpr {

constexpr int kRsBlocks = 8;            // blocks (outputs of one phase) per work item: the accumulators of a lane
constexpr int kRsChunk = 8;             // coefficients in registers at a time
constexpr int kRsMaxThreads = 512;
constexpr int kRsLdsWords = 4096;       // staged samples per channel: 16 KiB, 32 KiB for two channels -- several workgroups per CU

struct ResampleArgs {
    const float* x;
    float* out;
    const float* tab;                   // (P, n_taps)
    const int* first;                   // (P)
    int P, Q, n_taps;
    int in_len, out_len;
    int estride;                        // elements from one sample of a channel to the next (channels_last: C)
    int groups;                         // signals per batch item: C, or C / 2 with NCH = 2
    long long in_item, out_item;        // elements per batch item
    long long in_group, out_group;      // elements from one signal of an item to the next
    int pt, n_pt;                       // phases per workgroup, phase tiles
    int ng, nb;                         // block groups and blocks per workgroup (nb <= 8 ng)
    int n_blocks;                       // ceil(out_len / P)
    int tiles_per_signal;               // n_pt * ceil(n_blocks / nb)
    int lds_stride;                     // LDS words per channel (>= every span of the launch)
};

template <int NCH>
__global__ __launch_bounds__(kRsMaxThreads) void k_resample(ResampleArgs a) {
    extern __shared__ float rs_lds[];
    const int tid = threadIdx.x, n_threads = blockDim.x;
    const int s = blockIdx.x / a.tiles_per_signal, t = blockIdx.x - s * a.tiles_per_signal;
    const int bt = t / a.n_pt, ptile = t - bt * a.n_pt;
    const int item_b = s / a.groups, g = s - item_b * a.groups;
    const float* in = a.x + item_b * a.in_item + g * a.in_group;
    float* out = a.out + item_b * a.out_item + g * a.out_group;

    const int p0 = ptile * a.pt, p1 = min(p0 + a.pt, a.P) - 1;
    const int b0 = bt * a.nb, nb = min(a.nb, a.n_blocks - b0);
    const int f0 = a.first[p0];
    const int lo = b0 * a.Q + f0;                                       // first staged sample (may be < 0)
    // (first[] rises with the phase: kpr_resample_table; a table that does not stays inside the slab and gives wrong values only)
    const int span = min((nb - 1) * a.Q + a.first[p1] - f0 + a.n_taps, a.lds_stride);

    for (int w = tid; w < span * NCH; w += n_threads) {
        const int i = w / NCH, ch = w - i * NCH;
        const int gi = lo + i;
        float v = 0.0f;
        if (gi >= 0 && gi < a.in_len) v = in[gi * a.estride + ch];
        rs_lds[ch * a.lds_stride + i] = v;
    }
    __syncthreads();

    const int n_items = a.pt * a.ng;
    for (int item = tid; item < n_items; item += n_threads) {
        const int bg = item / a.pt, p = p0 + (item - bg * a.pt);
        if (p > p1 || bg >= nb) continue;
        const float* row = a.tab + p * a.n_taps;
        const int fo = a.first[p] - f0;
        int off[kRsBlocks];
#pragma unroll
        for (int j = 0; j < kRsBlocks; ++j) {
            const int bj = bg + j * a.ng;
            off[j] = (bj < nb ? bj : bg) * a.Q + fo;                    // (a block past the tile repeats block bg; never stored)
        }
        float acc[NCH][kRsBlocks];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int j = 0; j < kRsBlocks; ++j) acc[ch][j] = 0.0f;
        int k = 0;
        for (; k + kRsChunk <= a.n_taps; k += kRsChunk) {
            float c[kRsChunk];
#pragma unroll
            for (int q = 0; q < kRsChunk; ++q) c[q] = row[k + q];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int j = 0; j < kRsBlocks; ++j)
#pragma unroll
                    for (int q = 0; q < kRsChunk; ++q)
                        acc[ch][j] = fmaf(c[q], rs_lds[ch * a.lds_stride + off[j] + k + q], acc[ch][j]);
        }
        for (; k < a.n_taps; ++k) {
            const float c = row[k];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int j = 0; j < kRsBlocks; ++j) acc[ch][j] = fmaf(c, rs_lds[ch * a.lds_stride + off[j] + k], acc[ch][j]);
        }
#pragma unroll
        for (int j = 0; j < kRsBlocks; ++j) {
            const int bj = bg + j * a.ng;
            if (bj < nb) {
                const int m = (b0 + bj) * a.P + p;                      // (b0 + bj < n_blocks: at most out_len + P - 1)
                if (m < a.out_len) {
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) out[m * a.estride + ch] = acc[ch][j];
                }
            }
        }
    }
}

}  // namespace kpr
