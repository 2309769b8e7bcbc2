// kpr_resample_direct_kernels.h -- rational sample-rate conversion without a table (backend.resample(method='direct'),
// kapre_amd.PitchShift): the taps of every output are computed where they are used, so the number of phases does not matter.
// Forward and adjoint in one kernel.  Part of the single translation unit kapre_hip.hip.
//
//   out[i] = s sum_j in[j] w(c (j P - i Q)),   in[j] = 0 outside 0 .. in_len - 1
//   w(t)   = sinc(t) cos^2(pi t / (2 L)) for |t| < L, else 0;   c = rolloff / max(orig, new);   s = rolloff min(orig, new) / orig
//
// with the rates reduced by their gcd; forward (P, Q) = (new, orig), adjoint (orig, new): the same function and the same
// outputs as kpr_resample_kernels.h.  The position of output i is the integer pair i Q = a P + r, 0 <= r < P, in 64 bits:
// a lane divides once per tile and then steps by the launch constants (threads Q) div P and mod P, carrying r in 32 bits.
// Only phi = r / P in [0, 1] becomes a float (rounded once, from a double product).  Every output sums the same window of
// n_taps = 2 H inputs, H = ceil(L max / (rolloff P)): tap k reads in[a - H + 1 + k] at
//
//   x = (float)(k - H + 1) - phi;   t = beta x   (beta = c P <= 1);   tap = |t| < L ? s (sinpi(t) / (pi t)) cospi(t / (2 L))^2 : 0
//
// in float32, t == 0 giving s: a pure function of (i, k, the rate pair) -- not of lane, tile, batch position, layout or channel
// count.  The window holds the support |j P - i Q| < L max / rolloff and at most one input more at either end, whose tap is an
// exact 0.  The sum runs over k in ascending order from 0.0f in FMAs; no atomics: the same inputs give the same bits.
//
// A workgroup of 64 .. 256 lanes owns `per_lane` x threads consecutive outputs of one signal (or of NCH = 2 interleaved
// channels of one, which share every tap).  It stages the one contiguous input span they read into LDS -- coalesced loads,
// interleaved channels taken apart on the way, zeros outside the signal -- and after the one barrier lane l computes the outputs
// l, l + threads, ...: consecutive lanes hold consecutive outputs, the stores are coalesced.  Nothing crosses workgroups, no
// spin waits, every loop bound is a launch constant.  Neighbouring lanes read LDS words Q / P apart: below 1 (up-sampling)
// several lanes share a word, at 2.76 (44100 -> 16000) a read group spreads over three bank rows; with about ninety vector
// instructions per tap between two LDS reads (91 in the compiled loop) that does not show.  The kernel is bound by the vector ALU.
#pragma once

namespace kpr {

constexpr int kRdMaxThreads = 256;
constexpr int kRdMaxPerLane = 4;          // outputs per lane and tile
constexpr int kRdLdsWords = 6144;         // staged samples per channel: 24 KiB, 48 KiB for two channels
constexpr int kRdMaxTaps = 128;

struct ResampleDirectArgs {
    const float* x;
    float* out;
    int P, Q;                           // reduced rates of this direction
    int n_taps, H;                      // n_taps = 2 H
    int in_len, out_len;
    int estride;                        // elements from one sample of a channel to the next (channels_last: C)
    int groups;                         // signals per batch item: C, or C / 2 with NCH = 2
    long long in_item, out_item;        // elements per batch item
    long long in_group, out_group;      // elements from one signal of an item to the next
    int per_lane;                       // outputs per lane
    int tile;                           // outputs per workgroup = threads * per_lane
    int tiles_per_signal;
    int step_a, step_r;                 // threads * Q = step_a * P + step_r
    int lds_stride;                     // LDS words per channel: the span of a tile
    double inv_p;                       // 1 / P
    float beta, scale;                  // c P and s, rounded once
    float inv_2l, lim;                  // 1 / (2 L), L
};

// tap k of an output at phase phi: see the head of the file
__device__ __forceinline__ float rd_tap(float d, float phi, const ResampleDirectArgs& a) {
    const float xk = __fsub_rn(d, phi);
    const float t = __fmul_rn(a.beta, xk);
    const float sp = sinpif(t);
    const float cw = cospif(__fmul_rn(t, a.inv_2l));
    const float den = __fmul_rn(3.14159265358979323846f, t);
    const float sinc = t == 0.0f ? 1.0f : __fdiv_rn(sp, den);
    const float w = __fmul_rn(sinc, __fmul_rn(cw, cw));
    return fabsf(t) < a.lim ? __fmul_rn(a.scale, w) : 0.0f;
}

template <int NCH>
__global__ __launch_bounds__(kRdMaxThreads) void k_resample_direct(ResampleDirectArgs a) {
    extern __shared__ float rd_lds[];
    const int tid = threadIdx.x, n_threads = blockDim.x;
    const int s = blockIdx.x / a.tiles_per_signal, tl = blockIdx.x - s * a.tiles_per_signal;
    const int item_b = s / a.groups, g = s - item_b * a.groups;
    const float* in = a.x + item_b * a.in_item + g * a.in_group;
    float* out = a.out + item_b * a.out_item + g * a.out_group;

    const int i0 = tl * a.tile;                                          // (out_len < 2^30: no overflow)
    const long long a0 = ((long long)i0 * a.Q) / a.P;                    // uniform: the tile's first position
    const long long lo = a0 - a.H + 1;                                   // first staged sample (may be < 0, may lie past in_len)

    for (int w = tid; w < a.lds_stride * NCH; w += n_threads) {
        const int i = w / NCH, ch = w - i * NCH;
        const long long gi = lo + i;
        float v = 0.0f;
        if (gi >= 0 && gi < a.in_len) v = in[(int)gi * a.estride + ch];
        rd_lds[ch * a.lds_stride + i] = v;
    }
    __syncthreads();

    // the one 64-bit division of this lane: i Q = pos P + r
    const long long iq = (long long)(i0 + tid) * a.Q;
    const long long pos = iq / a.P;
    unsigned r = (unsigned)(iq - pos * a.P);
    int rel = (int)(pos - a0);                                           // window start in LDS: (pos - H + 1) - lo
    int i = i0 + tid;
    const float d0 = (float)(1 - a.H);
    for (int m = 0; m < a.per_lane; ++m) {
        const float phi = (float)((double)r * a.inv_p);
        float acc[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) acc[ch] = 0.0f;
        float d = d0;
        for (int k = 0; k < a.n_taps; ++k) {
            const float tap = rd_tap(d, phi, a);
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) acc[ch] = fmaf(tap, rd_lds[ch * a.lds_stride + rel + k], acc[ch]);
            d += 1.0f;
        }
        if (i < a.out_len) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) out[i * a.estride + ch] = acc[ch];
        }
        i += n_threads;
        rel += a.step_a;
        r += (unsigned)a.step_r;                                         // (both below 2^31)
        if (r >= (unsigned)a.P) { r -= (unsigned)a.P; rel += 1; }
    }
}

}  // namespace kpr
