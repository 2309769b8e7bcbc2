// kpr_lfilter_kernels.h -- one biquad section along time (signal.LFilter, backend.lfilter): the kernel family whose lanes run
// ALONG time.  Part of the single translation unit kapre_hip.hip.
//
//   y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2],   x, y = 0 for t < 0        (REV: t+1, t+2, zero past the end)
//
// float32 at both ends, float64 in between.  A lane owns kLfLane consecutive samples of one series, a wave 64 lanes' worth, a
// workgroup step kLfWaves waves' worth; a workgroup walks the steps of its part of the series in scan order.  The chunks are
// aligned to the start of the series in memory in both directions: REV walks them from the last to the first and every chunk
// from its last sample to its first, so the ragged chunk is the FIRST one of a reverse scan, where zero input meets a zero state
// and stays exactly zero.  No chunk of a ragged length ever hands a carry on, so every carry matrix is one of a full length.
//
// A lane runs the transposed direct form II, y = b0 x + z1; z1' = b1 x - a1 y + z2; z2' = b2 x - a2 y, whose state z holds the
// history of input and output together.  That choice decides the accuracy: a chunk scanned from the zero state then yields the
// filter's response to the chunk alone, a signal of the output's own size; with the state (y[t-1], y[t-2]) of the direct form it
// would be a ramp hundreds of times larger that has to cancel against the carried part (a high-pass of a step or an impulse).
// A chunk of n samples scanned from z = 0 ends in l; from the carry-in c it ends in M_n^T c + l, M_n being the n-th power of
// the companion matrix (built on the host from the impulse response of 1 / A(z), LfTab).  Between chunks the state travels as
// w = (z1 + sigma z2, -sigma z2), sigma = +-1 by the half plane of the poles, and the matrices are in that basis
// (kpr_host_lfilter.h says why: in the plain basis the entries of M_n are large and cancel).  Per step:
//   1. the lane scans its samples from the zero state;
//   2. the end states combine across the lanes of the wave in six shuffle steps with the matrices of 16 2^k samples (an
//      inclusive scan);
//   3. the waves' totals go through a double-buffered LDS slab, one barrier per step; every wave chains them in order with
//      the matrix of 1024 samples from the step's carry-in, which gives it its own carry-in and, at the end, the next step's;
//   4. the lane's carry-in is (matrix of 16 i samples) (wave carry-in) + (the exclusive scan value of lane i), and the lane runs
//      its samples a second time from there: every y[t] that is stored comes from the sequential arithmetic, only the carries
//      took the chunked route.
// Information flows in scan order only: a sample never reaches an output that precedes it.
//
// MODE: LF_FULL is the above, from a zero carry (whole-signal form: one workgroup per series) or from the carry-in of its
// segment (third launch of the segmented form).  LF_ENDS stops after 3 and stores the zero-state end state of its segment
// (first launch of the segmented form; the last segment in scan order has no successor and returns at once).  k_lfilter_combine
// chains the segments of a series (second launch).  LF_FIR (a1 = a2 = 0) is the three-tap sum from the samples themselves: no scan, no barrier, no carries.
// VEC: 16-byte accesses (contiguous series whose length is a multiple of four, 16-byte aligned pointers).  No atomics.
#pragma once

namespace kpr {

constexpr int kLfLane = 16;                                   // samples a lane owns per step
constexpr int kLfWaves = 4;                                   // waves of a workgroup
constexpr int kLfWaveSamples = 64 * kLfLane;                  // 1024
constexpr int kLfStep = kLfWaves * kLfWaveSamples;            // 4096: samples of one workgroup step
constexpr int kLfSegSteps = 2;                                // steps of one segment of the segmented form
constexpr int kLfSeg = kLfSegSteps * kLfStep;                 // 8192

enum { LF_FULL = 0, LF_ENDS = 1, LF_FIR = 2 };

// the carry matrices of one section, row-major (m00, m01, m10, m11): s' = M s
struct LfTab {
    double lane[64][4];          // of 16 i samples (all: transposed, in the carried basis): what lane rank i applies to its wave's carry-in
    double scan[6][4];           // of 16 2^k samples: shuffle step k of the wave's scan
    double wave[4];              // of 1024 samples
    double seg[4];               // of 8192 samples: k_lfilter_combine
};

struct LfArgs {
    const float* x;
    float* out;
    double* ends;                // LF_ENDS: (series, n_seg, 2) zero-state end states
    const double* carry;         // LF_FULL: (series, n_seg, 2) carry-ins, NULL: zero
    double b0, b1, b2, na1, na2; // na = -a
    double sigma;                // +-1: carries are (z1 + sigma z2, -sigma z2)
    int len;                     // samples of a series
    int stride;                  // elements between consecutive samples
    int channels;
    long long item, chan;        // elements between batch items / between the channels of one
    int n_seg, seg_steps;        // workgroups per series and the steps each walks
    LfTab tab;
};

KPR_DEV void lf_apply(const double* __restrict__ m, double p1, double p2, double& l1, double& l2) {
    l1 = fma(m[0], p1, fma(m[1], p2, l1));
    l2 = fma(m[2], p1, fma(m[3], p2, l2));
}

// one sample of the transposed direct form II: the output, and the state moved on
KPR_DEV double lf_sample(const LfArgs& a, double x, double& z1, double& z2) {
    const double y = fma(a.b0, x, z1);
    z1 = fma(a.b1, x, fma(a.na1, y, z2));
    z2 = fma(a.b2, x, a.na2 * y);
    return y;
}

template <bool VEC, bool REV, int MODE>
__global__ __launch_bounds__(64 * kLfWaves) void k_lfilter(const LfArgs a) {
    constexpr int L = kLfLane, W = kLfWaves;
    __shared__ double slab[2][W][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int series = blockIdx.x / a.n_seg, seg = blockIdx.x - series * a.n_seg;
    if (MODE == LF_ENDS && seg == (REV ? 0 : a.n_seg - 1)) return;               // nothing follows it
    const long long base = (long long)(series / a.channels) * a.item + (long long)(series % a.channels) * a.chan;
    const float* __restrict__ x = a.x + base;
    float* __restrict__ out = a.out + base;
    const int n_steps = (a.len + kLfStep - 1) / kLfStep;
    const int st_lo = seg * a.seg_steps, st_hi = min(st_lo + a.seg_steps, n_steps);
    const int lr = REV ? 63 - lane : lane, wr = REV ? W - 1 - wave : wave;       // ranks in scan order

    double c1 = 0.0, c2 = 0.0;                                                   // the step's carry-in
    if constexpr (MODE == LF_FULL)
        if (a.carry) {
            c1 = a.carry[2 * (long long)blockIdx.x];
            c2 = a.carry[2 * (long long)blockIdx.x + 1];
        }

    for (int j = 0; j < st_hi - st_lo; ++j) {
        const int step = REV ? st_hi - 1 - j : st_lo + j;
        const int t0 = step * kLfStep + tid * L;
        // the lane's samples in memory order, zero outside the series
        float xv[L];
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < L; k += 4) {
                float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (t0 + k < a.len) q = *reinterpret_cast<const float4*>(x + t0 + k);
                xv[k] = q.x; xv[k + 1] = q.y; xv[k + 2] = q.z; xv[k + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < L; ++k) xv[k] = t0 + k < a.len ? x[(long long)(t0 + k) * a.stride] : 0.0f;
        }
        float o[L];                                                              // scan order (q = 0: the lane's first sample of the scan)
        if constexpr (MODE == LF_FIR) {
            // the two samples that precede the lane's in scan order, zero outside the series
            const int tp1 = REV ? t0 + L : t0 - 1, tp2 = REV ? t0 + L + 1 : t0 - 2;
            const float xp1 = (tp1 >= 0 && tp1 < a.len) ? x[(long long)tp1 * a.stride] : 0.0f;
            const float xp2 = (tp2 >= 0 && tp2 < a.len) ? x[(long long)tp2 * a.stride] : 0.0f;
#pragma unroll
            for (int q = 0; q < L; ++q) {
                const double s0 = (double)xv[REV ? L - 1 - q : q];
                const double s1 = (double)(q >= 1 ? xv[REV ? L - q : q - 1] : xp1);
                const double s2 = (double)(q >= 2 ? xv[REV ? L + 1 - q : q - 2] : (q == 1 ? xp1 : xp2));
                o[q] = (float)fma(a.b2, s2, fma(a.b1, s1, a.b0 * s0));
            }
        } else {
            // 1. the lane's samples from the zero state
            double z1 = 0.0, z2 = 0.0;
#pragma unroll
            for (int q = 0; q < L; ++q) lf_sample(a, (double)xv[REV ? L - 1 - q : q], z1, z2);
            double l1 = z1 + a.sigma * z2, l2 = -a.sigma * z2;
            // 2. inclusive scan over the lanes of the wave
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int d = 1 << k;
                const double p1 = REV ? __shfl_down(l1, d) : __shfl_up(l1, d);
                const double p2 = REV ? __shfl_down(l2, d) : __shfl_up(l2, d);
                double n1 = l1, n2 = l2;
                lf_apply(a.tab.scan[k], p1, p2, n1, n2);
                if (lr >= d) { l1 = n1; l2 = n2; }
            }
            double e1 = REV ? __shfl_down(l1, 1) : __shfl_up(l1, 1);             // exclusive: what precedes the lane in its wave
            double e2 = REV ? __shfl_down(l2, 1) : __shfl_up(l2, 1);
            if (lr == 0) e1 = e2 = 0.0;
            // 3. the waves' totals, chained in scan order from the step's carry-in
            if (lr == 63) {
                slab[j & 1][wr][0] = l1;
                slab[j & 1][wr][1] = l2;
            }
            __syncthreads();
            double w1 = c1, w2 = c2, m1 = c1, m2 = c2;
#pragma unroll
            for (int r = 0; r < W; ++r) {
                if (r == wr) { m1 = w1; m2 = w2; }
                double n1 = slab[j & 1][r][0], n2 = slab[j & 1][r][1];
                lf_apply(a.tab.wave, w1, w2, n1, n2);
                w1 = n1; w2 = n2;
            }
            c1 = w1; c2 = w2;
            if constexpr (MODE == LF_ENDS) continue;
            // 4. the lane's carry-in, and its samples again from there
            const double* __restrict__ ml = a.tab.lane[lr];
            lf_apply(ml, m1, m2, e1, e2);
            z1 = e1 + e2;
            z2 = -a.sigma * e2;
#pragma unroll
            for (int q = 0; q < L; ++q) o[q] = (float)lf_sample(a, (double)xv[REV ? L - 1 - q : q], z1, z2);
        }
        if constexpr (MODE != LF_ENDS) {
            if constexpr (VEC) {
#pragma unroll
                for (int k = 0; k < L; k += 4)
                    if (t0 + k < a.len)
                        *reinterpret_cast<float4*>(out + t0 + k) = REV ? make_float4(o[L - 1 - k], o[L - 2 - k], o[L - 3 - k], o[L - 4 - k])
                                                                       : make_float4(o[k], o[k + 1], o[k + 2], o[k + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < L; ++k)
                    if (t0 + k < a.len) out[(long long)(t0 + k) * a.stride] = o[REV ? L - 1 - k : k];
            }
        }
    }
    if constexpr (MODE == LF_ENDS)
        if (tid == 0) {
            a.ends[2 * (long long)blockIdx.x] = c1;
            a.ends[2 * (long long)blockIdx.x + 1] = c2;
        }
}

// second launch of the segmented form: one lane per series chains the segments' zero-state end states in scan order,
// carry[first] = 0, carry[next] = M_seg carry[this] + ends[this].  The end state of the last segment is never read.
struct LfCombineArgs {
    const double* ends;
    double* carry;
    long long n_series;
    int n_seg, reverse;
    double seg[4];
};

__global__ __launch_bounds__(64) void k_lfilter_combine(const LfCombineArgs a) {
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_series) return;
    double c1 = 0.0, c2 = 0.0;
    for (int j = 0; j < a.n_seg; ++j) {
        const long long at = 2 * (s * a.n_seg + (a.reverse ? a.n_seg - 1 - j : j));
        a.carry[at] = c1;
        a.carry[at + 1] = c2;
        if (j + 1 < a.n_seg) {
            double n1 = a.ends[at], n2 = a.ends[at + 1];
            lf_apply(a.seg, c1, c2, n1, n2);
            c1 = n1; c2 = n2;
        }
    }
}

}  // namespace kpr
