// kpr_yin_kernels.h -- YIN fundamental-frequency tracking of a waveform (kapre_amd.signal.YIN, backend.yin): de Cheveigne &
// Kawahara (2002) steps 1-5 as librosa.yin arranges them, on this library's frames (not centred).  One launch, no atomics, no
// host reads: the same inputs give the same bits.  Part of the single translation unit kapre_hip.hip.
//
// Per series (batch item, channel) x of `time` samples, frame t = x[t hop ... t hop + frame_length), samples past the end 0:
//   d(tau) = sum_{j < W} (x[j] - x[j + tau])^2              tau = 0 ... tau_hi, float32, in this difference form, j ascending
//   c(tau) = sum_{k = 1 .. tau} d(k);   y(0) = 1;   y(tau) = d(tau) tau / c(tau), 1 where c(tau) == 0
//   i in [tau_min, tau_hi) is a trough when i == tau_min and y[i] < y[i+1], or i > tau_min and y[i] < y[i-1] and y[i] <= y[i+1]
//   tau* = the smallest trough with y < threshold, else the smallest index of min y over [tau_min, tau_hi]
//   a = (y+ - y0) + (y- - y0);  b = (y+ - y-) 0.5;  shift = |b| < |a| ? -b / a : 0, and 0 at tau* == tau_min or tau_hi
//   f0 = sr / (float(tau*) + shift);  cmnd = y[tau*]
// every operation rounded to float32 once.  A frame with a d(tau), tau <= tau_hi, that is not finite (a NaN or Inf sample that
// the frame reads, or an overflow) gives NaN twice; no other frame is touched by that sample.
//
// Work split.  A workgroup of 256 lanes owns a run of F consecutive frames of one series (F: kpr_yin_plan) and stages the run's
// sample span, (F - 1) hop + W + tau_hi + 16 floats, in LDS once, the channels_last stride resolved there, zeros past the
// signal's end.  Phase 1 is the arithmetic: a lane takes one unit = (row m, block of R = 8 consecutive lags) at a time and walks j
// in chunks of 8 with a sliding register window -- 8 floats x[j ..] (the same address for the lanes of a row: a broadcast) and 8
// new floats x[j + tau0 + 8 ..] feed 64 subtract / FMA pairs; with hop % 4 == 0 (VEC) the reads are four ds_read_b128.  Two forms:
//   direct   row m is frame m: d_m(tau) summed over the frame's W samples, j ascending;
//   shared   hop divides W: row m is the block sum s(m, tau) = sum_{j < hop} (x[m hop + j] - x[m hop + j + tau])^2, computed once
//            per run, and d_t(tau) = s(t, tau) + s(t + 1, tau) + ... + s(t + W / hop - 1, tau), added in that order in phase 2:
//            F - 1 + W / hop block rows instead of F W / hop.  Nothing is carried from frame to frame.
// Phase 2, one wave per frame, four frames at a time: rows of 64 lags, lag = 64 i + lane (conflict-free); the prefix sum c is a
// wave scan per row (shuffles, fixed order) plus the carry of the rows before; y goes to an LDS row; after a barrier the first
// trough below the threshold is a ballot per row, its fallback a (value, index) minimum with the smaller index on ties; every
// lane refines, lane 0 stores.  The matrix instructions have no use here: per frame the product is a Hankel matrix-vector
// product with no operand shared between frames, and energy minus correlation cancels exactly at the troughs.
#pragma once

namespace kpr {

constexpr int kYinThreads = 256;
constexpr int kYinWaves = kYinThreads / 64;
constexpr int kYinR = 8;                  // lags per unit, samples per chunk
constexpr int kYinMaxRun = 8;             // frames per workgroup at most
constexpr int kYinMaxBlocks = 16;         // W / hop of the shared form at most
constexpr int kYinLdsFloats = 16384;      // 64 KiB: no opt-in, two workgroups per CU

struct YinArgs {
    const float* x;
    float* f0;
    float* cmnd;
    float* curve;                       // (series, frames, tau_hi + 1) or NULL
    long long item, chan;               // the series of x (kpr_series.h)
    long long out_item, out_chan;       // the same for f0 / cmnd, whose series are the frames
    int stride, out_stride;
    int C, time, frames, runs, F;       // runs per series = ceil(frames / F)
    int W, hop, tau_min, tau_hi;
    int nb;                             // shared: W / hop
    int Q, LP;                          // lag blocks per row; floats per row (a multiple of 64)
    int span;                           // staged floats per run
    float thr, sr;
};

template <bool VEC>
KPR_DEV void yin_load8(const float* p, float* r) {
    if constexpr (VEC) {
        const f4 u = *reinterpret_cast<const f4*>(p), v = *reinterpret_cast<const f4*>(p + 4);
        r[0] = u.x; r[1] = u.y; r[2] = u.z; r[3] = u.w; r[4] = v.x; r[5] = v.y; r[6] = v.z; r[7] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = p[k];
    }
}

// one (sample, lag) pair: v_sub_f32 + v_fma_f32
KPR_DEV float yin_term(float a, float b, float acc) {
    const float d = __fsub_rn(a, b);
    return fmaf(d, d, acc);
}

// Compiled without the packed fp32 forms: every pair is two plain vector instructions, whose results do not depend on how the
// vectoriser happens to pair the eight accumulators of a lane.
template <bool SHARED, bool VEC>
__attribute__((target("no-packed-fp32-ops"))) __global__ __launch_bounds__(kYinThreads) void k_yin(YinArgs a) {
    extern __shared__ __align__(16) float yin_lds[];
    float* xs = yin_lds;                                                 // the span
    float* sums = xs + a.span;                                           // rows of LP floats: s(m, .) or d_m(.)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const SeriesUnit u = series_unit(a.runs, a.C);                       // unit: the run
    const float* in = u.at(a.x, a.item, a.chan);
    const auto [t0, fv] = frame_run(u.unit, a.F, a.frames);
    const long long g0 = (long long)t0 * a.hop;

    for (int i = tid; i < a.span; i += kYinThreads) {
        const long long gi = g0 + i;
        xs[i] = gi < a.time ? in[gi * a.stride] : 0.0f;
    }
    __syncthreads();

    // ---- phase 1: the sums of squared differences, one unit per lane and turn ----
    const int rows = SHARED ? fv - 1 + a.nb : fv;
    const int J = SHARED ? a.hop : a.W, J8 = J & ~7;
    for (int u = tid; u < rows * a.Q; u += kYinThreads) {
        const int m = u / a.Q, q = u - m * a.Q;
        const float* xa = xs + m * a.hop;                                // x[j]
        const float* xb = xa + q * kYinR;                                // x[j + tau0]
        float acc[kYinR], w[2 * kYinR], av[kYinR];
#pragma unroll
        for (int r = 0; r < kYinR; ++r) acc[r] = 0.0f;
        yin_load8<VEC>(xb, w);
        for (int j = 0; j < J8; j += 8) {
            yin_load8<VEC>(xa + j, av);
            yin_load8<VEC>(xb + j + 8, w + 8);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj)
#pragma unroll
                for (int r = 0; r < kYinR; ++r) acc[r] = yin_term(av[jj], w[jj + r], acc[r]);
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = w[k + 8];
        }
        for (int j = J8; j < J; ++j) {
            const float aj = xa[j];
#pragma unroll
            for (int r = 0; r < kYinR; ++r) acc[r] = yin_term(aj, xb[j + r], acc[r]);
        }
        float* o = sums + m * a.LP + q * kYinR;                          // (q R + 7 < LP: LP is a multiple of 64 above tau_hi)
#pragma unroll
        for (int r = 0; r < kYinR; ++r) o[r] = acc[r];
    }
    __syncthreads();

    // ---- phase 2: one wave per frame ----
    const int nl = a.tau_hi + 1;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    for (int tb = 0; tb < fv; tb += kYinWaves) {                         // (uniform: every wave reaches the barrier)
        const int t = tb + wave;
        const bool live = t < fv;
        float* yrow = SHARED ? sums + (a.F - 1 + a.nb + wave) * a.LP : sums + t * a.LP;
        bool bad = false;
        if (live) {
            float carry = 0.0f;
            for (int i0 = 0; i0 < nl; i0 += 64) {
                const int tau = i0 + lane;
                float d = 0.0f;
                if (tau < nl) {
                    d = sums[t * a.LP + tau];
                    if (SHARED)
                        for (int k = 1; k < a.nb; ++k) d = __fadd_rn(d, sums[(t + k) * a.LP + tau]);
                    bad |= !(d < inf);
                }
                float v = tau >= 1 ? d : 0.0f;                           // inclusive scan of the row, then the rows before
                for (int o = 1; o < 64; o <<= 1) {
                    const float n = __shfl_up(v, o, 64);
                    if (lane >= o) v = __fadd_rn(v, n);
                }
                const float c = __fadd_rn(carry, v);
                carry = __shfl(c, 63, 64);
                float y = 1.0f;
                if (tau >= 1 && c != 0.0f) y = __fdiv_rn(__fmul_rn(d, (float)tau), c);
                if (tau < nl) yrow[tau] = y;
            }
        }
        __syncthreads();
        if (live) {
            const bool frame_bad = __ballot(bad) != 0ull;
            int best = -1;
            for (int i0 = a.tau_min; i0 < a.tau_hi && best < 0; i0 += 64) {
                const int tau = i0 + lane;
                bool hit = false;
                if (tau < a.tau_hi) {
                    const float y0 = yrow[tau], yp = yrow[tau + 1];
                    const bool trough = tau == a.tau_min ? y0 < yp : (y0 < yrow[tau - 1] && y0 <= yp);
                    hit = trough && y0 < a.thr;
                }
                const unsigned long long mask = __ballot(hit);
                if (mask) best = i0 + __ffsll((long long)mask) - 1;
            }
            if (best < 0) {                                              // the smallest index of the minimum
                float bv = inf;
                int bi = 0x7fffffff;
                for (int tau = a.tau_min + lane; tau <= a.tau_hi; tau += 64) {
                    const float y = yrow[tau];
                    if (y < bv || bi == 0x7fffffff) { bv = y; bi = tau; }
                }
                for (int o = 32; o >= 1; o >>= 1) {
                    const float ov = __shfl_xor(bv, o, 64);
                    const int oi = __shfl_xor(bi, o, 64);
                    if (oi != 0x7fffffff && (bi == 0x7fffffff || ov < bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
                }
                best = bi;
            }
            const float y0 = yrow[best];
            float shift = 0.0f;
            if (best > a.tau_min && best < a.tau_hi) {
                const float ym = yrow[best - 1], yp = yrow[best + 1];
                const float pa = __fadd_rn(__fsub_rn(yp, y0), __fsub_rn(ym, y0));
                const float pb = __fmul_rn(__fsub_rn(yp, ym), 0.5f);
                if (fabsf(pb) < fabsf(pa)) shift = __fdiv_rn(-pb, pa);
            }
            const float f0 = __fdiv_rn(a.sr, __fadd_rn((float)best, shift));
            if (lane == 0) {
                const long long o = u.off(a.out_item, a.out_chan) + (long long)(t0 + t) * a.out_stride;
                a.f0[o] = frame_bad ? nan : f0;
                a.cmnd[o] = frame_bad ? nan : y0;
            }
            if (a.curve) {
                float* cv = a.curve + ((long long)u.s * a.frames + t0 + t) * nl;
                for (int tau = lane; tau < nl; tau += 64) cv[tau] = frame_bad ? nan : yrow[tau];
            }
        }
        if (SHARED) __syncthreads();                                     // the wave's y row is written again next turn
    }
}

}  // namespace kpr
