// kpr_cqt_kernels.h -- constant-Q transform of a waveform (kapre_amd.CQT, backend.cqt): an implicit GEMM on
// v_mfma_f32_16x16x4_f32.  One launch, no atomics, no host reads: the same inputs give the same bits.  Part of the single
// translation unit kapre_hip.hip.
//
// Per series x of `time` samples, bin k with N_k taps, L = N_0, off_k = (L - N_k) / 2, frame t starting at sample o + t hop:
//   C[t, k] = sum_{n < N_k} x[o + t hop + off_k + n] conj(w_k[n])                 samples outside [0, time) are exact zeros
// As a matrix product: rows = frames of one series (a Toeplitz matrix of the waveform, never formed), columns = (Re, -Im) of the
// bins, reduction = the L taps of a frame.  Bin k is non-zero on taps [off_k, off_k + N_k) only.
//
// Column tiles.  8 consecutive bins = 16 columns (column 2 b = Re w, 2 b + 1 = -Im w of bin 8 j + b).  Tile j reduces over its own
// tap range [lo_j, hi_j): the range of its lowest bin, lo_j rounded down to the step of 16 taps, hi_j up to it, cut at L.
//
// The table (packed tile form, built by the host: _ffi.cqt_pack).  Tile after tile, step after step, 64 float4 per step: lane
// (m = lane & 15, kq = lane >> 4) holds B[tap lo_j + 16 s + 4 kq + e][column m], e = 0 ... 3 -- the four values feed four MFMA
// k-steps, whose reduction index is then tap 4 kq + e of the step (the order of a reduction is free as long as both operands
// agree).  One coalesced 1 KiB read per step and wave, used for F / 16 row tiles.
//
// Work split.  A workgroup of 8 waves owns a run of F = 64 or 32 consecutive frames of one series (kpr_cqt_plan) and walks the
// host's list of phases: (tile, piece of its tap range that is staged at once).  Inside a phase the eight waves take eight
// consecutive slices of the steps (equal within one step) -- tile lengths fall geometrically, so a tile per wave would idle most
// waves --, every wave multiplies all F frames with its slice, the fragment of the table staying in registers across the F / 16
// row tiles.  The accumulators stay in registers across the phases of a tile; at its end the eight partial sums go to LDS and
// are added in wave order (ascending taps when the tile is one phase) by the lane that stores the bin.
//
// The frame operand.  SPAN form (hop < chunk: frames overlap): the (F - 1) hop + chunk samples of the run are staged once, sample
// i at i + pad (i / hop); lane (m, kq) reads frame m's taps at m (hop + pad) + ..., so the 16 lanes of a reduction group spread
// over the banks for every hop (pad: kpr_cqt_plan picks the least conflicting one; i / hop is one v_mul_hi with the host's magic
// number).  WIN form (hop >= chunk): every frame's piece is staged on its own row of chunk + pad floats.  VEC: one ds_read_b128 per
// row tile and step (SPAN: hop % 4 == 0, pad % 4 == 0; WIN always); else four scalar reads at the same taps.
// Taps at or beyond hi_j are taken out of the operand by a select, not by a zero in the table: a NaN sample beyond a frame's L
// taps never reaches it.
#pragma once

namespace kpr {

constexpr int kCqtThreads = 512;
constexpr int kCqtWaves = kCqtThreads / 64;
constexpr int kCqtStep = 16;               // taps per step: four MFMA k-steps of four
constexpr int kCqtTileBins = 8;            // bins per column tile
constexpr int kCqtMaxPhases = 64;
constexpr int kCqtLdsFloats = 40960;       // 160 KiB
enum { kCqtStage = 1, kCqtLast = 2 };

struct CqtPhase {
    int tab;                // float4 index of the phase's first step in the table
    int a, hi;              // first tap (a multiple of 16); end of the tile's tap range
    int nsteps;
    int c0, clen;           // the staged taps [c0, c0 + clen) that hold this phase (clen a multiple of 16)
    int tile, flags;        // kCqtStage: stage [c0, c0 + clen) first; kCqtLast: the tile ends here
};

struct CqtArgs {
    const float* x;
    const f4* table;
    float* out;                         // complex64 as float pairs, or float32 magnitudes
    long long item, chan;               // the series of x (kpr_series.h)
    long long out_item, out_chan;       // the same for out, in output elements
    int stride, out_t, out_k;           // elements from one sample / frame / bin to the next
    int C, time, frames, runs, K;
    int hop, origin;                    // frame t starts at sample origin + t hop
    int hopL, pad;                      // LDS: row m starts at m hopL; a word i lies at i + pad * (i / hop)
    unsigned magic;                     // floor(2^32 / hop) + 1 (SPAN), 0 (WIN: no skew inside a row)
    int pieces;                         // 1 (SPAN) or F (WIN)
    int red;                            // float offset of the reduction area: kCqtWaves x F x 16
    int n_phases;
    CqtPhase ph[kCqtMaxPhases];
};

KPR_DEV int cqt_word(int i, int pad, unsigned magic) { return i + pad * (int)__umulhi((unsigned)i, magic); }

// One step of 16 taps on all row tiles: this lane's taps are tap ... tap + 3 (tap = step start + 4 kq), bv their table values.
template <int RT, bool VEC>
KPR_DEV void cqt_step(const float* xs, const int (&row)[RT], f32x4 (&acc)[RT], f4 bv, int tap, int c0, int hi, int pad, unsigned magic) {
    f4 av[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = row[rt] + tap - c0;
        if constexpr (VEC) {
            av[rt] = *reinterpret_cast<const f4*>(xs + cqt_word(i, pad, magic));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) av[rt][e] = xs[cqt_word(i + e, pad, magic)];
        }
    }
    if (tap - (tap & 12) + kCqtStep > hi) {                               // (uniform) the tile's last step: taps beyond hi
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (tap + e >= hi) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) av[rt][e] = 0.0f;
            }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][e], bv[e], acc[rt], 0, 0, 0);
}

template <int RT, bool VEC, bool MAG>
__attribute__((target("no-packed-fp32-ops"))) __global__ __launch_bounds__(kCqtThreads) void k_cqt(CqtArgs a) {
    extern __shared__ __align__(16) float cqt_lds[];
    constexpr int F = 16 * RT;
    float* xs = cqt_lds;
    float* red = cqt_lds + a.red;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
    const SeriesUnit u = series_unit(a.runs, a.C);                       // unit: the run
    const float* in = u.at(a.x, a.item, a.chan);
    const auto [t0, fv] = frame_run(u.unit, F, a.frames);
    float* out = a.out + (u.off(a.out_item, a.out_chan) + (long long)t0 * a.out_t) * (MAG ? 1 : 2);
    const long long g_run = (long long)a.origin + (long long)t0 * a.hop;

    int row[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) row[rt] = (16 * rt + m) * a.hopL;
    f32x4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int p = 0; p < a.n_phases; ++p) {
        const CqtPhase& ph = a.ph[p];
        if (ph.flags & kCqtStage) {
            __syncthreads();                                             // the waves still read the piece before
            const int plen = a.pieces == 1 ? (F - 1) * a.hop + ph.clen : ph.clen;
            for (int q = 0; q < a.pieces; ++q) {
                const long long g0 = g_run + (long long)q * a.hop + ph.c0;
                for (int i0 = tid; i0 < plen; i0 += 4 * kCqtThreads) {   // four loads in flight per lane
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const long long g = g0 + i0 + j * kCqtThreads;
                        v[j] = (i0 + j * kCqtThreads < plen && g >= 0 && g < a.time) ? in[g * a.stride] : 0.0f;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = i0 + j * kCqtThreads;
                        if (i < plen) xs[cqt_word(q * a.hopL + i, a.pad, a.magic)] = v[j];
                    }
                }
            }
            __syncthreads();
        }
        // ---- this wave's slice of the phase's steps ----
        const int s0 = ph.nsteps * wave / kCqtWaves, s1 = ph.nsteps * (wave + 1) / kCqtWaves;
        if (s0 < s1) {
            const f4* tb = a.table + ph.tab + lane;
            // two steps per turn: each table fragment is requested one step before its MFMAs, into registers of its own
            f4 b0 = tb[(long long)s0 * 64];
            for (int st = s0; st < s1; st += 2) {
                const f4 b1 = tb[(long long)min(st + 1, s1 - 1) * 64];
                cqt_step<RT, VEC>(xs, row, acc, b0, ph.a + kCqtStep * st + 4 * kq, ph.c0, ph.hi, a.pad, a.magic);
                b0 = tb[(long long)min(st + 2, s1 - 1) * 64];
                if (st + 1 < s1) cqt_step<RT, VEC>(xs, row, acc, b1, ph.a + kCqtStep * (st + 1) + 4 * kq, ph.c0, ph.hi, a.pad, a.magic);
            }
        }
        if (!(ph.flags & kCqtLast)) continue;
        // ---- the tile's eight partial sums, added in wave order by the lane that stores the bin ----
        float* mine = red + wave * (F * 16);                             // lane holds D[row 16 rt + 4 kq + r][column m]
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mine[(16 * rt + 4 * kq + r) * 16 + m] = acc[rt][r];
            acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        for (int e = tid; e < F * kCqtTileBins; e += kCqtThreads) {
            const int fr = e >> 3, b = e & 7, k = ph.tile * kCqtTileBins + b;
            if (fr < fv && k < a.K) {
                const float* src = red + fr * 16 + 2 * b;
                f2 c = *reinterpret_cast<const f2*>(src);
#pragma unroll
                for (int w = 1; w < kCqtWaves; ++w) {
                    const f2 v = *reinterpret_cast<const f2*>(src + w * (F * 16));
                    c.x = __fadd_rn(c.x, v.x);
                    c.y = __fadd_rn(c.y, v.y);
                }
                const long long o = (long long)fr * a.out_t + (long long)k * a.out_k;
                if constexpr (MAG) out[o] = __fsqrt_rn(fmaf(c.x, c.x, __fmul_rn(c.y, c.y)));
                else *reinterpret_cast<f2*>(out + 2 * o) = c;
            }
        }
        __syncthreads();                                                 // the area is written again at the next tile's end
    }
}

}  // namespace kpr
