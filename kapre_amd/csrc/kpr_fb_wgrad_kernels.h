// kpr_fb_wgrad_kernels.h -- the weight gradient of a filterbank applied along the frequency axis (TrainableFilterbank):
//   gW[f][m] = sum over the rows r of x[r][f] g[r][m],    x: rows of n_freq bins, g: rows of n_filt filters, float32
// an A^T B product whose reduction axis is the slow axis of both operands, on v_mfma_f32_16x16x4_f32 (full float32 products).
// No atomics, no cross-wave sums: the same inputs give the same bits.  Part of the single translation unit kapre_hip.hip.
//
// Rows.  channels_first (b, c, t, f): R = b c t contiguous rows.  channels_last (b, t, f, c): R = b t rows of n_freq c floats,
// bin f of channel ch at f c + ch; the channels are summed into the one matrix, so a row contributes c steps to the reduction and
// the channel is nothing but the stride (c) and the offset (ch) of a fragment's LDS read.  One channel: the same memory image.
//
// Work split.  The output is cut into tiles of kWgTF = 64 bins by kWgNF = 128 filters (more filters: further column passes, each
// a workgroup of its own), the rows into slabs of S = chunks_per_slab x kc.  Grid: f-tiles x slabs x passes.  A workgroup of four
// waves owns one (tile, slab): wave w the f-subtiles 2 (w & 1), + 1 and the filter tiles 4 (w >> 1) ... + 3 -- eight 16 x 16
// accumulators that stay in its registers from the slab's first row to the store.  One slab: the store goes to gW.  Several: to
// the slab's own matrix in the workspace, and k_fb_wgrad_reduce adds the slabs of every (f, m) in ascending order.
//
// Data movement.  A chunk is kc = 4 RQ (16, 8 or 4) rows: the tile's 64 c floats of every x row and the pass's filters of every g
// row, read from global memory with 16-byte loads where the pointers and row lengths allow (V = 4), else 4-byte loads (both
// coalesced along the row), held in registers across the MFMAs of the chunk before, then stored to the other of two LDS buffers:
// one barrier per chunk.  Wave w loads the rows w, w + 4, ... of a chunk, lane l the columns V (l + 64 ci): slot s of a lane is
// row w + 4 (s % RQ), column step ci = s / RQ, both known when the kernel is compiled.
// LDS: row k of x at k px, of g at k pg, px / pg = the width plus the pad of kpr_host_fb_wgrad.h: an A fragment is lane (i, kq)
// reading word (k + kq) px + (16 j + i) c + ch, i. e. 16 consecutive words (c = 1) of four rows.  A 4-byte read is served 32 lanes
// at a time; with px = 16 mod 32 the two rows of either half start 16 banks apart and no two lanes meet in a bank; the B fragment
// likewise with pg.  (c even: the 16 words of a row lie 2 banks apart at least, two lanes per bank is the least possible.)
// The fragments of the next step are read before the MFMAs of this one.
//
// Tails.  Rows past R, bins past n_freq, filters past n_filt are +0.0 WRITTEN INTO LDS: a lane whose slot lies past the tail
// loads an element that exists (every load is unconditional and in bounds) and its register is ANDed with 0 on the way to LDS,
// so no fragment ever holds a value twice and nothing is multiplied by 0 to get rid of it: 0 x NaN can only occur in accumulators
// that are never stored.  A NaN in x[r][f0] reaches row f0 of gW, an Inf in g[r][m0] column m0, nothing else.
#pragma once

namespace kpr {

constexpr int kWgTF = 64, kWgNF = 128;     // bins and filters of a workgroup's output tile
constexpr int kWgThreads = 256;
constexpr int kWgSlotFloats = 16;          // floats a lane holds of each operand of the chunk in flight

struct FbWgradArgs {
    const float* x;
    const float* g;
    float* out;                            // gW (one slab) or the workspace: n_slabs matrices of n_freq x n_filt
    long long R, chunks;                   // rows; chunks of kc rows
    long long xrow, grow;                  // floats from one row to the next: n_freq c, n_filt c
    int n_freq, n_filt, c;
    int ftiles, n_slabs;                   // blockIdx.x = (pass n_slabs + slab) ftiles + f-tile
    int cps;                               // chunks per slab
    int px, pg;                            // floats per staged row
};

template <int V> struct WgVec { typedef float T; };
template <> struct WgVec<4> { typedef f4 T; };

// The chunk's rows of one operand into registers: `valid` (>= V) columns and `rows` (>= 1) rows exist.  Every slot loads, without
// a condition -- a load under its own condition makes hipcc wait for each one where it is issued --: a slot past the tail loads
// the last row / the last columns that exist, and wg_store replaces what it loaded by 0.
template <int V, int RQ>
KPR_DEV void wg_fetch(typename WgVec<V>::T (&r)[kWgSlotFloats / V], const float* src, long long rowstride, long long rows,
                      int valid, int wave, int lane) {
    typedef typename WgVec<V>::T T;
#pragma unroll
    for (int s = 0; s < kWgSlotFloats / V; ++s) {
        const long long row = min((long long)(wave + 4 * (s % RQ)), rows - 1);
        const int col = min((lane + 64 * (s / RQ)) * V, valid - V);
        r[s] = *reinterpret_cast<const T*>(src + row * rowstride + col);
    }
}
// ... and from the registers into LDS, the `width` columns that the fragments read: bit-wise AND with the lane's tail mask, so
// a row or column that does not exist is +0.0 whatever was loaded in its place (a NaN included: nothing is multiplied by 0)
template <int V, int RQ>
KPR_DEV void wg_store(const typename WgVec<V>::T (&r)[kWgSlotFloats / V], float* dst, int pitch, int width, long long rows, int valid,
                      int wave, int lane) {
#pragma unroll
    for (int s = 0; s < kWgSlotFloats / V; ++s) {
        const int row = wave + 4 * (s % RQ), col = (lane + 64 * (s / RQ)) * V;
        const unsigned keep = (row < rows && col < valid) ? 0xffffffffu : 0u;
        if (col < width) {
            float* at = dst + row * pitch + col;
            if constexpr (V == 4) {
                f4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = __uint_as_float(__float_as_uint(r[s][e]) & keep);
                *reinterpret_cast<f4*>(at) = v;
            } else {
                *at = __uint_as_float(__float_as_uint(r[s]) & keep);
            }
        }
    }
}

// the MFMAs of one chunk on this wave's nj x nt tiles (FULL: 2 x 4, no tests in the loop).  xa / gb: this lane's word of row kq,
// channel 0 in the wave's first f-subtile / filter tile; a step is four rows of one channel
template <bool FULL>
KPR_DEV void wg_chunk(f32x4 (&acc)[2][4], const float* xa, const float* gb, int steps, int c, int px, int pg, int nj, int nt) {
    float av[2], bv[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) av[j] = (FULL || j < nj) ? xa[16 * j * c] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) bv[t] = (FULL || t < nt) ? gb[16 * t * c] : 0.f;
    int ch = 0;
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        if (s + 1 < steps) {                                             // (the last step reads its own fragments again)
            ++ch; ++xa; ++gb;
            if (ch == c) { ch = 0; xa += 4 * px - c; gb += 4 * pg - c; }
        }
        float an[2], bn[4];
#pragma unroll
        for (int j = 0; j < 2; ++j) an[j] = (FULL || j < nj) ? xa[16 * j * c] : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) bn[t] = (FULL || t < nt) ? gb[16 * t * c] : 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (FULL || (j < nj && t < nt)) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[t], acc[j][t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) av[j] = an[j];
#pragma unroll
        for (int t = 0; t < 4; ++t) bv[t] = bn[t];
    }
}

template <int VX, int VG, int RQ>
__global__ __launch_bounds__(kWgThreads) void k_fb_wgrad(FbWgradArgs a) {
    extern __shared__ __align__(16) float wg_lds[];
    constexpr int KC = 4 * RQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), i = lane & 15, kq = lane >> 4;
    int bid = blockIdx.x;
    const int ft = bid % a.ftiles;
    bid /= a.ftiles;
    const int slab = bid % a.n_slabs, pass = bid / a.n_slabs;
    const int f0 = ft * kWgTF, m0 = pass * kWgNF;
    const int nf = min(kWgTF, a.n_freq - f0), nm = min(kWgNF, a.n_filt - m0);       // bins and filters of this tile that exist
    const int xvalid = nf * a.c, xwidth = kWgTF * a.c;                             // columns to load; columns the fragments read
    const int gvalid = nm * a.c, gwidth = ((nm + 15) & ~15) * a.c;
    const int buf = KC * (a.px + a.pg);                                            // floats of a buffer: KC rows of x, KC rows of g
    const long long c0 = (long long)slab * a.cps, r0 = c0 * KC;
    const int nch = (int)min((long long)a.cps, a.chunks - c0);
    const float* xp = a.x + r0 * a.xrow + (long long)f0 * a.c;
    const float* gp = a.g + r0 * a.grow + (long long)m0 * a.c;
    // this wave's accumulators: f-subtiles fs0, fs0 + 1 (nj of them exist) x filter tiles mt0 ... mt0 + 3 (nt exist)
    const int fs0 = 2 * (wave & 1), mt0 = 4 * (wave >> 1);
    const int nj = min(max((nf + 15) / 16 - fs0, 0), 2), nt = min(max((nm + 15) / 16 - mt0, 0), 4);
    f32x4 acc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    typename WgVec<VX>::T rx[kWgSlotFloats / VX];
    typename WgVec<VG>::T rg[kWgSlotFloats / VG];
    wg_fetch<VX, RQ>(rx, xp, a.xrow, a.R - r0, xvalid, wave, lane);
    wg_fetch<VG, RQ>(rg, gp, a.grow, a.R - r0, gvalid, wave, lane);
    wg_store<VX, RQ>(rx, wg_lds, a.px, xwidth, a.R - r0, xvalid, wave, lane);
    wg_store<VG, RQ>(rg, wg_lds + KC * a.px, a.pg, gwidth, a.R - r0, gvalid, wave, lane);
    __syncthreads();
    for (int n = 0; n < nch; ++n) {
        const bool more = n + 1 < nch;
        const long long rn = (long long)(n + 1) * KC;
        if (more) {                                                      // the next chunk's loads fly under this chunk's MFMAs
            wg_fetch<VX, RQ>(rx, xp + rn * a.xrow, a.xrow, a.R - r0 - rn, xvalid, wave, lane);
            wg_fetch<VG, RQ>(rg, gp + rn * a.grow, a.grow, a.R - r0 - rn, gvalid, wave, lane);
        }
        // lane (i, kq): rows kq, kq + 4, ... of the chunk; bin 16 (fs0 + j) + i, filter 16 (mt0 + t) + i of every channel
        const float* xs = wg_lds + (n & 1) * buf;
        const float* xa = xs + kq * a.px + (16 * fs0 + i) * a.c;
        const float* gb = xs + KC * a.px + kq * a.pg + (16 * mt0 + i) * a.c;
        if (nj == 2 && nt == 4) wg_chunk<true>(acc, xa, gb, RQ * a.c, a.c, a.px, a.pg, nj, nt);
        else if (nj > 0 && nt > 0) wg_chunk<false>(acc, xa, gb, RQ * a.c, a.c, a.px, a.pg, nj, nt);
        if (more) {
            float* nx = wg_lds + ((n + 1) & 1) * buf;                    // read last in iteration n - 1: every wave is past its barrier
            wg_store<VX, RQ>(rx, nx, a.px, xwidth, a.R - r0 - rn, xvalid, wave, lane);
            wg_store<VG, RQ>(rg, nx + KC * a.px, a.pg, gwidth, a.R - r0 - rn, gvalid, wave, lane);
        }
        __syncthreads();
    }
    // ---- lane (i, kq) holds D[bin 4 kq + e][filter i] of every tile: 16 lanes store 64 contiguous bytes ----
    float* out = a.out + (long long)slab * a.n_freq * a.n_filt;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = m0 + 16 * (mt0 + t) + i;
            if (j >= nj || t >= nt || m >= a.n_filt) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int f = f0 + 16 * (fs0 + j) + 4 * kq + e;
                if (f < a.n_freq) out[(long long)f * a.n_filt + m] = acc[j][t][e];
            }
        }
}

// gW[e] = the slabs' partial sums of element e, added in ascending slab order (no slab: zeros -- the call without rows)
__global__ __launch_bounds__(256) void k_fb_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ gw, long long n, int n_slabs) {
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += gridDim.x * 256LL) {
        float s = 0.f;
        for (int k = 0; k < n_slabs; ++k) s += ws[k * n + e];
        gw[e] = s;
    }
}

}  // namespace kpr
