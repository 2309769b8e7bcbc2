// kpr_cqt_adj_kernels.h -- the adjoint (backward pass) of the constant-Q transform of kpr_cqt_kernels.h: the cotangent of the
// complex spectrogram back to the waveform, again an implicit GEMM on v_mfma_f32_16x16x4_f32.  One launch, no atomics, no
// cross-wave sums: the same inputs give the same bits.  Part of the single translation unit kapre_hip.hip.
//
// With B[tau][2 k] = Re w_k[tau - off_k], B[tau][2 k + 1] = -Im w_k[tau - off_k] (zero outside a bin's taps) the forward is
// (Re C, Im C)[t, .] = sum_tau x[o + t hop + tau] B[tau][.], so with G2[t][2 k] = dl/dRe C[t, k], G2[t][2 k + 1] = dl/dIm C[t, k]
//   gx[s] = sum_t sum_c G2[t][c] B[s - o - t hop][c],    0 <= s < time,    frames outside [0, frames) are zero.
// Split along the hop, s = o + q hop + r (q the hop block, 0 <= r < hop), d = q - t:
//   gx[o + q hop + r] = sum_{d < D} sum_c G2[q - d][c] B[d hop + r][c],    D = ceil(L / hop)
// a gather and a matrix product: rows = the hop blocks q of one series (a Toeplitz matrix of the cotangent's frames, never
// formed), columns = the offsets r inside a hop in r-tiles of 16, reduction = the pairs (d, c).
//
// Fragments.  Column tile j of the bank (8 bins = 16 values c, tap range [lo_j, hi_j) as in the forward kernel) meets the 16 taps
// [d hop + 16 rt, + 16) of r-tile rt for a contiguous range of d only; one fragment per such (rt, j, d), none elsewhere.
//
// The table (built by the host: _ffi.cqt_pack_adjoint; it depends on the hop).  A header of Rt x T int4 (Rt = ceil(min(hop, L)
// / 16): the r-tiles any tap reaches, T tiles), entry rt T + j = {first fragment, first d, number of d, 0}; then the fragments,
// r-tile after r-tile, tile after tile, d ascending, 64 float4 each: lane (n = lane & 15, kq = lane >> 4) holds
// B[d hop + 16 rt + n][16 j + 4 kq + e], e = 0 ... 3, zero where 16 rt + n >= hop (that tap belongs to d + 1).  The four values feed
// four MFMA k-steps whose reduction index is then column 4 kq + e of the tile -- the order of a reduction is free as long as both
// operands agree --, so the frame operand of lane (m, kq) is ONE 16-byte LDS read: columns 16 j + 4 kq ... + 3 of row m - d.
// The kernel clamps what it reads from the header to the table and to [0, D): a foreign table cannot send it out of bounds.
//
// Work split.  A workgroup of 8 waves owns a run of F (64, 32 or 16) consecutive hop blocks of one series and stages the
// cotangent rows q0 - D + 1 ... q0 + F - 1 in LDS once: 16 T floats per row plus a pad (bank spread of the 16-byte reads), 8-byte
// pairs gathered from either output layout, rows outside [0, frames) and columns past the last bin as zeros.  A work item is an
// r-tile times a group of RTG (4, 2 or 1) row tiles; item it goes to wave it % 8, kAdjItems items per wave and pass.  An item's
// accumulators stay in registers from its first fragment to its last and are stored by the wave that owns them: nothing is
// added across waves.  A table fragment in registers serves the RTG row tiles; the next one is requested before the MFMAs of
// this one.  Where the F + D - 1 rows do not fit (or option "cqt_adjoint_rows" caps them) the reduction runs in chunks of d: the
// row window of a chunk is staged, every item of the wave adds its part, the accumulators of all kAdjItems items stay live.
// More than 8 kAdjItems items (large hops): further passes over the same windows.
// Every sample 0 <= s < time is stored exactly once; one that no tap covers is the accumulator's initial +0.0.
#pragma once

namespace kpr {

constexpr int kAdjItems = 4;               // items per wave and pass: 4 x RTG accumulators of four registers

struct CqtAdjArgs {
    const float* g;                     // complex64 as float pairs
    const f4* table;
    float* gx;
    long long item, chan;               // the series of gx (kpr_series.h)
    long long g_item, g_chan;           // the same for g, in complex elements
    int stride, g_t, g_k;               // elements from one sample / frame / bin to the next
    int C, time, frames, runs, K;
    int hop, origin;                    // hop block q starts at sample origin + q hop
    int T, Rt;                          // column tiles; r-tiles with an entry in the header
    int nfrag;                          // fragments in the table
    int D, dc, nchunks;                 // d < D, in chunks of dc
    int pitch;                          // floats per staged row
    int gshift, items, passes;          // row groups per r-tile = 1 << gshift; items = r-tiles << gshift
};

// the (tile, d) pairs of one item inside a chunk [d0, d1), in table order
struct CqtAdjCursor {
    int j, d, dh;
    const f4* tb;
};
KPR_DEV void cqt_adj_seek(CqtAdjCursor& c, const CqtAdjArgs& a, const int4* idx, const f4* frag, int d0, int d1) {
    for (; c.j < a.T; ++c.j) {
        const int4 e = idx[c.j];                                         // the same for every lane: kept in scalar registers
        const int ex = __builtin_amdgcn_readfirstlane(e.x), ey = __builtin_amdgcn_readfirstlane(e.y);
        const int ez = __builtin_amdgcn_readfirstlane(e.z);
        const int f0 = min(max(ex, 0), a.nfrag), dlo = min(max(ey, 0), a.D);
        const int dn = min(max(ez, 0), min(a.D - dlo, a.nfrag - f0));
        c.d = max(dlo, d0);
        c.dh = min(dlo + dn, d1);
        if (c.d < c.dh) {
            c.tb = frag + (long long)(f0 + c.d - dlo) * 64;
            return;
        }
    }
}

template <int RTG>
__attribute__((target("no-packed-fp32-ops"))) __global__ __launch_bounds__(kCqtThreads) void k_cqt_adj(CqtAdjArgs a) {
    extern __shared__ __align__(16) float cqt_adj_lds[];
    float* gs = cqt_adj_lds;
    const int F = (16 * RTG) << a.gshift;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
    const SeriesUnit u = series_unit(a.runs, a.C);                       // unit: the run of hop blocks
    const float* g = a.g + 2 * u.off(a.g_item, a.g_chan);
    float* out = u.at(a.gx, a.item, a.chan);
    const int q0 = u.unit * F;
    const int4* header = reinterpret_cast<const int4*>(a.table);
    const f4* frag = a.table + (long long)a.Rt * a.T;

    for (int pass = 0; pass < a.passes; ++pass) {
        f32x4 acc[kAdjItems][RTG];
#pragma unroll
        for (int i = 0; i < kAdjItems; ++i)
#pragma unroll
            for (int r = 0; r < RTG; ++r) acc[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int ch = 0; ch < a.nchunks; ++ch) {
            const int d0 = ch * a.dc, d1 = min(a.D, d0 + a.dc);
            if (a.nchunks > 1 || pass == 0) {                            // one chunk: the window of pass 0 serves every pass
                // ---- the rows q0 - d1 + 1 ... q0 + F - 1 - d0 of the cotangent ----
                const int nrows = F + d1 - d0 - 1, tfirst = q0 - d1 + 1;
                __syncthreads();                                         // the waves still read the window before
                for (int r0 = tid >> 7; r0 < nrows; r0 += 16) {          // four rows in flight per lane
                    for (int kp = tid & 127; kp < 8 * a.T; kp += 128) {
                        f2 v[4];
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            const int row = r0 + 4 * w, t = tfirst + row;
                            v[w] = f2{0.f, 0.f};
                            if (row < nrows && t >= 0 && t < a.frames && kp < a.K)
                                v[w] = *reinterpret_cast<const f2*>(g + 2 * ((long long)t * a.g_t + (long long)kp * a.g_k));
                        }
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            const int row = r0 + 4 * w;
                            if (row < nrows) *reinterpret_cast<f2*>(gs + row * a.pitch + 2 * kp) = v[w];
                        }
                    }
                }
                __syncthreads();
            }
            // ---- this wave's items: every fragment of the chunk on the item's row tiles ----
#pragma unroll
            for (int i = 0; i < kAdjItems; ++i) {
                const int it = (pass * kAdjItems + i) * kCqtWaves + wave;
                const int rt = it >> a.gshift, grp = it & ((1 << a.gshift) - 1);
                if (it >= a.items || rt >= a.Rt) continue;               // (uniform) no such item; an r-tile no tap reaches
                const int4* idx = header + (long long)rt * a.T;
                // lane (m, kq): row 16 (RTG grp + r) + m - d of the run, columns 16 j + 4 kq ... + 3
                const float* arow = gs + (16 * RTG * grp + m + d1 - 1) * a.pitch + 4 * kq;
                CqtAdjCursor cur{0, 0, 0, frag};
                cqt_adj_seek(cur, a, idx, frag, d0, d1);
                if (cur.j >= a.T) continue;
                f4 bv = cur.tb[lane];
                while (cur.j < a.T) {
                    CqtAdjCursor nxt = cur;
                    ++nxt.d;
                    nxt.tb += 64;
                    if (nxt.d >= nxt.dh) {
                        ++nxt.j;
                        cqt_adj_seek(nxt, a, idx, frag, d0, d1);
                    }
                    const f4 bn = (nxt.j < a.T ? nxt.tb : cur.tb)[lane]; // (past the last: this one again, not used)
                    const float* ap = arow - cur.d * a.pitch + 16 * cur.j;
                    f4 av[RTG];
#pragma unroll
                    for (int r = 0; r < RTG; ++r) av[r] = *reinterpret_cast<const f4*>(ap + 16 * r * a.pitch);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int r = 0; r < RTG; ++r)
                            acc[i][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r][e], bv[e], acc[i][r], 0, 0, 0);
                    cur = nxt;
                    bv = bn;
                }
            }
        }
        // ---- lane holds D[row 4 kq + e][column m] of every row tile: sample origin + q hop + 16 rt + m ----
#pragma unroll
        for (int i = 0; i < kAdjItems; ++i) {
            const int it = (pass * kAdjItems + i) * kCqtWaves + wave;
            const int rt = it >> a.gshift, grp = it & ((1 << a.gshift) - 1);
            const int col = 16 * rt + m;
            if (it >= a.items || col >= a.hop) continue;
#pragma unroll
            for (int r = 0; r < RTG; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long long s = a.origin + (long long)(q0 + 16 * (RTG * grp + r) + 4 * kq + e) * a.hop + col;
                    if (s >= 0 && s < a.time) out[s * a.stride] = acc[i][r][e];
                }
        }
    }
}

}  // namespace kpr
