// kpr_spec_fir_kernels.h -- a short complex FIR along the frame axis of every bin of a complex spectrogram: the middle launch of
// the partitioned overlap-save convolution (kapre_amd.Convolve, backend.fftconvolve).  Part of the single translation unit
// kapre_hip.hip.
//
//   Y[o, k, i] = sum_{p = 0}^{P - 1} X[o, k - p, i] H[ir(o), p, bin(i)],   0 <= k < frames_out,   X[o, r, i] = 0 for r outside [0, frames_in)
//   ir(o) = clamp(idx[o / outer_per_item], 0, n_ir - 1) (idx == NULL: 0),   bin(i) = i / band_div
//
// The sum runs in ascending p from +0, and one term is four FMAs in this order:
//   re = fma(xr, hr, re);  re = fma(-xi, hi, re);  im = fma(xr, hi, im);  im = fma(xi, hr, im)
// so a result depends on its 2 P inputs alone -- never on the launch shape -- and the same inputs give the same bits.  A term whose
// input row lies outside [0, frames_in) is skipped, not added as zero, and so is every tap p >= P of a bucket: a non-finite X bin
// reaches the rows k ... k + P - 1 of its own column and nothing else.
//
// Column groups (V = 2 or 1 complex64 values) are those of kpr_cols.h; time is tiled as there, R rows per wave and W waves per
// workgroup, but nothing is carried along time: a wave reads the R + P - 1 input rows its R output rows need, its halo included,
// so there is no barrier and no LDS.  The lane keeps its P filter values in registers for the whole launch; P is a run-time value
// inside a compile-time bucket PB (4, 8, 16, 32), and every loop below is fully unrolled over PB, so that no register array is
// indexed at run time; the tests `p < n_part` are uniform (scalar branches) and only exist for the taps a bucket may lack.
// Input rows are walked from the newest to the oldest, which is ascending p for every output row, one row ahead of the FMAs.
#pragma once

namespace kpr {

constexpr int kFirRows = 8;        // R: output rows of a wave per super-block
constexpr int kFirWaves = 4;       // W: waves of a workgroup = time chunks of a super-block
constexpr int kFirMaxPart = 32;    // P <= 32

struct FirArgs {
    const float2* x;
    float2* out;
    const float2* h;               // (n_ir, n_part, n_freq)
    const int* idx;                // may be NULL: one filter number per batch item
    int frames_in, frames_out;
    int n_part, n_ir, n_freq;
    unsigned band_div;             // bin(i) = i / band_div
    unsigned outer_per_item;       // outer items (channels) of one batch item
    unsigned inner;                // complex values of one row
    unsigned groups_per_item;      // inner / V
    long long n_groups;            // outer * groups_per_item
};

// the bucket of a partition count, and the least count that is sent to a bucket (taps below it need no test)
constexpr int fir_bucket(int n_part) { return n_part <= 4 ? 4 : n_part <= 8 ? 8 : n_part <= 16 ? 16 : 32; }
constexpr int fir_bucket_min(int pb) { return pb == 4 ? 1 : pb / 2 + 1; }

KPR_DEV void fir_mac(float2& acc, float2 x, float2 h) {
    acc.x = fmaf(x.x, h.x, acc.x);
    acc.x = fmaf(-x.y, h.y, acc.x);
    acc.y = fmaf(x.x, h.y, acc.y);
    acc.y = fmaf(x.y, h.x, acc.y);
}

template <int V, int PB>
__global__ __launch_bounds__(64 * kFirWaves) void k_spec_fir(FirArgs a) {
    constexpr int R = kFirRows, W = kFirWaves, PMIN = fir_bucket_min(PB);

    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const ColGroup cg = col_group<V>(a.n_groups, a.groups_per_item);
    const float2* xin = a.x + cg.item * (long long)a.frames_in * a.inner + cg.i0;
    float2* yout = a.out + cg.item * (long long)a.frames_out * a.inner + cg.i0;
    const int P = a.n_part;

    // the lane's filter: the item's table row, clamped into the table whatever idx[] holds
    float2 h[PB][V];
    {
        int ir = a.idx ? a.idx[cg.item / a.outer_per_item] : 0;
        ir = min(max(ir, 0), a.n_ir - 1);
        const float2* hp = a.h + (long long)ir * P * a.n_freq;
#pragma unroll
        for (int p = 0; p < PB; ++p)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                h[p][v] = make_float2(0.0f, 0.0f);
                if (p < PMIN || p < P) h[p][v] = hp[(long long)p * a.n_freq + (cg.i0 + v) / a.band_div];
            }
    }

    // input row k0 + jj - (PB - 1) of the lane's columns, when a tap of the wave reads it (the oldest tap that does is that of
    // output row 0: p = PB - 1 - jj) and it is a row of X
    auto fetch = [&](int k0, int jj, ColVec<float2, V>& z) -> bool {
        const int row = k0 + jj - (PB - 1);
        const bool use = PB - 1 - jj < P && (unsigned)row < (unsigned)a.frames_in;
#pragma unroll
        for (int v = 0; v < V; ++v) z.v[v] = make_float2(0.0f, 0.0f);
        if (use) z = col_load<V>(xin + (long long)row * a.inner);
        return use;
    };

    const int n_super = (a.frames_out + W * R - 1) / (W * R);
    for (int sb = blockIdx.y; sb < n_super; sb += gridDim.y) {
        const int k0 = (sb * W + wave) * R;
        if (k0 >= a.frames_out) continue;                              // (no barrier: a wave without rows just leaves)
        ColVec<float2, V> acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[r].v[v] = make_float2(0.0f, 0.0f);

        ColVec<float2, V> cur, nxt;
        bool use = fetch(k0, R + PB - 2, cur);
#pragma unroll
        for (int jj = R + PB - 2; jj >= 0; --jj) {
            bool use_nxt = false;
            if (jj > 0) use_nxt = fetch(k0, jj - 1, nxt);
            if (use) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int p = r + PB - 1 - jj;                     // a constant once unrolled
                    if (p >= 0 && p < PB && (p < PMIN || p < P)) {
#pragma unroll
                        for (int v = 0; v < V; ++v) fir_mac(acc[r].v[v], cur.v[v], h[p][v]);
                    }
                }
            }
            cur = nxt;
            use = use_nxt;
        }

#pragma unroll
        for (int r = 0; r < R; ++r)
            if (cg.live && k0 + r < a.frames_out) col_store<V>(yout + (long long)(k0 + r) * a.inner, acc[r]);
    }
}

}  // namespace kpr
