// kpr_cmvn_kernels.h -- per-utterance mean / variance normalisation along time (Kaldi's apply-cmvn --norm-vars, ESPnet's
// UtteranceMVN) and its input gradient: the kernel family whose hot loop is a REDUCTION along time that must finish before the
// first output can be written.  Part of the single translation unit kapre_hip.hip.
//
//   d[t] = x[t] - x[0];  m = (1/n) sum d[t];  c[t] = d[t] - m;  v = (1/n) sum c[t]^2;  rstd = (v + eps)^-1/2
//   y[t] = c[t] rstd (norm_vars) or c[t];   n = F
//   backward: gx[t] = rstd (gy[t] - mean(gy) - y[t] mean(gy y))  (norm_vars),  gx[t] = gy[t] - mean(gy)  (else)
//
// Column groups (V = 4 or 1 floats), super-blocks of W * R rows and the one barrier are those of kpr_cols.h.  There is no band
// divisor: every inner index is a column of its own.
//
// The chunk of a wave is its R rows (fewer at the end of the series).  A wave shifts its rows by x[0] (log-mel decibels sit at
// -60 +- a few: the shift keeps the sums small), forms its chunk's mean and M2 = sum (d - mean)^2 two-pass in registers, each
// sum sequential in row order, and leaves both in LDS, indexed by lane; the chunk's count follows from the shape.  After one
// barrier every wave merges the chunks into the running (n, mean, M2), one at a time in (super-block, wave) order, with the
// pairwise update (Chan, Golub, LeVeque 1979)
//   delta = mean_b - mean;  n' = n + n_b;  mean' = mean + delta (n_b / n');  M2' = (M2 + M2_b) + delta^2 (n n_b / n')
// -- every wave redundantly, so every wave ends up holding the column's statistics.  The LDS slab is double-buffered, which
// makes the one barrier per super-block sufficient.
//
// Two forms, one body (FORM).  CMVN_RES (F <= W R): the one super-block stays in registers between the reduction and the
// output -- one read, one write.  CMVN_STR (any F): sweep 1 walks the super-blocks and keeps nothing, sweep 2 reads the rows
// again and writes the output -- two reads, one write.  R is the same in both and so are the chunks, their arithmetic
// (cmvn_chunk, cmvn_merge, cmvn_out: contraction off, every operation rounded on its own) and the merge order: for F <= W R
// the two forms give the same bits.  The backward kernel is the same two forms over (y, gy) with two plain sums per column,
// added lane-sequentially, then over the waves in order, then over the super-blocks in order.  No atomics anywhere.
#pragma once

namespace kpr {

constexpr int kCmvnRows = 16;      // R: rows a wave holds in registers per super-block (both forms)
constexpr int kCmvnWaves = 8;      // W: waves of a workgroup = time chunks of a super-block; F_res = W * R = 128

enum { CMVN_RES = 0, CMVN_STR = 1 };
// forward: y = c rstd | the same and rstd per column | y = c (norm_vars off);  backward: from (y, rstd, gy) | from gy alone
enum { CMVN_FWD = 0, CMVN_FWD_RSTD = 1, CMVN_FWD_MEAN = 2, CMVN_BWD = 3, CMVN_BWD_MEAN = 4 };

struct CmvnArgs {
    const float* x;                // forward: x.  backward: y (not read by CMVN_BWD_MEAN)
    const float* gy;               // backward
    const float* rstd;             // CMVN_BWD: (outer, inner)
    float* out;                    // y, or gx
    float* rstd_out;               // CMVN_FWD_RSTD: (outer, inner)
    float eps;
    int frames;
    unsigned inner;                // elements of one row
    unsigned groups_per_item;      // inner / V
    long long n_groups;            // outer * groups_per_item
};

// rows of the chunk that starts at row tau0 of a series of `frames` rows
KPR_DEV int cmvn_count(int tau0, int frames) { return min(max(frames - tau0, 0), kCmvnRows); }

// One chunk of nb >= 1 rows, shifted in place (d = x - x0): its mean and, with M2, sum (d - mean)^2 -- two passes over the
// registers, each sum sequential in row order.  nb is the same for every lane of the wave.
template <int V, bool M2>
KPR_DEV void cmvn_chunk(ColVec<float, V> (&d)[kCmvnRows], const float (&x0)[V], int nb, float (&mean)[V], float (&m2)[V]) {
#pragma clang fp contract(off)
    const float fnb = (float)nb;
    float s[V], q[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s[v] = q[v] = 0.0f;
#pragma unroll
    for (int k = 0; k < kCmvnRows; ++k)
        if (k < nb)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                d[k].v[v] = d[k].v[v] - x0[v];
                s[v] = s[v] + d[k].v[v];
            }
#pragma unroll
    for (int v = 0; v < V; ++v) mean[v] = s[v] / fnb;
    if constexpr (M2) {
#pragma unroll
        for (int k = 0; k < kCmvnRows; ++k)
            if (k < nb)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float c = d[k].v[v] - mean[v];
                    q[v] = q[v] + c * c;
                }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) m2[v] = q[v];
}

// The pairwise update: the chunk (nb >= 1 rows, mean mb, M2 qb) joins the running (n, mean, m2).  The two weights depend on the
// counts alone.  n == 0 gives mean = mb and m2 = qb bit for bit (delta = mb, weights 1 and 0).
template <int V, bool M2>
KPR_DEV void cmvn_merge(int n, int nb, const float (&mb)[V], const float (&qb)[V], float (&mean)[V], float (&m2)[V]) {
#pragma clang fp contract(off)
    const float w1 = (float)nb / (float)(n + nb);
    const float w2 = (float)n * w1;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float delta = mb[v] - mean[v];
        mean[v] = mean[v] + delta * w1;
        if constexpr (M2) m2[v] = (m2[v] + qb[v]) + (delta * delta) * w2;
    }
}

// y of one element from its shifted value: (d - m) rstd, or d - m
template <bool NORM>
KPR_DEV float cmvn_out(float d, float m, float rstd) {
#pragma clang fp contract(off)
    const float c = d - m;
    return NORM ? c * rstd : c;
}

// backward, one element: rstd ((gy - mean(gy)) - y mean(gy y)), or gy - mean(gy)
template <bool NORM>
KPR_DEV float cmvn_bwd_out(float g, float y, float mg, float mgy, float rstd) {
#pragma clang fp contract(off)
    const float t = g - mg;
    return NORM ? rstd * (t - y * mgy) : t;
}

template <int V, int FORM, int MODE>
__global__ __launch_bounds__(64 * kCmvnWaves) void k_cmvn(CmvnArgs a) {
    constexpr int R = kCmvnRows, W = kCmvnWaves;
    constexpr bool BWD = MODE >= CMVN_BWD;
    constexpr bool NORM = MODE != CMVN_FWD_MEAN && MODE != CMVN_BWD_MEAN;
    constexpr bool RES = FORM == CMVN_RES;
    constexpr bool NEED_Y = MODE == CMVN_BWD;                         // the backward pass that reads y next to gy
    // forward: the chunks' mean and M2.  backward: their sum gy and sum gy y
    __shared__ float slab[2][2][W][V][64];

    // (the wave index as a scalar: a chunk's row count is then one too, and the guards below are scalar branches; `lane` is taken
    // ahead of it, not as cg.lane behind it: the order of the two instructions decides a register tie in one instance)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const ColGroup cg = col_group<V>(a.n_groups, a.groups_per_item);
    const long long base = cg.item * (long long)a.frames * a.inner + cg.i0;
    const long long col = cg.item * (long long)a.inner + cg.i0;      // of the (outer, inner) statistics

    ColVec<float, V> in[R];               // forward: x, shifted in place.  backward: gy
    ColVec<float, V> yy[NEED_Y ? R : 1];  // backward: y
    float x0[V], mean[V], m2[V];   // forward: the running mean and M2.  backward: the running sum gy and sum gy y
#pragma unroll
    for (int v = 0; v < V; ++v) mean[v] = m2[v] = 0.0f;
    if constexpr (!BWD) {
        // the wave that holds row 0 takes x[0] from there (RES); every other wave loads it
        if (!RES || wave != 0) {
            const ColVec<float, V> t = col_load<V>(a.x + base);
#pragma unroll
            for (int v = 0; v < V; ++v) x0[v] = t.v[v];
        }
    }

    const int n_super = RES ? 1 : (a.frames + W * R - 1) / (W * R);
    int n = 0;                     // rows merged so far
    for (int sb = 0; sb < n_super; ++sb) {
        const int tau0 = (sb * W + wave) * R;
        const int nb = cmvn_count(tau0, a.frames);
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (k < nb) {
                const long long off = base + (long long)(tau0 + k) * a.inner;
                in[k] = col_load<V>((BWD ? a.gy : a.x) + off);
                if constexpr (NEED_Y) yy[k] = col_load<V>(a.x + off);
            }
        float cm[V], cq[V];
        if constexpr (!BWD) {
            if (RES && wave == 0)
#pragma unroll
                for (int v = 0; v < V; ++v) x0[v] = in[0].v[v];
            if (nb > 0) cmvn_chunk<V, NORM>(in, x0, nb, cm, cq);
            else
#pragma unroll
                for (int v = 0; v < V; ++v) cm[v] = cq[v] = 0.0f;
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) cm[v] = cq[v] = 0.0f;
#pragma unroll
            for (int k = 0; k < R; ++k)
                if (k < nb)
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        cm[v] += in[k].v[v];
                        if constexpr (NEED_Y) cq[v] = fmaf(in[k].v[v], yy[k].v[v], cq[v]);
                    }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            slab[sb & 1][0][wave][v][lane] = cm[v];
            if constexpr (NORM) slab[sb & 1][1][wave][v][lane] = cq[v];
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int nw = cmvn_count((sb * W + w) * R, a.frames);
            if (nw > 0) {
                float mb[V], qb[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    mb[v] = slab[sb & 1][0][w][v][lane];
                    qb[v] = NORM ? slab[sb & 1][1][w][v][lane] : 0.0f;
                }
                if constexpr (!BWD) {
                    cmvn_merge<V, NORM>(n, nw, mb, qb, mean, m2);
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        mean[v] += mb[v];
                        if constexpr (NORM) m2[v] += qb[v];
                    }
                }
                n += nw;
            }
        }
    }

    // the column's statistics: every wave holds them
    const float fn = (float)a.frames;
    float rstd[V], mgy[V];
#pragma unroll
    for (int v = 0; v < V; ++v) rstd[v] = mgy[v] = 0.0f;
    if constexpr (!BWD) {
        if constexpr (NORM) {
#pragma unroll
            for (int v = 0; v < V; ++v) rstd[v] = __builtin_amdgcn_rsqf(m2[v] / fn + a.eps);
            if (MODE == CMVN_FWD_RSTD && wave == 0 && cg.live) {
                ColVec<float, V> o;
#pragma unroll
                for (int v = 0; v < V; ++v) o.v[v] = rstd[v];
                col_store<V>(a.rstd_out + col, o);
            }
        }
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            mean[v] = mean[v] / fn;                                  // mean(gy)
            if constexpr (NORM) mgy[v] = m2[v] / fn;                 // mean(gy y)
        }
        if constexpr (NORM) {
            const ColVec<float, V> t = col_load<V>(a.rstd + col);
#pragma unroll
            for (int v = 0; v < V; ++v) rstd[v] = t.v[v];
        }
    }

    // the outputs: from the registers (RES), or in a second sweep over the rows (STR)
    for (int sb = 0; sb < n_super; ++sb) {
        const int tau0 = (sb * W + wave) * R;
        const int nb = cmvn_count(tau0, a.frames);
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (k < nb) {
                const long long off = base + (long long)(tau0 + k) * a.inner;
                if constexpr (!RES) {
                    in[k] = col_load<V>((BWD ? a.gy : a.x) + off);
                    if constexpr (NEED_Y) yy[k] = col_load<V>(a.x + off);
                    if constexpr (!BWD) {
#pragma clang fp contract(off)
#pragma unroll
                        for (int v = 0; v < V; ++v) in[k].v[v] = in[k].v[v] - x0[v];
                    }
                }
                ColVec<float, V> o;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if constexpr (BWD) o.v[v] = cmvn_bwd_out<NORM>(in[k].v[v], NEED_Y ? yy[k].v[v] : 0.0f, mean[v], mgy[v], rstd[v]);
                    else o.v[v] = cmvn_out<NORM>(in[k].v[v], mean[v], rstd[v]);
                }
                if (cg.live) col_store<V>(a.out + off, o);
            }
    }
}

}  // namespace kpr
