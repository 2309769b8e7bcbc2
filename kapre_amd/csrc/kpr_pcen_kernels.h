// kpr_pcen_kernels.h -- per-channel energy normalisation (Wang et al. 2017) and its input gradient: the one kernel family of
// the library whose hot loop is a recurrence along time.  Part of the single translation unit kapre_hip.hip.
//
//   S[0] = E[0], S[t] = a S[t-1] + s E[t] (a = 1 - s);  y[t] = (E[t] (eps + S[t])^-alpha + delta)^r - delta^r
//   backward: G = (eps + S)^-alpha, u = E G + delta, p = gy r u^(r-1), q = -alpha p E G / (eps + S);
//             N[t] = q[t] + a N[t+1], N[F] = 0;  gE[t] = p G + s N[t] (t >= 1), gE[0] = p G + N[0]
//
// Both layouts are one problem: a contiguous (outer, F, inner) tensor scanned along F; the band of inner index i is
// i / band_div (channels_first: band_div 1, channels_last: band_div C).  Column groups (V = 4 or 1 floats), super-blocks of
// W * R rows and the one barrier are those of kpr_cols.h.
//
// Wave w loads its R rows (R independent 16-byte loads per lane in flight), runs the recurrence over them from a ZERO carry-in
// and leaves the end value L_w in LDS.  After the barrier every wave walks the W end values in order,
// c_(w+1) = a^R c_w + L_w from the state the previous super-block left -- the recurrence is linear, so the carry-in of a
// chunk only adds a^k carry -- and thereby holds both its own carry-in and, redundantly, the state after the super-block.
// It then runs the recurrence a second time over its registers from the true carry-in: each S[t] is produced by exactly
// the arithmetic of the sequential loop, only the carry-in took the chunked route; no table of powers a^1 .. a^R is
// needed (a^R alone, computed once per lane before the time loop).  The LDS slab is double-buffered, which makes the one
// barrier per super-block sufficient.  The backward kernel is the same scan in reversed time over q.
// The block is read once and written once; nothing but E (and S, gy) crosses HBM.
//
// Powers go through v_log_f32 / v_exp_f32: x^p = exp2(p log2 x) (pcen_pow).  delta^r comes out of the same routine as
// (. + delta)^r, so E[t] = 0 gives exactly 0.0.  Every base is >= eps or >= delta for a non-negative E: no denormal reaches the logarithm.
#pragma once

namespace kpr {

constexpr int kPcenRows = 8;       // R: rows a wave holds in registers per super-block
constexpr int kPcenWaves = 8;      // W: waves of a workgroup = time chunks of a super-block

// PCEN_BWD_PARAMS: the input gradient and the per-column partial sums of the four parameter gradients;
// PCEN_BWD_PARAMS_ONLY: the partial sums alone (a frozen front end: three streams read, nothing of block size written)
enum { PCEN_FWD = 0, PCEN_FWD_SMOOTH = 1, PCEN_BWD = 2, PCEN_BWD_PARAMS = 3, PCEN_BWD_PARAMS_ONLY = 4 };

struct PcenArgs {
    const float* x;
    const float* smooth;           // BWD: S of the forward pass
    const float* gy;               // BWD
    float* out;                    // y, or gE
    float* smooth_out;             // FWD_SMOOTH
    const float *s, *alpha, *delta, *r;
    float eps;
    int frames;
    unsigned inner;                // elements of one row
    unsigned groups_per_item;      // inner / V
    unsigned band_div;
    long long n_groups;            // outer * groups_per_item
    float* partials;               // BWD_PARAMS*: (4, outer * inner) sums over time per column, rows s, alpha, delta, r
};

// x^p for a normal x > 0.  log2 x is taken as k + log2 m (x = m 2^k, m in [0.5, 1)): the logarithm of the mantissa has an absolute
// error of 2^-24, where log2 x itself, about -20 for a quiet band, would carry 2^-19 -- 1.3e-6 of the power.  p k is split into
// its rounded value and the exact remainder, which joins the small term; one exponential each.  The product of the two is rounded
// here (no contraction into the caller's subtraction of delta^r: equal arguments must give equal results, bit for bit).
// The logarithm is a value of its own (PcenLog), so that the parameter gradients take ln x = (k + log2 m) ln 2 from the one the
// power already needed.
struct PcenLog {
    float k, l;                    // x = m 2^k: k, log2 m
};

KPR_DEV PcenLog pcen_log(float x) {
    PcenLog r;
    r.k = (float)__builtin_amdgcn_frexp_expf(x);
    r.l = __builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(x));
    return r;
}

KPR_DEV float pcen_exp(PcenLog lg, float p) {
#pragma clang fp contract(off)
    const float hi = p * lg.k;
    const float lo = fmaf(p, lg.l, fmaf(p, lg.k, -hi));
    return __builtin_amdgcn_exp2f(hi) * __builtin_amdgcn_exp2f(lo);
}

KPR_DEV float pcen_pow(float x, float p) { return pcen_exp(pcen_log(x), p); }

// ln x of a taken logarithm: k + log2 m is rounded once (|k + log2 m| 2^-24), the logarithm of the mantissa is good to 2^-24 absolute
KPR_DEV float pcen_ln(PcenLog lg) {
#pragma clang fp contract(off)
    return (lg.k + lg.l) * 0.693147180559945309f;
}

// One element's terms of the alpha, delta and r gradients, added to the lane's running sums (every operation rounded on its
// own: the sums must not depend on what else the instance computes).
//   alpha: -p E G ln(eps + S);  delta: gy r (u^(r-1) - delta^(r-1));  r: gy (u^r ln u - delta^r ln delta), u^r = u u^(r-1)
// E = 0 makes u = delta bit for bit, and the constants come out of the same routines: the delta and r terms are then exactly 0.
KPR_DEV void pcen_param_terms(float e, float g, float gr, float G, float p, float pw, float u, PcenLog les, PcenLog lu, float pd1,
                              float cr, float& s_alpha, float& s_delta, float& s_r) {
#pragma clang fp contract(off)
    s_alpha = s_alpha - p * e * G * pcen_ln(les);
    s_delta = s_delta + gr * (pw - pd1);
    s_r = s_r + g * (u * pw * pcen_ln(lu) - cr);
}

template <int V, int MODE>
__global__ __launch_bounds__(64 * kPcenWaves) void k_pcen(PcenArgs a) {
    constexpr int R = kPcenRows, W = kPcenWaves;
    constexpr bool BWD = MODE >= PCEN_BWD;
    constexpr bool PARAMS = MODE == PCEN_BWD_PARAMS || MODE == PCEN_BWD_PARAMS_ONLY;   // the parameter gradients' partial sums
    constexpr bool OUT = MODE != PCEN_BWD_PARAMS_ONLY;                                 // y, or gE, is written
    // PARAMS: four slabs, which after the time loop hold the W waves' sums of the four parameters
    __shared__ float ends[PARAMS ? 4 : 2][W][V][64];

    const ColGroup cg = col_group<V>(a.n_groups, a.groups_per_item);
    const int lane = cg.lane, wave = threadIdx.x >> 6;
    const long long base = cg.item * (long long)a.frames * a.inner + cg.i0;

    float ps[V], pa[V], palpha[V], pdelta[V], pr[V], pdr[V], paR[V], state[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const unsigned band = (cg.i0 + v) / a.band_div;
        ps[v] = a.s[band];
        palpha[v] = a.alpha[band];
        pdelta[v] = a.delta[band];
        pr[v] = a.r[band];
        pa[v] = 1.0f - ps[v];
        pdr[v] = pcen_pow(pdelta[v], pr[v]);
        float t = pa[v];
#pragma unroll
        for (int k = 1; k < R; ++k) t *= pa[v];
        paR[v] = t;
        state[v] = 0.0f;
    }
    // PARAMS: delta^(r-1), delta^r ln delta, and the lane's sums over its time chunks, [parameter][v] in the table's order
    float pd1[V], pcr[V], sums[4][V];
    if constexpr (PARAMS) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const PcenLog ld = pcen_log(pdelta[v]);
            pd1[v] = pcen_exp(ld, pr[v] - 1.0f);
            pcr[v] = pdelta[v] * pd1[v] * pcen_ln(ld);
#pragma unroll
            for (int q = 0; q < 4; ++q) sums[q][v] = 0.0f;
        }
    }

    const int n_super = (a.frames + W * R - 1) / (W * R);
    for (int sb = 0; sb < n_super; ++sb) {
        // scan position tau runs forward in time (FWD) or backward (BWD); row(tau) is the frame it names
        const int tau0 = (sb * W + wave) * R;
        ColVec<float, V> in[R];          // FWD: E.  BWD: q
        ColVec<float, V> dir[R];         // BWD: gy r u^(r-1) G, the part of gE that does not pass through S
        // PARAMS: E[t] - S[t-1], which waits for N[t] behind the barrier.  S[t-1] is the next row of the scan: the wave's own
        // rows, and one more row of `smooth` behind the chunk (never (E - S) / a: 0 / 0 at s = 1)
        ColVec<float, V> step[PARAMS ? R : 1], srow[PARAMS ? R + 1 : 1];
        if constexpr (PARAMS) {
#pragma unroll
            for (int k = 0; k <= R; ++k) {
                const int tau = tau0 + k;
                if (tau < a.frames) srow[k] = col_load<V>(a.smooth + base + (long long)(a.frames - 1 - tau) * a.inner);
                else
#pragma unroll
                    for (int v = 0; v < V; ++v) srow[k].v[v] = 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int tau = tau0 + k;
            const bool ok = tau < a.frames;
            const long long off = base + (long long)(BWD ? a.frames - 1 - tau : tau) * a.inner;
            if (!BWD) {
                if (ok) in[k] = col_load<V>(a.x + off);
                else
#pragma unroll
                    for (int v = 0; v < V; ++v) in[k].v[v] = 0.0f;
            } else {
                ColVec<float, V> e, sm, g;
                if (ok) {
                    e = col_load<V>(a.x + off);
                    if constexpr (PARAMS) sm = srow[k];
                    else sm = col_load<V>(a.smooth + off);
                    g = col_load<V>(a.gy + off);
                }
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if (ok) {
                        const float es = a.eps + sm.v[v];
                        const PcenLog les = pcen_log(es);
                        const float G = pcen_exp(les, -palpha[v]);
                        const float u = fmaf(e.v[v], G, pdelta[v]);
                        const PcenLog lu = pcen_log(u);
                        const float pw = pcen_exp(lu, pr[v] - 1.0f);
                        const float gr = g.v[v] * pr[v];
                        const float p = gr * pw;
                        const float d = p * G;
                        dir[k].v[v] = d;
                        in[k].v[v] = -palpha[v] * d * e.v[v] * __builtin_amdgcn_rcpf(es);
                        if constexpr (PARAMS) {
                            pcen_param_terms(e.v[v], g.v[v], gr, G, p, pw, u, les, lu, pd1[v], pcr[v], sums[1][v], sums[2][v],
                                             sums[3][v]);
                            step[k].v[v] = e.v[v] - srow[k + 1].v[v];
                        }
                    } else {
                        dir[k].v[v] = 0.0f;
                        in[k].v[v] = 0.0f;
                        if constexpr (PARAMS) step[k].v[v] = 0.0f;
                    }
                }
            }
        }
        // chunk end value from a zero carry-in.  FWD: the first frame of all starts the smoother, S[0] = E[0]
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0f;
#pragma unroll
        for (int k = 0; k < R; ++k)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (BWD) acc[v] = fmaf(pa[v], acc[v], in[k].v[v]);
                else if (k == 0) acc[v] = tau0 == 0 ? in[0].v[v] : ps[v] * in[0].v[v];
                else acc[v] = fmaf(pa[v], acc[v], ps[v] * in[k].v[v]);
            }
#pragma unroll
        for (int v = 0; v < V; ++v) ends[sb & 1][wave][v][lane] = acc[v];
        __syncthreads();
        float carry[V];
#pragma unroll
        for (int v = 0; v < V; ++v) carry[v] = state[v];
#pragma unroll
        for (int w = 0; w < W; ++w)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (w == wave) carry[v] = state[v];
                state[v] = fmaf(paR[v], state[v], ends[sb & 1][w][v][lane]);
            }
        // the recurrence once more, from the true carry-in, and the outputs
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int tau = tau0 + k;
            ColVec<float, V> o, sm;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (BWD) {
                    carry[v] = fmaf(pa[v], carry[v], in[k].v[v]);
                    if constexpr (OUT) o.v[v] = fmaf(tau == a.frames - 1 ? 1.0f : ps[v], carry[v], dir[k].v[v]);
                    // s: N[t] (E[t] - S[t-1]) for t >= 1; frame 0 (S[0] = E[0]) and the rows past the block add nothing
                    if constexpr (PARAMS)
                        if (tau < a.frames - 1) sums[0][v] = fmaf(carry[v], step[k].v[v], sums[0][v]);
                } else {
                    carry[v] = tau == 0 ? in[k].v[v] : fmaf(pa[v], carry[v], ps[v] * in[k].v[v]);
                    sm.v[v] = carry[v];
                    const float G = pcen_pow(a.eps + carry[v], -palpha[v]);
                    o.v[v] = pcen_pow(fmaf(in[k].v[v], G, pdelta[v]), pr[v]) - pdr[v];
                }
            }
            if (OUT && cg.live && tau < a.frames) {
                const long long off = base + (long long)(BWD ? a.frames - 1 - tau : tau) * a.inner;
                col_store<V>(a.out + off, o);
                if (MODE == PCEN_FWD_SMOOTH) col_store<V>(a.smooth_out + off, sm);
            }
        }
    }
    if constexpr (PARAMS) {
        // the W waves' sums, added in the order of the waves: wave q (< 4) owns parameter q of the workgroup's columns
        __syncthreads();                                             // (the last super-block's end values have been read)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int v = 0; v < V; ++v) ends[q][wave][v][lane] = sums[q][v];
        __syncthreads();
        if (wave < 4 && cg.live) {
            ColVec<float, V> o;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float t = ends[wave][0][v][lane];
#pragma unroll
                for (int w = 1; w < W; ++w) t += ends[wave][w][v][lane];
                o.v[v] = t;
            }
            col_store<V>(a.partials + (long long)wave * a.n_groups * V + cg.group * V, o);
        }
    }
}

// (4, n_bands) parameter gradients from k_pcen<V, PCEN_BWD_PARAMS*>'s (4, outer, inner) partial sums: one workgroup per
// (parameter, band) adds the outer * band_div columns of the band in double -- thread t the columns t, t + 256, ..., then the
// 256 threads pairwise through LDS.  The order is a function of the shape alone: the same inputs give the same bits.
__global__ __launch_bounds__(256) void k_pcen_param_reduce(const float* __restrict__ partials, float* __restrict__ gparams,
                                                           long long outer, unsigned inner, unsigned band_div, unsigned n_bands) {
    __shared__ double part[256];
    const unsigned q = blockIdx.x / n_bands, band = blockIdx.x - q * n_bands;
    const float* src = partials + (long long)q * outer * inner + band * band_div;
    const long long n = outer * band_div;
    double t = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const long long item = i / band_div;
        t += (double)src[item * inner + (i - item * band_div)];
    }
    part[threadIdx.x] = t;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) gparams[blockIdx.x] = (float)part[0];
}

}  // namespace kpr
