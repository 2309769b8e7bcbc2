// kpr_pcen_kernels.h -- per-channel energy normalisation (Wang et al. 2017) and its input gradient: the one kernel family of
// the library whose hot loop is a recurrence along time.  Part of the single translation unit kapre_hip.hip.
//
//   S[0] = E[0], S[t] = a S[t-1] + s E[t] (a = 1 - s);  y[t] = (E[t] (eps + S[t])^-alpha + delta)^r - delta^r
//   backward: G = (eps + S)^-alpha, u = E G + delta, p = gy r u^(r-1), q = -alpha p E G / (eps + S);
//             N[t] = q[t] + a N[t+1], N[F] = 0;  gE[t] = p G + s N[t] (t >= 1), gE[0] = p G + N[0]
//
// Both layouts are one problem: a contiguous (outer, F, inner) tensor scanned along F; the band of inner index i is
// i / band_div (channels_first: band_div 1, channels_last: band_div C).  A lane owns one column group -- four consecutive
// inner indices of one outer item, loaded and stored with 16-byte accesses (V = 4; inner % 4 == 0 and 16-byte aligned
// bases), or a single column (V = 1) -- and column groups are numbered through all outer items, so 64 consecutive groups
// fill a wave whatever `inner` is.
//
// Time is tiled.  A workgroup of W waves owns 64 column groups; one step covers a super-block of W * R rows: wave w
// loads its R rows (R independent 16-byte loads per lane in flight), runs the recurrence over them from a ZERO carry-in
// and leaves the end value L_w in LDS.  After one barrier every wave walks the W end values in order,
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

enum { PCEN_FWD = 0, PCEN_FWD_SMOOTH = 1, PCEN_BWD = 2 };

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
};

// x^p for a normal x > 0.  log2 x is taken as k + log2 m (x = m 2^k, m in [0.5, 1)): the logarithm of the mantissa has an absolute
// error of 2^-24, where log2 x itself, about -20 for a quiet band, would carry 2^-19 -- 1.3e-6 of the power.  p k is split into
// its rounded value and the exact remainder, which joins the small term; one exponential each.  The product of the two is rounded
// here (no contraction into the caller's subtraction of delta^r: equal arguments must give equal results, bit for bit).
KPR_DEV float pcen_pow(float x, float p) {
#pragma clang fp contract(off)
    const float k = (float)__builtin_amdgcn_frexp_expf(x);
    const float l = __builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(x));
    const float hi = p * k;
    const float lo = fmaf(p, l, fmaf(p, k, -hi));
    return __builtin_amdgcn_exp2f(hi) * __builtin_amdgcn_exp2f(lo);
}

template <int V>
struct PcenVec {
    float v[V];
};

template <int V>
KPR_DEV PcenVec<V> pcen_load(const float* p) {
    PcenVec<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int V>
KPR_DEV void pcen_store(float* p, const PcenVec<V>& r) {
    if constexpr (V == 4)
        *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else
        *p = r.v[0];
}

template <int V, int MODE>
__global__ __launch_bounds__(64 * kPcenWaves) void k_pcen(PcenArgs a) {
    constexpr int R = kPcenRows, W = kPcenWaves;
    constexpr bool BWD = MODE == PCEN_BWD;
    __shared__ float ends[2][W][V][64];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long group = (long long)blockIdx.x * 64 + lane;
    const bool live = group < a.n_groups;
    // (a lane past the last group runs along on group 0 with its stores masked: the barrier needs every wave)
    const long long gsafe = live ? group : 0;
    const long long item = gsafe / a.groups_per_item;
    const unsigned i0 = (unsigned)(gsafe - item * a.groups_per_item) * V;
    const long long base = item * (long long)a.frames * a.inner + i0;

    float ps[V], pa[V], palpha[V], pdelta[V], pr[V], pdr[V], paR[V], state[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const unsigned band = (i0 + v) / a.band_div;
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

    const int n_super = (a.frames + W * R - 1) / (W * R);
    for (int sb = 0; sb < n_super; ++sb) {
        // scan position tau runs forward in time (FWD) or backward (BWD); row(tau) is the frame it names
        const int tau0 = (sb * W + wave) * R;
        PcenVec<V> in[R];          // FWD: E.  BWD: q
        PcenVec<V> dir[R];         // BWD: gy r u^(r-1) G, the part of gE that does not pass through S
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int tau = tau0 + k;
            const bool ok = tau < a.frames;
            const long long off = base + (long long)(BWD ? a.frames - 1 - tau : tau) * a.inner;
            if (!BWD) {
                if (ok) in[k] = pcen_load<V>(a.x + off);
                else
#pragma unroll
                    for (int v = 0; v < V; ++v) in[k].v[v] = 0.0f;
            } else {
                PcenVec<V> e, sm, g;
                if (ok) {
                    e = pcen_load<V>(a.x + off);
                    sm = pcen_load<V>(a.smooth + off);
                    g = pcen_load<V>(a.gy + off);
                }
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if (ok) {
                        const float es = a.eps + sm.v[v];
                        const float G = pcen_pow(es, -palpha[v]);
                        const float u = fmaf(e.v[v], G, pdelta[v]);
                        const float p = g.v[v] * pr[v] * pcen_pow(u, pr[v] - 1.0f);
                        const float d = p * G;
                        dir[k].v[v] = d;
                        in[k].v[v] = -palpha[v] * d * e.v[v] * __builtin_amdgcn_rcpf(es);
                    } else {
                        dir[k].v[v] = 0.0f;
                        in[k].v[v] = 0.0f;
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
            PcenVec<V> o, sm;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (BWD) {
                    carry[v] = fmaf(pa[v], carry[v], in[k].v[v]);
                    o.v[v] = fmaf(tau == a.frames - 1 ? 1.0f : ps[v], carry[v], dir[k].v[v]);
                } else {
                    carry[v] = tau == 0 ? in[k].v[v] : fmaf(pa[v], carry[v], ps[v] * in[k].v[v]);
                    sm.v[v] = carry[v];
                    const float G = pcen_pow(a.eps + carry[v], -palpha[v]);
                    o.v[v] = pcen_pow(fmaf(in[k].v[v], G, pdelta[v]), pr[v]) - pdr[v];
                }
            }
            if (live && tau < a.frames) {
                const long long off = base + (long long)(BWD ? a.frames - 1 - tau : tau) * a.inner;
                pcen_store<V>(a.out + off, o);
                if (MODE == PCEN_FWD_SMOOTH) pcen_store<V>(a.smooth_out + off, sm);
            }
        }
    }
}

}  // namespace kpr
