// kpr_time_stretch_kernels.h -- phase-vocoder time stretching of a complex spectrogram (kapre_amd.TimeStretch): the second kernel
// family of the library, after PCEN, whose hot loop is a running sum along time.  Part of the single translation unit kapre_hip.hip.
//
//   output frame t reads the input rows i = idx[t] and i + 1 (rows >= frames_in are zero) with the weight a = alpha[t]:
//   Theta(x) = 2 rint(atan2f(im, re) c) as a 32-bit word, 2^32 = one turn, c = float32(2^30 / pi); 0 for a zero or non-finite bin
//   P[0] = Theta(X[0]),  P[t + 1] = P[t] + Theta(X[i + 1]) - Theta(X[i])                       (uint32: the sum wraps by itself)
//   m[t] = a |X[i + 1]| + (1 - a) |X[i]|,  |x| = sqrtf(re re + im im);   Y[t] = m[t] (cos, sin)(pi h),  h = (float)(int)P[t] 2^-31
//
// The expected phase advance of the textbook phase vocoder is absent: it enters the accumulated phase as a multiple of 2 pi
// (DESIGN 4.15).  Integer addition is associative, so the chunked sum below IS the sequential one, bit for bit.
//
// Column groups (V = 2 or 1 complex64 values), super-blocks of W * R OUTPUT frames and the one barrier are those of kpr_cols.h.
// A wave fetches the input rows its R frames need, forms Theta and |x|, sums its R phase increments from zero and leaves the word
// in LDS; after the barrier every wave adds the words of the waves before it to the state that the previous super-block left, and
// writes its rows.
//
// Row indices are the same for every lane, so they come from the table as scalar loads, and the wave picks one of two forms:
//   span form     idx[] does not fall and the R frames read at most R + 1 consecutive input rows (every rate <= 1): each INPUT row
//                 is loaded once and its Theta and |x| formed once -- R + 1 arc tangents for 2 R uses.  The frames that read the
//                 pair (j, j + 1) are emitted in a loop whose trip count is uniform: no register is indexed at run time.
//   general form  any table: both rows of every output frame are loaded and converted on their own.
// Theta and |x| are pure functions of a bin, so the two forms give the same bits.
#pragma once

namespace kpr {

constexpr int kPvRows = 8;         // R: output frames of a wave per super-block
constexpr int kPvWaves = 8;        // W: waves of a workgroup = time chunks of a super-block

struct PvArgs {
    const float2* x;
    float2* out;
    unsigned* phase;               // may be NULL: the phase words P[t], in out's layout
    const int* idx;                // frames_out entries
    const float* alpha;            // frames_out entries
    int frames_in, frames_out;
    unsigned inner;                // complex values of one row
    unsigned groups_per_item;      // inner / V
    long long n_groups;            // outer * groups_per_item
};

// the angle word of a bin: atan2f is in [-pi, pi], the product below 2^30 (1 + 2^-23) in magnitude; the factor 2 is a shift of the
// integer, so that +-pi wraps to the same word instead of saturating the conversion
KPR_DEV unsigned pv_angle(float2 z) {
#pragma clang fp contract(off)
    constexpr float c = (float)(1073741824.0 / 3.14159265358979323846);
    const bool ok = (z.x != 0.0f || z.y != 0.0f) && fabsf(z.x) < INFINITY && fabsf(z.y) < INFINITY;
    const unsigned w = (unsigned)(int)rintf(atan2f(z.y, z.x) * c) << 1;
    return ok ? w : 0u;
}

KPR_DEV float pv_abs(float2 z) { return sqrtf(fmaf(z.x, z.x, z.y * z.y)); }

KPR_DEV float pv_mix(float a, float one_minus_a, float lo, float hi) {
#pragma clang fp contract(off)
    return a * hi + one_minus_a * lo;
}

// one output row of a lane: Y = m (cos, sin)(pi h) and, when asked for, the phase words
template <int V>
KPR_DEV void pv_emit(const PvArgs& a, long long off, bool live, const unsigned (&P)[V], const float (&m)[V]) {
    ColVec<float2, V> o;
    ColVec<unsigned, V> p;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float sn, cs;
        sincospif((float)(int)P[v] * 4.656612873077392578125e-10f, &sn, &cs);
        o.v[v] = make_float2(m[v] * cs, m[v] * sn);
        p.v[v] = P[v];
    }
    if (!live) return;
    col_store<V>(a.out + off, o);
    if (a.phase) col_store<V>(a.phase + off, p);
}

template <int V>
__global__ __launch_bounds__(64 * kPvWaves) void k_time_stretch(PvArgs a) {
    constexpr int R = kPvRows, W = kPvWaves;
    __shared__ unsigned ends[2][W][V][64];

    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const ColGroup cg = col_group<V>(a.n_groups, a.groups_per_item);
    const int lane = cg.lane;
    const float2* xin = a.x + cg.item * (long long)a.frames_in * a.inner + cg.i0;
    const long long out_base = cg.item * (long long)a.frames_out * a.inner + cg.i0;

    // input row r of the lane's columns; the rows from frames_in on (the two padding frames; any index that is no row) are zero
    auto row = [&](unsigned r) -> ColVec<float2, V> {
        ColVec<float2, V> z;
#pragma unroll
        for (int v = 0; v < V; ++v) z.v[v] = make_float2(0.0f, 0.0f);
        if (r < (unsigned)a.frames_in) z = col_load<V>(xin + (long long)r * a.inner);
        return z;
    };

    typedef const int __attribute__((address_space(4)))* ConstI32;
    typedef const float __attribute__((address_space(4)))* ConstF32;
    const ConstI32 idx = (ConstI32)(unsigned long long)a.idx;
    const ConstF32 alpha = (ConstF32)(unsigned long long)a.alpha;

    unsigned state[V];             // P[first frame of the super-block]
    {
        const ColVec<float2, V> z = row(0u);
#pragma unroll
        for (int v = 0; v < V; ++v) state[v] = pv_angle(z.v[v]);
    }

    const int n_super = (a.frames_out + W * R - 1) / (W * R);
    for (int sb = 0; sb < n_super; ++sb) {
        const int t0 = (sb * W + wave) * R;
        const int nk = min(R, a.frames_out - t0);                     // frames of this wave (<= 0: none; it still meets the barrier)
        // the table entries of the R frames: uniform, and loaded through the constant address space (the host keeps the tables
        // clear of the outputs), hence scalar loads.  A frame past the last repeats the last entry: idx[] stays non-decreasing
        unsigned ia[R];
        float al[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int t = min(t0 + k, a.frames_out - 1);
            ia[k] = (unsigned)idx[t];
            al[k] = alpha[t];
        }
        bool rising = true;
#pragma unroll
        for (int k = 1; k < R; ++k) rising = rising && ia[k] >= ia[k - 1];
        const bool span = rising && ia[R - 1] - ia[0] <= (unsigned)(R - 1);

        // span form: Theta and |x| of the input rows ia[0] .. ia[0] + R, and how many frames read each pair
        unsigned th[R + 1][V];
        float mg[R + 1][V];
        int cnt[R];
        // general form: the increment and the magnitude of every frame
        unsigned inc[R][V];
        float mk[R][V];
        unsigned tot[V];
#pragma unroll
        for (int v = 0; v < V; ++v) tot[v] = 0u;

        if (nk > 0 && span) {
            ColVec<float2, V> in[R + 1];
#pragma unroll
            for (int j = 0; j <= R; ++j) in[j] = row(ia[0] + (unsigned)j);
#pragma unroll
            for (int j = 0; j <= R; ++j)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    th[j][v] = pv_angle(in[j].v[v]);
                    mg[j][v] = pv_abs(in[j].v[v]);
                }
#pragma unroll
            for (int j = 0; j < R; ++j) {
                int c = 0;
#pragma unroll
                for (int k = 0; k < R; ++k) c += (k < nk && ia[k] - ia[0] == (unsigned)j) ? 1 : 0;
                cnt[j] = c;
#pragma unroll
                for (int v = 0; v < V; ++v) tot[v] += (unsigned)c * (th[j + 1][v] - th[j][v]);
            }
        } else if (nk > 0) {
            ColVec<float2, V> lo[R], hi[R];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                lo[k] = row(ia[k]);
                hi[k] = row(ia[k] + 1u);
            }
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const float om = 1.0f - al[k];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    inc[k][v] = k < nk ? pv_angle(hi[k].v[v]) - pv_angle(lo[k].v[v]) : 0u;
                    mk[k][v] = pv_mix(al[k], om, pv_abs(lo[k].v[v]), pv_abs(hi[k].v[v]));
                    tot[v] += inc[k][v];
                }
            }
        }

#pragma unroll
        for (int v = 0; v < V; ++v) ends[sb & 1][wave][v][lane] = tot[v];
        __syncthreads();
        unsigned carry[V];
#pragma unroll
        for (int v = 0; v < V; ++v) carry[v] = state[v];
#pragma unroll
        for (int w = 0; w < W; ++w)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const unsigned e = ends[sb & 1][w][v][lane];
                if (w < wave) carry[v] += e;
                state[v] += e;
            }

        if (nk > 0 && span) {
            int k = 0;
#pragma unroll
            for (int j = 0; j < R; ++j)
                for (int n = 0; n < cnt[j]; ++n, ++k) {
                    const float ak = alpha[t0 + k], om = 1.0f - ak;
                    float m[V];
#pragma unroll
                    for (int v = 0; v < V; ++v) m[v] = pv_mix(ak, om, mg[j][v], mg[j + 1][v]);
                    pv_emit<V>(a, out_base + (long long)(t0 + k) * a.inner, cg.live, carry, m);
#pragma unroll
                    for (int v = 0; v < V; ++v) carry[v] += th[j + 1][v] - th[j][v];
                }
        } else if (nk > 0) {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                if (k < nk) pv_emit<V>(a, out_base + (long long)(t0 + k) * a.inner, cg.live, carry, mk[k]);
#pragma unroll
                for (int v = 0; v < V; ++v) carry[v] += inc[k][v];
            }
        }
    }
}

}  // namespace kpr
