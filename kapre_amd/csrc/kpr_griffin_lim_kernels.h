// kpr_griffin_lim_kernels.h -- Griffin-Lim phase reconstruction (kapre_amd.GriffinLim): what one iteration needs between the
// inverse and the forward transform, which are the library's own launches (kpr_host_griffin_lim.h chains them).
// Part of the single translation unit kapre_hip.hip (included there after kpr_augment_kernels.h, whose philox4x32_10 it uses, and
// kpr_misc_kernels.h, whose db_split it uses).
//
//   k_gl_init     mag = M^(1/power) and S_0 = mag e^{i phi}: phi = 0, or drawn per element from Philox4x32-10
//   k_gl_advance  the generator state's `calls` + 1, behind k_gl_init in stream order
//   k_gl_project  S = mag a / (|a| + 1e-16), a = R - c T (the fast Griffin-Lim momentum term of Perraudin, Balazs, Sondergaard 2013),
//                 and per (item, chunk) the two sums of the spectral convergence: (|R| - mag)^2 and mag^2
//   k_gl_finish   sc[item] = sqrt(sum num / sum den) over the item's chunks, in ascending order, one wave per item
//
// All of them are flat streams over the spectrogram's memory: an element is one complex bin, and nothing but k_gl_init's random
// draw knows the layout.  No float atomics and no cross-workgroup wait: the same inputs give the same bits.
#pragma once

namespace kpr {

constexpr int kGlChunk = 2048;         // most elements (bins) of one item that a workgroup of k_gl_project owns
constexpr float kGlTiny = 1e-16f;      // the guard of the projection's quotient (librosa, torchaudio)

struct GlSums {
    float num, den;
};

// S = mag a / (|a| + tiny) for one bin; the sums of its item take (|R| - mag)^2 and mag^2
template <bool MOM>
KPR_DEV float2 gl_project_one(float2 r, float2 t, float m, float c, GlSums& s) {
    const float d = sqrtf(fmaf(r.x, r.x, r.y * r.y)) - m;
    s.num = fmaf(d, d, s.num);
    s.den = fmaf(m, m, s.den);
    float2 a = r;
    if (MOM) {
        a.x = fmaf(-c, t.x, r.x);
        a.y = fmaf(-c, t.y, r.y);
    }
    const float q = m / (sqrtf(fmaf(a.x, a.x, a.y * a.y)) + kGlTiny);
    return make_float2(q * a.x, q * a.y);
}

// R, T (MOM only), S: complex64, mag: float32, n_items blocks of item_size elements each.  A workgroup owns at most kGlChunk
// consecutive elements of one item (k_specaug_apply's rule: `chunks` equal parts).  VEC = 4: every base is 16-byte aligned, so an
// element index that is a multiple of 4 starts a 16-byte word of mag and a 32-byte pair of R / T / S; the aligned middle of the range
// moves in such groups -- five 16-byte loads in flight per lane and group with momentum, three without, two groups per round (one round is a whole chunk) --
// and the up to 3 + 3 elements around it one by one.  VEC = 1: unaligned bases.
// part (may be NULL): float32 [n_items][chunks][2] = the lanes' sums of this workgroup, reduced in a fixed order.
template <int VEC, bool MOM>
__global__ __launch_bounds__(256) void k_gl_project(const float2* __restrict__ R, const float2* __restrict__ T,
                                                    const float* __restrict__ mag, long long item_size, int chunks, float c,
                                                    float2* __restrict__ S, float* __restrict__ part) {
    __shared__ GlSums red[4];
    const long long item = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)(item * chunks);
    const long long per = (item_size + chunks - 1) / chunks;       // <= kGlChunk (host)
    const long long lo = min(item_size, chunk * per), hi = min(item_size, lo + per);
    const long long g0 = item * item_size + lo, g1 = item * item_size + hi;
    long long a0, a1;
    db_split<VEC>(g0, g1, a0, a1);
    GlSums s{0.0f, 0.0f};
    for (int side = 0; side < 2; ++side) {                  // scalar head [g0, a0) and tail [a1, g1)
        const long long p0 = side ? a1 : g0, p1 = side ? g1 : a0;
        for (long long i = p0 + threadIdx.x; i < p1; i += blockDim.x)
            S[i] = gl_project_one<MOM>(R[i], MOM ? T[i] : make_float2(0.0f, 0.0f), mag[i], c, s);
    }
    if constexpr (VEC == 4) {
        const float4* r4 = reinterpret_cast<const float4*>(R);      // two bins per float4
        const float4* t4 = reinterpret_cast<const float4*>(T);
        const float4* m4 = reinterpret_cast<const float4*>(mag);    // four bins per float4
        float4* s4 = reinterpret_cast<float4*>(S);
        auto group = [&](long long g, float4 ra, float4 rb, float4 ta, float4 tb, float4 m) {
            const float2 o0 = gl_project_one<MOM>(make_float2(ra.x, ra.y), make_float2(ta.x, ta.y), m.x, c, s);
            const float2 o1 = gl_project_one<MOM>(make_float2(ra.z, ra.w), make_float2(ta.z, ta.w), m.y, c, s);
            const float2 o2 = gl_project_one<MOM>(make_float2(rb.x, rb.y), make_float2(tb.x, tb.y), m.z, c, s);
            const float2 o3 = gl_project_one<MOM>(make_float2(rb.z, rb.w), make_float2(tb.z, tb.w), m.w, c, s);
            s4[2 * g] = make_float4(o0.x, o0.y, o1.x, o1.y);
            s4[2 * g + 1] = make_float4(o2.x, o2.y, o3.x, o3.y);
        };
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const long long ghi = a1 / VEC;
        long long g = a0 / VEC + threadIdx.x;
        for (; g + blockDim.x < ghi; g += 2 * (long long)blockDim.x) {         // two groups in flight
            const long long h = g + blockDim.x;
            const float4 m_0 = m4[g], m_1 = m4[h];
            const float4 ra0 = r4[2 * g], rb0 = r4[2 * g + 1], ra1 = r4[2 * h], rb1 = r4[2 * h + 1];
            float4 ta0 = z, tb0 = z, ta1 = z, tb1 = z;
            if (MOM) { ta0 = t4[2 * g]; tb0 = t4[2 * g + 1]; ta1 = t4[2 * h]; tb1 = t4[2 * h + 1]; }
            group(g, ra0, rb0, ta0, tb0, m_0);
            group(h, ra1, rb1, ta1, tb1, m_1);
        }
        for (; g < ghi; g += blockDim.x)
            group(g, r4[2 * g], r4[2 * g + 1], MOM ? t4[2 * g] : z, MOM ? t4[2 * g + 1] : z, m4[g]);
    }
    if (!part) return;                                      // (uniform: a kernel argument)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s.num += __shfl_xor(s.num, o, 64);
        s.den += __shfl_xor(s.den, o, 64);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = part + 2 * (long long)blockIdx.x;
        p[0] = ((red[0].num + red[1].num) + red[2].num) + red[3].num;
        p[1] = ((red[0].den + red[1].den) + red[2].den) + red[3].den;
    }
}

// sc[item] = sqrt(sum num / sum den): one wave per item.  The lanes fetch 64 chunk pairs at a time (one coalesced load), then every
// lane adds them in ascending chunk order, in double, reading lane k's pair with v_readlane (k is uniform): the order of the sum
// is the chunk order whatever the count, and no load waits for an addition.
// An item without energy (mag == 0 everywhere) gives 0 / 0 = NaN, as the definition does.
__global__ __launch_bounds__(64) void k_gl_finish(const float* __restrict__ part, int chunks, float* __restrict__ sc) {
    const float2* p = reinterpret_cast<const float2*>(part) + (long long)blockIdx.x * chunks;
    double num = 0.0, den = 0.0;
    for (int k0 = 0; k0 < chunks; k0 += 64) {
        const int n = min(64, chunks - k0);
        float2 v = make_float2(0.0f, 0.0f);
        if ((int)threadIdx.x < n) v = p[k0 + threadIdx.x];
        for (int k = 0; k < n; ++k) {
            num += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), k));
            den += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), k));
        }
    }
    if (threadIdx.x == 0) sc[blockIdx.x] = (float)sqrt(num / den);
}

// The random phase of element e (its index in the channels_first order (batch, ch, frame, bin), whatever the layout in memory):
// word e mod 4 of Philox4x32-10 with counter (e div 4, calls) and key seed; phi = 2 pi r 2^-32, evaluated as
// sincospi((int)r 2^-31) -- the same angle, and the conversion of r then rounds by at most 2^-25 of a half turn.
KPR_DEV float2 gl_unit(unsigned r) {
    float sn, cs;
    sincospif((float)(int)r * 4.656612873077392578125e-10f, &sn, &cs);
    return make_float2(cs, sn);
}
KPR_DEV void gl_draw4(unsigned long long group, unsigned long long seed, unsigned long long calls, unsigned (&c)[4]) {
    c[0] = (unsigned)group; c[1] = (unsigned)(group >> 32); c[2] = (unsigned)calls; c[3] = (unsigned)(calls >> 32);
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
}

struct GlInitArgs {
    const float* M;
    float* mag;                        // NULL: power == 1, M is the magnitude
    float2* S;                         // NULL: only mag is wanted (a caller-supplied S_0 with power != 1)
    const unsigned long long* state;   // RAND: (seed, calls), read only
    long long n;                       // elements
    long long plane;                   // frames * bins
    int C;                             // channels interleaved in memory (channels_last with more than one), else 1
    float inv_power;
};

KPR_DEV float gl_root(float m, float inv_power) {
    return inv_power == 1.0f ? m : inv_power == 0.5f ? sqrtf(m) : powf(m, inv_power);
}

// A grid-stride stream over groups of VEC elements (VEC = 4: M, mag and S 16-byte aligned and n % 4 == 0 is not needed: the last
// up to three elements go one by one).  The draw of an element depends on its index alone: with C == 1 a group of four
// elements is one Philox block; with interleaved channels every element finds its own block.
template <int VEC, bool RAND>
__global__ __launch_bounds__(256) void k_gl_init(GlInitArgs a) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    unsigned long long seed = 0, calls = 0;
    if (RAND) { seed = a.state[0]; calls = a.state[1]; }
    auto canon = [&](long long m) -> unsigned long long {          // memory index -> index in the channels_first order
        if (a.C == 1) return (unsigned long long)m;
        const long long per_item = a.plane * a.C, b = m / per_item, rem = m - b * per_item;
        const long long fk = rem / a.C, ch = rem - fk * a.C;
        return (unsigned long long)((b * a.C + ch) * a.plane + fk);
    };
    auto one = [&](long long i) {
        const float m = gl_root(a.M[i], a.inv_power);
        if (a.mag) a.mag[i] = m;
        if (!a.S) return;
        float2 u = make_float2(1.0f, 0.0f);
        if (RAND) {
            const unsigned long long e = canon(i);
            unsigned c[4];
            gl_draw4(e >> 2, seed, calls, c);
            const unsigned w = (unsigned)e & 3u;
            u = gl_unit(w == 0 ? c[0] : w == 1 ? c[1] : w == 2 ? c[2] : c[3]);
        }
        a.S[i] = make_float2(m * u.x, m * u.y);
    };
    const long long step = (long long)gridDim.x * blockDim.x, tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nv = VEC == 4 ? a.n / 4 : 0;
    if constexpr (VEC == 4) {
        const vf* m4 = reinterpret_cast<const vf*>(a.M);
        vf* o4 = reinterpret_cast<vf*>(a.mag);
        float4* s4 = reinterpret_cast<float4*>(a.S);
        for (long long g = tid; g < nv; g += step) {
            vf m = m4[g];
#pragma unroll
            for (int u = 0; u < VEC; ++u) m[u] = gl_root(m[u], a.inv_power);
            if (a.mag) o4[g] = m;
            if (!a.S) continue;
            float2 ph[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) ph[u] = make_float2(1.0f, 0.0f);
            if (RAND) {
                unsigned c[4];
                if (a.C == 1) {
                    gl_draw4((unsigned long long)g, seed, calls, c);
#pragma unroll
                    for (int u = 0; u < 4; ++u) ph[u] = gl_unit(c[u]);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const unsigned long long e = canon(4 * g + u);
                        gl_draw4(e >> 2, seed, calls, c);
                        const unsigned w = (unsigned)e & 3u;
                        ph[u] = gl_unit(w == 0 ? c[0] : w == 1 ? c[1] : w == 2 ? c[2] : c[3]);
                    }
                }
            }
            s4[2 * g] = make_float4(m[0] * ph[0].x, m[0] * ph[0].y, m[1] * ph[1].x, m[1] * ph[1].y);
            s4[2 * g + 1] = make_float4(m[2] * ph[2].x, m[2] * ph[2].y, m[3] * ph[3].x, m[3] * ph[3].y);
        }
    }
    for (long long i = nv * 4 + tid; i < a.n; i += step) one(i);
}

// One wave: every lane reads the state before the barrier, one lane stores calls + 1 behind it (k_specaug_draw's ending).  It is a
// launch of its own because k_gl_init reads the state from many workgroups: only the stream orders their reads before this store.
__global__ __launch_bounds__(64) void k_gl_advance(unsigned long long* state) {
    const unsigned long long calls = state[1];
    __syncthreads();
    if (threadIdx.x == 0) state[1] = calls + 1;
}

}  // namespace kpr
