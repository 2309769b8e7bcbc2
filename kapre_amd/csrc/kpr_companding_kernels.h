// kpr_companding_kernels.h -- mu-law companding (signal.py:236-361 over backend.py:302-341) and ConcatenateFrequencyMap
// (time_frequency.py:647-744) with their backward passes.  Part of the single translation unit kapre_hip.hip.
//
// All of them stream: every output word is written once, every input word read once, no LDS.  The access pattern is driven
// by the OUTPUT: a lane owns four consecutive output words and stores them with one 16-byte access on the 16-byte aligned
// middle of the range; the up to 3 + 3 words around it are stored one by one.  What a lane reads for its four words is a
// 16-byte load wherever the four sources are consecutive -- at whatever 4-byte aligned address they lie (load16 below) -- so
// a view that starts on any word, and an input whose alignment differs from the output's, take the same kernel.
#pragma once

namespace kpr {

constexpr int kStreamUnroll = 4;                           // 16-byte loads a lane has in flight
constexpr int kStreamChunk = 256 * kStreamUnroll;          // 16-byte groups per workgroup
constexpr long long kCompandMaxElems = 1LL << 40;          // elements per call (the grid: 2^28 workgroups of 4096)

typedef unsigned cw4 __attribute__((ext_vector_type(4)));

// four consecutive words from a 4-byte aligned address (the compiler picks one 16-byte access where the target allows it)
KPR_DEV cw4 load16(const unsigned* p) {
    cw4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// words of the head in front of the first 16-byte boundary of p (p is 4-byte aligned), at most n
KPR_DEV unsigned head_words(const void* p, unsigned long long n) {
    const unsigned h = (4u - (unsigned)(((unsigned long long)p >> 2) & 3u)) & 3u;
    return (unsigned long long)h < n ? h : (unsigned)n;
}

// ------------------------------------------------------------------------------------------
// mu-law.  mu = Q - 1, log1p(mu) = ln Q.
//   encode: v = sign(x) log1p(mu |x|) / ln Q, code = int32(trunc((v + 1) / 2 * mu + 0.5))
//           = trunc(fma(copysign(log2(fma(mu, |x|, 1)) / log2 Q, x), mu / 2, Q / 2)): what decides the code is the ABSOLUTE
//           error of v, so the relative accuracy log1p buys near 0 is not needed and one v_log_f32 does; mu / 2 and Q / 2 are
//           exact.  A NaN gives code 0.
//   decode: s = 2 code / mu - 1 = k / mu with k = 2 code - mu (exact for integer codes),
//           out = sign(s) (exp(|s| ln Q) - 1) / mu = sign(k) (exp2(|k| c) - 1) / mu, c = log2(Q) / mu.
//           |k| c reaches 16, where one float32 rounding is 2^-21 and costs 3e-7 of the result; so c is carried as hi + lo,
//           p = |k| c_hi rounded, e = its exact remainder (fma) + |k| c_lo, and exp2(p + e) = exp2(p) (1 + e ln 2).  1 / mu
//           is carried the same way.
//   decode backward (float codes): d out / d code = 2 ln Q / mu^2 exp(|s| ln Q).
// ------------------------------------------------------------------------------------------
struct MuLawDev {
    float mu, half_mu, half_q, inv_log2q;    // encode
    float c_hi, c_lo, inv_hi, inv_lo;        // decode
    float gcoef;                             // 2 ln Q / mu^2
};

enum { MU_ENCODE = 0, MU_DECODE_I32 = 1, MU_DECODE_F32 = 2, MU_DECODE_BWD = 3 };

KPR_DEV float mu_expand(float k, const MuLawDev& p) {       // exp(|s| ln Q) of k = 2 code - mu
    const float ak = fabsf(k);
    const float q = ak * p.c_hi;
    float e = fmaf(ak, p.c_hi, -q);
    e = fmaf(ak, p.c_lo, e);
    const float E = __builtin_amdgcn_exp2f(q);
    return fmaf(E * 0.693147180559945309f, e, E);
}

template <int OP>
KPR_DEV unsigned mu_word(unsigned w, unsigned gw, const MuLawDev& p) {
    if (OP == MU_ENCODE) {
        const float x = __uint_as_float(w);
        const float t = __builtin_amdgcn_logf(fmaf(p.mu, fabsf(x), 1.0f)) * p.inv_log2q;
        const float v = fmaf(copysignf(t, x), p.half_mu, p.half_q);
        return v == v ? (unsigned)(int)v : 0u;
    }
    const float code = OP == MU_DECODE_I32 ? (float)(int)w : __uint_as_float(w);
    const float k = fmaf(2.0f, code, -p.mu);
    const float E = mu_expand(k, p);
    if (OP == MU_DECODE_BWD) return __float_as_uint(__uint_as_float(gw) * (p.gcoef * E));
    const float d = E - 1.0f;
    return __float_as_uint(copysignf(fmaf(d, p.inv_hi, d * p.inv_lo), k));
}

// in / g / out: n 4-byte words each (g only for MU_DECODE_BWD).  A workgroup owns kStreamChunk 16-byte groups of the aligned
// middle; workgroup 0 also stores the head and the tail.  out == in is allowed (a lane stores exactly the words it loaded).
template <int OP>
__global__ __launch_bounds__(256) void k_mu_law(const unsigned* in, const unsigned* g, unsigned* out, long long n, MuLawDev p) {
    const unsigned head = head_words(out, (unsigned long long)n);
    const long long nv = (n - head) >> 2;
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const unsigned tail = (unsigned)(n - head - 4 * nv);
        const long long i = threadIdx.x < 4 ? (long long)threadIdx.x : (long long)head + 4 * nv + (threadIdx.x - 4);
        if (threadIdx.x < 4 ? threadIdx.x < head : threadIdx.x - 4 < tail)
            out[i] = mu_word<OP>(in[i], OP == MU_DECODE_BWD ? g[i] : 0u, p);
    }
    const long long v0 = (long long)blockIdx.x * kStreamChunk + threadIdx.x;
    cw4 a[kStreamUnroll], b[kStreamUnroll];
#pragma unroll
    for (int q = 0; q < kStreamUnroll; ++q) {
        const long long v = v0 + q * 256;
        if (v < nv) {
            a[q] = load16(in + head + 4 * v);
            if (OP == MU_DECODE_BWD) b[q] = load16(g + head + 4 * v);
        }
    }
#pragma unroll
    for (int q = 0; q < kStreamUnroll; ++q) {
        const long long v = v0 + q * 256;
        if (v < nv) {
            cw4 r;
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = mu_word<OP>(a[q][u], OP == MU_DECODE_BWD ? b[q][u] : 0u, p);
            *reinterpret_cast<cw4*>(out + head + 4 * v) = r;
        }
    }
}

// ------------------------------------------------------------------------------------------
// ConcatenateFrequencyMap and its adjoint.  Per batch item the output is rows of `rin` input words followed by `rmap` map
// words: channels_last (T, F, C) -> (T, F, C + 1): rin = C, rmap = 1, the map word of row r is bin r % F;
// channels_first (C, T, F) -> (C + 1, T, F): one row, rin = C T F, rmap = T F, map word j is bin j % F.
// The adjoint (DROP) copies the first rin words of every row of rin + rmap.
// An item has fewer than 2^31 output words (host), so everything below the item base is 32-bit arithmetic.
// map(f) = f / (F - 1) as f * (1 / (F - 1)) -- two roundings, within 2^-24 of the quotient -- with 1.0 written at f = F - 1;
// F == 1: last = -1 and inv = 0, the one bin holds 0.0.
// ------------------------------------------------------------------------------------------
struct FmapArgs {
    unsigned rin, rmap, n_freq, osz;    // osz: words of one item of the kernel's OUTPUT
    int last;
    float inv;
    int chunks;                         // workgroups per item
};

template <bool DROP, bool CL>
__global__ __launch_bounds__(256) void k_freq_map(const unsigned* __restrict__ in, unsigned* __restrict__ out, FmapArgs a) {
    const unsigned item = blockIdx.x / a.chunks, chunk = blockIdx.x - item * a.chunks;
    const unsigned rout = a.rin + a.rmap;
    const unsigned rows = (DROP ? a.osz / a.rin : a.osz / rout);
    const unsigned* src = in + (long long)item * rows * (DROP ? rout : a.rin);
    unsigned* dst = out + (long long)item * a.osz;
    const unsigned head = head_words(dst, a.osz);
    const unsigned nv = (a.osz - head) >> 2;

    auto fmap = [&](unsigned f) -> unsigned { return __float_as_uint((int)f == a.last ? 1.0f : (float)f * a.inv); };
    auto one = [&](unsigned l) -> unsigned {               // output word l of the item
        if (DROP) {
            const unsigned r = CL ? l / a.rin : 0u, c = l - r * a.rin;
            return src[r * rout + c];
        }
        const unsigned r = CL ? l / rout : 0u, c = l - r * rout;
        if (c < a.rin) return src[r * a.rin + c];
        return fmap(CL ? r % a.n_freq : (c - a.rin) % a.n_freq);
    };

    if (chunk == 0 && threadIdx.x < 8) {
        const unsigned tail = a.osz - head - 4 * nv;
        const unsigned l = threadIdx.x < 4 ? threadIdx.x : head + 4 * nv + (threadIdx.x - 4);
        if (threadIdx.x < 4 ? threadIdx.x < head : threadIdx.x - 4 < tail) dst[l] = one(l);
    }
#pragma unroll
    for (int q = 0; q < kStreamUnroll; ++q) {
        const unsigned v = chunk * kStreamChunk + q * 256 + threadIdx.x;
        if (v >= nv) continue;
        const unsigned l = head + 4 * v;
        cw4 r;
        if (!CL) {                                          // one row: consecutive words on both sides
            if (DROP || l + 3 < a.rin) {
                r = load16(src + l);
            } else if (l >= a.rin) {
                unsigned f = (l - a.rin) % a.n_freq;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    r[u] = fmap(f);
                    f = f + 1 == a.n_freq ? 0u : f + 1;
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = one(l + u);
            }
        } else {
            const unsigned rlen = DROP ? a.rin : rout;
            unsigned row = l / rlen, c = l - row * rlen;
            if (c + 3 < a.rin) {
                r = load16(src + row * (DROP ? rout : a.rin) + c);
            } else {
                unsigned f = DROP ? 0u : row % a.n_freq;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    r[u] = c < a.rin ? src[row * (DROP ? rout : a.rin) + c] : fmap(f);
                    if (++c == rlen) {
                        c = 0;
                        ++row;
                        f = f + 1 == a.n_freq ? 0u : f + 1;
                    }
                }
            }
        }
        *reinterpret_cast<cw4*>(dst + l) = r;
    }
}

}  // namespace kpr
