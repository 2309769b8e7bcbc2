// kpr_mix_kernels.h -- AddNoise (augmentation.AddNoise, backend.add_noise): a noise signal that tiles circularly, mixed into a
// waveform at a requested signal-to-noise ratio, and the input gradient of that.  Part of the single translation unit kapre_hip.hip
// (included there after kpr_misc_kernels.h, whose db_split it uses).
//
// An item is the n = C T floats of one batch entry; float e of it belongs to sample t = e mod T (channels_first or mono: C rows of T) or
// t = e / C (channels_last), and its noise sample is seg[t] = noise_k[(o + t) mod L] with (k, o, snr) the item's row of the int32
// draw table (index, offset, snr as float32 bits, 0) and L = lengths[k]; k, L and o are clamped into the bank here, whatever the
// table holds.
//   forward   Sx = sum a^2 over the item, Sn = sum seg^2 over t (counted on the floats of channel 0), both float64 sums of the exact
//             products; g = (float)(sqrt((Sx / (C T)) / (Sn / T)) 10^(-snr / 20)), +0 when Sx == 0 or Sn == 0;
//             out = fmaf(g, seg, a)
//   backward  D = sum a seg over the item (a: the cotangent), coef = (float)((D g) / Sx) with (Sx, g) of the forward's stats row, 0
//             when Sx == 0; out = fmaf(coef, b, a) (b: the forward's input, read plainly)
// Two forms.  Streamed: k_mix_sums leaves one pair of float64 partial sums per chunk of kMixChunk floats in a workspace
// [item][chunk][2]; every workgroup of k_mix_apply adds its item's pairs in ascending chunk order -- so all of them form the same
// bits -- and streams its chunk.  Resident: one 1024-lane workgroup per item keeps the item in registers (kMixResPerLane floats per
// lane) between its sums and its FMAs: one launch, one read.  No atomics in either; within a form the order of every sum is fixed
// by the geometry, so the same call gives the same bits; the two forms sum in different orders and agree within the error bound only.
// The stats row of an item: float64 (Sx, Sn, g, D).
#pragma once

namespace kpr {

constexpr int kMixChunk = 8192;            // floats of one item per workgroup of the streamed form
constexpr int kMixResPerLane = 48;         // floats per lane of the resident form: 12 x 16 bytes, or 48 words
constexpr int kMixResMax = 1024 * kMixResPerLane;   // 49152 floats per item (a second of 44.1 kHz mono is 44100)

struct MixArgs {
    const float* a;          // forward: x; backward: the cotangent
    const float* b;          // backward: the forward's x; forward: not read
    const float* noise;      // (n_noise, stride)
    const int* lengths;      // n_noise
    const int* table;        // (items, 4)
    float* out;
    double* stats;           // (items, 4) written (may be NULL in the backward pass)
    const double* stats_in;  // backward: the forward's rows
    double* ws;              // streamed form: (items, chunks, 2)
    unsigned n, C, T, cf;    // cf: the floats of a channel are consecutive (channels_first, or one channel)
    int n_noise, chunks;
    long long stride;
};

struct MixItem {
    const float* seg;        // the item's noise row
    unsigned L, o;
    float snr;
};

KPR_DEV MixItem mix_item(const MixArgs& m, long long item) {
    const int* row = m.table + 4 * item;                    // wave-uniform
    const int k = min(max(row[0], 0), m.n_noise - 1);
    MixItem it;
    it.seg = m.noise + (long long)k * m.stride;
    it.L = (unsigned)min((long long)max(m.lengths[k], 1), m.stride);
    it.o = (unsigned)min(max(row[1], 0), (int)it.L - 1);
    it.snr = __int_as_float(row[2]);
    return it;
}

// The noise position of a float, carried along without a division per sample: c counts inside the period M (the channel of a
// channels_last float, the sample of a channels_first one), p = (o + t) mod L.  A step of n floats is (nc, np) = (n mod C,
// (n / C) mod L) and p moves one further when c wraps [channels_last], or (n mod T, (n mod T) mod L) and p moves back by T when c
// wraps [channels_first]; p stays below 3 L before the two conditional subtractions.
struct MixStep {
    unsigned nc, np;
};
struct MixWalk {
    unsigned M, L, T, wadj, cf;     // uniform
    unsigned c, p;                  // of this lane
    KPR_DEV MixWalk(const MixArgs& m, const MixItem& it) : M(m.cf ? m.T : m.C), L(it.L), T(m.T), cf(m.cf), c(0), p(0) {
        wadj = m.cf ? (L - m.T % L) % L : 1u % L;
    }
    KPR_DEV MixStep stride(unsigned n) const {
        if (cf) return MixStep{n % M, (n % M) % L};
        return MixStep{n % M, (n / M) % L};
    }
    KPR_DEV void seek(unsigned e, unsigned o) {
        const unsigned q = e / M;
        c = e - q * M;
        p = (o + (cf ? c : q)) % L;
    }
    KPR_DEV void step(const MixStep& s) {
        c += s.nc;
        p += s.np;
        if (c >= M) { c -= M; p += wadj; }
        if (p >= L) p -= L;
        if (p >= L) p -= L;
    }
    KPR_DEV bool first(unsigned e) const { return cf ? e < T : c == 0; }     // a float of channel 0
};

// The noise samples r[u] of the VEC floats from float e0 on (w stands on e0); bit u of the result: float e0 + u belongs to channel 0.
// VEC floats of one channels_first row whose samples do not wrap are VEC consecutive noise samples: one 16-byte load from a
// 4-byte aligned address.  Everything else walks float by float.
template <int VEC>
KPR_DEV unsigned mix_fetch(const MixWalk& w, const MixStep& s1e, const float* seg, unsigned e0, float (&r)[VEC]) {
    if (VEC > 1 && w.cf && w.c + VEC <= w.M && w.p + VEC <= w.L) {
        typedef float vfu __attribute__((ext_vector_type(VEC), aligned(4)));
        const vfu t = *reinterpret_cast<const vfu*>(seg + w.p);
#pragma unroll
        for (int u = 0; u < VEC; ++u) r[u] = t[u];
        return e0 < w.T ? (1u << VEC) - 1u : 0u;
    }
    MixWalk e = w;
    unsigned fm = 0u;
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
        r[u] = seg[e.p];
        fm |= (e.first(e0 + u) ? 1u : 0u) << u;
        e.step(s1e);
    }
    return fm;
}

KPR_DEV double mix_wave_sum(double v) {                     // every lane ends with the same bits (a + b == b + a)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the workgroup's two sums in every lane: lanes of a wave by butterfly, the NW waves through LDS in ascending order
template <int NW>
KPR_DEV void mix_block_sum(double& s0, double& s1, double* sh) {
    s0 = mix_wave_sum(s0);
    s1 = mix_wave_sum(s1);
    if ((threadIdx.x & 63) == 0) {
        sh[2 * (threadIdx.x >> 6)] = s0;
        sh[2 * (threadIdx.x >> 6) + 1] = s1;
    }
    __syncthreads();
    s0 = 0.0;
    s1 = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        s0 += sh[2 * w];
        s1 += sh[2 * w + 1];
    }
}

KPR_DEV double mix_snr_factor(float snr) { return pow(10.0, -(double)snr / 20.0); }
KPR_DEV float mix_gain(double Sx, double Sn, double factor, unsigned C, unsigned T) {
    if (Sx == 0.0 || Sn == 0.0) return 0.0f;
    return (float)(sqrt((Sx / ((double)C * (double)T)) / (Sn / (double)T)) * factor);
}
KPR_DEV float mix_coef(double D, double g, double Sx) { return Sx == 0.0 ? 0.0f : (float)((D * g) / Sx); }

template <bool BWD>
KPR_DEV void mix_acc(double& s0, double& s1, float av, float sv, bool first) {
    if (BWD) {
        s0 += (double)av * (double)sv;
    } else {
        s0 += (double)av * (double)av;
        if (first) s1 += (double)sv * (double)sv;
    }
}

// Streamed form, launch 1: the partial sums of chunk (item, chunk).  16-byte loads of `a` on the aligned middle of the chunk, four
// in flight per lane, scalar loads on the up to 3 + 3 floats around it (VEC = 4); VEC = 1: bases that are not 16-byte aligned.
template <int VEC, bool BWD>
__global__ __launch_bounds__(256) void k_mix_sums(MixArgs m) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    __shared__ double sh[8];
    const long long item = blockIdx.x / m.chunks;
    const unsigned chunk = blockIdx.x - (unsigned)(item * m.chunks);
    const unsigned lo = chunk * kMixChunk, hi = min(m.n, lo + kMixChunk);
    const MixItem it = mix_item(m, item);
    MixWalk w(m, it);
    const long long base = item * m.n, g0 = base + lo, g1 = base + hi;
    long long a0, a1;
    db_split<VEC>(g0, g1, a0, a1);
    const unsigned B = blockDim.x;
    const MixStep s1e = w.stride(1), sB = w.stride(B);
    double s0 = 0.0, s1 = 0.0;
    for (int part = 0; part < 2; ++part) {                  // scalar head [g0, a0) and tail [a1, g1)
        const long long p0 = part ? a1 : g0, p1 = part ? g1 : a0;
        long long i = p0 + threadIdx.x;
        if (i < p1) w.seek((unsigned)(i - base), it.o);
        for (; i < p1; i += B) {
            mix_acc<BWD>(s0, s1, m.a[i], it.seg[w.p], w.first((unsigned)(i - base)));
            w.step(sB);
        }
    }
    if (VEC == 4) {
        const vf* ai = reinterpret_cast<const vf*>(m.a);
        const MixStep sV = w.stride(B * VEC);
        const long long vhi = a1 / VEC;
        long long i = a0 / VEC + threadIdx.x;
        if (i < vhi) w.seek((unsigned)(i * VEC - base), it.o);
        auto take = [&](const vf& v, long long iv) {        // the VEC floats from float iv * VEC on; w stands on the first
            float r[VEC];
            const unsigned fm = mix_fetch<VEC>(w, s1e, it.seg, (unsigned)(iv * VEC - base), r);
#pragma unroll
            for (int u = 0; u < VEC; ++u) mix_acc<BWD>(s0, s1, v[u], r[u], (fm >> u) & 1u);
            w.step(sV);
        };
        for (; i + 3 * (long long)B < vhi; i += 4 * (long long)B) {
            vf v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = ai[i + q * (long long)B];
#pragma unroll
            for (int q = 0; q < 4; ++q) take(v[q], i + q * (long long)B);
        }
        for (; i < vhi; i += B) take(ai[i], i);
    }
    mix_block_sum<4>(s0, s1, sh);
    if (threadIdx.x == 0) {
        double* dst = m.ws + 2 * ((long long)item * m.chunks + chunk);
        dst[0] = s0;
        dst[1] = s1;
    }
}

// Streamed form, launch 2: the item's sums from the workspace (every lane of every workgroup of the item adds the same pairs in the
// same order: uniform loads, no barrier), the scale s = g or coef, then out = fmaf(s, second, a) over the chunk, the second operand
// being the wrapped noise (forward) or b (backward).  The workgroup of chunk 0 writes the item's stats row.
template <int VEC, bool BWD>
__global__ __launch_bounds__(256) void k_mix_apply(MixArgs m) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    const long long item = blockIdx.x / m.chunks;
    const unsigned chunk = blockIdx.x - (unsigned)(item * m.chunks);
    const unsigned lo = chunk * kMixChunk, hi = min(m.n, lo + kMixChunk);
    const MixItem it = mix_item(m, item);
    double S0 = 0.0, S1 = 0.0;
    const double* part = m.ws + 2 * (long long)item * m.chunks;
    for (int k = 0; k < m.chunks; ++k) {
        S0 += part[2 * k];
        S1 += part[2 * k + 1];
    }
    float s;
    if (BWD) {
        const double Sx = m.stats_in[4 * item], Sn = m.stats_in[4 * item + 1], g = m.stats_in[4 * item + 2];
        s = mix_coef(S0, g, Sx);
        if (m.stats && chunk == 0 && threadIdx.x == 0) {
            double* st = m.stats + 4 * item;
            st[0] = Sx; st[1] = Sn; st[2] = g; st[3] = S0;
        }
    } else {
        s = mix_gain(S0, S1, mix_snr_factor(it.snr), m.C, m.T);
        if (chunk == 0 && threadIdx.x == 0) {
            double* st = m.stats + 4 * item;
            st[0] = S0; st[1] = S1; st[2] = (double)s; st[3] = 0.0;
        }
    }
    MixWalk w(m, it);
    const long long base = item * m.n, g0 = base + lo, g1 = base + hi;
    long long a0, a1;
    db_split<VEC>(g0, g1, a0, a1);
    const unsigned B = blockDim.x;
    const MixStep s1e = w.stride(1), sB = w.stride(B);
    for (int pt = 0; pt < 2; ++pt) {                        // scalar head [g0, a0) and tail [a1, g1)
        const long long p0 = pt ? a1 : g0, p1 = pt ? g1 : a0;
        long long i = p0 + threadIdx.x;
        if (!BWD && i < p1) w.seek((unsigned)(i - base), it.o);
        for (; i < p1; i += B) {
            m.out[i] = fmaf(s, BWD ? m.b[i] : it.seg[w.p], m.a[i]);
            if (!BWD) w.step(sB);
        }
    }
    if (VEC == 4) {
        const vf* ai = reinterpret_cast<const vf*>(m.a);
        const vf* bi = reinterpret_cast<const vf*>(m.b);
        vf* oi = reinterpret_cast<vf*>(m.out);
        const MixStep sV = w.stride(B * VEC);
        const long long vhi = a1 / VEC;
        long long i = a0 / VEC + threadIdx.x;
        if (!BWD && i < vhi) w.seek((unsigned)(i * VEC - base), it.o);
        auto second = [&](long long iv) -> vf {
            if (BWD) return bi[iv];
            float f[VEC];
            mix_fetch<VEC>(w, s1e, it.seg, (unsigned)(iv * VEC - base), f);
            vf r;
#pragma unroll
            for (int u = 0; u < VEC; ++u) r[u] = f[u];
            w.step(sV);
            return r;
        };
        for (; i + 3 * (long long)B < vhi; i += 4 * (long long)B) {
            vf v[4], r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = ai[i + q * (long long)B];
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = second(i + q * (long long)B);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int u = 0; u < VEC; ++u) v[q][u] = fmaf(s, r[q][u], v[q][u]);
                oi[i + q * (long long)B] = v[q];
            }
        }
        for (; i < vhi; i += B) {
            vf v = ai[i];
            const vf r = second(i);
#pragma unroll
            for (int u = 0; u < VEC; ++u) v[u] = fmaf(s, r[u], v[u]);
            oi[i] = v;
        }
    }
}

// Resident form: one workgroup of 1024 lanes per item of at most kMixResMax floats.  Lane l holds the floats (q 1024 + l) VEC ...
// + VEC - 1, q = 0 ... 48 / VEC - 1, from one load each; the sums go lane -> wave (butterfly) -> LDS (one barrier), float64; the
// FMAs run from the registers.  VEC = 4: n % 4 == 0 behind 16-byte aligned bases (every item then starts aligned); VEC = 1 otherwise.
template <int VEC, bool BWD>
__global__ __launch_bounds__(1024) void k_mix_res(MixArgs m) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    constexpr int NQ = kMixResPerLane / VEC;
    // the noise loads of at most this many steps are in flight at once: without the fence between groups hipcc hoists all NQ of
    // them above the arithmetic and the item no longer fits the 128 registers of a lane
    constexpr int kMixResGroup = VEC == 4 ? 4 : 8;
    __shared__ double sh[32];
    const long long item = blockIdx.x;
    const MixItem it = mix_item(m, item);
    const long long base = item * m.n;
    const vf* ai = reinterpret_cast<const vf*>(m.a + base);
    const unsigned nv = m.n / VEC;                          // (VEC == 4: n % 4 == 0)
    MixWalk w(m, it);
    const MixStep s1e = w.stride(1), sV = w.stride(1024 * VEC);
    // 10^(-snr / 20) first, while the registers are free: pow() next to a resident item does not fit a lane's 128
    double factor = BWD ? 0.0 : mix_snr_factor(it.snr);
    asm volatile("" : "+v"(factor) : : "memory");
    // this lane holds the steps q < qn.  qn goes through an empty asm in front of every pass: the 48 comparisons are formed
    // again there instead of waiting in 96 scalar registers (and, spilled, in vector registers) from the first pass on
    unsigned qn = threadIdx.x < nv ? (nv - threadIdx.x + 1023u) >> 10 : 0u;
    vf v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const unsigned iv = q * 1024 + threadIdx.x;
        if (q < qn) v[q] = ai[iv];
    }
    double s0 = 0.0, s1 = 0.0;
    w.seek(min(threadIdx.x * VEC, m.n - 1), it.o);
    const MixWalk w0 = w;
    asm volatile("" : "+v"(qn));
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const unsigned iv = q * 1024 + threadIdx.x;
        if (q < qn) {
            float r[VEC];
            const unsigned fm = mix_fetch<VEC>(w, s1e, it.seg, iv * VEC, r);
#pragma unroll
            for (int u = 0; u < VEC; ++u) mix_acc<BWD>(s0, s1, v[q][u], r[u], (fm >> u) & 1u);
        }
        w.step(sV);
        if (q % kMixResGroup == kMixResGroup - 1) asm volatile("" ::: "memory");
    }
    mix_block_sum<16>(s0, s1, sh);
    float s;
    if (BWD) {
        const double Sx = m.stats_in[4 * item], Sn = m.stats_in[4 * item + 1], g = m.stats_in[4 * item + 2];
        s = mix_coef(s0, g, Sx);
        if (m.stats && threadIdx.x == 0) {
            double* st = m.stats + 4 * item;
            st[0] = Sx; st[1] = Sn; st[2] = g; st[3] = s0;
        }
    } else {
        s = mix_gain(s0, s1, factor, m.C, m.T);
        if (threadIdx.x == 0) {
            double* st = m.stats + 4 * item;
            st[0] = s0; st[1] = s1; st[2] = (double)s; st[3] = 0.0;
        }
    }
    const vf* bi = reinterpret_cast<const vf*>(BWD ? m.b + base : m.a);
    vf* oi = reinterpret_cast<vf*>(m.out + base);
    w = w0;
    asm volatile("" : "+v"(w.c), "+v"(w.p), "+v"(qn));     // walk again: the positions of the first pass must not stay in registers
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const unsigned iv = q * 1024 + threadIdx.x;
        if (q < qn) {
            vf r;
            if (BWD) {
                r = bi[iv];
            } else {
                float f[VEC];
                mix_fetch<VEC>(w, s1e, it.seg, iv * VEC, f);
#pragma unroll
                for (int u = 0; u < VEC; ++u) r[u] = f[u];
            }
            vf o = v[q];
#pragma unroll
            for (int u = 0; u < VEC; ++u) o[u] = fmaf(s, r[u], o[u]);
            oi[iv] = o;
        }
        if (!BWD) w.step(sV);
        if (q % kMixResGroup == kMixResGroup - 1) asm volatile("" ::: "memory");
    }
}

}  // namespace kpr
