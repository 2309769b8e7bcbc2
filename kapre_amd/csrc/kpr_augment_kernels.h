// kpr_augment_kernels.h -- the training-only layers of kapre/augmentation.py: SpecAugment (draw + apply) and ChannelSwap (gather).
// Part of the single translation unit kapre_hip.hip (included there after kpr_misc_kernels.h, whose db_split it uses).
//
// SpecAugment draws its masks ON THE DEVICE: the generator state (uint64 seed, uint64 calls) lives in device memory, so a training
// step needs no host-to-device copy and a captured hipGraph draws new masks at every replay.  The generator is Philox4x32-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter based, so the draw of (item, mask) does not
// depend on the launch geometry.  The mask table is int32 [n_items][n_time_masks + n_freq_masks][2] = (first, last), both
// inclusive (augmentation.py:211-214 masks `start <= i <= start + width`), time masks first.
#pragma once

namespace kpr {

constexpr int kAugMaxMasks = 32;       // masks per axis (host check)
constexpr int kAugMaxFreq = 65536;     // bins per row: the frequency mask of an item is a bitmap in LDS (8 KiB)
constexpr int kAugChunk = 8192;        // most floats of one item that a workgroup of k_specaug_apply copies
constexpr int kGatherMaxCh = 64;       // channels whose permutation travels in the kernel arguments

struct AugGeom {
    int n_items, n_tm, n_fm, n_time, n_freq, tparam, fparam;
};

// c = Philox4x32-10(counter c, key (k0, k1))
KPR_DEV void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// One workgroup.  Entry (item, m): counter (item, m, calls_lo, calls_hi), key (seed_lo, seed_hi);
// width = mulhi(r0, param) in 0 .. param - 1, first = mulhi(r1, limit - width) in 0 .. limit - width - 1, last = first + width.
// The host guarantees 1 <= param <= limit on an axis that has masks, so limit - width >= 1 and last <= limit - 1.
// Every lane reads the state before the barrier; one lane stores calls + 1 behind it.
__global__ __launch_bounds__(1024) void k_specaug_draw(int* __restrict__ table, AugGeom a, unsigned long long* state) {
    const unsigned long long seed = state[0], calls = state[1];
    const int nm = a.n_tm + a.n_fm;
    const int n = a.n_items * nm;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int item = e / nm, m = e - item * nm;
        unsigned c[4] = {(unsigned)item, (unsigned)m, (unsigned)calls, (unsigned)(calls >> 32)};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        const bool time = m < a.n_tm;
        const unsigned param = time ? a.tparam : a.fparam, limit = time ? a.n_time : a.n_freq;
        const unsigned width = __umulhi(c[0], param);
        const unsigned first = __umulhi(c[1], limit - width);
        table[2 * e] = (int)first;
        table[2 * e + 1] = (int)(first + width);
    }
    __syncthreads();
    if (threadIdx.x == 0) state[1] = calls + 1;
}

// One workgroup, the same state and the same generator as k_specaug_draw.  Entry item: counter (item, 0, calls_lo, calls_hi),
// key (seed_lo, seed_hi); out[item] = mulhi(r0, n_choices), uniform in 0 .. n_choices - 1 (augmentation.Reverb: which impulse
// response an item gets).  One lane stores calls + 1 behind the barrier.
__global__ __launch_bounds__(1024) void k_index_draw(int* __restrict__ out, int n_items, unsigned n_choices, unsigned long long* state) {
    const unsigned long long seed = state[0], calls = state[1];
    for (int e = threadIdx.x; e < n_items; e += blockDim.x) {
        unsigned c[4] = {(unsigned)e, 0u, (unsigned)calls, (unsigned)(calls >> 32)};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        out[e] = (int)__umulhi(c[0], n_choices);
    }
    __syncthreads();
    if (threadIdx.x == 0) state[1] = calls + 1;
}

// One workgroup, the same state and the same generator again (augmentation.AddNoise: which noise, from where, how loud).  Entry
// item: counter (item, 0, calls_lo, calls_hi), key (seed_lo, seed_hi) -> r0, r1, r2; the int32[4] row of the item is
//   index  = mulhi(r0, n_noise)                       uniform in 0 .. n_noise - 1
//   offset = mulhi(r1, lengths[index])                uniform in 0 .. L - 1 (a length below 1 counts as 1)
//   snr    = (float)fma(snr_d, r2 2^-32, snr_lo)      as float32 bits; ONE float64 fma (r2 2^-32 is exact) rounded once to float32,
//                                                     snr_d = the float64 difference snr_hi - snr_lo formed by the host
//   0
// One lane stores calls + 1 behind the barrier.
__global__ __launch_bounds__(1024) void k_noise_draw(int* __restrict__ table, int n_items, unsigned n_noise,
                                                     const int* __restrict__ lengths, double snr_lo, double snr_d,
                                                     unsigned long long* state) {
    const unsigned long long seed = state[0], calls = state[1];
    for (int e = threadIdx.x; e < n_items; e += blockDim.x) {
        unsigned c[4] = {(unsigned)e, 0u, (unsigned)calls, (unsigned)(calls >> 32)};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        const unsigned index = __umulhi(c[0], n_noise);
        const unsigned offset = __umulhi(c[1], (unsigned)max(lengths[index], 1));
        const float snr = (float)fma(snr_d, (double)c[2] * 0x1p-32, snr_lo);
        reinterpret_cast<int4*>(table)[e] = make_int4((int)index, (int)offset, __float_as_int(snr), 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) state[1] = calls + 1;
}

// out = masked ? mask_value : x (tf.where, augmentation.py:264): a copy, bit for bit on the elements that pass.  x / out are n_items
// blocks of n_time x n_freq floats (one channel: channels_first and channels_last are the same bytes).  A workgroup owns at most
// kAugChunk consecutive floats of one item; it turns the item's intervals into two LDS bitmaps -- the rows its floats touch, the
// bins of a row -- and then streams: 16-byte accesses on the aligned middle of its range, four loads in flight per lane, scalar
// accesses on the up to 3 + 3 floats around it (VEC = 4; rows of 1025 or 201 bins start on any word).  VEC = 1: unaligned bases.
// out == x is allowed (a lane stores exactly the floats it loaded; hence no __restrict__ on the two).  A form for out == x that
// loads nothing and stores only the masked elements was built and measured (profiles/augment_times.md): 0.5 x the copy on a block
// that stays in the Infinity Cache, 1.1 x on a 654 MB block -- a frequency mask is a few words of every 320-byte row, so DRAM
// rewrites every line anyway -- and was dropped.
template <int VEC>
__global__ __launch_bounds__(256) void k_specaug_apply(const float* x, const int* __restrict__ table, AugGeom a, int chunks,
                                                       float mv, float* out) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    __shared__ unsigned tm[kAugChunk / 32 + 2];             // bit r: row t0 + r is masked
    __shared__ unsigned fm[kAugMaxFreq / 32 + 1];           // bit f: bin f is masked (+ one word: 64-bit windows)
    const int item = blockIdx.x / chunks, chunk = blockIdx.x - item * chunks;
    const unsigned F = a.n_freq, isz = (unsigned)a.n_time * F;
    const unsigned per = (isz + chunks - 1) / chunks;       // <= kAugChunk (host)
    const unsigned lo = min(isz, chunk * per), hi = min(isz, lo + per);
    if (lo >= hi) return;
    const unsigned t0 = lo / F, t1 = (hi - 1) / F;
    const int tw = (int)((t1 - t0) / 32 + 1), fw = (int)((F + 31) / 32 + 1);
    for (int i = threadIdx.x; i < tw; i += blockDim.x) tm[i] = 0u;
    for (int i = threadIdx.x; i < fw; i += blockDim.x) fm[i] = 0u;
    __syncthreads();
    const int* iv = table + (long long)item * (a.n_tm + a.n_fm) * 2;       // wave-uniform: scalar loads
    for (int k = 0; k < a.n_tm; ++k) {
        const int p0 = max(iv[2 * k], (int)t0), p1 = min(iv[2 * k + 1], (int)t1);
        for (int p = p0 + (int)threadIdx.x; p <= p1; p += blockDim.x) atomicOr(&tm[(p - t0) >> 5], 1u << ((p - t0) & 31));
    }
    iv += 2 * a.n_tm;
    for (int k = 0; k < a.n_fm; ++k) {
        const int p0 = max(iv[2 * k], 0), p1 = min(iv[2 * k + 1], (int)F - 1);
        for (int p = p0 + (int)threadIdx.x; p <= p1; p += blockDim.x) atomicOr(&fm[p >> 5], 1u << (p & 31));
    }
    __syncthreads();

    auto masked = [&](unsigned idx) -> bool {               // float idx of the item
        const unsigned t = idx / F, f = idx - t * F, r = t - t0;
        return (((tm[r >> 5] >> (r & 31)) | (fm[f >> 5] >> (f & 31))) & 1u) != 0u;
    };
    auto masked4 = [&](unsigned idx) -> unsigned {          // bit u: float idx + u
        const unsigned t = idx / F, f = idx - t * F, r = t - t0;
        if (f + 3 < F) {                                    // four bins of one row (always, when n_freq % 4 == 0)
            const unsigned row = 0u - ((tm[r >> 5] >> (r & 31)) & 1u);
            const unsigned long long w = ((unsigned long long)fm[(f >> 5) + 1] << 32) | fm[f >> 5];
            return row | (unsigned)(w >> (f & 31));
        }
        unsigned m = 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) m |= (masked(idx + u) ? 1u : 0u) << u;
        return m;
    };

    const long long base = (long long)item * isz;
    const long long g0 = base + lo, g1 = base + hi;
    long long a0, a1;
    db_split<VEC>(g0, g1, a0, a1);
    for (int part = 0; part < 2; ++part) {                  // scalar head [g0, a0) and tail [a1, g1)
        const long long p0 = part ? a1 : g0, p1 = part ? g1 : a0;
        for (long long i = p0 + threadIdx.x; i < p1; i += blockDim.x) {
            const float v = x[i];
            out[i] = masked((unsigned)(i - base)) ? mv : v;
        }
    }
    if (VEC == 4) {
        const vf* xi = reinterpret_cast<const vf*>(x);
        vf* oi = reinterpret_cast<vf*>(out);
        const long long vhi = a1 / VEC;                      // (base need not be a multiple of 4: idx comes from the float index)
        long long i = a0 / VEC + threadIdx.x;
        for (; i + 3 * (long long)blockDim.x < vhi; i += 4 * (long long)blockDim.x) {   // four loads in flight
            vf v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = xi[i + q * (long long)blockDim.x];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned m = masked4((unsigned)((i + q * (long long)blockDim.x) * VEC - base));
#pragma unroll
                for (int u = 0; u < VEC; ++u) v[q][u] = ((m >> u) & 1u) ? mv : v[q][u];
                oi[i + q * (long long)blockDim.x] = v[q];
            }
        }
        for (; i < vhi; i += blockDim.x) {
            vf v = xi[i];
            const unsigned m = masked4((unsigned)(i * VEC - base));
#pragma unroll
            for (int u = 0; u < VEC; ++u) v[u] = ((m >> u) & 1u) ? mv : v[u];
            oi[i] = v;
        }
    }
}

// ChannelSwap: x viewed as (outer, C, inner) 4-byte words (a complex64 element is two), out[o][c][:] = x[o][perm[c]][:].
struct GatherPerm {
    int p[kGatherMaxCh];
};

// Long rows (channels_first spectrograms and waveforms): a workgroup row per (o, c), so the permutation is read with a uniform
// index; V = uint4 when inner % 4 == 0 and both bases are 16-byte aligned (every row then is), four loads in flight per lane.
template <typename V>
__global__ __launch_bounds__(256) void k_channel_gather(const V* __restrict__ x, V* __restrict__ out, long long rows, int C,
                                                        long long inner, GatherPerm perm) {
    for (long long oc = blockIdx.y; oc < rows; oc += gridDim.y) {
        const long long o = oc / C;
        const int c = (int)(oc - o * C);
        const V* src = x + (o * C + perm.p[c]) * inner;
        V* dst = out + oc * inner;
        const long long step = (long long)gridDim.x * blockDim.x;
        long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        for (; i + 3 * step < inner; i += 4 * step) {
            V v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = src[i + q * step];
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[i + q * step] = v[q];
        }
        for (; i < inner; i += step) dst[i] = src[i];
    }
}

// Short rows (channels_last: inner is one element): a lane per o walks its C rows, the permutation again read uniformly.
__global__ __launch_bounds__(256) void k_channel_gather_rows(const unsigned* __restrict__ x, unsigned* __restrict__ out,
                                                             long long outer, int C, int inner, GatherPerm perm) {
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < outer; o += (long long)gridDim.x * blockDim.x) {
        const unsigned* src = x + o * C * inner;
        unsigned* dst = out + o * C * inner;
        for (int c = 0; c < C; ++c) {
            const int pc = perm.p[c];
            for (int w = 0; w < inner; ++w) dst[c * inner + w] = src[pc * inner + w];
        }
    }
}

}  // namespace kpr
