// kpr_hpss_kernels.h -- median-filter harmonic-percussive separation of a spectrogram (kapre_amd.HPSS): the one kernel family of the
// library that is a rank filter over a 2-D neighbourhood.  Part of the single translation unit kapre_hip.hip.
//
//   H[t, f] = median of S[r(t + d, T), f], |d| <= hh      P[t, f] = median of S[t, r(f + d, F)], |d| <= hp
//   r(i, n): j = i mod 2n (non-negative); j < n ? j : 2n - 1 - j                                  (half-sample symmetric)
//   soft(X, R): Z = max(X, R); bad = Z < 2^-126; a = X / Z, c = R / Z (Z := 1 where bad); m = a^p / (a^p + c^p); bad: m = bad_value
//               p = inf: m = X > R
//   Mh = soft(H, P mh),  Mp = soft(P, H mp);  harmonic = S Mh,  percussive = S Mp;  S = |D| for a complex input, which the masks
//   then multiply
//
// One launch reads S once and writes both outputs.  A workgroup of four waves owns a 64 x 64 (time x frequency) tile of one plane:
//   1. it stages the tile with its cross-shaped halo -- hh rows above and below, hp columns left and right, r() applied -- in LDS as
//      ORDER KEYS: the float's bits with the usual sign flip, every NaN mapped to the top key.  Unsigned order of the keys is the
//      order of numpy.sort (NaN last), exact for denormals whatever the float mode, and the median becomes min / max / med3 on
//      integers.  Rows are 2 HALO + 65 words apart, an odd number: the reads of step 2, whose lanes differ in t, hit 64 banks.
//   2. frequency walk: lane = row t, wave = a run of 16 consecutive columns.  P goes to a second LDS tile.  Barrier.
//   3. time walk: lane = column f, wave = a run of 16 consecutive rows.  H stays in the lane, P comes from LDS, S from the key (or D
//      from memory), and the lane writes its outputs -- consecutive lanes, consecutive f.
// A run keeps the SORTED WINDOW in 2 HALO + 1 registers: the first window is sorted by Batcher's merge exchange network (191
// comparators for 32 inputs), every further output REPLACES the window's oldest element by its newest in one branch-free pass:
//     m[i] = med3(w[i], w[i + 1], n)   (w[-1] = 0, w[K] = top)        w'[i] = w[i] > thr ? m[i] : m[i - 1]
//     thr = n >= o ? o - 1 : o         (o: the key that leaves, n: the key that enters)
// that is three operations per slot.  Removing "one copy of o" is well defined on a multiset, so ties need no care: slots below
// the first copy of o (n >= o) or above the last one (n < o) keep their value -- med3 returns w[i] there --, the slots between the
// gap and n's place shift by one, and n lands where med3 picks it.  A window shorter than 2 HALO + 1 is padded with
// equal numbers of 0 and top keys, which are never removed (no real key is 0; a NaN that leaves removes one top key, and any one
// will do), so the median stays in the middle slot.  Every register index is a compile-time constant.
#pragma once

#include <utility>

namespace kpr {

constexpr int kHpTile = 64;        // frames and bins of a tile
constexpr int kHpRun = 16;         // consecutive outputs of a lane per walk
constexpr int kHpWaves = kHpTile / kHpRun;

struct HpssArgs {
    const void* x;
    void* out_h;                   // either may be NULL
    void* out_p;
    int frames, freq, ch;
    int hh, hp;                    // (kh - 1) / 2, (kp - 1) / 2
    int tiles_t, tiles_f;
    long long x_b, x_c, x_t, x_f;  // element strides of x: batch item, channel, frame, bin
    long long o_b, o_c, o_t, o_f;  // and of the outputs
    int mode;                      // 0: S M (D M), 1: the masks, 2: the medians H and P themselves
    int pmode;                     // 1: power 1, 2: power 2, 3: power inf, 0: powf
    float power, mh, mp, bad_value;
};

KPR_DEV unsigned hp_key(float v) {
    const unsigned b = __float_as_uint(v);
    const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return (b & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : k;
}
KPR_DEV float hp_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// |z| as Magnitude (k_cplx_to_real) forms it: the square of the imaginary part rounded, then one fused multiply-add under the
// root (tests/test_hpss_gpu.py::test_complex_input compares the medians of D with those of Magnitude()(D) bit for bit)
KPR_DEV float hp_abs(float2 z) { return sqrtf(fmaf(z.x, z.x, z.y * z.y)); }

KPR_DEV int hp_reflect(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int m = 2 * n;
    int j = i % m;
    j = j < 0 ? j + m : j;
    return j < n ? j : m - 1 - j;
}

// Batcher's merge exchange (Knuth 5.2.2 M) for N inputs as a list of comparators, made at compile time
template <int N>
struct HpNet {
    int a[N * 8], b[N * 8], n;
};
template <int N>
constexpr HpNet<N> hp_make_net() {
    HpNet<N> r{};
    int c = 0;
    for (int p = 1; p < N; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        r.a[c] = i + j;
                        r.b[c] = i + j + k;
                        ++c;
                    }
    r.n = c;
    return r;
}
template <int N>
inline constexpr HpNet<N> kHpNet = hp_make_net<N>();

template <int A, int B, int N>
KPR_DEV void hp_cswap(unsigned (&w)[N]) {
    const unsigned lo = min(w[A], w[B]), hi = max(w[A], w[B]);
    w[A] = lo;
    w[B] = hi;
}
template <int N, size_t... I>
KPR_DEV void hp_sort_impl(unsigned (&w)[N], std::index_sequence<I...>) {
    (hp_cswap<kHpNet<N>.a[I], kHpNet<N>.b[I]>(w), ...);
}
template <int N>
KPR_DEV void hp_sort(unsigned (&w)[N]) {
    hp_sort_impl<N>(w, std::make_index_sequence<kHpNet<N>.n>{});
}

KPR_DEV unsigned hp_med3(unsigned a, unsigned b, unsigned c) { return min(max(a, b), max(min(a, b), c)); }

// the sorted window w[0 .. K) (w[K] = top key) with one copy of o taken out and n put in
template <int K>
KPR_DEV void hp_replace(unsigned (&w)[K + 1], unsigned o, unsigned n) {
    const unsigned thr = n >= o ? o - 1u : o;
    unsigned below = min(w[0], n);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const unsigned m = hp_med3(w[i], w[i + 1], n);
        const unsigned nw = w[i] > thr ? m : below;
        below = m;
        w[i] = nw;
    }
}

// kHpRun medians of a lane: positions s .. s + kHpRun - 1 of a line of keys whose element p lies at base[(p + HALO) * stride]
template <int HALO, class Emit>
KPR_DEV void hp_walk(const unsigned* base, int stride, int s, int h, Emit&& emit) {
    constexpr int K = 2 * HALO + 1;
    unsigned w[K + 1];
#pragma unroll
    for (int d = 0; d < K; ++d) {
        const unsigned v = base[(s + d) * stride];
        const bool in = (d < HALO ? HALO - d : d - HALO) <= h;
        w[d] = in ? v : (d < HALO ? 0u : 0xffffffffu);
    }
    w[K] = 0xffffffffu;
    hp_sort<K + 1>(w);
    emit(0, w[HALO]);
#pragma unroll 1
    for (int r = 1; r < kHpRun; ++r) {
        const unsigned o = base[(s + r - 1 + HALO - h) * stride];
        const unsigned n = base[(s + r + HALO + h) * stride];
        hp_replace<K>(w, o, n);
        emit(r, w[HALO]);
    }
}

// librosa's softmask in float32, as written at the head of this file.  Z = max(X, R) IS X or R, so of X / Z and R / Z one is x / x
// -- 1 for every finite x that is not 0, NaN for Inf and NaN -- and only the other one is divided: the bits of two divisions for one.
KPR_DEV void hp_ratios(float X, float R, float& p, float& q, bool& bad) {
    float Z = fmaxf(X, R);
    bad = Z < 1.17549435e-38f;
    Z = bad ? 1.0f : Z;                                                  // (what follows is then overwritten by bad_value)
    const float one = Z < INFINITY ? 1.0f : __builtin_nanf("");
    const bool xz = X == Z, rz = R == Z;
    const float quo = (xz ? R : X) / Z;
    p = xz ? one : quo;
    q = rz ? one : quo;
}
KPR_DEV void hp_powers(float& p, float& q, const HpssArgs& a) {
#pragma clang fp contract(off)
    if (a.pmode == 1) return;
    if (a.pmode == 2) {
        p = p * p;
        q = q * q;
    } else {
        p = powf(p, a.power);
        q = powf(q, a.power);
    }
}
struct HpMasks {
    float h, p;
};
// Mh = soft(H, P mh) and Mp = soft(P, H mp).  With both margins 1 the two share Z, the ratios (swapped) and -- float addition
// commutes -- the denominator: three divisions per bin instead of four, again with the same bits.
KPR_DEV HpMasks hp_masks(float H, float P, const HpssArgs& a) {
#pragma clang fp contract(off)
    const float Rh = P * a.mh, Rp = H * a.mp;
    HpMasks m = {0.0f, 0.0f};
    if (a.pmode == 3) {
        m.h = H > Rh ? 1.0f : 0.0f;
        m.p = P > Rp ? 1.0f : 0.0f;
        return m;
    }
    float p, q;
    bool bad;
    if (a.mh == 1.0f && a.mp == 1.0f) {
        hp_ratios(H, P, p, q, bad);
        hp_powers(p, q, a);
        const float d = p + q;
        m.h = bad ? a.bad_value : p / d;
        m.p = bad ? a.bad_value : q / d;
        return m;
    }
    if (a.out_h) {
        hp_ratios(H, Rh, p, q, bad);
        hp_powers(p, q, a);
        m.h = bad ? a.bad_value : p / (p + q);
    }
    if (a.out_p) {
        hp_ratios(P, Rp, p, q, bad);
        hp_powers(p, q, a);
        m.p = bad ? a.bad_value : p / (p + q);
    }
    return m;
}

template <int HALO, bool CPLX>
__global__ __launch_bounds__(64 * kHpWaves) void k_hpss(HpssArgs a) {
    constexpr int TILE = kHpTile, W = TILE + 2 * HALO + 1;
    __shared__ unsigned keys[TILE + 2 * HALO][W];
    __shared__ float Ps[TILE][TILE + 1];

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned per_plane = (unsigned)a.tiles_t * (unsigned)a.tiles_f;
    const unsigned plane = blockIdx.x / per_plane, rem = blockIdx.x % per_plane;
    const int t0 = (int)(rem / (unsigned)a.tiles_f) * TILE, f0 = (int)(rem % (unsigned)a.tiles_f) * TILE;
    const long long b = plane / (unsigned)a.ch, c = plane % (unsigned)a.ch;
    const long long xbase = b * a.x_b + c * a.x_c, obase = b * a.o_b + c * a.o_c;
    const int T = a.frames, F = a.freq, hh = a.hh, hp = a.hp;

    // 1. the tile and its cross-shaped halo, as keys (the four corners are never read)
    {
        const int rows = TILE + 2 * hh, cols = TILE + 2 * hp;
        long long fo[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) fo[u] = (long long)hp_reflect(f0 + lane + 64 * u - hp, F) * a.x_f;
        for (int i = wave; i < rows; i += kHpWaves) {
            const long long row = xbase + (long long)hp_reflect(t0 + i - hh, T) * a.x_t;
            const bool core_row = i >= hh && i < hh + TILE;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = lane + 64 * u;
                const bool core_col = j >= hp && j < hp + TILE;
                if (j < cols && (core_row || core_col)) {
                    float s;
                    if constexpr (CPLX) {
                        const float2 z = ((const float2*)a.x)[row + fo[u]];
                        s = hp_abs(z);
                    } else {
                        s = ((const float*)a.x)[row + fo[u]];
                    }
                    keys[HALO - hh + i][HALO - hp + j] = hp_key(s);
                }
            }
        }
    }
    __syncthreads();

    // 2. frequency walk: this lane's row, the wave's 16 columns (a run wholly past the last bin is skipped)
    const int s = wave * kHpRun;
    if (f0 + s < F)
        hp_walk<HALO>(&keys[HALO + lane][0], 1, s, hp, [&](int r, unsigned k) { Ps[lane][s + r] = hp_val(k); });
    __syncthreads();

    // 3. time walk: this lane's column, the wave's 16 rows; masks and stores
    if (t0 + s < T) {
        const int f = f0 + lane;
        const bool col_ok = f < F;
        hp_walk<HALO>(&keys[0][HALO + lane], W, s, hh, [&](int r, unsigned k) {
#pragma clang fp contract(off)
            const int t = t0 + s + r;
            if (!(col_ok && t < T)) return;
            const float H = hp_val(k), P = Ps[s + r][lane];
            const long long oo = obase + t * a.o_t + f * a.o_f;
            if (a.mode == 2) {
                if (a.out_h) ((float*)a.out_h)[oo] = H;
                if (a.out_p) ((float*)a.out_p)[oo] = P;
                return;
            }
            const HpMasks mk = hp_masks(H, P, a);
            const float Mh = mk.h, Mp = mk.p;
            if (a.mode == 1) {
                if (a.out_h) ((float*)a.out_h)[oo] = Mh;
                if (a.out_p) ((float*)a.out_p)[oo] = Mp;
                return;
            }
            if constexpr (CPLX) {
                const float2 z = ((const float2*)a.x)[xbase + t * a.x_t + f * a.x_f];
                if (a.out_h) ((float2*)a.out_h)[oo] = make_float2(z.x * Mh, z.y * Mh);
                if (a.out_p) ((float2*)a.out_p)[oo] = make_float2(z.x * Mp, z.y * Mp);
            } else {
                const float S = hp_val(keys[HALO + s + r][HALO + lane]);
                if (a.out_h) ((float*)a.out_h)[oo] = S * Mh;
                if (a.out_p) ((float*)a.out_p)[oo] = S * Mp;
            }
        });
    }
}

}  // namespace kpr
