// kpr_misc_kernels.h -- Magnitude / Phase, MagnitudeToDecibel (log + clamp passes), generic fp32-MFMA GEMM k_gemm.
// Part of the single translation unit kapre_hip.hip (included there, in this order; not stand-alone).
#pragma once

namespace kpr {

// ------------------------------------------------------------------------------------------
// elementwise complex -> real
// ------------------------------------------------------------------------------------------
// |v| = sqrt(fma(re, re, fl(im * im))): ONE fused multiply-add under the root, written out so that the optimiser's contraction
// does not decide the last bit (and cannot decide it differently in an unrolled body and its remainder).  hp_abs (HPSS) and
// pv_abs (TimeStretch) form the same expression: their magnitudes equal Magnitude()'s bit for bit.  The squares overflow from
// components of about 1.8e19 (+Inf) and underflow under about 1e-19 (INTEGRATION.md "Non-finite values").
__global__ void k_cplx_to_real(const float2* __restrict__ x, long long n, int phase,
                               float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        float2 v = x[i];
        out[i] = phase ? atan2f(v.y, v.x) : sqrtf(fmaf(v.x, v.x, v.y * v.y));
    }
}

// ------------------------------------------------------------------------------------------
// decibel
// ------------------------------------------------------------------------------------------
__global__ void k_stats_init(unsigned* stats, long long n_items) {
    // grid-stride: launches cap the grid (grid_1d), items do not have a cap
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_items;
         i += (long long)gridDim.x * blockDim.x) {
        stats[2 * i] = 0u;
        stats[2 * i + 1] = 0xffffffffu;
    }
}

// log pass: out = 10 log10(max(x, amin)) - ref_term, per-item max/min into stats.
// VEC = 4: 16-byte loads / stores (item_size % 4 == 0 and 16-byte aligned bases; chunk bounds are
// then multiples of 4 as well)
// A block owns the floats [g0, g1) of the flat array (one chunk of one item).  VEC = 4: 16-byte
// loads / stores on the 16-byte aligned middle of the range, scalar accesses on the (at most 3 + 3)
// floats before and after it -- item sizes are usually odd (K = n_fft/2 + 1 bins per frame), so
// neither the items nor the chunks start on 16-byte boundaries.  Needs 16-byte aligned base pointers.
template <int VEC>
KPR_DEV void db_split(long long g0, long long g1, long long& a0, long long& a1) {
    if (VEC == 1) { a0 = g1; a1 = g1; return; }
    a0 = min(g1, (g0 + VEC - 1) / VEC * VEC);
    a1 = max(a0, g1 / VEC * VEC);
}

// log pass: out = 10 log10(max(x, amin)) - ref_term, per-item max/min into stats.
template <int VEC>
__global__ __launch_bounds__(256) void k_db_log(const float* __restrict__ x, long long item_size, int chunks, DbDev db,
                         unsigned* __restrict__ stats, float* __restrict__ out) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    const long long item = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const long long per = (item_size + chunks - 1) / chunks;
    const long long lo = min(item_size, chunk * per), hi = min(item_size, lo + per);
    const long long g0 = item * item_size + lo, g1 = item * item_size + hi;
    long long a0, a1;
    db_split<VEC>(g0, g1, a0, a1);
    float mx = -INFINITY, mn = INFINITY;
    // scalar head [g0, a0) and tail [a1, g1)
    for (int part = 0; part < 2; ++part) {
        const long long p0 = part ? a1 : g0, p1 = part ? g1 : a0;
        for (long long i = p0 + threadIdx.x; i < p1; i += blockDim.x) {
            const float d = to_db(x[i], db);
            out[i] = d;
            mx = fmaxf(mx, d);
            mn = fminf(mn, d);
        }
    }
    const vf* xi = reinterpret_cast<const vf*>(x);
    vf* oi = reinterpret_cast<vf*>(out);
    const long long vhi = a1 / VEC;
    long long i = a0 / VEC + threadIdx.x;
    for (; i + 3 * (long long)blockDim.x < vhi; i += 4 * (long long)blockDim.x) {   // four loads in flight
        vf v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = xi[i + q * (long long)blockDim.x];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int u = 0; u < VEC; ++u) {
                const float d = to_db(v[q][u], db);
                v[q][u] = d;
                mx = fmaxf(mx, d);
                mn = fminf(mn, d);
            }
            oi[i + q * (long long)blockDim.x] = v[q];
        }
    }
    for (; i < vhi; i += blockDim.x) {
        vf v = xi[i];
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
            const float d = to_db(v[u], db);
            v[u] = d;
            mx = fmaxf(mx, d);
            mn = fminf(mn, d);
        }
        oi[i] = v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        mn = fminf(mn, __shfl_xor(mn, o, 64));
    }
    // ONE pair of atomics per block: the statistics of 16 neighbouring items share a cache line, and
    // same-line atomics serialise in L2 (~25 ns each) -- with a pair per wave and 20 chunks per item
    // this kernel spent half of its time queueing there
    __shared__ float red[2][4];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wv] = mx; red[1][wv] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
        mn = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
        if (mx >= mn) {
            atomicMax(&stats[2 * item], enc_f(mx));
            atomicMin(&stats[2 * item + 1], enc_f(mn));
        }
    }
}
// slots: statistics slots per item (DbDev::slot_mask + 1; slot s of item b at stats[s * slot_stride + 2 b]), reduced here
template <int VEC>
__global__ __launch_bounds__(256) void k_db_clamp(float* __restrict__ out, long long item_size, int chunks, float dyn,
                           const unsigned* __restrict__ stats, int slots, int slot_stride) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    const long long item = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    unsigned umax, umin;
    if (slots == 1) {
        umax = stats[2 * item];
        umin = stats[2 * item + 1];
    } else {
        // lane s of the first wave fetches slot s (slots <= 32): one memory round trip, not one per slot
        __shared__ unsigned red[2];
        if (threadIdx.x < 64) {
            const bool have = (int)threadIdx.x < slots;
            umax = have ? stats[(long long)threadIdx.x * slot_stride + 2 * item] : 0u;
            umin = have ? stats[(long long)threadIdx.x * slot_stride + 2 * item + 1] : 0xffffffffu;
            for (int o = 32; o > 0; o >>= 1) {
                umax = max(umax, (unsigned)__shfl_xor((int)umax, o, 64));
                umin = min(umin, (unsigned)__shfl_xor((int)umin, o, 64));
            }
            if (threadIdx.x == 0) { red[0] = umax; red[1] = umin; }
        }
        __syncthreads();
        umax = red[0];
        umin = red[1];
    }
    const float thr = dec_f(umax) - dyn;
    if (dec_f(umin) >= thr) return;
    const long long per = (item_size + chunks - 1) / chunks;
    const long long lo = min(item_size, chunk * per), hi = min(item_size, lo + per);
    const long long g0 = item * item_size + lo, g1 = item * item_size + hi;
    long long a0, a1;
    db_split<VEC>(g0, g1, a0, a1);
    for (long long i = g0 + threadIdx.x; i < a0; i += blockDim.x) out[i] = fmaxf(out[i], thr);
    for (long long i = a1 + threadIdx.x; i < g1; i += blockDim.x) out[i] = fmaxf(out[i], thr);
    vf* oi = reinterpret_cast<vf*>(out);
    for (long long i = a0 / VEC + threadIdx.x; i < a1 / VEC; i += blockDim.x) {
        vf v = oi[i];
#pragma unroll
        for (int u = 0; u < VEC; ++u) v[u] = fmaxf(v[u], thr);
        oi[i] = v;
    }
}

// ------------------------------------------------------------------------------------------
// Banded filterbank product for long rows (K = 2049 / 4097 bins, n_fft 4096 / 8192: beyond the 1025-
// column tile of the MFMA consumers): out[frame][m] = sum_{k in band(m)} mag[frame][k] * fb[k][m].
// A mel / log bank has ~2 K non-zeros in total, so this is a bandwidth kernel: four magnitude rows in
// LDS per step, a wave per 16-filter tile with its band (klo / khi from kpr_filterbank_kranges) cut into
// four interleaved slices across the lanes (fb reads are 64-byte segments, LDS reads four-address multicasts).
// Optional decibel epilogue with per-item max / min (clamp pass afterwards), as the fused kernels.
// ------------------------------------------------------------------------------------------
constexpr int kBandRows = 4;

__global__ __launch_bounds__(256) void k_band_mel(const float* __restrict__ mag, Geom g,
                                                  const float* __restrict__ fb, MelSched sch, DbDev db,
                                                  unsigned* __restrict__ item_stats, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K = g.K, M = sch.M;
    const int ostride = spec_stride(g);
    const long long nsteps = (g.total_frames + kBandRows - 1) / kBandRows;
    for (long long step = blockIdx.x; step < nsteps; step += gridDim.x) {
        const long long f0 = step * kBandRows;
        const int nr = (int)min((long long)kBandRows, g.total_frames - f0);
        __syncthreads();                                           // rows of the previous step are no longer read
        for (int i = threadIdx.x; i < nr * K; i += blockDim.x) smem[i] = mag[f0 * K + i];   // contiguous rows
        __syncthreads();
        // decibel statistics: one pair of atomics per step when its rows belong to one batch item (the
        // usual case), per element only on the steps that straddle two items
        const FramePos p_first = frame_pos(g, f0), p_last = frame_pos(g, f0 + nr - 1);
        const bool one_item = p_first.b == p_last.b;
        float wmax = -INFINITY, wmin = INFINITY;
        // a wave per 16-filter tile: lane = (filter in tile, k slice); the four slices take every fourth bin of
        // the tile's band (four loads in flight each) and are summed by two shuffles, then slice r writes
        // row r.  Tiles are dealt narrow / wide alternately (bands grow with the filter index).
        const int lane = threadIdx.x & 63, ml = lane & 15, sl = lane >> 4;
        for (int i = threadIdx.x >> 6; i < sch.ntiles; i += (int)(blockDim.x >> 6)) {
            const int t = (i & 1) ? sch.ntiles - 1 - (i >> 1) : (i >> 1);
            const int m = 16 * t + ml, mc = min(m, M - 1);
            const int klo = sch.klo[t], khi = min((int)sch.khi[t], K);
            float acc[kBandRows] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k0 = klo + sl; k0 < khi; k0 += 16) {
                float w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = fb[(long long)min(k0 + 4 * u, khi - 1) * M + mc];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = min(k0 + 4 * u, khi - 1);
                    const float wu = (k0 + 4 * u < khi) ? w[u] : 0.0f;
#pragma unroll
                    for (int r = 0; r < kBandRows; ++r) acc[r] += smem[r * K + k] * wu;
                }
            }
#pragma unroll
            for (int r = 0; r < kBandRows; ++r) {
                acc[r] += __shfl_xor(acc[r], 16, 64);
                acc[r] += __shfl_xor(acc[r], 32, 64);
            }
            const int r = sl;                                    // slice r stores row r
            if (r < nr && m < M) {
                const long long gf = f0 + r;
                FramePos p = frame_pos(g, gf);
                float v = acc[0];
#pragma unroll
                for (int q = 1; q < kBandRows; ++q) v = (r == q) ? acc[q] : v;
                if (db.enabled) {
                    v = to_db(v, db);
                    if (one_item) { wmax = fmaxf(wmax, v); wmin = fminf(wmin, v); }
                    else {
                        atomicMax(&item_stats[2 * p.b], enc_f(v));
                        atomicMin(&item_stats[2 * p.b + 1], enc_f(v));
                    }
                }
                out[spec_base(g, p, gf, M) + (long long)m * ostride] = v;
            }
        }
        if (db.enabled && one_item) {
            for (int o = 32; o > 0; o >>= 1) {
                wmax = fmaxf(wmax, __shfl_xor(wmax, o, 64));
                wmin = fminf(wmin, __shfl_xor(wmin, o, 64));
            }
            if ((threadIdx.x & 63) == 0 && wmax >= wmin) {
                atomicMax(&item_stats[2 * p_first.b], enc_f(wmax));
                atomicMin(&item_stats[2 * p_first.b + 1], enc_f(wmin));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// generic fp32-MFMA GEMM:  C[r][n] = sum_k A(r,k) * Bm[k][n]
// rows r are decomposed as r = (r2*D1 + r1)*D0 + r0 for input and output addressing
// ------------------------------------------------------------------------------------------
enum { A_PLAIN = 0, A_CABS = 1, A_FRAME = 2, A_CPLX = 3 };
enum { E_PLAIN = 0, E_CPLX = 1, E_WINDOW = 2, E_DB = 3 };

struct RowMap {
    long long rows;
    int D0, D1;
    long long s2, s1, s0;   // base = r2*s2 + r1*s1 + r0*s0
    long long es;           // element stride along k (input) / n (output)
    KPR_DEV long long base(long long r, long long* r2_out = nullptr) const {
        long long r0 = r % D0, q = r / D0;
        long long r1 = q % D1, r2 = q / D1;
        if (r2_out) *r2_out = r2;
        return r2 * s2 + r1 * s1 + r0 * s0;
    }
};

struct GemmArgs {
    RowMap in, out;
    int Kdim, N;            // reduction length, output columns
    int ldb;                // row stride of Bm
    // A_FRAME: time geometry
    long long T; int hop, pad_left; long long t_es;
    const float* window;    // A_FRAME analysis window / E_WINDOW synthesis window
    int win;
    DbDev db;
    unsigned* stats;
    int has_kr;             // per 64-column block k range
    short klo[kMaxTiles], khi[kMaxTiles];   // per 16-col tile (multiples of 4)
};

// Row part of the A accessor, computed ONCE per thread (its row is fixed): the row decomposition costs
// two 64-bit divisions and two modulos -- per element, as in the first version, they dominated the kernel.
struct GemmRow {
    bool ok;
    long long base;     // A_PLAIN / A_CABS / A_CPLX: element offset of the row;  A_FRAME: offset of the signal
    long long t0;       // A_FRAME: first sample of the frame (may be negative: left padding)
};
template <int AMODE>
KPR_DEV GemmRow gemm_row(const GemmArgs& ga, long long r) {
    GemmRow g;
    g.ok = r < ga.in.rows;
    const long long rc = g.ok ? r : 0;
    if constexpr (AMODE == A_FRAME) {
        const long long r0 = rc % ga.in.D0, q = rc / ga.in.D0;
        const long long r1 = q % ga.in.D1, r2 = q / ga.in.D1;
        g.base = r2 * ga.in.s2 + r1 * ga.in.s1;
        g.t0 = r0 * ga.hop - ga.pad_left;
    } else {
        g.base = ga.in.base(rc);
        g.t0 = 0;
    }
    return g;
}
// unconditional load from a clamped position, then select (a load under a condition is waited for on the spot)
template <int AMODE>
KPR_DEV float gemm_load_a(const float* __restrict__ a, const GemmArgs& ga, const GemmRow& g, int k) {
    const bool kin = g.ok && k < ga.Kdim;
    const int kc = min(k, ga.Kdim - 1);
    if constexpr (AMODE == A_PLAIN) {
        const float v = a[g.base + (long long)kc * ga.in.es];
        return kin ? v : 0.0f;
    } else if constexpr (AMODE == A_CABS) {
        const float2 v = reinterpret_cast<const float2*>(a)[g.base + (long long)kc * ga.in.es];
        return kin ? sqrtf(v.x * v.x + v.y * v.y) : 0.0f;
    } else if constexpr (AMODE == A_CPLX) {
        // k indexes interleaved (re, im): complex element k>>1, part k&1
        const float v = a[2 * (g.base + (long long)(kc >> 1) * ga.in.es) + (kc & 1)];
        return kin ? v : 0.0f;
    } else {  // A_FRAME: rows are frames
        const long long t = g.t0 + kc, tc = min(max(t, 0LL), ga.T - 1);
        const float v = a[g.base + tc * ga.t_es] * ga.window[kc];
        return (kin && t >= 0 && t < ga.T) ? v : 0.0f;
    }
}

template <int AMODE, int EPI>
__global__ __launch_bounds__(256) void k_gemm(const float* __restrict__ a,
                                              const float* __restrict__ bm, GemmArgs ga,
                                              float* __restrict__ out) {
    constexpr int TM = 64, TN = 64, KC = 16, LDX = 18, LDB = 80;
    __shared__ float Xs[TM * LDX];
    __shared__ float Bs[KC * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * TM;
    const int col0 = blockIdx.y * TN;
    int klo = 0, khi = (ga.Kdim + 3) & ~3;
    if (ga.has_kr) {
        klo = 1 << 30; khi = 0;
        for (int t = col0 / 16; t < (col0 + TN) / 16 && t * 16 < ga.N; ++t) {
            klo = min(klo, (int)ga.klo[t]); khi = max(khi, (int)ga.khi[t]);
        }
        if (klo > khi) klo = khi;
    }
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int jcol = lane & 15, kq = lane >> 4;
    const GemmRow grow = gemm_row<AMODE>(ga, row0 + (tid >> 2));        // this thread's row of the X tile
    for (int kc = klo; kc < khi; kc += KC) {
        {   // stage X tile: thread -> (row = tid>>2, 4 consecutive k)
            const int r = tid >> 2, kk = (tid & 3) * 4;
            float xv[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = gemm_load_a<AMODE>(a, ga, grow, kc + kk + i);
            // stage B tile: thread -> (k = tid>>4, 4 consecutive n); clamped loads, then select
            const int kb = tid >> 4, nn = (tid & 15) * 4;
            const int kg = kc + kb, kgc = min(kg, ga.Kdim - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ng = col0 + nn + i;
                const float v = bm[(long long)kgc * ga.ldb + min(ng, ga.N - 1)];
                bv[i] = (kg < ga.Kdim && ng < ga.N) ? v : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) { Xs[r * LDX + kk + i] = xv[i]; Bs[kb * LDB + nn + i] = bv[i]; }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KC; ks += 4) {
            const float bfrag = Xs[(wave * 16 + jcol) * LDX + ks + kq];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float afrag = Bs[(ks + kq) * LDB + nt * 16 + jcol];
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag, bfrag, acc[nt], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // lane holds C[row = row0 + wave*16 + jcol][col = col0 + nt*16 + 4*kq + r]
    const long long r = row0 + wave * 16 + jcol;
    if (r >= ga.out.rows) return;
    long long r2 = 0;
    const long long ob = ga.out.base(r, &r2);
    float mx = -INFINITY, mn = INFINITY;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = col0 + nt * 16 + 4 * kq + i;
            if (n >= ga.N) continue;
            float v = acc[nt][i];
            if constexpr (EPI == E_PLAIN) {
                out[ob + (long long)n * ga.out.es] = v;
            } else if constexpr (EPI == E_CPLX) {
                out[2 * (ob + (long long)(n >> 1) * ga.out.es) + (n & 1)] = v;
            } else if constexpr (EPI == E_WINDOW) {
                out[ob + (long long)n * ga.out.es] = (n < ga.win) ? v * ga.window[n] : 0.0f;
            } else {
                v = to_db(v, ga.db);
                mx = fmaxf(mx, v); mn = fminf(mn, v);
                out[ob + (long long)n * ga.out.es] = v;
            }
        }
    }
    if constexpr (EPI == E_DB) {
        if (mx >= mn) {
            atomicMax(&ga.stats[2 * r2], enc_f(mx));
            atomicMin(&ga.stats[2 * r2 + 1], enc_f(mn));
        }
    }
}

// development aid for PMC calibration: stream-read n float2 (8 B per lane, the access width of the
// development aid (kpr_debug_sclk_mhz): the shader clock UNDER A DENSE VECTOR LOAD -- what the FFT kernels actually run at.
// Every wave runs `iters` blocks of 64 independent packed FMAs and records s_memtime ticks per 100 MHz s_memrealtime tick.
__global__ __launch_bounds__(256) void k_sclk(int iters, float* __restrict__ out_mhz) {
    f2 a[8], b = f2{1.0000001f, 0.9999999f};
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = f2{1.0f + threadIdx.x * 1e-3f + i, 0.5f};
    const unsigned long long t0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int i = 0; i < 8; ++i) asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(a[i]) : "v"(b));
    }
    const unsigned long long t1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += a[i].x + a[i].y;
    if ((threadIdx.x & 63) == 0) {
        const float mhz = (r1 > r0) ? 100.0f * (float)(t1 - t0) / (float)(r1 - r0) : 0.0f;
        out_mhz[blockIdx.x * 4 + (threadIdx.x >> 6)] = (s == 1.2345e-30f) ? 0.0f : mhz;
    }
}

// frame loads) and write one float per workgroup
__global__ void k_calib_read8(const float2* __restrict__ x, long long n, float* __restrict__ out) {
    float acc = 0.0f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        float2 v = x[i];
        acc += v.x + v.y;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

// zero-fill columns [n0, n1) of every output row (E_WINDOW with win_length > n_fft)
__global__ void k_fill_cols(float* out, long long rows, long long ld, int n0, int n1) {
    const long long total = rows * (n1 - n0);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x)
        out[(i / (n1 - n0)) * ld + n0 + (i % (n1 - n0))] = 0.0f;
}

}  // namespace kpr
