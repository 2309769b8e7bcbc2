// kpr_mdct_kernels.h -- the modified discrete cosine transform of a waveform and its inverse (kapre_amd.MDCT / InverseMDCT,
// backend.mdct / inverse_mdct; tf.signal.mdct / inverse_mdct): k_mdct and k_imdct.  Part of the single translation unit kapre_hip.hip.
//
// Frame length N = 4 NC, M = N / 2 coefficients per frame, hop M.  With the windowed frame cut into quarters a, b, c, d the
// transform is a DCT-IV of the fold u = [-rev(c) - d, a - rev(b)], and that is one NC-point complex FFT between two twiddles:
//   v[n] = (u[2n] + i u[M-1-2n]) pre[n],  V = FFT_NC(v),  Y[k] = V[k] post[k],  X[2k] = Re Y[k],  X[M-1-2k] = -Im Y[k]
// with pre[n] = exp(-i pi (4n+1) / (4M)) and post[k] = scale exp(-i pi k / M), both host tables in float64 (kpr_host_mdct.h).  The
// DCT-IV is its own inverse up to the scale, so the inverse runs the SAME core on v[n] = X[2n] + i X[M-1-2n] and unfolds
// a = u2, b = -rev(u2), c = -rev(u1), d = -u1 (u1, u2 the halves of u) under the window.  In the frame's two halves A (= a, b) and
// B (= c, d) both directions touch the same two positions per FFT point n:
//   n <  NC/2:  p = NC-1-2n, q = NC+2n:    u[2n] = -(wB[p] B[p] + wB[q] B[q]),  u[M-1-2n] = wA[p] A[p] - wA[q] A[q]
//   n >= NC/2:  p = 2n-NC,   q = 3NC-1-2n: u[2n] =   wA[p] A[p] - wA[q] A[q],   u[M-1-2n] = -(wB[p] B[p] + wB[q] B[q])
// and the inverse writes Y's parts to the same p, q with the same signs (it is the transpose).
//
// Work split (as k_stft / k_mel_pw): L = NC / 16 lanes own a frame, 16 complex points each in the layout n = fl + L m, G = 64 / L
// frames per wave step.  A wave owns a run of R consecutive frames (k_mdct) or output blocks of M samples (k_imdct) of one series
// and needs no other wave between its first load and its last store; the only barrier is the one behind the staging of the
// window and the two twiddle tables, which the four waves of a workgroup share.
//   k_mdct   Neighbouring frames share a half.  The run's samples are therefore staged ONCE, block by block (block j = samples
//            j M ... j M + M of the padded series), in a wave-private ring of G + 1 blocks: a step loads G new blocks with
//            16-byte-per-lane loads of consecutive addresses (whole cache lines; the layout's stride and the zeros outside the
//            signal are resolved there) and keeps the last block of the step before.  The fold then reads LDS at p and q.  The
//            coefficients leave through the frame's LDS row in the interleaved order as 16-byte-per-lane stores
//            (channels_first) or as strided words from the registers (channels_last with several channels).
//   k_imdct  Output block j is the second half of frame j-1 plus the first half of frame j.  A run of R blocks transforms R + 1
//            frames: the frame before the run is computed again, that is the seam.  Each frame's halves go to two LDS rows
//            (first halves H1, second halves H2 in two banks that alternate per step, so that the last frame's second half
//            survives into the next step); the wave then adds H1[g] + H2[g-1] and stores the block.  Two terms: the order of
//            the sum cannot matter.  No atomics, every output sample is written once; a frame outside 0 ... T-1 contributes +0.0.
// A frame's arithmetic depends on nothing but its own samples: its bits are independent of its place in a wave, run or launch.
#pragma once

namespace kpr {

constexpr int kMdctWaves = 4;

struct MdctArgs {
    const float* in;
    float* out;
    const float* window;                // N floats
    const float2* fft_tw;               // exp(-2 pi i j / (2 NC)), j < 2 NC (FftTw::load)
    const float2* tab;                  // pre[NC], then post[NC] with the scale folded in
    long long item, chan;               // the waveform's series (kpr_series.h)
    long long c_item, c_chan, c_frame;  // the coefficients: series, and from one frame to the next
    int stride, c_k;                    // from one sample / one coefficient to the next
    int C, len, frames;                 // channels, samples per series (k_imdct: of the output), frames per series
    int R, runs, units;                 // frames (k_imdct: blocks) per run, runs per series, workgroups per series
    int pad;                            // M with pad_begin, else 0
};

__host__ __device__ constexpr size_t mdct_lds_bytes(int NC, bool inverse) {
    const int G = 64 / (NC / kPts), M = 2 * NC;
    return sizeof(float) * ((size_t)8 * NC + (size_t)kMdctWaves * M * (inverse ? 3 * G : 2 * G + 1));
}

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

// samples i ... i + 3 of a series of len samples, zeros outside it
KPR_DEV f4 mdct_load4(const float* __restrict__ in, long long i, int len, int stride) {
    if (stride == 1 && i >= 0 && i + 3 < len) return *reinterpret_cast<const f4u*>(in + i);
    f4 v;
    v.x = (i >= 0 && i < len) ? in[i * stride] : 0.0f;
    v.y = (i + 1 >= 0 && i + 1 < len) ? in[(i + 1) * stride] : 0.0f;
    v.z = (i + 2 >= 0 && i + 2 < len) ? in[(i + 2) * stride] : 0.0f;
    v.w = (i + 3 >= 0 && i + 3 < len) ? in[(i + 3) * stride] : 0.0f;
    return v;
}
KPR_DEV void mdct_store4(float* __restrict__ out, long long i, int len, int stride, f4 v) {
    if (stride == 1 && i >= 0 && i + 3 < len) { *reinterpret_cast<f4u*>(out + i) = v; return; }
    if (i >= 0 && i < len) out[i * stride] = v.x;
    if (i + 1 >= 0 && i + 1 < len) out[(i + 1) * stride] = v.y;
    if (i + 2 >= 0 && i + 2 < len) out[(i + 2) * stride] = v.z;
    if (i + 3 >= 0 && i + 3 < len) out[(i + 3) * stride] = v.w;
}

// what both kernels share: the LDS image of the window and the tables, the FFT twiddles of the lane, the wave's run
template <int NC>
struct MdctWave {
    static constexpr int L = NC / kPts, G = 64 / L, M = 2 * NC;
    typedef typename SwzFor<NC>::type SW;
    float* win;
    f2 *pre, *post;
    float* priv;                        // the wave's private rows
    FftTw<NC, SW> tw;
    int lane, wave, fl, grp;

    // (every lane of the workgroup; ends with the barrier)
    KPR_DEV void setup(float* lds, const MdctArgs& a, int priv_floats) {
        const int tid = threadIdx.x;
        lane = tid & 63; wave = tid >> 6; fl = lane & (L - 1); grp = lane / L;
        win = lds;
        pre = reinterpret_cast<f2*>(lds + 4 * NC);
        post = pre + NC;
        priv = lds + 8 * NC + wave * priv_floats;
        for (int i = tid; i < NC; i += 64 * kMdctWaves)
            *reinterpret_cast<f4*>(win + 4 * i) = *reinterpret_cast<const f4u*>(a.window + 4 * i);
        for (int i = tid; i < 2 * NC; i += 64 * kMdctWaves) {
            const float2 w = a.tab[i];
            pre[i] = f2{w.x, w.y};
        }
        tw.load(a.fft_tw, fl);
        __syncthreads();
    }
    // slot m of this lane: the FFT point n and the two positions it folds
    static KPR_DEV void pq(int fl, int m, int& n, int& p, int& q) {
        n = fl + L * m;
        if (m < kPts / 2) { p = NC - 1 - 2 * n; q = NC + 2 * n; }
        else { p = 2 * n - NC; q = 3 * NC - 1 - 2 * n; }
    }
    // z (layout fl + L m) -> Y = FFT(z pre) post, in place
    KPR_DEV void core(f2 (&z)[kPts], float* row) {
#pragma unroll
        for (int m = 0; m < kPts; ++m) z[m] = cmul(z[m], pre[fl + L * m]);
        tw.refresh();
        cfft_forward<NC, SW>(z, tw, row);
#pragma unroll
        for (int m = 0; m < kPts; ++m) z[m] = cmul(z[m], post[fl + L * m]);
    }
};

template <int NC, bool OUT_CL>
__global__ __launch_bounds__(64 * kMdctWaves) void k_mdct(MdctArgs a) {
    typedef MdctWave<NC> W;
    constexpr int L = W::L, G = W::G, M = W::M, S = G + 1;
    extern __shared__ __attribute__((aligned(16))) float mdct_lds[];
    W w;
    w.setup(mdct_lds, a, (S + G) * M);
    const SeriesUnit u = series_unit(a.units, a.C);
    const int run = u.unit * kMdctWaves + w.wave;
    if (run >= a.runs) return;
    const FrameRun fr_ = frame_run(run, a.R, a.frames);
    const int t0 = fr_.t0, fv = fr_.fv;
    const float* in = u.at(a.in, a.item, a.chan);
    float* out = u.at(a.out, a.c_item, a.c_chan);
    float* span = w.priv;                                   // ring of S blocks: block b of the run in slot b % S
    float* row = span + S * M + w.grp * M;                  // the frame's exchange row, then its coefficients
    const int fl = w.fl, lane = w.lane;
    auto load_block = [&](int b) {
        if (b > fv) return;                                 // (wave-uniform: no frame of the run reads it)
        const long long i0 = (long long)(t0 + b) * M - a.pad;
        float* dst = span + (b % S) * M;
#pragma unroll
        for (int it = 0; it < NC / 128; ++it) {
            const int e = 4 * (lane + 64 * it);
            *reinterpret_cast<f4*>(dst + e) = mdct_load4(in, i0 + e, a.len, a.stride);
        }
    };
#pragma unroll 1
    for (int f0 = 0; f0 < fv; f0 += G) {
        KPR_LDS_FENCE_W();
        if (f0 == 0) load_block(0);
#pragma unroll
        for (int g = 1; g <= G; ++g) load_block(f0 + g);
        KPR_LDS_FENCE_R();
        const int fr = f0 + w.grp;
        const bool valid = fr < fv;
        const float *A = span + (fr % S) * M, *B = span + ((fr + 1) % S) * M;
        const float *wA = w.win, *wB = w.win + M;
        f2 z[kPts];
#pragma unroll
        for (int m = 0; m < kPts; ++m) {
            int n, p, q;
            W::pq(fl, m, n, p, q);
            const float sb = -fmaf(wB[p], B[p], wB[q] * B[q]), sa = fmaf(wA[p], A[p], -(wA[q] * A[q]));
            z[m] = m < kPts / 2 ? f2{sb, sa} : f2{sa, sb};
        }
        w.core(z, row);
        if constexpr (!OUT_CL) {
            KPR_LDS_FENCE_W();
#pragma unroll
            for (int m = 0; m < kPts; ++m) {
                const int k = fl + L * m;
                row[2 * k] = z[m].x;
                row[M - 1 - 2 * k] = -z[m].y;
            }
            KPR_LDS_FENCE_R();
            if (valid) {
                float* o = out + (long long)(t0 + fr) * a.c_frame;
#pragma unroll
                for (int q4 = 0; q4 < kPts / 2; ++q4) {
                    const int i4 = fl + L * q4;
                    *reinterpret_cast<f4u*>(o + 4 * i4) = *reinterpret_cast<const f4*>(row + 4 * i4);
                }
            }
            KPR_LDS_FENCE_X();
        } else if (valid) {
            float* o = out + (long long)(t0 + fr) * a.c_frame;
#pragma unroll
            for (int m = 0; m < kPts; ++m) {
                const int k = fl + L * m;
                o[(long long)(2 * k) * a.c_k] = z[m].x;
                o[(long long)(M - 1 - 2 * k) * a.c_k] = -z[m].y;
            }
        }
    }
}

template <int NC, bool IN_CL>
__global__ __launch_bounds__(64 * kMdctWaves) void k_imdct(MdctArgs a) {
    typedef MdctWave<NC> W;
    constexpr int L = W::L, G = W::G, M = W::M;
    extern __shared__ __attribute__((aligned(16))) float mdct_lds[];
    W w;
    w.setup(mdct_lds, a, 3 * G * M);
    const SeriesUnit u = series_unit(a.units, a.C);
    const int run = u.unit * kMdctWaves + w.wave;
    if (run >= a.runs) return;
    const FrameRun br_ = frame_run(run, a.R, (int)(((long long)a.len + a.pad + M - 1) / M));
    const int j0 = br_.t0, bv = br_.fv;                     // the run's blocks j0 ... j0 + bv - 1, frames j0 - 1 ... j0 + bv - 1
    const float* in = u.at(a.in, a.c_item, a.c_chan);
    float* out = u.at(a.out, a.item, a.chan);
    float* H1 = w.priv;                                     // G rows: the coefficients of a frame, then its first half
    float* H2 = H1 + G * M;                                 // 2 banks of G rows: the exchange row, then the second half
    const int fl = w.fl, lane = w.lane, grp = w.grp;
    int cur = 0;
#pragma unroll 1
    for (int i0 = 0; i0 <= bv; i0 += G, cur ^= 1) {
        float* H2c = H2 + cur * (G * M);
        const float* H2p = H2 + (cur ^ 1) * (G * M);
        const int f = j0 - 1 + i0 + grp;                    // this lane group's frame
        const bool valid = i0 + grp <= bv && f >= 0 && f < a.frames;
        KPR_LDS_FENCE_W();
        if constexpr (!IN_CL) {
#pragma unroll
            for (int it = 0; it < kPts / 2; ++it) {
                const int e4 = lane + 64 * it, g = e4 / (M / 4), off = 4 * (e4 - g * (M / 4));
                const int fg = j0 - 1 + i0 + g;
                f4 v = f4{0.0f, 0.0f, 0.0f, 0.0f};
                if (i0 + g <= bv && fg >= 0 && fg < a.frames) v = *reinterpret_cast<const f4u*>(in + (long long)fg * a.c_frame + off);
                *reinterpret_cast<f4*>(H1 + g * M + off) = v;
            }
        } else {
            const float* c = in + (long long)(valid ? f : 0) * a.c_frame;
#pragma unroll 4
            for (int k = fl; k < M; k += L) H1[grp * M + k] = valid ? c[(long long)k * a.c_k] : 0.0f;
        }
        KPR_LDS_FENCE_R();
        f2 z[kPts];
#pragma unroll
        for (int m = 0; m < kPts; ++m) {
            const int n = fl + L * m;
            z[m] = f2{H1[grp * M + 2 * n], H1[grp * M + M - 1 - 2 * n]};
        }
        w.core(z, H2c + grp * M);
        float o1[kPts][2], o2[kPts][2];
        const float *wA = w.win, *wB = w.win + M;
#pragma unroll
        for (int m = 0; m < kPts; ++m) {
            int n, p, q;
            W::pq(fl, m, n, p, q);
            // what is folded with a minus sign in k_mdct is written with one here
            const float ya = m < kPts / 2 ? -z[m].y : z[m].x, yb = m < kPts / 2 ? -z[m].x : z[m].y;
            o1[m][0] = valid ? ya * wA[p] : 0.0f;
            o1[m][1] = valid ? -ya * wA[q] : 0.0f;
            o2[m][0] = valid ? yb * wB[p] : 0.0f;
            o2[m][1] = valid ? yb * wB[q] : 0.0f;
        }
        KPR_LDS_FENCE_W();
#pragma unroll
        for (int m = 0; m < kPts; ++m) {
            int n, p, q;
            W::pq(fl, m, n, p, q);
            H1[grp * M + p] = o1[m][0];
            H1[grp * M + q] = o1[m][1];
            H2c[grp * M + p] = o2[m][0];
            H2c[grp * M + q] = o2[m][1];
        }
        KPR_LDS_FENCE_R();
#pragma unroll
        for (int it = 0; it < kPts / 2; ++it) {
            const int e4 = lane + 64 * it, g = e4 / (M / 4), off = 4 * (e4 - g * (M / 4));
            const int br = i0 + g - 1;                      // the block that frame g's first half ends in
            const f4 first = *reinterpret_cast<const f4*>(H1 + g * M + off);
            const f4 second = *reinterpret_cast<const f4*>((g > 0 ? H2c + (g - 1) * M : H2p + (G - 1) * M) + off);
            if (br >= 0 && br < bv) mdct_store4(out, (long long)(j0 + br) * M - a.pad + off, a.len, a.stride, first + second);
        }
        KPR_LDS_FENCE_X();
    }
}

}  // namespace kpr
