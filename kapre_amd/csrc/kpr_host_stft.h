// kpr_host_stft.h -- host side of kpr_stft_kernels.h (and of the forward kernel of kpr_generic_kernels.h): the DFT-as-GEMM forward
// transform, the launchers of every forward FFT family, stft_pow2_kernel, StftRoute / stft_route, launch_stft, stft_workspace_bytes,
// and run_stft_f32 / run_stft_f64, the bodies of kpr_stft_f32 / kpr_stft_f64.
// Part of the single translation unit kapre_hip.hip (included there after kpr_host_fft.h; not stand-alone).
#pragma once

namespace kpr {

enum { STFT_K, STFT_K3, STFT_K3_CL };                                   // power-of-two STFT kernels (stft_pow2_kernel)

// STFT of every frame into `out` (complex64, in g's output layout), through the DFT-as-GEMM path
static int stft_gemm(const float* x, const Geom& g, const float* window, float* out_cplx, hipStream_t st) {
    const float* dft = nullptr;
    if (int e = get_dft_fwd(g.n_fft, &dft)) return e;
    GemmArgs ga{};
    ga.in.rows = g.total_frames; ga.in.D0 = g.F; ga.in.D1 = g.C;
    if (g.in_cl) { ga.in.s2 = g.T * g.C; ga.in.s1 = 1; ga.t_es = g.C; }
    else { ga.in.s2 = (long long)g.C * g.T; ga.in.s1 = g.T; ga.t_es = 1; }
    ga.in.s0 = 0; ga.in.es = 0;
    ga.out = frames_out_map(g, g.K);
    ga.Kdim = std::min(g.win, g.n_fft);
    ga.N = 2 * g.K;
    ga.ldb = 2 * g.K;
    ga.T = g.T; ga.hop = g.hop; ga.pad_left = g.pad_left;
    ga.window = window; ga.win = g.win;
    return run_gemm<A_FRAME, E_CPLX>(x, dft, ga, out_cplx, st);
}

// k_stft3_cl / k_stft3 / k_stft at a power-of-two n_fft (g as launched: frame numbering g.cfast, output layout g.out_cl)
static int stft_pow2_kernel(const Geom& g, int mode, int cus) {
    const int NC = g.n_fft / 2, G = 64 / (NC / kPts);
    const long long ngroups = (g.total_frames + G - 1) / G;          // wave-loads of G frames
    // channels_last output with several channels (round 4): k_stft3 writes the G channel-frames of a wave as neighbours
    // (n_fft 1024, complex output, even channel count); everything else of that layout stays on k_stft
    const bool cl_ok = g.cfast && (g.C % G) == 0;
    if (mode == KPR_OUT_PHASE || NC < 512 || (g.out_cl && !cl_ok)) return STFT_K;   // (the n_fft 256 / 512 instances spill at 128 VGPRs)
    // k_stft3: one sixteen-wave workgroup per CU drawing frame groups from an LDS counter (stft_variant 0 = automatic, from
    // 8 groups per CU up -- tools/sweep_dispatch.py stft: 13.5 groups per CU 12.2 vs 14.0 us, 2.6 per CU 10.3 vs 7.0 us
    // against k_stft; 3 = always; 1 = k_stft).  The round-3 kernel with static runs per wave (k_stft2) lost to one of the
    // two on every shape of the sweep (profiles/r05_sweep_before_prune.log) and was removed in round 5.
    if (!(opt(OPT_STFT_VARIANT) == 3 || (opt(OPT_STFT_VARIANT) == 0 && ngroups >= 8LL * cus))) return STFT_K;
    // the CL instance (channel-pair fetch at n_fft 1024; channels_last store) whenever a side is interleaved and
    // the G frames of a wave are channels of one (item, frame) -- also for interleaved input with
    // channels_first output (per-row stores there); n_fft 2048 (one frame per wave): channels_last output only
    return cl_ok && (NC == 512 || g.out_cl) ? STFT_K3_CL : STFT_K3;
}

template <int NC, int MODE, bool CL>
static int launch_stft3(const float* x, const Geom& g, const float* window, const float2* tw, void* out, int cus,
                        hipStream_t st) {
    constexpr int G = 64 / (NC / kPts);
    const long long ngroups = (g.total_frames + G - 1) / G;
    const size_t lds3 = stft3_lds_bytes(NC);
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_stft3<NC, MODE, CL>))) return e;
    const unsigned grid3 = (unsigned)std::max<long long>(1, std::min<long long>((ngroups + kStft3Waves - 1) / kStft3Waves, cus));
    hipLaunchKernelGGL((k_stft3<NC, MODE, CL>), dim3(grid3), dim3(64 * kStft3Waves), lds3, st, x, g, window, tw, out,
                       (int)(ngroups / grid3), (int)(ngroups % grid3));
    return launch_check(CL ? "k_stft3_cl" : "k_stft3", NC, MODE == KPR_OUT_COMPLEX ? "complex" : "magnitude");
}

template <int NC, int MODE, bool OUT_CL>
static int launch_stft_inst(const float* x, const Geom& g, const float* window, const float2* tw, void* out, int cus,
                            hipStream_t st) {
    constexpr int G = 64 / (NC / kPts);
    const long long ngroups = (g.total_frames + G - 1) / G;          // wave-loads of G frames
    const size_t lds = stft_lds_bytes(NC);
    // workgroups the hardware can keep resident per CU (registers + LDS), asked from the runtime
    static PerDevice<int> resident_dev;
    int slot;
    if (int e = device_slot(&slot)) return e;
    int& resident = resident_dev.at[slot >= 0 ? slot : 0];             // (a device without a slot shares slot 0)
    if (!resident) {
        KPR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_stft<NC, MODE, OUT_CL>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        int nb = 0;
        KPR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_stft<NC, MODE, OUT_CL>,
                                                             64 * KPR_STFT_WAVES, lds));
        resident = std::max(1, nb);
        if (opt(OPT_VERBOSE))
            fprintf(stderr, "[kapre_hip] k_stft<%d,%d,%d>: %d resident workgroups per CU (lds %zu B)\n", NC, MODE,
                    (int)OUT_CL, resident, lds);
    }
    // at least one group per wave when there is enough work
    const unsigned grid = (unsigned)std::max<long long>(
        1, std::min<long long>((ngroups + KPR_STFT_WAVES - 1) / KPR_STFT_WAVES, (long long)resident * cus));
    hipLaunchKernelGGL((k_stft<NC, MODE, OUT_CL>), dim3(grid), dim3(64 * KPR_STFT_WAVES), lds, st, x, g,
                       window, tw, out, ngroups, g_debug_stamps);
    return launch_check("k_stft", NC, OUT_CL ? (MODE == KPR_OUT_COMPLEX ? "complex,cl" : MODE == KPR_OUT_MAGNITUDE ? "magnitude,cl" : "phase,cl")
                                             : (MODE == KPR_OUT_COMPLEX ? "complex" : MODE == KPR_OUT_MAGNITUDE ? "magnitude" : "phase"));
}

// kernel: stft_pow2_kernel's choice
template <int NC>
static int launch_stft_pow2(int kernel, const float* x, const Geom& g, const float* window, const float2* tw, int mode,
                            void* out, int cus, hipStream_t st) {
    auto run = [&](auto mode_c) -> int {
        constexpr int MODE = decltype(mode_c)::value;
        if constexpr (MODE != KPR_OUT_PHASE && NC >= 512) {
            if (kernel == STFT_K3_CL) return launch_stft3<NC, MODE, true>(x, g, window, tw, out, cus, st);
            if (kernel == STFT_K3) return launch_stft3<NC, MODE, false>(x, g, window, tw, out, cus, st);
        }
        return g.out_cl ? launch_stft_inst<NC, MODE, true>(x, g, window, tw, out, cus, st)
                        : launch_stft_inst<NC, MODE, false>(x, g, window, tw, out, cus, st);
    };
    switch (mode) {
        case KPR_OUT_COMPLEX:   return run(std::integral_constant<int, KPR_OUT_COMPLEX>{});
        case KPR_OUT_MAGNITUDE: return run(std::integral_constant<int, KPR_OUT_MAGNITUDE>{});
        default:                return run(std::integral_constant<int, KPR_OUT_PHASE>{});
    }
}

template <int R>
static int launch_stft_big_inst(const float* x, const Geom& g, const float* window, int mode, void* out, hipStream_t st) {
    constexpr int NW = (R == 2) ? 4 : 2;
    const float2 *tw2048 = nullptr, *twbig = nullptr;
    if (int e = get_twiddles(2048, &tw2048)) return e;
    if (int e = get_twiddles(g.n_fft, &twbig)) return e;
    const size_t lds = sizeof(float) * 2 * (size_t)NW * (R * 1024 + 1);
    static LdsOptIn lds_opt_in;
    return launch_framewise(&k_stft_big<R>, &lds_opt_in, g.total_frames, NW, 2, 64 * NW, lds, st, "k_stft_big", 0,
                            x, g, window, tw2048, twbig, mode, out);
}

static int launch_stft_big(const float* x, const Geom& g, const float* window, int mode, void* out, hipStream_t st) {
    return g.n_fft == 4096 ? launch_stft_big_inst<2>(x, g, window, mode, out, st)
                           : launch_stft_big_inst<4>(x, g, window, mode, out, st);
}

template <int M>
static int launch_stft_bs_m(const float* x, const Geom& g, const float* window, const float2* tw,
                            const float2* bs, int mode, void* out, hipStream_t st) {
    constexpr int L = M / kPts, G = 64 / L;
    const long long ngroups = (g.total_frames + G - 1) / G;
    const size_t lds = sizeof(float) * ((size_t)4 * G * bs_slot_words(M, g.n_fft / 2) + 2 * (size_t)(3 * M + g.n_fft / 2 + 2));
    static LdsOptIn lds_opt_in;
    return launch_framewise(&k_stft_bs<M>, &lds_opt_in, ngroups, 4, 2, 256, lds, st, "k_stft_bs", 0,
                            x, g, window, tw, bs, mode, out, ngroups);
}

template <class FF>
static int launch_stft_mr_inst(const float* x, const Geom& g, const float* window, const float2* tw, int mode,
                               void* out, hipStream_t st) {
    constexpr int G = 64 / FF::L;
    const long long ngroups = (g.total_frames + G - 1) / G;
    const size_t lds = mr_lds_bytes<FF>();
    static LdsOptIn lds_opt_in;
    return launch_framewise(&k_stft_mr<FF>, &lds_opt_in, ngroups, 4, 3 /* ~150 VGPRs: three workgroups per CU */, 256, lds, st,
                            "k_stft_mr", FF::N, x, g, window, tw, mode, out, ngroups);
}

static int launch_stft_mr(const float* x, const Geom& g, const float* window, int mode, void* out, hipStream_t st) {
    const float2* tw = nullptr;
    if (int e = get_twiddles(g.n_fft, &tw)) return e;
    return with_mr(g.n_fft, [&](auto ff) {
        return launch_stft_mr_inst<typename decltype(ff)::type>(x, g, window, tw, mode, out, st);
    });
}

static int launch_stft_bs(const float* x, const Geom& g, const float* window, int mode, void* out,
                          hipStream_t st) {
    const int m = bluestein_m(g.n_fft);
    const float2 *tw = nullptr, *bs = nullptr;
    if (int e = get_twiddles(2 * m, &tw)) return e;
    if (int e = get_bluestein(g.n_fft, &bs)) return e;
    return with_pow2(m, [&](auto m_c) { return launch_stft_bs_m<m_c>(x, g, window, tw, bs, mode, out, st); });
}

// the run-time mixed-radix forward FFT, T = float (FAM_GEN) or double (run_stft_f64); LDS opt-in state per T and instance
template <typename T>
static int launch_stft_gen(const T* x, const Geom& g, const T* window, int mode, void* out, hipStream_t st) {
    typedef typename Cplx<T>::type T2;
    GenLaunch l;
    if (int e = gen_launch_plan(sizeof(T2), g.n_fft, &l)) return e;
    const T2* tw = nullptr;
    if (int e = twiddles_of<T>(g.n_fft, &tw)) return e;
    static LdsOptIn opt_in[2];
    return launch_gen(l.tw_lds ? &k_stft_gen<T, true> : &k_stft_gen<T, false>, opt_in[l.tw_lds ? 1 : 0], l, g, st,
                      sizeof(T) == 4 ? "k_stft_gen<float>" : "k_stft_gen<double>", x, g, window, tw, l.p, mode, out);
}

struct StftRoute {
    int fam;                   // FAM_*
    int kernel;                // FAM_POW2: stft_pow2_kernel
    int cfast;                 // Geom::cfast of the launch
    int64_t workspace;         // bytes the call needs
};

// s: the cropped geometry (forward_geom), g: its Geom
static StftRoute stft_route(const kpr_stft_geom* s, const Geom& g, int mode, int cus) {
    StftRoute r{fft_family(s), STFT_K, 0, 0};
    if (r.fam == FAM_POW2) {
        // channel-fastest frame numbering whenever either side is interleaved: the frames that share the waveform's cache
        // lines / the spectrogram's channel runs sit in one wave
        Geom gk = g;
        gk.cfast = r.cfast = ((g.in_cl || g.out_cl) && g.C > 1) ? 1 : 0;
        r.kernel = stft_pow2_kernel(gk, mode, cus);
    }
    // every FFT family writes |X| / phase itself; the DFT-GEMM path with a real-valued epilogue stages the complex spectrum in
    // the workspace
    if (r.fam == FAM_GEMM && mode != KPR_OUT_COMPLEX) r.workspace = (int64_t)sizeof(float) * 2 * g.total_frames * g.K;
    return r;
}

// the forward transform of route `r` into `out` (the DFT-GEMM family: complex output only)
static int launch_stft(const StftRoute& r, const float* x, const Geom& g, const float* window, int mode, void* out, int cus,
                       hipStream_t st) {
    switch (r.fam) {
        case FAM_POW2: {
            const float2* tw = nullptr;
            if (int e = get_twiddles(g.n_fft, &tw)) return e;
            return with_pow2(g.n_fft / 2, [&](auto nc) {
                return launch_stft_pow2<decltype(nc)::value>(r.kernel, x, g, window, tw, mode, out, cus, st);
            });
        }
        case FAM_MR:  return launch_stft_mr(x, g, window, mode, out, st);
        case FAM_BS:  return launch_stft_bs(x, g, window, mode, out, st);
        case FAM_BIG: return launch_stft_big(x, g, window, mode, out, st);
        case FAM_GEN: return launch_stft_gen<float>(x, g, window, mode, out, st);
        default:      return stft_gemm(x, g, window, (float*)out, st);
    }
}

// kpr_stft_workspace_bytes (and the forward transforms of Griffin-Lim)
static int64_t stft_workspace_bytes(const kpr_stft_geom* s, int mode) {
    if (check_geom(s)) return -1;
    const kpr_stft_geom se = forward_geom(s);
    // (no device query: the CU count only picks among kernels that need no workspace)
    return stft_route(&se, make_geom(&se, frames_of(s)), mode, 256).workspace;
}

// ---- kpr_stft_f32: checks, route, launch (run_griffin_lim runs it once per iteration) ----
static int run_stft_f32(const float* x, const kpr_stft_geom* s, const float* window, void* out, int mode,
                        void* workspace, int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = check_geom(s)) return e;
    if (mode < 0 || mode > 2) return fail(KPR_E_BADARG, "bad output mode %d", mode);
    const long long F = frames_of(s);
    const kpr_stft_geom se = forward_geom(s);                    // win_length > n_fft: cropped frames (see forward_geom)
    s = &se;
    Geom g = make_geom(s, F);
    if (g.total_frames == 0) return 0;
    if (!x || !window || !out) return fail(KPR_E_BADARG, "x / window / out must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const StftRoute r = stft_route(s, g, mode, cus);
    g.cfast = r.cfast;
    if (r.fam != FAM_GEMM || mode == KPR_OUT_COMPLEX) return launch_stft(r, x, g, window, mode, out, cus, st);
    if (!workspace || workspace_bytes < r.workspace)
        return fail(KPR_E_WORKSPACE, "stft workspace: need %lld bytes", (long long)r.workspace);
    if (int e = stft_gemm(x, g, window, (float*)workspace, st)) return e;
    const long long n = g.total_frames * g.K;
    hipLaunchKernelGGL(k_cplx_to_real, dim3(grid_1d(n, 256)), dim3(256), 0, st,
                       (const float2*)workspace, n, mode == KPR_OUT_PHASE ? 1 : 0, (float*)out);
    return launch_check("k_cplx_to_real");
}

// ---- kpr_stft_f64: the generic engine at every transform size ----
static int run_stft_f64(const double* x, const kpr_stft_geom* s, const double* window, void* out, int mode, kpr_stream_t stream) {
    if (int e = check_geom(s)) return e;
    if (mode < KPR_OUT_COMPLEX || mode > KPR_OUT_PHASE) return fail(KPR_E_BADARG, "bad mode %d", mode);
    const long long F = frames_of(s);
    Geom g = make_geom(s, F);
    if (g.total_frames == 0) return 0;
    if (!x || !window || !out) return fail(KPR_E_BADARG, "x / window / out must not be NULL");
    g.win = std::min(g.win, g.n_fft);                            // win_length > n_fft: cropped frames (see forward_geom)
    return launch_stft_gen<double>(x, g, window, mode, out, (hipStream_t)stream);
}

}  // namespace kpr
