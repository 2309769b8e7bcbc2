// kpr_host_istft.h -- host side of kpr_istft_kernels.h / kpr_istft_pw_kernels.h (and of the inverse kernel of kpr_generic_kernels.h):
// the plans and launchers of the one-launch inverse kernels, the inverse-FFT launchers of the two-kernel path, IstftRoute /
// istft_route, the overlap-add tail, istft_workspace_bytes, and run_istft_f32 / run_istft_f64, the bodies of kpr_istft_f32 / _f64.
// Part of the single translation unit kapre_hip.hip (included there after kpr_host_stft.h; not stand-alone).
#pragma once

namespace kpr {

struct IstftRoute {
    int fam;                   // IST_*, else the irFFT family (FAM_*) of the two-kernel path
    int S, il;                 // IST_PW: register slots per hop, interleaved instance
    int rj;                    // IST_WS / IST_WS_MR: rows read per sample group
    IstftPwPlan pw;
    IstftWsPlan ws;
    IstftPlan fused;
    size_t lds;
    unsigned grid;
    long long nitems;          // IST_WS / IST_WS_MR: items, IST_FUSED: blocks
};

static bool istft_fused_plan(const kpr_stft_geom* s, long long F, const float* out, int cus, IstftRoute* r) {
    const int NC = s->n_fft / 2, L = NC / kPts, G = 64 / L, NW = NC == 1024 ? 8 : 4;
    const int win = s->win_length, hop = s->hop_length;
    if (hop > win || F < 1) return false;                   // gaps between frames: two-kernel path
    const int R = (win + hop - 1) / hop;
    const int RS = ((std::max(win, NC) + 3) & ~3) + 4;
    const int spare = (G > 1) ? NW * (G - 1) : 0;           // scratch rows for idle frame slots
    // rows: as many as fit next to a second workgroup on the CU (80 KiB each), at most 16; if that
    // leaves too few new frames per block, take the whole CU (160 KiB) instead
    // (an 8-wave workgroup at ~190 VGPRs fills the CU's register file on its own)
    int NR = (NW == 8) ? 0 : std::min(16, (int)(80 * 1024 / (sizeof(float) * RS)) - spare);
    if (NR < R + 3) NR = std::min(16, (int)(160 * 1024 / (sizeof(float) * RS)) - spare);
    if (NR < R + 1) return false;
    IstftPlan& pl = r->fused;
    pl.n_sig = (long long)s->batch * s->channels;
    pl.t_out = (F - 1) * (long long)hop + win;
    pl.F = (int)F; pl.C = s->channels; pl.win = win; pl.hop = hop;
    pl.NR = NR; pl.R = R; pl.FB = NR - R + 1;
    pl.RS = RS;
    pl.chunks = (int)((pl.t_out + (long long)pl.FB * hop - 1) / ((long long)pl.FB * hop));
    pl.spec_cl = s->out_layout == KPR_CHANNELS_LAST;
    pl.wave_cl = s->in_layout == KPR_CHANNELS_LAST;
    pl.vec4 = hop % 4 == 0 && win % 4 == 0 && !(pl.wave_cl && s->channels > 1) &&
              (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const size_t lds = sizeof(float) * (size_t)(NR + spare) * pl.RS;
    if (lds > 160 * 1024) return false;
    r->fam = IST_FUSED;
    r->lds = lds;
    r->nitems = pl.n_sig * pl.chunks;
    const int per_cu = std::max(1, (int)(160 * 1024 / lds));
    r->grid = (unsigned)std::min<long long>(r->nitems, (long long)std::min(per_cu, 2) * cus);
    return true;
}

template <int NC, int NW>
static int launch_istft_fused(const float2* spec, const IstftRoute& r, const float* synth, const float2* tw, float* out,
                              hipStream_t st) {
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_istft_fused<NC, NW>))) return e;
    hipLaunchKernelGGL((k_istft_fused<NC, NW>), dim3(r.grid), dim3(NW * 64), r.lds, st, spec, r.fused, synth,
                       tw, out, r.nitems);
    return launch_check("k_istft_fused", NC);
}

// segments per signal for k_istft_ws: rounds of `cus` workgroups x (blocks + halo frames) per segment
static int istft_ws_segments(long long n_sig, int Q, int R, int cus) {
    // cost of a schedule in frame times: rounds of `cus` workgroups x (hop blocks + halo frames + the
    // fixed start of a segment: first spectrum rows from HBM, pipeline fill -- about 20 frames' worth)
    int best = 1;
    double best_cost = 1e300;
    const int smax = std::max(1, std::min(4096, Q / (4 * R)));
    for (int sg = 1; sg <= smax; ++sg) {
        const long long rounds = (n_sig * sg + cus - 1) / cus;
        const double cost = (double)rounds * ((Q + sg - 1) / sg + R - 1 + 20);
        if (cost < best_cost * 0.999) { best_cost = cost; best = sg; }
        if (n_sig * sg > 8LL * cus) break;          // more segments than that only add halos
    }
    return best;
}

template <int NC, int RJ>
static int launch_istft_ws_inst(const float2* spec, const IstftWsPlan& pl, size_t lds, unsigned grid,
                                const float* synth, const float2* tw, float* out, int nitems, hipStream_t st) {
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_istft_ws<NC, RJ>))) return e;
    if (int e = status_word_ready()) return e;                  // (the kernel's bounded waits report there)
    hipLaunchKernelGGL((k_istft_ws<NC, RJ>), dim3(grid), dim3(kIwThreads), lds, st, spec, pl, synth, tw, out,
                       nitems, g_debug_stamps);
    return launch_check("k_istft_ws", NC, RJ == 2 ? "rj2" : RJ == 4 ? "rj4" : "rj8");
}

// Plan of the ring kernels (k_istft_ws, k_istft_ws_mr); false when they do not apply.
//   row_min: floats a ring row needs as FFT exchange buffer, G: frames per producer ticket,
//   spare: extra rows (exchange rows of idle frame slots), extra: LDS bytes behind rows / flags / counters
//   vec_min: 4 = only groups of four samples per consumer lane (k_istft_ws), 2 = pairs allowed as well
//   *vec: samples per consumer lane and group the plan uses (4 or 2)
static bool istft_ws_plan(const kpr_stft_geom* s, long long F, const float* out, int row_min, int G, int spare,
                          size_t extra, int cus, int vec_min, IstftWsPlan* plo, size_t* lds, int* rj, int* vec,
                          long long* nitems) {
    const int win = s->win_length, hop = s->hop_length;
    if (hop > win || F < 1 || opt(OPT_ISTFT_PATH) == 1 || opt(OPT_ISTFT_PATH) == 2) return false;
    // contiguous waveform and contiguous spectrogram rows (channels_first, or one channel)
    if ((s->in_layout == KPR_CHANNELS_LAST && s->channels > 1) || (s->out_layout == KPR_CHANNELS_LAST && s->channels > 1))
        return false;
    // VEC samples per lane in the overlap-add: hop, win multiples of VEC, 4 * VEC byte aligned waveform
    int VEC = 0;
    if (hop % 4 == 0 && win % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) VEC = 4;
    else if (vec_min <= 2 && hop % 2 == 0 && win % 2 == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0) VEC = 2;
    if (!VEC) return false;
    const long long n_sig = (long long)s->batch * s->channels;
    const long long t_out = (F - 1) * (long long)hop + win;
    if (n_sig * 4096 >= (1LL << 31) || t_out + hop >= (1LL << 31)) return false;
    IstftWsPlan pl;
    pl.t_out = t_out;
    pl.F = (int)F; pl.C = s->channels; pl.win = win; pl.hop = hop;
    pl.R = (win + hop - 1) / hop;
    const int RJ = pl.R <= 2 ? 2 : pl.R <= 4 ? 4 : 8;         // rows read per sample group
    if (pl.R > 8) return false;
    if (VEC == 2 && RJ != 4) return false;                     // pairs: only the four-row instance is built
    const int per_pass = 64 * (kIwReads / RJ);                 // sample groups per consumer pass
    if (hop / VEC > per_pass) return false;                    // a hop block must fit one pass
    pl.RS = ((std::max(win, row_min) + 3) & ~3) + 4;
    pl.Q = (int)F - 1 + pl.R;
    pl.QB = std::min(16, per_pass / (hop / VEC));
    auto bytes = [&](int nr) { return sizeof(float) * (size_t)(nr + spare) * pl.RS + sizeof(int) * (size_t)(nr + 8) + extra; };
    int NR = 128;
    while (NR > 1 && bytes(NR) > 160 * 1024) NR >>= 1;
    // room for the frames of the two passes in flight (R-1+2*QB), the producers' tickets and slack
    if (NR < pl.R - 1 + 2 * pl.QB + 2 * G + 1 || pl.R - 1 + pl.QB > 64) return false;
    pl.NR = NR;
    pl.segs = istft_ws_segments(n_sig, pl.Q, pl.R, cus);
    pl.QS = (pl.Q + pl.segs - 1) / pl.segs;
    pl.segs = (pl.Q + pl.QS - 1) / pl.QS;                       // no empty segment
    *plo = pl;
    *lds = bytes(NR);
    *rj = RJ;
    *vec = VEC;
    *nitems = n_sig * pl.segs;
    return true;
}

// k_istft_ws at a power-of-two n_fft
static bool istft_ring_plan(const kpr_stft_geom* s, long long F, const float* out, int cus, IstftRoute* r) {
    const int NC = s->n_fft / 2, G = 64 / (NC / kPts);
    int vec;
    if (!istft_ws_plan(s, F, out, NC, G, kIwProd * (G - 1), 0, cus, 4, &r->ws, &r->lds, &r->rj, &vec, &r->nitems)) return false;
    r->fam = IST_WS;
    r->grid = (unsigned)std::min<long long>(r->nitems, cus);
    return true;
}

template <int NC>
static int launch_istft_ws(const float2* spec, const IstftRoute& r, const float* synth, const float2* tw, float* out,
                           hipStream_t st) {
    switch (r.rj) {
        case 2:  return launch_istft_ws_inst<NC, 2>(spec, r.ws, r.lds, r.grid, synth, tw, out, (int)r.nitems, st);
        case 4:  return launch_istft_ws_inst<NC, 4>(spec, r.ws, r.lds, r.grid, synth, tw, out, (int)r.nitems, st);
        default: return launch_istft_ws_inst<NC, 8>(spec, r.ws, r.lds, r.grid, synth, tw, out, (int)r.nitems, st);
    }
}

// ---- k_istft_pw: every wave a complete worker, the overlap-add in registers (kpr_istft_pw_kernels.h) ---------------------
template <int NC, int S, bool IL>
static int launch_istft_pw_inst(const float2* spec, const IstftPwPlan& pl_in, unsigned grid, const float* synth,
                                const float2* tw, float* out, hipStream_t st) {
    constexpr int W = 16, NSTR = W * (64 / (NC / kPts));
    IstftPwPlan pl = pl_in;
    // as many LDS stashes for the partial head blocks as fit behind the exchange rows and tables (the streams of the first
    // frame run -- one per channel -- have no predecessor)
    pl.n_stash = (int)std::min<size_t>(NSTR - (IL ? pl.C : 1), (160 * 1024 - ipw_lds_bytes(NC, W)) / ipw_stash_bytes(NC, S));
    const size_t lds = ipw_lds_bytes(NC, W) + pl.n_stash * ipw_stash_bytes(NC, S);
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_istft_pw<NC, S, W, IL>))) return e;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_istft_pw<%d,%d,%s>: grid %u, lds %zu B (%d stashes), %d segments per signal, %d items\n", NC, S,
                IL ? "interleaved" : "contiguous", grid, lds, pl.n_stash, pl.segs, pl.nitems);
    if (int e = status_word_ready()) return e;                  // (the kernel's bounded waits report there)
    hipLaunchKernelGGL((k_istft_pw<NC, S, W, IL>), dim3(grid), dim3(W * 64), lds, st, spec, pl, synth, tw, out);
    return launch_check(IL ? "k_istft_pw_il" : "k_istft_pw", NC, S == 2 ? "s2" : S == 4 ? "s4" : "s8");
}
static bool istft_pw_plan(const kpr_stft_geom* s, long long F, int cus, IstftRoute* r) {
    const int NC = s->n_fft / 2, L = NC / kPts, G = 64 / L, NSTR = 16 * G;
    const int win = s->win_length, hop = s->hop_length;
    // hop = S x (2 L samples), S = 2 / 4 / 8: the next frame's samples sit S register slots further down in the same lane
    if (hop % (2 * L) || win > 2 * NC || hop > win || F < 1) return false;
    const int S = hop / (2 * L);
    if (S != 2 && S != 4 && S != 8) return false;
    // contiguous waveform and contiguous spectrogram rows (channels_first, or one channel): a stream = a frame run of one
    // signal.  An interleaved side (channels_last, C > 1; round 4): the IL instances, streams = (frame run, channel) with
    // the channel fastest, an item = a segment of one batch item -- C a power of two that divides the streams of a workgroup,
    // hop = n_fft / 4 or / 2 (the instances that are built)
    const bool il = (s->in_layout == KPR_CHANNELS_LAST && s->channels > 1) || (s->out_layout == KPR_CHANNELS_LAST && s->channels > 1);
    const int C = s->channels;
    if (il && ((C & (C - 1)) != 0 || C > NSTR || S == 2)) return false;
    const int runs = il ? NSTR / C : NSTR;                                       // frame runs per item
    const long long n_sig = il ? (long long)s->batch : (long long)s->batch * s->channels;
    const long long t_out = (F - 1) * (long long)hop + win;
    if (n_sig * 4096 >= (1LL << 31) || t_out + 2LL * NC >= (1LL << 31) || F >= (1LL << 30)) return false;
    // segments per signal: every stream of a segment needs R - 1 frames of its own (run boundaries are two-party sums);
    // cost of a schedule = rounds of `cus` workgroups x (frames per stream + a fixed start)
    const int R = kPts / S;
    const long long need = (long long)runs * (R - 1);
    const int segs_max = (int)std::min<long long>(4096, F / need);
    if (segs_max < 1) return false;
    int segs = 1;
    double best = 1e300;
    for (int sg = 1; sg <= segs_max; ++sg) {
        const long long rounds = (n_sig * sg + cus - 1) / cus;
        const double cost = (double)rounds * ((double)((F + sg - 1) / sg + R - 1 + runs - 1) / runs + 3.0);
        if (cost < best * 0.999) { best = cost; segs = sg; }
        if (n_sig * sg > 8LL * cus) break;
    }
    // fewer items than three quarters of the CUs: the ring kernel (32 x 434 frames at n_fft 1024 = 128 items: 30.8 vs 31.5 us)
    if (opt(OPT_ISTFT_PATH) == 0 && n_sig * segs * 4 < 3LL * cus) return false;
    IstftPwPlan& pl = r->pw;
    pl.t_out = t_out; pl.F = (int)F; pl.win = win; pl.hop = hop; pl.segs = segs; pl.nitems = (int)(n_sig * segs);
    pl.seg_q = (int)(F / segs); pl.seg_r = (int)(F % segs);
    pl.n_stash = 0;
    pl.C = il ? C : 1;
    // (kpr_stft_geom: in_layout = the WAVEFORM's layout, out_layout = the SPECTROGRAM's -- for the inverse as well)
    pl.in_cl = (il && s->out_layout == KPR_CHANNELS_LAST) ? 1 : 0;              // the kernel's input: the spectrogram
    pl.out_cl = (il && s->in_layout == KPR_CHANNELS_LAST) ? 1 : 0;              // its output: the waveform
    r->fam = IST_PW;
    r->S = S;
    r->il = il;
    r->grid = (unsigned)std::min<long long>(pl.nitems, cus);
    return true;
}

template <int NC>
static int launch_istft_pw(const float2* spec, const IstftRoute& r, const float* synth, const float2* tw, float* out,
                           hipStream_t st) {
    if (r.il) return r.S == 4 ? launch_istft_pw_inst<NC, 4, true>(spec, r.pw, r.grid, synth, tw, out, st)
                              : launch_istft_pw_inst<NC, 8, true>(spec, r.pw, r.grid, synth, tw, out, st);
    switch (r.S) {
        case 2:  return launch_istft_pw_inst<NC, 2, false>(spec, r.pw, r.grid, synth, tw, out, st);
        case 4:  return launch_istft_pw_inst<NC, 4, false>(spec, r.pw, r.grid, synth, tw, out, st);
        default: return launch_istft_pw_inst<NC, 8, false>(spec, r.pw, r.grid, synth, tw, out, st);
    }
}

template <int R>
static int launch_irfft_big_inst(const float2* spec, const Geom& g, const float* synth, float* frames, hipStream_t st) {
    constexpr int NW = (R == 2) ? 4 : 2;
    const float2 *tw2048 = nullptr, *twbig = nullptr;
    if (int e = get_twiddles(2048, &tw2048)) return e;
    if (int e = get_twiddles(g.n_fft, &twbig)) return e;
    const size_t lds = sizeof(float) * 2 * (size_t)(2 * NW) * (R * 1024 + 1);
    static LdsOptIn lds_opt_in;
    return launch_framewise(&k_irfft_big<R>, &lds_opt_in, g.total_frames, NW, 1 /* 128 KiB of LDS */, 64 * NW, lds, st, "k_irfft_big", 0,
                            spec, g, synth, tw2048, twbig, frames);
}

static int launch_irfft_big(const float2* spec, const Geom& g, const float* synth, float* frames, hipStream_t st) {
    return g.n_fft == 4096 ? launch_irfft_big_inst<2>(spec, g, synth, frames, st)
                           : launch_irfft_big_inst<4>(spec, g, synth, frames, st);
}

template <int M>
static int launch_irfft_bs_m(const float2* spec, const Geom& g, const float* synth, const float2* tw,
                             const float2* bs, float* frames, hipStream_t st) {
    constexpr int L = M / kPts, G = 64 / L;
    const long long ngroups = (g.total_frames + G - 1) / G;
    const size_t lds = sizeof(float) * ((size_t)4 * G * ((M + M / 32 + 24 + 3) / 4 * 4) +
                                        2 * (size_t)(3 * M + g.n_fft / 2 + 2));
    // (under 64 KiB at every M: no LDS opt-in)
    return launch_framewise(&k_irfft_bs<M>, nullptr, ngroups, 4, 2, 256, lds, st, "k_irfft_bs", 0, spec, g, synth, tw, bs, frames, ngroups);
}

template <class FF>
static int launch_irfft_mr_inst(const float2* spec, const Geom& g, const float* synth, const float2* tw,
                                float* frames, hipStream_t st) {
    constexpr int G = 64 / FF::L;
    const long long ngroups = (g.total_frames + G - 1) / G;
    const size_t lds = mr_lds_bytes<FF>();
    static LdsOptIn lds_opt_in;
    return launch_framewise(&k_irfft_mr<FF>, &lds_opt_in, ngroups, 4, 2, 256, lds, st, "k_irfft_mr", 0,
                            spec, g, synth, tw, frames, ngroups);
}

static int launch_irfft_mr(const float2* spec, const Geom& g, const float* synth, float* frames, hipStream_t st) {
    const float2* tw = nullptr;
    if (int e = get_twiddles(g.n_fft, &tw)) return e;
    return with_mr(g.n_fft, [&](auto ff) {
        return launch_irfft_mr_inst<typename decltype(ff)::type>(spec, g, synth, tw, frames, st);
    });
}

template <class FF, int RJ, int VEC>
static int launch_istft_ws_mr_inst(const float2* spec, const IstftWsPlan& pl, size_t lds, unsigned grid,
                                   const float* synth, const float2* tw, float* out, int nitems, hipStream_t st) {
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_istft_ws_mr<FF, RJ, VEC>))) return e;
    if (int e = status_word_ready()) return e;                  // (the kernel's bounded waits report there)
    hipLaunchKernelGGL((k_istft_ws_mr<FF, RJ, VEC>), dim3(grid), dim3(kIwThreads), lds, st, spec, pl, synth, tw,
                       out, nitems);
    return launch_check("k_istft_ws_mr", FF::N, RJ == 2 ? (VEC == 4 ? "rj2,v4" : "rj2,v2") : RJ == 4 ? (VEC == 4 ? "rj4,v4" : "rj4,v2")
                                                                                   : (VEC == 4 ? "rj8,v4" : "rj8,v2"));
}

// the ring kernel with mixed-radix producers (n_fft with a mixed-radix plan)
static bool istft_ws_mr_plan(const kpr_stft_geom* s, long long F, const float* out, int cus, IstftRoute* r) {
    if (!mixed_radix_plan(s->n_fft) || !opt(OPT_MIXED_RADIX) || s->win_length > s->n_fft) return false;
    int vec = 0;
    bool ok = false;
    with_mr(s->n_fft, [&](auto ff) {
        using FF = typename decltype(ff)::type;
        // rows double as exchange rows (ROW complex words); window pairs and the twiddle table behind the counters
        ok = istft_ws_plan(s, F, out, 2 * FF::ROW, 64 / FF::L, 0, sizeof(float) * 2 * 3 * (size_t)FF::N, cus, 2, &r->ws, &r->lds,
                           &r->rj, &vec, &r->nitems);
        return 0;
    });
    if (!ok || r->rj > 4) return false;                         // more than four overlapping frames: two-kernel path
    // hop or win_length not a multiple of four: the consumer would sum and store 8 bytes per lane.  Those 18 instances
    // (k_istft_ws_mr<FF, 4, 2>) were removed in round 6: on 64 x 10 s @ 16 kHz they beat irFFT + overlap-add as two kernels by at
    // most 1.4x (n_fft 200 / hop 50: 156 vs 214 us, 1000 / 250: 154 vs 189, 120 / 30: 156 vs 187) and LOST at 360 / 90 (205 vs
    // 138) and 600 / 150 (245 vs 199) -- profiles/r06_sweep_before_prune.log; VERDICT r05 item 7 asked for > 1.5x.
    if (vec == 2) return false;
    r->fam = IST_WS_MR;
    r->grid = (unsigned)std::min<long long>(r->nitems, cus);
    return true;
}

static int launch_istft_ws_mr(const float2* spec, const IstftRoute& r, int n_fft, const float* synth, float* out, hipStream_t st) {
    const float2* tw = nullptr;
    if (int e = get_twiddles(n_fft, &tw)) return e;
    return with_mr(n_fft, [&](auto ff) {
        using FF = typename decltype(ff)::type;
        return r.rj == 2 ? launch_istft_ws_mr_inst<FF, 2, 4>(spec, r.ws, r.lds, r.grid, synth, tw, out, (int)r.nitems, st)
                         : launch_istft_ws_mr_inst<FF, 4, 4>(spec, r.ws, r.lds, r.grid, synth, tw, out, (int)r.nitems, st);
    });
}

static int launch_irfft_bs(const float2* spec, const Geom& g, const float* synth, float* frames,
                           hipStream_t st) {
    const int m = bluestein_m(g.n_fft);
    const float2 *tw = nullptr, *bs = nullptr;
    if (int e = get_twiddles(2 * m, &tw)) return e;
    if (int e = get_bluestein(g.n_fft, &bs)) return e;
    return with_pow2(m, [&](auto m_c) { return launch_irfft_bs_m<m_c>(spec, g, synth, tw, bs, frames, st); });
}

template <int NC>
static int launch_irfft_fast(const float2* spec, const Geom& g, const float* synth,
                             const float2* tw, float* frames, hipStream_t st) {
    constexpr int L = NC / kPts, G = 64 / L;
    const long long nblocks = (g.total_frames + 4 * G - 1) / (4 * G);
    const size_t lds = sizeof(float) * (4 * G * NC + 4 * G * (2 * NC + 8));          // 49 KiB at every NC: no LDS opt-in, two per CU
    return launch_framewise(&k_irfft<NC>, nullptr, nblocks, 1, 2, 256, lds, st, "k_irfft", 0, spec, g, synth, tw, frames, nblocks);
}

// the run-time mixed-radix inverse FFT, T = float (FAM_GEN) or double (run_istft_f64); LDS opt-in state per T and instance
template <typename T>
static int launch_irfft_gen(const typename Cplx<T>::type* spec, const Geom& g, const T* synth_window, T* frames, hipStream_t st) {
    typedef typename Cplx<T>::type T2;
    GenLaunch l;
    if (int e = gen_launch_plan(sizeof(T2), g.n_fft, &l)) return e;
    const T2* tw = nullptr;
    if (int e = twiddles_of<T>(g.n_fft, &tw)) return e;
    static LdsOptIn opt_in[2];
    return launch_gen(l.tw_lds ? &k_irfft_gen<T, true> : &k_irfft_gen<T, false>, opt_in[l.tw_lds ? 1 : 0], l, g, st,
                      sizeof(T) == 4 ? "k_irfft_gen<float>" : "k_irfft_gen<double>", spec, g, synth_window, tw, l.p, frames);
}

// the workspace of the two-kernel path (kpr_istft_workspace_bytes, kpr_istft_f64_workspace_bytes): every windowed frame
template <typename T>
static int64_t istft_workspace_bytes(const kpr_stft_geom* s, int64_t n_frames) {
    if (check_geom(s) || n_frames < 0) return -1;
    return 256 + (int64_t)sizeof(T) * s->batch * s->channels * n_frames * s->win_length;
}

// the second kernel of the two-kernel path: overlap-add of the windowed frames in the workspace into the waveform
// (interleaved: the waveform is channels_last)
template <typename T>
static int run_ola(const T* frames, const kpr_stft_geom* s, int64_t n_frames, bool interleaved, T* out, hipStream_t st) {
    const long long t_out = (n_frames - 1) * (long long)s->hop_length + s->win_length;
    const long long n_sig = (long long)s->batch * s->channels;
    hipLaunchKernelGGL(k_ola<T>, dim3(grid_1d(n_sig * t_out, 256)), dim3(256), 0, st, frames, n_sig,
                       (int)n_frames, s->channels, s->win_length, s->hop_length, t_out, interleaved ? 1 : 0, out);
    return launch_check("k_ola");
}

// F: frames per signal, g: the call's Geom, out: the waveform (alignment of the overlap-add stores)
static IstftRoute istft_route(const kpr_stft_geom* s, long long F, const Geom& g, const float* out, int cus) {
    IstftRoute r{};
    const int path = opt(OPT_ISTFT_PATH);
    if (fast_nfft(s->n_fft) && path != 2) {
        // fused irFFT + window + overlap-add (no workspace traffic) whenever the frames overlap.
        // Launches of a few thousand frames -- batch 1 ... 8 of clips, the serving case -- are latency bound and the
        // barrier kernel (many small workgroups, one barrier) beats the ring kernel's serial walk over short segments:
        // 4 x 434 frames at n_fft 1024 12.0 vs 15.2 us, 16 x 83 at n_fft 2048 16.0 vs 20.3, 16 x 61 at n_fft 512 8.0 vs
        // 9.1; from ~3.5 k frames up the ring kernel wins (16 x 434: 20.0 vs 24.4; cfg4: 77 vs 122)
        // (tools/kbench_istft_variants.py; kpr_set_option("istft_path", 3) = the ring kernel whatever the size).
        const bool small = path == 0 && g.total_frames <= 3072;
        // k_istft_pw (round 4): hop = n_fft / 8, / 4, / 2, launches that fill the chip (istft_path 4 = wherever it applies)
        if (((path == 0 && !small) || path == 4) && s->n_fft >= 512 && istft_pw_plan(s, F, cus, &r)) return r;
        // the wave-specialised ring kernel when its preconditions hold, then the barrier kernel
        if (!small && istft_ring_plan(s, F, out, cus, &r)) return r;
        if (istft_fused_plan(s, F, out, cus, &r)) return r;
        if (small && istft_ring_plan(s, F, out, cus, &r)) return r;   // the barrier kernel did not apply (no overlap ...): the ring kernel may
    }
    // n_fft = 2^a 5^b ...: the ring kernel with mixed-radix producers
    if (!fast_nfft(s->n_fft) && path != 2 && istft_ws_mr_plan(s, F, out, cus, &r)) return r;
    r.fam = fft_family(s);
    return r;
}

// ---- kpr_istft_f32: checks, route, launch (run_griffin_lim runs it once per iteration) ----
static int run_istft_f32(const void* spec, const kpr_stft_geom* s, int64_t n_frames, const float* synth_window, float* out,
                         void* workspace, int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = check_geom(s)) return e;
    if (n_frames < 0) return fail(KPR_E_BADARG, "negative frame count");
    Geom g = make_geom(s, n_frames);
    g.pad_left = 0;
    if (g.total_frames == 0) return 0;
    if (!spec || !synth_window || !out) return fail(KPR_E_BADARG, "spec / window / out must not be NULL");
    const int64_t need = istft_workspace_bytes<float>(s, n_frames);
    if (!workspace || workspace_bytes < need)
        return fail(KPR_E_WORKSPACE, "istft workspace: need %lld bytes", (long long)need);
    hipStream_t st = (hipStream_t)stream;
    float* frames = reinterpret_cast<float*>(workspace);
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const IstftRoute r = istft_route(s, n_frames, g, out, cus);
    const float2* sp = (const float2*)spec;
    if (r.fam >= IST_PW) {
        if (r.fam == IST_WS_MR) return launch_istft_ws_mr(sp, r, s->n_fft, synth_window, out, st);
        const float2* tw = nullptr;
        if (int e = get_twiddles(s->n_fft, &tw)) return e;
        return with_pow2(s->n_fft / 2, [&](auto nc) {
            constexpr int NC = decltype(nc)::value;
            if (r.fam == IST_WS) return launch_istft_ws<NC>(sp, r, synth_window, tw, out, st);
            if (r.fam == IST_FUSED) return launch_istft_fused<NC, NC == 1024 ? 8 : 4>(sp, r, synth_window, tw, out, st);
            if constexpr (NC >= 256) return launch_istft_pw<NC>(sp, r, synth_window, tw, out, st);
            else return no_instance("k_istft_pw");
        });
    }
    // two-kernel path: irFFT + synthesis window into the workspace, then the overlap-add
    if (r.fam == FAM_POW2) {
        const float2* tw = nullptr;
        if (int e = get_twiddles(s->n_fft, &tw)) return e;
        if (int e = with_pow2(s->n_fft / 2, [&](auto nc) { return launch_irfft_fast<nc>(sp, g, synth_window, tw, frames, st); }))
            return e;
    } else if (r.fam == FAM_MR) {     // n_fft with a mixed-radix plan: one N-point inverse FFT per frame
        if (int e = launch_irfft_mr(sp, g, synth_window, frames, st)) return e;
    } else if (r.fam == FAM_BS) {     // even non-power-of-two n_fft: inverse chirp-z, then the gather
        if (int e = launch_irfft_bs(sp, g, synth_window, frames, st)) return e;
    } else if (r.fam == FAM_BIG) {    // 4096 / 8192: sub-FFT kernel, then the gather
        if (int e = launch_irfft_big(sp, g, synth_window, frames, st)) return e;
    } else if (r.fam == FAM_GEN) {    // small prime factors: run-time mixed-radix inverse FFT, then the gather
        if (int e = launch_irfft_gen<float>(sp, g, synth_window, frames, st)) return e;
    } else {
        const float* idft = nullptr;
        if (int e = get_dft_inv(s->n_fft, &idft)) return e;
        GemmArgs ga{};
        ga.in = frames_out_map(g, g.K);          // spectrum in the caller's layout (complex units)
        ga.out = frames_contig_map(g, g.win);
        ga.Kdim = 2 * g.K; ga.N = std::min(g.n_fft, g.win); ga.ldb = g.n_fft;
        ga.window = synth_window; ga.win = g.win;
        if (int e = run_gemm<A_CPLX, E_WINDOW>((const float*)spec, idft, ga, frames, st)) return e;
        if (g.win > g.n_fft) {
            hipLaunchKernelGGL(k_fill_cols, dim3(grid_1d(g.total_frames * (g.win - g.n_fft), 256)),
                               dim3(256), 0, st, frames, g.total_frames, (long long)g.win, g.n_fft,
                               g.win);
            if (int e = launch_check("k_fill_cols")) return e;
        }
    }
    return run_ola<float>(frames, s, n_frames, s->in_layout == KPR_CHANNELS_LAST, out, st);
}

// ---- kpr_istft_f64: the generic engine into the workspace, then the overlap-add ----
static int run_istft_f64(const void* spec, const kpr_stft_geom* s, int64_t n_frames, const double* synth_window, double* out,
                         void* workspace, int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = check_geom(s)) return e;
    if (n_frames < 0) return fail(KPR_E_BADARG, "negative frame count");
    Geom g = make_geom(s, n_frames);
    g.pad_left = 0;
    if (g.total_frames == 0) return 0;
    if (!spec || !synth_window || !out) return fail(KPR_E_BADARG, "spec / window / out must not be NULL");
    const int64_t need = istft_workspace_bytes<double>(s, n_frames);
    if (!workspace || workspace_bytes < need)
        return fail(KPR_E_WORKSPACE, "istft (float64) workspace: need %lld bytes", (long long)need);
    hipStream_t st = (hipStream_t)stream;
    double* frames = reinterpret_cast<double*>(workspace);
    if (int e = launch_irfft_gen<double>((const double2*)spec, g, synth_window, frames, st)) return e;
    return run_ola<double>(frames, s, n_frames, s->in_layout == KPR_CHANNELS_LAST && s->channels > 1, out, st);
}

}  // namespace kpr
