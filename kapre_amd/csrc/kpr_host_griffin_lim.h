// kpr_host_griffin_lim.h -- host side of Griffin-Lim (kpr_griffin_lim_kernels.h): the tiling, the argument checks and launches of
// the step and of the initial spectrum, the workspace layout, and the loop that chains them with the library's own inverse and
// forward transforms (run_istft_f32 / run_stft_f32: dispatch and results are those of kpr_istft_f32 / kpr_stft_f32).
// Part of the single translation unit kapre_hip.hip (included there after kpr_host_ops.h; not stand-alone).
#pragma once

namespace kpr {

static long long gl_chunks(long long item_size) { return (item_size + kGlChunk - 1) / kGlChunk; }

static size_t gl_align(size_t n) { return (n + 255) & ~(size_t)255; }

static size_t gl_part_bytes(int64_t n_items, int64_t item_size) {
    return gl_align((size_t)8 * (size_t)n_items * (size_t)gl_chunks(item_size));
}

// the projection step and, with sc_out, the convergence figure of every item (two launches)
static int run_gl_project(const void* R, const void* T, const float* mag, int64_t n_items, int64_t item_size, float c, void* S,
                          float* sc_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (n_items < 0 || item_size < 0) return fail(KPR_E_BADARG, "negative n_items / item_size");
    if (!(c >= 0.0f && c < 1.0f)) return fail(KPR_E_BADARG, "c = momentum / (1 + momentum) must lie in [0, 1), got %g", (double)c);
    if (T && c == 0.0f) T = nullptr;                                 // not read
    if (!T && c != 0.0f) return fail(KPR_E_BADARG, "T must not be NULL when c != 0");
    if (n_items == 0 || item_size == 0) return 0;
    if (!R || !mag || !S) return fail(KPR_E_BADARG, "R / mag / S must not be NULL");
    if (item_size > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "item_size = %lld elements: 2^31 or more is not supported", (long long)item_size);
    const long long chunks = gl_chunks(item_size);
    if (n_items * chunks > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "too many items (%lld chunks)", (long long)(n_items * chunks));
    if ((((uintptr_t)R) | ((uintptr_t)T) | ((uintptr_t)S)) & 7) return fail(KPR_E_BADARG, "R / T / S must be 8-byte aligned");
    if ((((uintptr_t)mag) | ((uintptr_t)sc_out)) & 3) return fail(KPR_E_BADARG, "mag / sc_out must be 4-byte aligned");
    const size_t n = (size_t)n_items * (size_t)item_size;
    if (ranges_overlap(S, n * 8, R, n * 8) || ranges_overlap(S, n * 8, T, n * 8) || ranges_overlap(S, n * 8, mag, n * 4))
        return fail(KPR_E_BADARG, "S overlaps an input (there is no in-place form)");
    float* part = nullptr;
    if (sc_out) {
        const size_t need = (size_t)8 * (size_t)n_items * (size_t)chunks;
        if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
            return fail(KPR_E_WORKSPACE, "projection workspace: %zu bytes needed (8 per item and chunk, 8-byte aligned), got %zu", need,
                        workspace ? workspace_bytes : (size_t)0);
        if (ranges_overlap(workspace, need, S, n * 8) || ranges_overlap(workspace, need, R, n * 8) || ranges_overlap(workspace, need, T, n * 8) ||
            ranges_overlap(workspace, need, mag, n * 4) || ranges_overlap(sc_out, (size_t)n_items * 4, S, n * 8))
            return fail(KPR_E_BADARG, "the workspace or sc_out overlaps another argument");
        part = (float*)workspace;
    }
    const bool v4 = ((((uintptr_t)R) | ((uintptr_t)T) | ((uintptr_t)S) | ((uintptr_t)mag)) & 15) == 0;
    const dim3 grid((unsigned)(n_items * chunks)), block(256);
    const float2 *r = (const float2*)R, *t = (const float2*)T;
    with_vec<4>(v4, [&](auto v) {
        if (T) hipLaunchKernelGGL((k_gl_project<v, true>), grid, block, 0, st, r, t, mag, (long long)item_size, (int)chunks, c, (float2*)S, part);
        else hipLaunchKernelGGL((k_gl_project<v, false>), grid, block, 0, st, r, t, mag, (long long)item_size, (int)chunks, c, (float2*)S, part);
    });
    if (int e = launch_check("k_gl_project", v4 ? 4 : 1, T ? "mom" : "plain")) return e;
    if (!sc_out) return 0;
    hipLaunchKernelGGL(k_gl_finish, dim3((unsigned)n_items), dim3(64), 0, st, (const float*)part, (int)chunks, sc_out);
    return launch_check("k_gl_finish");
}

// mag = M^(1/power) into mag_out (NULL: power == 1) and S_0 into S (NULL: mag only); init_mode 0: zero phase, 1: random
static int run_gl_init(const float* M, int64_t batch, int channels, int64_t plane, int layout, double power, int init_mode,
                       void* rng_state, float* mag_out, void* S, hipStream_t st) {
    if (batch < 0 || channels <= 0 || plane < 0 || (unsigned)layout > 1u) return fail(KPR_E_BADARG, "bad batch/channels/plane/layout");
    if (!(power > 0.0) || !std::isfinite(power)) return fail(KPR_E_BADARG, "power must be positive and finite, got %g", power);
    if (init_mode != 0 && init_mode != 1) return fail(KPR_E_BADARG, "init_mode must be 0 (zero phase) or 1 (random), got %d", init_mode);
    if (init_mode == 1 && S && (!rng_state || ((uintptr_t)rng_state & 7))) return fail(KPR_E_BADARG, "rng_state must be an 8-byte aligned pointer");
    if ((power != 1.0) != (mag_out != nullptr)) return fail(KPR_E_BADARG, "mag_out goes with power != 1 (with power == 1 M is the magnitude)");
    const long long n = (long long)batch * channels * plane;
    if (n == 0) return 0;
    if (!M || (!S && !mag_out)) return fail(KPR_E_BADARG, "M and one of mag_out / S must not be NULL");
    if ((((uintptr_t)M) | ((uintptr_t)mag_out)) & 3 || ((uintptr_t)S & 7)) return fail(KPR_E_BADARG, "M / mag_out must be 4-byte, S 8-byte aligned");
    if (ranges_overlap(S, (size_t)n * 8, M, (size_t)n * 4) || ranges_overlap(mag_out, (size_t)n * 4, M, (size_t)n * 4) ||
        ranges_overlap(S, (size_t)n * 8, mag_out, (size_t)n * 4))
        return fail(KPR_E_BADARG, "M, mag_out and S must not overlap");
    GlInitArgs a;
    a.M = M; a.mag = mag_out; a.S = (float2*)S; a.state = (const unsigned long long*)rng_state;
    a.n = n; a.plane = plane;
    a.C = (layout == KPR_CHANNELS_LAST && channels > 1) ? channels : 1;
    a.inv_power = (float)(1.0 / power);
    const bool v4 = ((((uintptr_t)M) | ((uintptr_t)mag_out) | ((uintptr_t)S)) & 15) == 0;
    const bool rnd = init_mode == 1 && S;
    const dim3 grid(grid_1d(v4 ? (n + 3) / 4 : n, 256, 1 << 16)), block(256);
    with_vec<4>(v4, [&](auto v) {
        if (rnd) hipLaunchKernelGGL((k_gl_init<v, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_gl_init<v, false>), grid, block, 0, st, a);
    });
    if (int e = launch_check("k_gl_init", v4 ? 4 : 1, rnd ? "rand" : "zero")) return e;
    if (!rnd) return 0;
    hipLaunchKernelGGL(k_gl_advance, dim3(1), dim3(64), 0, st, (unsigned long long*)rng_state);
    return launch_check("k_gl_advance");
}

// the workspace of kpr_griffin_lim_f32: | S | R/T (one, or two with momentum) | mag (power != 1) | chunk sums | istft | stft |
struct GlLayout {
    size_t spec, mag, part, istft, stft, total;
    int n_spec;
};

static int gl_layout(const kpr_stft_geom* g, int64_t n_frames, bool with_momentum, bool with_power, kpr_stft_geom* fwd, GlLayout* l) {
    if (int e = check_geom(g)) return e;
    if (n_frames < 0) return fail(KPR_E_BADARG, "negative frame count");
    if (g->pad_begin || g->pad_end) return fail(KPR_E_BADARG, "Griffin-Lim frames without padding: pad_begin and pad_end must be 0");
    *fwd = *g;
    fwd->time = n_frames > 0 ? (n_frames - 1) * (int64_t)g->hop_length + g->win_length : 0;
    if (int e = check_geom(fwd)) return e;
    const size_t n = (size_t)g->batch * g->channels * (size_t)n_frames * (size_t)(g->n_fft / 2 + 1);
    l->n_spec = with_momentum ? 3 : 2;
    l->spec = gl_align(n * 8);
    l->mag = with_power ? gl_align(n * 4) : 0;
    l->part = gl_part_bytes(g->batch, (int64_t)(n / (size_t)std::max<int64_t>(g->batch, 1)));
    const int64_t wi = istft_workspace_bytes<float>(g, n_frames), wf = stft_workspace_bytes(fwd, KPR_OUT_COMPLEX);
    if (wi < 0 || wf < 0) return KPR_E_BADARG;
    l->istft = gl_align((size_t)wi);
    l->stft = gl_align((size_t)wf);
    l->total = l->n_spec * l->spec + l->mag + l->part + l->istft + l->stft;
    return 0;
}

static int run_griffin_lim(const float* M, const kpr_stft_geom* g, int64_t n_frames, const float* window, const float* synth_window,
                           int n_iter, double momentum, double power, int init_mode, const void* init, void* rng_state,
                           float* wave_out, float* sc_out, void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    if (n_iter < 0) return fail(KPR_E_BADARG, "n_iter must not be negative, got %d", n_iter);
    if (!(momentum >= 0.0 && momentum < 1.0)) return fail(KPR_E_BADARG, "momentum must lie in [0, 1), got %g", momentum);
    if (!(power > 0.0) || !std::isfinite(power)) return fail(KPR_E_BADARG, "power must be positive and finite, got %g", power);
    if (init_mode < 0 || init_mode > 2) return fail(KPR_E_BADARG, "init_mode must be 0 (zero phase), 1 (random) or 2 (given), got %d", init_mode);
    const bool mom = momentum != 0.0, pw = power != 1.0;
    kpr_stft_geom fwd;
    GlLayout l;
    if (int e = gl_layout(g, n_frames, mom, pw, &fwd, &l)) return e;
    const int K = g->n_fft / 2 + 1;
    const int64_t item = (int64_t)g->channels * n_frames * K;
    if (g->batch == 0 || item == 0) return 0;
    if (!M || !window || !synth_window || !wave_out) return fail(KPR_E_BADARG, "mag / window / synth_window / wave_out must not be NULL");
    if (init_mode == 2 && (!init || ((uintptr_t)init & 7))) return fail(KPR_E_BADARG, "init_mode 2 needs an 8-byte aligned complex64 init");
    if (init_mode == 1 && !rng_state) return fail(KPR_E_BADARG, "init_mode 1 needs rng_state");
    if (!workspace || workspace_bytes < l.total || ((uintptr_t)workspace & 15))
        return fail(KPR_E_WORKSPACE, "griffin-lim workspace: %zu bytes needed (kpr_griffin_lim_workspace_bytes, 16-byte aligned), got %zu",
                    l.total, workspace ? workspace_bytes : (size_t)0);
    const hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    void* S = w;                        w += l.spec;
    void* B[2] = {w, nullptr};          w += l.spec;
    if (mom) { B[1] = w;                w += l.spec; }
    float* magw = pw ? (float*)w : nullptr;   w += l.mag;
    void* part = w;                     w += l.part;
    void* wsi = w;                      w += l.istft;
    void* wsf = w;
    const float* mag = pw ? magw : M;
    const float c = (float)(momentum / (1.0 + momentum));

    // S_0 (and mag): one launch; a given S_0 is read where it is
    if (init_mode != 2 || pw)
        if (int e = run_gl_init(M, g->batch, g->channels, (int64_t)n_frames * K, g->out_layout, power, init_mode == 1 ? 1 : 0, rng_state,
                                magw, init_mode == 2 ? nullptr : S, st))
            return e;
    const void* cur = init_mode == 2 ? init : S;
    for (int n = 1; n <= n_iter; ++n) {
        void* R = B[mom ? (n - 1) & 1 : 0];
        const void* T = (mom && n > 1) ? B[n & 1] : nullptr;         // T_0 = 0: the first step is the plain one; afterwards T_n = R_n
        if (int e = run_istft_f32(cur, g, n_frames, synth_window, wave_out, wsi, (int64_t)l.istft, stream)) return e;
        if (int e = run_stft_f32(wave_out, &fwd, window, R, KPR_OUT_COMPLEX, wsf, (int64_t)l.stft, stream)) return e;
        if (int e = run_gl_project(R, T, mag, g->batch, item, T ? c : 0.0f, S, sc_out ? sc_out + (size_t)(n - 1) * g->batch : nullptr,
                                   part, l.part, st))
            return e;
        cur = S;
    }
    return run_istft_f32(cur, g, n_frames, synth_window, wave_out, wsi, (int64_t)l.istft, stream);
}

}  // namespace kpr
