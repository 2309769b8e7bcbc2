// kpr_host_mdct.h -- host side of the MDCT and its inverse (kpr_mdct_kernels.h): the plan (frames or blocks per wave run), the
// twiddle tables, the argument checks and the one launch of each.  Option "mdct_run": 0 automatic, n = at most n frames (forward)
// or output blocks (inverse) per run.
// Part of the single translation unit kapre_hip.hip (after kpr_host_ops.h: frame_count; not stand-alone).
#pragma once

namespace kpr {

struct MdctPlan {
    int NC, L, G, R;                    // FFT points, lanes per frame, frames per wave step, frames / blocks per run
};

static int mdct_plan(int frame_length, MdctPlan* p) {
    if (frame_length != 512 && frame_length != 1024 && frame_length != 2048 && frame_length != 4096)
        return fail(KPR_E_UNSUPPORTED, "mdct: frame_length must be 512, 1024, 2048 or 4096, got %d", frame_length);
    p->NC = frame_length / 4;
    p->L = p->NC / kPts;
    p->G = 64 / p->L;
    // automatic: eight wave steps and at least 16 frames -- the inverse's one redundant frame per run stays under 1/16 of its work
    p->R = opt(OPT_MDCT_RUN) > 0 ? opt(OPT_MDCT_RUN) : std::max(16, 8 * p->G);
    return 0;
}

// The scale of a call.  norm 0: the forward transform carries s = 2 and the inverse s' = 1 / M (tf.signal); norm 1 ('ortho'): both
// sqrt(2 / M).  adjoint swaps the two, which makes each entry point the other's transpose.
enum { MDCT_SCALE_TWO, MDCT_SCALE_INV_M, MDCT_SCALE_ORTHO };
static int mdct_scale_kind(bool inverse, int norm, int adjoint) {
    if (norm) return MDCT_SCALE_ORTHO;
    return (inverse != (adjoint != 0)) ? MDCT_SCALE_INV_M : MDCT_SCALE_TWO;
}

// pre[n] = exp(-i pi (4n + 1) / (4M)), then post[k] = scale exp(-i pi k / M), n, k < NC; key = frame_length + 65536 kind
static std::map<std::pair<int, int>, float2*> g_mdct_tab;
static void build_mdct_table(int key, std::vector<float2>& h) {
    const int N = key & 0xffff, kind = key >> 16, M = N / 2, NC = N / 4;
    const double scale = kind == MDCT_SCALE_TWO ? 2.0 : kind == MDCT_SCALE_INV_M ? 1.0 / M : std::sqrt(2.0 / M);
    h.resize(2 * NC);
    for (int n = 0; n < NC; ++n) {
        const double a = -M_PI * (4.0 * n + 1.0) / (4.0 * M), b = -M_PI * n / M;
        h[n] = make_float2((float)std::cos(a), (float)std::sin(a));
        h[NC + n] = make_float2((float)(scale * std::cos(b)), (float)(scale * std::sin(b)));
    }
}

template <int NC>
static int launch_mdct(bool inverse, bool cl, const MdctArgs& a, unsigned grid, hipStream_t st) {
    const size_t lds = mdct_lds_bytes(NC, inverse);
    static LdsOptIn opt_in[4];
    auto go = [&](auto kern, LdsOptIn& oi, const char* name, const char* detail) -> int {
        if (int e = allow_big_lds(oi, reinterpret_cast<const void*>(kern))) return e;
        if (opt(OPT_VERBOSE))
            fprintf(stderr, "[kapre_hip] %s<%d,%s>: grid %u, lds %zu B, runs of %d, %d per series\n", name, NC, detail, grid, lds, a.R, a.runs);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kMdctWaves), lds, st, a);
        return launch_check(name, NC, detail);
    };
    if (!inverse) return cl ? go(&k_mdct<NC, true>, opt_in[0], "k_mdct", "cl") : go(&k_mdct<NC, false>, opt_in[1], "k_mdct", "cf");
    return cl ? go(&k_imdct<NC, true>, opt_in[2], "k_imdct", "cl") : go(&k_imdct<NC, false>, opt_in[3], "k_imdct", "cf");
}

// Both directions.  wave: the waveform (forward: read, inverse: written) of wave_len samples per series in wave_layout; coef: the
// coefficients, n_frames rows of M per series in coef_layout.
static int run_mdct(bool inverse, const float* in, float* out, int64_t batch, int channels, int64_t wave_len, int wave_layout,
                    int64_t n_frames, int coef_layout, int frame_length, const float* window, int norm, int adjoint, int pad_begin,
                    kpr_stream_t stream) {
    const char* op = inverse ? "imdct" : "mdct";
    const std::string pre = std::string(op) + ": ";
    MdctPlan p;
    if (int e = mdct_plan(frame_length, &p)) return e;
    if ((unsigned)norm > 1u || (unsigned)adjoint > 1u || (unsigned)pad_begin > 1u)
        return fail(KPR_E_BADARG, "%s: norm, adjoint and pad_begin are 0 or 1", op);
    const int N = frame_length, M = N / 2;
    if (int e = check_reach(op, wave_len, 1, 31)) return e;
    if (n_frames > 0x7fffffffLL / M) return fail(KPR_E_UNSUPPORTED, "%s: %lld frames of %d coefficients: 2^31 or more per series are not supported", op, (long long)n_frames, M);
    // one channel in channels_last is the channels_first image
    const Series sw = series_of(wave_layout, channels, wave_len, true);
    const bool ccl = coef_layout == KPR_CHANNELS_LAST && channels > 1;
    const uintptr_t nw = (uintptr_t)batch * sw.item * 4, nc = (uintptr_t)batch * channels * (uintptr_t)n_frames * M * 4;
    const int pad = pad_begin ? M : 0;
    // what the launch has to cover: the forward transform's frames, the inverse's output blocks
    const long long units_of_work = inverse ? (wave_len + pad + M - 1) / M : n_frames;
    if (batch == 0 || channels == 0 || units_of_work <= 0) return 0;
    if (int e = check_ptrs(pre.c_str(), {{inverse ? "X" : "x", in, inverse ? nc : nw, 4, inverse && n_frames == 0, false},
                                         {"window", window, (uintptr_t)N * 4, 4, false, false},
                                         {"out", out, inverse ? nw : nc, 4, false, true}}))
        return e;
    const long long runs = (units_of_work + p.R - 1) / p.R, units = (runs + kMdctWaves - 1) / kMdctWaves;
    long long grid;
    if (int e = grid_of(units, batch, channels, op, &grid)) return e;
    MdctArgs a;
    a.in = in; a.out = out; a.window = window;
    if (int e = get_twiddles(2 * p.NC, &a.fft_tw)) return e;
    if (int e = cached_table(g_mdct_tab, N + 65536 * mdct_scale_kind(inverse, norm, adjoint), build_mdct_table, &a.tab)) return e;
    a.item = sw.item; a.chan = sw.chan; a.stride = sw.stride;
    a.c_item = (long long)channels * n_frames * M;
    a.c_chan = ccl ? 1 : n_frames * M;
    a.c_frame = ccl ? (long long)M * channels : M;
    a.c_k = ccl ? channels : 1;
    a.C = channels; a.len = (int)wave_len; a.frames = (int)n_frames;
    a.R = p.R; a.runs = (int)runs; a.units = (int)units; a.pad = pad;
    return with_pow2(p.NC, [&](auto nc_c) { return launch_mdct<decltype(nc_c)::value>(inverse, ccl, a, (unsigned)grid, (hipStream_t)stream); });
}

static int run_mdct_fwd(const float* x, int64_t batch, int channels, int64_t time, int layout, int frame_length, const float* window,
                        int norm, int adjoint, int pad_begin, int pad_end, int out_layout, float* out, kpr_stream_t stream) {
    if (int e = check_series("mdct: bad batch/channels/time/layout", batch, channels, time, layout | out_layout, true)) return e;
    MdctPlan p;
    if (int e = mdct_plan(frame_length, &p)) return e;
    if ((unsigned)pad_begin > 1u || (unsigned)pad_end > 1u) return fail(KPR_E_BADARG, "mdct: pad_begin and pad_end are 0 or 1");
    if (int e = check_reach("mdct", time, 1, 31)) return e;
    const int64_t frames = frame_count(time + (pad_begin ? frame_length / 2 : 0), frame_length, frame_length / 2, pad_end);
    return run_mdct(false, x, out, batch, channels, time, layout, frames, out_layout, frame_length, window, norm, adjoint, pad_begin, stream);
}

static int run_mdct_inv(const float* X, int64_t batch, int channels, int64_t n_frames, int layout, int frame_length, const float* window,
                        int norm, int adjoint, int pad_begin, int64_t out_len, int out_layout, float* out, kpr_stream_t stream) {
    if (int e = check_series("imdct: bad batch/channels/n_frames/layout", batch, channels, n_frames, layout | out_layout, true)) return e;
    if (out_len < 0) return fail(KPR_E_BADARG, "imdct: out_len must not be negative, got %lld", (long long)out_len);
    return run_mdct(true, X, out, batch, channels, out_len, out_layout, n_frames, layout, frame_length, window, norm, adjoint, pad_begin, stream);
}

}  // namespace kpr
