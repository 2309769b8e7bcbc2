// kpr_host_yin.h -- host side of the YIN pitch tracker (kpr_yin_kernels.h): the plan (frames per workgroup run, the form), the
// argument checks and the one launch.  Option "yin_variant": 0 automatic, 1 the direct form for every shape.
// Part of the single translation unit kapre_hip.hip (after kpr_host_ops.h: frame_count; not stand-alone).
#pragma once

namespace kpr {

struct YinPlan {
    int form;                           // KPR_YIN_DIRECT / KPR_YIN_SHARED
    int F, nb, Q, LP, span;             // YinArgs' fields of the same names
    size_t lds;
};

// The limits of the definition (include/kapre_hip.h), then the largest run whose span, sum rows and y rows fit the LDS budget:
// the shared form where hop divides W into 2 ... kYinMaxBlocks blocks and a run of at least two frames fits, else the direct form.
static int yin_plan(int frame_length, int W, int hop, int tau_min, int tau_hi, YinPlan* p) {
    if (frame_length < 1 || frame_length > 4096) return fail(KPR_E_BADARG, "yin: frame_length must lie in 1 ... 4096, got %d", frame_length);
    if (W < 2 || W > frame_length - 3)
        return fail(KPR_E_BADARG, "yin: win_length must lie in 2 ... frame_length - 3 = %d, got %d", frame_length - 3, W);
    if (hop < 1) return fail(KPR_E_BADARG, "yin: hop must be at least 1, got %d", hop);
    if (tau_min < 1 || tau_hi > frame_length - W - 1 || tau_hi - tau_min < 2)
        return fail(KPR_E_BADARG, "yin: lags %d ... %d: tau_min >= 1, tau_hi <= frame_length - win_length - 1 = %d and at least "
                    "three lags are required", tau_min, tau_hi, frame_length - W - 1);
    const int nl = tau_hi + 1;
    p->LP = (nl + 63) / 64 * 64;
    p->Q = (nl + kYinR - 1) / kYinR;
    p->nb = W % hop == 0 ? W / hop : 0;
    auto span_of = [&](int F) -> long long { return ((long long)(F - 1) * hop + W + tau_hi + 16 + 3) / 4 * 4; };
    auto floats_of = [&](int F, bool shared) -> long long {
        return span_of(F) + (long long)(shared ? F - 1 + p->nb + kYinWaves : F) * p->LP;
    };
    p->form = KPR_YIN_DIRECT;
    p->F = 1;
    bool found = false;
    if (opt(OPT_YIN_VARIANT) != 1 && p->nb >= 2 && p->nb <= kYinMaxBlocks)
        for (int F = kYinMaxRun; F >= 2 && !found; --F)
            if (floats_of(F, true) <= kYinLdsFloats) { p->form = KPR_YIN_SHARED; p->F = F; found = true; }
    for (int F = kYinMaxRun; F >= 1 && !found; --F)
        if (floats_of(F, false) <= kYinLdsFloats) { p->F = F; found = true; }
    // (F = 1 always fits: at most 4096 + 16 staged floats and one row of 4096)
    const bool shared = p->form == KPR_YIN_SHARED;
    if (!shared) p->nb = 0;
    p->span = (int)span_of(p->F);
    p->lds = (size_t)floats_of(p->F, shared) * sizeof(float);
    return 0;
}

static int run_yin(const float* x, int64_t batch, int channels, int64_t time, int layout, double sample_rate, int frame_length,
                   int win_length, int hop, int tau_min, int tau_hi, double trough_threshold, int pad_end, float* f0, float* cmnd,
                   float* curve, kpr_stream_t stream) {
    if (int e = check_series("yin: bad batch/channels/time/layout", batch, channels, time, layout, true)) return e;
    const float sr = (float)sample_rate, thr = (float)trough_threshold;
    if (!(sr > 0.0f) || !std::isfinite(sr)) return fail(KPR_E_BADARG, "yin: the sample rate must be positive and finite, got %g", sample_rate);
    if (!(thr > 0.0f)) return fail(KPR_E_BADARG, "yin: trough_threshold must be positive, got %g", trough_threshold);
    YinPlan p;
    if (int e = yin_plan(frame_length, win_length, hop, tau_min, tau_hi, &p)) return e;
    if (int e = check_reach("yin", time, 1, 31)) return e;
    const int64_t frames = frame_count(time, frame_length, hop, pad_end);
    if (batch == 0 || channels == 0 || frames <= 0) return 0;
    const int nl = tau_hi + 1;
    const Series sx = series_of(layout, channels, time, true), so = series_of(layout, channels, frames, true);
    const uintptr_t nx = (uintptr_t)batch * sx.item * 4, no = (uintptr_t)batch * so.item * 4;
    if (int e = check_ptrs("yin: ", {{"x", x, nx, 4, false, false}, {"f0", f0, no, 4, false, true}, {"cmnd", cmnd, no, 4, false, true},
                                     {"curve", curve, no * nl, 4, true, true}}))
        return e;
    const long long runs = (frames + p.F - 1) / p.F;
    long long grid;
    if (int e = grid_of(runs, batch, channels, "yin", &grid)) return e;
    YinArgs a;
    a.x = x; a.f0 = f0; a.cmnd = cmnd; a.curve = curve;
    a.item = sx.item; a.chan = sx.chan; a.stride = sx.stride;
    a.out_item = so.item; a.out_chan = so.chan; a.out_stride = so.stride;
    a.C = channels; a.time = (int)time; a.frames = (int)frames; a.runs = (int)runs; a.F = p.F;
    a.W = win_length; a.hop = hop; a.tau_min = tau_min; a.tau_hi = tau_hi;
    a.nb = p.nb; a.Q = p.Q; a.LP = p.LP; a.span = p.span;
    a.thr = thr; a.sr = sr;
    const bool shared = p.form == KPR_YIN_SHARED, vec = hop % 4 == 0;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_yin<%s,v%d>: grid %lld, lds %zu B, runs of %d frames, %d lags in %d blocks, span %d\n",
                shared ? "shared" : "direct", vec ? 4 : 1, grid, p.lds, p.F, nl, p.Q, p.span);
    const dim3 g((unsigned)grid), blk(kYinThreads);
    const hipStream_t st = (hipStream_t)stream;
    if (shared && vec) hipLaunchKernelGGL((k_yin<true, true>), g, blk, p.lds, st, a);
    else if (shared) hipLaunchKernelGGL((k_yin<true, false>), g, blk, p.lds, st, a);
    else if (vec) hipLaunchKernelGGL((k_yin<false, true>), g, blk, p.lds, st, a);
    else hipLaunchKernelGGL((k_yin<false, false>), g, blk, p.lds, st, a);
    return launch_check(shared ? (vec ? "k_yin<shared,v4>" : "k_yin<shared,v1>") : (vec ? "k_yin<direct,v4>" : "k_yin<direct,v1>"));
}

}  // namespace kpr
