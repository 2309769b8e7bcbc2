// kpr_host_resample.h -- host side of the two resamplers (kpr_resample_kernels.h, kpr_resample_direct_kernels.h): the windowed-sinc
// table of the polyphase form (host only: kpr_resample_table) and its tile plan, the window and tile of the table-free form, the
// argument checks and the one launch of each.
// Part of the single translation unit kapre_hip.hip (included there after kpr_host_ops.h; not stand-alone).
#pragma once

namespace kpr {

// ---- Resample (kpr_resample_kernels.h): the windowed-sinc tables of both directions, the tile plan, the launch ----
// h(tau) = (base / orig) sinc(base tau) cos^2(pi base tau / (2 L)) for |base tau| < L, base = rolloff min(orig, new), with
// orig, new reduced by their gcd.  Output phase p of P reads the inputs (block) Q + j with u = j P - p Q:
// tau = +-u / (orig new) -- h is even, so the forward pass ((P, Q) = (new, orig)) and the adjoint ((orig, new)) are this one
// construction -- and base tau = rolloff u / max(orig, new).  first[p] is the smallest j with |u| < U = L max / rolloff,
// n_taps the largest support of a phase; first[] rises with p by at most ceil(Q / P) + 1 a step.
struct ResampleShape {
    int P, Q, n_taps;
    int orig, fnew, L;
    double rolloff, U;
};

static int resample_shape(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint, ResampleShape* r) {
    if (orig_freq <= 0 || new_freq <= 0)
        return fail(KPR_E_BADARG, "orig_freq and new_freq must be positive, got %d and %d", orig_freq, new_freq);
    if (lowpass_filter_width < 1) return fail(KPR_E_BADARG, "lowpass_filter_width must be at least 1, got %d", lowpass_filter_width);
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return fail(KPR_E_BADARG, "rolloff must lie in (0, 1], got %g", rolloff);
    int a = orig_freq, b = new_freq;
    while (b) { const int t = a % b; a = b; b = t; }
    r->orig = orig_freq / a;
    r->fnew = new_freq / a;
    r->L = lowpass_filter_width;
    r->rolloff = rolloff;
    r->P = adjoint ? r->orig : r->fnew;
    r->Q = adjoint ? r->fnew : r->orig;
    r->U = (double)lowpass_filter_width * (double)std::max(r->orig, r->fnew) / rolloff;
    // (the size before the walk over the phases: a support holds at most 2 U / P + 1 inputs)
    const double est = 2.0 * r->U / (double)r->P + 1.0;
    if (est > 132.0 || (double)r->P * est * 4.0 > 2.0 * 1048576.0)
        return fail(KPR_E_UNSUPPORTED, "resample %d -> %d%s: a table of %d phases x about %.0f taps = %.0f bytes; supported are at most 128 "
                    "taps and 1 MiB (1048576 bytes)", orig_freq, new_freq, adjoint ? " (adjoint)" : "", r->P, est, (double)r->P * est * 4.0);
    return 0;
}

// [lo, hi]: the j with |j P - p Q| < U
static void resample_support(const ResampleShape& r, int p, long long* lo, long long* hi) {
    const long long pq = (long long)p * r.Q;
    long long a = (long long)std::floor(((double)pq - r.U) / (double)r.P) + 1;
    while ((double)(a * r.P - pq) <= -r.U) ++a;
    while ((double)((a - 1) * r.P - pq) > -r.U) --a;
    long long b = (long long)std::ceil(((double)pq + r.U) / (double)r.P) - 1;
    while ((double)(b * r.P - pq) >= r.U) --b;
    while ((double)((b + 1) * r.P - pq) < r.U) ++b;
    *lo = a;
    *hi = b;
}

static int resample_taps(const ResampleShape& r) {
    long long n = 1;
    for (int p = 0; p < r.P; ++p) {
        long long lo, hi;
        resample_support(r, p, &lo, &hi);
        n = std::max(n, hi - lo + 1);
    }
    return (int)n;
}

static int resample_size(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint, ResampleShape* r) {
    if (int e = resample_shape(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint, r)) return e;
    r->n_taps = resample_taps(*r);
    const long long bytes = (long long)r->P * r->n_taps * 4;
    if (r->n_taps > 128 || bytes > 1048576)
        return fail(KPR_E_UNSUPPORTED, "resample %d -> %d%s: a table of %d phases x %d taps = %lld bytes; supported are at most 128 taps "
                    "and 1 MiB (1048576 bytes)", orig_freq, new_freq, adjoint ? " (adjoint)" : "", r->P, r->n_taps, bytes);
    return 0;
}

// kpr_resample_table: table_host[P][n_taps] and first_host[P] of the construction above (host only)
static int resample_table(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint, float* table_host,
                          int32_t* first_host) {
    ResampleShape r;
    if (!table_host || !first_host) return fail(KPR_E_BADARG, "table_host / first_host must not be NULL");
    if (int e = resample_size(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint, &r)) return e;
    const double scale = r.rolloff * (double)std::min(r.orig, r.fnew) / (double)r.orig;
    const double per_u = r.rolloff / (double)std::max(r.orig, r.fnew);
    for (int p = 0; p < r.P; ++p) {
        long long lo, hi;
        resample_support(r, p, &lo, &hi);
        first_host[p] = (int32_t)lo;
        for (int k = 0; k < r.n_taps; ++k) {
            const long long j = lo + k;
            double v = 0.0;
            if (j <= hi) {
                const double t = (double)(j * r.P - (long long)p * r.Q) * per_u;     // base tau
                const double c = std::cos(M_PI * t / (2.0 * r.L));
                v = scale * (t == 0.0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t)) * c * c;
            }
            table_host[(size_t)p * r.n_taps + k] = (float)v;
        }
    }
    return 0;
}

// the tile of the dispatch: `pt` phases x `nb` blocks per workgroup, work items of 8 blocks `ng` apart (kpr_resample_kernels.h).
// The staged span of a tile is at most (nb - 1) Q + (first[p0 + pt - 1] - first[p0]) + n_taps words per channel; the plan holds
// for both channel counts of the kernel, so kpr_resample_plan needs no layout.
struct ResamplePlan {
    int pt, n_pt, ng, nb, span, threads;
};

static ResamplePlan resample_plan(int P, int Q, int n_taps) {
    auto span_of = [&](int pt, int nb) -> long long {
        return (long long)(nb - 1) * Q + ((long long)(pt - 1) * Q) / P + 2 + n_taps;
    };
    // lanes at work in the rounds of `threads` work items
    auto best_threads = [](long long items, int* threads) -> double {
        double best = -1.0;
        for (int t = 128; t <= kRsMaxThreads; t += 64) {
            const double eff = (double)items / (double)((items + t - 1) / t * t);
            if (eff > best + 1e-9) { best = eff; *threads = t; }
        }
        return best;
    };
    ResamplePlan pl;
    pl.n_pt = (P + 1023) / 1024;
    pl.pt = (P + pl.n_pt - 1) / pl.n_pt;
    pl.ng = 0;
    double best = -1.0;
    for (int ng = 1; ng <= 1024; ++ng) {
        const long long items = (long long)pl.pt * ng, outputs = items * kRsBlocks;
        if (span_of(pl.pt, kRsBlocks * ng) > kRsLdsWords || (ng > 1 && outputs > 16384)) break;
        int threads = 0;
        double score = best_threads(items, &threads);
        if (outputs < 2048) score *= (double)outputs / 2048.0;        // a small tile only when nothing larger fits
        if (score > best + 1e-9) { best = score; pl.ng = ng; pl.threads = threads; }
    }
    if (pl.ng) {
        pl.nb = kRsBlocks * pl.ng;
    } else {                                     // a long step: fewer than eight blocks, then fewer phases
        pl.ng = 1;
        pl.nb = kRsBlocks - 1;
        while (pl.nb > 1 && span_of(pl.pt, pl.nb) > kRsLdsWords) --pl.nb;
        while (pl.pt > 1 && span_of(pl.pt, pl.nb) > kRsLdsWords) pl.pt = (pl.pt + 1) / 2;
        pl.n_pt = (P + pl.pt - 1) / pl.pt;
        best_threads(pl.pt, &pl.threads);
    }
    pl.span = (int)span_of(pl.pt, pl.nb);
    return pl;
}

static int resample_dims(int n_phases, int n_taps, int step) {
    if (n_phases < 1 || n_taps < 1 || step < 1) return fail(KPR_E_BADARG, "bad n_phases/n_taps/step (%d, %d, %d)", n_phases, n_taps, step);
    if (n_taps > 128 || (long long)n_phases * n_taps * 4 > 1048576)
        return fail(KPR_E_UNSUPPORTED, "a resample table of %d phases x %d taps = %lld bytes; supported are at most 128 taps and 1 MiB",
                    n_phases, n_taps, (long long)n_phases * n_taps * 4);
    if (step > 16 * 1048576) return fail(KPR_E_UNSUPPORTED, "a resample step of %d inputs per block is not supported", step);
    return 0;
}

static int run_resample(const float* x, int64_t batch, int channels, int64_t in_len, int layout, const float* table, const int32_t* first,
                        int n_phases, int n_taps, int step, int64_t out_len, float* out, kpr_stream_t stream) {
    if (int e = check_series("bad batch/channels/in_len/out_len/layout", batch, channels, std::min(in_len, out_len), layout, false)) return e;
    if (int e = resample_dims(n_phases, n_taps, step)) return e;
    const Series si = series_of(layout, channels, in_len, false), so = series_of(layout, channels, out_len, false);
    if (int e = check_reach("resample", std::max(in_len, out_len), si.stride, 30)) return e;
    if (batch == 0 || out_len == 0) return 0;
    // (the table and first[] in a list of their own: their sizes are not arguments, so they have never been compared with out)
    if (int e = check_ptrs("", {{"x", x, (uintptr_t)batch * si.item * 4, 4, in_len == 0, false},
                                {"out", out, (uintptr_t)batch * so.item * 4, 4, false, true}}))
        return e;
    if (int e = check_ptrs("", {{"table_dev", table, 0, 4, false, false}, {"first_dev", first, 0, 4, false, false}})) return e;
    const ResamplePlan pl = resample_plan(n_phases, step, n_taps);
    const long long n_blocks = (out_len + n_phases - 1) / n_phases;
    if (n_blocks * step >= (1LL << 31) - (1LL << 26))
        return fail(KPR_E_UNSUPPORTED, "resample: %lld outputs at %d inputs per %d outputs reach past 2^31 input samples", (long long)out_len,
                    step, n_phases);
    const int nch = layout == KPR_CHANNELS_LAST && channels % 2 == 0 ? 2 : 1;      // a pair of interleaved channels is one series
    ResampleArgs a;
    a.x = x; a.out = out; a.tab = table; a.first = first;
    a.P = n_phases; a.Q = step; a.n_taps = n_taps;
    a.in_len = (int)in_len; a.out_len = (int)out_len;
    a.stride = si.stride;
    a.groups = channels / nch;
    a.in_item = si.item; a.out_item = so.item;
    a.in_chan = si.chan * nch; a.out_chan = so.chan * nch;
    a.pt = pl.pt; a.n_pt = pl.n_pt; a.ng = pl.ng; a.nb = pl.nb;
    a.n_blocks = (int)n_blocks;
    const long long tiles = (long long)pl.n_pt * ((n_blocks + pl.nb - 1) / pl.nb);
    a.tiles_per_signal = (int)tiles;
    a.lds_stride = pl.span;
    long long grid;
    if (int e = grid_of(tiles, batch, a.groups, "resample", &grid)) return e;
    const size_t lds = (size_t)nch * pl.span * sizeof(float);
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_resample<%d>: grid %lld, lds %zu B, %d phases x %d taps, step %d; tile %d phases x %d blocks "
                "(%d outputs), %d block groups, %d lanes\n", nch, grid, lds, n_phases, n_taps, step, pl.pt, pl.nb, pl.nb * n_phases, pl.ng, pl.threads);
    with_vec<2>(nch == 2, [&](auto n) { hipLaunchKernelGGL(k_resample<n>, dim3((unsigned)grid), dim3(pl.threads), lds, (hipStream_t)stream, a); });
    return launch_check("k_resample", nch);
}

// ---- Resample without a table (kpr_resample_direct_kernels.h): the window, the tile, the launch ----
// The same h as above, evaluated per tap on the device.  Every output sums the window of n_taps = 2 H inputs,
// H = ceil(U / P), U = L max / rolloff: it holds the support |j P - i Q| < U of every output.  No limit on the number of phases.
struct ResampleDirectShape {
    int P, Q, H, n_taps;
    int orig, fnew, L;
    double rolloff;
    int threads, per_lane, span;        // the tile: threads x per_lane outputs over `span` staged inputs per channel
};

static int resample_direct_shape(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint,
                                 ResampleDirectShape* r) {
    if (orig_freq <= 0 || new_freq <= 0)
        return fail(KPR_E_BADARG, "orig_freq and new_freq must be positive, got %d and %d", orig_freq, new_freq);
    if (lowpass_filter_width < 1) return fail(KPR_E_BADARG, "lowpass_filter_width must be at least 1, got %d", lowpass_filter_width);
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return fail(KPR_E_BADARG, "rolloff must lie in (0, 1], got %g", rolloff);
    if ((unsigned)adjoint > 1u) return fail(KPR_E_BADARG, "adjoint must be 0 or 1, got %d", adjoint);
    int a = orig_freq, b = new_freq;
    while (b) { const int t = a % b; a = b; b = t; }
    r->orig = orig_freq / a;
    r->fnew = new_freq / a;
    r->L = lowpass_filter_width;
    r->rolloff = rolloff;
    r->P = adjoint ? r->orig : r->fnew;
    r->Q = adjoint ? r->fnew : r->orig;
    const double h = std::ceil((double)lowpass_filter_width * (double)std::max(r->orig, r->fnew) / rolloff / (double)r->P);
    if (2.0 * h > (double)kRdMaxTaps)
        return fail(KPR_E_UNSUPPORTED, "resample %d -> %d%s without a table: a support of %.0f taps; supported are at most %d taps",
                    orig_freq, new_freq, adjoint ? " (adjoint)" : "", 2.0 * h, kRdMaxTaps);
    r->H = (int)h;
    r->n_taps = 2 * r->H;
    // the largest tile whose span fits: (tile - 1) Q div P + 1 + n_taps staged inputs (Q / P <= 64 when the taps fit)
    auto span_of = [&](int tile) -> long long { return ((long long)(tile - 1) * r->Q) / r->P + 1 + r->n_taps; };
    r->threads = kRdMaxThreads;
    r->per_lane = kRdMaxPerLane;
    while (r->per_lane > 1 && span_of(r->threads * r->per_lane) > kRdLdsWords) --r->per_lane;
    while (r->threads > 64 && span_of(r->threads * r->per_lane) > kRdLdsWords) r->threads /= 2;
    r->span = (int)span_of(r->threads * r->per_lane);
    if (r->span > kRdLdsWords)                                           // (cannot happen: 63 * 64 + 1 + 128 words)
        return fail(KPR_E_UNSUPPORTED, "resample %d -> %d without a table: a tile of %d staged inputs", orig_freq, new_freq, r->span);
    return 0;
}

static int run_resample_direct(const float* x, int64_t batch, int channels, int64_t in_len, int layout, int orig_freq, int new_freq,
                               int lowpass_filter_width, double rolloff, int adjoint, int64_t out_len, float* out, kpr_stream_t stream) {
    if (int e = check_series("bad batch/channels/in_len/out_len/layout", batch, channels, std::min(in_len, out_len), layout, false)) return e;
    ResampleDirectShape r;
    if (int e = resample_direct_shape(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint, &r)) return e;
    const Series si = series_of(layout, channels, in_len, false), so = series_of(layout, channels, out_len, false);
    if (int e = check_reach("resample", std::max(in_len, out_len), si.stride, 30)) return e;
    if (batch == 0 || out_len == 0) return 0;
    if (int e = check_ptrs("", {{"x", x, (uintptr_t)batch * si.item * 4, 4, in_len == 0, false},
                                {"out", out, (uintptr_t)batch * so.item * 4, 4, false, true}}))
        return e;
    const int nch = layout == KPR_CHANNELS_LAST && channels % 2 == 0 ? 2 : 1;      // a pair of interleaved channels is one series
    const int mx = std::max(r.orig, r.fnew), mn = std::min(r.orig, r.fnew);
    ResampleDirectArgs a;
    a.x = x; a.out = out;
    a.P = r.P; a.Q = r.Q; a.n_taps = r.n_taps; a.H = r.H;
    a.in_len = (int)in_len; a.out_len = (int)out_len;
    a.stride = si.stride;
    a.groups = channels / nch;
    a.in_item = si.item; a.out_item = so.item;
    a.in_chan = si.chan * nch; a.out_chan = so.chan * nch;
    a.per_lane = r.per_lane;
    a.tile = r.threads * r.per_lane;
    const long long tiles = (out_len + a.tile - 1) / a.tile;
    a.tiles_per_signal = (int)tiles;
    const long long stepq = (long long)r.threads * r.Q;
    a.step_a = (int)(stepq / r.P);
    a.step_r = (int)(stepq % r.P);
    a.lds_stride = r.span;
    a.inv_p = 1.0 / (double)r.P;
    a.beta = (float)(rolloff * (double)r.P / (double)mx);
    a.scale = (float)(rolloff * (double)mn / (double)r.orig);
    a.inv_2l = (float)(1.0 / (2.0 * (double)r.L));
    a.lim = (float)r.L;
    long long grid;
    if (int e = grid_of(tiles, batch, a.groups, "resample", &grid)) return e;
    const size_t lds = (size_t)nch * r.span * sizeof(float);
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_resample_direct<%d>: grid %lld, lds %zu B, %d / %d, %d taps; tile %d lanes x %d outputs, "
                "%d staged inputs\n", nch, grid, lds, r.P, r.Q, r.n_taps, r.threads, r.per_lane, r.span);
    with_vec<2>(nch == 2, [&](auto n) {
        hipLaunchKernelGGL(k_resample_direct<n>, dim3((unsigned)grid), dim3(r.threads), lds, (hipStream_t)stream, a);
    });
    return launch_check("k_resample_direct", nch);
}

}  // namespace kpr
