// kpr_host_lfilter.h -- host side of the biquad section (kpr_lfilter_kernels.h): the coefficient checks, the carry matrices from the
// impulse response in long double and their cache, the plan (which form runs), the workspace layout and the launches.
// Part of the single translation unit kapre_hip.hip (included there after kpr_host_griffin_lim.h; not stand-alone).
#pragma once

namespace kpr {

// series below which the automatic dispatch cuts the time axis into segments (three launches, two reads) rather than walking
// every series with one workgroup: from the measurement in profiles/lfilter_times.md
constexpr long long kLfSegmentedBelow = 160;
constexpr int64_t kLfCarryMax = 1 << 20;                     // longest chunk kpr_lfilter_carry answers for

// coef = (b0, b1, b2, a1, a2), normalised by a0: finite, and (a1, a2) inside the stability triangle
static int lfilter_coef(const double* coef) {
    if (!coef) return fail(KPR_E_BADARG, "coef is NULL");
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(coef[i])) return fail(KPR_E_BADARG, "lfilter: coefficient %d is not finite", i);
    const double a1 = coef[3], a2 = coef[4];
    if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2))
        return fail(KPR_E_BADARG, "lfilter: a1 = %.17g, a2 = %.17g lie outside the stability triangle |a2| < 1, |a1| < 1 + a2", a1, a2);
    return 0;
}

// M_n = [[g[n], -a2 g[n-1]], [g[n-1], -a2 g[n-2]]] for every n of `want` (ascending), g the impulse response of 1 / A(z) run in
// long double: as stable as the filter itself (repeated squaring of the companion matrix is not).  sigma = 0: M_n as it stands.
// sigma = +-1: the matrix the kernels apply to a carried state, (T M_n T^-1)^T with T = [[1, 0], [1, -sigma]].  The transposed
// direct form's state z moves by M_n^T; it is carried as w = (z1 + sigma z2, -sigma z2), and in that basis M_n^T is the transpose
// above.  Why the basis (lfilter_sigma): with the poles near z = sigma the entries of M_n are large and nearly cancel -- for a
// 5 Hz high-pass at 48 kHz they reach 6e2 while M_n c is of the order of c -- so in the plain basis every product rounds at 6e2
// times the signal and the filter's own gain carries that error on.  Here the cancellation is done once, in long double, and
// what is left multiplies values of the signal's own size.
static void lfilter_carries(double a1d, double a2d, int sigma, const std::vector<int64_t>& want, std::vector<std::array<double, 4>>* out) {
    const long double a1 = a1d, a2 = a2d, sg = sigma;
    out->clear();
    long double g0 = 1.0L, g1 = 0.0L, g2 = 0.0L;             // g[n], g[n-1], g[n-2]
    int64_t n = 0;
    for (int64_t w : want) {
        for (; n < w; ++n) {
            const long double g = -a1 * g0 - a2 * g1;
            g2 = g1; g1 = g0; g0 = g;
        }
        if (w == 0) { out->push_back({1.0, 0.0, 0.0, 1.0}); continue; }
        const long double A = g0, B = -a2 * g1, C = g1, D = w == 1 ? 0.0L : -a2 * g2;
        if (sigma == 0) out->push_back({(double)A, (double)B, (double)C, (double)D});
        else out->push_back({(double)(A + sg * B), (double)(A + sg * B - sg * C - D), (double)(-sg * B), (double)(-sg * B + D)});
    }
}
// kpr_lfilter_carry: M_n in the plain basis for one chunk length n
static int lfilter_carry(const double* coef, int64_t n, double* M) {
    if (!M) return fail(KPR_E_BADARG, "M is NULL");
    if (int e = lfilter_coef(coef)) return e;
    if (n < 0 || n > kLfCarryMax) return fail(KPR_E_BADARG, "chunk length %lld outside [0, 2^20]", (long long)n);
    std::vector<std::array<double, 4>> m;
    lfilter_carries(coef[3], coef[4], 0, {n}, &m);
    std::copy(m[0].begin(), m[0].end(), M);
    return 0;
}
// the sign of the basis: poles in the right half plane (a1 <= 0) carry z1 + z2, in the left z1 - z2
static int lfilter_sigma(double a1) { return a1 <= 0.0 ? 1 : -1; }

// the table of a section, cached per (a1, a2): the plan's chunk lengths are constants of the library
static int lfilter_table(const double* coef, LfTab* tab) {
    static std::map<std::pair<double, double>, LfTab> cache;
    const std::pair<double, double> key(coef[3], coef[4]);
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = cache.find(key);
    if (it == cache.end()) {
        std::vector<int64_t> want;
        for (int i = 0; i < 64; ++i) want.push_back((int64_t)i * kLfLane);   // 0 ... 1008; holds 16 2^k for k <= 5
        want.push_back(kLfWaveSamples);
        want.push_back(kLfSeg);
        std::vector<std::array<double, 4>> m;
        lfilter_carries(coef[3], coef[4], lfilter_sigma(coef[3]), want, &m);
        LfTab t;
        for (int i = 0; i < 64; ++i) std::copy(m[i].begin(), m[i].end(), t.lane[i]);
        for (int k = 0; k < 6; ++k) std::copy(m[1 << k].begin(), m[1 << k].end(), t.scan[k]);
        std::copy(m[64].begin(), m[64].end(), t.wave);
        std::copy(m[65].begin(), m[65].end(), t.seg);
        if (cache.size() >= 256) cache.clear();                              // randomised equalisers: keep the map bounded
        it = cache.emplace(key, t).first;
    }
    *tab = it->second;
    return 0;
}

static int lfilter_dims(int64_t batch, int channels, int64_t len, int layout) {
    if (batch < 0 || channels <= 0 || len < 0 || (unsigned)layout > 1u) return fail(KPR_E_BADARG, "bad batch/channels/len/layout");
    const long long reach = layout == KPR_CHANNELS_LAST ? channels : 1;
    if (len * reach >= (1LL << 30))
        return fail(KPR_E_UNSUPPORTED, "lfilter: %lld samples x %d channels: 2^30 elements or more per signal are not supported",
                    (long long)len, channels);
    if (batch * (long long)channels * ((len + kLfSeg - 1) / kLfSeg + 1) > 0x7fffffffLL)
        return fail(KPR_E_UNSUPPORTED, "lfilter: too many segments (%lld series of %lld samples)", (long long)(batch * channels), (long long)len);
    return 0;
}

static long long lfilter_segments(int64_t len) { return std::max<long long>(1, (len + kLfSeg - 1) / kLfSeg); }

// 1 = whole-signal, 2 = segmented
static int lfilter_form(int64_t batch, int channels, int64_t len) {
    if (lfilter_segments(len) < 2) return 1;
    const int v = opt(OPT_LFILTER_VARIANT);
    if (v) return v;
    return batch * (long long)channels < kLfSegmentedBelow ? 2 : 1;
}

// | zero-state end states | carry-ins |, 2 doubles per (series, segment) each
static size_t lfilter_workspace(int64_t batch, int channels, int64_t len) {
    if (lfilter_segments(len) < 2) return 0;
    return (size_t)batch * channels * (size_t)lfilter_segments(len) * 32;
}

template <int MODE>
static int lfilter_launch(const LfArgs& a, bool vec, bool rev, long long grid, hipStream_t st) {
    const dim3 g((unsigned)grid), b(64 * kLfWaves);
    with_vec<4>(vec, [&](auto v) {
        constexpr bool V = decltype(v)::value > 1;
        if (rev) hipLaunchKernelGGL((k_lfilter<V, true, MODE>), g, b, 0, st, a);
        else hipLaunchKernelGGL((k_lfilter<V, false, MODE>), g, b, 0, st, a);
    });
    return launch_check("k_lfilter", vec ? 4 : 1, MODE == LF_FIR ? (rev ? "fir,rev" : "fir") : MODE == LF_ENDS ? (rev ? "ends,rev" : "ends")
                                                                                                               : (rev ? "full,rev" : "full"));
}

static int run_lfilter(const float* x, int64_t batch, int channels, int64_t len, int layout, const double* coef, int reverse, float* out,
                       void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    if (int e = lfilter_dims(batch, channels, len, layout)) return e;
    if (int e = lfilter_coef(coef)) return e;
    if (reverse != 0 && reverse != 1) return fail(KPR_E_BADARG, "reverse must be 0 or 1, got %d", reverse);
    if (batch == 0 || len == 0) return 0;
    if (!x || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    if ((((uintptr_t)x) | ((uintptr_t)out)) & 3) return fail(KPR_E_BADARG, "x / out must be 4-byte aligned");
    const size_t n_bytes = (size_t)batch * channels * (size_t)len * 4;
    // (the FIR form reads its neighbour's samples from x after that neighbour may have stored: there is no in-place form)
    if (ranges_overlap(x, n_bytes, out, n_bytes)) return fail(KPR_E_BADARG, "x and out overlap (there is no in-place form)");
    const bool cl = layout == KPR_CHANNELS_LAST && channels > 1;
    const bool fir = coef[3] == 0.0 && coef[4] == 0.0;
    const long long series = batch * (long long)channels, n_seg = lfilter_segments(len);
    const int form = fir ? 2 : lfilter_form(batch, channels, len);
    const hipStream_t st = (hipStream_t)stream;

    LfArgs a;
    a.x = x; a.out = out; a.ends = nullptr; a.carry = nullptr;
    a.b0 = coef[0]; a.b1 = coef[1]; a.b2 = coef[2]; a.na1 = -coef[3]; a.na2 = -coef[4];
    a.sigma = (double)lfilter_sigma(coef[3]);
    a.len = (int)len;
    a.stride = cl ? channels : 1;
    a.channels = channels;
    a.item = (long long)channels * len;
    a.chan = cl ? 1 : len;
    a.n_seg = form == 2 ? (int)n_seg : 1;
    a.seg_steps = form == 2 ? kLfSegSteps : (int)((len + kLfStep - 1) / kLfStep);
    const bool vec = !cl && len % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_lfilter: %lld series of %lld samples, stride %d, %s, %s, %d workgroup(s) per series, %s\n", series,
                (long long)len, a.stride, fir ? "fir" : form == 2 ? "segmented" : "whole-signal", reverse ? "reverse" : "forward", a.n_seg,
                vec ? "16-byte accesses" : "4-byte accesses");
    if (fir) {
        std::memset(&a.tab, 0, sizeof a.tab);
        return lfilter_launch<LF_FIR>(a, vec, reverse, series * a.n_seg, st);
    }
    if (int e = lfilter_table(coef, &a.tab)) return e;
    if (form == 1) return lfilter_launch<LF_FULL>(a, vec, reverse, series, st);

    const size_t need = lfilter_workspace(batch, channels, len);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
        return fail(KPR_E_WORKSPACE, "lfilter workspace: %zu bytes needed (kpr_lfilter_workspace_bytes, 8-byte aligned), got %zu", need,
                    workspace ? workspace_bytes : (size_t)0);
    if (ranges_overlap(workspace, need, x, n_bytes) || ranges_overlap(workspace, need, out, n_bytes))
        return fail(KPR_E_BADARG, "the workspace overlaps x or out");
    a.ends = (double*)workspace;
    double* carry = a.ends + 2 * series * n_seg;
    if (int e = lfilter_launch<LF_ENDS>(a, vec, reverse, series * n_seg, st)) return e;
    LfCombineArgs c;
    c.ends = a.ends; c.carry = carry; c.n_series = series; c.n_seg = (int)n_seg; c.reverse = reverse;
    std::copy(a.tab.seg, a.tab.seg + 4, c.seg);
    hipLaunchKernelGGL(k_lfilter_combine, dim3((unsigned)((series + 63) / 64)), dim3(64), 0, st, c);
    if (int e = launch_check("k_lfilter_combine")) return e;
    a.carry = carry;
    return lfilter_launch<LF_FULL>(a, vec, reverse, series * n_seg, st);
}

}  // namespace kpr
