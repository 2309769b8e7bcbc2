// kpr_host_ops.h -- the run_* bodies (argument checks + launch) of the elementwise, decibel, float64 filterbank, signal (Frame, Energy,
// Delta), augmentation, companding, PCEN, CMVN, Resample, TimeStretch and HPSS entry points, forward and backward, and the host-only
// frame count and resample table (kpr_misc_kernels.h, kpr_generic_kernels.h, kpr_grad_kernels.h, kpr_signal_kernels.h,
// kpr_augment_kernels.h, kpr_companding_kernels.h, kpr_pcen_kernels.h, kpr_cmvn_kernels.h, kpr_resample_kernels.h,
// kpr_resample_direct_kernels.h, kpr_time_stretch_kernels.h, kpr_hpss_kernels.h).  No body restarts the launch log or reads the status word: the entry points do.
// The three time-tiled launchers (PCEN, CMVN, TimeStretch) take their launch shape from col_launch (kpr_host.h; device side: kpr_cols.h).
// Part of the single translation unit kapre_hip.hip (included there after kpr_host_mel.h; not stand-alone).
#pragma once

namespace kpr {

// ---- Magnitude / Phase: |x| (phase = 0) or the angle (1) of n complex64 (T = float) / complex128 (T = double) values ----
// (the two precisions have always worded a negative n differently)
template <typename T>
static int run_cplx_to_real(const void* x, int64_t n, int phase, T* out, kpr_stream_t stream) {
    if (n < 0) return fail(KPR_E_BADARG, sizeof(T) == 4 ? "negative size" : "negative element count");
    if (n == 0) return 0;
    if (!x || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    const dim3 grid(grid_1d(n, 256));
    if constexpr (sizeof(T) == 4) hipLaunchKernelGGL(k_cplx_to_real, grid, dim3(256), 0, (hipStream_t)stream, (const float2*)x, (long long)n, phase, out);
    else hipLaunchKernelGGL(k_cplx_to_real_f64, grid, dim3(256), 0, (hipStream_t)stream, (const double2*)x, (long long)n, phase, out);
    return launch_check(sizeof(T) == 4 ? "k_cplx_to_real" : "k_cplx_to_real_f64");
}

// ---- backward passes (kpr_grad_kernels.h): launch helpers of the C entry points ----
template <typename T>
static int run_cplx_bwd(const void* x, const T* g, int64_t n, int phase, void* gx, kpr_stream_t stream) {
    if (n < 0) return fail(KPR_E_BADARG, "negative element count");
    if (n == 0) return 0;
    if (!x || !g || !gx) return fail(KPR_E_BADARG, "x / g / gx must not be NULL");
    hipLaunchKernelGGL(k_cplx_to_real_bwd<T>, dim3(grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const GCplx<T>*)x, g, (long long)n, phase, (GCplx<T>*)gx);
    return launch_check("k_cplx_to_real_bwd");
}
template <typename T>
static int run_edge_scale(const void* in, int64_t n, int n_freq, int inner, int n_fft, T s_edge, T s_mid, void* out,
                          kpr_stream_t stream) {
    if (n < 0 || n_freq <= 0 || inner <= 0 || n_fft <= 0) return fail(KPR_E_BADARG, "bad sizes");
    if (n_freq != n_fft / 2 + 1) return fail(KPR_E_BADARG, "n_freq %d is not n_fft / 2 + 1 (n_fft %d)", n_freq, n_fft);
    if (n % ((int64_t)n_freq * inner)) return fail(KPR_E_BADARG, "element count is not a multiple of n_freq * inner");
    if (n == 0) return 0;
    if (!in || !out) return fail(KPR_E_BADARG, "in / out must not be NULL");
    const int nyq = (n_fft & 1) ? -1 : n_fft / 2;
    hipLaunchKernelGGL(k_spec_edge_scale<T>, dim3(grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const GCplx<T>*)in, (long long)n, n_freq, inner, nyq, s_edge, s_mid, (GCplx<T>*)out);
    return launch_check("k_spec_edge_scale");
}
template <typename T>
static int run_db_bwd(const T* x, const T* gy, int64_t n_items, int64_t item_size, double ref_value, double amin,
                      double dynamic_range, T* gx, kpr_stream_t stream) {
    if (n_items < 0 || item_size < 0) return fail(KPR_E_BADARG, "negative size");
    if (int e = check_db_values(ref_value, amin, dynamic_range)) return e;
    if (n_items == 0 || item_size == 0) return 0;
    if (!x || !gy || !gx) return fail(KPR_E_BADARG, "x / gy / gx must not be NULL");
    if (n_items > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "decibel backward: more than 2^31 - 1 items");
    const double ref_term = 10.0 * std::log10(std::max(amin, ref_value));
    // float32: the forward (make_db / to_db) raises amin to the smallest normal float -- the backward floors at the same value
    const double amin_k = sizeof(T) == 4 ? std::max(amin, 1.17549435e-38) : amin;
    hipLaunchKernelGGL(k_db_bwd<T>, dim3((unsigned)n_items), dim3(1024), 0, (hipStream_t)stream, x, gy,
                       (long long)item_size, (T)amin_k, (T)ref_term, (T)dynamic_range, gx);
    return launch_check("k_db_bwd");
}

// ---- mu-law companding / ConcatenateFrequencyMap (kpr_companding_kernels.h): launch helpers of the C entry points ----
static int mu_law_args(int64_t n, int quantization_channels, MuLawDev* p) {
    if (n < 0) return fail(KPR_E_BADARG, "negative element count");
    if (quantization_channels < 2 || quantization_channels > 65536)
        return fail(KPR_E_BADARG, "quantization_channels %d outside [2, 65536]", quantization_channels);
    if (n > kCompandMaxElems)
        return fail(KPR_E_UNSUPPORTED, "%lld elements: one call takes at most 2^40", (long long)n);
    const double q = quantization_channels, mu = q - 1.0, l2q = std::log2(q), c = l2q / mu, inv = 1.0 / mu;
    p->mu = (float)mu;
    p->half_mu = (float)(0.5 * mu);
    p->half_q = (float)(0.5 * q);
    p->inv_log2q = (float)(1.0 / l2q);
    p->c_hi = (float)c;
    p->c_lo = (float)(c - (double)p->c_hi);
    p->inv_hi = (float)inv;
    p->inv_lo = (float)(inv - (double)p->inv_hi);
    p->gcoef = (float)(2.0 * std::log(q) / (mu * mu));
    return 0;
}

// the pointers of a streaming call: not NULL, 4-byte aligned, out either the input itself or clear of it
static int stream_ptrs(const void* in, const void* in2, const void* out, int64_t n, const char* names) {
    if (!in || !in2 || !out) return fail(KPR_E_BADARG, "%s must not be NULL", names);
    if ((((uintptr_t)in) | ((uintptr_t)in2) | ((uintptr_t)out)) & 3) return fail(KPR_E_BADARG, "%s must be 4-byte aligned", names);
    const uintptr_t nb = (uintptr_t)n * 4;
    for (const void* q : {in, in2})
        if (q != out && ranges_overlap(q, nb, out, nb)) return fail(KPR_E_BADARG, "%s overlap (only out == in, in place, is allowed)", names);
    return 0;
}

template <int OP>
static int run_mu_law(const void* in, const void* g, void* out, int64_t n, int quantization_channels, const char* names,
                      kpr_stream_t stream) {
    MuLawDev p;
    if (int e = mu_law_args(n, quantization_channels, &p)) return e;
    if (n == 0) return 0;
    if (int e = stream_ptrs(in, g, out, n, names)) return e;
    const long long groups = n / 4 + 1;
    hipLaunchKernelGGL(k_mu_law<OP>, dim3((unsigned)((groups + kStreamChunk - 1) / kStreamChunk)), dim3(256), 0,
                       (hipStream_t)stream, (const unsigned*)in, (const unsigned*)g, (unsigned*)out, (long long)n, p);
    return launch_check(OP == MU_ENCODE ? "k_mu_law_encode" : OP == MU_DECODE_BWD ? "k_mu_law_decode_bwd" : "k_mu_law_decode");
}

template <bool DROP>
static int run_freq_map(const float* in, int64_t batch, int channels, int64_t frames, int n_freq, int layout, float* out,
                        kpr_stream_t stream) {
    if (batch < 0 || channels <= 0 || frames < 0 || n_freq <= 0 || (unsigned)layout > 1u)
        return fail(KPR_E_BADARG, "bad batch/channels/frames/n_freq/layout");
    const long long plane = (long long)frames * n_freq;
    if (plane * ((long long)channels + 1) > 0x7fffffffLL)
        return fail(KPR_E_UNSUPPORTED, "frames * n_freq * (channels + 1) = %lld elements per item: 2^31 or more is not supported",
                    plane * ((long long)channels + 1));
    if (batch == 0 || plane == 0) return 0;
    const long long n_in = batch * plane * (channels + (DROP ? 1 : 0)), n_out = batch * plane * (channels + (DROP ? 0 : 1));
    if (!in || !out) return fail(KPR_E_BADARG, "%s must not be NULL", DROP ? "g / gx" : "x / out");
    if ((((uintptr_t)in) | ((uintptr_t)out)) & 3) return fail(KPR_E_BADARG, "the pointers must be 4-byte aligned");
    if (ranges_overlap(in, (uintptr_t)n_in * 4, out, (uintptr_t)n_out * 4)) return fail(KPR_E_BADARG, "input and output overlap");
    const bool cl = layout == KPR_CHANNELS_LAST;
    FmapArgs a;
    a.rin = (unsigned)(cl ? channels : plane * channels);
    a.rmap = (unsigned)(cl ? 1 : plane);
    a.n_freq = (unsigned)n_freq;
    a.osz = (unsigned)(plane * (channels + (DROP ? 0 : 1)));
    a.last = n_freq > 1 ? n_freq - 1 : -1;
    a.inv = n_freq > 1 ? (float)(1.0 / (double)(n_freq - 1)) : 0.0f;
    a.chunks = (int)(((long long)(a.osz >> 2) + kStreamChunk) / kStreamChunk);
    if (batch * a.chunks > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "too many items");
    const dim3 grid((unsigned)(batch * a.chunks));
    if (cl)
        hipLaunchKernelGGL((k_freq_map<DROP, true>), grid, dim3(256), 0, (hipStream_t)stream, (const unsigned*)in, (unsigned*)out, a);
    else
        hipLaunchKernelGGL((k_freq_map<DROP, false>), grid, dim3(256), 0, (hipStream_t)stream, (const unsigned*)in, (unsigned*)out, a);
    return launch_check(DROP ? "k_freq_map_drop" : "k_freq_map_concat");
}

// ---- PCEN (kpr_pcen_kernels.h): argument checks and launch of the forward / backward C entry points ----
// x (and smooth, gy for the backward pass) -> out; smooth_out only for the forward pass, may be NULL.
// gparams != NULL: the backward pass with the parameter gradients (kpr_pcen_bwd_params_f32), out = gx may then be NULL
static size_t pcen_params_workspace(int64_t outer, int64_t frames, int64_t inner) {
    return outer > 0 && frames > 0 && inner > 0 ? (size_t)16 * (size_t)outer * (size_t)inner : 0;
}

static int run_pcen(bool bwd, const float* x, const float* smooth, const float* gy, int64_t outer, int64_t frames, int64_t inner,
                    int band_div, int n_bands, const float* s, const float* alpha, const float* delta, const float* r, float eps,
                    float* out, float* smooth_out, kpr_stream_t stream, bool with_params = false, float* gparams = nullptr,
                    void* workspace = nullptr, size_t workspace_bytes = 0) {
    if (outer < 0 || frames < 0 || inner < 0 || band_div <= 0 || n_bands <= 0)
        return fail(KPR_E_BADARG, "bad outer/frames/inner/band_div/n_bands");
    if (with_params && (!gparams || ((uintptr_t)gparams & 3))) return fail(KPR_E_BADARG, "gparams must be a 4-byte aligned pointer");
    if (outer == 0 || frames == 0 || inner == 0) {
        if (!with_params) return 0;
        KPR_HIP(hipMemsetAsync(gparams, 0, (size_t)n_bands * 4 * sizeof(float), (hipStream_t)stream));    // empty sums
        return 0;
    }
    if (inner != (int64_t)n_bands * band_div)
        return fail(KPR_E_BADARG, "inner = %lld is not n_bands * band_div = %d * %d", (long long)inner, n_bands, band_div);
    if (!(eps > 0.0f)) return fail(KPR_E_BADARG, "eps must be positive");
    if (!x || (!out && !with_params) || !s || !alpha || !delta || !r || (bwd && (!smooth || !gy)))
        return fail(KPR_E_BADARG, with_params ? "x / smooth / gy and the parameter vectors must not be NULL"
                                  : bwd       ? "x / smooth / gy / gx and the parameter vectors must not be NULL"
                                              : "x / out and the parameter vectors must not be NULL");
    if (frames * inner > 0x7fffffffLL)
        return fail(KPR_E_UNSUPPORTED, "frames * inner = %lld elements per outer item: 2^31 or more is not supported",
                    (long long)(frames * inner));
    uintptr_t bits = (uintptr_t)x | (uintptr_t)out | (uintptr_t)smooth | (uintptr_t)gy | (uintptr_t)smooth_out | (uintptr_t)workspace;
    if (bits & 3) return fail(KPR_E_BADARG, "the pointers must be 4-byte aligned");
    const uintptr_t nb = (uintptr_t)outer * frames * inner * 4;
    {
        bool bad = ranges_overlap(out, nb, smooth_out, nb);
        for (const float* in : {x, smooth, gy}) bad = bad || ranges_overlap(out, nb, in, nb) || ranges_overlap(smooth_out, nb, in, nb);
        if (bad) return fail(KPR_E_BADARG, "an output overlaps an input or the other output (there is no in-place form)");
    }
    if (with_params) {
        const size_t need = pcen_params_workspace(outer, frames, inner);
        const uintptr_t ng = (uintptr_t)n_bands * 16;
        bool bad = ranges_overlap(gparams, ng, workspace, need);
        for (const float* t : {x, smooth, gy, (const float*)out})
            bad = bad || ranges_overlap(gparams, ng, t, nb) || ranges_overlap(workspace, need, t, nb);
        for (const float* t : {s, alpha, delta, r}) bad = bad || ranges_overlap(gparams, ng, t, (uintptr_t)n_bands * 4);
        if (bad) return fail(KPR_E_BADARG, "gparams or the workspace overlaps another argument");
        if (!workspace || workspace_bytes < need)
            return fail(KPR_E_WORKSPACE, "workspace of %zu bytes needed (kpr_pcen_bwd_params_workspace_bytes), got %zu", need,
                        workspace ? workspace_bytes : (size_t)0);
    }
    ColLaunch l;
    if (int e = col_launch(outer, inner, 4, kPcenWaves, (bits & 15) == 0, &l)) return e;
    PcenArgs a;
    a.x = x; a.smooth = smooth; a.gy = gy; a.out = out; a.smooth_out = smooth_out;
    a.s = s; a.alpha = alpha; a.delta = delta; a.r = r;
    a.eps = eps;
    a.frames = (int)frames;
    a.inner = l.inner;
    a.groups_per_item = l.groups_per_item;
    a.band_div = (unsigned)band_div;
    a.n_groups = l.n_groups;
    a.partials = (float*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    const int mode = with_params ? (out ? PCEN_BWD_PARAMS : PCEN_BWD_PARAMS_ONLY) : bwd ? PCEN_BWD : smooth_out ? PCEN_FWD_SMOOTH : PCEN_FWD;
    with_vec<4>(l.wide, [&](auto v) {
        switch (mode) {
            case PCEN_FWD: hipLaunchKernelGGL((k_pcen<v, PCEN_FWD>), l.grid, l.block, 0, st, a); break;
            case PCEN_FWD_SMOOTH: hipLaunchKernelGGL((k_pcen<v, PCEN_FWD_SMOOTH>), l.grid, l.block, 0, st, a); break;
            case PCEN_BWD: hipLaunchKernelGGL((k_pcen<v, PCEN_BWD>), l.grid, l.block, 0, st, a); break;
            case PCEN_BWD_PARAMS: hipLaunchKernelGGL((k_pcen<v, PCEN_BWD_PARAMS>), l.grid, l.block, 0, st, a); break;
            default: hipLaunchKernelGGL((k_pcen<v, PCEN_BWD_PARAMS_ONLY>), l.grid, l.block, 0, st, a); break;
        }
    });
    if (!with_params) return launch_check(bwd ? "k_pcen_bwd" : "k_pcen", l.wide ? 4 : 1);
    if (int e = launch_check(out ? "k_pcen_bwd_params" : "k_pcen_bwd_params_only", l.wide ? 4 : 1)) return e;
    hipLaunchKernelGGL(k_pcen_param_reduce, dim3(4u * (unsigned)n_bands), dim3(256), 0, st, (const float*)workspace, gparams,
                       (long long)outer, (unsigned)inner, (unsigned)band_div, (unsigned)n_bands);
    return launch_check("k_pcen_param_reduce");
}

// ---- CMVN (kpr_cmvn_kernels.h): argument checks and launch of the forward / backward C entry points ----
// forward: x -> out (and rstd_out, may be NULL).  backward: x is y of the forward pass; (y, rstd, gy) -> out = gx with norm_vars,
// gy alone -> gx without (y and rstd are then not read and may be NULL)
template <int V, int FORM>
static void launch_cmvn(int mode, dim3 grid, dim3 block, hipStream_t st, const CmvnArgs& a) {
    switch (mode) {
        case CMVN_FWD: hipLaunchKernelGGL((k_cmvn<V, FORM, CMVN_FWD>), grid, block, 0, st, a); break;
        case CMVN_FWD_RSTD: hipLaunchKernelGGL((k_cmvn<V, FORM, CMVN_FWD_RSTD>), grid, block, 0, st, a); break;
        case CMVN_FWD_MEAN: hipLaunchKernelGGL((k_cmvn<V, FORM, CMVN_FWD_MEAN>), grid, block, 0, st, a); break;
        case CMVN_BWD: hipLaunchKernelGGL((k_cmvn<V, FORM, CMVN_BWD>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((k_cmvn<V, FORM, CMVN_BWD_MEAN>), grid, block, 0, st, a); break;
    }
}

static int run_cmvn(bool bwd, const float* x, const float* rstd, const float* gy, int64_t outer, int64_t frames, int64_t inner,
                    int norm_vars, float eps, float* out, float* rstd_out, kpr_stream_t stream) {
    if (outer < 0 || frames < 0 || inner < 0) return fail(KPR_E_BADARG, "bad outer/frames/inner");
    if (norm_vars != 0 && norm_vars != 1) return fail(KPR_E_BADARG, "norm_vars must be 0 or 1, got %d", norm_vars);
    if (!bwd && !(eps >= 0.0f && std::isfinite(eps))) return fail(KPR_E_BADARG, "eps must be finite and not negative");
    if (rstd_out && !norm_vars) return fail(KPR_E_BADARG, "rstd_out needs norm_vars = 1 (there is no rstd without the variance)");
    if (outer == 0 || frames == 0 || inner == 0) return 0;
    if (!norm_vars && bwd) x = rstd = nullptr;                       // not read
    if (!out || (!bwd && !x) || (bwd && (!gy || (norm_vars && (!x || !rstd)))))
        return fail(KPR_E_BADARG, !bwd ? "x / out must not be NULL" : norm_vars ? "y / rstd / gy / gx must not be NULL"
                                                                                : "gy / gx must not be NULL");
    if (frames * inner > 0x7fffffffLL)
        return fail(KPR_E_UNSUPPORTED, "frames * inner = %lld elements per outer item: 2^31 or more is not supported",
                    (long long)(frames * inner));
    const uintptr_t bits = (uintptr_t)x | (uintptr_t)out | (uintptr_t)rstd | (uintptr_t)gy | (uintptr_t)rstd_out;
    if (bits & 3) return fail(KPR_E_BADARG, "the pointers must be 4-byte aligned");
    {
        const uintptr_t nb = (uintptr_t)outer * frames * inner * 4, ns = (uintptr_t)outer * inner * 4;
        bool bad = ranges_overlap(out, nb, rstd_out, ns) || ranges_overlap(out, nb, rstd, ns) || ranges_overlap(rstd_out, ns, rstd, ns);
        for (const float* in : {x, gy}) bad = bad || ranges_overlap(out, nb, in, nb) || ranges_overlap(rstd_out, ns, in, nb);
        if (bad) return fail(KPR_E_BADARG, "an output overlaps an input or the other output (there is no in-place form)");
    }
    const bool res = frames <= kCmvnRows * kCmvnWaves && opt(OPT_CMVN_VARIANT) == 0;
    ColLaunch l;
    if (int e = col_launch(outer, inner, 4, kCmvnWaves, (bits & 15) == 0, &l)) return e;
    CmvnArgs a;
    a.x = x; a.gy = gy; a.rstd = rstd; a.out = out; a.rstd_out = rstd_out;
    a.eps = eps;
    a.frames = (int)frames;
    a.inner = l.inner;
    a.groups_per_item = l.groups_per_item;
    a.n_groups = l.n_groups;
    const int mode = bwd ? (norm_vars ? CMVN_BWD : CMVN_BWD_MEAN) : !norm_vars ? CMVN_FWD_MEAN : rstd_out ? CMVN_FWD_RSTD : CMVN_FWD;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_cmvn%s<%d,%s>: grid %lld x %d lanes, %d rows per wave, %d waves per workgroup, resident up to %d "
                "frames; %lld frames = %lld super-block(s), norm_vars %d%s\n", bwd ? "_bwd" : "", l.wide ? 4 : 1, res ? "res" : "str", (long long)l.grid.x,
                64 * kCmvnWaves, kCmvnRows, kCmvnWaves, kCmvnRows * kCmvnWaves, (long long)frames,
                (long long)((frames + kCmvnRows * kCmvnWaves - 1) / (kCmvnRows * kCmvnWaves)), norm_vars, rstd_out ? ", rstd kept" : "");
    const hipStream_t st = (hipStream_t)stream;
    with_vec<4>(l.wide, [&](auto v) {
        if (res) launch_cmvn<v, CMVN_RES>(mode, l.grid, l.block, st, a);
        else launch_cmvn<v, CMVN_STR>(mode, l.grid, l.block, st, a);
    });
    return launch_check(bwd ? "k_cmvn_bwd" : "k_cmvn", l.wide ? 4 : 1, res ? "res" : "str");
}

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
    if (batch < 0 || channels <= 0 || in_len < 0 || out_len < 0 || (unsigned)layout > 1u)
        return fail(KPR_E_BADARG, "bad batch/channels/in_len/out_len/layout");
    if (int e = resample_dims(n_phases, n_taps, step)) return e;
    // one signal is addressed with 32-bit element offsets (as kpr_num_frames)
    const bool cl = layout == KPR_CHANNELS_LAST;
    const long long reach = cl ? channels : 1;
    if (in_len * reach >= (1LL << 30) || out_len * reach >= (1LL << 30))
        return fail(KPR_E_UNSUPPORTED, "resample: %lld -> %lld samples x %d channels: 2^30 elements or more per signal are not supported",
                    (long long)in_len, (long long)out_len, channels);
    if (batch == 0 || out_len == 0) return 0;
    if ((!x && in_len > 0) || !out || !table || !first) return fail(KPR_E_BADARG, "x / out / table_dev / first_dev must not be NULL");
    if ((((uintptr_t)x) | ((uintptr_t)out) | ((uintptr_t)table) | ((uintptr_t)first)) & 3)
        return fail(KPR_E_BADARG, "the pointers must be 4-byte aligned");
    if (ranges_overlap(x, (uintptr_t)batch * channels * in_len * 4, out, (uintptr_t)batch * channels * out_len * 4))
        return fail(KPR_E_BADARG, "x and out overlap");
    const ResamplePlan pl = resample_plan(n_phases, step, n_taps);
    const long long n_blocks = (out_len + n_phases - 1) / n_phases;
    if (n_blocks * step >= (1LL << 31) - (1LL << 26))
        return fail(KPR_E_UNSUPPORTED, "resample: %lld outputs at %d inputs per %d outputs reach past 2^31 input samples", (long long)out_len,
                    step, n_phases);
    const int nch = cl && channels % 2 == 0 ? 2 : 1;
    ResampleArgs a;
    a.x = x; a.out = out; a.tab = table; a.first = first;
    a.P = n_phases; a.Q = step; a.n_taps = n_taps;
    a.in_len = (int)in_len; a.out_len = (int)out_len;
    a.estride = cl ? channels : 1;
    a.groups = channels / nch;
    a.in_item = (long long)channels * in_len; a.out_item = (long long)channels * out_len;
    a.in_group = cl ? nch : in_len; a.out_group = cl ? nch : out_len;
    a.pt = pl.pt; a.n_pt = pl.n_pt; a.ng = pl.ng; a.nb = pl.nb;
    a.n_blocks = (int)n_blocks;
    const long long tiles = (long long)pl.n_pt * ((n_blocks + pl.nb - 1) / pl.nb);
    a.tiles_per_signal = (int)tiles;
    a.lds_stride = pl.span;
    const long long grid = tiles * batch * a.groups;
    if (tiles > 0x7fffffffLL || grid > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "resample: too many tiles (%lld)", grid);
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
    if (batch < 0 || channels <= 0 || in_len < 0 || out_len < 0 || (unsigned)layout > 1u)
        return fail(KPR_E_BADARG, "bad batch/channels/in_len/out_len/layout");
    ResampleDirectShape r;
    if (int e = resample_direct_shape(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint, &r)) return e;
    // one signal is addressed with 32-bit element offsets (as kpr_resample_f32); compared without a product that could overflow
    const bool cl = layout == KPR_CHANNELS_LAST;
    const long long reach = cl ? channels : 1;
    const long long most = ((1LL << 30) - 1) / reach;                    // len * reach < 2^30  <=>  len <= most
    if (in_len > most || out_len > most)
        return fail(KPR_E_UNSUPPORTED, "resample: %lld -> %lld samples x %d channels: 2^30 elements or more per signal are not supported",
                    (long long)in_len, (long long)out_len, channels);
    if (batch == 0 || out_len == 0) return 0;
    if ((!x && in_len > 0) || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    if ((((uintptr_t)x) | ((uintptr_t)out)) & 3) return fail(KPR_E_BADARG, "the pointers must be 4-byte aligned");
    if (ranges_overlap(x, (uintptr_t)batch * channels * in_len * 4, out, (uintptr_t)batch * channels * out_len * 4))
        return fail(KPR_E_BADARG, "x and out overlap");
    const int nch = cl && channels % 2 == 0 ? 2 : 1;
    const int mx = std::max(r.orig, r.fnew), mn = std::min(r.orig, r.fnew);
    ResampleDirectArgs a;
    a.x = x; a.out = out;
    a.P = r.P; a.Q = r.Q; a.n_taps = r.n_taps; a.H = r.H;
    a.in_len = (int)in_len; a.out_len = (int)out_len;
    a.estride = cl ? channels : 1;
    a.groups = channels / nch;
    a.in_item = (long long)channels * in_len; a.out_item = (long long)channels * out_len;
    a.in_group = cl ? nch : in_len; a.out_group = cl ? nch : out_len;
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
    const long long grid = tiles * batch * a.groups;
    if (grid > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "resample: too many tiles (%lld)", grid);
    const size_t lds = (size_t)nch * r.span * sizeof(float);
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_resample_direct<%d>: grid %lld, lds %zu B, %d / %d, %d taps; tile %d lanes x %d outputs, "
                "%d staged inputs\n", nch, grid, lds, r.P, r.Q, r.n_taps, r.threads, r.per_lane, r.span);
    with_vec<2>(nch == 2, [&](auto n) {
        hipLaunchKernelGGL(k_resample_direct<n>, dim3((unsigned)grid), dim3(r.threads), lds, (hipStream_t)stream, a);
    });
    return launch_check("k_resample_direct", nch);
}

// ---- TimeStretch (kpr_time_stretch_kernels.h): argument checks and the one launch of the phase vocoder ----
// x: (outer, frames_in, inner) complex64 -> out: (outer, frames_out, inner); idx / alpha: frames_out device entries, never read here
static int run_time_stretch(const void* x, int64_t outer, int64_t frames_in, int64_t frames_out, int64_t inner, const int32_t* idx,
                            const float* alpha, void* out, uint32_t* phase_out, kpr_stream_t stream) {
    if (outer < 0 || frames_in < 0 || frames_out < 0 || inner < 0) return fail(KPR_E_BADARG, "bad outer/frames_in/frames_out/inner");
    const long long lim = 1LL << 30;
    if (inner > 0 && (frames_in > (lim - 1) / inner || frames_out > (lim - 1) / inner))
        return fail(KPR_E_UNSUPPORTED, "time stretch: %lld -> %lld frames x %lld columns: 2^30 elements or more per outer item are not "
                    "supported", (long long)frames_in, (long long)frames_out, (long long)inner);
    if (outer == 0 || frames_out == 0 || inner == 0) return 0;
    if ((!x && frames_in > 0) || !out || !idx || !alpha) return fail(KPR_E_BADARG, "x / out / idx / alpha must not be NULL");
    if ((((uintptr_t)x) | ((uintptr_t)out)) & 7) return fail(KPR_E_BADARG, "x / out must be 8-byte aligned");
    if ((((uintptr_t)idx) | ((uintptr_t)alpha) | ((uintptr_t)phase_out)) & 3)
        return fail(KPR_E_BADARG, "idx / alpha / phase_out must be 4-byte aligned");
    if (outer > (1LL << 59) / (std::max(frames_in, frames_out) * inner))                     // (the byte counts below stay in 64 bits)
        return fail(KPR_E_UNSUPPORTED, "time stretch: outer = %lld items of that size are not supported", (long long)outer);
    {
        const uintptr_t nx = (uintptr_t)outer * frames_in * inner * 8, no = (uintptr_t)outer * frames_out * inner * 8, nt = (uintptr_t)frames_out * 4;
        if (ranges_overlap(out, no, x, nx)) return fail(KPR_E_BADARG, "x and out overlap (there is no in-place form)");
        if (ranges_overlap(phase_out, no / 2, x, nx) || ranges_overlap(phase_out, no / 2, out, no))
            return fail(KPR_E_BADARG, "phase_out overlaps x or out");
        for (const void* t : {(const void*)idx, (const void*)alpha})
            if (ranges_overlap(t, nt, out, no) || ranges_overlap(t, nt, phase_out, no / 2))
                return fail(KPR_E_BADARG, "idx / alpha overlap an output");
    }
    ColLaunch l;
    if (int e = col_launch(outer, inner, 2, kPvWaves, ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0 && (((uintptr_t)phase_out) & 7) == 0, &l))
        return e;
    PvArgs a;
    a.x = (const float2*)x; a.out = (float2*)out; a.phase = phase_out;
    a.idx = idx; a.alpha = alpha;
    a.frames_in = (int)frames_in; a.frames_out = (int)frames_out;
    a.inner = l.inner;
    a.groups_per_item = l.groups_per_item;
    a.n_groups = l.n_groups;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_time_stretch<%d>: grid %lld x %d lanes, %d frames per wave, %d waves per workgroup; %lld -> %lld "
                "frames = %lld super-block(s)%s\n", l.wide ? 2 : 1, (long long)l.grid.x, 64 * kPvWaves, kPvRows, kPvWaves, (long long)frames_in,
                (long long)frames_out, (long long)((frames_out + kPvRows * kPvWaves - 1) / (kPvRows * kPvWaves)),
                phase_out ? ", phase words kept" : "");
    with_vec<2>(l.wide, [&](auto v) { hipLaunchKernelGGL(k_time_stretch<v>, l.grid, l.block, 0, (hipStream_t)stream, a); });
    return launch_check("k_time_stretch", l.wide ? 2 : 1);
}

// ---- HPSS (kpr_hpss_kernels.h): argument checks and the one launch of the harmonic-percussive separation ----
// x: float32 (CPLX = false) or complex64 spectrogram of `ch` channels in `layout`; out_h / out_p: tensors of out_ch channels in
// the same layout, of which each output fills the first ch.  The window instance: 15 slots when both windows fit, else 31.
static int hpss_half_windows(int kh, int kp, int* hh, int* hp) {
    if (kh < 3 || kh > 31 || kp < 3 || kp > 31 || kh % 2 == 0 || kp % 2 == 0)
        return fail(KPR_E_BADARG, "hpss: window lengths must be odd and in 3 ... 31, got kh = %d, kp = %d", kh, kp);
    *hh = (kh - 1) / 2;
    *hp = (kp - 1) / 2;
    return 0;
}
template <bool CPLX>
static int run_hpss(const void* x, int64_t batch, int ch, int64_t frames, int64_t freq, int layout, int kh, int kp, double power,
                    double margin_h, double margin_p, int want_mask, void* out_h, void* out_p, int out_ch, kpr_stream_t stream) {
    if (batch < 0 || ch < 0 || frames < 0 || freq < 0 || (unsigned)layout > 1u) return fail(KPR_E_BADARG, "bad batch/ch/frames/freq/layout");
    int hh, hp;
    if (int e = hpss_half_windows(kh, kp, &hh, &hp)) return e;
    if (!(power > 0.0) || !(margin_h >= 1.0) || !(margin_p >= 1.0) || std::isinf(margin_h) || std::isinf(margin_p))
        return fail(KPR_E_BADARG, "hpss: power must be > 0 (inf allowed) and the margins finite and >= 1");
    if ((unsigned)want_mask > 2u) return fail(KPR_E_BADARG, "hpss: want_mask must be 0 (values), 1 (masks) or 2 (medians)");
    if (out_ch < ch) return fail(KPR_E_BADARG, "hpss: out_ch = %d is less than ch = %d", out_ch, ch);
    const long long lim = 1LL << 30;
    if (freq > 0 && frames > (lim - 1) / freq)
        return fail(KPR_E_UNSUPPORTED, "hpss: %lld frames x %lld bins: planes of 2^30 elements or more are not supported",
                    (long long)frames, (long long)freq);
    if (batch == 0 || ch == 0 || frames == 0 || freq == 0) return 0;
    if (!x) return fail(KPR_E_BADARG, "x must not be NULL");
    if (!out_h && !out_p) return fail(KPR_E_BADARG, "hpss: out_h and out_p must not both be NULL");
    const unsigned ein = CPLX ? 8 : 4, eout = (CPLX && !want_mask) ? 8 : 4;
    if ((((uintptr_t)x) & (ein - 1)) || ((((uintptr_t)out_h) | ((uintptr_t)out_p)) & (eout - 1)))
        return fail(KPR_E_BADARG, "x / out_h / out_p are not aligned to their element size");
    const long long plane = frames * freq;
    if (batch > (1LL << 59) / (plane * out_ch)) return fail(KPR_E_UNSUPPORTED, "hpss: batch = %lld items of that size are not supported", (long long)batch);
    const bool cl = layout == KPR_CHANNELS_LAST;
    {
        // the bytes an output touches lie within [p, p + span): the first ch channels of a (batch, out_ch) tensor
        const uintptr_t nx = (uintptr_t)batch * ch * plane * ein;
        const uintptr_t slot = cl ? 1 : (uintptr_t)plane;                          // elements from one channel to the next
        const uintptr_t span = ((uintptr_t)(batch - 1) * out_ch * plane + (cl ? (uintptr_t)(plane - 1) * out_ch + ch : (uintptr_t)ch * plane)) * eout;
        if (ranges_overlap(out_h, span, x, nx) || ranges_overlap(out_p, span, x, nx))
            return fail(KPR_E_BADARG, "hpss: an output overlaps x (there is no in-place form)");
        if (ranges_overlap(out_h, span, out_p, span)) {
            // the one allowed way to interleave: both fill channel ranges of ONE out_ch-channel tensor that do not meet
            const uintptr_t lo = std::min((uintptr_t)out_h, (uintptr_t)out_p), hi = std::max((uintptr_t)out_h, (uintptr_t)out_p);
            const uintptr_t d = (hi - lo) / eout;
            if ((hi - lo) % eout || d % slot || d / slot < (uintptr_t)ch || d / slot + ch > (uintptr_t)out_ch)
                return fail(KPR_E_BADARG, "hpss: out_h and out_p overlap");
        }
    }
    const long long tiles_t = (frames + kHpTile - 1) / kHpTile, tiles_f = (freq + kHpTile - 1) / kHpTile;
    const long long blocks = (long long)batch * ch * tiles_t * tiles_f;
    if (blocks > 0x7fffffffLL || (long long)batch * ch > 0x7fffffffLL)
        return fail(KPR_E_UNSUPPORTED, "hpss: too many tiles: %lld", blocks);
    HpssArgs a;
    a.x = x; a.out_h = out_h; a.out_p = out_p;
    a.frames = (int)frames; a.freq = (int)freq; a.ch = ch;
    a.hh = hh; a.hp = hp;
    a.tiles_t = (int)tiles_t; a.tiles_f = (int)tiles_f;
    if (cl) {
        a.x_b = plane * ch; a.x_c = 1; a.x_t = freq * ch; a.x_f = ch;
        a.o_b = plane * out_ch; a.o_c = 1; a.o_t = freq * out_ch; a.o_f = out_ch;
    } else {
        a.x_b = plane * ch; a.x_c = plane; a.x_t = freq; a.x_f = 1;
        a.o_b = plane * out_ch; a.o_c = plane; a.o_t = freq; a.o_f = 1;
    }
    a.mode = want_mask;
    a.pmode = std::isinf(power) ? 3 : power == 1.0 ? 1 : power == 2.0 ? 2 : 0;
    a.power = (float)power; a.mh = (float)margin_h; a.mp = (float)margin_p;
    a.bad_value = (margin_h == 1.0 && margin_p == 1.0) ? 0.5f : 0.0f;
    const bool small = hh <= 7 && hp <= 7;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_hpss<%d,%s>: %lld tiles of %d x %d, windows %d x %d, %s\n", small ? 15 : 31, CPLX ? "c64" : "f32",
                blocks, kHpTile, kHpTile, kh, kp, want_mask == 2 ? "medians" : want_mask ? "masks" : "values");
    const dim3 grid((unsigned)blocks), block(64 * kHpWaves);
    if (small) hipLaunchKernelGGL((k_hpss<7, CPLX>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_hpss<15, CPLX>), grid, block, 0, (hipStream_t)stream, a);
    return launch_check("k_hpss", small ? 15 : 31, CPLX ? "c64" : "f32");
}

// ---- Frame / Energy / Delta (kpr_signal_kernels.h) and their backward passes (kpr_grad_kernels.h) ----
// frames per signal (kpr_frame_count); -1 with the message set: bad sizes
static int64_t frame_count(int64_t time, int frame_length, int hop_length, int pad_end) {
    if (time < 0 || frame_length <= 0 || hop_length <= 0) {
        fail(KPR_E_BADARG, "bad time/frame_length/hop_length (%lld, %d, %d)", (long long)time, frame_length,
             hop_length);
        return -1;
    }
    if (pad_end) return (time + hop_length - 1) / hop_length;
    return time < frame_length ? 0 : 1 + (time - frame_length) / hop_length;
}

static int frame_args(int64_t batch, int channels, int64_t time, int layout, int frame_length,
                      int hop_length, int pad_end, float pad_value, FrameArgs* a) {
    if (batch < 0 || channels <= 0 || (unsigned)layout > 1u)
        return fail(KPR_E_BADARG, "bad batch/channels/layout (%lld, %d, %d)", (long long)batch, channels, layout);
    const int64_t f = frame_count(time, frame_length, hop_length, pad_end);
    if (f < 0) return KPR_E_BADARG;
    if (f > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "too many frames per signal");
    a->n_sig = batch * channels; a->T = time; a->C = channels; a->F = (int)f; a->L = frame_length;
    a->hop = hop_length; a->cl = layout == KPR_CHANNELS_LAST && channels > 1; a->pad_value = pad_value;
    return 0;
}

static int run_frame_f32(const float* x, int64_t batch, int channels, int64_t time, int layout, int frame_length, int hop_length,
                         int pad_end, float pad_value, float* out, kpr_stream_t stream) {
    FrameArgs a;
    if (int e = frame_args(batch, channels, time, layout, frame_length, hop_length, pad_end, pad_value, &a))
        return e;
    const long long nrows = (a.cl ? (long long)batch : a.n_sig) * a.F;
    if (nrows == 0) return 0;
    if (!x || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    const int rowlen = a.cl ? a.L * a.C : a.L;
    const bool vec = (rowlen & 3) == 0 && (((uintptr_t)out) & 15) == 0;
    const long long work = nrows * (vec ? rowlen / 4 : rowlen);
    with_vec<4>(vec, [&](auto v) {
        hipLaunchKernelGGL(k_frame<v>, dim3(grid_1d(work, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x, a, out, nrows);
    });
    return launch_check("k_frame");
}

static int run_energy_f32(const float* x, int64_t batch, int channels, int64_t time, int layout, int frame_length, int hop_length,
                          int pad_end, float pad_value, float scale, float* out, kpr_stream_t stream) {
    FrameArgs a;
    if (int e = frame_args(batch, channels, time, layout, frame_length, hop_length, pad_end, pad_value, &a))
        return e;
    a.cl = layout == KPR_CHANNELS_LAST;            // output order depends on it even for one channel
    const long long nout = a.n_sig * a.F;
    if (nout == 0) return 0;
    if (!x || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    if (time == 0) return fail(KPR_E_UNSUPPORTED, "energy of an empty signal with pad_end");
    const int chunks = (a.F + kEnFrames - 1) / kEnFrames;
    const int q = frame_length / hop_length;
    size_t lds = sizeof(float) * 2 * (size_t)(kEnFrames + q + 1);
    if (lds > 64 * 1024) return fail(KPR_E_UNSUPPORTED, "frame_length / hop_length = %d is too large", q);
    // room for one partial sum per float4 of a workgroup's range (streaming path), when it fits 64 KiB
    int part_words = 0;
    if (hop_length % 4 == 0) {
        const size_t pw = (size_t)(kEnFrames + q + 1) * (hop_length / 4);
        if (lds + sizeof(float) * pw <= 64 * 1024) { part_words = (int)pw; lds += sizeof(float) * pw; }
    }
    hipLaunchKernelGGL(k_energy, dim3((unsigned)std::min<long long>(a.n_sig * chunks, 1 << 16)), dim3(256), lds,
                       (hipStream_t)stream, x, a, scale, out, chunks, part_words);
    return launch_check("k_energy");
}

static int run_frame_bwd_f32(const float* g, int64_t batch, int channels, int64_t time, int layout, int frame_length,
                             int hop_length, int pad_end, float* gx, kpr_stream_t stream) {
    FrameArgs a;
    if (int e = frame_args(batch, channels, time, layout, frame_length, hop_length, pad_end, 0.0f, &a)) return e;
    a.cl = layout == KPR_CHANNELS_LAST;
    const long long total = a.n_sig * a.T;
    if (total == 0) return 0;
    if (!gx || (!g && a.F > 0)) return fail(KPR_E_BADARG, "g / gx must not be NULL");
    hipLaunchKernelGGL(k_frame_bwd, dim3(grid_1d(total, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, g, a, gx);
    return launch_check("k_frame_bwd");
}

static int run_energy_bwd_f32(const float* x, const float* g, int64_t batch, int channels, int64_t time, int layout,
                              int frame_length, int hop_length, int pad_end, float scale, float* gx, kpr_stream_t stream) {
    FrameArgs a;
    if (int e = frame_args(batch, channels, time, layout, frame_length, hop_length, pad_end, 0.0f, &a)) return e;
    a.cl = layout == KPR_CHANNELS_LAST;
    const long long total = a.n_sig * a.T;
    if (total == 0) return 0;
    if (!x || !gx || (!g && a.F > 0)) return fail(KPR_E_BADARG, "x / g / gx must not be NULL");
    hipLaunchKernelGGL(k_energy_bwd, dim3(grid_1d(total, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x, g, a,
                       scale, gx);
    return launch_check("k_energy_bwd");
}

// Delta and its backward pass: the checks, the rows x columns view of the tensor and the filter's half width and scale
struct DeltaArgs { long long total, outer, inner; int n; float scale; };
static int delta_args(int64_t batch, int channels, int64_t frames, int n_freq, int layout, int win_length, int pad_mode, DeltaArgs* a) {
    if (batch < 0 || channels <= 0 || frames < 0 || n_freq <= 0 || (unsigned)layout > 1u)
        return fail(KPR_E_BADARG, "bad batch/channels/frames/n_freq/layout");
    if (win_length < 3 || (win_length & 1) == 0)
        return fail(KPR_E_BADARG, "win_length must be odd and >= 3, got %d", win_length);
    if (pad_mode < 0 || pad_mode > 2) return fail(KPR_E_BADARG, "bad pad mode %d", pad_mode);
    a->total = (long long)batch * channels * frames * n_freq;
    a->n = (win_length - 1) / 2;
    double denom = 0;
    for (int i = 1; i <= a->n; ++i) denom += 2.0 * i * i;
    a->scale = (float)(1.0 / denom);
    a->outer = layout == KPR_CHANNELS_LAST ? batch : batch * channels;
    a->inner = layout == KPR_CHANNELS_LAST ? (long long)n_freq * channels : n_freq;
    return 0;
}

static int run_delta_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout, int win_length,
                         int pad_mode, float* out, kpr_stream_t stream) {
    DeltaArgs a;
    if (int e = delta_args(batch, channels, frames, n_freq, layout, win_length, pad_mode, &a)) return e;
    if (a.total == 0) return 0;
    if (!x || !out || x == out) return fail(KPR_E_BADARG, "x / out must not be NULL or aliased");
    const bool vec = (a.inner & 3) == 0 && ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0;
    with_vec<4>(vec, [&](auto v) {
        hipLaunchKernelGGL(k_delta<v>, dim3(grid_1d(a.total / v, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x, a.outer,
                           (long long)frames, a.inner, a.n, pad_mode, a.scale, out);
    });
    return launch_check("k_delta");
}

static int run_delta_bwd_f32(const float* g, int64_t batch, int channels, int64_t frames, int n_freq, int layout, int win_length,
                             int pad_mode, float* gx, kpr_stream_t stream) {
    DeltaArgs a;
    if (int e = delta_args(batch, channels, frames, n_freq, layout, win_length, pad_mode, &a)) return e;
    if (a.total == 0) return 0;
    if (!g || !gx || g == gx) return fail(KPR_E_BADARG, "g / gx must not be NULL or aliased");
    hipLaunchKernelGGL(k_delta_bwd, dim3(grid_1d(a.total, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, g, a.outer,
                       (long long)frames, a.inner, a.n, pad_mode, a.scale, gx);
    return launch_check("k_delta_bwd");
}

// ---- SpecAugment / ChannelSwap (kpr_augment_kernels.h) ----
static int aug_geom(int64_t n_items, int n_time_masks, int n_freq_masks, int n_time, int n_freq, AugGeom* a) {
    if (n_items < 0 || n_time <= 0 || n_freq <= 0) return fail(KPR_E_BADARG, "bad n_items/n_time/n_freq");
    if (n_time_masks < 0 || n_freq_masks < 0 || n_time_masks > kAugMaxMasks || n_freq_masks > kAugMaxMasks)
        return fail(KPR_E_BADARG, "mask counts (%d, %d) outside [0, %d] per axis", n_time_masks, n_freq_masks, kAugMaxMasks);
    if ((long long)n_time * n_freq > 0x7fffffffLL)
        return fail(KPR_E_UNSUPPORTED, "n_time * n_freq = %lld elements per item: 2^31 or more is not supported",
                    (long long)n_time * n_freq);
    *a = AugGeom{(int)n_items, n_time_masks, n_freq_masks, n_time, n_freq, 0, 0};
    return 0;
}

static int run_spec_augment_draw(int32_t* table, int64_t n_items, int n_time_masks, int n_freq_masks, int n_time, int n_freq,
                                 int time_mask_param, int freq_mask_param, void* state, kpr_stream_t stream) {
    AugGeom a;
    if (int e = aug_geom(n_items, n_time_masks, n_freq_masks, n_time, n_freq, &a)) return e;
    // augmentation.py:245: an axis shorter than its mask parameter is an error (only asked of an axis that has masks)
    if (n_time_masks > 0 && (time_mask_param < 1 || time_mask_param > n_time))
        return fail(KPR_E_BADARG, "time_mask_param %d outside [1, n_time = %d]", time_mask_param, n_time);
    if (n_freq_masks > 0 && (freq_mask_param < 1 || freq_mask_param > n_freq))
        return fail(KPR_E_BADARG, "freq_mask_param %d outside [1, n_freq = %d]", freq_mask_param, n_freq);
    // the draw is one workgroup (the counter has one writer): 2^20 entries are 1024 per lane, some tens of microseconds
    if (n_items * (long long)(n_time_masks + n_freq_masks) > (1LL << 20))
        return fail(KPR_E_UNSUPPORTED, "mask table of %lld entries: the one-workgroup draw takes at most 2^20",
                    (long long)(n_items * (long long)(n_time_masks + n_freq_masks)));
    if (!state) return fail(KPR_E_BADARG, "state must not be NULL");
    if (a.n_items * (a.n_tm + a.n_fm) > 0 && !table) return fail(KPR_E_BADARG, "table must not be NULL");
    a.tparam = time_mask_param;
    a.fparam = freq_mask_param;
    // (a call without entries still advances the counter: one launch, one step of the stream)
    hipLaunchKernelGGL(k_specaug_draw, dim3(1), dim3(1024), 0, (hipStream_t)stream, table, a, (unsigned long long*)state);
    return launch_check("k_specaug_draw");
}

static int run_index_draw(int32_t* out, int64_t n_items, int n_choices, void* state, kpr_stream_t stream) {
    if (n_items < 0 || n_choices < 1) return fail(KPR_E_BADARG, "bad n_items / n_choices (%lld, %d)", (long long)n_items, n_choices);
    if (n_items > (1LL << 20))
        return fail(KPR_E_UNSUPPORTED, "%lld items: the one-workgroup draw takes at most 2^20", (long long)n_items);
    if (!state) return fail(KPR_E_BADARG, "state must not be NULL");
    if (n_items > 0 && !out) return fail(KPR_E_BADARG, "out must not be NULL");
    if (ranges_overlap(out, (uintptr_t)n_items * 4, state, 16)) return fail(KPR_E_BADARG, "out overlaps state");
    // (a call without items still advances the counter: one launch, one step of the stream)
    hipLaunchKernelGGL(k_index_draw, dim3(1), dim3(1024), 0, (hipStream_t)stream, out, (int)n_items, (unsigned)n_choices,
                       (unsigned long long*)state);
    return launch_check("k_index_draw");
}

static int run_spec_augment_apply(const float* x, float* out, const int32_t* table, int64_t n_items, int n_time_masks,
                                  int n_freq_masks, int n_time, int n_freq, float mask_value, kpr_stream_t stream) {
    AugGeom a;
    if (int e = aug_geom(n_items, n_time_masks, n_freq_masks, n_time, n_freq, &a)) return e;
    if (n_items == 0) return 0;
    if (!x || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    if (n_time_masks + n_freq_masks > 0 && !table) return fail(KPR_E_BADARG, "table must not be NULL");
    const long long isz = (long long)n_time * n_freq;
    const bool vec = ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0;
    if (n_freq > kAugMaxFreq)
        return fail(KPR_E_UNSUPPORTED, "n_freq = %d: the copy form holds at most %d bins per row", n_freq, kAugMaxFreq);
    // partial overlap would let a workgroup read what another has already masked (out == x: in place)
    const uintptr_t nb = (uintptr_t)(n_items * isz * 4);
    if (x != out && ranges_overlap(x, nb, out, nb)) return fail(KPR_E_BADARG, "x and out overlap (only out == x, in place, is allowed)");
    const long long chunks = (isz + kAugChunk - 1) / kAugChunk;
    if (n_items * chunks > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "too many items");
    with_vec<4>(vec, [&](auto v) {
        hipLaunchKernelGGL(k_specaug_apply<v>, dim3((unsigned)(n_items * chunks)), dim3(256), 0, (hipStream_t)stream, x, table, a,
                           (int)chunks, mask_value, out);
    });
    return launch_check("k_specaug_apply");
}

static int run_channel_gather(const void* x, void* out, int64_t outer, int n_ch, int64_t inner, int elem_bytes, const int32_t* perm,
                              kpr_stream_t stream) {
    if (outer < 0 || n_ch <= 0 || inner < 0) return fail(KPR_E_BADARG, "bad outer/n_ch/inner");
    if (elem_bytes != 4 && elem_bytes != 8) return fail(KPR_E_BADARG, "elem_bytes must be 4 (float32) or 8 (complex64), got %d", elem_bytes);
    if (n_ch > kGatherMaxCh)
        return fail(KPR_E_UNSUPPORTED, "%d channels: the permutation travels in the kernel arguments, at most %d", n_ch, kGatherMaxCh);
    if (!perm) return fail(KPR_E_BADARG, "perm must not be NULL");
    GatherPerm gp{};
    for (int c = 0; c < n_ch; ++c) {
        if (perm[c] < 0 || perm[c] >= n_ch) return fail(KPR_E_BADARG, "perm[%d] = %d outside [0, %d)", c, perm[c], n_ch);
        gp.p[c] = perm[c];
    }
    const long long words = inner * (elem_bytes / 4);                 // 4-byte words per (o, c) row
    if (outer == 0 || words == 0) return 0;
    if (!x || !out || x == out) return fail(KPR_E_BADARG, "x / out must not be NULL or aliased");
    const long long rows = outer * n_ch;
    if (words < 64) {
        if (words * n_ch > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "row too long");
        hipLaunchKernelGGL(k_channel_gather_rows, dim3(grid_1d(outer, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned*)x, (unsigned*)out, (long long)outer, n_ch, (int)words, gp);
        return launch_check("k_channel_gather_rows");
    }
    const bool vec = (words & 3) == 0 && ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0;
    const long long units = vec ? words / 4 : words;
    const dim3 grid((unsigned)std::min<long long>((units + 1023) / 1024, 64), (unsigned)std::min<long long>(rows, 65535));
    if (vec)
        hipLaunchKernelGGL(k_channel_gather<uint4>, grid, dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (uint4*)out, rows,
                           n_ch, units, gp);
    else
        hipLaunchKernelGGL(k_channel_gather<unsigned>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned*)x,
                           (unsigned*)out, rows, n_ch, units, gp);
    return launch_check("k_channel_gather");
}

// ---- float64 ApplyFilterbank and MagnitudeToDecibel (kpr_generic_kernels.h) ----
static int run_apply_filterbank_f64(const double* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                                    const double* fb, int n_filt, double* out, kpr_stream_t stream) {
    if (int e = check_rows_args(batch, channels, frames, n_freq, n_filt, layout, "bad filterbank shape", "bad layout %d")) return e;
    const long long total = (long long)batch * channels * frames * n_filt;
    if (total == 0) return 0;
    if (!x || !fb || !out) return fail(KPR_E_BADARG, "x / fb / out must not be NULL");
    hipLaunchKernelGGL(k_filterbank_f64, dim3(grid_1d(total, 256)), dim3(256), 0, (hipStream_t)stream, x,
                       (long long)batch, channels, (long long)frames, n_freq,
                       (layout == KPR_CHANNELS_LAST && channels > 1) ? 1 : 0, fb, n_filt, out);
    return launch_check("k_filterbank_f64");
}

static int run_mag_to_db_f64(const double* x, int64_t n_items, int64_t item_size, double ref_value, double amin,
                             double dynamic_range, double* out, kpr_stream_t stream) {
    if (n_items < 0 || item_size < 0) return fail(KPR_E_BADARG, "negative size");
    if (int e = check_db_values(ref_value, amin, dynamic_range)) return e;
    if (n_items == 0 || item_size == 0) return 0;
    if (!x || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    if (n_items > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "float64 decibel: more than 2^31 - 1 items");
    const double ref_term = 10.0 * std::log10(std::max(amin, ref_value));
    hipLaunchKernelGGL(k_db_f64, dim3((unsigned)n_items), dim3(1024), 0, (hipStream_t)stream, x,
                       (long long)item_size, amin, ref_term, dynamic_range, out);
    return launch_check("k_db_f64");
}

// ---- float32 MagnitudeToDecibel: statistics, the log pass, the clamp (the helpers it shares with the fused mel: kpr_host_mel.h) ----
static int64_t db_workspace_bytes(int64_t n_items) {
    if (n_items < 0) return -1;
    return 256 + (int64_t)sizeof(unsigned) * 2 * std::max<int64_t>(1, n_items);
}

static int run_mag_to_db_f32(const float* x, int64_t n_items, int64_t item_size, const kpr_db_params* db, float* out,
                             void* workspace, int64_t workspace_bytes, kpr_stream_t stream) {
    if (!db) return fail(KPR_E_BADARG, "db params are NULL");
    kpr_db_params p = *db;
    p.enabled = 1;
    if (int e = check_db(&p)) return e;
    if (n_items < 0 || item_size < 0) return fail(KPR_E_BADARG, "negative size");
    if (n_items == 0 || item_size == 0) return 0;
    if (!x || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    if (!workspace || workspace_bytes < db_workspace_bytes(n_items))
        return fail(KPR_E_WORKSPACE, "db workspace: need %lld bytes", (long long)db_workspace_bytes(n_items));
    hipStream_t st = (hipStream_t)stream;
    DbDev dbd = make_db(&p);
    unsigned* stats = reinterpret_cast<unsigned*>(workspace);
    if (int e = stats_init(stats, n_items, st)) return e;
    int chunks = db_chunks(n_items, item_size);
    if (opt(OPT_DB_CHUNKS) > 0) chunks = opt(OPT_DB_CHUNKS);
    // (aligned bases: 16-byte accesses on the aligned middle of every chunk)
    with_vec<4>(((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0, [&](auto v) {
        hipLaunchKernelGGL(k_db_log<v>, dim3((unsigned)(n_items * chunks)), dim3(256), 0, st, x, (long long)item_size, chunks, dbd, stats, out);
    });
    if (int e = launch_check("k_db_log")) return e;
    return db_clamp(out, n_items, item_size, dbd.dyn, stats, st);
}

}  // namespace kpr
