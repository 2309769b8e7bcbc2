// kpr_host_mix.h -- host side of kpr_mix_kernels.h and of k_noise_draw (kpr_augment_kernels.h): argument checks, the choice between
// the streamed and the resident form, the launches of AddNoise and of its backward pass (augmentation.AddNoise, backend.add_noise).
// Part of the single translation unit kapre_hip.hip (after kpr_host.h).
#pragma once

namespace kpr {

enum { MIX_STREAMED = 1, MIX_RESIDENT = 2 };

struct MixDims {
    long long n;             // floats per item
    long long chunks;        // of the streamed form
};

static int mix_dims(int64_t batch, int channels, int64_t time, int layout, MixDims* d) {
    if (batch < 0 || channels < 1 || time < 1)
        return fail(KPR_E_BADARG, "bad batch/channels/time (%lld, %d, %lld)", (long long)batch, channels, (long long)time);
    if ((unsigned)layout > 1u) return fail(KPR_E_BADARG, "bad layout %d", layout);
    if (time >= (1LL << 30) / channels + ((1LL << 30) % channels != 0))
        return fail(KPR_E_UNSUPPORTED, "time * channels = %lld elements per batch item: 2^30 or more is not supported",
                    (long long)(time * (long long)channels));
    d->n = time * (long long)channels;
    d->chunks = (d->n + kMixChunk - 1) / kMixChunk;
    if (batch * d->chunks > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "too many items: batch = %lld", (long long)batch);
    return 0;
}

// Which form a call takes under option "addnoise_variant": 1 streams every shape; 2 keeps every item of at most kMixResMax floats in
// registers; 0 does so for batches of at least kMixResMinItems.  The resident form is one workgroup per item and one workgroup per
// compute unit at a time (its registers leave room for no second one), so it needs a workgroup for each of the 256 compute units
// before its single read pays: profiles/addnoise_times.md, items of 44100 floats forward / backward, streamed against resident --
// 256 items 30.1 / 33.9 against 24.5 / 26.2 us, 128 items 18.0 / 18.7 against 19.4 / 17.2, 64 items 13.7 / 11.4 against 17.7 / 13.9,
// 8 items 9.5 / 7.4 against 16.2 / 10.7.
constexpr long long kMixResMinItems = 256;
static int mix_form(const MixDims& d, long long batch) {
    const int v = opt(OPT_ADDNOISE_VARIANT);
    if (v == 1 || d.n > kMixResMax) return MIX_STREAMED;
    return (v == 2 || batch >= kMixResMinItems) ? MIX_RESIDENT : MIX_STREAMED;
}

static int mix_plan(int64_t batch, int channels, int64_t time, int layout, int* out) {
    if (!out) return fail(KPR_E_BADARG, "out is NULL");
    MixDims d;
    if (int e = mix_dims(batch, channels, time, layout, &d)) return e;
    out[0] = kMixChunk;
    out[1] = (int)d.chunks;
    out[2] = kMixResMax;
    out[3] = mix_form(d, batch);
    return 0;
}

static int64_t mix_workspace_bytes(int64_t batch, int channels, int64_t time, int layout) {
    MixDims d;
    if (mix_dims(batch, channels, time, layout, &d)) return -1;
    return (int64_t)(batch * d.chunks * 16);
}

static int run_noise_draw(int32_t* table, int64_t n_items, int n_noise, const int32_t* lengths, double snr_lo, double snr_hi,
                          void* state, kpr_stream_t stream) {
    if (n_items < 0 || n_noise < 1) return fail(KPR_E_BADARG, "bad n_items / n_noise (%lld, %d)", (long long)n_items, n_noise);
    if (!std::isfinite(snr_lo) || !std::isfinite(snr_hi) || snr_lo > snr_hi)
        return fail(KPR_E_BADARG, "snr range [%g, %g]: both ends must be finite and ordered", snr_lo, snr_hi);
    if (n_items > (1LL << 20))
        return fail(KPR_E_UNSUPPORTED, "%lld items: the one-workgroup draw takes at most 2^20", (long long)n_items);
    if (!state) return fail(KPR_E_BADARG, "state must not be NULL");
    if (!lengths) return fail(KPR_E_BADARG, "lengths must not be NULL");
    if (n_items > 0 && !table) return fail(KPR_E_BADARG, "table must not be NULL");
    if (((uintptr_t)table) & 15) return fail(KPR_E_BADARG, "table must be 16-byte aligned");
    if (ranges_overlap(table, (uintptr_t)n_items * 16, state, 16) || ranges_overlap(table, (uintptr_t)n_items * 16, lengths, (uintptr_t)n_noise * 4))
        return fail(KPR_E_BADARG, "table overlaps state / lengths");
    // (a call without items still advances the counter: one launch, one step of the stream)
    hipLaunchKernelGGL(k_noise_draw, dim3(1), dim3(1024), 0, (hipStream_t)stream, table, (int)n_items, (unsigned)n_noise, lengths,
                       snr_lo, snr_hi - snr_lo, (unsigned long long*)state);
    return launch_check("k_noise_draw");
}

template <bool BWD>
static void launch_mix(int form, bool vec, long long batch, const MixArgs& m, hipStream_t st) {
    with_vec<4>(vec, [&](auto v) {
        if (form == MIX_RESIDENT) {
            hipLaunchKernelGGL((k_mix_res<v, BWD>), dim3((unsigned)batch), dim3(1024), 0, st, m);
        } else {
            const dim3 grid((unsigned)(batch * m.chunks));
            hipLaunchKernelGGL((k_mix_sums<v, BWD>), grid, dim3(256), 0, st, m);
            hipLaunchKernelGGL((k_mix_apply<v, BWD>), grid, dim3(256), 0, st, m);
        }
    });
}

// forward: a = x, b = NULL, stats written; backward: a = gy, b = x, stats_in = the forward's rows, stats may be NULL
static int run_add_noise(bool bwd, const float* a, const float* b, int64_t batch, int channels, int64_t time, int layout,
                         const float* noise, int n_noise, int64_t stride, const int32_t* lengths, const int32_t* table,
                         const double* stats_in, float* out, double* stats, void* workspace, size_t workspace_bytes,
                         kpr_stream_t stream) {
    MixDims d;
    if (int e = mix_dims(batch, channels, time, layout, &d)) return e;
    if (n_noise < 1 || stride < 1 || stride > 0x7fffffffLL)
        return fail(KPR_E_BADARG, "bad noise bank (n_noise %d, stride %lld)", n_noise, (long long)stride);
    if (batch == 0) return 0;
    if (!a || !out || (bwd && !b)) return fail(KPR_E_BADARG, bwd ? "gy / x / gx must not be NULL" : "x / out must not be NULL");
    if (!noise || !lengths || !table) return fail(KPR_E_BADARG, "noise / lengths / table must not be NULL");
    if (bwd ? !stats_in : !stats) return fail(KPR_E_BADARG, "stats must not be NULL");
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)out) | ((uintptr_t)noise) | ((uintptr_t)lengths) | ((uintptr_t)table)) & 3)
        return fail(KPR_E_BADARG, "pointers must be 4-byte aligned");
    if ((((uintptr_t)stats) | ((uintptr_t)stats_in) | ((uintptr_t)workspace)) & 7)
        return fail(KPR_E_BADARG, "stats / workspace must be 8-byte aligned");
    const uintptr_t nb = (uintptr_t)batch * (uintptr_t)d.n * 4, ns = (uintptr_t)batch * 32;
    if (ranges_overlap(out, nb, a, nb) || ranges_overlap(out, nb, b, nb))
        return fail(KPR_E_BADARG, bwd ? "gx overlaps gy / x (there is no in-place form)" : "x and out overlap (there is no in-place form)");
    if (ranges_overlap(out, nb, noise, (uintptr_t)n_noise * (uintptr_t)stride * 4) || ranges_overlap(out, nb, lengths, (uintptr_t)n_noise * 4) ||
        ranges_overlap(out, nb, table, (uintptr_t)batch * 16) || ranges_overlap(out, nb, stats_in, ns) || ranges_overlap(out, nb, stats, ns))
        return fail(KPR_E_BADARG, "out overlaps noise / lengths / table / stats");
    const int form = mix_form(d, batch);
    const uintptr_t need = (uintptr_t)batch * (uintptr_t)d.chunks * 16;
    if (form == MIX_STREAMED) {
        if (!workspace || workspace_bytes < need)
            return fail(KPR_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, (size_t)need);
        if (ranges_overlap(workspace, need, out, nb) || ranges_overlap(workspace, need, a, nb) || ranges_overlap(workspace, need, b, nb) ||
            ranges_overlap(workspace, need, stats, ns) || ranges_overlap(workspace, need, stats_in, ns))
            return fail(KPR_E_BADARG, "workspace overlaps x / out / stats");
    }
    MixArgs m;
    m.a = a; m.b = b; m.noise = noise; m.lengths = lengths; m.table = table; m.out = out; m.stats = stats; m.stats_in = stats_in;
    m.ws = (double*)workspace;
    m.n = (unsigned)d.n; m.C = (unsigned)channels; m.T = (unsigned)time;
    m.cf = (layout == KPR_CHANNELS_FIRST || channels == 1) ? 1u : 0u;
    m.n_noise = n_noise; m.chunks = (int)d.chunks; m.stride = stride;
    bool vec = ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)out)) & 15) == 0;
    if (form == MIX_RESIDENT) vec = vec && (d.n & 3) == 0;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] add_noise%s: %s form, %lld items of %lld floats, %lld chunks, %s accesses\n", bwd ? " (backward)" : "",
                form == MIX_RESIDENT ? "resident" : "streamed", (long long)batch, d.n, d.chunks, vec ? "16-byte" : "4-byte");
    if (bwd) launch_mix<true>(form, vec, batch, m, (hipStream_t)stream);
    else launch_mix<false>(form, vec, batch, m, (hipStream_t)stream);
    const char* detail = bwd ? "bwd" : "fwd";
    if (form == MIX_RESIDENT) return launch_check("k_mix_res", vec ? 4 : 1, detail);
    if (int e = launch_check("k_mix_sums", vec ? 4 : 1, detail)) return e;
    return launch_check("k_mix_apply", vec ? 4 : 1, detail);
}

}  // namespace kpr
