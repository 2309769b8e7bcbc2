// kpr_host_convolve.h -- host side of kpr_spec_fir_kernels.h: argument checks, the bucket and the one launch of the spectral FIR
// (kapre_amd.Convolve, backend.fftconvolve).  Part of the single translation unit kapre_hip.hip (after kpr_host.h).
#pragma once

namespace kpr {

// out[0 ... 2] = rows per wave, waves per workgroup, bucket: the same tiling for every shape, the bucket from n_part alone
static int spec_fir_plan(int64_t frames_out, int64_t inner, int n_part, int* out) {
    if (!out) return fail(KPR_E_BADARG, "out is NULL");
    if (frames_out < 0 || inner < 0) return fail(KPR_E_BADARG, "bad frames_out/inner");
    if (n_part < 1 || n_part > kFirMaxPart) return fail(KPR_E_BADARG, "n_part = %d outside [1, %d]", n_part, kFirMaxPart);
    out[0] = kFirRows;
    out[1] = kFirWaves;
    out[2] = fir_bucket(n_part);
    return 0;
}

template <int V>
static void launch_spec_fir(int bucket, const ColLaunch& l, const FirArgs& a, hipStream_t st) {
    switch (bucket) {
        case 4: hipLaunchKernelGGL((k_spec_fir<V, 4>), l.grid, l.block, 0, st, a); break;
        case 8: hipLaunchKernelGGL((k_spec_fir<V, 8>), l.grid, l.block, 0, st, a); break;
        case 16: hipLaunchKernelGGL((k_spec_fir<V, 16>), l.grid, l.block, 0, st, a); break;
        default: hipLaunchKernelGGL((k_spec_fir<V, 32>), l.grid, l.block, 0, st, a); break;
    }
}

// x: (outer, frames_in, inner) complex64 -> out: (outer, frames_out, inner); h: (n_ir, n_part, inner / band_div) complex64 on the
// device; idx: `items` device int32 or NULL, never read here
static int run_spec_fir(const void* x, int64_t outer, int64_t frames_in, int64_t inner, int band_div, const void* h, int n_ir, int n_part,
                        const int32_t* idx, int64_t items, void* out, int64_t frames_out, kpr_stream_t stream) {
    if (outer < 0 || frames_in < 0 || frames_out < 0 || inner < 0) return fail(KPR_E_BADARG, "bad outer/frames_in/frames_out/inner");
    if (n_part < 1 || n_part > kFirMaxPart) return fail(KPR_E_BADARG, "n_part = %d outside [1, %d]", n_part, kFirMaxPart);
    if (n_ir < 1 || band_div < 1 || items < 0) return fail(KPR_E_BADARG, "bad n_ir/band_div/items (%d, %d, %lld)", n_ir, band_div, (long long)items);
    if (inner % band_div != 0) return fail(KPR_E_BADARG, "inner = %lld is no multiple of band_div = %d", (long long)inner, band_div);
    if (outer > 0 && (items < 1 || outer % items != 0))
        return fail(KPR_E_BADARG, "outer = %lld is no multiple of items = %lld", (long long)outer, (long long)items);
    const long long lim = 1LL << 30;
    if (inner > 0 && (frames_in > (lim - 1) / inner || frames_out > (lim - 1) / inner))
        return fail(KPR_E_UNSUPPORTED, "spectral FIR: %lld -> %lld frames x %lld columns: 2^30 elements or more per outer item are not "
                    "supported", (long long)frames_in, (long long)frames_out, (long long)inner);
    if (outer == 0 || frames_out == 0 || inner == 0) return 0;
    if ((!x && frames_in > 0) || !h || !out) return fail(KPR_E_BADARG, "x / h / out must not be NULL");
    if ((((uintptr_t)x) | ((uintptr_t)out) | ((uintptr_t)h)) & 7) return fail(KPR_E_BADARG, "x / h / out must be 8-byte aligned");
    if (((uintptr_t)idx) & 3) return fail(KPR_E_BADARG, "idx must be 4-byte aligned");
    if (outer > (1LL << 59) / (std::max<int64_t>(std::max(frames_in, frames_out), 1) * inner))        // (the byte counts below stay in 64 bits)
        return fail(KPR_E_UNSUPPORTED, "spectral FIR: outer = %lld items of that size are not supported", (long long)outer);
    const int64_t n_freq = inner / band_div;
    if (n_freq > 0x7fffffffLL / ((int64_t)n_ir * n_part))
        return fail(KPR_E_UNSUPPORTED, "spectral FIR: a table of %d x %d x %lld values is not supported", n_ir, n_part, (long long)n_freq);
    {
        const uintptr_t nx = (uintptr_t)outer * frames_in * inner * 8, no = (uintptr_t)outer * frames_out * inner * 8;
        const uintptr_t nh = (uintptr_t)n_ir * n_part * n_freq * 8, ni = (uintptr_t)items * 4;
        if (ranges_overlap(out, no, x, nx)) return fail(KPR_E_BADARG, "x and out overlap (there is no in-place form)");
        if (ranges_overlap(out, no, h, nh) || ranges_overlap(out, no, idx, ni)) return fail(KPR_E_BADARG, "h / idx overlap out");
    }
    ColLaunch l;
    if (int e = col_launch(outer, inner, 2, kFirWaves, ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0, &l)) return e;
    const long long n_super = (frames_out + kFirRows * kFirWaves - 1) / (kFirRows * kFirWaves);
    l.grid.y = (unsigned)std::min<long long>(n_super, 65535);
    FirArgs a;
    a.x = (const float2*)x; a.out = (float2*)out; a.h = (const float2*)h; a.idx = idx;
    a.frames_in = (int)frames_in; a.frames_out = (int)frames_out;
    a.n_part = n_part; a.n_ir = n_ir; a.n_freq = (int)n_freq;
    a.band_div = (unsigned)band_div;
    a.outer_per_item = (unsigned)(outer / items);
    a.inner = l.inner;
    a.groups_per_item = l.groups_per_item;
    a.n_groups = l.n_groups;
    const int bucket = fir_bucket(n_part);
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_spec_fir<%d,%d>: grid %u x %u, %d lanes, %d rows per wave; %lld -> %lld frames, %d partitions, "
                "%d filters%s\n", l.wide ? 2 : 1, bucket, l.grid.x, l.grid.y, 64 * kFirWaves, kFirRows, (long long)frames_in,
                (long long)frames_out, n_part, n_ir, idx ? ", indexed" : "");
    if (l.wide) launch_spec_fir<2>(bucket, l, a, (hipStream_t)stream);
    else launch_spec_fir<1>(bucket, l, a, (hipStream_t)stream);
    char detail[16];
    snprintf(detail, sizeof detail, "p%d", bucket);
    return launch_check("k_spec_fir", l.wide ? 2 : 1, detail);
}

}  // namespace kpr
