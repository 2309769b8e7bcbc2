// kpr_host_fb_wgrad.h -- host side of the filterbank weight gradient (kpr_fb_wgrad_kernels.h): the launch plan (rows per chunk,
// LDS pitches, slabs, column passes), the workspace size, the argument checks and the one or two launches.  Option
// "fb_wgrad_rows": 0 automatic, n = at most n rows per slab, rounded up to the chunk (tests: the slab seam and the reduce launch
// at small shapes).  Part of the single translation unit kapre_hip.hip (after kpr_host.h; not stand-alone).
#pragma once

namespace kpr {

struct FbWgradPlan {
    int c;                              // channels folded into a row (channels_last), else 1
    int kc, px, pg;                     // rows per chunk; floats per staged row of x and of g
    int ftiles, passes;
    long long chunks, cps, n_slabs, S;  // chunks of kc rows; chunks per slab; slabs; rows per slab = cps kc
    size_t lds;
};

// Words of one bank (32 banks) that a fragment read touches at most in either half of the wave (a 4-byte read is served 32 lanes
// at a time): lane (i, kq) reads word kq pitch + i stride
static int fb_wgrad_bank_load(int pitch, int stride) {
    int worst = 0;
    for (int half = 0; half < 64; half += 32) {
        int load[32] = {0};
        for (int l = half; l < half + 32; ++l) worst = std::max(worst, ++load[(unsigned)((l >> 4) * pitch + (l & 15) * stride) & 31]);
    }
    return worst;
}
// the smallest pitch >= width, a multiple of 4 (16-byte stores), with the least bank load
static int fb_wgrad_pitch(int width, int stride) {
    const int base = (width + 3) & ~3;
    int best = base;
    for (int p = base + 4; p < base + 32; p += 4)
        if (fb_wgrad_bank_load(p, stride) < fb_wgrad_bank_load(best, stride)) best = p;
    return best;
}

// rows: the rows of the reduction -- batch x channels x frames (channels_first), batch x frames (channels_last)
static int fb_wgrad_plan(int64_t rows, int n_freq, int n_filt, int channels, int layout, FbWgradPlan* p) {
    if (rows < 0 || n_freq <= 0 || n_filt <= 0 || channels <= 0)
        return fail(KPR_E_BADARG, "filterbank_wgrad: bad sizes (rows %lld, n_freq %d, n_filt %d, channels %d)", (long long)rows, n_freq,
                    n_filt, channels);
    if ((unsigned)layout > 1u) return fail(KPR_E_BADARG, "filterbank_wgrad: bad layout enum %d", layout);
    p->c = layout == KPR_CHANNELS_LAST ? channels : 1;
    // a lane holds kWgSlotFloats floats of each operand of the chunk in flight: (kc / 4) rows x ceil(width / 64) columns
    const long long xw = (long long)kWgTF * p->c, gw = (long long)((std::min(n_filt, kWgNF) + 15) & ~15) * p->c;
    p->kc = 0;
    for (int kc = 16; kc >= 4 && !p->kc; kc /= 2)
        if ((xw + 63) / 64 * kc <= 4 * kWgSlotFloats && (gw + 63) / 64 * kc <= 4 * kWgSlotFloats) p->kc = kc;
    if (!p->kc)
        return fail(KPR_E_UNSUPPORTED, "filterbank_wgrad: %d interleaved channels x %d filters: four rows of a tile exceed the "
                    "registers that stage them", p->c, std::min(n_filt, kWgNF));
    p->px = fb_wgrad_pitch((int)xw, p->c);
    p->pg = fb_wgrad_pitch((int)gw, p->c);
    p->lds = sizeof(float) * 2 * (size_t)p->kc * (p->px + p->pg);
    p->ftiles = (n_freq + kWgTF - 1) / kWgTF;
    p->passes = (n_filt + kWgNF - 1) / kWgNF;
    p->chunks = (rows + p->kc - 1) / p->kc;
    if (opt(OPT_FB_WGRAD_ROWS) > 0) {
        p->cps = (opt(OPT_FB_WGRAD_ROWS) + p->kc - 1) / p->kc;
    } else {
        // about 512 workgroups, a slab of at least eight chunks: a function of the shape alone
        const long long want = (512 + (long long)p->ftiles * p->passes - 1) / ((long long)p->ftiles * p->passes);
        p->cps = std::max<long long>(8, (p->chunks + want - 1) / want);
    }
    p->cps = std::max<long long>(1, std::min(p->cps, p->chunks));
    p->n_slabs = (p->chunks + p->cps - 1) / p->cps;
    p->S = p->cps * p->kc;
    if (p->S > 0x7fffffffLL || p->n_slabs * p->ftiles * p->passes > 0x7fffffffLL)
        return fail(KPR_E_UNSUPPORTED, "filterbank_wgrad: %lld rows in %lld slabs x %d tiles x %d passes: too many", (long long)rows,
                    p->n_slabs, p->ftiles, p->passes);
    return 0;
}

static int64_t fb_wgrad_workspace_bytes(int64_t rows, int n_freq, int n_filt, int channels, int layout) {
    FbWgradPlan p;
    if (fb_wgrad_plan(rows, n_freq, n_filt, channels, layout, &p)) return -1;
    return p.n_slabs > 1 ? (int64_t)sizeof(float) * p.n_slabs * n_freq * n_filt : 0;
}

template <int VX, int VG>
static void launch_fb_wgrad(const FbWgradArgs& a, int kc, long long grid, size_t lds, hipStream_t st) {
    const dim3 g((unsigned)grid), b(kWgThreads);
    if (kc == 16) hipLaunchKernelGGL((k_fb_wgrad<VX, VG, 4>), g, b, lds, st, a);
    else if (kc == 8) hipLaunchKernelGGL((k_fb_wgrad<VX, VG, 2>), g, b, lds, st, a);
    else hipLaunchKernelGGL((k_fb_wgrad<VX, VG, 1>), g, b, lds, st, a);
}

static int run_fb_wgrad(const float* x, const float* g, int64_t batch, int channels, int64_t frames, int n_freq, int n_filt, int layout,
                        void* ws, int64_t ws_bytes, float* gw, kpr_stream_t stream) {
    if (batch < 0 || frames < 0) return fail(KPR_E_BADARG, "filterbank_wgrad: bad batch / frames");
    if (channels <= 0 || (unsigned)layout > 1u || n_freq <= 0 || n_filt <= 0)
        return fail(KPR_E_BADARG, "filterbank_wgrad: bad channels / n_freq / n_filt / layout");
    const bool cl = layout == KPR_CHANNELS_LAST;
    if (frames && batch > 0x7fffffffffffffffLL / frames / channels) return fail(KPR_E_UNSUPPORTED, "filterbank_wgrad: too many rows");
    const int64_t rows = batch * frames * (cl ? 1 : channels);
    FbWgradPlan p;
    if (int e = fb_wgrad_plan(rows, n_freq, n_filt, channels, layout, &p)) return e;
    const long long n = (long long)n_freq * n_filt;
    const size_t need = p.n_slabs > 1 ? sizeof(float) * (size_t)p.n_slabs * n : 0;
    const uintptr_t xb = (uintptr_t)rows * p.c * n_freq * 4, gb = (uintptr_t)rows * p.c * n_filt * 4;
    if (int e = check_ptrs("filterbank_wgrad: ", {{"x", x, xb, 4, rows == 0, false},
                                                   {"g", g, gb, 4, rows == 0, false},
                                                   {"workspace", ws, need, 16, need == 0, true},
                                                   {"gw", gw, (uintptr_t)n * 4, 4, false, true}}))
        return e;
    if (need && (ws_bytes < 0 || (size_t)ws_bytes < need))
        return fail(KPR_E_WORKSPACE, "workspace of %zu bytes needed (kpr_filterbank_wgrad_workspace_bytes), got %lld", need,
                    (long long)ws_bytes);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned rgrid = (unsigned)std::min<long long>((n + 255) / 256, 4096);
    if (rows == 0) {                                                     // no rows: the zero matrix
        hipLaunchKernelGGL(k_fb_wgrad_reduce, dim3(rgrid), dim3(256), 0, st, (const float*)nullptr, gw, n, 0);
        return launch_check("k_fb_wgrad_reduce");
    }
    FbWgradArgs a;
    a.x = x; a.g = g; a.out = p.n_slabs > 1 ? static_cast<float*>(ws) : gw;
    a.R = rows; a.chunks = p.chunks;
    a.xrow = (long long)n_freq * p.c; a.grow = (long long)n_filt * p.c;
    a.n_freq = n_freq; a.n_filt = n_filt; a.c = p.c;
    a.ftiles = p.ftiles; a.n_slabs = (int)p.n_slabs;
    a.cps = (int)p.cps;
    a.px = p.px; a.pg = p.pg;
    // 16-byte loads: every row and every tile starts on a 16-byte boundary and ends on one.  (x alone: the instance with 4-byte loads)
    const bool vg = (((uintptr_t)g) & 15) == 0 && a.grow % 4 == 0, vx = vg && (((uintptr_t)x) & 15) == 0 && a.xrow % 4 == 0;
    const long long grid = p.n_slabs * p.ftiles * p.passes;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_fb_wgrad<x%d,g%d>: grid %lld = %d f-tiles x %lld slabs x %d passes, lds %zu B, %lld rows of "
                "%d channel(s) in chunks of %d, %lld chunks per slab (S = %lld), pitches %d / %d\n", vx ? 4 : 1, vg ? 4 : 1, grid,
                p.ftiles, p.n_slabs, p.passes, p.lds, (long long)rows, p.c, p.kc, p.cps, p.S, p.px, p.pg);
    if (vx) launch_fb_wgrad<4, 4>(a, p.kc, grid, p.lds, st);
    else if (vg) launch_fb_wgrad<1, 4>(a, p.kc, grid, p.lds, st);
    else launch_fb_wgrad<1, 1>(a, p.kc, grid, p.lds, st);
    if (int e = launch_check(vx ? "k_fb_wgrad<x4,g4>" : vg ? "k_fb_wgrad<x1,g4>" : "k_fb_wgrad<x1,g1>")) return e;
    if (p.n_slabs > 1) {
        hipLaunchKernelGGL(k_fb_wgrad_reduce, dim3(rgrid), dim3(256), 0, st, (const float*)ws, gw, n, (int)p.n_slabs);
        return launch_check("k_fb_wgrad_reduce");
    }
    return 0;
}

}  // namespace kpr
