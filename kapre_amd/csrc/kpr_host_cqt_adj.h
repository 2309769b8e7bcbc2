// kpr_host_cqt_adj.h -- host side of the adjoint of the constant-Q transform (kpr_cqt_adj_kernels.h): the fragment index and the
// table size from the bins' lengths and the hop, the launch plan (hop blocks per run, rows staged at once, the split into work
// items), the argument checks and the one launch.  Option "cqt_adjoint_rows": 0 automatic, n caps the cotangent rows staged at
// once (at least a run; tests: the chunked reduction at small shapes).
// Part of the single translation unit kapre_hip.hip (after kpr_host_cqt.h: cqt_plan, cqt_pick_pad; not stand-alone).
#pragma once

namespace kpr {

struct CqtAdjPlan {
    int F, RTG, gshift;                 // hop blocks per run; row tiles per item; row groups per r-tile = 1 << gshift
    int R, Rt, T, D;                    // r-tiles of a hop; those a tap reaches; column tiles; d < D
    int dc, nchunks, rows, pitch;       // d per chunk; rows staged at once; floats per row
    int items, passes;
    long long nfrag, table_floats;
    size_t lds;
};

// the d range of r-tile rt and a tile's taps [lo, hi): the fragments d with [d hop + 16 rt, + w) meeting it, w the r-tile's width
static void cqt_adj_range(int lo, int hi, int hop, int rt, int* dlo, int* dn) {
    const long long w = std::min(16, hop - 16 * rt), first = (long long)lo - 16 * rt - w + 1, last = (long long)hi - 1 - 16 * rt;
    *dlo = first > 0 ? (int)((first + hop - 1) / hop) : 0;
    *dn = last < 0 ? 0 : std::max(0, (int)(last / hop) + 1 - *dlo);
}

static int cqt_adj_plan(const int32_t* lengths, int K, int hop, CqtAdjPlan* p) {
    CqtPlan fp;                                                          // the forward's checks of lengths and hop, and its tiles
    if (int e = cqt_plan(lengths, K, hop, &fp)) return e;
    const int L = lengths[0];
    p->T = (int)fp.tiles.size();
    p->R = (int)(((long long)hop + 15) / 16);
    p->Rt = (std::min(hop, L) + 15) / 16;
    p->D = (int)((L + (long long)hop - 1) / hop);
    p->nfrag = 0;
    for (int rt = 0; rt < p->Rt; ++rt)
        for (const CqtTile& t : fp.tiles) {
            int dlo, dn;
            cqt_adj_range(t.lo, t.hi, hop, rt, &dlo, &dn);
            p->nfrag += dn;
        }
    p->table_floats = 4LL * p->Rt * p->T + 256 * p->nfrag;
    if (p->nfrag > 0x7fffffffLL / 256) return fail(KPR_E_UNSUPPORTED, "cqt_adjoint: %lld fragments: the table is too large", p->nfrag);
    // a row: 16 T floats and the pad that spreads the 16-byte operand reads over the banks
    p->pitch = 16 * p->T + cqt_pick_pad(16 * p->T, true);
    const int fit = kCqtLdsFloats / p->pitch;
    // the largest run whose whole window fits; else the largest that leaves as many rows again for a chunk; else 16
    p->F = 0;
    for (int F = 64; F >= 16 && !p->F; F /= 2)
        if (F + p->D - 1 <= fit) p->F = F;
    for (int F = 64; F >= 32 && !p->F; F /= 2)
        if (2 * F <= fit) p->F = F;
    if (!p->F) p->F = 16;
    if (fit < p->F) return fail(KPR_E_UNSUPPORTED, "cqt_adjoint: a run of 16 rows of %d floats does not fit the LDS", p->pitch);
    const int cap = opt(OPT_CQT_ADJOINT_ROWS) > 0 ? std::max(opt(OPT_CQT_ADJOINT_ROWS), p->F) : fit;
    p->dc = std::min(p->D, std::min(fit, cap) - p->F + 1);
    p->nchunks = (p->D + p->dc - 1) / p->dc;
    p->rows = p->F + p->dc - 1;
    p->lds = (size_t)p->rows * p->pitch * sizeof(float);
    // items: row groups as large as leave every wave one (a fragment in registers serves the group's row tiles)
    const int RT = p->F / 16;
    p->RTG = 1;
    for (int g = std::min(4, RT); g > 1; g /= 2)
        if ((long long)p->R * (RT / g) >= kCqtWaves) { p->RTG = g; break; }
    p->gshift = RT / p->RTG == 4 ? 2 : RT / p->RTG == 2 ? 1 : 0;
    p->items = p->R << p->gshift;
    p->passes = (p->items + kAdjItems * kCqtWaves - 1) / (kAdjItems * kCqtWaves);
    return 0;
}

template <int RTG>
static int launch_cqt_adj(const CqtAdjArgs& a, long long grid, size_t lds, hipStream_t st) {
    static LdsOptIn optin;
    if (int e = allow_big_lds(optin, reinterpret_cast<const void*>(&k_cqt_adj<RTG>))) return e;
    hipLaunchKernelGGL((k_cqt_adj<RTG>), dim3((unsigned)grid), dim3(kCqtThreads), lds, st, a);
    return 0;
}

static int run_cqt_adjoint(const void* g, int64_t batch, int channels, int64_t time, int layout, const int32_t* lengths, int n_bins,
                           const float* table, int64_t table_floats, int hop, int center, int pad_end, int g_layout, float* gx,
                           kpr_stream_t stream) {
    if (int e = check_series("cqt_adjoint: bad batch/channels/time/layout", batch, channels, time, layout | g_layout, true)) return e;
    CqtAdjPlan p;
    if (int e = cqt_adj_plan(lengths, n_bins, hop, &p)) return e;
    if (table_floats != p.table_floats)
        return fail(KPR_E_BADARG, "cqt_adjoint: the packed table of these lengths and this hop has %lld floats, got %lld", p.table_floats,
                    (long long)table_floats);
    if (int e = check_reach("cqt_adjoint", time, 1, 31)) return e;
    const int L = lengths[0];
    const int64_t frames = std::max<int64_t>(0, center ? 1 + time / hop : frame_count(time, L, hop, pad_end));
    if (batch == 0 || channels == 0 || time == 0) return 0;
    // gx: the series; g: one (frames, n_bins) plane per series, a bin `sg.stride` elements from the next.  No frames: gx is zeros
    const Series sx = series_of(layout, channels, time, true), sg = series_of(g_layout, channels, frames * n_bins, true);
    if (int e = check_ptrs("cqt_adjoint: ", {{"g", g, (uintptr_t)batch * sg.item * 8, 8, frames == 0, false},
                                             {"table", table, (uintptr_t)table_floats * 4, 16, false, false},
                                             {"gx", gx, (uintptr_t)batch * sx.item * 4, 4, false, true}}))
        return e;
    const int origin = center ? -(L / 2) : 0;
    const long long blocks = (time - origin + hop - 1) / hop, runs = (blocks + p.F - 1) / p.F;
    long long grid;
    if (int e = grid_of(runs, batch, channels, "cqt_adjoint", &grid)) return e;
    if (runs * p.F >= (1LL << 31)) return fail(KPR_E_UNSUPPORTED, "cqt_adjoint: %lld hop blocks: 2^31 or more are not supported", blocks);
    CqtAdjArgs a;
    a.g = static_cast<const float*>(g); a.table = reinterpret_cast<const f4*>(table); a.gx = gx;
    a.item = sx.item; a.chan = sx.chan; a.stride = sx.stride;
    a.g_item = sg.item; a.g_chan = sg.chan;
    a.g_t = n_bins * sg.stride; a.g_k = sg.stride;
    a.C = channels; a.time = (int)time; a.frames = (int)frames; a.runs = (int)runs; a.K = n_bins;
    a.hop = hop; a.origin = origin;
    a.T = p.T; a.Rt = p.Rt; a.nfrag = (int)p.nfrag;
    a.D = p.D; a.dc = p.dc; a.nchunks = p.nchunks; a.pitch = p.pitch;
    a.gshift = p.gshift; a.items = p.items; a.passes = p.passes;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_cqt_adj<g%d>: grid %lld, lds %zu B, runs of %d hop blocks, %d rows of %d floats at once, "
                "%d chunks of %d d (D = %d), %d r-tiles x %d row groups = %d items in %d passes, %d tiles, %lld fragments, "
                "table %lld floats\n", p.RTG, grid, p.lds, p.F, p.rows, p.pitch, p.nchunks, p.dc, p.D, p.R, 1 << p.gshift, p.items,
                p.passes, p.T, p.nfrag, p.table_floats);
    const hipStream_t st = (hipStream_t)stream;
    int e = p.RTG == 4 ? launch_cqt_adj<4>(a, grid, p.lds, st) : p.RTG == 2 ? launch_cqt_adj<2>(a, grid, p.lds, st)
                                                                             : launch_cqt_adj<1>(a, grid, p.lds, st);
    if (e) return e;
    return launch_check(p.RTG == 4 ? "k_cqt_adj<g4>" : p.RTG == 2 ? "k_cqt_adj<g2>" : "k_cqt_adj<g1>");
}

}  // namespace kpr
