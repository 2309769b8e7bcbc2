// kpr_host_cqt.h -- host side of the constant-Q transform (kpr_cqt_kernels.h): the tile ranges and the table size from the
// bins' lengths, the launch plan (frames per run, chunk, LDS form and skew, the phase list), the argument checks and the one
// launch.  Option "cqt_chunk": 0 automatic, n caps the taps staged at once (tests: the multi-chunk path at small shapes).
// Part of the single translation unit kapre_hip.hip (after kpr_host_ops.h: frame_count; not stand-alone).
#pragma once

namespace kpr {

struct CqtTile { int lo, hi, tab; };    // tap range [lo, hi), lo a multiple of 16; float4 index of its first step

struct CqtPlan {
    int RT;                             // F / 16
    int chunk;                          // taps staged at once at most (a multiple of 16)
    bool win, vec;
    int hopL, pad, pieces, red;
    unsigned magic;
    int items;                          // (phase, wave) slices that hold at least one step
    size_t lds;
    long long table_floats;
    std::vector<CqtTile> tiles;
    std::vector<CqtPhase> phases;
};

// Words of one bank that the 64 lanes of a step's operand read touch at most: lane (m, kq) reads words m pitch + 4 kq + e.
static int cqt_bank_load(int pitch, bool vec) {
    int worst = 0;
    for (int e0 = 0; e0 < (vec ? 1 : 4); ++e0) {                         // scalar: each e is a read of its own
        int load[32] = {0};
        for (int l = 0; l < 64; ++l)
            for (int e = e0; e < (vec ? 4 : e0 + 1); ++e) ++load[(unsigned)((l & 15) * pitch + 4 * (l >> 4) + e) & 31];
        for (int b = 0; b < 32; ++b) worst = std::max(worst, load[b]);
    }
    return worst;
}
static int cqt_pick_pad(int base, bool vec) {
    int best = 0, load = cqt_bank_load(base, vec);
    for (int pad = vec ? 4 : 1; pad < 32; pad += vec ? 4 : 1)
        if (cqt_bank_load(base + pad, vec) < load) { best = pad; load = cqt_bank_load(base + pad, vec); }
    return best;
}

// lengths[k] = N_k: N_0 = L <= 65536, non-increasing, at least 2.  Tile j = bins 8 j ... 8 j + 7, tap range of bin 8 j.
static int cqt_plan(const int32_t* lengths, int K, int hop, CqtPlan* p) {
    if (!lengths || K < 1) return fail(KPR_E_BADARG, "cqt: lengths must not be NULL and n_bins at least 1");
    if (hop < 1) return fail(KPR_E_BADARG, "cqt: hop must be at least 1, got %d", hop);
    const int L = lengths[0];
    if (L < 2 || L > 65536) return fail(KPR_E_BADARG, "cqt: the longest kernel must have 2 ... 65536 taps, got %d", L);
    for (int k = 0; k < K; ++k)
        if (lengths[k] < 2 || (k && lengths[k] > lengths[k - 1]))
            return fail(KPR_E_BADARG, "cqt: lengths must be non-increasing and at least 2 (bin %d: %d)", k, lengths[k]);
    long long tab = 0;
    int longest = 0;
    p->tiles.clear();
    for (int k = 0; k < K; k += kCqtTileBins) {
        const int off = (L - lengths[k]) / 2, lo = off & ~15;
        const int hi = std::min(L, lo + (off + lengths[k] - lo + 15) / 16 * 16);
        p->tiles.push_back({lo, hi, (int)tab});
        tab += (long long)((hi - lo + 15) / 16) * 64;
        longest = std::max(longest, (hi - lo + 15) / 16 * 16);
        if (lo < 0 || hi > L || hi <= lo || tab > 0x7fffffffLL / 4) return fail(KPR_E_BADARG, "cqt: tile %d has no valid tap range", k / 8);
    }
    p->table_floats = tab * 4;
    // the largest run whose staged samples fit: SPAN at F = 64, at F = 32, at F = 32 in chunks of at least 2048 taps; else WIN
    const int cap = opt(OPT_CQT_CHUNK) > 0 ? (opt(OPT_CQT_CHUNK) + 15) / 16 * 16 : longest;
    const int want = std::min(cap, longest);
    auto span_words = [&](int F, int chunk, int pad) -> long long {
        const long long last = (long long)(F - 1) * hop + chunk - 1;
        return (last + pad * (last / hop) + 1 + 3) / 4 * 4;
    };
    p->win = hop >= want;
    p->vec = p->win || hop % 4 == 0;
    p->RT = 0;
    if (!p->win) {
        p->pad = hop == 1 ? 0 : cqt_pick_pad(hop, p->vec);
        for (int F = 64; F >= 32 && !p->RT; F /= 2) {
            const long long room = kCqtLdsFloats - kCqtWaves * F * 16;
            if (span_words(F, want, p->pad) <= room) { p->RT = F / 16; p->chunk = want; }
            else if (F == 32) {
                int c = want;
                while (c >= 2048 && span_words(F, c, p->pad) > room) c -= 16;
                if (c >= 2048) { p->RT = 2; p->chunk = c; }
            }
        }
        if (!p->RT) { p->win = true; p->vec = true; }
    }
    if (p->win) {
        p->RT = 2;
        const int room = (kCqtLdsFloats - kCqtWaves * 32 * 16) / 32;     // floats per frame row
        p->chunk = std::min(want, (room - 28) & ~15);
        p->pad = cqt_pick_pad(p->chunk, true);
        p->hopL = p->chunk + p->pad;
        p->magic = 0;
        p->pieces = 32;
        p->red = 32 * p->hopL;
        p->pad = 0;                                                      // (the skew of a row start is in hopL; none inside a row)
    } else {
        p->hopL = hop;
        p->magic = hop == 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)hop) + 1u;
        p->pieces = 1;
        p->red = (int)span_words(16 * p->RT, p->chunk, p->pad);
    }
    p->lds = (size_t)(p->red + kCqtWaves * 16 * p->RT * 16) * sizeof(float);
    if (p->lds > (size_t)kCqtLdsFloats * 4) return fail(KPR_E_UNSUPPORTED, "cqt: the plan needs %zu bytes of LDS", p->lds);
    // phases: every tile in pieces of `chunk` taps; a piece that lies inside the staged taps is not staged again
    p->phases.clear();
    p->items = 0;
    int sc0 = 0, sclen = 0;
    for (size_t j = 0; j < p->tiles.size(); ++j) {
        const CqtTile& t = p->tiles[j];
        for (int a = t.lo; a < t.hi; a += p->chunk) {
            CqtPhase ph;
            ph.a = a; ph.hi = t.hi; ph.tile = (int)j;
            ph.nsteps = (std::min(a + p->chunk, t.hi) - a + 15) / 16;
            ph.tab = t.tab + (a - t.lo) / 16 * 64;
            ph.flags = a + p->chunk >= t.hi ? kCqtLast : 0;
            if (sclen == 0 || a < sc0 || a + ph.nsteps * 16 > sc0 + sclen) {
                sc0 = a; sclen = ph.nsteps * 16;
                ph.flags |= kCqtStage;
            }
            ph.c0 = sc0; ph.clen = sclen;
            p->phases.push_back(ph);
            p->items += std::min(ph.nsteps, kCqtWaves);
        }
    }
    if (p->phases.size() > (size_t)kCqtMaxPhases)
        return fail(KPR_E_UNSUPPORTED, "cqt: %zu phases (tiles x chunks): at most %d are supported", p->phases.size(), kCqtMaxPhases);
    return 0;
}

template <int RT, bool VEC, bool MAG>
static int launch_cqt(const CqtArgs& a, long long grid, size_t lds, hipStream_t st) {
    static LdsOptIn optin;
    if (int e = allow_big_lds(optin, reinterpret_cast<const void*>(&k_cqt<RT, VEC, MAG>))) return e;
    hipLaunchKernelGGL((k_cqt<RT, VEC, MAG>), dim3((unsigned)grid), dim3(kCqtThreads), lds, st, a);
    return 0;
}

static int run_cqt(const float* x, int64_t batch, int channels, int64_t time, int layout, const int32_t* lengths, int n_bins,
                   const float* table, int64_t table_floats, int hop, int center, int pad_end, int out_layout, int magnitude,
                   void* out, kpr_stream_t stream) {
    if (int e = check_series("cqt: bad batch/channels/time/layout", batch, channels, time, layout | out_layout, true)) return e;
    CqtPlan p;
    if (int e = cqt_plan(lengths, n_bins, hop, &p)) return e;
    if (table_floats != p.table_floats)
        return fail(KPR_E_BADARG, "cqt: the packed table of these lengths has %lld floats, got %lld", p.table_floats, (long long)table_floats);
    if (int e = check_reach("cqt", time, 1, 31)) return e;
    const int L = lengths[0];
    const int64_t frames = center ? 1 + time / hop : frame_count(time, L, hop, pad_end);
    if (batch == 0 || channels == 0 || frames <= 0) return 0;
    // x: the series; out: one (frames, n_bins) plane per series, a bin `so.stride` elements from the next
    const Series sx = series_of(layout, channels, time, true), so = series_of(out_layout, channels, frames * n_bins, true);
    const unsigned esz = magnitude ? 4 : 8;
    if (int e = check_ptrs("cqt: ", {{"x", x, (uintptr_t)batch * sx.item * 4, 4, false, false},
                                     {"table", table, (uintptr_t)table_floats * 4, 16, false, false},
                                     {"out", out, (uintptr_t)batch * so.item * esz, esz, false, true}}))
        return e;
    const int F = 16 * p.RT;
    const long long runs = (frames + F - 1) / F;
    long long grid;
    if (int e = grid_of(runs, batch, channels, "cqt", &grid)) return e;
    if (frames * hop + L >= (1LL << 40)) return fail(KPR_E_UNSUPPORTED, "cqt: %lld frames at a hop of %d reach past 2^40 samples", (long long)frames, hop);
    CqtArgs a;
    a.x = x; a.table = reinterpret_cast<const f4*>(table); a.out = static_cast<float*>(out);
    a.item = sx.item; a.chan = sx.chan; a.stride = sx.stride;
    a.out_item = so.item; a.out_chan = so.chan;
    a.out_t = n_bins * so.stride; a.out_k = so.stride;
    a.C = channels; a.time = (int)time; a.frames = (int)frames; a.runs = (int)runs; a.K = n_bins;
    a.hop = hop; a.origin = center ? -(L / 2) : 0;
    a.hopL = p.hopL; a.pad = p.pad; a.magic = p.magic; a.pieces = p.pieces; a.red = p.red;
    a.n_phases = (int)p.phases.size();
    std::copy(p.phases.begin(), p.phases.end(), a.ph);
    const bool mag = magnitude != 0;
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_cqt<v%d,%s>: grid %lld, lds %zu B, runs of %d frames, %s form (row %d, pad %d), chunk %d, "
                "%zu tiles in %d phases, %d work items, table %lld floats\n", p.vec ? 4 : 1, mag ? "mag" : "cplx", grid, p.lds, F,
                p.win ? "WIN" : "SPAN", p.hopL, p.pad, p.chunk, p.tiles.size(), a.n_phases, p.items, p.table_floats);
    const hipStream_t st = (hipStream_t)stream;
    int e;
    if (p.RT == 4) e = p.vec ? (mag ? launch_cqt<4, true, true>(a, grid, p.lds, st) : launch_cqt<4, true, false>(a, grid, p.lds, st))
                             : (mag ? launch_cqt<4, false, true>(a, grid, p.lds, st) : launch_cqt<4, false, false>(a, grid, p.lds, st));
    else e = p.vec ? (mag ? launch_cqt<2, true, true>(a, grid, p.lds, st) : launch_cqt<2, true, false>(a, grid, p.lds, st))
                   : (mag ? launch_cqt<2, false, true>(a, grid, p.lds, st) : launch_cqt<2, false, false>(a, grid, p.lds, st));
    if (e) return e;
    return launch_check(p.vec ? (mag ? "k_cqt<v4,mag>" : "k_cqt<v4,cplx>") : (mag ? "k_cqt<v1,mag>" : "k_cqt<v1,cplx>"));
}

}  // namespace kpr
