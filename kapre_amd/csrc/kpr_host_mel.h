// kpr_host_mel.h -- host side of the mel / filterbank / decibel kernels (kpr_mel_kernels.h, kpr_mel_ts_kernels.h, kpr_mel_pw_kernels.h,
// kpr_fb_pw_kernels.h, kpr_mel_mr_kernels.h, k_db_* and k_band_mel of kpr_misc_kernels.h): tile ranges, the schedules and their
// caches, the packed filterbank (header, band plan, verification, the host-only pack / k-range builders), the launchers, the decibel
// helpers, the workspace sizes, MelRoute / mel_route and run_mel_f32, fb_route and the two float32 ApplyFilterbank bodies.
// Part of the single translation unit kapre_hip.hip (included there after kpr_host_istft.h; not stand-alone).
#pragma once

namespace kpr {

// Per 16-filter tile: the k range [lo, hi) the fused kernel walks, padded to whole chunks of
// kChunkRows rows inside [0, mel_row_cap(K)] (rows outside the caller's exact-zero range hold
// zeros for this tile, rows >= K do not exist and are packed as zeros).
static int tile_ranges(int K, int M, const int32_t* kr_host, int* lo_out, int* hi_out) {
    const int ntiles = (M + 15) / 16;
    if (ntiles > kMaxTiles)
        return fail(KPR_E_UNSUPPORTED, "n_filt=%d exceeds the %d-filter limit", M, kMaxTiles * 16);
    const int kp = (K + 3) & ~3;
    const int cap = mel_row_cap(K);
    for (int t = 0; t < ntiles; ++t) {
        int lo = 0, hi = kp;
        if (kr_host) {
            lo = kr_host[2 * t]; hi = kr_host[2 * t + 1];
            if (lo < 0 || hi > kp || lo > hi || (lo & 3) || (hi & 3))
                return fail(KPR_E_BADARG, "bad filterbank k-range for tile %d: [%d,%d)", t, lo, hi);
        }
        lo &= ~7;       // whole 8-row blocks (a tile's first row stays 32-byte aligned within the magnitude row)
        int need = std::max(kChunkRows, (hi - lo + kChunkRows - 1) / kChunkRows * kChunkRows);
        hi = std::min(cap, lo + need);
        lo = std::max(0, hi - need);
        if (hi - lo != need)
            return fail(KPR_E_UNSUPPORTED, "n_freq=%d too small for the fused kernel", K);
        lo_out[t] = lo; hi_out[t] = hi;
    }
    return 0;
}

static int build_sched(int K, int M, const int32_t* kr_host, MelSched* sch) {
    int lo[kMaxTiles], hi[kMaxTiles];
    if (int e = tile_ranges(K, M, kr_host, lo, hi)) return e;
    const int ntiles = (M + 15) / 16;
    sch->M = M;
    sch->ntiles = ntiles;
    int total = 0;
    for (int t = 0; t < ntiles; ++t) {
        sch->klo[t] = (short)lo[t]; sch->khi[t] = (short)hi[t];
        sch->chunk0[t] = (unsigned short)total;          // packed layout: tiles in natural order
        total += (hi[t] - lo[t]) / kChunkRows;
    }
    // 4 equal contiguous slices of the chunk stream; tiles straddling a cut are split
    int cut[5];
    for (int w = 0; w <= 4; ++w) cut[w] = (int)(((long long)total * w + 2) / 4);
    cut[0] = 0; cut[4] = total;
    int nseg = 0, w = 0;
    sch->wave_seg0[0] = 0;
    for (int t = 0; t < ntiles; ++t) {
        int c = sch->chunk0[t];
        const int cend = c + (hi[t] - lo[t]) / kChunkRows;
        sch->t_s0[t] = (unsigned char)nseg;
        sch->t_ns[t] = 0;
        while (c < cend) {
            while (w < 3 && c >= cut[w + 1]) { ++w; sch->wave_seg0[w] = nseg; }
            const int e = std::min(cend, cut[w + 1] > c ? cut[w + 1] : cend);
            if (nseg >= kMaxSegs) return fail(KPR_E_UNSUPPORTED, "too many filterbank segments");
            sch->seg_tile[nseg] = (unsigned char)t;
            sch->seg_nch[nseg] = e - c;
            sch->seg_k0[nseg] = lo[t] + (c - sch->chunk0[t]) * kChunkRows;
            ++sch->t_ns[t];
            ++nseg;
            c = e;
        }
    }
    while (w < 4) { ++w; sch->wave_seg0[w] = nseg; }
    sch->nseg = nseg;
    for (int i = 0; i < 4; ++i) {
        sch->wave_chunk0[i] = (unsigned short)cut[i];
        sch->wave_nchunks[i] = (unsigned short)(cut[i + 1] - cut[i]);
    }
    return 0;
}

// ---- packed filterbank: 64-float header + MFMA fragments + band plan -----------------------------
// header words (uint32): [0] magic 'KPFB' [1] n_freq [2] n_filt [3] tiles [4] chunks [5] k-range hash
//   [6] float offset of the band plan section from the start of the blob (0: the matrix has no band plan)
//   [7] L (lanes per frame the plan is laid out for) [8] NR [9] CMQ [10] partial sums per frame [11] section words
constexpr int kPackHeaderFloats = 64;
constexpr uint32_t kPackMagic = 0x4b504642u;
// chunks (512 floats of fragments each) of the packed matrix of a schedule
static int packed_chunks(const MelSched& sch) {
    int chunks = 0;
    for (int t = 0; t < sch.ntiles; ++t) chunks += (sch.khi[t] - sch.klo[t]) / kChunkRows;
    return chunks;
}

// Band plan of k_mel_pw (kpr_mel_pw_kernels.h has the arithmetic): possible when n_freq - 1 is 128 ... 1024 (the fused
// power-of-two sizes) and every bin below Nyquist has at most two non-zeros, in neighbouring filters a(k), a(k) + 1 with
// a(k) non-decreasing -- mel banks of any scale / normalisation, any triangular bank.  Returns the section size in words
// (0: no plan) and fills `sec` (capacity pw_section_cap(K) words) and the header fields.
// lanes per row of a band plan for K = n_freq rows: the K - 1 bins below Nyquist in groups of 16 per lane, L a power of two (8 ...
// 64).  The fused kernel k_mel_pw needs K - 1 == 16 L exactly (n_fft 256 ... 2048); the stand-alone kernel k_fb_pw takes any K - 1
// that is a multiple of four (round 6: n_fft 400 -> 200 bins on 16 lanes, 13 of them in use; the bins beyond K - 1 have zero weights
// and are never loaded).  0: no plan for this K.
static int pw_plan_lanes(int K) {
    const int nb = K - 1;
    if (nb < 4 || nb > 1024 || (nb & 3)) return 0;
    int L = 8;
    while (kPts * L < nb) L *= 2;
    return L;
}
static int pw_section_cap(int K) {
    const int L = pw_plan_lanes(K);
    return L ? kPwEmaskWords + pw_table_words(L, kPwMaxRounds, kPwMaxCmq) : 0;
}
static int build_band_plan(const float* fb, int K, int M, uint32_t* sec, uint32_t* hdr_fields /* [7..11] */) {
    const int cap = pw_section_cap(K);
    if (!cap) return 0;
    const int NB = K - 1;                                             // bins below Nyquist
    const int L = pw_plan_lanes(K), NC = kPts * L, G = 64 / L;       // NC >= NB: the plan's padded bin count
    const int NR = (M + L - 1) / L;
    if (NR > kPwMaxRounds) return 0;
    std::vector<int> a(NC);
    std::vector<float> w0(NC, 0.0f), w1(NC, 0.0f);
    int prev = 0;
    for (int k = 0; k < NC; ++k) {
        int idx[3], n = 0;
        for (int m = 0; k < NB && m < M && n < 3; ++m) {              // (bins NB ... NC - 1 do not exist: no weights)
            const float v = fb[(size_t)k * M + m];
            if (v != 0.0f || v != v) idx[n++] = m;
        }
        if (n > 2) return 0;
        if (n == 2 && idx[1] != idx[0] + 1) return 0;
        if (n == 0) a[k] = prev;
        else if (n == 2) {
            if (idx[0] < prev) return 0;
            a[k] = idx[0];
            w0[k] = fb[(size_t)k * M + idx[0]];
            w1[k] = fb[(size_t)k * M + idx[1]];
        } else {
            const int m = idx[0];
            const float v = fb[(size_t)k * M + m];
            if (m == prev) { a[k] = prev; w0[k] = v; }
            else if (m == prev + 1) { a[k] = prev; w1[k] = v; }       // (keeps the running segment going)
            else if (m > prev + 1) { a[k] = m; w0[k] = v; }
            else return 0;
        }
        prev = a[k];
    }
    // partial sums: a lane's 16 bins, cut where a(k) changes; listed lane by lane = in bin order, so the partial sums of one
    // segment are neighbours in the list
    unsigned long long emask[16] = {0};
    std::vector<int> first(M + 1, 0), cnt(M + 1, 0), P(L, 0);
    int nlist = 0;
    for (int fl = 0; fl < L; ++fl) {
        P[fl] = 8 * nlist;
        bool any = false;                                             // the running piece has a non-zero weight
        for (int i = 0; i < 16; ++i) {
            const int k = 16 * fl + i;
            any = any || w0[k] != 0.0f || w1[k] != 0.0f;
            // a piece whose weights are all zero leaves the accumulators at zero: nothing to append (bins outside
            // [f_min, f_max] would otherwise form one piece per lane of a very long "segment")
            if ((i == 15 || a[k + 1] != a[k]) && any) {
                emask[i] |= 1ull << fl;
                if (cnt[a[k]] == 0) first[a[k]] = nlist;
                ++cnt[a[k]];
                ++nlist;
                any = false;
            }
        }
    }
    // the list grows from the start of the row (every magnitude, Nyquist included, is in registers by then) and must stop
    // short of the zero words at its end
    if (2 * nlist > pw_zero_word(NC)) return 0;
    int cm = 1;
    for (int m = 0; m < M; ++m) cm = std::max(cm, cnt[m]);
    const int CMQ = (cm + 3) / 4;
    if (CMQ > kPwMaxCmq) return 0;
    for (int i = 0; i < 16; ++i) {
        unsigned long long e = 0;
        for (int gq = 0; gq < G; ++gq) e |= emask[i] << (L * gq);
        sec[2 * i] = (uint32_t)(e & 0xffffffffull);
        sec[2 * i + 1] = (uint32_t)(e >> 32);
    }
    uint32_t* tab = sec + kPwEmaskWords;
    auto putf = [](uint32_t* p, float v) { std::memcpy(p, &v, 4); };
    for (int fl = 0; fl < L; ++fl)
        for (int j = 0; j < 8; ++j)
            for (int e = 0; e < 4; ++e) {
                const int k = 16 * fl + 2 * j + (e >> 1);
                putf(&tab[(j * L + fl) * 4 + e], (e & 1) ? w1[k] : w0[k]);
            }
    for (int fl = 0; fl < L; ++fl) tab[32 * L + fl] = (uint32_t)P[fl];
    const uint32_t zoff = 4u * (uint32_t)pw_zero_word(NC);
    for (int r = 0; r < NR; ++r)
        for (int fl = 0; fl < L; ++fl) {
            const int m = fl + L * r;
            putf(&tab[33 * L + r * L + fl], m < M ? fb[(size_t)NB * M + m] : 0.0f);     // the Nyquist row
            for (int q = 0; q < CMQ; ++q)
                for (int e = 0; e < 4; ++e) {
                    const int sidx = 4 * q + e;
                    uint32_t ou = zoff, od = zoff;
                    if (m < M && sidx < cnt[m]) ou = 8u * (uint32_t)(first[m] + sidx);
                    if (m >= 1 && m < M && sidx < cnt[m - 1]) od = 8u * (uint32_t)(first[m - 1] + sidx) + 4u;
                    tab[(33 + NR) * L + (((r * CMQ + q) * L) + fl) * 4 + e] = ou | (od << 16);
                }
        }
    hdr_fields[0] = (uint32_t)L; hdr_fields[1] = (uint32_t)NR; hdr_fields[2] = (uint32_t)CMQ; hdr_fields[3] = (uint32_t)nlist;
    hdr_fields[4] = (uint32_t)(kPwEmaskWords + pw_table_words(L, NR, CMQ));
    return (int)hdr_fields[4];
}

static uint32_t kranges_hash(int K, int M, const int32_t* kr_host) {
    uint32_t h = 0x811c9dc5u;
    auto mix = [&h](uint32_t v) { for (int i = 0; i < 4; ++i) { h ^= (v >> (8 * i)) & 0xffu; h *= 16777619u; } };
    mix((uint32_t)K); mix((uint32_t)M);
    if (kr_host) for (int i = 0; i < 2 * ((M + 15) / 16); ++i) mix((uint32_t)kr_host[i]);
    else mix(0xdeadbeefu);
    return h;
}

struct SchedKey {
    int K, M; uint32_t h;
    bool operator<(const SchedKey& o) const { return K != o.K ? K < o.K : M != o.M ? M < o.M : h < o.h; }
};
static std::map<SchedKey, MelSched> g_sched;                          // built once per filterbank geometry
struct PackInfo { uint32_t band_off, L, NR, CMQ, nlist; };          // what the verified header says about the band plan
static std::map<std::pair<const void*, SchedKey>, PackInfo> g_pack_ok;    // packed blobs already verified

// schedule of (K, M, k-ranges): cached, so the steady-state call does no host work beyond a lookup
static int get_sched(int K, int M, const int32_t* kr_host, MelSched* out, uint32_t* hash_out = nullptr) {
    if ((M + 15) / 16 > kMaxTiles || K > 32000)            // 64 tiles; row bounds are stored as 16-bit values
        return fail(KPR_E_UNSUPPORTED, "filterbank %d x %d exceeds the packed schedule (%d filters, 32000 rows)", K, M,
                    kMaxTiles * 16);
    const SchedKey key{K, M, kranges_hash(K, M, kr_host)};
    if (hash_out) *hash_out = key.h;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_sched.find(key);
    if (it == g_sched.end()) {
        MelSched sch;
        if (int e = build_sched(K, M, kr_host, &sch)) return e;
        if (g_sched.size() > 256) g_sched.clear();
        it = g_sched.emplace(key, sch).first;
    }
    *out = it->second;
    return 0;
}

// A packed blob must describe the SAME matrix geometry and k-ranges as the call's arguments: its header
// (written by kpr_filterbank_pack) is read back from the device ONCE per (pointer, geometry, k-ranges)
// -- a 32-byte copy on the call's stream on first use, waited for, so that it is ordered after an upload of the
// blob on that stream (not legal during stream capture: warm up first, as for the table uploads) -- and compared.
// Mismatch = BADARG.  Best effort by design: the cache is keyed on the device address, so a different buffer that
// later lands on the same address with the same geometry arguments is not re-read.
static int verify_packed(const float* fb_packed, int K, int M, const int32_t* kr_host, const MelSched& sch,
                         hipStream_t st, PackInfo* info = nullptr) {
    const SchedKey key{K, M, kranges_hash(K, M, kr_host)};
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_pack_ok.find({fb_packed, key});
        if (it != g_pack_ok.end()) { if (info) *info = it->second; return 0; }
    }
    uint32_t hdr[12] = {0};
    KPR_HIP(hipMemcpyAsync(hdr, fb_packed, sizeof(hdr), hipMemcpyDeviceToHost, st));
    KPR_HIP(hipStreamSynchronize(st));
    const int chunks = packed_chunks(sch);
    if (hdr[0] != kPackMagic)
        return fail(KPR_E_BADARG, "fb_packed does not start with a kpr_filterbank_pack header");
    if ((int)hdr[1] != K || (int)hdr[2] != M || (int)hdr[3] != sch.ntiles || (int)hdr[4] != chunks || hdr[5] != key.h)
        return fail(KPR_E_BADARG, "fb_packed was packed for another filterbank (%u x %u, %u tiles, %u chunks, "
                    "k-range hash %08x) than this call describes (%d x %d, %d tiles, %d chunks, hash %08x)",
                    hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], K, M, sch.ntiles, chunks, key.h);
    PackInfo pi{hdr[6], hdr[7], hdr[8], hdr[9], hdr[10]};
    if (pi.band_off) {                                          // a band plan this build cannot run = no band plan
        const int NC = kPts * pw_plan_lanes(K);                       // (the plan's padded bin count; 0: no plan for this K)
        const bool sane = pw_section_cap(K) && (int)pi.L == pw_plan_lanes(K) && (int)pi.NR == (M + (int)pi.L - 1) / (int)pi.L &&
                          pi.CMQ >= 1 && (int)pi.CMQ <= kPwMaxCmq && pi.band_off == (uint32_t)(kPackHeaderFloats + chunks * 512) &&
                          hdr[11] == (uint32_t)(kPwEmaskWords + pw_table_words((int)pi.L, (int)pi.NR, (int)pi.CMQ)) &&
                          2 * (int)pi.nlist <= pw_zero_word(NC);                 // (the partial-sum list fits in front of the zero words)
        if (!sane) pi = PackInfo{0, 0, 0, 0, 0};
    }
    if (info) *info = pi;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_pack_ok.size() > 1024) g_pack_ok.clear();
    g_pack_ok[{fb_packed, key}] = pi;
    return 0;
}

// kpr_filterbank_forget: drop what is cached about one packed blob (NULL: about all of them)
static int filterbank_forget(const float* fb_packed) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!fb_packed) { g_pack_ok.clear(); return 0; }
    for (auto it = g_pack_ok.begin(); it != g_pack_ok.end();)
        it = (it->first.first == (const void*)fb_packed) ? g_pack_ok.erase(it) : std::next(it);
    return 0;
}

// ---- the host-only filterbank builders: kpr_filterbank_pack_floats, kpr_filterbank_pack, kpr_filterbank_kranges ----
static int64_t filterbank_pack_floats(int n_freq, int n_filt, const int32_t* fb_kranges_host) {
    if (n_freq <= 0 || n_filt <= 0) return -1;
    MelSched sch;
    if (build_sched(n_freq, n_filt, fb_kranges_host, &sch)) return -1;
    return (int64_t)packed_chunks(sch) * 512 + kPackHeaderFloats + pw_section_cap(n_freq);   // header | fp32 MFMA fragments | band plan
}

static int filterbank_pack(const float* fb_host, int n_freq, int n_filt, const int32_t* fb_kranges_host, float* out_host) {
    if (!fb_host || !out_host || n_freq <= 0 || n_filt <= 0)
        return fail(KPR_E_BADARG, "bad arguments to kpr_filterbank_pack");
    MelSched sch;
    if (int e = build_sched(n_freq, n_filt, fb_kranges_host, &sch)) return e;
    {
        uint32_t hdr[kPackHeaderFloats] = {0};
        const int chunks = packed_chunks(sch);
        hdr[0] = kPackMagic; hdr[1] = (uint32_t)n_freq; hdr[2] = (uint32_t)n_filt; hdr[3] = (uint32_t)sch.ntiles;
        hdr[4] = (uint32_t)chunks; hdr[5] = kranges_hash(n_freq, n_filt, fb_kranges_host);
        if (const int cap = pw_section_cap(n_freq)) {                 // band plan for k_mel_pw (after the fragments)
            uint32_t* sec = reinterpret_cast<uint32_t*>(out_host) + kPackHeaderFloats + (size_t)chunks * 512;
            std::memset(sec, 0, sizeof(uint32_t) * cap);
            if (build_band_plan(fb_host, n_freq, n_filt, sec, &hdr[7])) hdr[6] = (uint32_t)(kPackHeaderFloats + chunks * 512);
        }
        std::memcpy(out_host, hdr, sizeof(hdr));
        out_host += kPackHeaderFloats;
    }
    for (int t = 0; t < sch.ntiles; ++t) {
        size_t pos = (size_t)sch.chunk0[t] * 512;
        for (int c = 0; c < (sch.khi[t] - sch.klo[t]) / kChunkRows; ++c)
            for (int g = 0; g < 2; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int s4 = 0; s4 < 4; ++s4) {
                        const int k = sch.klo[t] + kChunkRows * c + 16 * g + 4 * s4 + (l >> 4);
                        const int m = 16 * t + (l & 15);
                        out_host[pos++] = (k < n_freq && m < n_filt) ? fb_host[(size_t)k * n_filt + m] : 0.0f;
                    }
    }
    return 0;
}

static int filterbank_kranges(const float* fb_host, int n_freq, int n_filt, int32_t* out_host) {
    if (!fb_host || !out_host || n_freq <= 0 || n_filt <= 0)
        return fail(KPR_E_BADARG, "bad arguments to kpr_filterbank_kranges");
    const int ntiles = (n_filt + 15) / 16;
    for (int t = 0; t < ntiles; ++t) {
        int lo = n_freq, hi = 0;
        for (int k = 0; k < n_freq; ++k)
            for (int m = t * 16; m < std::min(n_filt, t * 16 + 16); ++m) {
                float v = fb_host[(size_t)k * n_filt + m];
                if (v != 0.0f || v != v) { lo = std::min(lo, k); hi = std::max(hi, k + 1); }
            }
        if (lo >= hi) { lo = 0; hi = 0; }
        out_host[2 * t] = lo & ~3;
        out_host[2 * t + 1] = (hi + 3) & ~3;
    }
    return 0;
}

template <int NC, bool FROM_MAG, bool RES, bool LD8 = false>
static int launch_mel_ws_inst(const float* x, const Geom& g, const float* window, const float2* tw,
                              const float* fbp, const MelSched& sch, const DbDev& db, unsigned* stats,
                              float* out, hipStream_t st) {
    const size_t lds = mel_ws_lds_bytes(NC, sch.nseg, FROM_MAG ? 2 : 1);     // (the LD8 form uses one group's worth less)
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_mel_ws<NC, FROM_MAG, RES, LD8>))) return e;
    const long long ntiles = (g.total_frames + kFT - 1) / kFT;
    if (ntiles > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "too many frames");
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    constexpr int G = 64 / (NC / kPts);
    constexpr int RF = kWsProd * G;                                // frames per round
    const long long nrounds = (g.total_frames + RF - 1) / RF;
    const unsigned grid = (unsigned)std::min<long long>(nrounds, cus);         // 1 workgroup / CU
    const long long tickets = (g.total_frames + G - 1) / G;                    // a ticket = G frames (one wave's round)
    if (int e = status_word_ready()) return e;                  // (the kernel's bounded waits report there)
    hipLaunchKernelGGL((k_mel_ws<NC, FROM_MAG, RES, LD8>), dim3(grid), dim3(kWsThreads), lds, st, x, g, window, tw, fbp,
                       sch, db, stats, out, (int)(tickets / grid), (int)(tickets % grid), g_debug_stamps);
    return launch_check("k_mel_ws", NC);
}

// the longest filterbank slice (chunks) of the four consumer waves of k_mel_ws
static int slice_max(const MelSched& sch) {
    int m = 0;
    for (int i = 0; i < 4; ++i) m = std::max(m, (int)sch.wave_nchunks[i]);
    return m;
}

enum { WS_PLAIN, WS_RES, WS_LD8 };                               // k_mel_ws instances (mel_ws_form)
static int mel_ws_form(const MelSched& sch, bool from_mag, int K) {
    // every consumer wave's slice fits the register-resident form (mel banks: 37 chunks at 1025 x 128)?
    if (!from_mag) return slice_max(sch) <= kWsResident && opt(OPT_MEL_VARIANT) != 2 ? WS_RES : WS_PLAIN;
    return K > 512 ? WS_LD8 : WS_PLAIN;                            // wide rows: 8 loaders
}

// fbp: the fragment section of the packed blob (behind its header); form: mel_ws_form
template <int NC, bool FROM_MAG = false>
static int launch_mel_ws(int form, const float* x, const Geom& g, const float* window, const float2* tw,
                         const float* fbp, const MelSched& sch, const DbDev& db, unsigned* stats,
                         float* out, hipStream_t st) {
    if constexpr (FROM_MAG) {
        if (form == WS_LD8) return launch_mel_ws_inst<NC, true, false, true>(x, g, window, tw, fbp, sch, db, stats, out, st);
    } else {
        if (form == WS_RES) return launch_mel_ws_inst<NC, false, true>(x, g, window, tw, fbp, sch, db, stats, out, st);
    }
    return launch_mel_ws_inst<NC, FROM_MAG, false>(x, g, window, tw, fbp, sch, db, stats, out, st);
}

// ---- k_mel_ts: schedule (whole (frame tile, filter tile) items per wave, heavy filter tiles cut) + launch ----------
// Builds the per-wave chunk-entry table described at MelSchedTs (host copy in *tab).
// FT = 16-frame tiles per round, S = magnitude row stride (floats), nwaves = waves per workgroup of the kernel the table
// is for: k_mel_ts (8 waves; entry word 1 = float offset 16 ft S + k0) or k_mel_mr (4 waves, S = 0: entry word 1 =
// k0 | ft << 16, the kernel forms the row address itself).
static int build_sched_ts(int K, int M, const int32_t* kr_host, int FT, int S, int nwaves, MelSchedTs* sch,
                          std::vector<unsigned>* tab) {
    int lo[kMaxTiles], hi[kMaxTiles];
    const int ntiles = (M + 15) / 16;
    if (ntiles > kTsMaxTiles) return fail(KPR_E_UNSUPPORTED, "filterbank too wide for k_mel_ts");
    if (int e = tile_ranges(K, M, kr_host, lo, hi)) return e;
    std::memset(sch, 0, sizeof(*sch));
    sch->M = M; sch->ntiles = ntiles; sch->FT = FT;
    int total = 0, nch[kTsMaxTiles], chunk0[kTsMaxTiles + 1];
    for (int t = 0; t < ntiles; ++t) {
        chunk0[t] = total;
        nch[t] = (hi[t] - lo[t]) / kChunkRows;
        total += nch[t];
    }
    chunk0[ntiles] = total;
    if (total > 60000) return fail(KPR_E_UNSUPPORTED, "filterbank too wide for k_mel_ts");
    // parts: a filter tile with more chunks than an even share of the round's work is cut into near-equal parts
    const int share = std::max(1, (FT * total + nwaves - 1) / nwaves);
    std::vector<MelItemTs> parts;
    int nslots = 0;
    for (int ft = 0; ft < FT; ++ft)
        for (int t = 0; t < ntiles; ++t) {
            const int np = std::min(4, (nch[t] + share - 1) / share);
            int c = chunk0[t];
            const int slot0 = nslots;
            for (int pi = 0; pi < np; ++pi) {
                const int n = (nch[t] * (pi + 1)) / np - (nch[t] * pi) / np;
                if (n > 255) return fail(KPR_E_UNSUPPORTED, "filterbank too wide for k_mel_ts");
                MelItemTs im{};
                im.ft = (unsigned char)ft; im.t = (unsigned char)t; im.nch = (unsigned char)n; im.c0 = (unsigned short)c;
                if (pi == 0) { im.kind = 0; im.slot0 = (unsigned char)slot0; im.nslots = (unsigned char)(np - 1); }
                else { im.kind = 1; im.slot0 = (unsigned char)nslots++; im.nslots = 0; }
                parts.push_back(im);
                c += n;
            }
        }
    if (nslots > kTsMaxSlots) return fail(KPR_E_UNSUPPORTED, "too many cut filter tiles for k_mel_ts");
    sch->nslots = nslots;
    // longest first onto the least loaded SIMD (waves w and w + 4 share one), then onto its less loaded wave; a wave takes
    // at most one owner of a cut tile (its accumulators stay live across the second barrier)
    std::vector<int> order(parts.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return parts[a].nch > parts[b].nch; });
    int wload[kTsWaves] = {0}, wown[kTsWaves] = {0};
    std::vector<int> mine[kTsWaves];
    for (int idx : order) {
        const MelItemTs& im = parts[idx];
        const bool cut_owner = im.kind == 0 && im.nslots > 0;
        int best = -1;
        for (int w = 0; w < nwaves; ++w) {
            if (wload[w] + im.nch > kTsMaxEnt) continue;
            if (cut_owner && wown[w]) continue;
            if (best < 0) { best = w; continue; }
            const int sl = wload[w & 3] + wload[(w & 3) + 4], bl = wload[best & 3] + wload[(best & 3) + 4];   // (zero beyond nwaves)
            if (sl < bl || (sl == bl && wload[w] < wload[best])) best = w;
        }
        if (best < 0) return fail(KPR_E_UNSUPPORTED, "too many filterbank chunks for k_mel_ts");
        mine[best].push_back(idx);
        wload[best] += im.nch;
        if (cut_owner) wown[best] = 1;
    }
    tab->assign(8 + 3 * kTsWaves * kTsMaxEnt, 0u);
    for (int w = 0; w < nwaves; ++w) {
        // order per wave: parts, whole tiles, the owner of a cut tile last
        auto rank = [&](int i) { const MelItemTs& im = parts[i]; return im.kind == 1 ? 0 : (im.nslots == 0 ? 1 : 2); };
        std::stable_sort(mine[w].begin(), mine[w].end(), [&](int a, int b) { return rank(a) < rank(b); });
        int n = 0;
        for (int idx : mine[w]) {
            const MelItemTs& im = parts[idx];
            for (int i = 0; i < im.nch; ++i, ++n) {
                unsigned* e = tab->data() + 8 + 3 * (w * kTsMaxEnt + n);
                const bool last = i + 1 == im.nch;
                e[0] = (unsigned)(im.c0 + i) | (last ? 0x80000000u : 0u);
                const unsigned k0 = (unsigned)(lo[im.t] + kChunkRows * (im.c0 + i - chunk0[im.t]));
                e[1] = S ? (unsigned)(16 * im.ft * S) + k0 : (k0 | (unsigned)im.ft << 16);
                e[2] = last ? ((unsigned)im.kind | (unsigned)im.t << 1 | (unsigned)im.ft << 5 | (unsigned)im.slot0 << 8 |
                               (unsigned)im.nslots << 16) : 0u;
            }
        }
        (*tab)[w] = (unsigned)n;
    }
    return 0;
}

struct SchedTsKey {
    int dev, K, M, FT, S, nwaves; uint32_t h;
    bool operator<(const SchedTsKey& o) const {
        return std::tie(dev, K, M, FT, S, nwaves, h) < std::tie(o.dev, o.K, o.M, o.FT, o.S, o.nwaves, o.h);
    }
};
static std::map<SchedTsKey, MelSchedTs> g_sched_ts;      // entries own a small device table (kept for the process lifetime)

static int get_sched_ts(int K, int M, const int32_t* kr_host, int FT, int S, int nwaves, MelSchedTs* out) {
    int dev;
    if (int e = cur_device(&dev)) return e;
    const SchedTsKey key{dev, K, M, FT, S, nwaves, kranges_hash(K, M, kr_host)};
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_sched_ts.find(key);
    if (it == g_sched_ts.end()) {
        MelSchedTs sch;
        std::vector<unsigned> tab;
        if (int e = build_sched_ts(K, M, kr_host, FT, S, nwaves, &sch, &tab)) return e;
        unsigned* d = nullptr;
        KPR_HIP(hipMalloc(&d, tab.size() * sizeof(unsigned)));
        KPR_HIP(hipMemcpy(d, tab.data(), tab.size() * sizeof(unsigned), hipMemcpyHostToDevice));   // first use only, like the twiddles
        sch.tab = d;
        it = g_sched_ts.emplace(key, sch).first;
    }
    *out = it->second;
    return 0;
}

// true when k_mel_ts can take the call (geometry of the filterbank schedule + LDS); *sch is filled then
static bool mel_ts_ok(int n_fft, int K, int M, const int32_t* kr_host, const Geom& g, MelSchedTs* sch, int RF = 0) {
    if (n_fft != 2048 && n_fft != 1024 && n_fft != 512 && n_fft != 256) return false;
    if ((M + 15) / 16 > kTsMaxTiles || g.total_frames >= 0x7fffff00LL) return false;
    const int NC = n_fft / 2;
    if (!RF) RF = mel_ts_rf(NC);
    if (get_sched_ts(K, M, kr_host, RF / 16, mel_ws_row_stride(NC + 1), kTsWaves, sch)) return false;
    return mel_ts_lds_bytes(NC, sch->nslots, RF) <= 80 * 1024;       // two workgroups per CU
}

template <int NC, int RF_ = 0>
static int launch_mel_ts(const float* x, const Geom& g, const float* window, const float2* tw, const float* fbp,
                         const MelSchedTs& sch, const DbDev& db, unsigned* stats, float* out, hipStream_t st) {
    constexpr int G = 64 / (NC / kPts), RF = RF_ ? RF_ : mel_ts_rf(NC);
    const size_t lds = mel_ts_lds_bytes(NC, sch.nslots, RF);
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_mel_ts<NC, RF_>))) return e;
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const long long tickets = (g.total_frames + G - 1) / G;                     // a ticket = G frames (the unit the runs are cut at)
    const long long nrounds = (g.total_frames + RF - 1) / RF;
    const unsigned grid = (unsigned)std::min<long long>(nrounds, 2LL * cus);    // 2 workgroups / CU
    hipLaunchKernelGGL((k_mel_ts<NC, RF_>), dim3(grid), dim3(kTsWaves * 64), lds, st, x, g, window, tw, fbp, sch, db, stats, out,
                       (int)(tickets / grid), (int)(tickets % grid), g_debug_stamps);
    return launch_check("k_mel_ts", NC);
}

// ---- k_mel_pw: every wave owns its frames end to end, banded mel sums (kpr_mel_pw_kernels.h) -------------------------
template <int NC, int W>
static int launch_mel_pw(const float* x, const Geom& g, const float* window, const float2* tw, const float* blob,
                         const PackInfo& pi, int M, const DbDev& db, unsigned* stats, float* out, hipStream_t st) {
    constexpr int L = NC / kPts, G = 64 / L;
    PwPlan pl{(int)pi.L, (int)pi.NR, (int)pi.CMQ, (int)pi.nlist, M, reinterpret_cast<const unsigned*>(blob) + pi.band_off,
              reinterpret_cast<const unsigned*>(blob), pi.band_off, 0, 0};
    const size_t lds = pw_lds_bytes(NC, W, pl.NR, pl.CMQ);
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_mel_pw<NC, W>))) return e;
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const long long tickets = (g.total_frames + G - 1) / G;                     // a ticket = G frames of one wave
    const int per_cu = std::max(1, std::min(16 / W, (int)(160 * 1024 / lds)));  // sixteen waves per CU (128 VGPRs)
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((tickets + W - 1) / W, (long long)per_cu * cus));
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_mel_pw<%d,%d>: grid %u, lds %zu B, NR %d CMQ %d list %d, %lld tickets\n", NC, W, grid, lds,
                pl.NR, pl.CMQ, pl.nlist, tickets);
    if (int e = status_word_ready()) return e;                  // (a stale band plan is reported there)
    hipLaunchKernelGGL((k_mel_pw<NC, W>), dim3(grid), dim3(W * 64), lds, st, x, g, window, tw, pl, db, stats, out,
                       (int)(tickets / grid), (int)(tickets % grid), g_debug_stamps);
    return launch_check("k_mel_pw", NC, W == 4 ? "w4" : W == 8 ? "w8" : "w16");
}
// the plain-output instance k_mel_plain_pw (kpr_mel_pw_kernels.h): n_fft 2048, no decibels, contiguous rows in, linear rows out,
// a band plan of exactly (NR, CMQ) -- mel_route checks all of it (MelRoute::plain).  Same grid, LDS and ticket split as launch_mel_pw.
template <int NC, int W, int NR, int CMQ>
static int launch_mel_pw_plain(const float* x, const Geom& g, const float* window, const float2* tw, const float* blob,
                               const PackInfo& pi, int M, float* out, hipStream_t st) {
    PwPlan pl{(int)pi.L, (int)pi.NR, (int)pi.CMQ, (int)pi.nlist, M, reinterpret_cast<const unsigned*>(blob) + pi.band_off,
              reinterpret_cast<const unsigned*>(blob), pi.band_off, 0, 0};
    if (pl.L * kPts != NC || pl.NR != NR || pl.CMQ != CMQ) return no_instance("k_mel_plain_pw");
    const size_t lds = pw_lds_bytes(NC, W, NR, CMQ);
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_mel_plain_pw<NC, W, NR, CMQ>))) return e;
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const long long tickets = g.total_frames;                                   // a ticket = one frame of one wave
    const int per_cu = std::max(1, std::min(16 / W, (int)(160 * 1024 / lds)));  // sixteen waves per CU (128 VGPRs)
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((tickets + W - 1) / W, (long long)per_cu * cus));
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_mel_pw<%d,%d,plain>: grid %u, lds %zu B, NR %d CMQ %d list %d, %lld tickets\n", NC, W, grid, lds,
                pl.NR, pl.CMQ, pl.nlist, tickets);
    if (int e = status_word_ready()) return e;                  // (a stale band plan is reported there)
    hipLaunchKernelGGL((k_mel_plain_pw<NC, W, NR, CMQ>), dim3(grid), dim3(W * 64), lds, st, x, g, window, tw, pl, out,
                       (int)(tickets / grid), (int)(tickets % grid), g_debug_stamps);
    // the general kernel's label with ",plain" behind it: "k_mel_pw<1024,w16>,plain" (what matches the general label matches this one)
    if (int e = launch_check("k_mel_pw", NC, W == 4 ? "w4" : W == 8 ? "w8" : "w16")) return e;
    if (g_launches.size() < 200) g_launches += ",plain";
    return 0;
}
static int launch_mel_pw_plain_w(int w, const float* x, const Geom& g, const float* window, const float2* tw, const float* blob,
                                 const PackInfo& pi, int M, float* out, hipStream_t st) {
    switch (w) {
        case 4:  return launch_mel_pw_plain<1024, 4, 2, 1>(x, g, window, tw, blob, pi, M, out, st);
        case 16: return launch_mel_pw_plain<1024, 16, 2, 1>(x, g, window, tw, blob, pi, M, out, st);
        default: return launch_mel_pw_plain<1024, 8, 2, 1>(x, g, window, tw, blob, pi, M, out, st);
    }
}
constexpr int kPwPairWaves = 12;                                 // waves per workgroup of the PAIR form
// the PAIR form's channels_last staging: output slots (0: 8-byte stores) of M x C floats each
static int mel_pw_pair_slots(const Geom& g, const PackInfo& pi, int M, const float* out) {
    const int NC = g.n_fft / 2, G = 64 / (NC / kPts), W = kPwPairWaves;
    // channels_last output with C >= 4: the M x C block of an (item, frame) through a ring of LDS slots, stored as one contiguous
    // run by the last of its C / 2 pair-waves (kpr_mel_pw_kernels.h; n_fft 2048 only).  A power of two, whatever fits the CU's LDS, and
    // at least the blocks the W waves can hold pairs of (need / 2: progress is guaranteed by the ticket order with any ring of one
    // slot or more -- tests/test_cl_ring_model.py -- but waves prefetch a ticket ahead, so with fewer slots than 2x the in-flight
    // span the bounded slot wait is taken routinely, not exceptionally); else (or C = 2, whose 8-byte pairs are contiguous
    // anyway) the 8-byte stores.
    const int CP = g.C / 2;
    if (G == 1 && g.out_cl && CP >= 2 && g.C <= 64 && opt(OPT_MEL_CL_STAGE) != 0 && (M * g.C) % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        const int blk = M * g.C;
        const int need = 2 * ((W * G + CP - 1) / CP) + 2;
        int slots = 32;
        while (slots >= 4 && pw_lds_bytes(NC, W, (int)pi.NR, (int)pi.CMQ, true, slots, blk) > 160 * 1024) slots >>= 1;
        if (slots >= 4 && slots >= need / 2) return slots;
    }
    return 0;
}

// the PAIR form (interleaved waveforms, even channel count: two channel-frames per fetch; three waves per SIMD)
template <int NC>
static int launch_mel_pw_pair(const float* x, const Geom& g, const float* window, const float2* tw, const float* blob,
                              const PackInfo& pi, int M, int cl_slots, const DbDev& db, unsigned* stats, float* out, hipStream_t st) {
    constexpr int L = NC / kPts, G = 64 / L, W = kPwPairWaves;
    PwPlan pl{(int)pi.L, (int)pi.NR, (int)pi.CMQ, (int)pi.nlist, M, reinterpret_cast<const unsigned*>(blob) + pi.band_off,
              reinterpret_cast<const unsigned*>(blob), pi.band_off, cl_slots, cl_slots ? M * g.C : 0};
    const int CP = g.C / 2;
    const size_t lds = pw_lds_bytes(NC, W, pl.NR, pl.CMQ, true, pl.cl_slots, pl.cl_blk);
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_mel_pw<NC, W, true>))) return e;
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const long long pairs = g.total_frames / 2;
    long long tickets = (pairs + G - 1) / G;                                    // a ticket = G channel pairs of one wave
    const int unit = pl.cl_slots ? CP : 1;                                      // staged: workgroups own whole blocks (CP tickets = G blocks)
    tickets = (tickets + unit - 1) / unit;                                      // ... counted in units from here on
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((tickets * unit + W - 1) / W, (long long)cus));
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_mel_pw<%d,%d,pair>: grid %u, lds %zu B, %lld ticket units of %d, %d output slots\n", NC, W, grid, lds,
                tickets, unit, pl.cl_slots);
    if (int e = status_word_ready()) return e;                  // (a stale band plan is reported there)
    hipLaunchKernelGGL((k_mel_pw<NC, W, true>), dim3(grid), dim3(W * 64), lds, st, x, g, window, tw, pl, db, stats, out,
                       (int)(tickets / grid), (int)(tickets % grid), g_debug_stamps);
    return launch_check("k_mel_pw_pair", NC);
}
template <int NC>
static int launch_mel_pw_w(int w, const float* x, const Geom& g, const float* window, const float2* tw, const float* blob,
                           const PackInfo& pi, int M, const DbDev& db, unsigned* stats, float* out, hipStream_t st) {
    switch (w) {
        case 4:  return launch_mel_pw<NC, 4>(x, g, window, tw, blob, pi, M, db, stats, out, st);
        case 16: return launch_mel_pw<NC, 16>(x, g, window, tw, blob, pi, M, db, stats, out, st);
        default: return launch_mel_pw<NC, 8>(x, g, window, tw, blob, pi, M, db, stats, out, st);
    }
}

// ---- k_fb_pw: the stand-alone ApplyFilterbank as banded row sums (kpr_fb_pw_kernels.h; round 6) -------------------------
// ST: two interleaved channels (channels_last, C = 2): `rows` counts (item, frame) blocks of K x 2 floats
template <int NC, bool ST>
static int launch_fb_pw(const float* x, long long rows, int K, const float* blob, const PackInfo& pi, int M, const float* fb, float* out,
                        hipStream_t st) {
    constexpr int L = NC / kPts, G = 64 / L;
    PwPlan pl{(int)pi.L, (int)pi.NR, (int)pi.CMQ, (int)pi.nlist, M, reinterpret_cast<const unsigned*>(blob) + pi.band_off,
              reinterpret_cast<const unsigned*>(blob), pi.band_off, 0, 0};
    const size_t lds = fb_pw_lds_bytes(NC, pl.NR, pl.CMQ, ST);
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_fb_pw<NC, ST>))) return e;
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const long long tickets = (rows + G - 1) / G;                               // a ticket = G rows (ST: blocks) of one wave
    const int per_cu = std::max(1, std::min(16 / kFbW, (int)(160 * 1024 / lds)));   // sixteen waves per CU (eight: 22.5 vs 20.7 us)
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((tickets + kFbW - 1) / kFbW, (long long)per_cu * cus));
    if (opt(OPT_VERBOSE))
        fprintf(stderr, "[kapre_hip] k_fb_pw<%d%s>: grid %u, lds %zu B, NR %d CMQ %d list %d, %lld tickets\n", NC, ST ? ",st" : "", grid, lds,
                pl.NR, pl.CMQ, pl.nlist, tickets);
    if (int e = status_word_ready()) return e;                  // (a stale band plan is reported there)
    hipLaunchKernelGGL((k_fb_pw<NC, ST>), dim3(grid), dim3(kFbW * 64), lds, st, x, rows, K, M, pl, fb, out, (int)(tickets / grid),
                       (int)(tickets % grid));
    return ST ? launch_check("k_fb_pw", NC, "st") : launch_check("k_fb_pw", NC);
}

// ---- k_mel_mr: the same schedule for the mixed-radix sizes (four-wave workgroups, up to three per CU) ---------------
template <class FF>
static int launch_mel_mr_inst(const float* x, const Geom& g, const float* window, const float2* tw, const float* fbp,
                              const MelSchedTs& sch, const DbDev& db, unsigned* stats, float* out, hipStream_t st) {
    constexpr int G = 64 / FF::L, RF = mel_mr_rf<FF>();
    const size_t lds = mel_mr_lds_bytes<FF>(sch.nslots);
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_mel_mr<FF>))) return e;
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const long long tickets = (g.total_frames + G - 1) / G;                      // runs are cut at G-frame granularity
    const long long nrounds = (g.total_frames + RF - 1) / RF;
    const int per_cu = std::max(1, std::min(12 / kMrWaves, (int)(160 * 1024 / lds)));      // 12 waves per CU at 168 VGPRs
    const unsigned grid = (unsigned)std::min<long long>(nrounds, (long long)per_cu * cus);
    hipLaunchKernelGGL((k_mel_mr<FF>), dim3(grid), dim3(kMrWaves * 64), lds, st, x, g, window, tw, fbp, sch, db, stats, out,
                       (int)(tickets / grid), (int)(tickets % grid), g_debug_stamps);
    return launch_check("k_mel_mr", FF::N);
}

// statistics slots per item for a batch of n items (DbDev::slot_mask): as many as keep slots x items <= 2048,
// at most 32, one for batches of 256 items and more (every word then collects a handful of atomics anyway)
// (the statistics region of the workspace is sized for db_slots_cap, whatever the option says: a workspace sized under one
//  "db_slots" value stays valid under any other -- ADVICE r03)
static int db_slots_cap(long long n_items) { return n_items <= 8192 ? 32 : 1; }
static int db_slots(long long n_items) {
    if (opt(OPT_DB_SLOTS) > 0) {                                 // forced (A/B runs, tests): rounded down to a power of two
        int f = 1;
        while (2 * f <= opt(OPT_DB_SLOTS)) f *= 2;
        return std::min(f, db_slots_cap(n_items));
    }
    int s = 1;
    while (s < 32 && (long long)(2 * s) * n_items <= 2048 && n_items < 256) s *= 2;
    return s;
}

static DbDev make_db(const kpr_db_params* db) {
    DbDev d{0, 1e-5f, 0.0f, 80.0f, 0, 0};
    if (db && db->enabled) {
        d.enabled = 1;
        // (to_db feeds max(x, amin) to v_log_f32, which has no denormal support: an amin below the smallest normal float --
        //  a floor under -379 dB -- is raised to it)
        d.amin = std::max(db->amin, 1.17549435e-38f);
        d.ref_term = (float)(10.0 * std::log10(std::max((double)db->amin, (double)db->ref_value)));
        d.dyn = db->dynamic_range;
    }
    return d;
}

// same checks (and order) as backend.py:168-173
static int check_db_values(double ref_value, double amin, double dynamic_range) {
    if (!(ref_value > 0)) return fail(KPR_E_BADARG, "ref_value must be positive");
    if (!(amin > 0)) return fail(KPR_E_BADARG, "amin must be positive");
    if (!(dynamic_range > 0)) return fail(KPR_E_BADARG, "dynamic_range must be positive");
    return 0;
}
static int check_db(const kpr_db_params* db) {
    return db && db->enabled ? check_db_values(db->ref_value, db->amin, db->dynamic_range) : 0;
}

// blocks per item of the decibel passes: enough blocks to fill the GPU (about 2048), at least 4096
// floats each, and few per item (every block ends with two atomics on the item's statistics)
static int db_chunks(long long n_items, long long item_size) {
    const long long want = (2048 + n_items - 1) / std::max<long long>(1, n_items);
    return (int)std::max<long long>(1, std::min<long long>(std::min<long long>(256, want), item_size / 4096));
}

// the statistics words of n_items items (x slots) to their initial values: ahead of every decibel pass
static int stats_init(unsigned* stats, long long n_items, hipStream_t st) {
    hipLaunchKernelGGL(k_stats_init, dim3(grid_1d(n_items, 256)), dim3(256), 0, st, stats, n_items);
    return launch_check("k_stats_init");
}

static int db_clamp(float* out, long long n_items, long long item_size, float dyn,
                    const unsigned* stats, hipStream_t st, int slots = 1) {
    if (n_items <= 0 || item_size <= 0) return 0;
    const int chunks = db_chunks(n_items, item_size);
    const int stride = (int)(2 * n_items);
    if ((((uintptr_t)out) & 15) == 0)            // 16-byte accesses on the aligned middle of every chunk
        hipLaunchKernelGGL(k_db_clamp<4>, dim3((unsigned)(n_items * chunks)), dim3(256), 0, st, out,
                           item_size, chunks, dyn, stats, slots, stride);
    else
        hipLaunchKernelGGL(k_db_clamp<1>, dim3((unsigned)(n_items * chunks)), dim3(256), 0, st, out,
                           item_size, chunks, dyn, stats, slots, stride);
    return launch_check("k_db_clamp");
}

// banded filterbank product on contiguous |X| rows (k_band_mel)
static int run_band_mel(const float* mag, const Geom& g, const float* fb, const MelSched& sch, const DbDev& dbd,
                        unsigned* stats, float* out, hipStream_t st) {
    // (k_band_mel's own atomics use slot 0; the other slots keep their initial values and drop out of the reduction)
    const size_t lds = sizeof(float) * (size_t)kBandRows * g.K;
    static LdsOptIn lds_opt_in;
    if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_band_mel))) return e;
    const long long nsteps = (g.total_frames + kBandRows - 1) / kBandRows;
    hipLaunchKernelGGL(k_band_mel, dim3(grid_1d(nsteps, 1, 256 * 8)), dim3(256), lds, st, mag, g, fb, sch, dbd, stats, out);
    return launch_check("k_band_mel");
}

static bool fused_nfft(int n_fft) { return n_fft == 512 || n_fft == 1024 || n_fft == 2048; }

static int64_t stats_region_bytes(int64_t batch) {
    int64_t b = 256 + (int64_t)sizeof(unsigned) * 2 * std::max<int64_t>(1, batch) * db_slots_cap(batch);
    return (b + 255) & ~(int64_t)255;
}
// ... plus the frame-contiguous complex spectrum the two-kernel path stages behind it
static int64_t mel_staged_bytes(int64_t batch, long long total_frames, int K) {
    return stats_region_bytes(batch) + (int64_t)sizeof(float) * 2 * total_frames * K;
}

// kpr_mel_workspace_bytes / kpr_mel_workspace_bytes_unpacked (unpacked: always the staged size)
static int64_t mel_workspace_bytes(const kpr_stft_geom* s, int n_filt, bool unpacked) {
    if (check_geom(s) || n_filt <= 0) return -1;
    // two-kernel path (stages the complex spectrum): every n_fft without a fused kernel, and filterbanks with more
    // 16-filter tiles than the tile-synchronous kernel's schedule holds (banks without a band plan of more than 256 filters are
    // beyond k_mel_ts, and beyond k_mel_ws whenever a consumer's slice exceeds 64 chunks -- always at n_fft 512; ADVICE r05: such a
    // call used to fail with KPR_E_WORKSPACE once k_mel_fused, the catch-all of round 1, was gone).  A bank of at most 256
    // filters that neither kernel's schedule holds (dense matrices) still needs kpr_mel_workspace_bytes_unpacked(): the call then
    // fails with KPR_E_WORKSPACE and names that size; the Python layer retries with it.
    if (unpacked || !fused_nfft(s->n_fft) || (n_filt + 15) / 16 > kTsMaxTiles)
        return mel_staged_bytes(s->batch, s->batch * s->channels * frames_of(s), s->n_fft / 2 + 1);
    return stats_region_bytes(s->batch);
}

enum { MEL_PW, MEL_PW_PAIR, MEL_TS, MEL_WS, MEL_MR, MEL_STAGED };     // MEL_STAGED: an STFT into the workspace, then a product
enum { PROD_GEMM, PROD_WS, PROD_BAND };                                 // the product of MEL_STAGED

struct MelRoute {
    int fam;
    int cfast;                 // Geom::cfast of the launch
    int w;                     // MEL_PW: waves per workgroup
    int plain;                 // MEL_PW: the plain-output instance k_mel_plain_pw (launch_mel_pw_plain)
    int cl_slots;              // MEL_PW_PAIR: mel_pw_pair_slots
    int rf64;                  // MEL_TS: the 64-frame-round instance (n_fft 512)
    int ws_form;               // MEL_WS, PROD_WS: mel_ws_form
    MelSchedTs ts;             // MEL_TS, MEL_MR
    StftRoute stage;           // MEL_STAGED: the STFT that stages the frame-contiguous spectrum
    int stage_mode;            //   complex, or |X| for PROD_WS / PROD_BAND
    int product;
    int64_t workspace;         // bytes the call needs
};

// s: the cropped geometry, g: its Geom; packed: a verified packed filterbank (pi: its band plan), kr: k-ranges (NULL: dense)
static MelRoute mel_route(const kpr_stft_geom* s, const Geom& g, int M, bool packed, const PackInfo& pi, const MelSched& sch,
                          const int32_t* kr, const float* out, int cus, bool db_on) {
    MelRoute r{};
    const int n_fft = s->n_fft, mv = opt(OPT_MEL_VARIANT);
    const bool fits = g.total_frames < 0x7fffff00LL;
    // channel-fastest frame numbering: the C frames that share cache lines sit in one wave
    const int cfast = (g.in_cl && g.C > 1) ? 1 : 0;
    // k_mel_pw (round 4): n_fft 256 ... 2048 with a band plan in the packed filterbank (mel / triangular banks) -- the
    // default since round 4 (same-box sweeps against k_mel_ws / k_mel_ts / the ring kernel: tools/sweep_dispatch.py mel).
    // mel_variant 5 / 6 / 7 = k_mel_pw with 8 / 4 / 16 waves per workgroup, 8 = its PAIR form where it applies (A/B runs, tests).
    if (packed && pi.band_off && (fused_nfft(n_fft) || n_fft == 256) && s->win_length <= n_fft && (int)pi.L * kPts == g.K - 1 &&
        fits && (mv >= 5 || mv == 0)) {
        r.cfast = cfast;
        // waves per workgroup: sixteen (one workgroup per CU, one copy of the tables, tickets shared by the whole CU) once
        // there are sixteen tickets per CU; smaller launches are spread over more, smaller workgroups
        const long long tickets_w = (g.total_frames + (64 / (n_fft / 32)) - 1) / (64 / (n_fft / 32));
        // (tools/sweep_dispatch.py mel, gpurun_out/r04i: 8-wave workgroups win from ~4 tickets per CU up -- 8.2 vs 9.1 us at
        //  1328 tickets -- and 16-wave ones from 16 per CU: 14.8 vs 15.9 vs 17.6 us at 5312)
        const int w_auto = tickets_w >= 16LL * cus ? 16 : tickets_w >= 4LL * cus ? 8 : 4;
        r.w = mv == 6 ? 4 : mv == 7 ? 16 : mv == 5 ? 8 : w_auto;
        // interleaved waveforms with an even channel count, launches that fill the chip: the PAIR form (kpr_mel_pw_kernels.h).
        // n_fft 1024 stereo stays on the plain kernel (its stereo pair fetch does the same at four waves per SIMD).
        // mel_variant 8 forces it wherever it applies (tests), 5 / 6 / 7 never take it.
        const bool pair_ok = cfast && (g.C % 2) == 0 && (n_fft == 2048 || n_fft == 1024);
        const bool pair_auto = pair_ok && (n_fft == 2048 || g.C >= 4) && tickets_w >= 24LL * cus;
        r.fam = MEL_PW;
        // n_fft 2048 without decibels on contiguous rows, linear output rows, the (NR, CMQ) = (2, 1) plan (128 mel filters at 44.1 kHz):
        // the plain-output instance ("mel_pw_plain" 0 = never: A/B runs, tests); `fits` keeps total_frames below 2^31
        r.plain = n_fft == 2048 && !db_on && (g.C == 1 || (!g.in_cl && !g.out_cl)) && pi.L == 64 && pi.NR == 2 && pi.CMQ == 1 &&
                  opt(OPT_MEL_PW_PLAIN) != 0;
        if (pair_ok && (mv == 8 || (mv == 0 && pair_auto))) {
            Geom gk = g;
            gk.cfast = cfast;
            r.fam = MEL_PW_PAIR;
            r.cl_slots = mel_pw_pair_slots(gk, pi, M, out);
        }
        return r;
    }
    // k_mel_ts when its schedule holds the bank (fills r.ts)
    auto ts = [&]() {
        // n_fft 512, long runs (>= 64 k frames, two 64-frame rounds per workgroup): 64-frame rounds, two tickets per wave
        // (256 x 2 x 1 s @22 kHz, dB: 61 vs 65 us; 43 k frames mono: 29.7 vs 27.6, hence the threshold)
        r.rf64 = n_fft == 512 && g.total_frames >= 65536 && mel_ts_ok(n_fft, g.K, M, kr, g, &r.ts, 64);
        if (!r.rf64 && !mel_ts_ok(n_fft, g.K, M, kr, g, &r.ts)) return false;
        r.fam = MEL_TS;
        r.cfast = cfast;
        return true;
    };
    if (fused_nfft(n_fft) && packed) {
        // Banks WITHOUT a band plan (log-frequency banks, dense matrices) or a forced variant: the MFMA kernels.
        // mel_variant: 0 = automatic, 2 = k_mel_ws with a streamed filterbank slice, 3 = k_mel_ws wherever it applies,
        // 4 = the tile-synchronous kernel k_mel_ts wherever it applies (A/B runs, tests).  The round-1 4-wave ring kernel
        // (k_mel_fused, mel_variant 1) lost on every shape of tools/sweep_dispatch.py (profiles/r05_sweep_before_prune.log:
        // within 4 % of k_mel_ts on launches of a few thousand frames at n_fft 512, 25-95 % behind elsewhere) and was
        // removed in round 5.
        // k_mel_ts: n_fft 512 (sweep, log-frequency bank: 38.6 vs 58.8 us on 256 x 1 s @22 kHz; 14.0 vs 13.4 on 16 clips),
        // interleaved stereo at n_fft 1024 (pair fetch: 126 vs 180 us on 64 x 2 x 10 s @16 kHz), n_fft 1024 from ~12 k frames
        // up (32-frame rounds: 6-9 % faster than k_mel_ws on 256 x 10 s @16 kHz); k_mel_ws for the rest of n_fft 1024 / 2048
        const bool stereo_cl = g.in_cl && g.C == 2 && n_fft == 1024;
        const bool long_1024 = n_fft == 1024 && g.total_frames >= 12288;
        if ((mv == 4 || (mv == 0 && (n_fft == 512 || stereo_cl || long_1024))) && ts()) return r;
        // (the consumers keep one lane of schedule per chunk of their slice)
        if ((n_fft == 2048 || n_fft == 1024) && slice_max(sch) <= 64 && fits && mel_ws_lds_bytes(n_fft / 2, sch.nseg) <= 160 * 1024) {
            r.fam = MEL_WS;
            r.cfast = cfast;
            r.ws_form = mel_ws_form(sch, false, g.K);
            return r;
        }
        // what k_mel_ws cannot take (very wide banks): k_mel_ts if its schedule holds the bank, else the two-launch path below
        if (ts()) return r;
    }
    // n_fft 256 (round 3): the tile-synchronous kernel takes it too (eight lanes per frame, 64-frame rounds); mel_variant 3
    // keeps the two-launch path
    if (packed && n_fft == 256 && s->win_length <= n_fft && mv != 3 && ts()) return r;
    // mixed-radix sizes (n_fft 400, 320, 640 ...: speech front ends): one launch as well (k_mel_mr);
    // kpr_set_option("mel_variant", 3) keeps the two-launch path of round 2 (A/B runs, tests)
    if (packed && mixed_radix_plan(n_fft) && opt(OPT_MIXED_RADIX) && s->win_length <= n_fft && mv != 3 &&
        (M + 15) / 16 <= kTsMaxTiles && fits) {
        bool ok = false;
        with_mr(n_fft, [&](auto ff) {
            using FF = typename decltype(ff)::type;
            // no schedule, or more LDS than a CU has: the two-launch path
            ok = get_sched_ts(FF::N + 1, M, kr, mel_mr_nt<FF>(), 0, kMrWaves, &r.ts) == 0 && mel_mr_lds_bytes<FF>(r.ts.nslots) <= 160 * 1024;
            return 0;
        });
        if (ok) {
            r.fam = MEL_MR;
            r.cfast = cfast;
            return r;
        }
    }
    // two-kernel path: STFT (frame-contiguous) -> (|.| x filterbank) product [+ dB]
    r.fam = MEL_STAGED;
    r.workspace = mel_staged_bytes(s->batch, g.total_frames, g.K);
    r.stage = StftRoute{fft_family(s), STFT_K, 0, 0};
    r.stage_mode = KPR_OUT_COMPLEX;
    r.product = PROD_GEMM;
    if (r.stage.fam == FAM_POW2) {             // Stockham STFT (n_fft = 256, or no packed filterbank given)
        Geom gc = g;
        gc.out_cl = 0;
        r.stage.kernel = stft_pow2_kernel(gc, KPR_OUT_COMPLEX, cus);
    } else if (r.stage.fam == FAM_MR || r.stage.fam == FAM_BS) {
        // even non-power-of-two n_fft: wide packed filterbank: |X| rows straight into the fused kernel's MFMA consumers
        // (loader producers, FROM_MAG) instead of the complex spectrum + generic GEMM
        if (packed && g.K <= 1025 && slice_max(sch) <= 64 && !g.out_cl && fits && mel_ws_lds_bytes(1024, sch.nseg, 2) <= 160 * 1024) {
            r.stage_mode = KPR_OUT_MAGNITUDE;
            r.product = PROD_WS;
            r.ws_form = mel_ws_form(sch, true, g.K);
        } else if (kr) {                       // e.g. channels_last output with several channels: |X| rows + banded product
            r.stage_mode = KPR_OUT_MAGNITUDE;
            r.product = PROD_BAND;
        }
    } else if (r.stage.fam == FAM_BIG && kr) {
        // n_fft 4096 / 8192: |X| rows, then the banded product (a mel / log bank has ~2 K non-zeros: bandwidth work)
        r.stage_mode = KPR_OUT_MAGNITUDE;
        r.product = PROD_BAND;
    }
    return r;
}

// ---- kpr_mel_f32: checks, the packed filterbank, route, launch [+ the decibel clamp] ----
static int run_mel_f32(const float* x, const kpr_stft_geom* s, const float* window, const float* fb, const float* fb_packed, int n_filt,
                       const int32_t* fb_kranges_host, const kpr_db_params* db, float* out, void* workspace, int64_t workspace_bytes,
                       kpr_stream_t stream) {
    if (int e = check_geom(s)) return e;
    if (int e = check_db(db)) return e;
    if (n_filt <= 0) return fail(KPR_E_BADARG, "n_filt must be positive");
    const long long F = frames_of(s);
    const int64_t need = mel_workspace_bytes(s, n_filt, false);
    const kpr_stft_geom se = forward_geom(s);                    // win_length > n_fft: cropped frames (see forward_geom)
    s = &se;
    Geom g = make_geom(s, F);
    if (g.total_frames == 0) return 0;
    if (!x || !window || !fb || !out)
        return fail(KPR_E_BADARG, "x / window / fb / out must not be NULL");
    if (!workspace || workspace_bytes < need)
        return fail(KPR_E_WORKSPACE, "mel workspace: need %lld bytes", (long long)need);
    hipStream_t st = (hipStream_t)stream;
    MelSched sch{};
    const int sched_rc = get_sched(g.K, n_filt, fb_kranges_host, &sch);
    if (sched_rc != 0 && sched_rc != KPR_E_UNSUPPORTED) return sched_rc;          // malformed k-ranges etc.: report
    const bool have_sched = sched_rc == 0;                                         // UNSUPPORTED: more tiles than the
    if (!have_sched) { fb_packed = nullptr; fb_kranges_host = nullptr; }           // schedule holds -> dense GEMM
    PackInfo pinfo{0, 0, 0, 0, 0};
    const float* blob = fb_packed;
    if (fb_packed) {
        if (int e = verify_packed(fb_packed, g.K, n_filt, fb_kranges_host, sch, st, &pinfo)) return e;
        fb_packed += kPackHeaderFloats;
    }
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const MelRoute r = mel_route(s, g, n_filt, blob != nullptr, pinfo, sch, fb_kranges_host, out, cus, db && db->enabled);
    if (workspace_bytes < r.workspace)
        return fail(KPR_E_WORKSPACE, "mel workspace (unpacked filterbank path): need %lld bytes", (long long)r.workspace);
    DbDev dbd = make_db(db);
    unsigned* stats = reinterpret_cast<unsigned*>(workspace);
    const int slots = dbd.enabled ? db_slots(s->batch) : 1;       // statistics slots per item (small batches, see DbDev)
    if (dbd.enabled) {
        dbd.slot_mask = slots - 1;
        dbd.slot_stride = (int)(2 * s->batch);
        if (int e = stats_init(stats, (long long)s->batch * slots, st)) return e;
    }
    g.cfast = r.cfast;
    const float2* tw = nullptr;
    if (r.fam != MEL_STAGED)
        if (int e = get_twiddles(s->n_fft, &tw)) return e;
    auto run = [&]() -> int {
        switch (r.fam) {
            case MEL_PW:
                if (r.plain) return launch_mel_pw_plain_w(r.w, x, g, window, tw, blob, pinfo, n_filt, out, st);
                return with_pow2(s->n_fft / 2, [&](auto nc) {
                    return launch_mel_pw_w<nc>(r.w, x, g, window, tw, blob, pinfo, n_filt, dbd, stats, out, st);
                });
            case MEL_PW_PAIR:
                return with_pow2(s->n_fft / 2, [&](auto nc) {
                    if constexpr (nc >= 512) return launch_mel_pw_pair<nc>(x, g, window, tw, blob, pinfo, n_filt, r.cl_slots, dbd, stats, out, st);
                    else return no_instance("k_mel_pw_pair");
                });
            case MEL_TS:
                if (r.rf64) return launch_mel_ts<256, 64>(x, g, window, tw, fb_packed, r.ts, dbd, stats, out, st);
                return with_pow2(s->n_fft / 2, [&](auto nc) {
                    return launch_mel_ts<nc>(x, g, window, tw, fb_packed, r.ts, dbd, stats, out, st);
                });
            case MEL_WS:
                return with_pow2(s->n_fft / 2, [&](auto nc) {
                    if constexpr (nc >= 512) return launch_mel_ws<nc>(r.ws_form, x, g, window, tw, fb_packed, sch, dbd, stats, out, st);
                    else return no_instance("k_mel_ws");
                });
            case MEL_MR:
                return with_mr(s->n_fft, [&](auto ff) {
                    return launch_mel_mr_inst<typename decltype(ff)::type>(x, g, window, tw, fb_packed, r.ts, dbd, stats, out, st);
                });
        }
        float* spec = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + stats_region_bytes(s->batch));
        Geom gc = g;
        gc.out_cl = 0;
        if (int e = launch_stft(r.stage, x, gc, window, r.stage_mode, spec, cus, st)) return e;
        if (r.product == PROD_WS) return launch_mel_ws<1024, true>(r.ws_form, spec, g, nullptr, nullptr, fb_packed, sch, dbd, stats, out, st);
        if (r.product == PROD_BAND) return run_band_mel(spec, g, fb, sch, dbd, stats, out, st);
        GemmArgs ga{};
        ga.in = frames_contig_map(g, g.K);
        ga.out = frames_out_map(g, n_filt);
        ga.Kdim = g.K; ga.N = n_filt; ga.ldb = n_filt;
        ga.db = dbd; ga.stats = stats;
        if (fb_kranges_host) {
            ga.has_kr = 1;
            for (int t = 0; t < sch.ntiles; ++t) { ga.klo[t] = sch.klo[t]; ga.khi[t] = sch.khi[t]; }
        }
        return dbd.enabled ? run_gemm<A_CABS, E_DB>(spec, fb, ga, out, st) : run_gemm<A_CABS, E_PLAIN>(spec, fb, ga, out, st);
    };
    if (int e = run()) return e;
    return dbd.enabled ? db_clamp(out, s->batch, (long long)s->channels * F * n_filt, dbd.dyn, stats, st, slots) : 0;
}

// narrow matrices (LogmelToMFCC's DCT, small filterbanks) on contiguous rows of a multiple of four floats: the thin GEMM
static bool thin_gemm_shape(int n_freq, int n_filt) { return (n_filt + 15) / 16 <= 4 && n_freq <= 512 && (n_freq & 3) == 0; }

// the Geom of a row product: `rows` rows of n_freq bins, interleaved = channel-fastest rows (channels_last, C > 1)
static Geom rows_geom(long long rows, long long frames, int channels, int n_freq, bool interleaved) {
    Geom g{};
    g.total_frames = rows; g.T = 0; g.F = (int)frames; g.C = channels;
    g.n_fft = 2 * (n_freq - 1); g.win = 0; g.hop = 0; g.pad_left = 0; g.K = n_freq;
    g.in_cl = 0; g.out_cl = interleaved ? 1 : 0; g.cfast = interleaved ? 1 : 0;
    geom_set_magic(g);
    return g;
}

enum { FB_PW, FB_WS, FB_BAND, FB_UNPACKED };      // FB_UNPACKED: run_apply_filterbank_f32 (thin GEMM or generic GEMM)

// calls whose packed filterbank is verified (get_sched + verify_packed) ahead of fb_route
static bool fb_packed_candidate(const float* x, const float* fb_packed, const float* out, long long rows, int n_freq, int n_filt) {
    return fb_packed && x && out && rows > 0 && rows < 0x7fffff00LL && n_freq <= 1025 && !thin_gemm_shape(n_freq, n_filt);
}
// verified: the packed header was verified (pi, sch); band_sch: the schedule FB_BAND runs with
static int fb_route(bool verified, const PackInfo& pi, const MelSched& sch, const float* x, const float* fb, const float* out,
                    long long rows, int channels, int n_freq, int n_filt, bool contiguous, const int32_t* kr, MelSched* band_sch) {
    if (verified) {
        // a bank with a band plan (mel / triangular banks; n_freq - 1 a multiple of four up to 1024: every even n_fft / 4): the banded
        // row kernel (round 6; 21 248 x 1025 -> 128: k_mel_ws 35 / 41 us, this one 19 / 25 -- same buffers / rotating) on contiguous rows
        // and on rows of TWO interleaved channels (channels_last stereo: the ST instances; 10 624 blocks of 1025 bins: 38 / 44 ->
        // 25 / 30 us, a single-block launch 8.1 -> 6.9).  More channels stay on the MFMA kernels (kpr_fb_pw_kernels.h).
        // fb_variant 1 = never (A/B runs, tests).
        if (pi.band_off && fb && (contiguous || channels == 2) && opt(OPT_FB_VARIANT) != 1 && pi.L >= 8 && pi.L <= 64) return FB_PW;
        // (channels_last with C > 1: the loader waves read rows strided by C, channel-fastest row order)
        if (slice_max(sch) <= 64 && mel_ws_lds_bytes(1024, sch.nseg, 2) <= 160 * 1024) return FB_WS;
    }
    // long contiguous rows of a banded matrix (K = 2049 / 4097 bins after an n_fft 4096 / 8192 STFT: beyond the
    // MFMA consumers' tile): the banded product instead of the generic GEMM
    if (x && out && fb && contiguous && rows > 0 && rows < 0x7fffff00LL && n_freq > 1025 && kr &&
        sizeof(float) * (size_t)kBandRows * n_freq <= 160 * 1024 && get_sched(n_freq, n_filt, kr, band_sch) == 0)
        return FB_BAND;
    return FB_UNPACKED;
}

// ---- kpr_apply_filterbank_f32: the thin GEMM on its shapes, else the generic GEMM (with the k-ranges, if given) ----
static int run_apply_filterbank_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout, const float* fb,
                                    int n_filt, const int32_t* fb_kranges_host, float* out, kpr_stream_t stream) {
    if (int e = check_rows_args(batch, channels, frames, n_freq, n_filt, layout, "bad sizes", "bad layout enum")) return e;
    const long long rows = batch * channels * frames;
    if (rows == 0) return 0;
    if (!x || !fb || !out) return fail(KPR_E_BADARG, "x / fb / out must not be NULL");
    const int ntiles = (n_filt + 15) / 16;
    if (ntiles > kMaxTiles || n_freq > 32000) fb_kranges_host = nullptr;   // GemmArgs holds 16-bit k-ranges for 64 tiles: dense product
    const bool contiguous = layout == KPR_CHANNELS_FIRST || channels == 1;
    if (contiguous && thin_gemm_shape(n_freq, n_filt) && (((uintptr_t)x) & 15) == 0) {
        const size_t lds = sizeof(float) * 4 * 64 * (size_t)ntiles * ((n_freq + 15) / 16);
        const unsigned grid = (unsigned)std::min<long long>((rows + 63) / 64, 256 * 8);
        hipStream_t st = (hipStream_t)stream;
        // thin_gemm_shape admits up to 4 tiles x 32 k-groups = 128 KiB of B fragments: above 64 KiB the instance opts in
        auto launch = [&](auto nt) -> int {
            static LdsOptIn lds_opt_in;
            if (lds > 64 * 1024)
                if (int e = allow_big_lds(lds_opt_in, reinterpret_cast<const void*>(&k_thin_gemm<nt>))) return e;
            hipLaunchKernelGGL(k_thin_gemm<nt>, dim3(grid), dim3(256), lds, st, x, rows, n_freq, fb, n_filt, out);
            return launch_check("k_thin_gemm");
        };
        switch (ntiles) {
            case 1: return launch(std::integral_constant<int, 1>{});
            case 2: return launch(std::integral_constant<int, 2>{});
            case 3: return launch(std::integral_constant<int, 3>{});
            default: return launch(std::integral_constant<int, 4>{});
        }
    }
    GemmArgs ga{};
    ga.in.rows = rows; ga.out.rows = rows;
    if (layout == KPR_CHANNELS_LAST) {
        // rows r = (b*F + f)*C + c
        ga.in.D0 = channels; ga.in.D1 = 1;
        ga.in.s2 = (long long)n_freq * channels; ga.in.s1 = 0; ga.in.s0 = 1; ga.in.es = channels;
        ga.out.D0 = channels; ga.out.D1 = 1;
        ga.out.s2 = (long long)n_filt * channels; ga.out.s1 = 0; ga.out.s0 = 1; ga.out.es = channels;
    } else {
        ga.in.D0 = 1; ga.in.D1 = 1; ga.in.s2 = n_freq; ga.in.s1 = 0; ga.in.s0 = 0; ga.in.es = 1;
        ga.out.D0 = 1; ga.out.D1 = 1; ga.out.s2 = n_filt; ga.out.s1 = 0; ga.out.s0 = 0; ga.out.es = 1;
    }
    ga.Kdim = n_freq; ga.N = n_filt; ga.ldb = n_filt;
    if (fb_kranges_host) {
        const int kp = (n_freq + 3) & ~3;
        ga.has_kr = 1;
        for (int t = 0; t < ntiles; ++t) {
            int lo = fb_kranges_host[2 * t], hi = fb_kranges_host[2 * t + 1];
            if (lo < 0 || hi > kp || lo > hi) return fail(KPR_E_BADARG, "bad k-range");
            ga.klo[t] = (short)lo; ga.khi[t] = (short)hi;
        }
    }
    return run_gemm<A_PLAIN, E_PLAIN>(x, fb, ga, out, (hipStream_t)stream);
}

// ---- kpr_apply_filterbank_packed_f32: the kernels of a verified packed filterbank (fb_route), else the body above ----
static int run_apply_filterbank_packed_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                                           const float* fb, const float* fb_packed, int n_filt, const int32_t* fb_kranges_host,
                                           float* out, kpr_stream_t stream) {
    if (int e = check_rows_args(batch, channels, frames, n_freq, n_filt, layout, "bad sizes", "bad layout enum")) return e;
    const long long rows = batch * channels * frames;
    const bool contiguous = layout == KPR_CHANNELS_FIRST || channels == 1;
    hipStream_t st = (hipStream_t)stream;
    MelSched sch{};
    PackInfo pinfo{0, 0, 0, 0, 0};
    const bool verified = fb_packed_candidate(x, fb_packed, out, rows, n_freq, n_filt) &&
                          get_sched(n_freq, n_filt, fb_kranges_host, &sch) == 0;
    if (verified)
        if (int e = verify_packed(fb_packed, n_freq, n_filt, fb_kranges_host, sch, st, &pinfo)) return e;
    switch (fb_route(verified, pinfo, sch, x, fb, out, rows, channels, n_freq, n_filt, contiguous, fb_kranges_host, &sch)) {
        case FB_PW:
            return with_pow2((int)pinfo.L * kPts, [&](auto nc) {
                return contiguous ? launch_fb_pw<nc, false>(x, rows, n_freq, fb_packed, pinfo, n_filt, fb, out, st)
                                  : launch_fb_pw<nc, true>(x, rows / 2, n_freq, fb_packed, pinfo, n_filt, fb, out, st);
            });
        case FB_WS:
            return launch_mel_ws<1024, true>(mel_ws_form(sch, true, n_freq), x, rows_geom(rows, frames, channels, n_freq, !contiguous),
                                             nullptr, nullptr, fb_packed + kPackHeaderFloats, sch, make_db(nullptr), nullptr, out, st);
        case FB_BAND:
            return run_band_mel(x, rows_geom(rows, frames, channels, n_freq, false), fb, sch, make_db(nullptr), nullptr, out, st);
        default:
            return run_apply_filterbank_f32(x, batch, channels, frames, n_freq, layout, fb, n_filt, fb_kranges_host, out, stream);
    }
}

}  // namespace kpr
