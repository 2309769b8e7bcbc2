// kpr_host.h -- host side shared by every kernel family: options, once-per-device state, launch log, device status word, LDS opt-in,
// CU count, with_vec, geometry checks (ranges_overlap, col_launch for the time-tiled kernels), the GEMM launcher, the device-table cache,
// the launcher of the framewise FFT kernels.
// Part of the single translation unit kapre_hip.hip (after the kernel headers, before kpr_host_fft.h / _stft.h / _istft.h / _mel.h / _ops.h).
#pragma once

namespace kpr {

static std::mutex g_mu;             // the caches of every family (device tables, schedules, verified packed filterbanks)

// Process-wide tuning switches (kpr_set_option): plain atomics, read on the launch path.  The
// library never reads the process environment.
enum { OPT_MEL_VARIANT, OPT_ISTFT_PATH, OPT_MIXED_RADIX, OPT_DB_CHUNKS, OPT_VERBOSE, OPT_STFT_VARIANT, OPT_DB_SLOTS, OPT_MEL_CL_STAGE, OPT_FB_VARIANT, OPT_MEL_PW_PLAIN,
       OPT_CMVN_VARIANT, OPT_LFILTER_VARIANT, OPT_ADDNOISE_VARIANT, OPT_COUNT };
static std::atomic<int> g_opt[OPT_COUNT] = {{0}, {0}, {1}, {0}, {0}, {0}, {0}, {1}, {0}, {1}, {0}, {0}, {0}};
static inline int opt(int id) { return g_opt[id].load(std::memory_order_relaxed); }

static int option_id(const char* name) {
    static const char* const names[OPT_COUNT] = {"mel_variant", "istft_path", "mixed_radix", "db_chunks", "verbose", "stft_variant", "db_slots",
                                                  "mel_cl_stage", "fb_variant", "mel_pw_plain", "cmvn_variant", "lfilter_variant", "addnoise_variant"};
    if (name)
        for (int i = 0; i < OPT_COUNT; ++i)
            if (std::strcmp(name, names[i]) == 0) return i;
    return -1;
}

static int cur_device(int* dev) {
    KPR_HIP(hipGetDevice(dev));
    return 0;
}

// State that is set up once per device: one entry per HIP device index 0 ... 63.  device_slot() is the only hipGetDevice of
// everything built on it; an index outside that range has no slot (-1), and every user states its own rule for that case.
constexpr int kDeviceSlots = 64;
template <class T>
struct PerDevice { T at[kDeviceSlots] = {}; };
static int device_slot(int* slot) {
    int dev = 0;
    KPR_HIP(hipGetDevice(&dev));
    *slot = (dev >= 0 && dev < kDeviceSlots) ? dev : -1;
    return 0;
}

static int grid_1d(long long n, int block, int cap = 256 * 16) {
    long long b = (n + block - 1) / block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// Names of the kernels this thread's most recent API call launched, in order ("k_stats_init + k_mel_pw<1024> + k_db_clamp");
// kpr_last_launches() hands it to diagnostics (bench.py prints it as roofline.kernel instead of a table of its own).
// The entry points that launch the hot kernels clear it on entry (launch_log_begin).
static thread_local std::string g_launches;
static void launch_log_begin() { g_launches.clear(); }

// ---- the device status word (kpr_common.h): one word of mapped, coherent host memory per process ------------------------------
struct StatusWord {
    std::mutex mu;
    std::atomic<unsigned*> host{nullptr};   // what the host reads (volatile); written once under `mu`, read without it by every call
    PerDevice<bool> installed;        // g_status_word of that device points at it
};
static StatusWord g_status;
// called by the launchers of the kernels that can raise it; everything is done once per device (a device without a slot: nothing)
static int status_word_ready() {
    int slot;
    if (int e = device_slot(&slot)) return e;
    if (slot < 0) return 0;
    std::lock_guard<std::mutex> lock(g_status.mu);
    if (g_status.installed.at[slot]) return 0;
    // (a first call under stream capture: the allocation and the symbol copy are not stream work)
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    int rc = 0;
    do {
        unsigned* hostp = g_status.host.load(std::memory_order_acquire);
        if (!hostp) {
            void* h = nullptr;
            hipError_t e = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
            if (e != hipSuccess) { rc = fail(KPR_E_HIP, "hipHostMalloc (status word) failed: %s", hipGetErrorString(e)); break; }
            *static_cast<volatile unsigned*>(h) = 0u;
            hostp = static_cast<unsigned*>(h);
            g_status.host.store(hostp, std::memory_order_release);
        }
        void* d = nullptr;
        hipError_t e = hipHostGetDevicePointer(&d, hostp, 0);
        if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_status_word), &d, sizeof d);
        if (e != hipSuccess) { rc = fail(KPR_E_HIP, "installing the status word failed: %s", hipGetErrorString(e)); break; }
        g_status.installed.at[slot] = true;
    } while (0);
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    return rc;
}
static const char* status_text(unsigned bits) {
    static thread_local char buf[384];
    snprintf(buf, sizeof buf, "0x%08x:%s%s%s%s%s%s%s", bits, (bits & kStMelWs) ? " k_mel_ws(bounded wait ran out)" : "",
             (bits & kStIstftWsCons) ? " k_istft_ws(consumer: bounded wait ran out)" : "",
             (bits & kStIstftWsProd) ? " k_istft_ws(producer: bounded wait ran out)" : "",
             (bits & kStIstftPw) ? " k_istft_pw(bounded wait ran out)" : "",
             (bits & kStMelPwSlot) ? " k_mel_pw_pair(bounded wait ran out)" : "",
             (bits & kStStalePlan) ? " k_mel_pw / k_fb_pw(the packed filterbank changed under a cached band plan: kpr_filterbank_forget)" : "",
             (bits & kStSelfTest) ? " self-test(bounded wait ran out)" : "");
    return buf;
}
// `detail`: the template arguments beyond the transform size that pick the INSTANCE ("s4", "w16", "rj4,v2" ...): the fuzz gate of
// tests/test_fuzz_gate.py asserts that every instance of the large-launch kernels was reached, not just every family
static int launch_check(const char* what, int tag = 0, const char* detail = nullptr) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(KPR_E_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    if (g_launches.size() < 200) {
        if (!g_launches.empty()) g_launches += " + ";
        g_launches += what;
        if (tag) {
            char b[48];
            if (detail) snprintf(b, sizeof b, "<%d,%s>", tag, detail);
            else snprintf(b, sizeof b, "<%d>", tag);
            g_launches += b;
        }
    }
    return 0;
}

// Kernels that use more than 64 KiB of dynamic LDS must opt in, once per (kernel, device).
// (benign race: the call is idempotent; a device without a slot sets the attribute every time)
typedef PerDevice<bool> LdsOptIn;
static int allow_big_lds(LdsOptIn& st, const void* fn) {
    int slot;
    if (int e = device_slot(&slot)) return e;
    if (slot < 0 || !st.at[slot]) {
        KPR_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if (slot >= 0) st.at[slot] = true;
    }
    return 0;
}

// compute units of the current device, asked once per device (a device without a slot: 256, not cached)
static int device_cus(int* cus) {
    static PerDevice<int> cached;
    int slot;
    if (int e = device_slot(&slot)) return e;
    *cus = 256;
    if (slot >= 0) {
        if (!cached.at[slot]) {
            int q = 0;
            KPR_HIP(hipDeviceGetAttribute(&q, hipDeviceAttributeMultiprocessorCount, slot));
            cached.at[slot] = q > 0 ? q : 256;
        }
        *cus = cached.at[slot];
    }
    return 0;
}

static long long* g_debug_stamps = nullptr;   // development aid: kpr_debug_stamps()

// the branch of a with_pow2 / with_mr body that the route never selects
static int no_instance(const char* what) { return fail(KPR_E_UNSUPPORTED, "no %s instance for this call", what); }

// wide -> f(std::integral_constant<int, VMAX>), else f(std::integral_constant<int, 1>): the vector-width instance of a kernel,
// picked at run time (with_pow2's idiom)
template <int VMAX, class Fn>
static auto with_vec(bool wide, Fn&& f) {
    if (wide) return f(std::integral_constant<int, VMAX>{});
    return f(std::integral_constant<int, 1>{});
}

// ---- geometry / validation ---------------------------------------------------------------------------------------------
// do the byte ranges [p, p + np) and [q, q + nq) overlap?  A NULL pointer names no range; ranges that touch do not overlap
static bool ranges_overlap(const void* p, uintptr_t np, const void* q, uintptr_t nq) {
    return p && q && (uintptr_t)p < (uintptr_t)q + nq && (uintptr_t)q < (uintptr_t)p + np;
}

// The launch shape of a time-tiled kernel (kpr_cols.h) over (outer, frames, inner): column groups of V columns where the caller's
// pointers are aligned for it and inner % V == 0, of one column otherwise; 64 groups per workgroup of `waves` waves.  inner,
// groups_per_item and n_groups go into the kernel's argument struct as they are.
struct ColLaunch {
    bool wide;
    unsigned inner, groups_per_item;
    long long n_groups;
    dim3 grid, block;
};
static int col_launch(int64_t outer, int64_t inner, int V, int waves, bool aligned, ColLaunch* l) {
    l->wide = aligned && inner % V == 0;
    l->inner = (unsigned)inner;
    l->groups_per_item = (unsigned)(l->wide ? inner / V : inner);
    l->n_groups = (long long)outer * l->groups_per_item;
    const long long blocks = (l->n_groups + 63) / 64;
    if (blocks > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "too many columns: outer * inner = %lld", (long long)(outer * inner));
    l->grid = dim3((unsigned)blocks);
    l->block = dim3(64 * waves);
    return 0;
}

static long long frames_of(const kpr_stft_geom* s) {
    long long t = s->time + (s->pad_begin ? (s->n_fft - s->hop_length) : 0);
    if (s->pad_end) return (t + s->hop_length - 1) / s->hop_length;
    if (t < s->win_length) return 0;
    return 1 + (t - s->win_length) / s->hop_length;
}

// Forward transforms with win_length > n_fft (time_frequency.py:174-182 hands both to tf.signal.stft): frames are cut with
// frame_length = win_length -- frames_of() and the right padding keep the caller's value -- and windowed, then rfft(fft_length)
// CROPS them to their first n_fft samples.  Everything behind the frame count therefore sees win_length = n_fft and the first n_fft
// entries of the caller's window: every FFT family takes these calls (through round 5 float32 fell back to the DFT-as-GEMM path and
// float64 refused them).
static kpr_stft_geom forward_geom(const kpr_stft_geom* s) {
    kpr_stft_geom e = *s;
    e.win_length = std::min(s->win_length, s->n_fft);
    return e;
}

static int check_geom(const kpr_stft_geom* s) {
    if (!s) return fail(KPR_E_BADARG, "geometry is NULL");
    if (s->batch < 0 || s->channels <= 0 || s->time < 0)
        return fail(KPR_E_BADARG, "bad batch/channels/time (%lld, %d, %lld)", (long long)s->batch,
                    s->channels, (long long)s->time);
    if (s->n_fft < 2 || s->win_length < 1 || s->hop_length < 1)
        return fail(KPR_E_BADARG, "bad n_fft/win_length/hop_length (%d, %d, %d)", s->n_fft,
                    s->win_length, s->hop_length);
    if ((unsigned)s->in_layout > 1u || (unsigned)s->out_layout > 1u)
        return fail(KPR_E_BADARG, "bad layout enum");
    if (s->pad_begin && s->n_fft < s->hop_length)
        return fail(KPR_E_BADARG, "pad_begin needs n_fft >= hop_length");
    // the kernels address one (batch item, channel) signal with 32-bit element offsets
    if (s->time * (long long)s->channels >= (1LL << 30))
        return fail(KPR_E_UNSUPPORTED, "time * channels = %lld elements per batch item: 2^30 or more is not supported",
                    (long long)(s->time * (long long)s->channels));
    return 0;
}

static Geom make_geom(const kpr_stft_geom* s, long long F) {
    Geom g;
    g.F = (int)F;
    g.C = s->channels;
    g.T = s->time;
    g.total_frames = s->batch * s->channels * F;
    g.n_fft = s->n_fft;
    g.win = s->win_length;
    g.hop = s->hop_length;
    g.pad_left = s->pad_begin ? (s->n_fft - s->hop_length) : 0;
    g.K = s->n_fft / 2 + 1;
    // with one channel the two layouts are the same memory image: take the contiguous paths
    // (Kapre's default is channels_last, so this is the common case)
    g.in_cl = s->in_layout == KPR_CHANNELS_LAST && s->channels > 1;
    g.out_cl = s->out_layout == KPR_CHANNELS_LAST && s->channels > 1;
    g.cfast = 0;
    geom_set_magic(g);
    return g;
}

// frame-row maps for GEMM paths: rows are global frames g = (b*C + c)*F + f
static RowMap frames_out_map(const Geom& g, long long Q) {
    RowMap m;
    m.rows = g.total_frames; m.D0 = g.F; m.D1 = g.C;
    if (g.out_cl) { m.s2 = (long long)g.F * Q * g.C; m.s1 = 1; m.s0 = Q * g.C; m.es = g.C; }
    else { m.s2 = (long long)g.C * g.F * Q; m.s1 = (long long)g.F * Q; m.s0 = Q; m.es = 1; }
    return m;
}
static RowMap frames_contig_map(Geom g, long long Q) {
    g.out_cl = 0;
    return frames_out_map(g, Q);
}

template <int AMODE, int EPI>
static int run_gemm(const float* a, const float* bm, const GemmArgs& ga, float* out,
                    hipStream_t st) {
    if (ga.in.rows <= 0 || ga.N <= 0) return 0;
    dim3 grid((unsigned)((ga.in.rows + 63) / 64), (unsigned)((ga.N + 63) / 64));
    hipLaunchKernelGGL((k_gemm<AMODE, EPI>), grid, dim3(256), 0, st, a, bm, ga, out);
    return launch_check("k_gemm");
}

// sizes and layout of a row product (the ApplyFilterbank entry points; each passes its own texts, layout_fmt may print the layout)
static int check_rows_args(int64_t batch, int channels, int64_t frames, int n_freq, int n_filt, int layout, const char* sizes_msg,
                           const char* layout_fmt) {
    if (batch < 0 || channels <= 0 || frames < 0 || n_freq <= 0 || n_filt <= 0) return fail(KPR_E_BADARG, "%s", sizes_msg);
    if ((unsigned)layout > 1u) return fail(KPR_E_BADARG, layout_fmt, layout);
    return 0;
}

// ---- device tables -----------------------------------------------------------------------------------------------------
// One table per (device, n_fft): build(n_fft, h) fills the host copy at first use, which is uploaded and kept for the process
// lifetime.  Lookup, build and upload run under g_mu.  (The upload is a blocking copy: not legal during stream capture, warm up first.)
template <class T, class Build>
static int cached_table(std::map<std::pair<int, int>, T*>& tables, int n_fft, Build&& build, const T** out) {
    int dev;
    if (int e = cur_device(&dev)) return e;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = tables.find({dev, n_fft});
    if (it == tables.end()) {
        std::vector<T> h;
        build(n_fft, h);
        T* d = nullptr;
        KPR_HIP(hipMalloc(&d, sizeof(T) * h.size()));
        KPR_HIP(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
        it = tables.emplace(std::make_pair(dev, n_fft), d).first;
    }
    *out = it->second;
    return 0;
}

// ---- the launch shape of the framewise FFT kernels ---------------------------------------------------------------------
// kern(args...) over `groups` units of work, `per_block` of them per workgroup of `threads`; at most `per_cu` workgroups per CU,
// fewer where their LDS does not fit that often.  opt_in: the kernel's LDS opt-in state (NULL: it stays under 64 KiB and has none);
// label and tag are launch_check's.
template <class Kern, class... Args>
static int launch_framewise(Kern kern, LdsOptIn* opt_in, long long groups, int per_block, int per_cu, unsigned threads, size_t lds,
                            hipStream_t st, const char* label, int tag, Args... args) {
    int cus = 256;
    if (opt_in)
        if (int e = allow_big_lds(*opt_in, reinterpret_cast<const void*>(kern))) return e;
    if (int e = device_cus(&cus)) return e;
    per_cu = std::max(1, std::min(per_cu, (int)(160 * 1024 / lds)));
    const long long grid = std::max<long long>(1, std::min<long long>((groups + per_block - 1) / per_block, (long long)per_cu * cus));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(threads), lds, st, args...);
    return launch_check(label, tag);
}

}  // namespace kpr
