// kpr_host_fft.h -- host side of the FFT building blocks (kpr_fft.h, kpr_fft_mr.h, kpr_generic_kernels.h): which transform sizes
// each family takes, the device tables (five builders over cached_table), with_pow2 / with_mr and the mixed-radix plan typedefs,
// the plan of the generic engine, fft_family, fft_plan (the body of kpr_fft_plan).
// Part of the single translation unit kapre_hip.hip (included there after kpr_host.h; not stand-alone).
#pragma once

namespace kpr {

static bool fast_nfft(int n_fft) {
    return n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048;
}

// n_fft 4096 / 8192: R = 2 / 4 sub-FFTs of 1024 points per frame (k_stft_big)
static bool big_nfft(int n_fft) { return n_fft == 4096 || n_fft == 8192; }

// Bluestein length M of an even n_fft that is not a power of two (k_stft_bs); 0: none
static int bluestein_m(int n_fft) {
    if (n_fft < 4 || (n_fft & 1)) return 0;
    const int ncr = n_fft / 2;
    int m = 128;
    while (m < 2 * ncr - 1) m *= 2;
    return m <= 1024 ? m : 0;
}

// ---- device tables: (device, n_fft) -> table (cached_table, kpr_host.h), one builder each ------------------------------------
// The float tables are computed in double precision with exactly reduced angles, the float64 twiddles in long double.
static std::map<std::pair<int, int>, float2*> g_tw, g_bs;           // twiddles, Bluestein tables
static std::map<std::pair<int, int>, float*> g_dft_fwd, g_dft_inv;  // [n_fft][2K], [2K][n_fft]
static std::map<std::pair<int, int>, double2*> g_tw64;

// twiddles: exp(-2 pi i j / n_fft), j < n_fft
static void build_twiddles(int n_fft, std::vector<float2>& h) {
    h.resize(n_fft);
    for (int j = 0; j < n_fft; ++j) {
        double a = -2.0 * M_PI * (double)j / (double)n_fft;
        h[j] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
}

// Bluestein tables for an even n_fft that is not a power of two (k_stft_bs), M = bluestein_m:
// [w: M][Bt: M][t: NCr + 1] as float2; Bt = FFT_M(chirp) / (2M) computed in double precision
static void build_bluestein(int n_fft, std::vector<float2>& h) {
    const int ncr = n_fft / 2, m = bluestein_m(n_fft);
    std::vector<double> wr(ncr), wi(ncr), br(m, 0.0), bi(m, 0.0);
    for (int n = 0; n < ncr; ++n) {
        const long long n2 = ((long long)n * n) % (2LL * ncr);           // exact angle reduction
        const double a = -M_PI * (double)n2 / (double)ncr;
        wr[n] = std::cos(a); wi[n] = std::sin(a);
    }
    for (int n = 0; n < ncr; ++n) { br[n] = wr[n]; bi[n] = -wi[n]; }
    for (int n = 1; n < ncr; ++n) { br[m - n] = wr[n]; bi[m - n] = -wi[n]; }
    // O(M^2) DFT of the chirp in double precision (once per n_fft and device; M <= 1024)
    h.resize(2 * (size_t)m + ncr + 1);
    for (int n = 0; n < m; ++n) h[n] = n < ncr ? make_float2((float)wr[n], (float)wi[n]) : make_float2(0.f, 0.f);
    for (int k = 0; k < m; ++k) {
        double sr = 0, si = 0;
        for (int n = 0; n < m; ++n) {
            if (br[n] == 0.0 && bi[n] == 0.0) continue;
            const double a = -2.0 * M_PI * (double)(((long long)k * n) % m) / (double)m;
            const double c = std::cos(a), sn = std::sin(a);
            sr += br[n] * c - bi[n] * sn;
            si += br[n] * sn + bi[n] * c;
        }
        h[m + k] = make_float2((float)(sr / (2.0 * m)), (float)(si / (2.0 * m)));
    }
    for (int k = 0; k <= ncr; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)n_fft;
        h[2 * (size_t)m + k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
}

// forward DFT matrix [n_fft rows n][2K cols]: col 2k = cos(2 pi k n/N), col 2k+1 = -sin(...)
// A sine whose exact value is 0 (k n mod N = 0 or N/2: the DC column, and the Nyquist column of an even N) is stored as 0, not as
// (float)sin(pi) = 1.2e-16: the imaginary parts of the DC and Nyquist bins of a real frame are then exact zeros, as rfft's are.
static void build_dft_fwd(int n_fft, std::vector<float>& h) {
    const int K = n_fft / 2 + 1;
    h.resize((size_t)n_fft * 2 * K);
    for (int n = 0; n < n_fft; ++n)
        for (int k = 0; k < K; ++k) {
            long long kn = ((long long)k * n) % n_fft;     // exact angle reduction
            double a = 2.0 * M_PI * (double)kn / (double)n_fft;
            h[(size_t)n * 2 * K + 2 * k] = (float)std::cos(a);
            h[(size_t)n * 2 * K + 2 * k + 1] = (2 * kn) % n_fft == 0 ? 0.0f : (float)(-std::sin(a));
        }
}

// inverse real DFT matrix [2K rows][n_fft cols]: row 2k = c_k cos(2 pi k n/N)/N,
// row 2k+1 = -c_k sin(2 pi k n/N)/N, c_k = 1 for DC (and Nyquist when N even) else 2
static void build_dft_inv(int n_fft, std::vector<float>& h) {
    const int K = n_fft / 2 + 1;
    h.resize((size_t)2 * K * n_fft);
    for (int k = 0; k < K; ++k) {
        const bool edge = (k == 0) || ((n_fft % 2 == 0) && k == n_fft / 2);
        const double ck = (edge ? 1.0 : 2.0) / (double)n_fft;
        for (int n = 0; n < n_fft; ++n) {
            long long kn = ((long long)k * n) % n_fft;
            double a = 2.0 * M_PI * (double)kn / (double)n_fft;
            h[(size_t)(2 * k) * n_fft + n] = (float)(ck * std::cos(a));
            h[(size_t)(2 * k + 1) * n_fft + n] = (edge || (2 * kn) % n_fft == 0) ? 0.0f : (float)(-ck * std::sin(a));
        }
    }
}

// float64 twiddles
static void build_twiddles64(int n_fft, std::vector<double2>& h) {
    h.resize(n_fft);
    for (int j = 0; j < n_fft; ++j) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)j / (long double)n_fft;
        h[j] = make_double2((double)cosl(a), (double)sinl(a));
    }
}

static int get_twiddles(int n_fft, const float2** out) { return cached_table(g_tw, n_fft, build_twiddles, out); }
static int get_bluestein(int n_fft, const float2** out) { return cached_table(g_bs, n_fft, build_bluestein, out); }
static int get_dft_fwd(int n_fft, const float** out) { return cached_table(g_dft_fwd, n_fft, build_dft_fwd, out); }
static int get_dft_inv(int n_fft, const float** out) { return cached_table(g_dft_inv, n_fft, build_dft_inv, out); }
static int get_twiddles64(int n_fft, const double2** out) { return cached_table(g_tw64, n_fft, build_twiddles64, out); }
// the twiddles of the generic engine's element type T (launch_stft_gen, launch_irfft_gen)
template <typename T>
static int twiddles_of(int n_fft, const typename Cplx<T>::type** out) {
    if constexpr (sizeof(T) == 4) return get_twiddles(n_fft, out);
    else return get_twiddles64(n_fft, out);
}

// n -> f(std::integral_constant<int, n>) for the power-of-two template sizes n = 128, 256, 512, 1024 (anything else: 1024) -- the
// half transform size NC = n_fft / 2 of the power-of-two kernels, the Bluestein length M, the bin count of k_fb_pw
template <class Fn>
static int with_pow2(int n, Fn&& f) {
    switch (n) {
        case 128: return f(std::integral_constant<int, 128>{});
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
        default:  return f(std::integral_constant<int, 1024>{});
    }
}

// ---- dispatch routes: which kernel (family, template instance, launch plan) a call runs, from host-side facts only --------
// The route functions (stft_route, mel_route, istft_route, fb_route next to their entry points) never launch and never
// synchronise; the launchers below take the route's plan and always launch.
enum { FAM_POW2, FAM_MR, FAM_BS, FAM_BIG, FAM_GEN, FAM_GEMM,            // FFT families (fft_family)
       IST_PW, IST_WS, IST_FUSED, IST_WS_MR };                          // one-launch inverse kernels (istft_route)

// Mixed-radix plans (kpr_fft_mr.h).  n_fft = 2^a 5^b: MrFft<R2, R3>, N = n_fft / 2 = 20 * R2 * R3;
// n_fft with a factor 3: TwoPassFft<N1, N2>, N = N1 * N2.
typedef MrFft<4, 1> Fft160;    typedef MrFft<5, 1> Fft200;    typedef MrFft<4, 2> Fft320;
typedef MrFft<10, 1> Fft400;   typedef MrFft<4, 4> Fft640;    typedef MrFft<20, 1> Fft800;
typedef MrFft<5, 5> Fft1000;
typedef TwoPassFft<8, 6> Fft96;     typedef TwoPassFft<4, 15> Fft120;   typedef TwoPassFft<8, 12> Fft192;
typedef TwoPassFft<8, 15> Fft240;   typedef TwoPassFft<12, 15> Fft360;  typedef TwoPassFft<16, 12> Fft384;
typedef TwoPassFft<16, 15> Fft480;  typedef TwoPassFft<20, 15> Fft600;  typedef TwoPassFft<15, 24> Fft720;
typedef TwoPassFft<16, 24> Fft768;  typedef TwoPassFft<20, 24> Fft960;
// (the smaller factor first where it matters: N1 values per lane are prefetched one ticket ahead, twice
//  over in the inverse kernels, and <24, .> spilled there)

// n_fft -> f(FftTag<plan>) for every size with a mixed-radix plan, none() for the others
template <class FF> struct FftTag { using type = FF; };
template <class Fn, class None>
static int with_mr(int n_fft, Fn&& f, None&& none) {
    switch (n_fft) {
        case 160: return f(FftTag<Fft160>{});   case 200: return f(FftTag<Fft200>{});    case 320: return f(FftTag<Fft320>{});
        case 400: return f(FftTag<Fft400>{});   case 640: return f(FftTag<Fft640>{});    case 800: return f(FftTag<Fft800>{});
        case 1000: return f(FftTag<Fft1000>{});
        case 96: return f(FftTag<Fft96>{});     case 120: return f(FftTag<Fft120>{});    case 192: return f(FftTag<Fft192>{});
        case 240: return f(FftTag<Fft240>{});   case 360: return f(FftTag<Fft360>{});    case 384: return f(FftTag<Fft384>{});
        case 480: return f(FftTag<Fft480>{});   case 600: return f(FftTag<Fft600>{});    case 720: return f(FftTag<Fft720>{});
        case 768: return f(FftTag<Fft768>{});   case 960: return f(FftTag<Fft960>{});
        default: return none();
    }
}
template <class Fn>
static int with_mr(int n_fft, Fn&& f) {
    return with_mr(n_fft, f, [&] { return fail(KPR_E_UNSUPPORTED, "no mixed-radix plan for n_fft %d", n_fft); });
}
template <class FF> struct IsTwoPass : std::false_type {};
template <int N1, int N2> struct IsTwoPass<TwoPassFft<N1, N2>> : std::true_type {};
// 1: MrFft plan (forward, inverse and ring-ISTFT kernels), 2: TwoPassFft plan (forward and inverse), 0: none
static int mixed_radix_plan(int n_fft) {
    return with_mr(n_fft, [](auto ff) { return IsTwoPass<typename decltype(ff)::type>::value ? 2 : 1; }, [] { return 0; });
}

template <class FF>
static size_t mr_lds_bytes() {
    constexpr int G = 64 / FF::L;
    return sizeof(float) * 2 * ((size_t)4 * G * mr_row_stride<FF>() + 3 * (size_t)FF::N);
}

// Bluestein STFT (even n_fft that is not a power of two, n_fft <= 1024, win_length <= n_fft)
static bool bluestein_ok(const kpr_stft_geom* s) {
    return !fast_nfft(s->n_fft) && bluestein_m(s->n_fft) > 0 && s->win_length <= s->n_fft;
}

/* ---- size-generic FFT engine (kpr_generic_kernels.h): plan + launch helpers --------------------------- */
// run-time radices of n: 4s first, then 2, then the odd primes; false when a prime factor exceeds 64 (a pass costs
// R multiply-adds per point: beyond that the DFT-as-GEMM path is the better fallback) or n is out of range
static bool gen_plan(int n, GenPlan* p) {
    if (n < 2) return false;
    p->n = n;
    p->npass = 0;
    int m = n;
    auto push = [&](int r) { if (p->npass < kGenMaxPasses) p->radix[p->npass] = r; ++p->npass; };
    while (m % 4 == 0) { push(4); m /= 4; }
    if (m % 2 == 0) { push(2); m /= 2; }
    for (int f = 3; f <= 64 && m > 1; f += 2)
        while (m % f == 0) { push(f); m /= f; }
    return m == 1 && p->npass <= kGenMaxPasses;
}

// the FFT length a frame is transformed with: n_fft / 2 for even sizes (real-FFT packing), n_fft for odd ones
static int gen_fft_len(int n_fft) { return (n_fft % 2 == 0 && n_fft >= 4) ? n_fft / 2 : n_fft; }

// LDS of one workgroup: two frame buffers of the FFT length, plus the n_fft-entry twiddle table when it fits as well
static bool gen_lds(size_t elem_bytes, int n_fft, size_t* lds, int* tw_lds) {
    const size_t buf = elem_bytes * (size_t)gen_fft_len(n_fft), tab = elem_bytes * (size_t)n_fft;
    if (2 * buf > 160 * 1024) return false;
    *tw_lds = 2 * buf + tab <= 160 * 1024;
    *lds = 2 * buf + (*tw_lds ? tab : 0);
    return true;
}

// plan and LDS of the generic engine for one transform size; tw_lds: the twiddle table fits in LDS as well (the kernel instance)
struct GenLaunch { GenPlan p; size_t lds; int tw_lds; };

// elem_bytes: sizeof(float2) or sizeof(double2).  false: no plan.  float64 has no other family to fall back to: an n_fft with a
// prime factor above 64 gets ONE pass of radix n_fft (a direct DFT), and only the LDS limits it.
static bool gen_fits(size_t elem_bytes, int n_fft, GenLaunch* l) {
    const int m = gen_fft_len(n_fft);
    if (!gen_plan(m, &l->p)) {
        if (elem_bytes != sizeof(double2)) return false;
        l->p.n = m; l->p.npass = 1; l->p.radix[0] = m;
    }
    return gen_lds(elem_bytes, n_fft, &l->lds, &l->tw_lds);
}

static bool gen_ok_f32(const kpr_stft_geom* s) {
    GenLaunch l;
    return s->win_length <= s->n_fft && gen_fits(sizeof(float2), s->n_fft, &l);
}

// the same for a launcher: no plan is an error
static int gen_launch_plan(size_t elem_bytes, int n_fft, GenLaunch* l) {
    if (gen_fits(elem_bytes, n_fft, l)) return 0;
    if (elem_bytes == sizeof(double2))
        return fail(KPR_E_UNSUPPORTED, "float64 path: n_fft = %d does not fit in LDS (limit 10240 even / 5120 odd)", n_fft);
    return fail(KPR_E_UNSUPPORTED, "no generic FFT plan for n_fft %d", n_fft);
}

static int gen_grid(const Geom& g, size_t lds) {
    const long long per_cu = std::max<long long>(1, std::min<long long>(8, (160 * 1024) / std::max<size_t>(lds, 1)));
    return (int)std::max<long long>(1, std::min<long long>(g.total_frames, 256 * per_cu));
}

// one workgroup per frame of g, up to gen_grid: kern = the k_stft_gen / k_irfft_gen instance of l.tw_lds, opt_in its LDS opt-in
template <class Kern, class... Args>
static int launch_gen(Kern kern, LdsOptIn& opt_in, const GenLaunch& l, const Geom& g, hipStream_t st, const char* label,
                      Args... args) {
    if (int e = allow_big_lds(opt_in, reinterpret_cast<const void*>(kern))) return e;
    hipLaunchKernelGGL(kern, dim3(gen_grid(g, l.lds)), dim3(kF64Threads), l.lds, st, args...);
    return launch_check(label);
}

// the FFT family of a transform size, in dispatch order (forward transforms: the cropped geometry of forward_geom)
static int fft_family(const kpr_stft_geom* s) {
    if (fast_nfft(s->n_fft)) return FAM_POW2;
    // even n_fft that is not a power of two: sizes with a mixed-radix plan take one N-point FFT per frame instead of two chirp-z FFTs
    if (bluestein_ok(s)) return mixed_radix_plan(s->n_fft) && opt(OPT_MIXED_RADIX) ? FAM_MR : FAM_BS;
    if (big_nfft(s->n_fft)) return FAM_BIG;
    // every other size with small prime factors (odd sizes, 1200, 1536, 2000 ...): run-time mixed-radix FFT
    if (gen_ok_f32(s)) return FAM_GEN;
    return FAM_GEMM;
}

// kpr_fft_plan: the dispatch's own answer (fft_family) for the cropped geometry of a forward transform
static int fft_plan(int n_fft, int win_length) {
    if (n_fft < 2 || win_length < 1) return -1;
    kpr_stft_geom s{};
    s.batch = 1; s.channels = 1; s.time = n_fft; s.n_fft = n_fft; s.win_length = std::min(win_length, n_fft); s.hop_length = 1;
    // The one input on which this function has never agreed with the dispatch: n_fft 4096 / 8192 with win_length > n_fft.  The
    // forward transform crops such frames and runs k_stft_big; this function has answered as if the sub-FFT family refused them,
    // and callers may have recorded that answer, so it stays.
    if (big_nfft(n_fft) && win_length > n_fft) return gen_ok_f32(&s) ? KPR_FFT_GENERIC : KPR_FFT_DFT_GEMM;
    switch (fft_family(&s)) {
        case FAM_POW2: return KPR_FFT_POW2;
        case FAM_MR:   return mixed_radix_plan(n_fft) == 1 ? KPR_FFT_MIXED_RADIX : KPR_FFT_TWO_PASS;
        case FAM_BS:   return KPR_FFT_BLUESTEIN;
        case FAM_BIG:  return KPR_FFT_SUB_FFT;
        case FAM_GEN:  return KPR_FFT_GENERIC;
        default:       return KPR_FFT_DFT_GEMM;
    }
}

}  // namespace kpr
