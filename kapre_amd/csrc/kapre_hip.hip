// kapre_hip.hip -- gfx950 kernels + C ABI (include/kapre_hip.h) for Kapre's time-frequency path.
//
// One translation unit; the kernels live in the headers included below, one per kernel family:
//   kpr_fft.h, kpr_fft_mr.h   FFT building blocks: packed-f32 complex arithmetic, in-register DFTs,
//                             LDS exchange policies, the power-of-two Stockham passes, the mixed-radix
//                             (2^a 5^b) passes, real-FFT pairing
//   kpr_common.h              errors, frame geometry, sample fetch, and the wave-protocol pieces every kernel family shares:
//                             ticket draw, bounded waits, window pairs into LDS
//   kpr_cols.h                the column groups of the time-tiled kernels (k_pcen, k_cmvn, k_time_stretch): ColGroup, ColVec
//   kpr_mel_kernels.h        k_mel_ws: waveform -> [frame + window + rFFT -> |X| -> (K x M)
//                             filterbank on fp32 MFMA -> optional 10 log10], the whole Sequential of
//                             composed.py:138-261 in one launch; FROM_MAG: stand-alone ApplyFilterbank
//   kpr_mel_ts_kernels.h      k_mel_ts: the same Sequential, tile-synchronous (16 equal waves, two barriers per round) --
//                             the default fused mel kernel since round 3
//   kpr_mel_pw_kernels.h      k_mel_pw: the same Sequential with every wave owning its frames end to end and the mel product
//                             as banded sums on the vector ALU (round 4; banks with <= 2 non-zeros per bin)
//   kpr_stft_kernels.h        k_stft / k_stft_big / k_stft_bs / k_stft_mr: frame + window + rFFT with complex /
//                             magnitude / phase epilogue (time_frequency.py:164-185 [+ :359 / :402])
//   kpr_istft_kernels.h       k_istft_ws / k_istft_ws_mr / k_istft_fused, k_irfft* + k_ola
//                             (time_frequency.py:304-317)
//   kpr_generic_kernels.h     k_stft_gen / k_irfft_gen (run-time mixed-radix FFT for every transform size without a tuned
//                             plan, float32 and float64) and the float64 layer chain (time_frequency.py:155)
//   kpr_signal_kernels.h      k_frame, k_energy, k_delta, k_thin_gemm (signal.py, time_frequency.py:563-644)
//   kpr_misc_kernels.h        Magnitude / Phase, k_db_* (backend.py:126-194: log pass with per-item max/min
//                             statistics, then the dynamic-range clamp), k_gemm (generic fp32-MFMA GEMM:
//                             dense filterbanks and the DFT-as-GEMM path for transform sizes no FFT
//                             kernel covers -- the idea of the reference's kapre/tflite_compatible_stft.py:14-75)
//   kpr_grad_kernels.h        backward passes of the elementwise layers (tf.abs / tf.math.angle on complex data, the
//                             decibel map, the bin scaling that turns the inverse-STFT launch into STFT^T and back)
//   kpr_augment_kernels.h     SpecAugment (device-drawn masks) and ChannelSwap (augmentation.py)
//   kpr_companding_kernels.h  mu-law encode / decode (signal.py:236-361) and ConcatenateFrequencyMap (time_frequency.py:647-744),
//                             forward and backward: output-driven streaming kernels
//   kpr_pcen_kernels.h        per-channel energy normalisation and its input gradient: a recurrence along time, tiled over
//                             the waves of a workgroup (chunk end values through LDS, one barrier per super-block)
//   kpr_cmvn_kernels.h        per-utterance mean / variance normalisation and its input gradient: a reduction along time in
//                             the same geometry (chunk statistics through LDS, merged pairwise in a fixed order), resident in
//                             registers up to 128 frames, two sweeps beyond
//   kpr_resample_kernels.h    rational sample-rate conversion (signal.Resample): a polyphase gather over a staged input span,
//                             forward and adjoint in one kernel
//   kpr_griffin_lim_kernels.h Griffin-Lim phase reconstruction: the initial spectrum (zero or Philox phase), the projection onto the
//                             given magnitude with the momentum term and the convergence sums, the per-item convergence figure
//   kpr_time_stretch_kernels.h phase-vocoder time stretching of a complex spectrogram: a running sum of 32-bit angle words along time
//                             in the same geometry (chunk sums through LDS, one barrier per super-block)
//   kpr_lfilter_kernels.h     one biquad IIR section along time on a waveform (signal.LFilter): lanes run along time, float64
//                             inside; carries across lanes, waves and steps through companion-matrix powers; a whole-signal
//                             and a segmented (three-launch) form; the reverse scan is the adjoint
//   kpr_spec_fir_kernels.h    a short complex FIR along the frame axis of every bin of a complex spectrogram with a per-item filter
//                             table: the middle launch of the partitioned FFT convolution (signal.Convolve, augmentation.Reverb);
//                             filter values in registers, no LDS, no barrier
// The host code (table caches, launch plans, routes, argument validation) follows the kernels: kpr_host.h (shared by every family),
// then kpr_host_fft.h, kpr_host_stft.h, kpr_host_istft.h, kpr_host_mel.h, kpr_host_ops.h, kpr_host_griffin_lim.h, kpr_host_lfilter.h, kpr_host_convolve.h next to their kernel headers.
// This file: the C ABI -- the extern "C" entry points, grouped as in include/kapre_hip.h.
//
// gfx950 only: wave64, v_mfma_f32_16x16x4_f32, 160 KiB LDS.  No CUDA/compat paths.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <type_traits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kapre_hip.h"
#include "kpr_fft.h"
#include "kpr_fft_mr.h"

#include "kpr_common.h"
#include "kpr_cols.h"
#include "kpr_mel_kernels.h"
#include "kpr_mel_ts_kernels.h"
#include "kpr_mel_pw_kernels.h"
#include "kpr_fb_pw_kernels.h"
#include "kpr_mel_mr_kernels.h"
#include "kpr_signal_kernels.h"
#include "kpr_stft_kernels.h"
#include "kpr_istft_kernels.h"
#include "kpr_istft_pw_kernels.h"
#include "kpr_generic_kernels.h"
#include "kpr_misc_kernels.h"
#include "kpr_grad_kernels.h"
#include "kpr_augment_kernels.h"
#include "kpr_companding_kernels.h"
#include "kpr_pcen_kernels.h"
#include "kpr_cmvn_kernels.h"
#include "kpr_resample_kernels.h"
#include "kpr_griffin_lim_kernels.h"
#include "kpr_time_stretch_kernels.h"
#include "kpr_hpss_kernels.h"
#include "kpr_lfilter_kernels.h"
#include "kpr_spec_fir_kernels.h"

#include "kpr_host.h"
#include "kpr_host_fft.h"
#include "kpr_host_stft.h"
#include "kpr_host_istft.h"
#include "kpr_host_mel.h"
#include "kpr_host_ops.h"
#include "kpr_host_griffin_lim.h"
#include "kpr_host_lfilter.h"
#include "kpr_host_convolve.h"

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace kpr;

extern "C" {

int kpr_version(void) { return KPR_VERSION; }

const char* kpr_last_error(void) { return g_err.c_str(); }

const char* kpr_last_launches(void) { return g_launches.c_str(); }

int kpr_device_status(unsigned* flags_out) {
    unsigned bits = 0;
    if (unsigned* hostp = g_status.host.load(std::memory_order_acquire)) bits = __atomic_exchange_n(hostp, 0u, __ATOMIC_ACQ_REL);
    if (flags_out) *flags_out = bits;
    if (bits & kStStalePlan) {                               // whatever was cached about packed blobs is re-read from the device
        std::lock_guard<std::mutex> lk(g_mu);
        g_pack_ok.clear();
    }
    if (bits) return fail(KPR_E_DEVICE, "kernels raised the device status word (%s)", status_text(bits));
    return 0;
}

// development / tests: a kernel whose wait can never end, with a limit of 64 polls -- the whole reporting chain without a protocol bug
__global__ void k_spin_selftest() {
    __shared__ int flag;
    if (threadIdx.x == 0) flag = 0;
    __syncthreads();
    spin_until_ge<2, 64>(&flag, 1, kStSelfTest);
}
int kpr_debug_spin_timeout(kpr_stream_t stream) {
    if (int e = status_word_ready()) return e;
    hipLaunchKernelGGL(k_spin_selftest, dim3(1), dim3(64), 0, (hipStream_t)stream);
    return launch_check("k_spin_selftest");
}

int kpr_set_option(const char* name, int value) {
    const int id = option_id(name);
    if (id < 0) return fail(KPR_E_BADARG, "unknown option '%s'", name ? name : "(null)");
    static const int lo[OPT_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, hi[OPT_COUNT] = {8, 4, 1, 4096, 1, 3, 32, 1, 1, 1, 1, 2};
    if (value < lo[id] || value > hi[id])
        return fail(KPR_E_BADARG, "option '%s': value %d outside [%d, %d]", name, value, lo[id], hi[id]);
    // kernels removed in round 5 (dominated on every shape of tools/sweep_dispatch.py): the 4-wave ring kernel k_mel_fused
    // (mel_variant 1) and the static-run STFT kernel k_stft2 (stft_variant 2)
    if ((id == OPT_MEL_VARIANT && value == 1) || (id == OPT_STFT_VARIANT && value == 2))
        return fail(KPR_E_BADARG, "option '%s': value %d names a kernel that was removed (KPR_VERSION >= 110)", name, value);
    g_opt[id].store(value, std::memory_order_relaxed);
    return 0;
}

int kpr_get_option(const char* name, int* value) {
    const int id = option_id(name);
    if (id < 0 || !value) return fail(KPR_E_BADARG, "unknown option '%s'", name ? name : "(null)");
    *value = opt(id);
    return 0;
}

/* diagnostics (declared in include/kapre_hip.h): device buffer of 12*32 + 1 int64: cycle stamps written by
 * the waves of one workgroup of k_mel_ws (the one whose index is stored in the last element; k_mel_fused
 * and k_stft: workgroup 0, 4*32 entries); NULL disables */
int kpr_debug_stamps(void* dev_buf) { g_debug_stamps = (long long*)dev_buf; return 0; }

/* development aid: known-traffic kernel for calibrating the FETCH_SIZE counter (reads n*8 bytes) */
int kpr_debug_calib_read8(const void* x, int64_t n_float2, float* out, kpr_stream_t stream) {
    hipLaunchKernelGGL(k_calib_read8, dim3(2048), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)x, (long long)n_float2, out);
    return launch_check("k_calib_read8");
}

/* development aid: shader clock (MHz) under a dense packed-f32 load: mean over the waves of 2 workgroups per CU running
 * ~100 us; out_mhz_host receives one float.  Blocking. */
int kpr_debug_sclk_mhz(float* out_mhz_host) {
    if (!out_mhz_host) return fail(KPR_E_BADARG, "out_mhz_host is NULL");
    int cus = 256;
    if (int e = device_cus(&cus)) return e;
    const int blocks = 2 * cus, n = blocks * 4;
    float* d = nullptr;
    KPR_HIP(hipMalloc(&d, n * sizeof(float)));
    hipLaunchKernelGGL(k_sclk, dim3(blocks), dim3(256), 0, 0, 600, d);          // warm-up (clock ramp)
    hipLaunchKernelGGL(k_sclk, dim3(blocks), dim3(256), 0, 0, 600, d);
    std::vector<float> h(n);
    hipError_t e1 = hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e1 != hipSuccess) return fail(KPR_E_HIP, "kpr_debug_sclk_mhz: %s", hipGetErrorString(e1));
    double s = 0;
    for (float v : h) s += v;
    *out_mhz_host = (float)(s / n);
    return 0;
}

int kpr_fft_fast_path(int n_fft) { return fast_nfft(n_fft) ? 1 : 0; }

// the dispatch's own answer (fft_family) for the cropped geometry of a forward transform
int kpr_fft_plan(int n_fft, int win_length) {
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

int64_t kpr_num_frames(const kpr_stft_geom* s) {
    if (check_geom(s)) return -1;
    return frames_of(s);
}

int64_t kpr_stft_workspace_bytes(const kpr_stft_geom* s, int mode) {
    if (check_geom(s)) return -1;
    const kpr_stft_geom se = forward_geom(s);
    // (no device query: the CU count only picks among kernels that need no workspace)
    return stft_route(&se, make_geom(&se, frames_of(s)), mode, 256).workspace;
}

int kpr_stft_f32(const float* x, const kpr_stft_geom* s, const float* window, void* out, int mode,
                 void* workspace, int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_stft_f32(x, s, window, out, mode, workspace, workspace_bytes, stream);
}

int64_t kpr_mel_workspace_bytes(const kpr_stft_geom* s, int n_filt, const kpr_db_params* db) {
    if (check_geom(s) || n_filt <= 0) return -1;
    (void)db;
    int64_t bytes = stats_region_bytes(s->batch);
    // two-kernel path (stages the complex spectrum): every n_fft without a fused kernel, and filterbanks with more
    // 16-filter tiles than the tile-synchronous kernel's schedule holds (banks without a band plan of more than 256 filters are
    // beyond k_mel_ts, and beyond k_mel_ws whenever a consumer's slice exceeds 64 chunks -- always at n_fft 512; ADVICE r05: such a
    // call used to fail with KPR_E_WORKSPACE once k_mel_fused, the catch-all of round 1, was gone).  A bank of at most 256
    // filters that neither kernel's schedule holds (dense matrices) still needs kpr_mel_workspace_bytes_unpacked(): the call then
    // fails with KPR_E_WORKSPACE and names that size; the Python layer retries with it.
    if (!fused_nfft(s->n_fft) || (n_filt + 15) / 16 > kTsMaxTiles)
        bytes += (int64_t)sizeof(float) * 2 * s->batch * s->channels * frames_of(s) *
                 (s->n_fft / 2 + 1);
    return bytes;
}

int kpr_filterbank_forget(const float* fb_packed) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!fb_packed) { g_pack_ok.clear(); return 0; }
    for (auto it = g_pack_ok.begin(); it != g_pack_ok.end();)
        it = (it->first.first == (const void*)fb_packed) ? g_pack_ok.erase(it) : std::next(it);
    return 0;
}

int64_t kpr_filterbank_pack_floats(int n_freq, int n_filt, const int32_t* fb_kranges_host) {
    if (n_freq <= 0 || n_filt <= 0) return -1;
    MelSched sch;
    if (build_sched(n_freq, n_filt, fb_kranges_host, &sch)) return -1;
    return (int64_t)packed_chunks(sch) * 512 + kPackHeaderFloats + pw_section_cap(n_freq);   // header | fp32 MFMA fragments | band plan
}

int kpr_filterbank_pack(const float* fb_host, int n_freq, int n_filt, const int32_t* fb_kranges_host,
                        float* out_host) {
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

int64_t kpr_mel_workspace_bytes_unpacked(const kpr_stft_geom* s, int n_filt) {
    if (check_geom(s) || n_filt <= 0) return -1;
    return stats_region_bytes(s->batch) +
           (int64_t)sizeof(float) * 2 * s->batch * s->channels * frames_of(s) * (s->n_fft / 2 + 1);
}

int kpr_mel_f32(const float* x, const kpr_stft_geom* s, const float* window, const float* fb,
                const float* fb_packed, int n_filt, const int32_t* fb_kranges_host,
                const kpr_db_params* db, float* out, void* workspace, int64_t workspace_bytes,
                kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    if (int e = check_geom(s)) return e;
    if (int e = check_db(db)) return e;
    if (n_filt <= 0) return fail(KPR_E_BADARG, "n_filt must be positive");
    const long long F = frames_of(s);
    const int64_t need = kpr_mel_workspace_bytes(s, n_filt, db);
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
        hipLaunchKernelGGL(k_stats_init, dim3(grid_1d(s->batch * slots, 256)), dim3(256), 0, st, stats,
                           (long long)s->batch * slots);
        if (int e = launch_check("k_stats_init")) return e;
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

int kpr_filterbank_kranges(const float* fb_host, int n_freq, int n_filt, int32_t* out_host) {
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

int kpr_abs_c64(const void* x, int64_t n, float* out, kpr_stream_t stream) { return run_cplx_to_real<float>(x, n, 0, out, stream); }
int kpr_angle_c64(const void* x, int64_t n, float* out, kpr_stream_t stream) { return run_cplx_to_real<float>(x, n, 1, out, stream); }

int kpr_apply_filterbank_f32(const float* x, int64_t batch, int channels, int64_t frames,
                             int n_freq, int layout, const float* fb, int n_filt,
                             const int32_t* fb_kranges_host, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

int kpr_apply_filterbank_packed_f32(const float* x, int64_t batch, int channels, int64_t frames,
                                    int n_freq, int layout, const float* fb, const float* fb_packed,
                                    int n_filt, const int32_t* fb_kranges_host, float* out,
                                    kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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
            return kpr_apply_filterbank_f32(x, batch, channels, frames, n_freq, layout, fb, n_filt, fb_kranges_host, out, stream);
    }
}

int64_t kpr_db_workspace_bytes(int64_t n_items) {
    if (n_items < 0) return -1;
    return 256 + (int64_t)sizeof(unsigned) * 2 * std::max<int64_t>(1, n_items);
}

int kpr_mag_to_db_f32(const float* x, int64_t n_items, int64_t item_size, const kpr_db_params* db,
                      float* out, void* workspace, int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    if (!db) return fail(KPR_E_BADARG, "db params are NULL");
    kpr_db_params p = *db;
    p.enabled = 1;
    if (int e = check_db(&p)) return e;
    if (n_items < 0 || item_size < 0) return fail(KPR_E_BADARG, "negative size");
    if (n_items == 0 || item_size == 0) return 0;
    if (!x || !out) return fail(KPR_E_BADARG, "x / out must not be NULL");
    if (!workspace || workspace_bytes < kpr_db_workspace_bytes(n_items))
        return fail(KPR_E_WORKSPACE, "db workspace: need %lld bytes",
                    (long long)kpr_db_workspace_bytes(n_items));
    hipStream_t st = (hipStream_t)stream;
    DbDev dbd = make_db(&p);
    unsigned* stats = reinterpret_cast<unsigned*>(workspace);
    hipLaunchKernelGGL(k_stats_init, dim3(grid_1d(n_items, 256)), dim3(256), 0, st, stats,
                       (long long)n_items);
    if (int e = launch_check("k_stats_init")) return e;
    int chunks = db_chunks(n_items, item_size);
    if (opt(OPT_DB_CHUNKS) > 0) chunks = opt(OPT_DB_CHUNKS);
    // (aligned bases: 16-byte accesses on the aligned middle of every chunk)
    with_vec<4>(((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0, [&](auto v) {
        hipLaunchKernelGGL(k_db_log<v>, dim3((unsigned)(n_items * chunks)), dim3(256), 0, st, x, (long long)item_size, chunks, dbd, stats, out);
    });
    if (int e = launch_check("k_db_log")) return e;
    return db_clamp(out, n_items, item_size, dbd.dyn, stats, st);
}

int64_t kpr_istft_workspace_bytes(const kpr_stft_geom* s, int64_t n_frames) {
    if (check_geom(s) || n_frames < 0) return -1;
    return 256 + (int64_t)sizeof(float) * s->batch * s->channels * n_frames * s->win_length;
}

int kpr_istft_f32(const void* spec, const kpr_stft_geom* s, int64_t n_frames,
                  const float* synth_window, float* out, void* workspace, int64_t workspace_bytes,
                  kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_istft_f32(spec, s, n_frames, synth_window, out, workspace, workspace_bytes, stream);
}

/* ---- float64 / complex128 variants -------------------------------------------------------------- */
int kpr_stft_f64(const double* x, const kpr_stft_geom* s, const double* window, void* out, int mode,
                 kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    if (int e = check_geom(s)) return e;
    if (mode < KPR_OUT_COMPLEX || mode > KPR_OUT_PHASE) return fail(KPR_E_BADARG, "bad mode %d", mode);
    const long long F = frames_of(s);
    Geom g = make_geom(s, F);
    if (g.total_frames == 0) return 0;
    if (!x || !window || !out) return fail(KPR_E_BADARG, "x / window / out must not be NULL");
    g.win = std::min(g.win, g.n_fft);                            // win_length > n_fft: cropped frames (see forward_geom)
    GenLaunch l;
    if (int e = gen_launch_plan(sizeof(double2), s->n_fft, &l)) return e;
    const double2* tw = nullptr;
    if (int e = get_twiddles64(s->n_fft, &tw)) return e;
    static LdsOptIn opt_in[2];
    return launch_gen(l.tw_lds ? &k_stft_gen<double, true> : &k_stft_gen<double, false>, opt_in[l.tw_lds ? 1 : 0], l, g,
                      (hipStream_t)stream, "k_stft_gen<double>", x, g, window, tw, l.p, mode, out);
}

int64_t kpr_istft_f64_workspace_bytes(const kpr_stft_geom* s, int64_t n_frames) {
    if (check_geom(s) || n_frames < 0) return -1;
    return 256 + (int64_t)sizeof(double) * s->batch * s->channels * n_frames * s->win_length;
}

int kpr_istft_f64(const void* spec, const kpr_stft_geom* s, int64_t n_frames, const double* synth_window,
                  double* out, void* workspace, int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    if (int e = check_geom(s)) return e;
    if (n_frames < 0) return fail(KPR_E_BADARG, "negative frame count");
    Geom g = make_geom(s, n_frames);
    g.pad_left = 0;
    if (g.total_frames == 0) return 0;
    if (!spec || !synth_window || !out) return fail(KPR_E_BADARG, "spec / window / out must not be NULL");
    const int64_t need = kpr_istft_f64_workspace_bytes(s, n_frames);
    if (!workspace || workspace_bytes < need)
        return fail(KPR_E_WORKSPACE, "istft (float64) workspace: need %lld bytes", (long long)need);
    GenLaunch l;
    if (int e = gen_launch_plan(sizeof(double2), s->n_fft, &l)) return e;
    const double2* tw = nullptr;
    if (int e = get_twiddles64(s->n_fft, &tw)) return e;
    hipStream_t st = (hipStream_t)stream;
    double* frames = reinterpret_cast<double*>(workspace);
    static LdsOptIn opt_in[2];
    if (int e = launch_gen(l.tw_lds ? &k_irfft_gen<double, true> : &k_irfft_gen<double, false>, opt_in[l.tw_lds ? 1 : 0], l, g, st,
                           "k_irfft_gen<double>", (const double2*)spec, g, synth_window, tw, l.p, frames))
        return e;
    return run_ola<double>(frames, s, n_frames, s->in_layout == KPR_CHANNELS_LAST && s->channels > 1, out, st);
}

int kpr_abs_c128(const void* x, int64_t n, double* out, kpr_stream_t stream) { return run_cplx_to_real<double>(x, n, 0, out, stream); }
int kpr_angle_c128(const void* x, int64_t n, double* out, kpr_stream_t stream) { return run_cplx_to_real<double>(x, n, 1, out, stream); }

int kpr_apply_filterbank_f64(const double* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                             const double* fb, int n_filt, double* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    if (int e = check_rows_args(batch, channels, frames, n_freq, n_filt, layout, "bad filterbank shape", "bad layout %d")) return e;
    const long long total = (long long)batch * channels * frames * n_filt;
    if (total == 0) return 0;
    if (!x || !fb || !out) return fail(KPR_E_BADARG, "x / fb / out must not be NULL");
    hipLaunchKernelGGL(k_filterbank_f64, dim3(grid_1d(total, 256)), dim3(256), 0, (hipStream_t)stream, x,
                       (long long)batch, channels, (long long)frames, n_freq,
                       (layout == KPR_CHANNELS_LAST && channels > 1) ? 1 : 0, fb, n_filt, out);
    return launch_check("k_filterbank_f64");
}

int kpr_mag_to_db_f64(const double* x, int64_t n_items, int64_t item_size, double ref_value, double amin,
                      double dynamic_range, double* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

/* ---- backward passes (kpr_grad_kernels.h) ---------------------------------------------------- */
int kpr_abs_c64_bwd(const void* x, const float* g, int64_t n, void* gx, kpr_stream_t stream) {
    return run_cplx_bwd<float>(x, g, n, 0, gx, stream);
}
int kpr_angle_c64_bwd(const void* x, const float* g, int64_t n, void* gx, kpr_stream_t stream) {
    return run_cplx_bwd<float>(x, g, n, 1, gx, stream);
}
int kpr_abs_c128_bwd(const void* x, const double* g, int64_t n, void* gx, kpr_stream_t stream) {
    return run_cplx_bwd<double>(x, g, n, 0, gx, stream);
}
int kpr_angle_c128_bwd(const void* x, const double* g, int64_t n, void* gx, kpr_stream_t stream) {
    return run_cplx_bwd<double>(x, g, n, 1, gx, stream);
}

int kpr_spec_edge_scale_c64(const void* in, int64_t n, int n_freq, int inner, int n_fft, float s_edge, float s_mid,
                            void* out, kpr_stream_t stream) {
    return run_edge_scale<float>(in, n, n_freq, inner, n_fft, s_edge, s_mid, out, stream);
}
int kpr_spec_edge_scale_c128(const void* in, int64_t n, int n_freq, int inner, int n_fft, double s_edge, double s_mid,
                             void* out, kpr_stream_t stream) {
    return run_edge_scale<double>(in, n, n_freq, inner, n_fft, s_edge, s_mid, out, stream);
}

int kpr_mag_to_db_bwd_f32(const float* x, const float* gy, int64_t n_items, int64_t item_size,
                          const kpr_db_params* db, float* gx, kpr_stream_t stream) {
    if (!db) return fail(KPR_E_BADARG, "db params are NULL");
    return run_db_bwd<float>(x, gy, n_items, item_size, db->ref_value, db->amin, db->dynamic_range, gx, stream);
}
int kpr_mag_to_db_bwd_f64(const double* x, const double* gy, int64_t n_items, int64_t item_size, double ref_value,
                          double amin, double dynamic_range, double* gx, kpr_stream_t stream) {
    return run_db_bwd<double>(x, gy, n_items, item_size, ref_value, amin, dynamic_range, gx, stream);
}

/* ---- Frame / Energy / Delta ------------------------------------------------------------------ */
int64_t kpr_frame_count(int64_t time, int frame_length, int hop_length, int pad_end) {
    if (time < 0 || frame_length <= 0 || hop_length <= 0) {
        fail(KPR_E_BADARG, "bad time/frame_length/hop_length (%lld, %d, %d)", (long long)time, frame_length,
             hop_length);
        return -1;
    }
    if (pad_end) return (time + hop_length - 1) / hop_length;
    return time < frame_length ? 0 : 1 + (time - frame_length) / hop_length;
}

int kpr_frame_f32(const float* x, int64_t batch, int channels, int64_t time, int layout,
                  int frame_length, int hop_length, int pad_end, float pad_value, float* out,
                  kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

int kpr_energy_f32(const float* x, int64_t batch, int channels, int64_t time, int layout,
                   int frame_length, int hop_length, int pad_end, float pad_value, float scale,
                   float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

int kpr_delta_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                  int win_length, int pad_mode, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

/* ---- Frame / Energy / Delta backward (kpr_grad_kernels.h) ---------------------------------- */
int kpr_frame_bwd_f32(const float* g, int64_t batch, int channels, int64_t time, int layout, int frame_length,
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

int kpr_energy_bwd_f32(const float* x, const float* g, int64_t batch, int channels, int64_t time, int layout,
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

int kpr_delta_bwd_f32(const float* g, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                      int win_length, int pad_mode, float* gx, kpr_stream_t stream) {
    DeltaArgs a;
    if (int e = delta_args(batch, channels, frames, n_freq, layout, win_length, pad_mode, &a)) return e;
    if (a.total == 0) return 0;
    if (!g || !gx || g == gx) return fail(KPR_E_BADARG, "g / gx must not be NULL or aliased");
    hipLaunchKernelGGL(k_delta_bwd, dim3(grid_1d(a.total, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, g, a.outer,
                       (long long)frames, a.inner, a.n, pad_mode, a.scale, gx);
    return launch_check("k_delta_bwd");
}

/* ---- SpecAugment / ChannelSwap (kpr_augment_kernels.h) -------------------------------------- */
int kpr_spec_augment_draw(int32_t* table, int64_t n_items, int n_time_masks, int n_freq_masks, int n_time, int n_freq,
                          int time_mask_param, int freq_mask_param, void* state, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

int kpr_index_draw(int32_t* out, int64_t n_items, int n_choices, void* state, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

int kpr_spec_augment_apply_f32(const float* x, float* out, const int32_t* table, int64_t n_items, int n_time_masks,
                               int n_freq_masks, int n_time, int n_freq, float mask_value, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

int kpr_channel_gather(const void* x, void* out, int64_t outer, int n_ch, int64_t inner, int elem_bytes, const int32_t* perm,
                       kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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

/* ---- mu-law companding / ConcatenateFrequencyMap (kpr_companding_kernels.h) ------------------ */
int kpr_mu_law_encode_f32(const float* x, int64_t n, int quantization_channels, int32_t* out, kpr_stream_t stream) {
    return run_mu_law<MU_ENCODE>(x, x, out, n, quantization_channels, "x / out", stream);
}
int kpr_mu_law_decode_i32(const int32_t* code, int64_t n, int quantization_channels, float* out, kpr_stream_t stream) {
    return run_mu_law<MU_DECODE_I32>(code, code, out, n, quantization_channels, "code / out", stream);
}
int kpr_mu_law_decode_f32(const float* code, int64_t n, int quantization_channels, float* out, kpr_stream_t stream) {
    return run_mu_law<MU_DECODE_F32>(code, code, out, n, quantization_channels, "code / out", stream);
}
int kpr_mu_law_decode_bwd_f32(const float* code, const float* g, int64_t n, int quantization_channels, float* gx,
                              kpr_stream_t stream) {
    return run_mu_law<MU_DECODE_BWD>(code, g, gx, n, quantization_channels, "code / g / gx", stream);
}

int kpr_freq_map_concat_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout, float* out,
                            kpr_stream_t stream) {
    return run_freq_map<false>(x, batch, channels, frames, n_freq, layout, out, stream);
}
int kpr_freq_map_concat_bwd_f32(const float* g, int64_t batch, int channels, int64_t frames, int n_freq, int layout, float* gx,
                                kpr_stream_t stream) {
    return run_freq_map<true>(g, batch, channels, frames, n_freq, layout, gx, stream);
}

/* ---- PCEN (kpr_pcen_kernels.h) ---------------------------------------------------------------- */
int kpr_pcen_plan(int64_t frames, int64_t inner, int* rows_per_wave, int* waves_per_group) {
    if (frames < 0 || inner < 0 || !rows_per_wave || !waves_per_group) return fail(KPR_E_BADARG, "bad frames/inner or NULL result");
    *rows_per_wave = kPcenRows;
    *waves_per_group = kPcenWaves;
    return 0;
}
int kpr_pcen_f32(const float* x, int64_t outer, int64_t frames, int64_t inner, int band_div, int n_bands, const float* s,
                 const float* alpha, const float* delta, const float* r, float eps, float* out, float* smooth_out,
                 kpr_stream_t stream) {
    return run_pcen(false, x, nullptr, nullptr, outer, frames, inner, band_div, n_bands, s, alpha, delta, r, eps, out, smooth_out,
                    stream);
}
int kpr_pcen_bwd_f32(const float* x, const float* smooth, const float* gy, int64_t outer, int64_t frames, int64_t inner,
                     int band_div, int n_bands, const float* s, const float* alpha, const float* delta, const float* r, float eps,
                     float* gx, kpr_stream_t stream) {
    return run_pcen(true, x, smooth, gy, outer, frames, inner, band_div, n_bands, s, alpha, delta, r, eps, gx, nullptr, stream);
}
size_t kpr_pcen_bwd_params_workspace_bytes(int64_t outer, int64_t frames, int64_t inner) {
    return pcen_params_workspace(outer, frames, inner);
}
int kpr_pcen_bwd_params_f32(const float* x, const float* smooth, const float* gy, int64_t outer, int64_t frames, int64_t inner,
                            int band_div, int n_bands, const float* s, const float* alpha, const float* delta, const float* r,
                            float eps, float* gx, float* gparams, void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    return run_pcen(true, x, smooth, gy, outer, frames, inner, band_div, n_bands, s, alpha, delta, r, eps, gx, nullptr, stream, true,
                    gparams, workspace, workspace_bytes);
}

/* ---- CMVN (kpr_cmvn_kernels.h) ---------------------------------------------------------------- */
int kpr_cmvn_plan(int64_t frames, int64_t inner, int* rows_per_wave, int* waves_per_group, int* resident_frames) {
    if (frames < 0 || inner < 0 || !rows_per_wave || !waves_per_group || !resident_frames)
        return fail(KPR_E_BADARG, "bad frames/inner or NULL result");
    *rows_per_wave = kCmvnRows;
    *waves_per_group = kCmvnWaves;
    *resident_frames = kCmvnRows * kCmvnWaves;
    return 0;
}
int kpr_cmvn_f32(const float* x, int64_t outer, int64_t frames, int64_t inner, int norm_vars, float eps, float* out, float* rstd_out,
                 kpr_stream_t stream) {
    return run_cmvn(false, x, nullptr, nullptr, outer, frames, inner, norm_vars, eps, out, rstd_out, stream);
}
int kpr_cmvn_bwd_f32(const float* y, const float* rstd, const float* gy, int64_t outer, int64_t frames, int64_t inner, int norm_vars,
                     float* gx, kpr_stream_t stream) {
    return run_cmvn(true, y, rstd, gy, outer, frames, inner, norm_vars, 0.0f, gx, nullptr, stream);
}

/* ---- Resample (kpr_resample_kernels.h) ---------------------------------------------------------- */
int kpr_resample_table_size(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint, int* n_phases,
                            int* n_taps, int* step) {
    ResampleShape r;
    if (!n_phases || !n_taps || !step) return fail(KPR_E_BADARG, "n_phases / n_taps / step must not be NULL");
    if (int e = resample_size(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint, &r)) return e;
    *n_phases = r.P;
    *n_taps = r.n_taps;
    *step = r.Q;
    return 0;
}
int kpr_resample_table(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint, float* table_host,
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
int kpr_resample_plan(int n_phases, int n_taps, int step, int* outputs_per_tile) {
    if (!outputs_per_tile) return fail(KPR_E_BADARG, "outputs_per_tile must not be NULL");
    if (int e = resample_dims(n_phases, n_taps, step)) return e;
    *outputs_per_tile = resample_plan(n_phases, step, n_taps).nb * n_phases;
    return 0;
}
int kpr_resample_f32(const float* x, int64_t batch, int channels, int64_t in_len, int layout, const float* table_dev,
                     const int32_t* first_dev, int n_phases, int n_taps, int step, int64_t out_len, float* out, kpr_stream_t stream) {
    return run_resample(x, batch, channels, in_len, layout, table_dev, first_dev, n_phases, n_taps, step, out_len, out, stream);
}

/* ---- Griffin-Lim (kpr_griffin_lim_kernels.h) ---------------------------------------------------- */
int kpr_griffin_lim_plan(int64_t item_size, int* chunk_elems, int* chunks_per_item) {
    if (item_size < 0 || !chunk_elems || !chunks_per_item) return fail(KPR_E_BADARG, "bad item_size or NULL result");
    *chunk_elems = kGlChunk;
    if (item_size > 0x7fffffffLL) return fail(KPR_E_UNSUPPORTED, "item_size = %lld elements: 2^31 or more is not supported", (long long)item_size);
    *chunks_per_item = (int)gl_chunks(item_size);
    return 0;
}
int kpr_gl_project_f32(const void* R, const void* T, const float* mag, int64_t n_items, int64_t item_size, float c, void* S_out,
                       float* sc_out, void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_gl_project(R, T, mag, n_items, item_size, c, S_out, sc_out, workspace, workspace_bytes, (hipStream_t)stream);
}
int kpr_gl_init_f32(const float* M, int64_t batch, int channels, int64_t plane, int layout, double power, int init_mode,
                    void* rng_state, float* mag_out, void* S_out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_gl_init(M, batch, channels, plane, layout, power, init_mode, rng_state, mag_out, S_out, (hipStream_t)stream);
}
int64_t kpr_griffin_lim_workspace_bytes(const kpr_stft_geom* g, int64_t n_frames, int with_momentum, int with_power) {
    kpr_stft_geom fwd;
    GlLayout l;
    if (gl_layout(g, n_frames, with_momentum != 0, with_power != 0, &fwd, &l)) return -1;
    return (int64_t)l.total;
}
int kpr_griffin_lim_f32(const float* mag, const kpr_stft_geom* g, int64_t n_frames, const float* window, const float* synth_window,
                        int n_iter, double momentum, double power, int init_mode, const void* init, void* rng_state, float* wave_out,
                        float* sc_out, void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_griffin_lim(mag, g, n_frames, window, synth_window, n_iter, momentum, power, init_mode, init, rng_state, wave_out, sc_out,
                           workspace, workspace_bytes, stream);
}

/* ---- TimeStretch (kpr_time_stretch_kernels.h) -------------------------------------------------- */
int kpr_time_stretch_plan(int64_t frames_out, int64_t inner, int* rows_per_wave, int* waves_per_group) {
    if (frames_out < 0 || inner < 0 || !rows_per_wave || !waves_per_group) return fail(KPR_E_BADARG, "bad frames_out/inner or NULL result");
    *rows_per_wave = kPvRows;
    *waves_per_group = kPvWaves;
    return 0;
}
int kpr_time_stretch_c64(const void* x, int64_t outer, int64_t frames_in, int64_t frames_out, int64_t inner, const int32_t* idx,
                         const float* alpha, void* out, uint32_t* phase_out, kpr_stream_t stream) {
    return run_time_stretch(x, outer, frames_in, frames_out, inner, idx, alpha, out, phase_out, stream);
}

/* ---- HPSS (kpr_hpss_kernels.h) ------------------------------------------------------------------ */
int kpr_hpss_plan(int64_t frames, int64_t freq, int kh, int kp, int* tile_frames, int* tile_freq) {
    int hh, hp;
    if (frames < 0 || freq < 0 || !tile_frames || !tile_freq) return fail(KPR_E_BADARG, "bad frames/freq or NULL result");
    if (int e = hpss_half_windows(kh, kp, &hh, &hp)) return e;
    *tile_frames = kHpTile;
    *tile_freq = kHpTile;
    return 0;
}
int kpr_hpss_f32(const float* x, int64_t batch, int ch, int64_t frames, int64_t freq, int layout, int kh, int kp, double power,
                 double margin_h, double margin_p, int want_mask, float* out_h, float* out_p, int out_ch, kpr_stream_t stream) {
    return run_hpss<false>(x, batch, ch, frames, freq, layout, kh, kp, power, margin_h, margin_p, want_mask, out_h, out_p, out_ch, stream);
}
int kpr_hpss_c64(const void* x, int64_t batch, int ch, int64_t frames, int64_t freq, int layout, int kh, int kp, double power,
                 double margin_h, double margin_p, int want_mask, void* out_h, void* out_p, int out_ch, kpr_stream_t stream) {
    return run_hpss<true>(x, batch, ch, frames, freq, layout, kh, kp, power, margin_h, margin_p, want_mask, out_h, out_p, out_ch, stream);
}

/* ---- LFilter (kpr_lfilter_kernels.h) ------------------------------------------------------------ */
int kpr_lfilter_plan(int64_t batch, int channels, int64_t len, int layout, int* out) {
    if (!out) return fail(KPR_E_BADARG, "out is NULL");
    if (int e = lfilter_dims(batch, channels, len, layout)) return e;
    out[0] = kLfLane;
    out[1] = kLfWaveSamples;
    out[2] = kLfStep;
    out[3] = kLfSeg;
    out[4] = lfilter_form(batch, channels, len);
    return 0;
}
int kpr_lfilter_carry(const double coef[5], int64_t n, double M[4]) {
    if (!M) return fail(KPR_E_BADARG, "M is NULL");
    if (int e = lfilter_coef(coef)) return e;
    if (n < 0 || n > kLfCarryMax) return fail(KPR_E_BADARG, "chunk length %lld outside [0, 2^20]", (long long)n);
    std::vector<std::array<double, 4>> m;
    lfilter_carries(coef[3], coef[4], 0, {n}, &m);
    std::copy(m[0].begin(), m[0].end(), M);
    return 0;
}
int64_t kpr_lfilter_workspace_bytes(int64_t batch, int channels, int64_t len, int layout) {
    if (lfilter_dims(batch, channels, len, layout)) return -1;
    return (int64_t)lfilter_workspace(batch, channels, len);
}
int kpr_lfilter_f32(const float* x, int64_t batch, int channels, int64_t len, int layout, const double coef[5], int reverse, float* out,
                    void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    return run_lfilter(x, batch, channels, len, layout, coef, reverse, out, workspace, workspace_bytes, stream);
}

/* ---- Convolve (kpr_spec_fir_kernels.h) ---------------------------------------------------------- */
int kpr_spec_fir_plan(int64_t frames_out, int64_t inner, int n_part, int* out) { return spec_fir_plan(frames_out, inner, n_part, out); }
int kpr_spec_fir_c64(const void* x, int64_t outer, int64_t frames_in, int64_t inner, int band_div, const void* h, int n_ir, int n_part,
                     const int32_t* idx, int64_t items, void* out, int64_t frames_out, kpr_stream_t stream) {
    return run_spec_fir(x, outer, frames_in, inner, band_div, h, n_ir, n_part, idx, items, out, frames_out, stream);
}

}  // extern "C"
