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
//   kpr_resample_direct_kernels.h the same conversion without a table: taps computed per output from an exact integer position,
//                             any pair of rates (backend.resample(method='direct'), signal.PitchShift)
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
//   kpr_mix_kernels.h         a circularly tiled noise signal mixed into a waveform at a per-item signal-to-noise ratio
//                             (augmentation.AddNoise) and its input gradient: float64 energy / dot-product sums along time without
//                             atomics, then out = a + s b; streamed (two launches, a workspace of chunk sums) or resident in the
//                             registers of one workgroup per item (one launch)
// The host code (table caches, launch plans, routes, argument validation, the bodies of the entry points) follows the kernels: kpr_host.h
// (shared by every family), then kpr_host_fft.h, kpr_host_stft.h, kpr_host_istft.h, kpr_host_mel.h, kpr_host_ops.h, kpr_host_griffin_lim.h,
// kpr_host_lfilter.h, kpr_host_convolve.h, kpr_host_mix.h next to their kernel headers.  No header calls an entry point.
// This file: the C ABI and nothing else -- the extern "C" entry points, grouped as in include/kapre_hip.h.  Each is at most api_enter(),
// the unpacking its C signature needs, and one call into namespace kpr; only the kpr_debug_* functions launch anything here.
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
#include "kpr_resample_direct_kernels.h"
#include "kpr_griffin_lim_kernels.h"
#include "kpr_time_stretch_kernels.h"
#include "kpr_hpss_kernels.h"
#include "kpr_lfilter_kernels.h"
#include "kpr_spec_fir_kernels.h"
#include "kpr_mix_kernels.h"

#include "kpr_host.h"
#include "kpr_host_fft.h"
#include "kpr_host_stft.h"
#include "kpr_host_istft.h"
#include "kpr_host_mel.h"
#include "kpr_host_ops.h"
#include "kpr_host_griffin_lim.h"
#include "kpr_host_lfilter.h"
#include "kpr_host_convolve.h"
#include "kpr_host_mix.h"

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace kpr;

// Entry of every API call that launches hot kernels: the launch log restarts, and a status word raised by an EARLIER call's
// kernels fails this one (sticky until kpr_device_status reads it -- like a HIP sticky error, but recoverable).
// The rule: an entry point that enters does so as its first statement, here and nowhere below this file.  The host-only functions
// (sizes, plans, tables, options) never enter, and neither do the older gradient entry points -- kpr_abs_* / kpr_angle_*_bwd,
// kpr_spec_edge_scale_*, kpr_mag_to_db_bwd_*, kpr_frame_bwd_f32, kpr_energy_bwd_f32, kpr_delta_bwd_f32 -- whose launches join the
// log of the call before them (tests/test_grad_gate.py reads it so).  The newer backward calls (mu-law decode, freq-map, PCEN,
// CMVN) enter.
static int api_enter() {
    launch_log_begin();
    if (unsigned* hostp = g_status.host.load(std::memory_order_acquire)) {
        const unsigned bits = *static_cast<volatile unsigned*>(hostp);
        if (bits)
            return fail(KPR_E_DEVICE, "a kernel of an earlier call raised the device status word (%s): its results are wrong; "
                        "kpr_device_status() reads and clears the condition", status_text(bits));
    }
    return 0;
}

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
    static const int lo[OPT_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, hi[OPT_COUNT] = {8, 4, 1, 4096, 1, 3, 32, 1, 1, 1, 1, 2, 2};
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

int kpr_fft_plan(int n_fft, int win_length) { return fft_plan(n_fft, win_length); }
int64_t kpr_num_frames(const kpr_stft_geom* s) {
    if (check_geom(s)) return -1;
    return frames_of(s);
}
int64_t kpr_stft_workspace_bytes(const kpr_stft_geom* s, int mode) { return stft_workspace_bytes(s, mode); }
int kpr_stft_f32(const float* x, const kpr_stft_geom* s, const float* window, void* out, int mode, void* workspace,
                 int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_stft_f32(x, s, window, out, mode, workspace, workspace_bytes, stream);
}
int64_t kpr_mel_workspace_bytes(const kpr_stft_geom* s, int n_filt, const kpr_db_params* db) {
    (void)db;
    return mel_workspace_bytes(s, n_filt, false);
}
int64_t kpr_mel_workspace_bytes_unpacked(const kpr_stft_geom* s, int n_filt) { return mel_workspace_bytes(s, n_filt, true); }
int kpr_filterbank_forget(const float* fb_packed) { return filterbank_forget(fb_packed); }
int64_t kpr_filterbank_pack_floats(int n_freq, int n_filt, const int32_t* fb_kranges_host) {
    return filterbank_pack_floats(n_freq, n_filt, fb_kranges_host);
}
int kpr_filterbank_pack(const float* fb_host, int n_freq, int n_filt, const int32_t* fb_kranges_host, float* out_host) {
    return filterbank_pack(fb_host, n_freq, n_filt, fb_kranges_host, out_host);
}
int kpr_filterbank_kranges(const float* fb_host, int n_freq, int n_filt, int32_t* out_host) {
    return filterbank_kranges(fb_host, n_freq, n_filt, out_host);
}
int kpr_mel_f32(const float* x, const kpr_stft_geom* s, const float* window, const float* fb, const float* fb_packed, int n_filt,
                const int32_t* fb_kranges_host, const kpr_db_params* db, float* out, void* workspace, int64_t workspace_bytes,
                kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_mel_f32(x, s, window, fb, fb_packed, n_filt, fb_kranges_host, db, out, workspace, workspace_bytes, stream);
}
int kpr_abs_c64(const void* x, int64_t n, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_cplx_to_real<float>(x, n, 0, out, stream);
}
int kpr_angle_c64(const void* x, int64_t n, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_cplx_to_real<float>(x, n, 1, out, stream);
}
int kpr_apply_filterbank_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout, const float* fb,
                             int n_filt, const int32_t* fb_kranges_host, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_apply_filterbank_f32(x, batch, channels, frames, n_freq, layout, fb, n_filt, fb_kranges_host, out, stream);
}
int kpr_apply_filterbank_packed_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                                    const float* fb, const float* fb_packed, int n_filt, const int32_t* fb_kranges_host, float* out,
                                    kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_apply_filterbank_packed_f32(x, batch, channels, frames, n_freq, layout, fb, fb_packed, n_filt, fb_kranges_host, out, stream);
}
int64_t kpr_db_workspace_bytes(int64_t n_items) { return db_workspace_bytes(n_items); }
int kpr_mag_to_db_f32(const float* x, int64_t n_items, int64_t item_size, const kpr_db_params* db, float* out, void* workspace,
                      int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_mag_to_db_f32(x, n_items, item_size, db, out, workspace, workspace_bytes, stream);
}
int64_t kpr_istft_workspace_bytes(const kpr_stft_geom* s, int64_t n_frames) { return istft_workspace_bytes<float>(s, n_frames); }
int kpr_istft_f32(const void* spec, const kpr_stft_geom* s, int64_t n_frames, const float* synth_window, float* out, void* workspace,
                  int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_istft_f32(spec, s, n_frames, synth_window, out, workspace, workspace_bytes, stream);
}

/* ---- float64 / complex128 variants -------------------------------------------------------------- */
int kpr_stft_f64(const double* x, const kpr_stft_geom* s, const double* window, void* out, int mode, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_stft_f64(x, s, window, out, mode, stream);
}
int64_t kpr_istft_f64_workspace_bytes(const kpr_stft_geom* s, int64_t n_frames) { return istft_workspace_bytes<double>(s, n_frames); }
int kpr_istft_f64(const void* spec, const kpr_stft_geom* s, int64_t n_frames, const double* synth_window, double* out, void* workspace,
                  int64_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_istft_f64(spec, s, n_frames, synth_window, out, workspace, workspace_bytes, stream);
}
int kpr_abs_c128(const void* x, int64_t n, double* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_cplx_to_real<double>(x, n, 0, out, stream);
}
int kpr_angle_c128(const void* x, int64_t n, double* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_cplx_to_real<double>(x, n, 1, out, stream);
}
int kpr_apply_filterbank_f64(const double* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout, const double* fb,
                             int n_filt, double* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_apply_filterbank_f64(x, batch, channels, frames, n_freq, layout, fb, n_filt, out, stream);
}
int kpr_mag_to_db_f64(const double* x, int64_t n_items, int64_t item_size, double ref_value, double amin, double dynamic_range,
                      double* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_mag_to_db_f64(x, n_items, item_size, ref_value, amin, dynamic_range, out, stream);
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
int kpr_spec_edge_scale_c64(const void* in, int64_t n, int n_freq, int inner, int n_fft, float s_edge, float s_mid, void* out,
                            kpr_stream_t stream) {
    return run_edge_scale<float>(in, n, n_freq, inner, n_fft, s_edge, s_mid, out, stream);
}
int kpr_spec_edge_scale_c128(const void* in, int64_t n, int n_freq, int inner, int n_fft, double s_edge, double s_mid, void* out,
                             kpr_stream_t stream) {
    return run_edge_scale<double>(in, n, n_freq, inner, n_fft, s_edge, s_mid, out, stream);
}
int kpr_mag_to_db_bwd_f32(const float* x, const float* gy, int64_t n_items, int64_t item_size, const kpr_db_params* db, float* gx,
                          kpr_stream_t stream) {
    if (!db) return fail(KPR_E_BADARG, "db params are NULL");
    return run_db_bwd<float>(x, gy, n_items, item_size, db->ref_value, db->amin, db->dynamic_range, gx, stream);
}
int kpr_mag_to_db_bwd_f64(const double* x, const double* gy, int64_t n_items, int64_t item_size, double ref_value, double amin,
                          double dynamic_range, double* gx, kpr_stream_t stream) {
    return run_db_bwd<double>(x, gy, n_items, item_size, ref_value, amin, dynamic_range, gx, stream);
}

/* ---- Frame / Energy / Delta ------------------------------------------------------------------ */
int64_t kpr_frame_count(int64_t time, int frame_length, int hop_length, int pad_end) {
    return frame_count(time, frame_length, hop_length, pad_end);
}
int kpr_frame_f32(const float* x, int64_t batch, int channels, int64_t time, int layout, int frame_length, int hop_length, int pad_end,
                  float pad_value, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_frame_f32(x, batch, channels, time, layout, frame_length, hop_length, pad_end, pad_value, out, stream);
}
int kpr_energy_f32(const float* x, int64_t batch, int channels, int64_t time, int layout, int frame_length, int hop_length, int pad_end,
                   float pad_value, float scale, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_energy_f32(x, batch, channels, time, layout, frame_length, hop_length, pad_end, pad_value, scale, out, stream);
}
int kpr_delta_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout, int win_length, int pad_mode,
                  float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_delta_f32(x, batch, channels, frames, n_freq, layout, win_length, pad_mode, out, stream);
}

/* ---- Frame / Energy / Delta backward (kpr_grad_kernels.h) ---------------------------------- */
int kpr_frame_bwd_f32(const float* g, int64_t batch, int channels, int64_t time, int layout, int frame_length, int hop_length,
                      int pad_end, float* gx, kpr_stream_t stream) {
    return run_frame_bwd_f32(g, batch, channels, time, layout, frame_length, hop_length, pad_end, gx, stream);
}
int kpr_energy_bwd_f32(const float* x, const float* g, int64_t batch, int channels, int64_t time, int layout, int frame_length,
                       int hop_length, int pad_end, float scale, float* gx, kpr_stream_t stream) {
    return run_energy_bwd_f32(x, g, batch, channels, time, layout, frame_length, hop_length, pad_end, scale, gx, stream);
}
int kpr_delta_bwd_f32(const float* g, int64_t batch, int channels, int64_t frames, int n_freq, int layout, int win_length, int pad_mode,
                      float* gx, kpr_stream_t stream) {
    return run_delta_bwd_f32(g, batch, channels, frames, n_freq, layout, win_length, pad_mode, gx, stream);
}

/* ---- SpecAugment / ChannelSwap (kpr_augment_kernels.h) -------------------------------------- */
int kpr_spec_augment_draw(int32_t* table, int64_t n_items, int n_time_masks, int n_freq_masks, int n_time, int n_freq,
                          int time_mask_param, int freq_mask_param, void* state, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_spec_augment_draw(table, n_items, n_time_masks, n_freq_masks, n_time, n_freq, time_mask_param, freq_mask_param, state, stream);
}
int kpr_index_draw(int32_t* out, int64_t n_items, int n_choices, void* state, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_index_draw(out, n_items, n_choices, state, stream);
}
int kpr_spec_augment_apply_f32(const float* x, float* out, const int32_t* table, int64_t n_items, int n_time_masks, int n_freq_masks,
                               int n_time, int n_freq, float mask_value, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_spec_augment_apply(x, out, table, n_items, n_time_masks, n_freq_masks, n_time, n_freq, mask_value, stream);
}
int kpr_channel_gather(const void* x, void* out, int64_t outer, int n_ch, int64_t inner, int elem_bytes, const int32_t* perm,
                       kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_channel_gather(x, out, outer, n_ch, inner, elem_bytes, perm, stream);
}

/* ---- mu-law companding / ConcatenateFrequencyMap (kpr_companding_kernels.h) ------------------ */
int kpr_mu_law_encode_f32(const float* x, int64_t n, int quantization_channels, int32_t* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_mu_law<MU_ENCODE>(x, x, out, n, quantization_channels, "x / out", stream);
}
int kpr_mu_law_decode_i32(const int32_t* code, int64_t n, int quantization_channels, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_mu_law<MU_DECODE_I32>(code, code, out, n, quantization_channels, "code / out", stream);
}
int kpr_mu_law_decode_f32(const float* code, int64_t n, int quantization_channels, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_mu_law<MU_DECODE_F32>(code, code, out, n, quantization_channels, "code / out", stream);
}
int kpr_mu_law_decode_bwd_f32(const float* code, const float* g, int64_t n, int quantization_channels, float* gx, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_mu_law<MU_DECODE_BWD>(code, g, gx, n, quantization_channels, "code / g / gx", stream);
}
int kpr_freq_map_concat_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout, float* out,
                            kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_freq_map<false>(x, batch, channels, frames, n_freq, layout, out, stream);
}
int kpr_freq_map_concat_bwd_f32(const float* g, int64_t batch, int channels, int64_t frames, int n_freq, int layout, float* gx,
                                kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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
    if (int e = api_enter()) return e;
    return run_pcen(false, x, nullptr, nullptr, outer, frames, inner, band_div, n_bands, s, alpha, delta, r, eps, out, smooth_out,
                    stream);
}
int kpr_pcen_bwd_f32(const float* x, const float* smooth, const float* gy, int64_t outer, int64_t frames, int64_t inner, int band_div,
                     int n_bands, const float* s, const float* alpha, const float* delta, const float* r, float eps, float* gx,
                     kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_pcen(true, x, smooth, gy, outer, frames, inner, band_div, n_bands, s, alpha, delta, r, eps, gx, nullptr, stream);
}
size_t kpr_pcen_bwd_params_workspace_bytes(int64_t outer, int64_t frames, int64_t inner) {
    return pcen_params_workspace(outer, frames, inner);
}
int kpr_pcen_bwd_params_f32(const float* x, const float* smooth, const float* gy, int64_t outer, int64_t frames, int64_t inner,
                            int band_div, int n_bands, const float* s, const float* alpha, const float* delta, const float* r,
                            float eps, float* gx, float* gparams, void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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
    if (int e = api_enter()) return e;
    return run_cmvn(false, x, nullptr, nullptr, outer, frames, inner, norm_vars, eps, out, rstd_out, stream);
}
int kpr_cmvn_bwd_f32(const float* y, const float* rstd, const float* gy, int64_t outer, int64_t frames, int64_t inner, int norm_vars,
                     float* gx, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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
    return resample_table(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint, table_host, first_host);
}
int kpr_resample_plan(int n_phases, int n_taps, int step, int* outputs_per_tile) {
    if (!outputs_per_tile) return fail(KPR_E_BADARG, "outputs_per_tile must not be NULL");
    if (int e = resample_dims(n_phases, n_taps, step)) return e;
    *outputs_per_tile = resample_plan(n_phases, step, n_taps).nb * n_phases;
    return 0;
}
int kpr_resample_f32(const float* x, int64_t batch, int channels, int64_t in_len, int layout, const float* table_dev,
                     const int32_t* first_dev, int n_phases, int n_taps, int step, int64_t out_len, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_resample(x, batch, channels, in_len, layout, table_dev, first_dev, n_phases, n_taps, step, out_len, out, stream);
}

/* ---- Resample without a table (kpr_resample_direct_kernels.h) ------------------------------------ */
int kpr_resample_direct_plan(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint, int* n_taps,
                             int* outputs_per_tile) {
    ResampleDirectShape r;
    if (!n_taps || !outputs_per_tile) return fail(KPR_E_BADARG, "n_taps / outputs_per_tile must not be NULL");
    if (int e = resample_direct_shape(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint, &r)) return e;
    *n_taps = r.n_taps;
    *outputs_per_tile = r.threads * r.per_lane;
    return 0;
}
int kpr_resample_direct_f32(const float* x, int64_t batch, int channels, int64_t in_len, int layout, int orig_freq, int new_freq,
                            int lowpass_filter_width, double rolloff, int adjoint, int64_t out_len, float* out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_resample_direct(x, batch, channels, in_len, layout, orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint,
                               out_len, out, stream);
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
    if (int e = api_enter()) return e;
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
    if (int e = api_enter()) return e;
    return run_hpss<false>(x, batch, ch, frames, freq, layout, kh, kp, power, margin_h, margin_p, want_mask, out_h, out_p, out_ch, stream);
}
int kpr_hpss_c64(const void* x, int64_t batch, int ch, int64_t frames, int64_t freq, int layout, int kh, int kp, double power,
                 double margin_h, double margin_p, int want_mask, void* out_h, void* out_p, int out_ch, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
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
int kpr_lfilter_carry(const double coef[5], int64_t n, double M[4]) { return lfilter_carry(coef, n, M); }
int64_t kpr_lfilter_workspace_bytes(int64_t batch, int channels, int64_t len, int layout) {
    if (lfilter_dims(batch, channels, len, layout)) return -1;
    return (int64_t)lfilter_workspace(batch, channels, len);
}
int kpr_lfilter_f32(const float* x, int64_t batch, int channels, int64_t len, int layout, const double coef[5], int reverse, float* out,
                    void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_lfilter(x, batch, channels, len, layout, coef, reverse, out, workspace, workspace_bytes, stream);
}

/* ---- Convolve (kpr_spec_fir_kernels.h) ---------------------------------------------------------- */
int kpr_spec_fir_plan(int64_t frames_out, int64_t inner, int n_part, int* out) { return spec_fir_plan(frames_out, inner, n_part, out); }
int kpr_spec_fir_c64(const void* x, int64_t outer, int64_t frames_in, int64_t inner, int band_div, const void* h, int n_ir, int n_part,
                     const int32_t* idx, int64_t items, void* out, int64_t frames_out, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_spec_fir(x, outer, frames_in, inner, band_div, h, n_ir, n_part, idx, items, out, frames_out, stream);
}

/* ---- AddNoise (kpr_mix_kernels.h, k_noise_draw of kpr_augment_kernels.h) ---------------------- */
int kpr_noise_draw(int32_t* table, int64_t n_items, int n_noise, const int32_t* lengths, double snr_lo, double snr_hi, void* state,
                   kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_noise_draw(table, n_items, n_noise, lengths, snr_lo, snr_hi, state, stream);
}
int kpr_add_noise_plan(int64_t batch, int channels, int64_t time, int layout, int* out) {
    return mix_plan(batch, channels, time, layout, out);
}
int64_t kpr_add_noise_workspace_bytes(int64_t batch, int channels, int64_t time, int layout) {
    return mix_workspace_bytes(batch, channels, time, layout);
}
int kpr_add_noise_f32(const float* x, int64_t batch, int channels, int64_t time, int layout, const float* noise, int n_noise,
                      int64_t stride, const int32_t* lengths, const int32_t* table, float* out, double* stats, void* workspace,
                      size_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_add_noise(false, x, nullptr, batch, channels, time, layout, noise, n_noise, stride, lengths, table, nullptr, out, stats,
                         workspace, workspace_bytes, stream);
}
int kpr_add_noise_bwd_f32(const float* gy, const float* x, int64_t batch, int channels, int64_t time, int layout, const float* noise,
                          int n_noise, int64_t stride, const int32_t* lengths, const int32_t* table, const double* stats, float* gx,
                          double* stats_out, void* workspace, size_t workspace_bytes, kpr_stream_t stream) {
    if (int e = api_enter()) return e;
    return run_add_noise(true, gy, x, batch, channels, time, layout, noise, n_noise, stride, lengths, table, stats, gx, stats_out,
                         workspace, workspace_bytes, stream);
}

}  // extern "C"
