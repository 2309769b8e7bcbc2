/*
 * kapre_hip.h -- C ABI of libkapre_hip.so: Kapre's time-frequency hot path as hand-written
 * gfx950 (MI355X / CDNA4) HIP kernels.
 *
 * This is the drop-in boundary.  The reference (keunwoochoi/kapre 0.4.0) has no FFI of its own:
 * each Keras layer's call() hands its tensors to TensorFlow ops.  Every entry point below
 * replaces the group of tf.* calls of ONE reference call() (file:line cited per function), so a
 * Kapre maintainer can bind it from the layer with a ctypes stub.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / HIP types in signatures
 *    (kpr_stream_t is the raw hipStream_t value, 0 = the default stream).
 *  - Every data pointer is a DEVICE pointer owned by the caller unless the name ends in _host.
 *    The library never allocates caller-visible memory; scratch comes from the caller
 *    (sizes from kpr_*_workspace_bytes).  The library keeps only immutable per-process caches
 *    (twiddle / DFT tables keyed by device and transform size).
 *  - Every call only ENQUEUES work on `stream` and never synchronises (first use of a new
 *    n_fft uploads a table with a blocking copy before enqueueing).
 *  - Return value: 0 = ok, negative = error (KPR_E_*); text via kpr_last_error() (thread local).
 *  - Data formats follow Kapre: waveforms are (batch, time, ch) "channels_last" or
 *    (batch, ch, time) "channels_first"; spectrograms are (batch, frame, freq, ch)
 *    "channels_last" or (batch, ch, frame, freq) "channels_first".
 *  - float32 / complex64 (interleaved re,im) is Kapre's floatx and the tuned path; the *_f64 / *_c128 entry
 *    points serve layers built with dtype='float64'.
 */
#ifndef KAPRE_HIP_H
#define KAPRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KPR_VERSION 120 /* 0.1.20 (round 6): stand-alone ApplyFilterbank on banks with a band plan = k_fb_pw (banded row sums; a row
                           * with a NaN / Inf bin returns the DENSE product's result); forward transforms with win_length > n_fft
                           * (cropped frames) on every FFT family, float64 included; option "fb_variant"; kpr_mel_workspace_bytes
                           * covers banks of more than 256 filters;
                           * 111 -> + kpr_device_status / KPR_E_DEVICE: a bounded wait that runs out inside a kernel is reported
                           * (round 5); 110 -> kernels k_mel_fused / k_stft2 removed: kpr_set_option("mel_variant", 1) and
                           * ("stft_variant", 2) are rejected (round 5);
                           * 101 -> + kpr_last_launches, banded mel plan in the packed filterbank (round 4);
                           * 100 -> backward entry points, kpr_filterbank_forget, kpr_debug_sclk_mhz (round 3) */

typedef void* kpr_stream_t;

enum { KPR_CHANNELS_FIRST = 0, KPR_CHANNELS_LAST = 1 };

/* what the STFT kernel writes */
enum {
    KPR_OUT_COMPLEX = 0,   /* complex64, STFT.call                      time_frequency.py:146-187 */
    KPR_OUT_MAGNITUDE = 1, /* float32 |X|, STFT.call + Magnitude.call   time_frequency.py:351-359 */
    KPR_OUT_PHASE = 2      /* float32 angle(X), STFT.call + Phase.call  time_frequency.py:394-402 */
};

enum {
    KPR_OK = 0,
    KPR_E_BADARG = -1,      /* invalid argument (null pointer, non-positive size, bad enum) */
    KPR_E_UNSUPPORTED = -2, /* configuration not implemented */
    KPR_E_HIP = -3,         /* a HIP runtime call failed */
    KPR_E_WORKSPACE = -4,   /* workspace missing or too small */
    KPR_E_DEVICE = -5       /* a kernel of an EARLIER call gave up one of its bounded waits (see kpr_device_status) */
};

/* decibel parameters of backend.magnitude_to_decibel (backend.py:126-194); enabled = 0 skips it */
typedef struct {
    int32_t enabled;
    float ref_value;
    float amin;
    float dynamic_range;
} kpr_db_params;

/* geometry of one STFT configuration (STFT.__init__, time_frequency.py:101-144) */
typedef struct {
    int64_t batch;
    int32_t channels;
    int64_t time;        /* samples per channel */
    int32_t n_fft;
    int32_t win_length;  /* frame_length of tf.signal.stft / inverse_stft.  Forward transforms with win_length > n_fft: frames are cut and
                          * counted with win_length, windowed, and cropped to their first n_fft samples (rfft semantics); the inverse
                          * zero-extends its n_fft-point frames to win_length (time_frequency.py:174-182, :307-314)              */
    int32_t hop_length;
    int32_t pad_begin;   /* left zero pad of n_fft - hop samples (time_frequency.py:169-172) */
    int32_t pad_end;     /* tf.signal.stft(pad_end=...)                                      */
    int32_t in_layout;   /* waveform layout  KPR_CHANNELS_*                                  */
    int32_t out_layout;  /* spectrogram layout KPR_CHANNELS_*                                */
} kpr_stft_geom;

int kpr_version(void);
const char* kpr_last_error(void);
/* Kernels the calling thread's most recent forward call (any kpr_*_f32 / _f64 / _c64 / _c128 entry point) launched, in order,
 * with the template arguments that pick the instance, e.g. "k_stats_init + k_mel_pw<1024,w16> + k_db_clamp",
 * "k_istft_pw_il<512,s4>", "k_stft<512,magnitude,cl>" (thread local; diagnostics: bench.py reports it as roofline.kernel so
 * that the label is what the dispatch actually chose, tests/test_fuzz_gate.py asserts which instance a launch size reached). */
const char* kpr_last_launches(void);

/* Device status.  The kernels whose waves hand work to each other through LDS flags (k_mel_ws, k_istft_ws[_mr], k_istft_pw) bound
 * every such wait (~0.2 s): a protocol error must not hang the GPU.  A wait that runs out leaves wrong values in that launch's
 * output AND raises a bit in a word of mapped host memory:
 *   - every later forward call of the process fails with KPR_E_DEVICE (checked on entry, no synchronisation: a volatile host
 *     read) until kpr_device_status() has read the word;
 *   - kpr_device_status(&flags) returns the bits raised so far and clears them: 0 / flags = 0 when healthy, KPR_E_DEVICE otherwise
 *     (bit 0 k_mel_ws, 1 k_istft_ws consumer, 2 k_istft_ws producer, 3 k_istft_pw, 4 stale band plan -- below --, 5 the output
 *     slot ring of k_mel_pw's PAIR form, 31 the self-test).  It does not synchronise: call it after the stream of the launches in question has been waited for.
 *     flags_out may be NULL.
 * Bit 4: k_mel_pw found that the packed filterbank at fb_packed no longer carries the band plan the library had cached for that
 * address (another blob was written there without kpr_filterbank_forget): that launch computed nothing; reading the status also
 * drops the cache, so the call can simply be repeated.
 * kpr_debug_spin_timeout launches a one-wave kernel whose wait cannot end (limit 64 polls): the reporting chain under test. */
int kpr_device_status(unsigned* flags_out);
int kpr_debug_spin_timeout(kpr_stream_t stream);

/* Process-wide tuning switches (thread safe; take effect for calls issued afterwards).  The library
 * never reads the process environment: what a call does depends on its arguments and these only.
 *   "mel_variant"  0 = automatic (default: the per-wave kernel k_mel_pw for n_fft 256 / 512 / 1024 / 2048 whenever the packed
 *                  filterbank carries a band plan -- mel and other triangular banks; for other matrices (log-frequency
 *                  banks, dense ones) the MFMA kernels: k_mel_ts at n_fft 256 / 512, for interleaved stereo and long runs at
 *                  n_fft 1024, k_mel_ws for the rest of n_fft 1024 / 2048; k_mel_mr for the 18 sizes with a mixed-radix /
 *                  two-pass plan: 96 ... 1000) | 2 = k_mel_ws with the filterbank streamed from L2 per tile (instead of
 *                  register-resident slices) | 3 = k_mel_ws wherever it applies, STFT + filterbank as two launches for
 *                  n_fft 256 and the mixed-radix sizes | 4 = the tile-synchronous kernel k_mel_ts wherever it applies |
 *                  5 / 6 / 7 = k_mel_pw with 8 / 4 / 16 waves per workgroup | 8 = its PAIR form (interleaved waveforms with
 *                  an even channel count at n_fft 1024 / 2048: two channel-frames per fetch; automatic for launches that
 *                  fill the chip) wherever it applies (A/B runs, tests).  1 (the round-1 ring kernel, removed) is rejected
 *   "stft_variant" 0 = automatic (default, channels_first complex / magnitude output and the interleaved-pair layouts:
 *                  k_stft3 -- sixteen-wave workgroups drawing frame groups from an LDS counter -- from 8 groups per CU up,
 *                  k_stft below) | 1 = k_stft | 3 = k_stft3 wherever it applies.  2 (k_stft2, removed) is rejected
 *   "istft_path"   0 = automatic (default: k_istft_pw -- overlap-add in registers, sixteen complete waves per CU -- for
 *                  n_fft 512 / 1024 / 2048 with hop = n_fft / 8, / 4 or / 2 and launches that fill the chip (channels_last with a
 *                  power-of-two channel count included, hop = n_fft / 4 or / 2); else the ring
 *                  kernel, the barrier kernel for launches of up to 3072 frames) | 1 = no wave-specialised ring kernel |
 *                  2 = irFFT + overlap-add as two kernels | 3 = the ring kernel whenever its preconditions hold |
 *                  4 = k_istft_pw whenever its preconditions hold.  Paths 1, 2, 3 produce bit-identical waveforms (same
 *                  frames, ascending order); k_istft_pw sums the R - 1 hop blocks at each boundary between two of its
 *                  frame runs as (earlier frames) + (later frames): deterministic, at most two roundings away (tests)
 *   "mixed_radix"  1 = mixed-radix FFTs for n_fft = 2^a 3^b 5^c plans (default) | 0 = Bluestein instead
 *   "db_chunks"    0 = automatic (default) | n = blocks per batch item of the decibel passes
 *   "db_slots"     0 = automatic (default) | n = statistics slots per batch item in the fused decibel kernels (rounded
 *                  down to a power of two, at most 32; 1 = the single slot of rounds 1-2): small batches spread the
 *                  workgroups' closing max / min atomics over several words per item (bit-identical results)
 *   "mel_cl_stage" 1 = (default) the PAIR form of k_mel_pw with a channels_last output of four or more channels collects the
 *                  n_filt x C block of every (item, frame) in LDS and writes it as one contiguous run | 0 = 8-byte (c, c + 1) stores
 *                  per filter (A/B runs, tests; bit-identical results)
 *   "fb_variant"   0 = automatic (default: stand-alone ApplyFilterbank with a band plan in the packed filterbank -- mel / triangular
 *                  banks, n_freq - 1 a multiple of four up to 1024 -- runs k_fb_pw, banded row sums, on contiguous rows and on rows of
 *                  two interleaved channels) | 1 = the MFMA kernels of rounds 2-5 for every bank (A/B runs, tests)
 *   "mel_pw_plain" 1 = (default) n_fft 2048 mel launches without decibels on contiguous input rows with a linear output (one
 *                  channel, or channels_first in and out) and a band plan of two rounds / one offset quad (the 128-filter mel bank
 *                  at 44.1 kHz) run k_mel_plain_pw, the plain-output instance of k_mel_pw | 0 = k_mel_pw for those too (A/B runs,
 *                  tests; bit-identical results)
 *   "cmvn_variant" 0 = automatic (default: kpr_cmvn_f32 / kpr_cmvn_bwd_f32 keep a series of up to resident_frames frames
 *                  (kpr_cmvn_plan) in registers -- one read, one write) | 1 = the streamed form, two sweeps, for every frame count
 *                  (A/B runs, tests; bit-identical results)
 *   "lfilter_variant" 0 = automatic (default: kpr_lfilter_f32 walks every series with one workgroup, or cuts the time axis into
 *                  segments when batch * channels is too small to fill the device) | 1 = whole-signal for every shape | 2 = segmented
 *                  for every shape (A/B runs, tests; results within the error bound of each other, not bit-identical)
 *   "addnoise_variant" 0 = automatic (default: in a batch of at least 256 items kpr_add_noise_f32 / kpr_add_noise_bwd_f32 keep an
 *                  item of at most kpr_add_noise_plan's resident limit in the registers of one workgroup, one launch, and stream
 *                  longer items and smaller batches in two) | 1 = streamed for
 *                  every shape | 2 = resident wherever it applies (A/B runs, tests; results within the error bound of each other,
 *                  not bit-identical)
 *   "verbose"      1 = print launch plans to stderr
 * Unknown name or out-of-range value: KPR_E_BADARG. */
int kpr_set_option(const char* name, int value);
int kpr_get_option(const char* name, int* value);

/* Diagnostics, not needed by a binder.  kpr_debug_stamps: device buffer of 12*32 + 1 int64 that the waves
 * of one workgroup fill with s_memtime stamps (NULL = off, the default); kpr_debug_calib_read8: a kernel
 * with exactly known HBM traffic (reads n_float2 * 8 bytes) for calibrating the rocprofv3 counters. */
int kpr_debug_stamps(void* dev_buf);
int kpr_debug_calib_read8(const void* x, int64_t n_float2, float* out, kpr_stream_t stream);
/* shader clock in MHz measured under a dense packed-f32 vector load (s_memtime ticks per 100 MHz s_memrealtime tick,
 * mean over all waves); blocking; bench.py prints it as sclk_mhz */
int kpr_debug_sclk_mhz(float* out_mhz_host);

/* 1 when n_fft (256, 512, 1024, 2048) runs directly on the LDS Stockham FFT kernels.  n_fft =
 * 2^a 5^b in {160, 200, 320, 400, 640, 800, 1000} and the sizes with a factor 3 in {96, 120, 192, 240,
 * 360, 384, 480, 600, 720, 768, 960} run mixed-radix FFTs, the other even sizes up to 1024 Bluestein's
 * algorithm on top of the Stockham FFT, 4096 and 8192 two / four 1024-point sub-FFTs per frame (forward),
 * the rest a DFT-as-GEMM path. */
int kpr_fft_fast_path(int n_fft);

/* Which forward / inverse FFT family a transform size runs (the float32 STFT / InverseSTFT entry points; fused mel kernels
 * exist for 256 ... 2048 and for the 18 mixed-radix / two-pass sizes).  <0 on bad args. */
enum {
    KPR_FFT_DFT_GEMM = 0,    /* a prime factor above 64: DFT as a GEMM, O(n_fft^2) per frame                     */
    KPR_FFT_POW2 = 1,        /* 256, 512, 1024, 2048: Stockham FFT, 16 points per lane                            */
    KPR_FFT_MIXED_RADIX = 2, /* 2^a 5^b: 160, 200, 320, 400, 640, 800, 1000                                       */
    KPR_FFT_TWO_PASS = 3,    /* sizes with a factor 3: 96, 120, 192, 240, 360, 384, 480, 600, 720, 768, 960       */
    KPR_FFT_BLUESTEIN = 4,   /* the other even sizes up to 1024: chirp-z on the Stockham FFT                      */
    KPR_FFT_SUB_FFT = 5,     /* 4096, 8192: two / four 1024-point sub-FFTs per frame                              */
    KPR_FFT_GENERIC = 6      /* everything else whose prime factors are <= 64: run-time mixed radix in LDS        */
};
/* (win_length > n_fft is classified as win_length = n_fft since KPR_VERSION 120: the forward transform crops its frames) */
int kpr_fft_plan(int n_fft, int win_length);

/* number of frames tf.signal.stft produces for this geometry (after the optional pad_begin);
 * mirrors the reference tests' helpers tests/test_time_frequency.py:32-39.  <0 on bad args. */
int64_t kpr_num_frames(const kpr_stft_geom* g);

/* ---------------------------------------------------------------------------------------------
 * STFT  (replaces tf.transpose + tf.pad + tf.signal.stft + tf.transpose, time_frequency.py:164-185;
 * with mode != KPR_OUT_COMPLEX also the tf.abs / tf.math.angle of the following layer).
 *   x       : float32 waveform in g->in_layout
 *   window  : float32[win_length] analysis window (backend.get_window_fn(name)(win_length)); win_length > n_fft: all win_length
 *             values are passed, the first n_fft are used
 *   out     : complex64 / float32 spectrogram in g->out_layout, n_frames x (n_fft/2+1) per channel
 *   workspace: size from kpr_stft_workspace_bytes (0 for every size the FFT kernels cover)
 */
int64_t kpr_stft_workspace_bytes(const kpr_stft_geom* g, int mode);
int kpr_stft_f32(const float* x, const kpr_stft_geom* g, const float* window, void* out, int mode,
                 void* workspace, int64_t workspace_bytes, kpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused melspectrogram: STFT -> Magnitude -> ApplyFilterbank [-> MagnitudeToDecibel]
 * (the Sequential built by composed.get_melspectrogram_layer, composed.py:138-261; also serves
 * get_log_frequency_spectrogram_layer, composed.py:264-385, with a log filterbank).
 *   fb      : float32 filterbank, row-major (n_freq = n_fft/2+1, n_filt) exactly as
 *             backend.filterbank_mel returns it (backend.py:231)
 *   fb_packed : DEVICE copy of the blob kpr_filterbank_pack builds on the host (same fb, same kranges),
 *             uploaded by the caller; the fused single-kernel path needs it.  The blob starts with a header
 *             naming the matrix it was packed from; on the first call with a given (pointer, n_freq, n_filt,
 *             kranges) the header is read back (one 32-byte copy on the call's stream, waited for -- not under stream
 *             capture) and a blob packed for another matrix shape or other kranges is refused with KPR_E_BADARG.
 *             NULL = two-kernel path (STFT, then |.| x fb GEMM), which needs the larger workspace
 *             kpr_mel_workspace_bytes_unpacked.
 *   fb_kranges_host : optional HOST int32[2*ceil(n_filt/16)] from kpr_filterbank_kranges
 *             (rows outside [lo,hi) of a 16-filter tile are exactly zero and are skipped);
 *             NULL = treat the matrix as dense
 *   out     : float32 (batch, frame, n_filt, ch) or (batch, ch, frame, n_filt)
 *   workspace: kpr_mel_workspace_bytes (dB item statistics; two-kernel path scratch for every n_fft without a fused
 *             kernel and for more than 1024 filters, where fb_packed is ignored); with fb_packed == NULL
 *             kpr_mel_workspace_bytes_unpacked
 *   errors  : malformed fb_kranges_host -> KPR_E_BADARG (only a filterbank too wide for the packed schedule falls
 *             back to the dense product silently)
 */
int64_t kpr_mel_workspace_bytes(const kpr_stft_geom* g, int n_filt, const kpr_db_params* db);
int64_t kpr_mel_workspace_bytes_unpacked(const kpr_stft_geom* g, int n_filt);
int kpr_mel_f32(const float* x, const kpr_stft_geom* g, const float* window, const float* fb,
                const float* fb_packed, int n_filt, const int32_t* fb_kranges_host,
                const kpr_db_params* db, float* out, void* workspace, int64_t workspace_bytes,
                kpr_stream_t stream);

/* Packed (MFMA-fragment order) copy of a filterbank for kpr_mel_f32: size in floats, and the
 * HOST-side packer.  Layout: 64 header words (uint32: 'KPFB' magic, n_freq, n_filt, tiles, chunks, hash of
 * the kranges, zeros), then for 16-filter tile t, chunk c (32 rows), half g, lane l,
 * s = 0..3:
 * out[64 + ((chunk0(t)+c)*2+g)*256 + l*4 + s] = fb[lo(t) + 32c + 16g + 4s + (l>>4)][16t + (l&15)]
 * (0 outside the matrix), lo(t) (rounded down to a multiple of 8) / chunk counts derived from fb_kranges_host
 * (NULL = dense).
 * At most 1024 filters and 32000 rows (KPR_E_UNSUPPORTED beyond: callers then pass fb_packed = NULL and the
 * product runs as a dense GEMM). */
int64_t kpr_filterbank_pack_floats(int n_freq, int n_filt, const int32_t* fb_kranges_host);
int kpr_filterbank_pack(const float* fb_host, int n_freq, int n_filt,
                        const int32_t* fb_kranges_host, float* out_host);

/* The header check of a packed blob is cached per (device address, matrix shape, kranges).  A caller that frees a blob
 * tells the library so: a different buffer that later lands on the same address is then read and checked again instead of
 * being taken for the old one.  fb_packed = NULL forgets every blob.  Host-side bookkeeping only, never fails. */
int kpr_filterbank_forget(const float* fb_packed);

/* Scan a HOST copy of a (n_freq, n_filt) filterbank and write, per tile of 16 filters, the
 * half-open row range [lo, hi) (lo rounded down, hi rounded up to multiples of 4) outside of
 * which every entry of the tile is exactly 0.0f.  out_host has 2*ceil(n_filt/16) entries. */
int kpr_filterbank_kranges(const float* fb_host, int n_freq, int n_filt, int32_t* out_host);

/* ---------------------------------------------------------------------------------------------
 * Stand-alone layers (used when the user composes layers by hand instead of the fused helper)
 */

/* Magnitude.call (tf.abs, time_frequency.py:359) / Phase.call (tf.math.angle, :402) on n complex */
int kpr_abs_c64(const void* x, int64_t n, float* out, kpr_stream_t stream);
int kpr_angle_c64(const void* x, int64_t n, float* out, kpr_stream_t stream);

/* ApplyFilterbank.call (tf.tensordot + tf.transpose, time_frequency.py:535-548).
 *   x  : float32 (batch, frame, n_freq, ch) [layout = LAST] or (batch, ch, frame, n_freq) [FIRST]
 *   out: same layout with n_freq replaced by n_filt */
int kpr_apply_filterbank_f32(const float* x, int64_t batch, int channels, int64_t frames,
                             int n_freq, int layout, const float* fb, int n_filt,
                             const int32_t* fb_kranges_host, float* out, kpr_stream_t stream);

/* Same operation, fast path: with fb_packed (kpr_filterbank_pack of the same fb / kranges, on the
 * DEVICE)
 *   - banks with a band plan (at most two non-zeros per bin, in neighbouring filters: mel / triangular banks, n_freq - 1 a
 *     multiple of four up to 1024) on contiguous rows (channels_first, or one channel) and on rows of two interleaved channels
 *     (channels_last stereo): k_fb_pw, banded row sums straight from global memory (round 6).  A row that contains a NaN / Inf bin returns what the reference's dense tensordot returns -- every filter NaN or
 *     +-Inf -- (the row is recomputed against fb, which therefore must be the matrix fb_packed was packed from);
 *   - other wide banded matrices (log-frequency banks, interleaved rows): the fused kernel's MFMA consumers fed by loader waves;
 *     a non-finite bin poisons the 16-filter tiles whose row range contains it, not the other filters of the row;
 *   - everything else falls through to kpr_apply_filterbank_f32 (dense: a non-finite bin poisons the whole row, unless
 *     fb_kranges_host lets the GEMM skip the tiles that do not contain it).
 * fb_packed may be NULL. */
int kpr_apply_filterbank_packed_f32(const float* x, int64_t batch, int channels, int64_t frames,
                                    int n_freq, int layout, const float* fb, const float* fb_packed,
                                    int n_filt, const int32_t* fb_kranges_host, float* out,
                                    kpr_stream_t stream);

/* MagnitudeToDecibel.call -> backend.magnitude_to_decibel (backend.py:126-194).
 * x is viewed as n_items rows of item_size elements (Kapre: item = one batch element, all other
 * axes flattened; a rank-1 input is ONE item).  In-place (out == x) is allowed.
 * workspace: kpr_db_workspace_bytes(n_items). */
int64_t kpr_db_workspace_bytes(int64_t n_items);
int kpr_mag_to_db_f32(const float* x, int64_t n_items, int64_t item_size, const kpr_db_params* db,
                      float* out, void* workspace, int64_t workspace_bytes, kpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * InverseSTFT.call (tf.transpose + tf.signal.inverse_stft + tf.transpose, time_frequency.py:304-317)
 *   spec         : complex64 spectrogram, g->out_layout, n_frames x (n_fft/2+1) per channel
 *   synth_window : float32[win_length] = tf.signal.inverse_stft_window_fn(hop, fwd)(win_length)
 *   out          : float32 waveform in g->in_layout, length (n_frames-1)*hop + win_length
 * g->time, pad_begin and pad_end are ignored; n_frames is given explicitly.
 */
int64_t kpr_istft_workspace_bytes(const kpr_stft_geom* g, int64_t n_frames);
int kpr_istft_f32(const void* spec, const kpr_stft_geom* g, int64_t n_frames,
                  const float* synth_window, float* out, void* workspace, int64_t workspace_bytes,
                  kpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * float64 / complex128 variants.  Kapre computes in the dtype of the Keras layer ("complex64 if x is float32,
 * complex128 if x is float64", time_frequency.py:155); a layer built with dtype='float64' runs these.  Same
 * arguments and layouts as the float32 entry points above with double / complex128 (interleaved re,im) data;
 * any n_fft whose frame fits in LDS (even n_fft <= 10240, odd <= 5120), any win_length.  Plain size-generic kernels: float64
 * is not the hot path.
 */
int kpr_stft_f64(const double* x, const kpr_stft_geom* g, const double* window, void* out, int mode,
                 kpr_stream_t stream);
int64_t kpr_istft_f64_workspace_bytes(const kpr_stft_geom* g, int64_t n_frames);
int kpr_istft_f64(const void* spec, const kpr_stft_geom* g, int64_t n_frames, const double* synth_window,
                  double* out, void* workspace, int64_t workspace_bytes, kpr_stream_t stream);
int kpr_abs_c128(const void* x, int64_t n, double* out, kpr_stream_t stream);
int kpr_angle_c128(const void* x, int64_t n, double* out, kpr_stream_t stream);
int kpr_apply_filterbank_f64(const double* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                             const double* fb, int n_filt, double* out, kpr_stream_t stream);
/* backend.magnitude_to_decibel (backend.py:126-194) in float64; in-place (out == x) is allowed */
int kpr_mag_to_db_f64(const double* x, int64_t n_items, int64_t item_size, double ref_value, double amin,
                      double dynamic_range, double* out, kpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Backward passes (vector-Jacobian products).  The reference's layers are TensorFlow graphs and therefore
 * differentiable: a Kapre front end sits inside model.fit / tf.GradientTape (time_frequency.py:146-187, :289-319,
 * :351-359, :402, :535-548; backend.py:186-192).  Complex cotangents follow TensorFlow's convention
 * (dL/dRe + i dL/dIm).  The LINEAR layers need no kernels of their own -- their adjoints are forward launches:
 *   STFT^T          (spectrogram cotangent G -> waveform cotangent):  kpr_spec_edge_scale_c64(G, s_edge = 1,
 *                   s_mid = 0.5), then kpr_istft_f32 with synth_window = n_fft * analysis window; sample t of the
 *                   waveform is sample t + pad_left of that output (zero where no frame reaches);
 *   InverseSTFT^T   (waveform cotangent -> spectrogram cotangent):  kpr_stft_f32 (no padding) with window =
 *                   2 / n_fft * synthesis window, then kpr_spec_edge_scale_c64(s_edge = 0.5, s_mid = 1) in place;
 *   ApplyFilterbank^T:  kpr_apply_filterbank_f32 with the transposed matrix (n_freq <-> n_filt).
 * kapre_amd/autograd.py composes exactly these calls.  The entry points below cover the non-linear layers.
 */

/* Magnitude (tf.abs on complex: g * x / |x|, 0 at x == 0) and Phase (tf.math.angle: g * (-im + i re) / |x|^2).
 * x, gx: n complex (interleaved re, im); g: n real */
int kpr_abs_c64_bwd(const void* x, const float* g, int64_t n, void* gx, kpr_stream_t stream);
int kpr_angle_c64_bwd(const void* x, const float* g, int64_t n, void* gx, kpr_stream_t stream);
int kpr_abs_c128_bwd(const void* x, const double* g, int64_t n, void* gx, kpr_stream_t stream);
int kpr_angle_c128_bwd(const void* x, const double* g, int64_t n, void* gx, kpr_stream_t stream);

/* out = in * (bin is DC, or Nyquist of an even n_fft ? s_edge : s_mid) on a complex spectrogram whose frequency axis
 * has n_freq = n_fft / 2 + 1 bins and `inner` elements per bin step (channels for channels_last data, 1 for
 * channels_first); n = complex element count.  In place (out == in) is allowed. */
int kpr_spec_edge_scale_c64(const void* in, int64_t n, int n_freq, int inner, int n_fft, float s_edge, float s_mid,
                            void* out, kpr_stream_t stream);
int kpr_spec_edge_scale_c128(const void* in, int64_t n, int n_freq, int inner, int n_fft, double s_edge, double s_mid,
                             void* out, kpr_stream_t stream);

/* backend.magnitude_to_decibel (backend.py:186-192) backward, from the layer's INPUT x and the output cotangent gy:
 * gx = 10 / (ln 10 * x) * [x >= amin] * (gy [l >= max_l - dynamic_range] + [l == max_l] / ties * sum of the gy
 * below the floor), l = the decibel value before the floor -- the floor moves with the item's maximum, as in
 * TensorFlow's gradient of tf.maximum(l, reduce_max(l) - dynamic_range).  Items as in kpr_mag_to_db_f32. */
int kpr_mag_to_db_bwd_f32(const float* x, const float* gy, int64_t n_items, int64_t item_size,
                          const kpr_db_params* db, float* gx, kpr_stream_t stream);
int kpr_mag_to_db_bwd_f64(const double* x, const double* gy, int64_t n_items, int64_t item_size, double ref_value,
                          double amin, double dynamic_range, double* gx, kpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Consumers / neighbours of the path (kapre/signal.py, time_frequency.py:563-644)
 */

/* frames tf.signal.frame produces: 1 + (time - frame_length) / hop (0 when time < frame_length),
 * ceil(time / hop) with pad_end.  <0 on bad args. */
int64_t kpr_frame_count(int64_t time, int frame_length, int hop_length, int pad_end);

/* Frame.call (tf.signal.frame, signal.py:86-104).
 *   x  : float32 (batch, time, ch) [layout = LAST] or (batch, ch, time) [FIRST]
 *   out: (batch, n_frames, frame_length, ch) [LAST] or (batch, ch, n_frames, frame_length) [FIRST];
 *        samples beyond the end of the signal (pad_end) are pad_value */
int kpr_frame_f32(const float* x, int64_t batch, int channels, int64_t time, int layout,
                  int frame_length, int hop_length, int pad_end, float pad_value, float* out,
                  kpr_stream_t stream);

/* Energy.call (signal.py:187-213): scale * sum over the frame of x^2, frames as above,
 * scale = ref_duration / (frame_length / sample_rate).
 *   out: (batch, n_frames, ch) [LAST] or (batch, ch, n_frames) [FIRST] */
int kpr_energy_f32(const float* x, int64_t batch, int channels, int64_t time, int layout,
                   int frame_length, int hop_length, int pad_end, float pad_value, float scale,
                   float* out, kpr_stream_t stream);

/* tf.pad modes Delta accepts (time_frequency.py:596-600) */
enum { KPR_PAD_CONSTANT = 0, KPR_PAD_SYMMETRIC = 1, KPR_PAD_REFLECT = 2 };

/* Delta.call (tf.pad + K.conv2d with the kernel [-n .. n] / (2 sum i^2), time_frequency.py:614-635).
 *   x, out: float32 (batch, time, freq, ch) [LAST] or (batch, ch, time, freq) [FIRST]
 *   win_length: odd, >= 3.  In-place (out == x) is NOT allowed. */
int kpr_delta_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                  int win_length, int pad_mode, float* out, kpr_stream_t stream);

/* Backward passes of the three layers above (cotangent of the output -> cotangent of the input; shapes and layouts
 * as in the forward entry points).  Gather form, deterministic.
 *   Frame^T : gx[t] = sum of g[f][t - f hop] over the frames that cover sample t (padding receives nothing)
 *   Energy^T: gx[t] = 2 scale x[t] * sum of g[f] over the frames that cover t
 *   Delta^T : the transposed correlation including the mirror images the padding mode folds back */
int kpr_frame_bwd_f32(const float* g, int64_t batch, int channels, int64_t time, int layout, int frame_length,
                      int hop_length, int pad_end, float* gx, kpr_stream_t stream);
int kpr_energy_bwd_f32(const float* x, const float* g, int64_t batch, int channels, int64_t time, int layout,
                       int frame_length, int hop_length, int pad_end, float scale, float* gx, kpr_stream_t stream);
int kpr_delta_bwd_f32(const float* g, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                      int win_length, int pad_mode, float* gx, kpr_stream_t stream);

/* ---- augmentation.py: SpecAugment and ChannelSwap (training-only layers) ---------------------------------------
 * SpecAugment.  x / out: float32, n_items blocks of n_time x n_freq (one channel, so (B, T, F, 1) and (B, 1, T, F)
 * are the same bytes).  table: device int32 [n_items][n_time_masks + n_freq_masks][2] = (first, last) INCLUSIVE
 * (augmentation.py:211-214), time masks first.  At most 32 masks per axis (KPR_E_BADARG beyond).
 *
 * kpr_spec_augment_draw fills `table` on the device and adds 1 to the call counter: no host-to-device copy per step,
 * and a captured graph draws a new table at every replay.
 *   state : 16 bytes of device memory OWNED BY THE CALLER: uint64 seed, uint64 calls.  The caller initialises both
 *           (calls usually 0) and must not touch them while a draw is in flight; two draws on one state must be
 *           ordered (same stream, or events).
 *   draws : Philox4x32-10, counter (item, mask, calls_lo, calls_hi), key (seed_lo, seed_hi) -> r0, r1;
 *           width = mulhi32(r0, param), first = mulhi32(r1, limit - width), last = first + width
 *           (param = the axis' mask parameter, limit = n_time / n_freq): 1 .. param elements inside the axis.
 *           An entry depends on (seed, calls, item, mask) only -- never on the launch geometry.
 *   errors: a mask parameter outside [1, axis length] on an axis that has masks -> KPR_E_BADARG.
 *           One workgroup draws the whole table: at most 2^20 entries (n_items x masks; KPR_E_UNSUPPORTED beyond).
 *
 * kpr_spec_augment_apply_f32: out = mask_value on the elements whose frame lies in a time interval or whose bin lies
 * in a frequency interval of the item, x elsewhere (bit for bit: NaN, Inf, -0 and denormals pass).
 *   out != x: a copy (x is not modified; x and out must not overlap partially).  out == x: the same kernel in place.
 *   n_freq <= 65536 (KPR_E_UNSUPPORTED beyond).
 *   Intervals are clamped to the axes; with mask_value = 0 the call is the layer's own adjoint. */
int kpr_spec_augment_draw(int32_t* table, int64_t n_items, int n_time_masks, int n_freq_masks, int n_time, int n_freq,
                          int time_mask_param, int freq_mask_param, void* state, kpr_stream_t stream);
int kpr_spec_augment_apply_f32(const float* x, float* out, const int32_t* table, int64_t n_items, int n_time_masks,
                               int n_freq_masks, int n_time, int n_freq, float mask_value, kpr_stream_t stream);

/* kpr_index_draw: out[item] = an index uniform in [0, n_choices), n_items device int32 (augmentation.Reverb: the impulse response
 * of every batch item).  The same 16-byte state, generator and rules as kpr_spec_augment_draw: Philox4x32-10, counter
 * (item, 0, calls_lo, calls_hi), key (seed_lo, seed_hi) -> r0; out[item] = mulhi32(r0, n_choices); calls advances by one (also for
 * n_items == 0).  n_choices < 1 or n_items < 0: KPR_E_BADARG; more than 2^20 items: KPR_E_UNSUPPORTED.  One launch, one workgroup,
 * no host reads: capturable. */
int kpr_index_draw(int32_t* out, int64_t n_items, int n_choices, void* state, kpr_stream_t stream);

/* ChannelSwap (tf.gather along the channel axis): x, out viewed as (outer, n_ch, inner) elements of elem_bytes = 4
 * (float32) or 8 (complex64); out[o][c][:] = x[o][perm_host[c]][:].  channels_first: outer = batch, inner = the rest;
 * channels_last: outer = everything in front of the channel axis, inner = 1.
 *   perm_host: n_ch HOST int32 in [0, n_ch) -- copied into the kernel arguments, so the call neither reads it later nor
 *              copies anything to the device.  At most 64 channels (KPR_E_UNSUPPORTED beyond).  In place is not allowed. */
int kpr_channel_gather(const void* x, void* out, int64_t outer, int n_ch, int64_t inner, int elem_bytes,
                       const int32_t* perm_host, kpr_stream_t stream);

/* ---- signal.py: MuLawEncoding / MuLawDecoding (backend.mu_law_encoding / mu_law_decoding, backend.py:302-341) ----
 * Elementwise over n elements of any shape; mu = quantization_channels - 1, quantization_channels in [2, 65536]
 * (KPR_E_BADARG outside).  Pointers are 4-byte aligned device pointers at ANY word (views are fine); out may be the
 * input itself (in place), partial overlap is KPR_E_BADARG.  n <= 2^40 (KPR_E_UNSUPPORTED beyond); n == 0 launches nothing.
 *   encode    : out = int32(trunc((sign(x) log1p(mu |x|) / log1p(mu) + 1) / 2 * mu + 0.5)).  Inputs outside [-1, 1] are
 *               NOT clipped (the formula as it stands, as TensorFlow); a NaN gives code 0 (TensorFlow leaves that cast
 *               unspecified).  Against the formula in float64: never more than one code away, and the same code wherever
 *               the value before truncation is at least quantization_channels * 2^-21 away from an integer.
 *   decode    : s = 2 code / mu - 1, out = sign(s) (exp(|s| log1p(mu)) - 1) / mu, from int32 codes (_i32) or from float32
 *               codes (_f32: what Keras' cast to floatx hands the layer, and the differentiable form).
 *   decode_bwd: gx = g * 2 log1p(mu) / mu^2 * exp(|s| log1p(mu)), the derivative of decode_f32 w.r.t. the code. */
int kpr_mu_law_encode_f32(const float* x, int64_t n, int quantization_channels, int32_t* out, kpr_stream_t stream);
int kpr_mu_law_decode_i32(const int32_t* code, int64_t n, int quantization_channels, float* out, kpr_stream_t stream);
int kpr_mu_law_decode_f32(const float* code, int64_t n, int quantization_channels, float* out, kpr_stream_t stream);
int kpr_mu_law_decode_bwd_f32(const float* code, const float* g, int64_t n, int quantization_channels, float* gx,
                              kpr_stream_t stream);

/* ---- time_frequency.py:647-744: ConcatenateFrequencyMap ---------------------------------------------------------
 * x: float32 (batch, frames, n_freq, channels) [LAST] or (batch, channels, frames, n_freq) [FIRST]; out: the same with
 * channels + 1.  The first `channels` channels are x bit for bit; the new last channel holds f / (n_freq - 1) for bin f
 * (tf.linspace(0, 1, n_freq)): exactly 0.0 at f = 0, exactly 1.0 at f = n_freq - 1, within 2^-24 elsewhere; n_freq == 1: 0.0.
 * One pass: every output byte is written once, every input byte read once.  4-byte aligned pointers at any word; x and out
 * must not overlap.  frames * n_freq * (channels + 1) < 2^31 per batch item (KPR_E_UNSUPPORTED beyond).
 * _bwd is the adjoint: gx = g without its last channel (g has channels + 1 channels, gx has `channels`). */
int kpr_freq_map_concat_f32(const float* x, int64_t batch, int channels, int64_t frames, int n_freq, int layout, float* out,
                            kpr_stream_t stream);
int kpr_freq_map_concat_bwd_f32(const float* g, int64_t batch, int channels, int64_t frames, int n_freq, int layout,
                                float* gx, kpr_stream_t stream);

/* ---- PCEN: per-channel energy normalisation (Wang et al. 2017), kapre_amd.time_frequency.PCEN ------------------------
 * x: a non-negative float32 spectrogram seen as a contiguous (outer, frames, inner) block scanned along `frames`; the band
 * of inner index i is i / band_div and inner == n_bands * band_div (KPR_E_BADARG otherwise):
 *   (batch, ch, frames, mel) [channels_first]: outer = batch * ch, inner = mel,      band_div = 1
 *   (batch, frames, mel, ch) [channels_last] : outer = batch,      inner = mel * ch, band_div = ch
 * s, alpha, delta, r: device float32 vectors of n_bands values (0 < s <= 1, alpha >= 0, delta > 0, r > 0: the caller checks
 * them, the library does not read them on the host); eps > 0.  Per (outer, inner) column, a = 1 - s:
 *   S[0] = x[0], S[t] = a S[t-1] + s x[t];  out[t] = (x[t] (eps + S[t])^-alpha + delta)^r - delta^r
 * x == 0 gives exactly 0.0.  A negative x is outside the contract (NaN where the base of a power goes negative).
 * smooth_out (may be NULL): receives S, which kpr_pcen_bwd_f32 takes as `smooth`.
 * _bwd: gx = d sum(gy * out) / dx (the parameters are constants; _bwd_params below is the form that differentiates them), one launch:
 *   G = (eps + S)^-alpha, u = x G + delta, p = gy r u^(r-1), q = -alpha p x G / (eps + S), N[t] = q[t] + a N[t+1], N[frames] = 0,
 *   gx[t] = p G + s N[t] for t >= 1, gx[0] = p G + N[0].
 * One pass: every input byte is read once, every output byte written once.  Pointers are 4-byte aligned; 16-byte accesses
 * are used when inner % 4 == 0 and every pointer is 16-byte aligned.  Outputs must not overlap inputs or each other (x == out
 * is KPR_E_BADARG).  frames * inner < 2^31 (KPR_E_UNSUPPORTED beyond).  outer, frames or inner == 0: returns 0, launches nothing.
 * kpr_pcen_plan (host only): the time tiling of the dispatch -- a workgroup of *waves_per_group waves covers
 * *waves_per_group * *rows_per_wave consecutive frames per step, *rows_per_wave per wave; chunk boundaries for tests.
 * _bwd_params: the backward pass of a PCEN whose parameters are learned.  gparams: (4, n_bands) float32, rows in the order of
 * the arguments (s, alpha, delta, r), the gradient of sum(gy * out) with respect to each band's parameter.  With the values of
 * _bwd and es = eps + S, the sums running over every (outer item, column of the band, frame):
 *   g_alpha[b] = sum -p x G ln(es)
 *   g_delta[b] = sum p - gy r delta^(r-1)                      (evaluated as gy r (u^(r-1) - delta^(r-1)))
 *   g_r[b]     = sum gy (u^r ln u - delta^r ln delta)          (u^r as u u^(r-1))
 *   g_s[b]     = sum over t >= 1 of N[t] (x[t] - S[t-1])       (frame 0 adds nothing: S[0] = x[0])
 *   x == 0 everywhere gives g_alpha = g_s = 0 exactly; frames == 1 gives g_s = 0 exactly.
 * gx: as _bwd writes it, bit for bit, or NULL: then no input gradient is computed or written (a frozen front end in front of a
 * learned PCEN).  gparams has the same bits either way, and the same inputs give the same bits on every call: no atomics; each
 * lane adds its frames in scan order, the waves of a workgroup are added in order, the workgroup leaves one float32 sum per
 * (parameter, column) in the workspace, and a second kernel adds the outer * band_div columns of each band in double, in an
 * order the shape fixes.  Two launches on `stream`, no host reads, capturable.
 * workspace: kpr_pcen_bwd_params_workspace_bytes = 16 * outer * inner bytes (0 for an empty shape), 4-byte aligned (16-byte
 * aligned for the 16-byte accesses); NULL or too small: KPR_E_WORKSPACE.  The argument rules of _bwd hold; gparams and the
 * workspace must not overlap anything else.  outer, frames or inner == 0: gparams is zeroed (one memset on `stream`). */
int kpr_pcen_plan(int64_t frames, int64_t inner, int* rows_per_wave, int* waves_per_group);
int kpr_pcen_f32(const float* x, int64_t outer, int64_t frames, int64_t inner, int band_div, int n_bands, const float* s,
                 const float* alpha, const float* delta, const float* r, float eps, float* out, float* smooth_out,
                 kpr_stream_t stream);
int kpr_pcen_bwd_f32(const float* x, const float* smooth, const float* gy, int64_t outer, int64_t frames, int64_t inner,
                     int band_div, int n_bands, const float* s, const float* alpha, const float* delta, const float* r, float eps,
                     float* gx, kpr_stream_t stream);
size_t kpr_pcen_bwd_params_workspace_bytes(int64_t outer, int64_t frames, int64_t inner);
int kpr_pcen_bwd_params_f32(const float* x, const float* smooth, const float* gy, int64_t outer, int64_t frames, int64_t inner,
                            int band_div, int n_bands, const float* s, const float* alpha, const float* delta, const float* r,
                            float eps, float* gx /* may be NULL */, float* gparams /* (4, n_bands) */, void* workspace,
                            size_t workspace_bytes, kpr_stream_t stream);

/* ---- CMVN: per-utterance mean / variance normalisation along time, kapre_amd.time_frequency.CMVN --------------------
 * x: a float32 block seen as contiguous (outer, frames, inner), normalised along `frames`; every (outer, inner) pair is a column
 * of its own (Kaldi's apply-cmvn --norm-vars per utterance, ESPnet's UtteranceMVN):
 *   (batch, ch, frames, mel) [channels_first]: outer = batch * ch, inner = mel
 *   (batch, frames, mel, ch) [channels_last] : outer = batch,      inner = mel * ch
 * Per column, n = frames:
 *   d[t] = x[t] - x[0];  m = (1/n) sum d[t];  c[t] = d[t] - m;  v = (1/n) sum c[t]^2 (population variance);  rstd = (v + eps)^-1/2
 *   out[t] = c[t] rstd (norm_vars = 1)   or   out[t] = c[t] (norm_vars = 0)
 * The shift by x[0] is part of the contract (decibel values sit far from 0: without it the sums lose five digits).  The sums
 * are taken per chunk of *rows_per_wave frames, two-pass (mean, then sum (d - mean)^2), and the chunks are merged in time order
 * with the pairwise update delta = mean_b - mean, mean += delta n_b / (n + n_b), M2 += M2_b + delta^2 n n_b / (n + n_b).
 * A constant column (frames == 1 included) gives +0.0 bit for bit for eps > 0.  A NaN or Inf anywhere in a column makes that
 * whole column non-finite and touches no other column.  The same inputs give the same bits on every call: no atomics; the order
 * of every sum is a function of the shape.
 * eps >= 0 and finite, norm_vars 0 or 1 (KPR_E_BADARG otherwise).
 * rstd_out (may be NULL): receives rstd per column, (outer, inner) values, which kpr_cmvn_bwd_f32 takes as `rstd`; with
 * norm_vars == 0 there is none: KPR_E_BADARG.
 * _bwd: gx = d sum(gy * out) / dx from the forward pass's OUTPUT y, one launch (the means run over the frames of a column):
 *   gx[t] = rstd (gy[t] - mean(gy) - y[t] mean(gy y))  (norm_vars = 1);   gx[t] = gy[t] - mean(gy)  (norm_vars = 0: y and rstd
 *   are not read and may be NULL).
 * Up to *resident_frames frames the series stays in registers (every input byte read once, every output byte written once);
 * beyond, or with option "cmvn_variant" = 1, the input is read twice -- same chunks, same order: the same bits.  Pointers are
 * 4-byte aligned; 16-byte accesses are used when inner % 4 == 0 and every pointer is 16-byte aligned.  Outputs must not overlap
 * inputs or each other (x == out is KPR_E_BADARG).  frames * inner < 2^31 (KPR_E_UNSUPPORTED beyond).  outer, frames or
 * inner == 0: returns 0, launches nothing.
 * kpr_cmvn_plan (host only): the time tiling of the dispatch, the same for every shape -- a workgroup of *waves_per_group waves
 * covers *waves_per_group * *rows_per_wave consecutive frames per step, *rows_per_wave per wave; *resident_frames is their
 * product; chunk boundaries for tests. */
int kpr_cmvn_plan(int64_t frames, int64_t inner, int* rows_per_wave, int* waves_per_group, int* resident_frames);
int kpr_cmvn_f32(const float* x, int64_t outer, int64_t frames, int64_t inner, int norm_vars, float eps,
                 float* out, float* rstd_out /* may be NULL; outer*inner values */, kpr_stream_t stream);
int kpr_cmvn_bwd_f32(const float* y, const float* rstd, const float* gy, int64_t outer, int64_t frames, int64_t inner,
                     int norm_vars, float* gx, kpr_stream_t stream);

/* ---- Resample: rational sample-rate conversion, kapre_amd.signal.Resample -------------------------------------------
 * Band-limited interpolation with a Hann-windowed sinc ("sinc_interp_hann").  With g = gcd(orig_freq, new_freq),
 * orig = orig_freq / g, new = new_freq / g, base = rolloff min(orig, new), L = lowpass_filter_width:
 *   h(tau) = (base / orig) sinc(base tau) cos^2(pi base tau / (2 L)) for |base tau| < L, else 0     (sinc(t) = sin(pi t) / (pi t))
 *   y[m]   = sum_n x[n] h(n / orig - m / new),  x[n] = 0 outside 0 <= n < T,  m = 0 .. ceil(new T / orig) - 1
 * and the adjoint gx[n] = sum_m gy[m] h(n / orig - m / new).  Both are one polyphase gather
 *   out[i] = sum_{k < n_taps} table[i mod n_phases][k] * in[(i div n_phases) * step + first[i mod n_phases] + k]
 * (reads outside 0 .. in_len - 1 give 0): forward (n_phases, step) = (new, orig), adjoint (orig, new), each with its own table.
 * kpr_resample_table_size / kpr_resample_table / kpr_resample_plan are host only and touch no device.
 *  _table_size: the shape of one direction's table (adjoint = 0 / 1).  n_taps is the largest support of a phase.  Supported:
 *               n_taps <= 128 and n_phases * n_taps * 4 <= 1 MiB, else KPR_E_UNSUPPORTED (the text names the table's size);
 *               rates <= 0, lowpass_filter_width < 1, rolloff outside (0, 1]: KPR_E_BADARG.
 *  _table:      table_host (n_phases, n_taps) float32 row-major and first_host (n_phases) int32.  Coefficients are computed in
 *               double and rounded once; a row is padded with 0.0 behind its support; first[] rises with the phase.
 *  _plan:       *outputs_per_tile = the consecutive outputs of one signal that a workgroup's staged input span serves (a whole
 *               number of n_phases): tile seams for tests.
 *  _f32:        x: float32 (batch, in_len, channels) [LAST] or (batch, channels, in_len) [FIRST]; out: the same with out_len
 *               (forward: ceil(new in_len / orig); adjoint: the forward's input length).  table_dev / first_dev: device copies of
 *               what _table wrote for (n_phases, n_taps, step).  One launch, forward or adjoint; the sum of an output runs over
 *               k in ascending order in float32 FMAs: the same inputs give the same bits (no atomics).  4-byte aligned pointers;
 *               x and out must not overlap; 2^30 elements or more per signal (per batch item for LAST): KPR_E_UNSUPPORTED.
 *               batch == 0 or out_len == 0: returns 0, launches nothing. */
int kpr_resample_table_size(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint, int* n_phases,
                            int* n_taps, int* step);
int kpr_resample_table(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint, float* table_host,
                       int32_t* first_host);
int kpr_resample_plan(int n_phases, int n_taps, int step, int* outputs_per_tile);
int kpr_resample_f32(const float* x, int64_t batch, int channels, int64_t in_len, int layout, const float* table_dev,
                     const int32_t* first_dev, int n_phases, int n_taps, int step, int64_t out_len, float* out, kpr_stream_t stream);

/* ---- Resample without a table: any pair of rates, backend.resample(method='direct'), kapre_amd.signal.PitchShift ------
 * The same h and the same outputs as the block above, with the taps computed on the device where they are used: no table, no
 * phase count, nothing cached or allocated.  With the rates reduced by their gcd, L = lowpass_filter_width:
 *   out[i] = s sum_j in[j] w(c (j P - i Q)),  in[j] = 0 outside 0 .. in_len - 1
 *   w(t)   = sinc(t) cos^2(pi t / (2 L)) for |t| < L, else 0;  c = rolloff / max(orig, new);  s = rolloff min(orig, new) / orig
 * forward (adjoint = 0): (P, Q) = (new, orig); adjoint (1): (orig, new).  The position i Q = a P + r of an output is exact 64-bit
 * integer arithmetic; only r / P becomes a float.  Every output sums a window of n_taps = 2 ceil(L max / (rolloff P)) inputs
 * from in[a - n_taps / 2 + 1] on, which holds its support and at most one input more at either end (tap exactly 0).
 * kpr_resample_direct_plan is host only and touches no device.
 *  _plan:  *n_taps as above, *outputs_per_tile = the consecutive outputs of one signal that a workgroup's staged input span
 *          serves: tile seams for tests.  Supported: n_taps <= 128, else KPR_E_UNSUPPORTED (the text names the tap count);
 *          rates <= 0, lowpass_filter_width < 1, rolloff outside (0, 1], adjoint outside 0 / 1: KPR_E_BADARG.
 *  _f32:   x: float32 (batch, in_len, channels) [LAST] or (batch, channels, in_len) [FIRST]; out: the same with out_len, a free
 *          argument >= 0 (forward: ceil(new in_len / orig) is the natural length; an index past it is the same sum: the filter's
 *          tail, then +0.0; adjoint: the forward's input length).  One launch.  A tap is a float32 function of (i, k, the rates)
 *          alone and the sum of an output runs over k in ascending order in float32 FMAs: the same inputs give the same bits,
 *          whatever the batch position, layout or channel count (no atomics).  4-byte aligned pointers; x and out must not
 *          overlap; 2^30 elements or more per signal (per batch item for LAST): KPR_E_UNSUPPORTED.
 *          batch == 0 or out_len == 0: returns 0, launches nothing. */
int kpr_resample_direct_plan(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint,
                             int* n_taps, int* outputs_per_tile);
int kpr_resample_direct_f32(const float* x, int64_t batch, int channels, int64_t in_len, int layout,
                            int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int adjoint,
                            int64_t out_len, float* out, kpr_stream_t stream);

/* ---- Griffin-Lim: magnitude spectrogram -> waveform, kapre_amd.time_frequency.GriffinLim ------------------------------
 * Phase reconstruction by alternating projections (Griffin & Lim 1984) with the momentum term of the fast variant (Perraudin,
 * Balazs & Sondergaard 2013), as librosa.griffinlim and torchaudio's GriffinLim run it, on this library's own transforms:
 * A = kpr_stft_f32 without padding, A+ = kpr_istft_f32 (untrimmed: (F - 1) hop + win samples, whose analysis has F frames again).
 * M: float32 (batch, frame, n_fft/2+1, ch) [LAST] or (batch, ch, frame, n_fft/2+1) [FIRST]; c = momentum / (1 + momentum):
 *   mag = M^(1/power)  (power == 1: M itself, bit for bit);   S_0 = mag e^{i phi};   T_0 = 0
 *   n = 1 .. n_iter:  R_n = A(A+(S_{n-1}));  sc_n = || |R_n| - mag || / || mag ||  per batch item;
 *                     a = R_n - c T_{n-1};   S_n = mag a / (|a| + 1e-16);   T_n = R_n
 *   y = A+(S_{n_iter})
 * momentum == 0 is the classical algorithm: T is neither read nor stored.  mag == 0 gives S == 0.  A NaN stays inside its batch
 * item, whose sc_n is NaN; an item with mag == 0 everywhere has sc_n = 0 / 0 = NaN too.  No float atomics: every sum has an order
 * fixed by the shape, the same inputs give the same bits.
 *
 * kpr_griffin_lim_plan (host only): the tiling of the step -- an item of item_size elements (complex bins) is cut into
 *   *chunks_per_item = ceil(item_size / *chunk_elems) equal parts, one workgroup each; seams for tests.
 * kpr_gl_project_f32: the step alone.  R, T, S_out: complex64, mag: float32, n_items x item_size elements each, contiguous; T may
 *   be NULL when c == 0 (it is then not read; c != 0 needs it); 0 <= c < 1.  S_out must not overlap an input.  sc_out (may be
 *   NULL): n_items float32, sc of R against mag; it needs the workspace: 8 bytes per item and chunk, 8-byte aligned
 *   (KPR_E_WORKSPACE).  R / T / S_out 8-byte, mag 4-byte aligned; 16-byte accesses when all four are 16-byte aligned.  One launch,
 *   two with sc_out.  item_size < 2^31.
 * kpr_gl_init_f32: mag and S_0 alone.  plane = frames * bins; M as above.  init_mode 0: phi = 0; 1: phi = 2 pi r 2^-32 with r
 *   word (e mod 4) of Philox4x32-10 under key seed and counter (e div 4, calls), e being the element's index in the FIRST order
 *   whatever the layout, and rng_state the 16-byte device state (uint64 seed, uint64 calls) of kpr_spec_augment_draw; a second
 *   launch then stores calls + 1.  mag_out: receives mag when power != 1, NULL when power == 1 (KPR_E_BADARG otherwise).
 *   S_out may be NULL (mag only; nothing is drawn).
 * kpr_griffin_lim_workspace_bytes: the scratch of kpr_griffin_lim_f32 for that geometry (-1: bad geometry).  It holds S, one
 *   buffer for R (two with momentum, alternating as R and T: T_n = R_n is a swap of pointers), mag when power != 1, the chunk sums
 *   and the scratch of the two transforms.
 * kpr_griffin_lim_f32: the whole run on `stream`: the init launch, per iteration the inverse transform, the forward transform,
 *   the step and the convergence figure, then one last inverse -- the dispatch and the bits of the transforms are those of
 *   kpr_istft_f32 / kpr_stft_f32 on the same tensors.  It never synchronises and copies nothing to the host.  g: batch, channels,
 *   n_fft, win_length, hop_length; in_layout = layout of the waveform, out_layout = layout of M; time is ignored, pad_begin and
 *   pad_end must be 0.  window / synth_window: win_length device floats, the forward window and its inverse_stft_window_fn
 *   companion.  n_iter == 0: y = A+(S_0).  init_mode 0 / 1 as above; 2: S_0 = init, complex64 in M's layout, used as it is.
 *   wave_out: (batch, (F-1) hop + win, ch) / (batch, ch, ...) float32; it also carries the waveform between the transforms.
 *   sc_out (may be NULL): n_iter x batch float32 on the device.  workspace 16-byte aligned.  KPR_E_BADARG: n_iter < 0, momentum
 *   outside [0, 1), power <= 0, bad init_mode or a missing init / rng_state, padding flags; a geometry that the transforms
 *   refuse gives their error.  batch == 0 or n_frames == 0: returns 0, launches nothing. */
int kpr_griffin_lim_plan(int64_t item_size, int* chunk_elems, int* chunks_per_item);
int kpr_gl_project_f32(const void* R, const void* T /* may be NULL */, const float* mag, int64_t n_items, int64_t item_size, float c,
                       void* S_out, float* sc_out /* may be NULL */, void* workspace, size_t workspace_bytes, kpr_stream_t stream);
int kpr_gl_init_f32(const float* M, int64_t batch, int channels, int64_t plane, int layout, double power, int init_mode,
                    void* rng_state, float* mag_out, void* S_out, kpr_stream_t stream);
int64_t kpr_griffin_lim_workspace_bytes(const kpr_stft_geom* g, int64_t n_frames, int with_momentum, int with_power);
int kpr_griffin_lim_f32(const float* mag, const kpr_stft_geom* g, int64_t n_frames, const float* window, const float* synth_window,
                        int n_iter, double momentum, double power, int init_mode, const void* init /* init_mode 2 */,
                        void* rng_state /* init_mode 1 */, float* wave_out, float* sc_out /* may be NULL; n_iter x batch */,
                        void* workspace, size_t workspace_bytes, kpr_stream_t stream);

/* ---- TimeStretch: phase-vocoder time stretching of a complex spectrogram, kapre_amd.time_frequency.TimeStretch ---------
 * x: complex64 (outer, frames_in, inner), contiguous -> out: (outer, frames_out, inner).  channels_first: outer = batch * ch,
 * inner = freq; channels_last: outer = batch, inner = freq * ch.  idx (int32) and alpha (float32): frames_out DEVICE entries, the
 * floor and the fraction of t * rate (the caller computes them in float64; the library never reads them on the host).  Output
 * frame t reads the rows i = idx[t] and i + 1; a row >= frames_in (the two padding frames; any index that is no row) reads as
 * zero, so idx[t] + 1 <= frames_in + 1 is the caller's contract and nothing outside x is touched whatever the table holds.
 *   Theta(x) = 2 rint(atan2f(im, re) c) as a uint32, 2^32 = one turn, c = float32(2^30 / pi); 0 for re == im == 0 (any signs),
 *              for a padding row and for a non-finite bin
 *   P[0] = Theta(X[0]);   P[t + 1] = P[t] + Theta(X[i + 1]) - Theta(X[i])      (uint32: the sum wraps by itself and is exact)
 *   m[t] = alpha[t] |X[i + 1]| + (1 - alpha[t]) |X[i]|,   |x| = sqrtf(re re + im im)
 *   out[t] = m[t] (cos, sin)(pi h),   h = (float)(int32)P[t] 2^-31
 * This is the phase vocoder of torchaudio.functional.phase_vocoder / librosa.phase_vocoder: the expected phase advance of a bin
 * enters the accumulated phase as a whole number of turns, so there is no hop length here.  With idx[t] = t and alpha = 0
 * P[t] = Theta(X[t]): the input comes back up to rounding.  A non-finite bin makes non-finite only the frames that read it; every
 * other frame is bit for bit what it would be with that bin set to 0.  The same inputs give the same bits: no atomics, and
 * integer addition does not care about the order.
 * phase_out (may be NULL): receives P, (outer, frames_out, inner) uint32.  x / out 8-byte, idx / alpha / phase_out 4-byte aligned;
 * 16-byte accesses when inner is even, x and out are 16-byte and phase_out is 8-byte aligned.  x == out or any overlap of an
 * output with an input: KPR_E_BADARG.  frames_in * inner or frames_out * inner >= 2^30: KPR_E_UNSUPPORTED.  outer, frames_out or
 * inner == 0: returns 0, launches nothing.  One launch, no host reads: capturable.
 * kpr_time_stretch_plan (host only): the time tiling of the dispatch, the same for every shape -- a workgroup of
 * *waves_per_group waves covers *waves_per_group * *rows_per_wave consecutive output frames per step, *rows_per_wave per wave;
 * chunk boundaries for tests. */
int kpr_time_stretch_plan(int64_t frames_out, int64_t inner, int* rows_per_wave, int* waves_per_group);
int kpr_time_stretch_c64(const void* x, int64_t outer, int64_t frames_in, int64_t frames_out, int64_t inner, const int32_t* idx,
                         const float* alpha, void* out, uint32_t* phase_out /* may be NULL: (outer, frames_out, inner) phase words */,
                         kpr_stream_t stream);

/* ---- HPSS: median-filter harmonic-percussive separation of a spectrogram, kapre_amd.time_frequency.HPSS --------------------
 * x: float32 (kpr_hpss_f32) or complex64 (kpr_hpss_c64) spectrogram, (batch, frames, freq, ch) [layout = LAST] or
 * (batch, ch, frames, freq) [FIRST], contiguous; every (batch item, channel) plane on its own.  kh, kp: odd, 3 ... 31.
 *   H[t, f] = median of S[r(t + d, frames), f], |d| <= (kh - 1) / 2        P[t, f] = median of S[t, r(f + d, freq)], |d| <= (kp - 1) / 2
 *   r(i, n): j = i mod 2n (non-negative); j < n ? j : 2n - 1 - j           (half-sample symmetric, defined for every n >= 1)
 *   S = x, or sqrtf(re re + im im) of a complex x.  The median is a selection: it equals one of the window's values bit for bit
 *   (the sign of a zero is unspecified), with NaN ordered above +Inf as in numpy.sort.
 *   soft(X, R): Z = max(X, R); bad = Z < 2^-126; a = X / Z, c = R / Z (Z := 1 where bad); m = a^power / (a^power + c^power);
 *               where bad: m = 0.5 if margin_h == margin_p == 1, else 0.   power = inf: m = X > R ? 1 : 0
 *   Mh = soft(H, P margin_h),  Mp = soft(P, H margin_p), in float32; power 1 and 2 without powf
 *   want_mask 0: out_h = x Mh, out_p = x Mp (complex64 for a complex x);  1: out_h = Mh, out_p = Mp (float32 for either x);
 *   2 (for tests): out_h = H, out_p = P (float32)
 * out_h / out_p: tensors in x's layout with out_ch >= ch channels, of which the call fills the first ch (so out_p = out_h + the
 * offset of channel ch of one tensor with out_ch = 2 ch stacks harmonic and percussive channels).  Either may be NULL, not both:
 * that side's masks and stores are skipped.  power > 0 (inf allowed), margins finite and >= 1, else KPR_E_BADARG; so are an even
 * kh / kp or one outside 3 ... 31, pointers not aligned to their element, an output that overlaps x, and outputs that overlap
 * each other in any way but as disjoint channel ranges of one out_ch-channel tensor.  frames * freq >= 2^30: KPR_E_UNSUPPORTED.
 * batch, ch, frames or freq == 0: returns 0, launches nothing.  One launch, no atomics, no host reads: capturable; the same
 * inputs give the same bits.
 * kpr_hpss_plan (host only): the tile of the dispatch, *tile_frames x *tile_freq outputs per workgroup; tile edges for tests. */
int kpr_hpss_plan(int64_t frames, int64_t freq, int kh, int kp, int* tile_frames, int* tile_freq);
int kpr_hpss_f32(const float* x, int64_t batch, int ch, int64_t frames, int64_t freq, int layout, int kh, int kp, double power,
                 double margin_h, double margin_p, int want_mask, float* out_h, float* out_p, int out_ch, kpr_stream_t stream);
int kpr_hpss_c64(const void* x, int64_t batch, int ch, int64_t frames, int64_t freq, int layout, int kh, int kp, double power,
                 double margin_h, double margin_p, int want_mask, void* out_h, void* out_p, int out_ch, kpr_stream_t stream);

/* ---- LFilter: one biquad IIR section along time on a waveform, kapre_amd.signal.LFilter ------------------------------------
 * x: float32 waveform, (batch, time, ch) [layout = LAST] or (batch, ch, time) [FIRST], contiguous; out: the same shape.
 * coef = (b0, b1, b2, a1, a2), already divided by a0, passed as doubles and used as such.  Every (batch item, channel) series:
 *   reverse 0:  y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2],   x, y = 0 for t < 0
 *   reverse 1:  y[t] = b0 x[t] + b1 x[t+1] + b2 x[t+2] - a1 y[t+1] - a2 y[t+2],   x, y = 0 for t >= len   (the adjoint of reverse 0)
 * in float64 arithmetic on the float32 samples, rounded to float32 once at the store: for a stable filter the output is the
 * float32 rounding of the float64 result up to the float64 error of the recurrence.  Required: every coefficient finite,
 * |a2| < 1 and |a1| < 1 + a2 (the stability triangle), else KPR_E_BADARG.  a1 == a2 == 0 (a pure FIR section) runs without a scan.
 * Two forms: whole-signal (one workgroup walks a series; one launch, one read, one write) and segmented (the time axis is cut into
 * segments of kpr_lfilter_plan's size: three launches on the stream, two reads, one write; chosen when batch * channels is small).
 * Option "lfilter_variant" forces one.  Each form gives the same bits from the same inputs; the two agree within the error
 * bound, not bit for bit.  The segmented form needs `workspace`: kpr_lfilter_workspace_bytes(...) bytes, 8-byte aligned, clear of
 * x and out (KPR_E_WORKSPACE when NULL or short; 0 bytes for a series of at most one segment; not read by the whole-signal form).
 * Pointers 4-byte aligned; 16-byte accesses for contiguous series whose length is a multiple of four behind 16-byte aligned
 * pointers.  x and out must not overlap (there is no in-place form).  2^30 elements or more per signal (per batch item for
 * LAST): KPR_E_UNSUPPORTED.  batch == 0 or len == 0: returns 0, launches nothing.  No atomics, no host reads: capturable.
 * Non-finite input: with t0 the first non-finite sample of a series in scan order, every output before t0 (after it for
 * reverse 1) equals bit for bit the output of the call in which that sample is 0; from t0 on the series is unspecified when a1 or
 * a2 is non-zero, and a pure FIR section is affected at t0 ... t0 + 2 (t0 - 2 ... t0) only.  Other series are never touched.
 * kpr_lfilter_plan (host only): out[0 ... 4] = samples per lane, per wave, per workgroup step, per segment, and the form
 * (1 whole-signal, 2 segmented) the dispatch uses for this shape under the current "lfilter_variant"; seams for tests.
 * kpr_lfilter_carry (host only): M (row-major 2 x 2) with (y[n-1], y[n-2]) = M (y[-1], y[-2]) for zero input, 0 <= n <= 2^20,
 * from the impulse response of 1 / A(z) in long double. */
int kpr_lfilter_plan(int64_t batch, int channels, int64_t len, int layout, int* out /* 5 */);
int kpr_lfilter_carry(const double coef[5], int64_t n, double M[4]);
int64_t kpr_lfilter_workspace_bytes(int64_t batch, int channels, int64_t len, int layout);
int kpr_lfilter_f32(const float* x, int64_t batch, int channels, int64_t len, int layout, const double coef[5] /* b0 b1 b2 a1 a2 */,
                    int reverse, float* out, void* workspace, size_t workspace_bytes, kpr_stream_t stream);

/* ---- Convolve: a short complex FIR along the frame axis of a complex spectrogram, kapre_amd.signal.Convolve ----------------
 * The middle launch of the partitioned overlap-save convolution (block length L, n_fft = 2 L, hop L): between kpr_stft_f32 with a
 * rectangular window and kpr_istft_f32 with the synthesis window [0] * L + [1] * L.
 * x: complex64 (outer, frames_in, inner), contiguous -> out: (outer, frames_out, inner); frames_out is the caller's choice.
 * channels_first: outer = batch * ch, inner = n_freq, band_div = 1; channels_last: outer = batch, inner = n_freq * ch,
 * band_div = ch; the bin of inner index i is i / band_div and n_freq = inner / band_div (inner % band_div != 0: KPR_E_BADARG).
 * h: complex64 DEVICE table (n_ir, n_part, n_freq), 1 <= n_part <= 32, n_ir >= 1 (KPR_E_BADARG otherwise).
 * idx: `items` DEVICE int32, one filter number per BATCH ITEM (outer % items == 0; the outer / items channels of an item share
 * its filter), or NULL: filter 0 for every item.  An entry outside [0, n_ir) is clamped into it: the kernel never reads outside
 * the table, whatever idx holds, and never reads idx on the host.
 *   out[o, k, i] = sum_{p = 0}^{n_part - 1} x[o, k - p, i] h[idx[o / (outer / items)], p, i / band_div]
 * with x[o, r, i] = 0 for r < 0 and r >= frames_in.  The sum runs in ascending p from +0, every term as the four FMAs
 * re += xr hr; re -= xi hi; im += xr hi; im += xi hr in that order; a term whose input row is outside x is skipped.  So the same
 * inputs give the same bits whatever the launch shape (no atomics), and a non-finite bin of x reaches the rows k ... k + n_part - 1
 * of its own column only.
 * x / h / out 8-byte, idx 4-byte aligned; 16-byte accesses when inner is even and x and out are 16-byte aligned.  x == out or any
 * overlap of out with x, h or idx: KPR_E_BADARG, as are negative sizes and NULL x / h / out.  frames_in * inner or
 * frames_out * inner >= 2^30: KPR_E_UNSUPPORTED.  outer, frames_out or inner == 0: returns 0, launches nothing.  One launch, no
 * workspace, no host reads: capturable.
 * kpr_spec_fir_plan (host only): out[0 ... 2] = output rows per wave, waves per workgroup (a workgroup covers their product of
 * consecutive output frames per step) and the compile-time bucket (4, 8, 16 or 32) that n_part runs in; seams for tests. */
int kpr_spec_fir_plan(int64_t frames_out, int64_t inner, int n_part, int* out /* 3 */);
int kpr_spec_fir_c64(const void* x, int64_t outer, int64_t frames_in, int64_t inner, int band_div, const void* h, int n_ir, int n_part,
                     const int32_t* idx /* may be NULL */, int64_t items, void* out, int64_t frames_out, kpr_stream_t stream);

/* ---- AddNoise: noise mixed into a waveform at a per-item signal-to-noise ratio, kapre_amd.augmentation.AddNoise ------------
 * x: float32 waveform, (batch, time, ch) [layout = LAST] or (batch, ch, time) [FIRST], contiguous; out: the same shape.
 * noise: float32 DEVICE bank (n_noise, stride), row k holding lengths[k] samples (DEVICE int32, 1 <= lengths[k] <= stride).
 * table: DEVICE int32 (batch, 4), the row of item b = (index, offset, snr in dB as float32 bits, 0).  The kernels clamp index into
 * [0, n_noise), the length into [1, stride] and offset into [0, length): they never read outside the bank, whatever the table
 * holds, and nothing is read on the host.  With k = index, o = offset, L = lengths[k], C = channels, T = time:
 *   seg[t]  = noise[k][(o + t) mod L]                                   the noise tiles circularly
 *   Sx      = sum_{c,t} x[b,c,t]^2,   Sn = sum_t seg[t]^2               float64 sums of the exact float32 products
 *   g       = sqrt((Sx / (C T)) / (Sn / T)) 10^(-snr / 20)              float64, rounded once to float32; +0 if Sx == 0 or Sn == 0
 *   out[b,c,t] = fmaf(g, seg[t], x[b,c,t])                              the channels of an item share its noise and its gain
 * so snr is the ratio of the item's mean signal power to the mean power of the noise that is added.  stats: DEVICE float64
 * (batch, 4), written: (Sx, Sn, g, 0) per item.  A NaN / Inf sample makes its own item non-finite and touches no other.
 * kpr_add_noise_bwd_f32, the exact input gradient (noise and snr are constants, the gain is not):
 *   D = sum_{c,t} gy[b,c,t] seg[t] (float64),  coef = (D g) / Sx rounded once to float32 (0 if Sx == 0),
 *   gx[b,c,t] = fmaf(coef, x[b,c,t], gy[b,c,t])
 * with (Sx, g) read from `stats`, the rows the forward call wrote; stats_out (may be NULL, may be `stats`): (Sx, Sn, g, D).
 * Two forms (option "addnoise_variant"): resident -- an item of at most kpr_add_noise_plan's limit of floats stays in the
 * registers of one workgroup, one launch, one read -- and streamed -- two launches, partial sums of chunks of the item in
 * `workspace`, added in ascending chunk order.  No atomics: each form gives the same bits from the same inputs; the two sum in
 * different orders and agree within the error bound, not bit for bit.  workspace: kpr_add_noise_workspace_bytes(...) bytes, 8-byte
 * aligned, clear of everything else (KPR_E_WORKSPACE when the streamed form finds it NULL or short; the resident form does not
 * read it).  16-byte accesses behind 16-byte aligned x / out (gy / x / gx); any 4-byte aligned base is taken.
 * Errors: NULL pointers, n_noise < 1, stride < 1, time < 1, channels < 1, out overlapping x (there is no in-place form) or any
 * other argument: KPR_E_BADARG; time * channels >= 2^30: KPR_E_UNSUPPORTED.  batch == 0: returns 0, launches nothing.  No host
 * reads, nothing copied per call: capturable.
 * kpr_add_noise_plan (host only): out[0 ... 3] = floats per chunk of the streamed form, chunks per item, the resident limit in
 * floats per item, and the form (1 streamed, 2 resident) the dispatch uses for this shape under the current option; seams for tests.
 * kpr_noise_draw: the table of a training step, drawn on the device.  The same 16-byte state, generator and rules as
 * kpr_index_draw: Philox4x32-10, counter (item, 0, calls_lo, calls_hi), key (seed_lo, seed_hi) -> r0, r1, r2;
 *   index = mulhi32(r0, n_noise), offset = mulhi32(r1, lengths[index]),
 *   snr = (float)fma(snr_hi - snr_lo, r2 * 2^-32, snr_lo): the difference rounded to float64, ONE float64 fma, one rounding to
 *   float32 -- uniform in [snr_lo, snr_hi], and snr_lo itself when the two are equal;
 * calls advances by one (also for n_items == 0).  table 16-byte aligned.  n_noise < 1, n_items < 0, snr_lo > snr_hi or either not
 * finite, NULL state / lengths / table: KPR_E_BADARG; more than 2^20 items: KPR_E_UNSUPPORTED.  One launch, one workgroup. */
int kpr_noise_draw(int32_t* table, int64_t n_items, int n_noise, const int32_t* lengths, double snr_lo, double snr_hi, void* state,
                   kpr_stream_t stream);
int kpr_add_noise_plan(int64_t batch, int channels, int64_t time, int layout, int* out /* 4 */);
int64_t kpr_add_noise_workspace_bytes(int64_t batch, int channels, int64_t time, int layout);
int kpr_add_noise_f32(const float* x, int64_t batch, int channels, int64_t time, int layout, const float* noise, int n_noise,
                      int64_t stride, const int32_t* lengths, const int32_t* table, float* out, double* stats, void* workspace,
                      size_t workspace_bytes, kpr_stream_t stream);
int kpr_add_noise_bwd_f32(const float* gy, const float* x, int64_t batch, int channels, int64_t time, int layout, const float* noise,
                          int n_noise, int64_t stride, const int32_t* lengths, const int32_t* table, const double* stats, float* gx,
                          double* stats_out, void* workspace, size_t workspace_bytes, kpr_stream_t stream);

/* LogmelToMFCC.call (tf.signal.mfccs_from_log_mel_spectrograms, signal.py:418-436) has no entry
 * point of its own: it is kpr_apply_filterbank_f32 with the (n_mels, n_mfccs) DCT-II matrix
 * M[n][k] = 2 cos(pi (2n+1) k / (2 n_mels)) / sqrt(2 n_mels) and fb_kranges_host = NULL. */

#ifdef __cplusplus
}
#endif
#endif /* KAPRE_HIP_H */
