"""ctypes binding of libkapre_hip.so (C ABI declared in include/kapre_hip.h).

PyTorch is only the device-memory container: tensors are passed as raw device pointers together
with the raw hipStream_t of torch's current stream.  There is NO CPU fallback: if the shared
library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# KAPRE_AMD_LIB: development override to A/B alternative builds of the same source
LIB_PATH = os.environ.get("KAPRE_AMD_LIB") or os.path.join(_HERE, "lib", "libkapre_hip.so")

CHANNELS_FIRST, CHANNELS_LAST = 0, 1
OUT_COMPLEX, OUT_MAGNITUDE, OUT_PHASE = 0, 1, 2
# the KPR_E_* return codes (include/kapre_hip.h)
E_BADARG, E_UNSUPPORTED, E_HIP, E_WORKSPACE, E_DEVICE = -1, -2, -3, -4, -5


class StftGeom(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int64), ("channels", ctypes.c_int32), ("time", ctypes.c_int64),
                ("n_fft", ctypes.c_int32), ("win_length", ctypes.c_int32),
                ("hop_length", ctypes.c_int32), ("pad_begin", ctypes.c_int32),
                ("pad_end", ctypes.c_int32), ("in_layout", ctypes.c_int32),
                ("out_layout", ctypes.c_int32)]


class DbParams(ctypes.Structure):
    _fields_ = [("enabled", ctypes.c_int32), ("ref_value", ctypes.c_float),
                ("amin", ctypes.c_float), ("dynamic_range", ctypes.c_float)]


EXPORTS = {
    # name: (restype, argtypes)
    "kpr_version": (ctypes.c_int, []),
    "kpr_last_error": (ctypes.c_char_p, []),
    "kpr_last_launches": (ctypes.c_char_p, []),
    "kpr_fft_fast_path": (ctypes.c_int, [ctypes.c_int]),
    "kpr_fft_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "kpr_num_frames": (ctypes.c_int64, [ctypes.POINTER(StftGeom)]),
    "kpr_stft_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(StftGeom), ctypes.c_int]),
    "kpr_stft_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StftGeom), ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                    ctypes.c_void_p]),
    "kpr_mel_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(StftGeom), ctypes.c_int,
                                                 ctypes.POINTER(DbParams)]),
    "kpr_mel_workspace_bytes_unpacked": (ctypes.c_int64, [ctypes.POINTER(StftGeom), ctypes.c_int]),
    "kpr_mel_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StftGeom), ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                   ctypes.POINTER(DbParams), ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_int64, ctypes.c_void_p]),
    "kpr_filterbank_forget": (ctypes.c_int, [ctypes.c_void_p]),
    "kpr_set_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "kpr_get_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    "kpr_debug_stamps": (ctypes.c_int, [ctypes.c_void_p]),
    "kpr_debug_sclk_mhz": (ctypes.c_int, [ctypes.POINTER(ctypes.c_float)]),
    "kpr_debug_calib_read8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "kpr_filterbank_pack_floats": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "kpr_filterbank_pack": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_filterbank_kranges": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_void_p]),
    "kpr_abs_c64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                   ctypes.c_void_p]),
    "kpr_angle_c64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_void_p]),
    "kpr_apply_filterbank_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_apply_filterbank_packed_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                       ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_db_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "kpr_mag_to_db_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.POINTER(DbParams), ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int64, ctypes.c_void_p]),
    # float64 / complex128 variants (layers built with dtype='float64')
    "kpr_stft_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StftGeom), ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "kpr_istft_f64_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(StftGeom), ctypes.c_int64]),
    "kpr_istft_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StftGeom), ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_void_p]),
    "kpr_abs_c128": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_angle_c128": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_apply_filterbank_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "kpr_mag_to_db_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]),
    # backward passes (kapre_amd/autograd.py)
    "kpr_abs_c64_bwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "kpr_angle_c64_bwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "kpr_abs_c128_bwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "kpr_angle_c128_bwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "kpr_spec_edge_scale_c64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "kpr_spec_edge_scale_c128": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "kpr_mag_to_db_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.POINTER(DbParams), ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_mag_to_db_bwd_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "kpr_frame_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_energy_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                          ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_delta_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_device_status": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint)]),
    "kpr_debug_spin_timeout": (ctypes.c_int, [ctypes.c_void_p]),
    "kpr_istft_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(StftGeom), ctypes.c_int64]),
    "kpr_istft_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StftGeom), ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_void_p]),
    "kpr_frame_count": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "kpr_frame_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_energy_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_delta_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p]),
    # augmentation layers (kapre_amd/augmentation.py)
    "kpr_spec_augment_draw": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_spec_augment_apply_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                  ctypes.c_void_p]),
    "kpr_channel_gather": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                          ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    # mu-law companding (kapre_amd/signal.py) and ConcatenateFrequencyMap (kapre_amd/time_frequency.py)
    "kpr_mu_law_encode_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "kpr_mu_law_decode_i32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "kpr_mu_law_decode_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "kpr_mu_law_decode_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_freq_map_concat_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_freq_map_concat_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                                   ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    # PCEN (kapre_amd/time_frequency.py)
    "kpr_pcen_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int)]),
    "kpr_pcen_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_pcen_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                        ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_pcen_bwd_params_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "kpr_pcen_bwd_params_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    # CMVN (kapre_amd/time_frequency.py)
    "kpr_cmvn_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int)]),
    "kpr_cmvn_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_float,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_cmvn_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                        ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    # Resample (kapre_amd/signal.py)
    "kpr_resample_table_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                               ctypes.POINTER(ctypes.c_int)]),
    "kpr_resample_table": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_resample_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "kpr_resample_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_resample_direct_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "kpr_resample_direct_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                               ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    # Griffin-Lim (kapre_amd/time_frequency.py)
    "kpr_griffin_lim_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "kpr_gl_project_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p]),
    "kpr_gl_init_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "kpr_griffin_lim_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(StftGeom), ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "kpr_griffin_lim_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StftGeom), ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p]),
    # TimeStretch (kapre_amd/time_frequency.py)
    "kpr_time_stretch_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int),
                                             ctypes.POINTER(ctypes.c_int)]),
    "kpr_time_stretch_c64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    # HPSS (kapre_amd/time_frequency.py)
    "kpr_hpss_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int)]),
    **{name: (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                             ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
       for name in ("kpr_hpss_f32", "kpr_hpss_c64")},
    # LFilter (kapre_amd/signal.py)
    "kpr_lfilter_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "kpr_lfilter_carry": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]),
    "kpr_lfilter_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    "kpr_lfilter_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_size_t, ctypes.c_void_p]),
    # Convolve (kapre_amd/signal.py) and Reverb (kapre_amd/augmentation.py)
    "kpr_spec_fir_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "kpr_spec_fir_c64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "kpr_index_draw": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    # AddNoise (kapre_amd/augmentation.py)
    "kpr_noise_draw": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]),
    "kpr_add_noise_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "kpr_add_noise_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    "kpr_add_noise_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kpr_add_noise_bwd_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_void_p]),
}

PAD_MODES = {"constant": 0, "symmetric": 1, "reflect": 2}

_lib = None
_lock = threading.Lock()


def lib():
    """The loaded shared library; raises RuntimeError (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "kapre_amd: %s is missing - build it with `python -m kapre_amd.build` "
                        "(or __graft_entry__.build()).  There is no CPU fallback." % LIB_PATH)
                # torch ships its own libamdhip64: import it FIRST so that libkapre_hip.so's dependency resolves to
                # that already-loaded copy -- loaded the other way round the process holds two HIP runtimes and
                # torch's device pointers mean nothing to ours ("no ROCm-capable device is detected")
                try:
                    import torch  # noqa: F401
                except ImportError:
                    pass
                handle = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in EXPORTS.items():
                    fn = getattr(handle, name)
                    fn.restype = res
                    fn.argtypes = args
                _lib = handle
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().kpr_last_error().decode("utf-8", "replace")
        raise RuntimeError("kapre_amd: %s failed (code %d): %s" % (what, rc, msg))


def checked_size(n, what: str) -> int:
    """The count an entry point of the ``*_bytes`` / ``*_count`` kind returned; a negative one is its error."""
    n = int(n)
    if n < 0:
        check(E_BADARG, what)
    return n


def set_option(name: str, value: int) -> int:
    """kpr_set_option; returns the previous value (so tests can restore it)."""
    old = ctypes.c_int(0)
    check(lib().kpr_get_option(name.encode(), ctypes.byref(old)), "kpr_get_option")
    check(lib().kpr_set_option(name.encode(), int(value)), "kpr_set_option")
    return old.value


def last_launches() -> str:
    """Kernel names the calling thread's most recent hot-path call launched (kpr_last_launches)."""
    return lib().kpr_last_launches().decode("utf-8", "replace")


def device_status(synchronize: bool = True, raise_on_error: bool = True) -> int:
    """kpr_device_status: the bits raised by kernels that gave up a bounded wait since the last call (0 = healthy), cleared by
    reading.  ``synchronize`` waits for the device first (the word is only final for launches that have finished).  With
    ``raise_on_error`` a non-zero word raises RuntimeError (the outputs of the affected launches are wrong)."""
    if synchronize:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    flags = ctypes.c_uint(0)
    rc = lib().kpr_device_status(ctypes.byref(flags))
    if rc != 0 and raise_on_error:
        check(rc, "kpr_device_status")
    return int(flags.value)


def sclk_mhz() -> float:
    """Shader clock in MHz under a dense packed-f32 vector load (kpr_debug_sclk_mhz; blocking, ~0.3 ms of GPU time)."""
    out = ctypes.c_float(0.0)
    check(lib().kpr_debug_sclk_mhz(ctypes.byref(out)), "kpr_debug_sclk_mhz")
    return float(out.value)


PACK_HEADER_FLOATS = 64

# kpr_fft_plan codes (include/kapre_hip.h)
FFT_DFT_GEMM, FFT_POW2, FFT_MIXED_RADIX, FFT_TWO_PASS, FFT_BLUESTEIN, FFT_SUB_FFT, FFT_GENERIC = range(7)


def layout(fmt) -> int:
    """The layout enum of a data-format string; an enum is returned as it is."""
    if isinstance(fmt, int):
        return fmt
    return CHANNELS_LAST if fmt == "channels_last" else CHANNELS_FIRST


def is_channels_last(fmt) -> bool:
    return fmt in ("channels_last", CHANNELS_LAST)


def current_stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("kapre_amd: no HIP device visible (torch.cuda.is_available() is "
                           "False); the MI355X kernels have no CPU fallback")


def as_device(x, dtype):
    """numpy / torch (any device, any dtype) -> contiguous torch tensor of ``dtype`` on the current GPU."""
    import torch
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and x.is_contiguous():
        return x                                   # steady-state fast path
    require_gpu()
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    if not x.is_cuda:
        x = x.to(torch.device("cuda", torch.cuda.current_device()))
    if x.dtype != dtype:
        x = x.to(dtype)
    return x.contiguous()


def is_f64(x) -> bool:
    """True for float64 / complex128 numpy arrays and torch tensors."""
    import torch
    if isinstance(x, np.ndarray):
        return x.dtype in (np.float64, np.complex128)
    return isinstance(x, torch.Tensor) and x.dtype in (torch.float64, torch.complex128)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


class DeviceConstants:
    """Constants (windows, filterbanks, tables) uploaded once per (key, device) and kept.  Without ``max_entries`` nothing is
    ever dropped: a captured graph replays the addresses it recorded.  With it the oldest entry goes first."""

    def __init__(self, max_entries=None):
        self._cache = {}
        self._lock = threading.RLock()
        self._max_entries = max_entries

    def get(self, key, device, make, on_new=None):
        """The tensor on ``device`` of the numpy array ``make()`` returns, or the tuple of tensors of its tuple of arrays
        (what is no array -- a tensor, a ``ResamplePlan`` -- moves itself: its ``to(device)`` is kept).  A hit is one dict
        lookup; a miss builds and uploads under the lock, so ``make`` runs once per (key, device) however many threads ask,
        and ``on_new(value)`` once, right after the upload."""
        k = (key, str(device))
        value = self._cache.get(k)
        if value is None:
            with self._lock:
                value = self._cache.get(k)
                if value is None:
                    import torch

                    def upload(a):
                        return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(device)

                    made = make()
                    value = tuple(upload(a) for a in made) if isinstance(made, tuple) else upload(made)
                    if on_new is not None:
                        on_new(value)
                    while self._max_entries is not None and len(self._cache) >= self._max_entries:
                        self._cache.pop(next(iter(self._cache)))
                    self._cache[k] = value
        return value

    def clear(self):
        with self._lock:
            self._cache.clear()

    def __len__(self):
        return len(self._cache)


def filterbank_pack(fb_host: np.ndarray, kranges: np.ndarray) -> np.ndarray:
    """Host copy of the filterbank in the MFMA-fragment order the fused kernel streams."""
    fb_host = np.ascontiguousarray(fb_host, dtype=np.float32)
    n_freq, n_filt = fb_host.shape
    kr = kranges.ctypes.data_as(ctypes.c_void_p) if kranges is not None else ctypes.c_void_p(0)
    n = checked_size(lib().kpr_filterbank_pack_floats(n_freq, n_filt, kr), "kpr_filterbank_pack_floats")
    out = np.zeros(n, dtype=np.float32)
    check(lib().kpr_filterbank_pack(fb_host.ctypes.data_as(ctypes.c_void_p), n_freq, n_filt, kr,
                                    out.ctypes.data_as(ctypes.c_void_p)), "kpr_filterbank_pack")
    return out


def filterbank_forget(addr: int):
    """Drop what the library cached about the packed filterbank at device address ``addr`` (it is being freed)."""
    lib().kpr_filterbank_forget(ctypes.c_void_p(addr))


def filterbank_kranges(fb_host: np.ndarray) -> np.ndarray:
    """Per 16-filter tile [lo, hi) row range outside of which the (n_freq, n_filt) matrix is 0."""
    fb_host = np.ascontiguousarray(fb_host, dtype=np.float32)
    n_freq, n_filt = fb_host.shape
    out = np.zeros(2 * ((n_filt + 15) // 16), dtype=np.int32)
    check(lib().kpr_filterbank_kranges(fb_host.ctypes.data_as(ctypes.c_void_p), n_freq, n_filt,
                                       out.ctypes.data_as(ctypes.c_void_p)),
          "kpr_filterbank_kranges")
    return out


# ---------------------------------------------------------------------------------------------
# native operations: one launcher per entry point family, shared by the layers and their backward passes.  Each picks
# the float32 / float64 entry point from the dtype of the (contiguous, device) tensor it is given, allocates the output
# and the workspace, and runs the call with the tensor's device current on torch's current stream there.
# ---------------------------------------------------------------------------------------------
def dims_of(shape, fmt):
    """(b, *inner, c) for channels_last, (b, c, *inner) for channels_first -> (b, c, *inner).  ``fmt`` is a data-format
    string or a layout enum."""
    if is_channels_last(fmt):
        return (shape[0], shape[-1], *shape[1:-1])
    return tuple(shape)


def shape_of(fmt, b, c, *inner):
    """The inverse of ``dims_of``."""
    return (b, *inner, c) if is_channels_last(fmt) else (b, c, *inner)


def workspace(nbytes: int, device):
    import torch
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _call(name: str, device, *args):
    """``name``(*args, stream) with ``device`` current; raises naming ``name`` when it fails."""
    import torch
    with torch.cuda.device(device):
        check(getattr(lib(), name)(*args, current_stream_ptr()), name)


def mel_workspace_bytes(g_ref, n_filt: int, db_ref, packed: bool) -> int:
    """kpr_mel_f32's scratch: without a packed filterbank it takes its two-kernel path, which stages the spectrum."""
    L = lib()
    return checked_size(L.kpr_mel_workspace_bytes(g_ref, n_filt, db_ref) if packed
                        else L.kpr_mel_workspace_bytes_unpacked(g_ref, n_filt), "kpr_mel_workspace_bytes")


def num_frames(geom: StftGeom) -> int:
    return checked_size(lib().kpr_num_frames(ctypes.byref(geom)), "kpr_num_frames")


def stft(x, geom: StftGeom, n_frames: int, window, mode: int):
    """STFT of the float32 / float64 waveform ``x`` (``geom``; ``n_frames = num_frames(geom)``) with ``window`` of x's
    dtype: complex spectrogram for OUT_COMPLEX, else real, laid out as geom.out_layout."""
    import torch
    f64 = x.dtype == torch.float64
    dtype = ((torch.complex128 if f64 else torch.complex64) if mode == OUT_COMPLEX else x.dtype)
    out = torch.empty(shape_of(geom.out_layout, geom.batch, geom.channels, n_frames, geom.n_fft // 2 + 1),
                      dtype=dtype, device=x.device)
    if f64:
        _call("kpr_stft_f64", x.device, ptr(x), ctypes.byref(geom), ptr(window), ptr(out), mode)
    else:
        ws_bytes = int(lib().kpr_stft_workspace_bytes(ctypes.byref(geom), mode))
        ws = workspace(ws_bytes, x.device)
        _call("kpr_stft_f32", x.device, ptr(x), ctypes.byref(geom), ptr(window), ptr(out), mode, ptr(ws), ws_bytes)
    return out


def istft(spec, window, n_fft: int, win_length: int, hop_length: int, wave_fmt, spec_fmt):
    """Inverse STFT of the complex64 / complex128 spectrogram ``spec`` (n_fft // 2 + 1 bins) with the synthesis
    ``window``: (n_frames - 1) hop + win samples per signal (untrimmed), float32 / float64."""
    import torch
    f64 = spec.dtype == torch.complex128
    b, c, f, _ = dims_of(spec.shape, spec_fmt)
    # StftGeom: in_layout = waveform layout, out_layout = spectrogram layout
    g = StftGeom(b, c, 0, int(n_fft), int(win_length), int(hop_length), 0, 0, layout(wave_fmt), layout(spec_fmt))
    t_out = (f - 1) * int(hop_length) + int(win_length) if f > 0 else 0
    out = torch.empty(shape_of(wave_fmt, b, c, t_out), dtype=torch.float64 if f64 else torch.float32,
                      device=spec.device)
    L = lib()
    ws_bytes = int((L.kpr_istft_f64_workspace_bytes if f64 else L.kpr_istft_workspace_bytes)(ctypes.byref(g), f))
    ws = workspace(ws_bytes, spec.device)
    _call("kpr_istft_f64" if f64 else "kpr_istft_f32", spec.device, ptr(spec), ctypes.byref(g), f, ptr(window),
          ptr(out), ptr(ws), ws_bytes)
    return out


def edge_scale(spec, n_fft: int, fmt, s_edge: float, s_mid: float, out=None):
    """``spec`` (complex) times s_edge on the DC / Nyquist bins, s_mid elsewhere."""
    import torch
    if out is None:
        out = torch.empty_like(spec)
    b, c, f, k = dims_of(spec.shape, fmt)
    inner = c if is_channels_last(fmt) else 1
    _call("kpr_spec_edge_scale_c128" if spec.dtype == torch.complex128 else "kpr_spec_edge_scale_c64", spec.device,
          ptr(spec), spec.numel(), int(k), int(inner), int(n_fft), float(s_edge), float(s_mid), ptr(out))
    return out


def _cplx_to_real_name(x, phase: bool) -> str:
    import torch
    if x.dtype == torch.complex128:
        return "kpr_angle_c128" if phase else "kpr_abs_c128"
    return "kpr_angle_c64" if phase else "kpr_abs_c64"


def cplx_to_real(x, phase: bool):
    """|x|, or angle(x) with ``phase``, of a complex64 / complex128 tensor: float32 / float64."""
    import torch
    out = torch.empty(x.shape, dtype=torch.float64 if x.dtype == torch.complex128 else torch.float32, device=x.device)
    _call(_cplx_to_real_name(x, phase), x.device, ptr(x), x.numel(), ptr(out))
    return out


def cplx_to_real_bwd(x, g, phase: bool):
    """Cotangent of ``x`` from the cotangent ``g`` of ``cplx_to_real(x, phase)``."""
    import torch
    g = g.contiguous().to(torch.float64 if x.dtype == torch.complex128 else torch.float32)
    gx = torch.empty_like(x)
    _call(_cplx_to_real_name(x, phase) + "_bwd", x.device, ptr(x), ptr(g), x.numel(), ptr(gx))
    return gx


def freq_matmul(x, fmt, mat, packed=None, kranges=None):
    """x . mat over the frequency axis of the rank-4 float32 / float64 tensor ``x`` (``mat``: (n_in, n_out), x's dtype).
    ``kranges`` (host int32 row ranges of a banded filterbank) selects the filterbank entry point, which also takes the
    optional MFMA-ordered copy ``packed``; without it float32 runs the plain GEMM."""
    import torch
    b, c, f, n_in = dims_of(x.shape, fmt)
    n_out = int(mat.shape[1])
    out = torch.empty(shape_of(fmt, b, c, f, n_out), dtype=x.dtype, device=x.device)
    args = (ptr(x), b, c, f, n_in, layout(fmt), ptr(mat))
    if x.dtype == torch.float64:
        _call("kpr_apply_filterbank_f64", x.device, *args, n_out, ptr(out))
    elif kranges is not None:
        _call("kpr_apply_filterbank_packed_f32", x.device, *args, ptr(packed), n_out,
              kranges.ctypes.data_as(ctypes.c_void_p), ptr(out))
    else:
        _call("kpr_apply_filterbank_f32", x.device, *args, n_out, ctypes.c_void_p(0), ptr(out))
    return out


def _db_items(x):
    """(items, item size) of the decibel entry points: the leading axis holds the items; a rank-1 tensor is one."""
    if x.dim() > 1:
        return x.shape[0], x.numel() // max(x.shape[0], 1)
    return 1, x.numel()


def mag_to_db(x, ref_value: float, amin: float, dynamic_range: float):
    """backend.magnitude_to_decibel of a float32 / float64 tensor."""
    import torch
    out = torch.empty_like(x)
    n_items, item = _db_items(x)
    if x.dtype == torch.float64:
        _call("kpr_mag_to_db_f64", x.device, ptr(x), n_items, item, float(ref_value), float(amin),
              float(dynamic_range), ptr(out))
    else:
        ws_bytes = int(lib().kpr_db_workspace_bytes(n_items))
        ws = workspace(ws_bytes, x.device)
        db = DbParams(1, float(ref_value), float(amin), float(dynamic_range))
        _call("kpr_mag_to_db_f32", x.device, ptr(x), n_items, item, ctypes.byref(db), ptr(out), ptr(ws), ws_bytes)
    return out


def mag_to_db_bwd(x, g, ref_value: float, amin: float, dynamic_range: float):
    """Cotangent of ``x`` from the cotangent ``g`` of ``mag_to_db(x, ...)``."""
    import torch
    g = g.contiguous().to(x.dtype)
    gx = torch.empty_like(x)
    n_items, item = _db_items(x)
    if x.dtype == torch.float64:
        _call("kpr_mag_to_db_bwd_f64", x.device, ptr(x), ptr(g), n_items, item, ref_value, amin, dynamic_range,
              ptr(gx))
    else:
        db = DbParams(1, ref_value, amin, dynamic_range)
        _call("kpr_mag_to_db_bwd_f32", x.device, ptr(x), ptr(g), n_items, item, ctypes.byref(db), ptr(gx))
    return gx


# float32-only signal operations (kapre_amd/signal.py, Delta)
def _frame_count(t, frame_length, hop_length, pad_end) -> int:
    return checked_size(lib().kpr_frame_count(t, frame_length, hop_length, int(bool(pad_end))), "kpr_frame_count")


def frame(x, fmt, frame_length, hop_length, pad_end, pad_value):
    """tf.signal.frame of the waveform ``x``: (b, frames, frame_length, c) / (b, c, frames, frame_length)."""
    import torch
    b, c, t = dims_of(x.shape, fmt)
    f = _frame_count(t, frame_length, hop_length, pad_end)
    out = torch.empty(shape_of(fmt, b, c, f, frame_length), dtype=torch.float32, device=x.device)
    _call("kpr_frame_f32", x.device, ptr(x), b, c, t, layout(fmt), frame_length, hop_length, int(bool(pad_end)),
          float(pad_value), ptr(out))
    return out


def frame_bwd(g, x_shape, fmt, frame_length, hop_length, pad_end):
    import torch
    b, c, t = dims_of(x_shape, fmt)
    gx = torch.empty(x_shape, dtype=torch.float32, device=g.device)
    _call("kpr_frame_bwd_f32", g.device, ptr(g), b, c, t, layout(fmt), frame_length, hop_length, int(bool(pad_end)),
          ptr(gx))
    return gx


def energy(x, fmt, frame_length, hop_length, pad_end, pad_value, scale):
    """``scale`` times the sum of squares of each frame of the waveform ``x``: (b, frames, c) / (b, c, frames)."""
    import torch
    b, c, t = dims_of(x.shape, fmt)
    f = _frame_count(t, frame_length, hop_length, pad_end)
    out = torch.empty(shape_of(fmt, b, c, f), dtype=torch.float32, device=x.device)
    _call("kpr_energy_f32", x.device, ptr(x), b, c, t, layout(fmt), frame_length, hop_length, int(bool(pad_end)),
          float(pad_value), float(scale), ptr(out))
    return out


def energy_bwd(x, g, fmt, frame_length, hop_length, pad_end, scale):
    import torch
    b, c, t = dims_of(x.shape, fmt)
    gx = torch.empty(x.shape, dtype=torch.float32, device=g.device)
    _call("kpr_energy_bwd_f32", g.device, ptr(x), ptr(g), b, c, t, layout(fmt), frame_length, hop_length,
          int(bool(pad_end)), float(scale), ptr(gx))
    return gx


def delta(x, fmt, win_length, mode: str, backward: bool = False):
    """Delta of the rank-4 ``x`` along its time axis, or with ``backward`` its adjoint (x is then the cotangent)."""
    import torch
    b, c, t, f = dims_of(x.shape, fmt)
    out = torch.empty_like(x)
    _call("kpr_delta_bwd_f32" if backward else "kpr_delta_f32", x.device, ptr(x), b, c, t, f, layout(fmt), win_length,
          PAD_MODES[mode.lower()], ptr(out))
    return out


# augmentation layers (kapre_amd/augmentation.py)
def spec_augment_draw(state, n_items, n_time_masks, n_freq_masks, n_time, n_freq, time_mask_param, freq_mask_param):
    """A fresh SpecAugment mask table, drawn on the device from ``state`` (int64[2] there: seed, calls; calls advances by
    one): int32 (n_items, n_time_masks + n_freq_masks, 2) of inclusive (first, last), time masks first."""
    import torch
    table = torch.empty((n_items, n_time_masks + n_freq_masks, 2), dtype=torch.int32, device=state.device)
    _call("kpr_spec_augment_draw", state.device, ptr(table), n_items, n_time_masks, n_freq_masks, n_time, n_freq,
          int(time_mask_param), int(freq_mask_param), ptr(state))
    return table


def spec_augment_apply(x, table, n_time_masks, n_freq_masks, n_time, n_freq, mask_value, inplace=False):
    """``mask_value`` on the masked elements of the float32 ``x`` (n_items blocks of n_time x n_freq), ``x`` elsewhere:
    a new tensor, or with ``inplace`` ``x`` itself (the same kernel with out == x: no second buffer)."""
    import torch
    out = x if inplace else torch.empty_like(x)
    _call("kpr_spec_augment_apply_f32", x.device, ptr(x), ptr(out), ptr(table), table.shape[0], n_time_masks, n_freq_masks,
          n_time, n_freq, float(mask_value))
    return out


def index_draw(state, n_items: int, n_choices: int):
    """``n_items`` int32 indices uniform in [0, n_choices), drawn on the device from ``state`` (int64[2] there: seed, calls;
    calls advances by one)."""
    import torch
    out = torch.empty((int(n_items),), dtype=torch.int32, device=state.device)
    _call("kpr_index_draw", state.device, ptr(out), int(n_items), int(n_choices), ptr(state))
    return out


def channel_gather(x, ch_axis: int, perm):
    """``x`` (float32 / complex64) with the channels of axis ``ch_axis`` in the order ``perm`` (tf.gather)."""
    import torch
    shape = tuple(x.shape)
    outer = int(np.prod(shape[:ch_axis], dtype=np.int64))
    inner = int(np.prod(shape[ch_axis + 1:], dtype=np.int64))
    out = torch.empty_like(x)
    perm_host = (ctypes.c_int32 * len(perm))(*[int(p) for p in perm])
    _call("kpr_channel_gather", x.device, ptr(x), ptr(out), outer, shape[ch_axis], inner, x.element_size(), perm_host)
    return out


# mu-law companding (kapre_amd/signal.py) and ConcatenateFrequencyMap (kapre_amd/time_frequency.py)
def mu_law_encode(x, quantization_channels: int):
    """backend.mu_law_encoding of the float32 ``x`` (any shape): int32 codes."""
    import torch
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    _call("kpr_mu_law_encode_f32", x.device, ptr(x), x.numel(), int(quantization_channels), ptr(out))
    return out


def mu_law_decode(code, quantization_channels: int):
    """backend.mu_law_decoding of int32 or float32 codes (any shape): float32."""
    import torch
    out = torch.empty(code.shape, dtype=torch.float32, device=code.device)
    _call("kpr_mu_law_decode_i32" if code.dtype == torch.int32 else "kpr_mu_law_decode_f32", code.device, ptr(code),
          code.numel(), int(quantization_channels), ptr(out))
    return out


def mu_law_decode_bwd(code, g, quantization_channels: int):
    """Cotangent of the float32 ``code`` from the cotangent ``g`` of ``mu_law_decode(code, ...)``."""
    import torch
    g = g.contiguous().to(torch.float32)
    gx = torch.empty_like(code)
    _call("kpr_mu_law_decode_bwd_f32", code.device, ptr(code), ptr(g), code.numel(), int(quantization_channels), ptr(gx))
    return gx


def freq_map_concat(x, fmt, backward: bool = False):
    """The rank-4 float32 ``x`` with the frequency map f / (n_freq - 1) as one more (last) channel, or with ``backward`` the
    adjoint: ``x`` (then the cotangent) without its last channel."""
    import torch
    b, c, t, f = dims_of(x.shape, fmt)
    if backward:
        c -= 1
    out = torch.empty(shape_of(fmt, b, c + (0 if backward else 1), t, f), dtype=torch.float32, device=x.device)
    _call("kpr_freq_map_concat_bwd_f32" if backward else "kpr_freq_map_concat_f32", x.device, ptr(x), b, c, t, f,
          layout(fmt), ptr(out))
    return out


# PCEN (kapre_amd/time_frequency.py)
def pcen_plan(frames: int, inner: int):
    """(rows_per_wave, waves_per_group): the time tiling kpr_pcen_f32 uses (host only)."""
    rows, waves = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().kpr_pcen_plan(int(frames), int(inner), ctypes.byref(rows), ctypes.byref(waves)), "kpr_pcen_plan")
    return rows.value, waves.value


def _time_geometry(shape, fmt):
    """(outer, frames, inner, band_div, n_bands) of a rank-4 ``shape``: the contiguous (outer, frames, inner) problem that the
    time-tiled launchers (PCEN, CMVN, TimeStretch) hand to the library; the band of inner index i is i // band_div"""
    b, c, t, m = dims_of(shape, fmt)
    if is_channels_last(fmt):
        return b, t, m * c, c, m
    return b * c, t, m, 1, m


def pcen(x, fmt, params, eps: float, want_smooth: bool = False):
    """PCEN of the rank-4 float32 ``x``; ``params``: the device float32 vectors (s, alpha, delta, r), one value per band.
    With ``want_smooth`` returns (out, S), S being what ``pcen_bwd`` needs."""
    import torch
    out = torch.empty_like(x)
    smooth = torch.empty_like(x) if want_smooth else None
    _call("kpr_pcen_f32", x.device, ptr(x), *_time_geometry(x.shape, fmt), *(ptr(p) for p in params), float(eps), ptr(out),
          ptr(smooth))
    return (out, smooth) if want_smooth else out


def pcen_bwd(x, smooth, g, fmt, params, eps: float):
    """Cotangent of ``x`` from the cotangent ``g`` of ``pcen(x, ...)`` and the smoother ``smooth`` of that call."""
    import torch
    g = g.contiguous().to(torch.float32)
    gx = torch.empty_like(x)
    _call("kpr_pcen_bwd_f32", x.device, ptr(x), ptr(smooth), ptr(g), *_time_geometry(x.shape, fmt), *(ptr(p) for p in params),
          float(eps), ptr(gx))
    return gx


def pcen_bwd_params(x, smooth, g, fmt, params, eps: float, want_gx: bool = True):
    """(gx or None, gparams): the cotangents of ``x`` (with ``want_gx``) and of the four parameter vectors, ``gparams`` being the
    (4, n_bands) float32 tensor with rows s, alpha, delta, r.  Two launches; the same inputs give the same bits."""
    import torch
    g = g.contiguous().to(torch.float32)
    geom = _time_geometry(x.shape, fmt)
    gx = torch.empty_like(x) if want_gx else None
    gparams = torch.empty((4, geom[4]), dtype=torch.float32, device=x.device)
    ws_bytes = int(lib().kpr_pcen_bwd_params_workspace_bytes(*geom[:3]))
    ws = workspace(ws_bytes, x.device)
    _call("kpr_pcen_bwd_params_f32", x.device, ptr(x), ptr(smooth), ptr(g), *geom, *(ptr(p) for p in params), float(eps),
          ptr(gx), ptr(gparams), ptr(ws), ws_bytes)
    return gx, gparams


# CMVN (kapre_amd/time_frequency.py)
def cmvn_plan(frames: int, inner: int):
    """(rows_per_wave, waves_per_group, resident_frames): the time tiling kpr_cmvn_f32 uses and the longest series it keeps in
    registers (host only)."""
    rows, waves, resident = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(lib().kpr_cmvn_plan(int(frames), int(inner), ctypes.byref(rows), ctypes.byref(waves), ctypes.byref(resident)),
          "kpr_cmvn_plan")
    return rows.value, waves.value, resident.value


def cmvn(x, fmt, norm_vars: bool, eps: float, want_rstd: bool = False):
    """Mean (and with ``norm_vars`` variance) normalisation along time of the rank-4 float32 ``x``.  With ``want_rstd``
    (``norm_vars`` only) returns (out, rstd), rstd per column being what ``cmvn_bwd`` needs."""
    import torch
    b, c, _, m = dims_of(x.shape, fmt)
    out = torch.empty_like(x)
    # (one value per column: x's shape without the time axis)
    rstd = torch.empty(shape_of(fmt, b, c, m), dtype=torch.float32, device=x.device) if want_rstd else None
    _call("kpr_cmvn_f32", x.device, ptr(x), *_time_geometry(x.shape, fmt)[:3], int(bool(norm_vars)), float(eps), ptr(out),
          ptr(rstd))
    return (out, rstd) if want_rstd else out


def cmvn_bwd(y, rstd, g, fmt, norm_vars: bool):
    """Cotangent of ``x`` from the cotangent ``g`` of ``y = cmvn(x, ...)`` and the ``rstd`` of that call (without ``norm_vars``:
    from ``g`` alone, ``y`` and ``rstd`` may be None)."""
    import torch
    g = g.contiguous().to(torch.float32)
    gx = torch.empty_like(g)
    _call("kpr_cmvn_bwd_f32", g.device, ptr(y), ptr(rstd), ptr(g), *_time_geometry(g.shape, fmt)[:3], int(bool(norm_vars)),
          ptr(gx))
    return gx


# Resample (kapre_amd/signal.py)
def resample_table_size(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint: bool):
    """(n_phases, n_taps, step) of one direction's polyphase table (host only).  ``ValueError`` naming the table's size when
    the library does not support it, ``RuntimeError`` for any other failure."""
    P, n, q = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = lib().kpr_resample_table_size(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff),
                                       int(bool(adjoint)), ctypes.byref(P), ctypes.byref(n), ctypes.byref(q))
    if rc == E_UNSUPPORTED:
        raise ValueError('kapre_amd: ' + lib().kpr_last_error().decode("utf-8", "replace"))
    check(rc, "kpr_resample_table_size")
    return P.value, n.value, q.value


def resample_table(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint: bool):
    """(table, first, step): the float32 (n_phases, n_taps) coefficients and the int32 (n_phases,) first input offsets of one
    direction, as numpy arrays (host only)."""
    n_phases, n_taps, step = resample_table_size(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint)
    table = np.zeros((n_phases, n_taps), dtype=np.float32)
    first = np.zeros(n_phases, dtype=np.int32)
    check(lib().kpr_resample_table(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff),
                                   int(bool(adjoint)), table.ctypes.data_as(ctypes.c_void_p),
                                   first.ctypes.data_as(ctypes.c_void_p)), "kpr_resample_table")
    return table, first, step


def resample_plan(n_phases: int, n_taps: int, step: int) -> int:
    """outputs_per_tile of kpr_resample_f32's dispatch (host only)."""
    n = ctypes.c_int(0)
    check(lib().kpr_resample_plan(int(n_phases), int(n_taps), int(step), ctypes.byref(n)), "kpr_resample_plan")
    return n.value


class ResamplePlan:
    """One direction of a rate conversion: the table and the offsets (as ``resample_table`` made them, or on one device), and
    their shape."""
    __slots__ = ("table", "first", "n_phases", "n_taps", "step")

    def __init__(self, table, first, step):
        self.table, self.first, self.step = table, first, int(step)
        self.n_phases, self.n_taps = int(table.shape[0]), int(table.shape[1])

    def to(self, device):
        import torch
        return ResamplePlan(torch.as_tensor(self.table).to(device), torch.as_tensor(self.first).to(device), self.step)


_RESAMPLE_CONSTS = DeviceConstants()


def resample_plans(orig_freq, new_freq, lowpass_filter_width, rolloff, device):
    """(forward, adjoint) ``ResamplePlan`` of the conversion on ``device``, built and uploaded on first use and kept."""
    key = (int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff))
    return _RESAMPLE_CONSTS.get(key, device, lambda: tuple(ResamplePlan(*resample_table(*key, adjoint))
                                                           for adjoint in (False, True)))


def resample(x, fmt, plan: ResamplePlan, out_len: int):
    """The polyphase gather ``plan`` of the float32 waveform ``x`` along time: ``out_len`` samples per signal (the forward
    pass with the forward plan, its adjoint with the adjoint plan and the forward's input length)."""
    import torch
    b, c, t = dims_of(x.shape, fmt)
    out = torch.empty(shape_of(fmt, b, c, int(out_len)), dtype=torch.float32, device=x.device)
    _call("kpr_resample_f32", x.device, ptr(x), b, c, t, layout(fmt), ptr(plan.table), ptr(plan.first), plan.n_phases,
          plan.n_taps, plan.step, int(out_len), ptr(out))
    return out


def resample_direct_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, adjoint: bool):
    """(n_taps, outputs_per_tile) of one direction of the table-free conversion (host only).  ``ValueError`` naming the tap
    count when the library does not support it, ``RuntimeError`` for any other failure."""
    n, tile = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib().kpr_resample_direct_plan(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff),
                                        int(bool(adjoint)), ctypes.byref(n), ctypes.byref(tile))
    if rc == E_UNSUPPORTED:
        raise ValueError('kapre_amd: ' + lib().kpr_last_error().decode("utf-8", "replace"))
    check(rc, "kpr_resample_direct_plan")
    return n.value, tile.value


def resample_direct(x, fmt, params, adjoint: bool, out_len: int):
    """The table-free conversion ``params`` = (orig_freq, new_freq, lowpass_filter_width, rolloff) of the float32 waveform
    ``x`` along time, or with ``adjoint`` its adjoint: ``out_len`` samples per signal, whatever the natural length is."""
    import torch
    b, c, t = dims_of(x.shape, fmt)
    out = torch.empty(shape_of(fmt, b, c, int(out_len)), dtype=torch.float32, device=x.device)
    orig_freq, new_freq, width, rolloff = params
    _call("kpr_resample_direct_f32", x.device, ptr(x), b, c, t, layout(fmt), int(orig_freq), int(new_freq), int(width),
          float(rolloff), int(bool(adjoint)), int(out_len), ptr(out))
    return out


# LFilter (kapre_amd/signal.py)
LFILTER_WHOLE, LFILTER_SEGMENTED = 1, 2


def _coef5(coef):
    """(b0, b1, b2, a1, a2) as the five C doubles of the ABI."""
    c = [float(v) for v in coef]
    if len(c) != 5:
        raise ValueError('a section is (b0, b1, b2, a1, a2), got %d values' % len(c))
    return (ctypes.c_double * 5)(*c)


def lfilter_plan(batch: int, channels: int, length: int, fmt):
    """(samples_per_lane, samples_per_wave, samples_per_step, samples_per_segment, form) of kpr_lfilter_f32's dispatch for
    this shape under the current ``lfilter_variant``; form is LFILTER_WHOLE or LFILTER_SEGMENTED (host only)."""
    out = (ctypes.c_int * 5)()
    check(lib().kpr_lfilter_plan(int(batch), int(channels), int(length), layout(fmt), out), "kpr_lfilter_plan")
    return tuple(int(v) for v in out)


def lfilter_carry(coef, n: int) -> np.ndarray:
    """The (2, 2) float64 matrix that carries the state (y[-1], y[-2]) over ``n`` samples of zero input (host only).
    ``ValueError`` for coefficients outside the stability triangle or an ``n`` the library does not answer for."""
    m = (ctypes.c_double * 4)()
    rc = lib().kpr_lfilter_carry(_coef5(coef), int(n), m)
    if rc == E_BADARG:
        raise ValueError('kapre_amd: ' + lib().kpr_last_error().decode("utf-8", "replace"))
    check(rc, "kpr_lfilter_carry")
    return np.array(list(m), dtype=np.float64).reshape(2, 2)


def lfilter(x, fmt, coef, reverse: bool):
    """One biquad section ``coef`` = (b0, b1, b2, a1, a2) along time over the float32 waveform ``x``, from the first sample to
    the last or with ``reverse`` from the last to the first (the adjoint: the backward pass of the other direction)."""
    import torch
    b, c, t = dims_of(x.shape, fmt)
    out = torch.empty_like(x)
    ws_bytes = checked_size(lib().kpr_lfilter_workspace_bytes(b, c, t, layout(fmt)), "kpr_lfilter_workspace_bytes")
    ws = workspace(ws_bytes, x.device)
    _call("kpr_lfilter_f32", x.device, ptr(x), b, c, t, layout(fmt), _coef5(coef), int(bool(reverse)), ptr(out), ptr(ws), ws_bytes)
    return out


# Griffin-Lim (kapre_amd/time_frequency.py)
GL_INIT_ZERO, GL_INIT_RANDOM, GL_INIT_GIVEN = 0, 1, 2


def griffin_lim_plan(item_size: int):
    """(chunk_elems, chunks_per_item): how kpr_gl_project_f32 cuts an item of ``item_size`` complex bins into workgroup
    ranges (host only)."""
    ch, n = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().kpr_griffin_lim_plan(int(item_size), ctypes.byref(ch), ctypes.byref(n)), "kpr_griffin_lim_plan")
    return ch.value, n.value


def gl_project(R, T, mag, c: float, want_sc: bool = False):
    """One Griffin-Lim projection: S = mag a / (|a| + 1e-16) with a = R - c T (``T`` None: a = R, ``c`` must be 0).
    ``R`` / ``T``: complex64, ``mag``: float32, the same shape, whose leading axis holds the items.  With ``want_sc``
    returns (S, sc), sc per item being || |R| - mag || / || mag ||."""
    import torch
    n_items = int(R.shape[0]) if R.dim() > 0 else 1
    item = R.numel() // max(n_items, 1)
    S = torch.empty_like(R)
    sc = torch.empty((n_items,), dtype=torch.float32, device=R.device) if want_sc else None
    ws_bytes = 8 * n_items * griffin_lim_plan(item)[1] if want_sc else 0
    ws = workspace(ws_bytes, R.device)
    _call("kpr_gl_project_f32", R.device, ptr(R), ptr(T), ptr(mag), n_items, item, float(c), ptr(S), ptr(sc), ptr(ws), ws_bytes)
    return (S, sc) if want_sc else S


def gl_init(M, fmt, power: float, init_mode: int, state=None):
    """(mag, S_0) of a Griffin-Lim run from the rank-4 float32 magnitude ``M``: mag = M^(1/power) (``M`` itself for power 1),
    S_0 = mag with zero phase (GL_INIT_ZERO) or with the Philox phase drawn from the device generator ``state``
    (GL_INIT_RANDOM; its ``calls`` advances by one)."""
    import torch
    b, c, f, k = dims_of(M.shape, fmt)
    mag = torch.empty_like(M) if float(power) != 1.0 else None
    S = torch.empty(M.shape, dtype=torch.complex64, device=M.device)
    _call("kpr_gl_init_f32", M.device, ptr(M), b, c, f * k, layout(fmt), float(power), int(init_mode), ptr(state), ptr(mag), ptr(S))
    return (M if mag is None else mag), S


def griffin_lim_workspace_bytes(geom: StftGeom, n_frames: int, momentum: float, power: float) -> int:
    return checked_size(lib().kpr_griffin_lim_workspace_bytes(ctypes.byref(geom), int(n_frames), int(momentum != 0),
                                                              int(power != 1)), "kpr_griffin_lim_workspace_bytes")


def griffin_lim(mag, window, synth_window, n_fft: int, win_length: int, hop_length: int, wave_fmt, spec_fmt, n_iter: int,
                momentum: float, power: float, init_mode: int, init=None, state=None, want_sc: bool = True, ws=None):
    """The whole Griffin-Lim run (kpr_griffin_lim_f32) on the rank-4 float32 magnitude ``mag``: (waveform, sc) with the
    untrimmed waveform of (n_frames - 1) hop + win samples and sc the (n_iter, batch) device tensor of the convergence
    figures (None without ``want_sc``).  ``ws``: a uint8 device tensor to use as scratch when it is large enough."""
    import torch
    b, c, f, _ = dims_of(mag.shape, spec_fmt)
    g = StftGeom(b, c, 0, int(n_fft), int(win_length), int(hop_length), 0, 0, layout(wave_fmt), layout(spec_fmt))
    t_out = (f - 1) * int(hop_length) + int(win_length) if f > 0 else 0
    out = torch.empty(shape_of(wave_fmt, b, c, t_out), dtype=torch.float32, device=mag.device)
    sc = torch.empty((int(n_iter), b), dtype=torch.float32, device=mag.device) if want_sc else None
    ws_bytes = griffin_lim_workspace_bytes(g, f, momentum, power)
    if ws is None or ws.numel() < ws_bytes:
        ws = workspace(ws_bytes, mag.device)
    _call("kpr_griffin_lim_f32", mag.device, ptr(mag), ctypes.byref(g), f, ptr(window), ptr(synth_window), int(n_iter),
          float(momentum), float(power), int(init_mode), ptr(init), ptr(state), ptr(out), ptr(sc), ptr(ws), ws.numel())
    return out, sc


# TimeStretch (kapre_amd/time_frequency.py)
def time_stretch_plan(frames_out: int, inner: int):
    """(rows_per_wave, waves_per_group): the time tiling kpr_time_stretch_c64 uses (host only)."""
    rows, waves = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().kpr_time_stretch_plan(int(frames_out), int(inner), ctypes.byref(rows), ctypes.byref(waves)),
          "kpr_time_stretch_plan")
    return rows.value, waves.value


def time_stretch(x, fmt, idx, alpha, frames_out: int, want_phase: bool = False):
    """Phase-vocoder time stretch of the rank-4 complex64 ``x`` along its frame axis: ``frames_out`` frames, output frame t read
    from the input rows idx[t] and idx[t] + 1 with the weight alpha[t] (int32 / float32 device tensors of ``frames_out``
    entries).  With ``want_phase`` returns (out, phase), phase being the uint32 phase words in out's layout (as an int32
    tensor)."""
    import torch
    b, c, _, m = dims_of(x.shape, fmt)
    outer, t, inner = _time_geometry(x.shape, fmt)[:3]
    out = torch.empty(shape_of(fmt, b, c, int(frames_out), m), dtype=torch.complex64, device=x.device)
    phase = torch.empty(out.shape, dtype=torch.int32, device=x.device) if want_phase else None
    _call("kpr_time_stretch_c64", x.device, ptr(x), outer, t, int(frames_out), inner, ptr(idx), ptr(alpha), ptr(out), ptr(phase))
    return (out, phase) if want_phase else out


# HPSS (kapre_amd/time_frequency.py)
HPSS_VALUES, HPSS_MASKS, HPSS_MEDIANS = 0, 1, 2


def hpss_plan(frames: int, freq: int, kh: int = 31, kp: int = 31):
    """(tile_frames, tile_freq): the tile of outputs a workgroup of kpr_hpss_* owns (host only)."""
    tf, tq = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().kpr_hpss_plan(int(frames), int(freq), int(kh), int(kp), ctypes.byref(tf), ctypes.byref(tq)), "kpr_hpss_plan")
    return tf.value, tq.value


def hpss(x, fmt, kh: int, kp: int, power: float, margin_h: float, margin_p: float, mode: int = HPSS_VALUES, output: str = "pair"):
    """Median-filter harmonic-percussive separation of the rank-4 float32 / complex64 spectrogram ``x`` in one launch.
    ``mode``: HPSS_VALUES (x times the masks, x's dtype), HPSS_MASKS or HPSS_MEDIANS (the two median-filtered spectrograms, for
    tests), both float32.  ``output``: 'pair' -> (harmonic, percussive) as two tensors; 'both' -> one tensor with the channel
    axis doubled, harmonic channels first; 'harmonic' / 'percussive' -> that one alone (the other side's masks and stores are
    skipped)."""
    import torch
    cplx = x.is_complex()
    b, c, t, m = dims_of(x.shape, fmt)
    odt = torch.complex64 if cplx and mode == HPSS_VALUES else torch.float32
    new = lambda ch: torch.empty(shape_of(fmt, b, ch, t, m), dtype=odt, device=x.device)
    at = lambda ten, off: ctypes.c_void_p(ten.data_ptr() + off * ten.element_size()) if ten.numel() else ctypes.c_void_p(0)
    if output == "both":
        res = new(2 * c)
        out_ch, ph, pp = 2 * c, at(res, 0), at(res, c if is_channels_last(fmt) else c * t * m)
    elif output == "pair":
        res = (new(c), new(c))
        out_ch, ph, pp = c, ptr(res[0]), ptr(res[1])
    else:
        res = new(c)
        out_ch, ph, pp = (c, ptr(res), ctypes.c_void_p(0)) if output == "harmonic" else (c, ctypes.c_void_p(0), ptr(res))
    _call("kpr_hpss_c64" if cplx else "kpr_hpss_f32", x.device, ptr(x), b, c, t, m, layout(fmt), int(kh), int(kp),
          float(power), float(margin_h), float(margin_p), int(mode), ph, pp, out_ch)
    return res


# Convolve (kapre_amd/signal.py) and Reverb (kapre_amd/augmentation.py)
def spec_fir_plan(frames_out: int, inner: int, n_part: int):
    """(rows_per_wave, waves_per_group, bucket): the time tiling kpr_spec_fir_c64 uses and the compile-time bucket that
    ``n_part`` partitions run in (host only)."""
    out = (ctypes.c_int * 3)()
    check(lib().kpr_spec_fir_plan(int(frames_out), int(inner), int(n_part), out), "kpr_spec_fir_plan")
    return tuple(int(v) for v in out)


def spec_fir(x, fmt, h, idx, frames_out: int):
    """A complex FIR along the frame axis of the rank-4 complex64 ``x``: ``frames_out`` frames, output frame k the sum over p of
    input frame k - p (zero outside ``x``) times h[idx[item], p, bin].  ``h``: complex64 device table (n_ir, n_part, n_freq);
    ``idx``: int32 device tensor of one filter number per batch item, or None for filter 0."""
    import torch
    b, c, _, m = dims_of(x.shape, fmt)
    outer, t, inner, band_div, _ = _time_geometry(x.shape, fmt)
    out = torch.empty(shape_of(fmt, b, c, int(frames_out), m), dtype=torch.complex64, device=x.device)
    _call("kpr_spec_fir_c64", x.device, ptr(x), outer, t, inner, band_div, ptr(h), int(h.shape[0]), int(h.shape[1]), ptr(idx), b,
          ptr(out), int(frames_out))
    return out


# AddNoise (kapre_amd/augmentation.py, backend.add_noise)
ADDNOISE_STREAMED, ADDNOISE_RESIDENT = 1, 2


def noise_draw(state, n_items: int, lengths, snr_lo: float, snr_hi: float):
    """The int32 (n_items, 4) device table of an AddNoise step -- (index, offset, snr as float32 bits, 0) per item -- drawn on
    the device from ``state`` (int64[2] there: seed, calls; calls advances by one): index uniform over the ``lengths`` (int32
    device vector, one entry per noise), offset uniform below the length of that noise, snr uniform in [snr_lo, snr_hi]."""
    import torch
    table = torch.empty((int(n_items), 4), dtype=torch.int32, device=state.device)
    _call("kpr_noise_draw", state.device, ptr(table), int(n_items), int(lengths.shape[0]), ptr(lengths), float(snr_lo),
          float(snr_hi), ptr(state))
    return table


def add_noise_plan(batch: int, channels: int, time: int, fmt):
    """(chunk_floats, chunks_per_item, resident_limit_floats, form) of kpr_add_noise_f32's dispatch for this shape under the
    current ``addnoise_variant``; form is ADDNOISE_STREAMED or ADDNOISE_RESIDENT (host only)."""
    out = (ctypes.c_int * 4)()
    check(lib().kpr_add_noise_plan(int(batch), int(channels), int(time), layout(fmt), out), "kpr_add_noise_plan")
    return tuple(int(v) for v in out)


def add_noise_workspace_bytes(batch: int, channels: int, time: int, fmt) -> int:
    """Bytes of workspace the streamed form of kpr_add_noise_f32 / kpr_add_noise_bwd_f32 needs for this shape (host only)."""
    return checked_size(lib().kpr_add_noise_workspace_bytes(int(batch), int(channels), int(time), layout(fmt)),
                        "kpr_add_noise_workspace_bytes")


def add_noise(x, fmt, bank, lengths, table):
    """(y, stats): the float32 waveform ``x`` plus, per batch item, the noise ``bank[index]`` read circularly from ``offset`` and
    scaled to the item's ``snr`` -- ``table`` is the int32 (batch, 4) device table of (index, offset, snr bits, 0), ``bank`` the
    float32 (n_noise, stride) device bank, ``lengths`` its int32 lengths.  stats: float64 (batch, 4) rows (Sx, Sn, g, 0)."""
    import torch
    b, c, t = dims_of(x.shape, fmt)
    out = torch.empty_like(x)
    stats = torch.empty((b, 4), dtype=torch.float64, device=x.device)
    ws_bytes = add_noise_workspace_bytes(b, c, t, fmt)
    ws = workspace(ws_bytes, x.device)
    _call("kpr_add_noise_f32", x.device, ptr(x), b, c, t, layout(fmt), ptr(bank), int(bank.shape[0]), int(bank.shape[1]),
          ptr(lengths), ptr(table), ptr(out), ptr(stats), ptr(ws), ws_bytes)
    return out, stats


def add_noise_bwd(gy, x, fmt, bank, lengths, table, stats):
    """(gx, stats_out): the cotangent of ``x`` from the cotangent ``gy`` of ``add_noise(x, ...)[0]`` and the ``stats`` that call
    returned; stats_out: float64 (batch, 4) rows (Sx, Sn, g, D)."""
    import torch
    gy = gy.contiguous().to(torch.float32)
    b, c, t = dims_of(x.shape, fmt)
    gx = torch.empty_like(x)
    stats_out = torch.empty((b, 4), dtype=torch.float64, device=x.device)
    ws_bytes = add_noise_workspace_bytes(b, c, t, fmt)
    ws = workspace(ws_bytes, x.device)
    _call("kpr_add_noise_bwd_f32", x.device, ptr(gy), ptr(x), b, c, t, layout(fmt), ptr(bank), int(bank.shape[0]),
          int(bank.shape[1]), ptr(lengths), ptr(table), ptr(stats), ptr(gx), ptr(stats_out), ptr(ws), ws_bytes)
    return gx, stats_out
