"""The host checks that the waveform families share (kpr_host.h: check_series, check_reach, check_ptrs, grid_of), through the C ABI
of every family that walks a (batch, channels, time) batch one series at a time: YIN, CQT, the two resamplers, LFilter, Frame and
Energy.  Every pointer is fabricated and never dereferenced: each call below is refused, or has nothing to do, before anything is
launched, so no device is needed.  The expected codes are literals, recorded from the library before the families shared these
checks: 0 nothing to do, -1 KPR_E_BADARG, -2 KPR_E_UNSUPPORTED, -4 KPR_E_WORKSPACE.

What differs between the families on purpose (and stays so): YIN and CQT take channels == 0 as an empty call, the others refuse it;
the reach of one series is 2^30 elements (samples x channel stride) for the resamplers and LFilter, 2^31 samples for YIN and CQT,
and Frame / Energy have no such limit, no alignment rule and no overlap rule (their rows hold the sizes, the layout and the NULLs)."""
import ctypes

import pytest

from kapre_amd import _ffi

X, OUT, TAB, FIRST, WS, F0, CMND, CURVE = 0x10000000, 0x20000000, 0x30000000, 0x38000000, 0x40000000, 0x50000000, 0x58000000, 0x60000000
LENGTHS = (ctypes.c_int32 * 1)(64)                   # one CQT bin of 64 taps: one tile of four steps, 4 * 64 float4 = 1024 floats
COEF = (ctypes.c_double * 5)(1.0, -2.0, 1.0, -1.9, 0.95)
LF_LEN = 100000                                      # two series of 100000 samples: LFilter's segmented form, which needs the workspace
LF_WS = 2 * 13 * 32                                  # kpr_lfilter_workspace_bytes(2, 1, 100000): 13 segments of 8192

# name -> (argument names in ABI order, a call that passes every check); "n" is the length on which the reach limit is counted
OPS = {
    "kpr_yin_f32": ("x batch ch n layout sr fl W hop lo hi thr pad_end f0 cmnd curve stream",
                    dict(x=X, batch=1, ch=1, n=9000, layout=0, sr=22050.0, fl=2048, W=1024, hop=512, lo=11, hi=340, thr=0.1, pad_end=0,
                         f0=F0, cmnd=CMND, curve=CURVE, stream=None)),                 # 14 frames: f0 / cmnd 56 bytes, curve 56 * 341
    "kpr_cqt_f32": ("x batch ch n layout lengths K table floats hop center pad_end out_layout mag out stream",
                    dict(x=X, batch=1, ch=1, n=900, layout=0, lengths=LENGTHS, K=1, table=TAB, floats=1024, hop=32, center=0, pad_end=0,
                         out_layout=0, mag=0, out=OUT, stream=None)),                  # 27 frames: out 216 bytes, the table 4096
    "kpr_resample_f32": ("x batch ch n layout table first P taps step out_len out stream",
                         dict(x=X, batch=2, ch=1, n=100, layout=1, table=TAB, first=FIRST, P=2, taps=13, step=1, out_len=200, out=OUT,
                              stream=None)),
    "kpr_resample_direct_f32": ("x batch ch n layout orig new width rolloff adjoint out_len out stream",
                                dict(x=X, batch=2, ch=1, n=100, layout=1, orig=1, new=2, width=6, rolloff=0.99, adjoint=0, out_len=200,
                                     out=OUT, stream=None)),
    "kpr_lfilter_f32": ("x batch ch n layout coef reverse out ws ws_bytes stream",
                        dict(x=X, batch=2, ch=1, n=LF_LEN, layout=1, coef=COEF, reverse=0, out=OUT, ws=WS, ws_bytes=LF_WS, stream=None)),
    "kpr_frame_f32": ("x batch ch n layout fl hop pad_end pad_value out stream",
                      dict(x=X, batch=2, ch=1, n=1000, layout=0, fl=50, hop=25, pad_end=0, pad_value=0.0, out=OUT, stream=None)),
    "kpr_energy_f32": ("x batch ch n layout fl hop pad_end pad_value scale out stream",
                       dict(x=X, batch=2, ch=1, n=1000, layout=0, fl=50, hop=25, pad_end=0, pad_value=0.0, scale=1.0, out=OUT, stream=None)),
}

B30, B31 = 1 << 30, 1 << 31
NOTHING = dict(batch=0)                              # past the limit checks such a call returns 0: nothing to do, nothing launched

# (what changes against the call that passes, the code) per entry point
ROWS = {
    "kpr_yin_f32": [
        (dict(batch=-1), -1), (dict(ch=-1), -1), (dict(n=-1), -1), (dict(layout=2), -1), (dict(ch=0), 0),
        (dict(n=B31), -2), (dict(n=B31 - 1, **NOTHING), 0), (dict(n=B31, ch=2, layout=1), -2), (dict(n=B31 - 1, ch=2, layout=1, **NOTHING), 0),
        (dict(x=None), -1), (dict(f0=None), -1), (dict(cmnd=None), -1),
        (dict(x=X + 2), -1), (dict(f0=F0 + 2), -1), (dict(cmnd=CMND + 1), -1), (dict(curve=CURVE + 2), -1),
        (dict(f0=X + 4), -1), (dict(cmnd=X + 35996), -1), (dict(curve=X + 8), -1),
        (dict(cmnd=F0 + 52), -1), (dict(curve=F0 + 4), -1), (dict(cmnd=CURVE + 56 * 341 - 4), -1),
    ],
    "kpr_cqt_f32": [
        (dict(batch=-1), -1), (dict(ch=-1), -1), (dict(n=-1), -1), (dict(layout=2), -1), (dict(out_layout=2), -1), (dict(ch=0), 0),
        (dict(n=B31), -2), (dict(n=B31 - 1, **NOTHING), 0), (dict(n=B31, ch=2, layout=1), -2), (dict(n=B31 - 1, ch=2, layout=1, **NOTHING), 0),
        (dict(x=None), -1), (dict(table=None), -1), (dict(out=None), -1),
        (dict(x=X + 2), -1), (dict(table=TAB + 8), -1), (dict(out=OUT + 4), -1), (dict(out=OUT + 2, mag=1), -1),
        (dict(out=X + 8), -1), (dict(out=TAB + 4088), -1),
    ],
    "kpr_resample_f32": [
        (dict(batch=-1), -1), (dict(ch=-1), -1), (dict(n=-1), -1), (dict(out_len=-1), -1), (dict(layout=2), -1), (dict(ch=0), -1),
        (dict(n=B30), -2), (dict(n=B30 - 1, out_len=0), 0), (dict(n=B30 >> 1, ch=2), -2), (dict(n=(B30 >> 1) - 1, ch=2, out_len=0), 0),
        (dict(out_len=B30), -2), (dict(n=B30 >> 1, ch=2, layout=0, out_len=0), 0),
        (dict(x=None), -1), (dict(out=None), -1), (dict(table=None), -1), (dict(first=None), -1),
        (dict(x=X + 2), -1), (dict(out=OUT + 1), -1), (dict(table=TAB + 2), -1), (dict(first=FIRST + 3), -1),
        (dict(out=X + 796), -1), (dict(x=OUT + 1596), -1),
    ],
    "kpr_resample_direct_f32": [
        (dict(batch=-1), -1), (dict(ch=-1), -1), (dict(n=-1), -1), (dict(out_len=-1), -1), (dict(layout=2), -1), (dict(ch=0), -1),
        (dict(n=B30), -2), (dict(n=B30 - 1, out_len=0), 0), (dict(n=B30 >> 1, ch=2), -2), (dict(n=(B30 >> 1) - 1, ch=2, out_len=0), 0),
        (dict(out_len=B30), -2), (dict(n=B30 >> 1, ch=2, layout=0, out_len=0), 0),
        (dict(x=None), -1), (dict(out=None), -1), (dict(x=X + 2), -1), (dict(out=OUT + 1), -1),
        (dict(out=X + 796), -1), (dict(x=OUT + 1596), -1),
    ],
    "kpr_lfilter_f32": [
        (dict(batch=-1), -1), (dict(ch=-1), -1), (dict(n=-1), -1), (dict(layout=2), -1), (dict(ch=0), -1),
        (dict(n=B30), -2), (dict(n=B30 - 1, batch=0), 0), (dict(n=B30 >> 1, ch=2), -2), (dict(n=(B30 >> 1) - 1, ch=2, batch=0), 0),
        (dict(n=B30 >> 1, ch=2, layout=0, batch=0), 0),
        (dict(x=None), -1), (dict(out=None), -1), (dict(x=X + 2), -1), (dict(out=OUT + 1), -1),
        (dict(out=X + 8 * LF_LEN - 4), -1), (dict(x=OUT + 4), -1),
        (dict(ws=None), -4), (dict(ws=WS + 4), -4), (dict(ws_bytes=LF_WS - 1), -4),
        (dict(ws=X + 64), -1), (dict(ws=OUT - 8), -1),
    ],
    "kpr_frame_f32": [
        (dict(batch=-1), -1), (dict(ch=-1), -1), (dict(n=-1), -1), (dict(layout=2), -1), (dict(ch=0), -1),
        (dict(n=B30, **NOTHING), 0), (dict(n=B30 >> 1, ch=2, layout=1, **NOTHING), 0),
        (dict(x=None), -1), (dict(out=None), -1),
    ],
    "kpr_energy_f32": [
        (dict(batch=-1), -1), (dict(ch=-1), -1), (dict(n=-1), -1), (dict(layout=2), -1), (dict(ch=0), -1),
        (dict(n=B30, **NOTHING), 0), (dict(n=B30 >> 1, ch=2, layout=1, **NOTHING), 0),
        (dict(x=None), -1), (dict(out=None), -1),
    ],
}


@pytest.mark.parametrize("name", sorted(OPS))
def test_return_codes_of_the_shared_checks(name):
    L = _ffi.lib()
    order, good = OPS[name]
    assert L.kpr_lfilter_workspace_bytes(2, 1, LF_LEN, 1) == LF_WS
    got = [(change, getattr(L, name)(*[{**good, **change}[k] for k in order.split()])) for change, _ in ROWS[name]]
    assert got == ROWS[name]
    # a refusal names its operation or the arguments at fault
    getattr(L, name)(*[{**good, "batch": -1}[k] for k in order.split()])
    assert b"batch" in L.kpr_last_error()
