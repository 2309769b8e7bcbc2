#!/usr/bin/env python3
"""Generate tests/golden/companding_cases.npz and companding_api.json by running the REAL reference code of the mu-law layers
and of ConcatenateFrequencyMap.

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout (KAPRE_REFERENCE, default /root/reference):

    python tools/make_golden_companding.py [--out DIR]

Like oracle/make_golden.py, the reference's kapre/{backend,signal,time_frequency}.py are imported unmodified on the numpy
stand-ins of oracle/ref_stubs.  The handful of TensorFlow symbols those stand-ins lack for these layers is added HERE, at run
time (oracle/ stays as it is): tf.math.sign / log1p / exp / abs, tf.linspace, tf.tile and K.cast_to_floatx.  As everywhere in
the stand-ins, arithmetic runs in float64: the float32 inputs are handed over as float64 copies and cast_to_floatx keeps
float64, so the stored decoder outputs are the float64 value of the reference's formula -- the better truth for a float32
kernel.  tf.cast(., tf.int32) is numpy's astype (truncation toward zero, as TensorFlow's cast).

The JSON records what a test needs of the reference's API: constructor parameters and defaults, get_config() dicts, the
exception type per bad argument, output dtypes and shapes.
"""
import argparse
import importlib
import inspect
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("KAPRE_REFERENCE", "/root/reference")
GOLDEN = os.path.join(REPO, "tests", "golden")
QS = (2, 16, 256, 1024, 65536)


def load_reference():
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_stubs"))
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import tensorflow as tf
    from tensorflow.keras import backend as K

    tf.math.sign = np.sign
    tf.math.log1p = np.log1p
    tf.math.exp = np.exp
    tf.math.abs = np.abs
    tf.linspace = lambda start, stop, num: np.linspace(start, stop, int(num))
    tf.tile = lambda x, multiples: np.tile(x, [int(m) for m in multiples])
    K.cast_to_floatx = lambda x: np.asarray(x, dtype=np.float64)

    pkg = types.ModuleType("kapre")
    pkg.__path__ = [os.path.join(REF, "kapre")]
    sys.modules["kapre"] = pkg
    return (importlib.import_module("kapre.backend"), importlib.import_module("kapre.signal"),
            importlib.import_module("kapre.time_frequency"))


def signature(cls):
    """[(name, default or '<required>')] of the constructor, without self / **kwargs"""
    out = []
    for p in inspect.signature(cls.__init__).parameters.values():
        if p.name == "self" or p.kind in (p.VAR_KEYWORD, p.VAR_POSITIONAL):
            continue
        out.append([p.name, "<required>" if p.default is p.empty else p.default])
    return out


def error_of(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return type(e).__name__
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    backend, sig, tfq = load_reference()

    speech = np.load(os.path.join(GOLDEN, "speech_test_file.npz"))["audio_data"].astype(np.float32)
    x = np.ascontiguousarray(speech[2000:6000].reshape(2, 2000, 1))
    arrays = {"speech_x": x}
    api = {"quantization_channels": list(QS), "backend": {}, "layers": {}, "errors": {}, "signatures": {}}

    # ---- backend.mu_law_encoding / mu_law_decoding
    for q in QS:
        codes = backend.mu_law_encoding(x.astype(np.float64), quantization_channels=q)
        dec = backend.mu_law_decoding(codes, quantization_channels=q)
        arrays["enc_q%d" % q] = np.asarray(codes)
        arrays["dec_q%d" % q] = np.asarray(dec)
        api["backend"][str(q)] = dict(encode_dtype=str(np.asarray(codes).dtype), decode_dtype=str(np.asarray(dec).dtype),
                                      shape=list(np.shape(codes)), code_min=int(np.min(codes)), code_max=int(np.max(codes)))

    # ---- the layers
    enc = sig.MuLawEncoding(quantization_channels=256, name="enc")
    dec = sig.MuLawDecoding(quantization_channels=256, name="dec")
    y_enc = np.asarray(enc(x.astype(np.float64)))
    y_dec = np.asarray(dec(y_enc))
    assert np.array_equal(y_enc, arrays["enc_q256"]) and np.array_equal(y_dec, arrays["dec_q256"])
    api["layers"]["MuLawEncoding"] = dict(kwargs=dict(quantization_channels=256, name="enc"), config=enc.get_config(),
                                          out_dtype=str(y_enc.dtype), out_shape=list(y_enc.shape))
    api["layers"]["MuLawDecoding"] = dict(kwargs=dict(quantization_channels=256, name="dec"), config=dec.get_config(),
                                          out_dtype=str(y_dec.dtype), out_shape=list(y_dec.shape))

    rng = np.random.default_rng(20240917)
    cfm_cases = {}
    for name, fmt, shape in (("cfm_cl", "channels_last", (2, 7, 5, 3)), ("cfm_cf", "channels_first", (2, 3, 7, 5)),
                             ("cfm_default", "default", (1, 4, 9, 1)), ("cfm_cl_onebin", "channels_last", (2, 3, 1, 2))):
        layer = tfq.ConcatenateFrequencyMap(data_format=fmt, name=name)
        xin = rng.standard_normal(shape).astype(np.float32)
        y = np.asarray(layer(xin))
        arrays[name + "_x"], arrays[name + "_y"] = xin, y
        cfm_cases[name] = dict(kwargs=dict(data_format=fmt, name=name), config=layer.get_config(), out_dtype=str(y.dtype),
                               out_shape=list(y.shape), resolved_data_format=layer.data_format)
    api["layers"]["ConcatenateFrequencyMap"] = cfm_cases

    # ---- constructor signatures and exception types
    for cls in (sig.MuLawEncoding, sig.MuLawDecoding, tfq.ConcatenateFrequencyMap):
        api["signatures"][cls.__name__] = signature(cls)
    api["errors"]["MuLawEncoding"] = [
        dict(kwargs=dict(quantization_channels=q), error=error_of(lambda q=q: sig.MuLawEncoding(quantization_channels=q)))
        for q in (1, 0, -5, 65537, 2, 65536)]
    api["errors"]["MuLawDecoding"] = [
        dict(kwargs=dict(quantization_channels=q), error=error_of(lambda q=q: sig.MuLawDecoding(quantization_channels=q)))
        for q in (1, 0, 65537, 256)]
    api["errors"]["ConcatenateFrequencyMap"] = [
        dict(kwargs=dict(data_format=f), error=error_of(lambda f=f: tfq.ConcatenateFrequencyMap(data_format=f)))
        for f in ("weird", 3, None, "channels_first")]
    api["provenance"] = ("generated by tools/make_golden_companding.py from the reference (kapre 0.4.0) on numpy stand-ins "
                         "for tensorflow, float64 arithmetic")

    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "companding_cases.npz"), **arrays)
    with open(os.path.join(args.out, "companding_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True, default=str)
        f.write("\n")
    print("wrote %d arrays and the API record to %s" % (len(arrays), args.out))


if __name__ == "__main__":
    main()
