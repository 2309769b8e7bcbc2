"""CPU tests of the mu-law layers (kapre_amd/signal.py), ConcatenateFrequencyMap (kapre_amd/time_frequency.py) and
install_as_kapre: API parity with the reference as recorded in tests/golden/companding_api.json (written by
tools/make_golden_companding.py from the reference's own classes), static shapes, call-time errors that must come before any
GPU work, persistence, the C ABI table, and the `kapre` import name in a fresh process.  Nothing here touches a GPU."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

import kapre_amd as kapre
from kapre_amd import (ConcatenateFrequencyMap, Input, Magnitude, MuLawDecoding, MuLawEncoding, STFT, Sequential, _ffi,
                       keras_shim)

with open(os.path.join(GOLDEN, 'companding_api.json')) as _f:
    API = json.load(_f)
CLASSES = {'MuLawEncoding': MuLawEncoding, 'MuLawDecoding': MuLawDecoding, 'ConcatenateFrequencyMap': ConcatenateFrequencyMap}
NEW_SYMBOLS = ['kpr_mu_law_encode_f32', 'kpr_mu_law_decode_i32', 'kpr_mu_law_decode_f32', 'kpr_mu_law_decode_bwd_f32',
               'kpr_freq_map_concat_f32', 'kpr_freq_map_concat_bwd_f32']
REFERENCE = os.environ.get('KAPRE_REFERENCE', '/root/reference')


def test_exports():
    assert kapre.MuLawEncoding is kapre.signal.MuLawEncoding and kapre.MuLawDecoding is kapre.signal.MuLawDecoding
    assert kapre.ConcatenateFrequencyMap is kapre.time_frequency.ConcatenateFrequencyMap
    assert {'MuLawEncoding', 'MuLawDecoding', 'ConcatenateFrequencyMap', 'install_as_kapre'} <= set(kapre.__all__)
    assert {'MuLawEncoding', 'MuLawDecoding'} <= set(kapre.signal.__all__)
    assert 'ConcatenateFrequencyMap' in kapre.time_frequency.__all__
    assert callable(kapre.backend.mu_law_encoding) and callable(kapre.backend.mu_law_decoding)
    assert list(inspect.signature(kapre.backend.mu_law_encoding).parameters) == ['signal', 'quantization_channels']
    assert list(inspect.signature(kapre.backend.mu_law_decoding).parameters) == ['signal_mu', 'quantization_channels']


@pytest.mark.parametrize('name', sorted(CLASSES))
def test_constructor_signature_is_the_references(name):
    params = [p for p in inspect.signature(CLASSES[name].__init__).parameters.values()
              if p.name != 'self' and p.kind not in (p.VAR_KEYWORD, p.VAR_POSITIONAL)]
    got = [[p.name, '<required>' if p.default is p.empty else p.default] for p in params]
    assert got == API['signatures'][name]
    assert any(p.kind == p.VAR_KEYWORD for p in inspect.signature(CLASSES[name].__init__).parameters.values())


@pytest.mark.parametrize('name', ['MuLawEncoding', 'MuLawDecoding'])
def test_mu_law_config_and_round_trip(name):
    rec = API['layers'][name]
    layer = CLASSES[name](**rec['kwargs'])
    assert layer.get_config() == rec['config']
    again = CLASSES[name].from_config(layer.get_config())
    assert again.get_config() == rec['config'] and again.quantization_channels == 256
    assert layer.compute_output_shape((None, 2048, 1)) == (None, 2048, 1)
    assert layer.compute_output_shape(tuple(rec['out_shape'])) == tuple(rec['out_shape'])
    assert type(layer).__dict__['_keras_registered_name'] == 'Kapre>' + name


@pytest.mark.parametrize('case', sorted(API['layers']['ConcatenateFrequencyMap']))
def test_concat_config_and_shapes(case):
    rec = API['layers']['ConcatenateFrequencyMap'][case]
    layer = ConcatenateFrequencyMap(**rec['kwargs'])
    assert layer.get_config() == rec['config']                     # the config keeps the ORIGINAL string ('default' stays)
    assert layer.data_format == rec['resolved_data_format'] and layer.data_format_original == rec['kwargs']['data_format']
    again = ConcatenateFrequencyMap.from_config(layer.get_config())
    assert again.get_config() == rec['config'] and again.data_format == layer.data_format
    arrays = np.load(os.path.join(GOLDEN, 'companding_cases.npz'))
    in_shape = arrays[case + '_x'].shape
    assert list(layer.compute_output_shape(in_shape)) == rec['out_shape']
    ch = 3 if layer.data_format == 'channels_last' else 1
    unknown = tuple(None if i in (0, ch) else d for i, d in enumerate(in_shape))
    assert layer.compute_output_shape(unknown) == unknown          # an unknown channel count stays unknown
    assert ConcatenateFrequencyMap.__dict__['_keras_registered_name'] == 'Kapre>ConcatenateFrequencyMap'


@pytest.mark.parametrize('name', sorted(CLASSES))
def test_constructor_exception_types(name):
    errors = {'ValueError': ValueError, 'TypeError': TypeError}
    assert API['errors'][name]
    for rec in API['errors'][name]:
        if rec['error'] is None:
            CLASSES[name](**rec['kwargs'])                          # (the reference's decoder validates nothing)
        else:
            with pytest.raises(errors[rec['error']]):
                CLASSES[name](**rec['kwargs'])
    with pytest.raises(TypeError):
        CLASSES[name](**dict(API['errors'][name][-1]['kwargs'], no_such_argument=1))


def test_call_errors_come_before_any_gpu_work():
    for fmt in ('channels_last', 'channels_first'):
        layer = ConcatenateFrequencyMap(data_format=fmt)
        with pytest.raises(ValueError, match='rank-4'):
            layer(np.zeros((2, 83, 128), np.float32))
        with pytest.raises(ValueError, match='rank-4'):
            layer(np.zeros((2, 83, 128, 1, 1), np.float32))
        with pytest.raises(TypeError, match='float32'):
            layer(np.zeros((2, 83, 128, 1), np.float64))
        with pytest.raises(TypeError, match='float32'):
            layer(np.zeros((2, 83, 128, 1), np.int32))
        import torch
        with pytest.raises(TypeError, match='float32'):
            layer(torch.zeros(2, 83, 128, 1, dtype=torch.complex64))


@pytest.mark.parametrize('ext', ['.keras', '.h5'])
def test_save_load(tmp_path, ext):
    models = {
        'enc': (Sequential([Input(shape=(2048, 1)), MuLawEncoding(256)]), (None, 2048, 1)),
        'dec': (Sequential([Input(shape=(2048, 1)), MuLawDecoding(256)]), (None, 2048, 1)),
        'cfm_default': (Sequential([Input(shape=(83, 128, 2)), ConcatenateFrequencyMap()]), (None, 83, 128, 3)),
        'cfm_cf': (Sequential([Input(shape=(2, 83, 128)), ConcatenateFrequencyMap(data_format='channels_first')]),
                   (None, 3, 83, 128)),
        'chain': (Sequential([STFT(n_fft=1024, hop_length=512, input_shape=(2048, 1)), Magnitude(), ConcatenateFrequencyMap()]),
                  (None, 3, 513, 2)),
    }
    for name, (model, out_shape) in models.items():
        assert model.output_shape == out_shape, name
        path = os.path.join(str(tmp_path), name + ext)
        model.save(path)
        custom = {type(l).__name__: type(l) for l in model.layers}
        for co in (None, custom):
            loaded = keras_shim.load_model(path, custom_objects=co)
            assert [type(l) for l in loaded.layers] == [type(l) for l in model.layers]
            assert [l.get_config() for l in loaded.layers] == [l.get_config() for l in model.layers]
            assert loaded.input_shape == model.input_shape and loaded.output_shape == out_shape


def test_new_symbols_are_in_the_header_and_the_ctypes_table():
    header = open(os.path.join(REPO, 'include', 'kapre_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in _ffi.EXPORTS, name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
        assert _ffi.EXPORTS[name][1][-1] is __import__('ctypes').c_void_p          # the stream comes last
    assert 'KPR_VERSION 120' in header


def _child(code, extra_path=None):
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([p for p in (extra_path, REPO) if p])
    return subprocess.run([sys.executable, '-c', code], env=env, cwd=str(extra_path or REPO), capture_output=True, text=True,
                          timeout=300)


def test_install_as_kapre_in_a_fresh_process(tmp_path):
    code = '''
import sys
import kapre_amd
assert 'kapre' not in sys.modules                      # nothing happens unless it is called
kapre_amd.install_as_kapre()
from kapre import STFT, MuLawEncoding
from kapre.time_frequency import ConcatenateFrequencyMap
from kapre.composed import get_melspectrogram_layer
import kapre, kapre.backend, kapre.signal, kapre.augmentation
assert kapre is kapre_amd and STFT is kapre_amd.STFT and MuLawEncoding is kapre_amd.MuLawEncoding
assert ConcatenateFrequencyMap is kapre_amd.ConcatenateFrequencyMap
assert get_melspectrogram_layer is kapre_amd.composed.get_melspectrogram_layer
assert kapre.backend is kapre_amd.backend and kapre.signal is kapre_amd.signal
assert kapre.augmentation is kapre_amd.augmentation
before = {k: v for k, v in sys.modules.items() if k == 'kapre' or k.startswith('kapre.')}
assert sorted(before) == ['kapre', 'kapre.augmentation', 'kapre.backend', 'kapre.composed', 'kapre.signal',
                          'kapre.time_frequency']
kapre_amd.install_as_kapre()                           # a second call is harmless
assert {k: v for k, v in sys.modules.items() if k == 'kapre' or k.startswith('kapre.')} == before
print('installed')
'''
    r = _child(code, str(tmp_path))
    assert r.returncode == 0 and 'installed' in r.stdout, r.stderr
    # a kapre that can really be found: refuse, and leave sys.modules alone
    fake = tmp_path / 'kapre'
    fake.mkdir()
    (fake / '__init__.py').write_text('REAL = True\n')
    code = '''
import sys
import kapre_amd
try:
    kapre_amd.install_as_kapre()
except RuntimeError as e:
    assert 'kapre' not in sys.modules, sorted(k for k in sys.modules if k.startswith('kapre'))
    print('refused:', e)
else:
    raise SystemExit('no error')
'''
    r = _child(code, str(tmp_path))
    assert r.returncode == 0 and 'refused' in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, 'kapre')), reason='the reference checkout is not on this machine')
def test_fixture_generator_is_reproducible(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'make_golden_companding.py'), '--out', str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want, got = np.load(os.path.join(GOLDEN, 'companding_cases.npz')), np.load(os.path.join(str(tmp_path), 'companding_cases.npz'))
    assert sorted(want.files) == sorted(got.files)
    for k in want.files:
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape, k
        assert want[k].tobytes() == got[k].tobytes(), k
    with open(os.path.join(str(tmp_path), 'companding_api.json')) as f:
        assert json.load(f) == API
