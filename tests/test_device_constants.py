"""_ffi.DeviceConstants, the one upload-once cache of the Python layer, and the caches that sit on it: built once however many
threads ask, evicted only where a bound was asked for, and the same tensor object at every later lookup.  No GPU: torch's CPU
device stands in for the device."""
import threading

import numpy as np
import pytest
import torch

import kapre_amd as kapre
from kapre_amd import _ffi, backend

CPU = torch.device('cpu')
WAIT = 10.0                # seconds; every wait below ends long before unless something is broken


def test_two_threads_on_a_cold_key_build_once():
    consts = _ffi.DeviceConstants()
    in_make, release = threading.Event(), threading.Event()
    second_inside = threading.Event()
    calls, got = [], {}

    class SameDevice:
        """names the CPU as the key's device part; get() asks for that name first thing, which is how the test sees it inside"""

        def __str__(self):
            second_inside.set()
            return str(CPU)

    def make():
        calls.append(1)
        in_make.set()
        assert release.wait(WAIT)
        return np.arange(3, dtype=np.float32)

    def ask(name, device):
        got[name] = consts.get('k', device, make)

    first = threading.Thread(target=ask, args=('first', CPU))
    first.start()
    assert in_make.wait(WAIT)                          # the first thread holds the lock, inside make
    second = threading.Thread(target=ask, args=('second', SameDevice()))
    second.start()
    assert second_inside.wait(WAIT)                    # the second is inside get, and the key has no entry yet
    release.set()
    first.join(WAIT)
    second.join(WAIT)
    assert not first.is_alive() and not second.is_alive()
    assert len(calls) == 1 and got['first'] is got['second']
    assert torch.equal(got['first'], torch.arange(3, dtype=torch.float32))


def test_max_entries_evicts_the_oldest_and_no_other():
    consts = _ffi.DeviceConstants(max_entries=2)
    a, b = (consts.get(k, CPU, lambda: np.zeros(1, np.float32)) for k in 'ab')
    c = consts.get('c', CPU, lambda: np.zeros(1, np.float32))
    assert len(consts) == 2
    assert consts.get('b', CPU, lambda: pytest.fail('b was evicted')) is b
    assert consts.get('c', CPU, lambda: pytest.fail('c was evicted')) is c
    assert consts.get('a', CPU, lambda: np.ones(1, np.float32)) is not a          # rebuilt: it was the oldest
    unbounded = _ffi.DeviceConstants()
    kept = [unbounded.get(i, CPU, lambda: np.zeros(1, np.float32)) for i in range(100)]
    assert len(unbounded) == 100 and all(unbounded.get(i, CPU, None) is t for i, t in enumerate(kept))


def test_clear_empties_the_cache():
    consts = _ffi.DeviceConstants()
    t = consts.get('k', CPU, lambda: np.zeros(2, np.float32))
    assert len(consts) == 1
    consts.clear()
    assert len(consts) == 0 and consts.get('k', CPU, lambda: np.zeros(2, np.float32)) is not t


def test_on_new_runs_once_per_upload_and_not_on_a_hit():
    consts = _ffi.DeviceConstants()
    seen = []
    t = consts.get('k', CPU, lambda: np.zeros(2, np.float32), on_new=seen.append)
    assert len(seen) == 1 and seen[0] is t
    assert consts.get('k', CPU, lambda: np.zeros(2, np.float32), on_new=seen.append) is t and len(seen) == 1
    other = consts.get('k', torch.device('meta'), lambda: np.zeros(2, np.float32), on_new=seen.append)   # another device: another upload
    assert len(seen) == 2 and seen[1] is other


def test_a_tuple_comes_back_as_a_tuple_in_the_same_order():
    consts = _ffi.DeviceConstants()
    got = consts.get('k', CPU, lambda: (np.zeros(2, np.float32), np.arange(3, dtype=np.int32)))
    assert isinstance(got, tuple) and [t.dtype for t in got] == [torch.float32, torch.int32]
    assert got[0].shape == (2,) and torch.equal(got[1], torch.arange(3, dtype=torch.int32))
    assert consts.get('k', CPU, None) is got


# ---------------------------------------------------------------- the caches that moved onto it: the same object at every lookup
def test_layer_constants_are_uploaded_once():
    stft = kapre.STFT(n_fft=64, hop_length=16)
    assert stft._window(CPU) is stft._window(CPU) and stft._window(CPU, True) is stft._window(CPU, True)
    assert stft._window(CPU).dtype == torch.float32 and stft._window(CPU, True).dtype == torch.float64
    mfcc = kapre.LogmelToMFCC(n_mfccs=5)
    assert mfcc._matrix(16, CPU) is mfcc._matrix(16, CPU) and tuple(mfcc._matrix(16, CPU).shape) == (16, 5)
    assert mfcc._matrix(12, CPU) is not mfcc._matrix(16, CPU)


def test_a_new_filterbank_gives_a_new_device_copy():
    fb = kapre.ApplyFilterbank('mel', dict(sample_rate=16000, n_freq=33, n_mels=8))
    t = fb._fb_device(CPU)
    assert fb._fb_device(CPU) is t and len(fb._consts) == 1
    fb.filterbank = fb.filterbank * np.float32(2.0)
    assert len(fb._consts) == 0
    t2 = fb._fb_device(CPU)
    assert t2 is not t and fb._fb_device(CPU) is t2
    np.testing.assert_array_equal(t2.numpy(), fb.filterbank)


def test_convolve_and_noise_plans_keep_their_device_copies():
    plan = backend.ConvolvePlan(np.arange(1.0, 6.0))
    for adjoint in (False, True):
        assert plan.table(CPU, adjoint) is plan.table(CPU, adjoint)
    assert plan.table(CPU, False) is not plan.table(CPU, True)
    assert backend.ConvolvePlan(np.arange(1.0, 6.0)).table(CPU) is plan.table(CPU)        # equal responses share the copy
    ones, tail = plan.windows(CPU)
    again = plan.windows(CPU)
    assert again[0] is ones and again[1] is tail
    noise = backend.NoisePlan([np.ones(4), np.ones(7)])
    bank, lengths = noise.device(CPU)
    assert noise.device(CPU)[0] is bank and noise.device(CPU)[1] is lengths
    assert tuple(bank.shape) == (2, 7) and lengths.tolist() == [4, 7]


def test_a_plan_keeps_its_table_when_the_shared_cache_drops_it():
    plan = backend.ConvolvePlan(np.arange(1.0, 4.0))
    t = plan.table(CPU)
    for k in range(40):                                # more constants than the shared cache keeps
        backend._CONVOLVE_CONSTS.get(('filler', k), CPU, lambda: np.zeros(1, np.float32))
    assert len(backend._CONVOLVE_CONSTS) == 32 and plan.table(CPU) is t


def test_resample_plans_reuse_their_tables():
    fwd, adj = _ffi.resample_plans(3, 2, 6, 0.99, CPU)
    fwd2, adj2 = _ffi.resample_plans(3, 2, 6, 0.99, CPU)
    assert fwd2.table is fwd.table and fwd2.first is fwd.first and adj2.table is adj.table and adj2.first is adj.first
    assert isinstance(fwd.table, torch.Tensor) and fwd.table.dtype == torch.float32 and fwd.first.dtype == torch.int32
    for plan, adjoint in ((fwd, False), (adj, True)):
        assert (plan.n_phases, plan.n_taps, plan.step) == _ffi.resample_table_size(3, 2, 6, 0.99, adjoint)
