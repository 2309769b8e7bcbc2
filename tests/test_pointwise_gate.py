"""-m gpu: the forward gate of the stand-alone pointwise layers -- Magnitude, Phase (k_cplx_to_real, k_cplx_to_real_f64) and
MagnitudeToDecibel (k_stats_init + k_db_log<1|4> + k_db_clamp<1|4>, k_db_f64).  The golden and oracle tests meet these kernels at a
few dozen values and tolerances of 1e-4 ... 1e-5; here they run on the case tables of tests/pointwise_model.py, the smallest shape
at which each branch of the launches exists (tests/test_pointwise_model_host.py proves on the CPU that the tables reach every
branch of pointwise_model.BRANCHES and that the checks below tell every one-line mutant of the kernels from the real thing).

Decibel    every case runs twice on one input (pointwise_model.db_input: a palette of 61 magnitudes over 2^-40 .. 2^21 plus 0, -0.0,
           -1, -Inf, a denormal and amin, every item scaled by its own power of two, items inside the dynamic range next to items
           with an active floor, each item's only maximum / only low element moved through the seven places of PLACES):
             run (a)  dynamic_range 1000, no floor: ONE bit pattern per input value wherever it stands (scalar head and tail, the
                      in-flight loop, the remainder loop, every chunk), within to_db_bound of the float64 oracle, values <= amin
                      exactly the bits of amin
             run (b)  the case's dynamic_range: assert_array_equal with max(f, item max - dyn) in float32, f from run (a) -- the
                      kernel's threshold is one float32 subtraction -- and the bound against the oracle
           aligned, with x one float into its buffer (k_db_log<1>, k_db_clamp<4>) and with out one float into its buffer (<1> in
           both passes; kpr_mag_to_db_f32 through _ffi._call exactly as _ffi.mag_to_db calls it, which also lets the test read the
           statistics words).  Three parameter sets, the last with ref_value < amin.
Magnitude  integer components in [-2047, 2047]: the sum of squares is exact whatever is fused, the root is known to the bit;
           random components over 2^+-40: the bits of pointwise_model.mag_fma, sqrt(fma(x, x, fl(y y))) -- on the second and
           third trip of the grid stride too, where the compiler's unrolled body and its remainder loop both run
Phase      float32 np.arctan2 to the bit on the IEEE special cases; PHASE_K_ULP ulp of float64 np.arctan2 elsewhere, signs and all
Every case poisons the output allocation with NaN first, asserts _ffi.last_launches() and calls kapre.check_device().  The last test
asserts that the cases that ran reached every branch outside pointwise_model.EXCLUDED and prints each kernel's worst error as a
fraction of its bound (DESIGN.md 4.8.3 quotes them).
"""
import ctypes

import numpy as np
import pytest
import torch

import kapre_oracle as o
import pointwise_model as m
import kapre_amd as kapre
from kapre_amd import _ffi
from test_signal_gate import poison

pytestmark = pytest.mark.gpu

REACHED = set()
WORST = {}
DB_LABEL = 'k_stats_init + k_db_log + k_db_clamp'
NAN_MESSAGE = ('the reference returns an all-NaN item here (tf.maximum and reduce_max propagate NaN; np.maximum in the oracle does '
               'too); to_db computes fmaxf(v, amin), so the NaN position returns the amin floor and the rest of the item is as '
               'without it -- pinned, INTEGRATION.md "Non-finite values"')


def note(what, frac):
    frac = frac if frac == frac else float('inf')
    WORST[what] = max(WORST.get(what, 0.0), frac)


def device_floats(x, offset):
    """a contiguous float32 device copy of x, `offset` floats past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    d = buf[offset:offset + t.numel()].view(t.shape)
    d.copy_(t)
    assert d.is_contiguous() and d.data_ptr() % 16 == 4 * offset and _ffi.as_device(d, torch.float32) is d
    return d


def run_db(xd, out_offset, ref, amin, dyn):
    """-> (out tensor, statistics words or None)"""
    n, sz = xd.shape
    if out_offset == 0:
        poison(xd.numel())
        out = _ffi.mag_to_db(xd, ref, amin, dyn)
        assert out.data_ptr() % 16 == 0
        stats = None
    else:                                                  # the call of _ffi.mag_to_db, with an output one float into its buffer
        buf = torch.full((xd.numel() + 4,), float('nan'), dtype=torch.float32, device='cuda')
        out = buf[out_offset:out_offset + xd.numel()].view(xd.shape)
        assert out.data_ptr() % 16 == 4 * out_offset
        ws_bytes = int(_ffi.lib().kpr_db_workspace_bytes(n))
        ws = _ffi.workspace(ws_bytes, xd.device)
        db = _ffi.DbParams(1, float(ref), float(amin), float(dyn))
        _ffi._call('kpr_mag_to_db_f32', xd.device, _ffi.ptr(xd), n, sz, ctypes.byref(db), _ffi.ptr(out), _ffi.ptr(ws), ws_bytes)
        stats = ws[:8 * n].view(torch.int32).cpu().numpy().view(np.uint32)
    assert _ffi.last_launches() == DB_LABEL, _ffi.last_launches()
    return out, stats


# ---------------------------------------------------------------------------------------------
# MagnitudeToDecibel, float32
# ---------------------------------------------------------------------------------------------
DB = {c['id']: c for c in m.DB_CASES}


@pytest.mark.parametrize('cid', list(DB))
def test_decibel(cid):
    c = DB[cid]
    n, sz = c['n_items'], c['item_size']
    old = _ffi.set_option('db_chunks', c['forced']) if c['forced'] else None
    try:
        full = None                                         # (fa, fb) of the variant that went through db_checks
        for rnd, variant, params in m.db_runs(c, list(DB).index(cid)):
            xo, oo = m.DB_VARIANTS[variant]
            ref, amin, dyn = params
            x, kinds = m.db_input(c, params, rnd)
            xd = device_floats(x, xo)
            fa_d, stats = run_db(xd, oo, ref, amin, m.DB_DYN_OFF)
            fb_d, _ = run_db(xd, oo, ref, amin, dyn)
            if c.get('big') and full is not None:
                # the large cases: the first variant went through every check; the others must reproduce its bits
                assert torch.equal(fa_d.view(torch.int32), full[0].view(torch.int32)), (cid, variant)
                assert torch.equal(fb_d.view(torch.int32), full[1].view(torch.int32)), (cid, variant)
            else:
                fa, fb = fa_d.cpu().numpy(), fb_d.cpu().numpy()
                fails, wa, wb = m.db_checks(x, fa, fb, params, o.magnitude_to_decibel, stats=stats)
                print('pointwise gate [decibel] %s %s round %d %r: worst error / bound = %.3f (a), %.3f (b)' % (cid, variant, rnd, params, wa, wb))
                note('k_db_log to_db_bound', wa)
                note('k_db_log + k_db_clamp bound after the floor', wb)
                assert not fails, (cid, variant, rnd, params, fails)
                # the items inside the dynamic range took the early return, the others the floor
                active = fa.min(1) < (fa.max(1) - np.float32(dyn)).astype(np.float32)
                assert [bool(a) for a in active] == [kind != 'narrow' and sz > 1 for kind in kinds]
                np.testing.assert_array_equal(fb[~active].view(np.uint32), fa[~active].view(np.uint32))
                full = (fa_d, fb_d)
                if stats is not None:
                    note('statistics words (exact)', 0.0)
            REACHED.update(m.db_branches(c, variant, early_return=sz == 1 or 'narrow' in kinds, floor=sz > 1))
        note('k_db_clamp against max(f, item max - dyn) (exact)', 0.0)
    finally:
        if old is not None:
            _ffi.set_option('db_chunks', old)
    kapre.check_device()


def test_decibel_nonfinite_pins():
    """+Inf makes its whole item +Inf, as the oracle does.  NaN is pinned to what the kernels do (see NAN_MESSAGE): the run equals,
    bit for bit, the run with 0 in the NaN's place.  -Inf and negative values are values under amin, as in the reference."""
    c = m.dbcase(4, 1027)
    ref, amin, dyn = m.DB_PARAMS[0]
    x, _ = m.db_input(c, m.DB_PARAMS[0], 0)
    x[:] = np.abs(np.where(np.isfinite(x), x, 1.0))
    x[2, 5], x[2, 1026] = -np.inf, -3.0
    clean = x.copy()
    clean[1, 700] = 0.0
    x[0, 513] = np.inf
    x[1, 700] = np.nan
    for f64 in (False, True):
        dt = torch.float64 if f64 else torch.float32
        layer = kapre.MagnitudeToDecibel(ref_value=ref, amin=amin, dynamic_range=dyn, dtype='float64' if f64 else 'float32')
        poison(x.size * (2 if f64 else 1))
        got = layer(torch.from_numpy(x).cuda().to(dt))
        assert _ffi.last_launches() == ('k_db_f64' if f64 else DB_LABEL)
        got = got.cpu().numpy()
        ref_run = layer(torch.from_numpy(clean).cuda().to(dt)).cpu().numpy()
        with np.errstate(all='ignore'):
            want = o.magnitude_to_decibel(x.astype(np.float64), ref, amin, dyn)
        assert np.isposinf(want[0]).all() and np.isposinf(got[0]).all()
        assert np.isnan(want[1]).all(), 'the oracle no longer propagates NaN'
        assert not np.isnan(got).any(), NAN_MESSAGE
        np.testing.assert_array_equal(got[1:], ref_run[1:], err_msg=NAN_MESSAGE)
        assert got[1, 700] == ref_run[1, 700] == ref_run[1].max() - dyn, NAN_MESSAGE      # the amin floor, raised to the item's floor
        # -Inf and negative input: the oracle's own values (np.maximum(x, amin) = amin), at the tolerance of the bound / of float64
        tol = 1e-11 if f64 else float(m.to_db_bound(x[2:], amin, ref).max() + m.U32 * np.abs(want[2:]).max())
        assert float(np.abs(got[2:] - want[2:]).max()) <= tol
    kapre.check_device()


# ---------------------------------------------------------------------------------------------
# MagnitudeToDecibel, float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('item_size', m.DB_F64_SIZES)
def test_decibel_float64(item_size):
    """k_db_f64 is one 1024-thread workgroup per item: items of 1, 1023, 1024, 1025 and 8193 values, the method of runs (a) / (b)"""
    c = m.dbcase(3, item_size)
    for rnd, (ref, amin, dyn) in enumerate(m.DB_PARAMS):
        x, _ = m.db_input(c, (ref, amin, dyn), rnd)
        xd = torch.from_numpy(x.astype(np.float64)).cuda()
        runs = []
        for d in (m.DB_DYN_OFF, dyn):
            poison(2 * x.size)
            got = kapre.MagnitudeToDecibel(ref_value=ref, amin=amin, dynamic_range=d, dtype='float64')(xd)
            assert _ffi.last_launches() == 'k_db_f64' and got.dtype == torch.float64
            runs.append(got.cpu().numpy())
        fa, fb = runs
        assert not np.isnan(fa).any()
        xb, fab = x.reshape(-1).view(np.uint32), fa.reshape(-1).view(np.uint64)
        order = np.argsort(xb, kind='stable')
        assert not ((xb[order][1:] == xb[order][:-1]) & (fab[order][1:] != fab[order][:-1])).any()
        under = fa[~(x.astype(np.float64) > amin)]
        assert under.size == 0 or (under == under[0]).all()
        ea = float(np.abs(fa - o.magnitude_to_decibel(x.astype(np.float64), ref, amin, m.DB_DYN_OFF)).max())
        np.testing.assert_array_equal(fb, np.maximum(fa, fa.max(1)[:, None] - dyn))
        eb = float(np.abs(fb - o.magnitude_to_decibel(x.astype(np.float64), ref, amin, dyn)).max())
        print('pointwise gate [decibel f64] item %d %r: max error %.3g (a), %.3g (b)' % (item_size, (ref, amin, dyn), ea, eb))
        note('k_db_f64 1e-11', max(ea, eb) / 1e-11)
        assert ea <= 1e-11 and eb <= 1e-11
    kapre.check_device()
    REACHED.update(m.db_f64_branches(item_size))


# ---------------------------------------------------------------------------------------------
# Magnitude
# ---------------------------------------------------------------------------------------------
def device_complex(re, im, misaligned=False):
    zn = np.empty(re.size, np.complex64)                   # (re + 1j * im would lose the sign of a zero and turn Inf into NaN)
    zn.real, zn.imag = re, im
    z = torch.from_numpy(zn)
    if not misaligned:
        d = z.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(z.numel() + 1, dtype=torch.complex64, device='cuda')
    d = buf[1:]
    d.copy_(z)
    assert d.data_ptr() % 16 == 8 and d.is_contiguous()
    return d


def run_c2r(layer, zd, label='k_cplx_to_real'):
    poison(zd.numel() * (2 if zd.dtype == torch.complex128 else 1))
    got = layer(zd)
    assert _ffi.last_launches() == (label if zd.numel() else ''), _ffi.last_launches()
    assert got.shape == zd.shape
    return got.cpu().numpy()


def check_magnitude(n, misaligned=False):
    rng = np.random.default_rng(n + 1)
    re, im = (rng.integers(-2047, 2048, n).astype(np.float32) for _ in range(2))
    got = run_c2r(kapre.Magnitude(), device_complex(re, im, misaligned))
    np.testing.assert_array_equal(got.view(np.uint32), np.sqrt((re * re + im * im).astype(np.float32)).view(np.uint32))
    note('k_cplx_to_real magnitude, integer components (exact)', 0.0)
    re, im = ((2.0 ** rng.uniform(-40, 40, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(2))
    if n > 8:
        im[: n // 2] = (re[: n // 2] * 2.0 ** rng.uniform(-3, 3, n // 2)).astype(np.float32)       # comparable squares
    got = run_c2r(kapre.Magnitude(), device_complex(re, im, misaligned))
    want = m.mag_fma(re, im)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, ('%d of %d elements are not sqrt(fma(x, x, fl(y y))), first at %d (trip %d of the grid stride)'
                           % (bad.size, n, bad[0], m.c2r_trips(n)[bad[0]]))
    note('k_cplx_to_real magnitude, bits of mag_fma (exact)', 0.0)
    kapre.check_device()
    REACHED.update(m.c2r_branches(n, misaligned=misaligned))


@pytest.mark.parametrize('n', m.C2R_SIZES)
def test_magnitude(n):
    check_magnitude(n)


@pytest.mark.parametrize('n', m.C2R_STRIDE_SIZES)
def test_magnitude_past_the_grid_cap(n):
    """4096 blocks of 256 threads: a second and a third element per thread.  The compiler unrolls the grid-stride loop by two, so
    the third trip runs the remainder loop after one pass of the unrolled body -- the same value must get the same bits in both"""
    check_magnitude(n)


def test_magnitude_misaligned_base():
    check_magnitude(257, misaligned=True)


def test_magnitude_out_of_range_pins():
    """documented domain: components between about 1e-19 and 1.8e19 in magnitude, or zero.  sqrtf(x^2 + y^2)
    overflows above it and underflows below it, which tf.abs does not: pinned, not promised"""
    re = np.float32([1e20, 0.0, -1e20, 1e-30, 0.0, 1e-30, 1.8e19, 1e-19])
    im = np.float32([0.0, 1e20, 1e20, 0.0, 1e-30, 1e-30, 0.0, 0.0])
    got = run_c2r(kapre.Magnitude(), device_complex(re, im))
    assert np.isposinf(got[:3]).all()
    np.testing.assert_array_equal(got[3:6], np.float32([0.0, 0.0, 0.0]))
    np.testing.assert_array_equal(got.view(np.uint32), m.mag_fma(re, im).view(np.uint32))
    np.testing.assert_allclose(got[6:], [1.8e19, 1e-19], rtol=2e-7)
    kapre.check_device()


def test_magnitude_and_phase_complex128():
    rng = np.random.default_rng(128)
    n = 257
    z = (2.0 ** rng.uniform(-40, 40, n)) * np.exp(1j * rng.uniform(-np.pi, np.pi, n))
    zd = torch.from_numpy(z).cuda()
    got = run_c2r(kapre.Magnitude(dtype='float64'), zd, 'k_cplx_to_real_f64')
    assert got.dtype == np.float64
    err = float(np.abs(got / np.abs(z) - 1).max())
    note('k_cplx_to_real_f64 magnitude 1e-15', err / 1e-15)
    assert err <= 1e-15
    got = run_c2r(kapre.Phase(dtype='float64'), zd, 'k_cplx_to_real_f64')
    err = float(np.abs(got - np.angle(z)).max())
    note('k_cplx_to_real_f64 phase 1e-15', err / 1e-15)
    assert err <= 1e-15
    kapre.check_device()
    REACHED.update(m.c2r_branches(n, f64=True) | m.c2r_branches(n, phase=True, f64=True))


# ---------------------------------------------------------------------------------------------
# Phase
# ---------------------------------------------------------------------------------------------
def test_phase_special_cases_to_the_bit():
    """atan2(+-0, +-0), (+-0, +-x), (+-y, +-0), (+-Inf, finite), (finite, +-Inf), (+-Inf, +-Inf): the signed zeros and the
    multiples of pi / 4 of IEEE 754 / C Annex F, which float32 np.arctan2 returns; NaN in either component gives NaN"""
    re, im = m.phase_special_inputs()
    got = run_c2r(kapre.Phase(), device_complex(re, im))
    want = np.arctan2(im, re)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, [(float(im[i]), float(re[i]), float(got[i]), float(want[i])) for i in bad]
    re = np.float32([np.nan, 1.0, np.nan, np.nan, 0.0])
    im = np.float32([1.0, np.nan, np.nan, np.inf, np.nan])
    assert np.isnan(run_c2r(kapre.Phase(), device_complex(re, im))).all()
    note('k_cplx_to_real phase, IEEE special cases (exact)', 0.0)
    kapre.check_device()
    REACHED.update(m.c2r_branches(re.size, phase=True))


@pytest.mark.parametrize('n', [0, 63, 257])
def test_phase_sizes(n):
    re, im = m.phase_inputs(seed=n, n=n)
    got = run_c2r(kapre.Phase(), device_complex(re, im))
    if n:
        assert float(m.ulp_error(got, np.arctan2(im.astype(np.float64), re.astype(np.float64))).max()) <= m.PHASE_K_ULP
    REACHED.update(m.c2r_branches(n, phase=True))


def test_phase_within_k_ulp_of_float64_arctan2():
    """all four quadrants, |im / re| from 2^-40 to 2^40, a tenth of the points hugging an axis; compared directly (no modulo) and
    with signs.  K = 6 ulp is the OpenCL full-profile limit for atan2, which the ROCm device library is written to; it is not a
    derived bound.  tests/test_pointwise_model_host.py measures float32 np.arctan2 against the same reference."""
    re, im = m.phase_inputs()
    got = run_c2r(kapre.Phase(), device_complex(re, im))
    want = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    assert (np.sign(got) == np.sign(want)).all()
    ulps = m.ulp_error(got, want)
    worst = float(ulps.max())
    ref = float(m.ulp_error(np.arctan2(im, re), want).max())
    print('pointwise gate [phase] worst error %.3f ulp of float64 arctan2 (bound %d; float32 np.arctan2 itself: %.3f ulp)' % (worst, m.PHASE_K_ULP, ref))
    note('k_cplx_to_real phase %d ulp' % m.PHASE_K_ULP, worst / m.PHASE_K_ULP)
    assert worst <= m.PHASE_K_ULP, (worst, float(re[ulps.argmax()]), float(im[ulps.argmax()]))
    kapre.check_device()
    REACHED.update(m.c2r_branches(re.size, phase=True))


# ---------------------------------------------------------------------------------------------
# what this file reached
# ---------------------------------------------------------------------------------------------
def test_every_branch_was_reached():
    """runs last: the union of the branch ids of the cases above is BRANCHES minus the declared exclusions"""
    if not REACHED:
        pytest.skip('the cases above did not run in this session')
    print('pointwise gate worst error / bound:')
    for what in sorted(WORST):
        print('  %-60s %.4f' % (what, WORST[what]))
    want = set(m.BRANCHES) - set(m.EXCLUDED)
    assert REACHED == want, (sorted(want - REACHED), sorted(REACHED - want))
