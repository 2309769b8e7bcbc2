"""AddNoise on the GPU: kpr_add_noise_f32 / kpr_add_noise_bwd_f32 in both forms (streamed and resident, option
``addnoise_variant``) against the float64 model of tests/mix_model.py, the draw against its numpy restatement, the layer, a
captured graph and the chain in front of the fused mel launch.

The bounds are derived, not tuned (one rounding of the gain and one FMA; mix_model.forward_bound / backward_bound):

    |y  - y64|  <= 2^-24 |y64|  + 2^-23 |g64 seg| + 2^-149
    |gx - gx64| <= 2^-24 |gx64| + |x| (2^-23 |coef64| + N 2^-52 g64 sum|gy seg| / Sx) + 2^-149

Every check prints its worst ratio to its bound.  K, the chunk of the streamed form, and the resident limit come from
kpr_add_noise_plan.  Batch 3 unless stated."""
import numpy as np
import pytest

import augment_model as am
import mix_model as mm

pytestmark = pytest.mark.gpu

BATCH = 3
RNG = np.random.default_rng(20264)
CF, CL = "channels_first", "channels_last"
LAYOUTS = ((1, CL), (2, CF), (2, CL), (3, CF), (3, CL))
NOISE_LENGTHS = (1, 3, 5, 37, 4099)
SNRS = np.array([-5.0, 0.0, 20.0], dtype=np.float32)


def to_np(t):
    return t.detach().cpu().numpy()


def to_layout(x_bct, fmt):
    """(b, c, t) -> the layout of ``fmt``, contiguous"""
    return np.array(np.moveaxis(x_bct, 1, 2) if fmt == CL else x_bct, order="C", copy=True)


def from_layout(y, fmt):
    return np.moveaxis(y, 2, 1) if fmt == CL else y


def geometry():
    from kapre_amd import _ffi
    K, _, limit, _ = _ffi.add_noise_plan(1, 1, 1, CL)
    return K, limit


class variant:
    """``with variant(v):`` -- addnoise_variant = v inside, the old value restored on the way out"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from kapre_amd import _ffi
        self.old = _ffi.set_option("addnoise_variant", self.v)

    def __exit__(self, *exc):
        from kapre_amd import _ffi
        _ffi.set_option("addnoise_variant", self.old)


def expected_label(v, n_floats, vec, mode="fwd"):
    _, limit = geometry()
    if v != 1 and n_floats <= limit:
        return "k_mix_res<%d,%s>" % (vec, mode)
    return "k_mix_sums<%d,%s> + k_mix_apply<%d,%s>" % (vec, mode, vec, mode)


def device_bank(noises):
    import torch
    from kapre_amd import backend
    bank, lengths = backend.noise_bank(noises)
    return bank, lengths, torch.from_numpy(bank).cuda(), torch.from_numpy(lengths).cuda()


def device_table(index, offset, snr):
    import torch
    host = np.zeros((len(index), 4), dtype=np.int32)
    host[:, 0], host[:, 1], host[:, 2] = index, offset, np.asarray(snr, dtype=np.float32).view(np.int32)
    return torch.from_numpy(host).cuda()


def run_forward(x_bct, fmt, bank_t, lengths_t, table_t, v, unaligned=False):
    """-> (y (b, c, t), stats (b, 4), launch label) under addnoise_variant ``v``"""
    import torch
    from kapre_amd import _ffi
    xl = to_layout(x_bct, fmt)
    if unaligned:                                   # a view one float past a 16-byte boundary
        buf = torch.zeros(xl.size + 1, dtype=torch.float32).cuda()
        xt = buf[1:].view(xl.shape)
        xt.copy_(torch.from_numpy(xl))
        assert xt.data_ptr() % 16 == 4 and xt.is_contiguous()
    else:
        xt = torch.from_numpy(xl).cuda()
    with variant(v):
        y, stats = _ffi.add_noise(xt, fmt, bank_t, lengths_t, table_t)
        label = _ffi.last_launches()
    return from_layout(to_np(y), fmt), to_np(stats), label


def check_forward(x, y, stats, seg, snr, what):
    """the forward bound and the stats rows; returns the worst ratio to the bound"""
    y64, st64 = mm.forward64(x, seg, snr)
    ratio = float(np.max(np.abs(y.astype(np.float64) - y64) / mm.forward_bound(y64, st64, seg)))
    N = x.shape[1] * x.shape[2]
    for b in range(x.shape[0]):
        for col in (0, 1):
            assert abs(stats[b, col] - st64[b, col]) <= N * 2.0 ** -53 * st64[b, col], (what, b, col, stats[b], st64[b])
        assert abs(stats[b, 2] - st64[b, 2]) <= 2.0 ** -24 * st64[b, 2], (what, b, stats[b], st64[b])
        assert stats[b, 2] == np.float64(np.float32(stats[b, 2])) and stats[b, 3] == 0.0
    assert ratio <= 1.0, (what, ratio)
    return ratio


def time_cases():
    K, _ = geometry()
    return (1, 3, 4, 5, K - 1, K, K + 1, 2 * K + 3)


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("t_case", range(8))
def test_forward_against_the_float64_model(t_case):
    """every T x L x (C, layout), offsets (0, 1, L - 1), snr (-5, 0, 20) and a different noise per item, both forms"""
    T = time_cases()[t_case]
    worst, launches = 0.0, 0
    for C, fmt in LAYOUTS:
        x = RNG.standard_normal((BATCH, C, T)).astype(np.float32)
        for L in NOISE_LENGTHS:
            bank, lengths, bank_t, lengths_t = device_bank(RNG.standard_normal((3, L)))
            index, offset = [2, 0, 1], [0, 1 % L, L - 1]
            seg = mm.segments(bank, lengths, index, offset, T)
            table_t = device_table(index, offset, SNRS)
            for v in (1, 2):
                y, stats, label = run_forward(x, fmt, bank_t, lengths_t, table_t, v)
                vec = 1 if (v != 1 and C * T <= geometry()[1] and (C * T) % 4) else 4
                assert label == expected_label(v, C * T, vec), (label, v, C, T)
                worst = max(worst, check_forward(x, y, stats, seg, SNRS, (T, C, fmt, L, v)))
                launches += 1
    print("T = %d: %d launches, worst |y - y64| / bound = %.4f" % (T, launches, worst))


@pytest.mark.parametrize("t_case", (3, 6))
def test_forward_from_an_unaligned_base(t_case):
    T = time_cases()[t_case]
    worst = 0.0
    for C, fmt in ((1, CL), (2, CL), (3, CF)):
        x = RNG.standard_normal((BATCH, C, T)).astype(np.float32)
        bank, lengths, bank_t, lengths_t = device_bank([RNG.standard_normal(37), RNG.standard_normal(5), RNG.standard_normal(4099)])
        index, offset = [0, 1, 2], [36, 0, 1]
        seg = mm.segments(bank, lengths, index, offset, T)
        table_t = device_table(index, offset, SNRS)
        for v in (1, 2):
            y, stats, label = run_forward(x, fmt, bank_t, lengths_t, table_t, v, unaligned=True)
            assert label == expected_label(v, C * T, 1), label
            worst = max(worst, check_forward(x, y, stats, seg, SNRS, (T, C, fmt, v)))
    print("unaligned base, T = %d: worst |y - y64| / bound = %.4f" % (T, worst))


def test_just_above_the_resident_limit_is_streamed():
    _, limit = geometry()
    bank, lengths, bank_t, lengths_t = device_bank(RNG.standard_normal((3, 4099)))
    index, offset = [2, 0, 1], [0, 1, 4098]
    table_t = device_table(index, offset, SNRS)
    for T in (limit, limit + 1):
        x = RNG.standard_normal((BATCH, 1, T)).astype(np.float32)
        seg = mm.segments(bank, lengths, index, offset, T)
        for v in (0, 2):
            y, stats, label = run_forward(x, CL, bank_t, lengths_t, table_t, v)
            resident = T == limit and v == 2                    # (variant 0 streams a batch of 3: the automatic rule asks for 256 items)
            assert label.startswith("k_mix_res") == resident and ("k_mix_sums" in label) != resident, (T, v, label)
            print("T = %d, variant %d: %s, worst ratio %.4f" % (T, v, label, check_forward(x, y, stats, seg, SNRS, (T, v))))
    # the automatic rule takes the resident form from 256 items on
    from kapre_amd import _ffi
    for b in (255, 256):
        x = RNG.standard_normal((b, 2, 33)).astype(np.float32)
        idx, off, snr = np.arange(b) % 3, np.arange(b) % 4099, np.linspace(-5.0, 20.0, b).astype(np.float32)
        y, stats, label = run_forward(x, CF, bank_t, lengths_t, device_table(idx, off, snr), 0)
        assert label.startswith("k_mix_res") == (b == 256), (b, label)
        assert _ffi.add_noise_plan(b, 2, 33, CF)[3] == (_ffi.ADDNOISE_RESIDENT if b == 256 else _ffi.ADDNOISE_STREAMED)
        check_forward(x, y, stats, mm.segments(bank, lengths, idx, off, 33), snr, ("auto", b))


def test_seams_with_a_unit_impulse():
    """noise = one unit impulse, L = T; one item per seam position in ONE launch: y - x is non-zero exactly at
    (pos - offset) mod L, for every chunk seam of the streamed form, the lane and step seams of the resident form, the first and
    last 16-byte boundaries, and their neighbours"""
    K, limit = geometry()
    T = 2 * K + 8
    assert T <= limit
    pos = 5
    noise = np.zeros(T)
    noise[pos] = 1.0
    spots = sorted(set(p for c in (0, 4, 8, 1024, 4096, K, K + 4096, 2 * K, T - 4, T) for p in range(c - 5, c + 6) if 0 <= p < T))
    offsets = [(pos - p) % T for p in spots]
    bank, lengths, bank_t, lengths_t = device_bank(noise)
    table_t = device_table([0] * len(spots), offsets, np.zeros(len(spots), np.float32))
    for C, fmt in ((1, CL), (2, CL), (2, CF)):
        x = RNG.uniform(0.5, 1.5, (len(spots), C, T)).astype(np.float32)
        for v in (1, 2):
            y, stats, label = run_forward(x, fmt, bank_t, lengths_t, table_t, v)
            assert label == expected_label(v, C * T, 4)
            for i, p in enumerate(spots):
                hit = np.nonzero((y[i] != x[i]).any(axis=0))[0]
                assert hit.tolist() == [p], (C, fmt, v, p, hit[:8])
                assert np.all(y[i][:, p] != x[i][:, p]) and stats[i, 1] == 1.0
    print("%d seam positions x 3 layouts x 2 forms" % len(spots))


def test_zero_energy_leaves_the_item_as_it_is():
    T = 1000
    x = RNG.standard_normal((BATCH, 2, T)).astype(np.float32)
    x[1] = 0.0                                                                # a silent item
    noise = RNG.standard_normal(3000)
    noise[:1500] = 0.0                                                        # a silent stretch: item 0 reads only zeros
    bank, lengths, bank_t, lengths_t = device_bank(noise)
    table_t = device_table([0, 0, 0], [100, 2000, 2000], SNRS)
    for fmt in (CF, CL):
        for v in (1, 2):
            y, stats, _ = run_forward(x, fmt, bank_t, lengths_t, table_t, v)
            assert np.array_equal(y[0], x[0]) and np.array_equal(y[1], x[1]) and not np.array_equal(y[2], x[2])
            assert stats[0, 1] == 0.0 and stats[1, 0] == 0.0 and stats[0, 2] == 0.0 and stats[1, 2] == 0.0 and stats[2, 2] > 0.0
            assert not np.signbit(stats[0, 2]) and not np.signbit(stats[1, 2])


def test_a_nan_stays_in_its_item_and_runs_repeat_their_bits():
    K, _ = geometry()
    T = K + 1
    x = RNG.standard_normal((BATCH, 2, T)).astype(np.float32)
    bank, lengths, bank_t, lengths_t = device_bank(RNG.standard_normal((2, 37)))
    table_t = device_table([0, 1, 0], [3, 36, 0], SNRS)
    bad = x.copy()
    bad[1, 1, K - 3] = np.nan
    inf = x.copy()
    inf[1, 0, 7] = np.inf
    for fmt in (CF, CL):
        for v in (1, 2):
            y, stats, _ = run_forward(x, fmt, bank_t, lengths_t, table_t, v)
            y2, stats2, _ = run_forward(x, fmt, bank_t, lengths_t, table_t, v)
            assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)) and np.array_equal(stats, stats2)      # same inputs, same bits
            for broken in (bad, inf):
                yb, _, _ = run_forward(broken, fmt, bank_t, lengths_t, table_t, v)
                assert np.array_equal(yb[0].view(np.uint32), y[0].view(np.uint32))
                assert np.array_equal(yb[2].view(np.uint32), y[2].view(np.uint32))
                assert not np.isfinite(yb[1]).all()


# ------------------------------------------------------------------ backward
def run_backward(x_bct, gy_bct, fmt, bank_t, lengths_t, table_t, v):
    import torch
    from kapre_amd import _ffi
    xt = torch.from_numpy(to_layout(x_bct, fmt)).cuda()
    gt = torch.from_numpy(to_layout(gy_bct, fmt)).cuda()
    with variant(v):
        _, stats = _ffi.add_noise(xt, fmt, bank_t, lengths_t, table_t)
        gx, stats_out = _ffi.add_noise_bwd(gt, xt, fmt, bank_t, lengths_t, table_t, stats)
        label = _ffi.last_launches()
    return from_layout(to_np(gx), fmt), to_np(stats), to_np(stats_out), label


def check_backward(x, gy, gx, seg, snr, what):
    _, st64 = mm.forward64(x, seg, snr)
    gx64, D, coef = mm.backward64(x, gy, seg, st64)
    ratio = float(np.max(np.abs(gx.astype(np.float64) - gx64) / mm.backward_bound(x, gy, seg, st64, gx64, coef)))
    assert ratio <= 1.0, (what, ratio)
    return ratio, D


@pytest.mark.parametrize("t_case", (3, 6, 7))
def test_backward_against_the_float64_model(t_case):
    T = time_cases()[t_case]
    worst = 0.0
    for C, fmt in LAYOUTS:
        x = RNG.standard_normal((BATCH, C, T)).astype(np.float32)
        gy = RNG.standard_normal((BATCH, C, T)).astype(np.float32)
        for L in (3, 37, 4099):
            bank, lengths, bank_t, lengths_t = device_bank(RNG.standard_normal((3, L)))
            index, offset = [2, 0, 1], [0, 1, L - 1]
            seg = mm.segments(bank, lengths, index, offset, T)
            table_t = device_table(index, offset, SNRS)
            for v in (1, 2):
                gx, stats, stats_out, label = run_backward(x, gy, fmt, bank_t, lengths_t, table_t, v)
                vec = 1 if (v != 1 and C * T <= geometry()[1] and (C * T) % 4) else 4
                assert label == expected_label(v, C * T, vec, "bwd"), label
                ratio, D = check_backward(x, gy, gx, seg, SNRS, (T, C, fmt, L, v))
                worst = max(worst, ratio)
                assert np.array_equal(stats_out[:, :3], stats[:, :3])
                scale = np.array([np.sum(np.abs(gy[b] * seg[b][None, :])) for b in range(BATCH)])
                assert np.all(np.abs(stats_out[:, 3] - D) <= C * T * 2.0 ** -53 * scale)
    print("backward, T = %d: worst |gx - gx64| / bound = %.4f" % (T, worst))


def test_backward_of_a_silent_item_is_the_cotangent():
    T = 700
    x = RNG.standard_normal((BATCH, 2, T)).astype(np.float32)
    x[1] = 0.0
    gy = RNG.standard_normal((BATCH, 2, T)).astype(np.float32)
    bank, lengths, bank_t, lengths_t = device_bank(RNG.standard_normal(37))
    table_t = device_table([0, 0, 0], [0, 1, 2], SNRS)
    for fmt in (CF, CL):
        for v in (1, 2):
            gx, _, _, _ = run_backward(x, gy, fmt, bank_t, lengths_t, table_t, v)
            assert np.array_equal(gx[1], gy[1]) and not np.array_equal(gx[0], gy[0])


@pytest.mark.parametrize("t_case", (3, 6))
@pytest.mark.parametrize("v", (1, 2))
def test_layer_autograd_against_torch_float64(t_case, v):
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, augmentation
    T = time_cases()[t_case]
    noises = [RNG.standard_normal(37), RNG.standard_normal(4099), RNG.standard_normal(5)]
    bank, lengths, _, _ = device_bank(noises)
    for C, fmt in ((1, CL), (2, CF), (3, CL)):
        layer = kapre.AddNoise(noises, snr_db=(-5.0, 20.0), input_data_format=fmt)
        x = RNG.standard_normal((BATCH, C, T)).astype(np.float32)
        r = RNG.standard_normal((BATCH, C, T)).astype(np.float32)
        xg = torch.from_numpy(to_layout(x, fmt)).cuda().requires_grad_(True)
        augmentation.set_seed(77)
        with variant(v):
            y = layer(xg, training=True)
            assert y.grad_fn is not None and _ffi.last_launches() == expected_label(v, C * T, 1 if (v == 2 and (C * T) % 4) else 4)
            (y * torch.from_numpy(to_layout(r, fmt)).cuda()).sum().backward()
        table = to_np(layer.last_draw)
        seg = mm.segments(bank, lengths, table[:, 0], table[:, 1], T)
        snr = table[:, 2].copy().view(np.float32)
        x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        y64 = mm.forward_torch64(x64, torch.from_numpy(seg), torch.from_numpy(snr.astype(np.float64)))
        (y64 * torch.from_numpy(r.astype(np.float64))).sum().backward()
        _, st64 = mm.forward64(x, seg, snr)
        gx64, _, coef = mm.backward64(x, r, seg, st64)
        bound = mm.backward_bound(x, r, seg, st64, gx64, coef)
        assert np.max(np.abs(x64.grad.numpy() - gx64)) <= 1e-12 * np.max(np.abs(gx64))       # the two float64 references agree
        gx = from_layout(to_np(xg.grad), fmt).astype(np.float64)
        ratio = float(np.max(np.abs(gx - x64.grad.numpy()) / bound))
        print("autograd T = %d, C = %d %s, variant %d: worst ratio %.4f" % (T, C, fmt, v, ratio))
        assert ratio <= 1.0
        assert np.max(np.abs(from_layout(to_np(y), fmt) - y64.detach().numpy()) / mm.forward_bound(y64.detach().numpy(), st64, seg)) <= 1.0


# ------------------------------------------------------------------ the draw and the layer
def test_layer_draw_is_its_numpy_restatement():
    import torch
    import kapre_amd as kapre
    from kapre_amd import augmentation
    noises = [RNG.standard_normal(1), RNG.standard_normal(7), RNG.standard_normal(4099)]
    layer = kapre.AddNoise(noises, snr_db=(5.0, 20.0))
    b = 64
    xt = torch.from_numpy(RNG.standard_normal((b, 100, 1)).astype(np.float32)).cuda()
    assert layer(xt) is xt and layer.last_draw is None
    augmentation.set_seed(4242)
    outs = []
    for calls in (0, 1):
        assert am.state_of(augmentation.device_state(xt.device)) == (4242, calls)
        outs.append(layer(xt, training=True))
        got = to_np(layer.last_draw)
        want = mm.noise_draw(4242, calls, b, [1, 7, 4099], 5.0, 20.0)
        assert got.dtype == np.int32 and got.shape == (b, 4)
        assert np.array_equal(got, want), calls                                              # index, offset and snr bits
        assert np.all(got[:, 1] < np.array([1, 7, 4099])[got[:, 0]]) and np.all(got[:, 1] >= 0)
        snr = got[:, 2].copy().view(np.float32)
        assert snr.min() >= 5.0 and snr.max() <= 20.0 and len(set(snr.tolist())) > b // 2
        assert tuple(layer.last_stats.shape) == (b, 4) and layer.last_stats.dtype == torch.float64
    assert not torch.equal(outs[0], outs[1])
    augmentation.set_seed(4242)
    assert torch.equal(layer(xt, training=True), outs[0]) and torch.equal(layer(xt, training=True), outs[1])   # bit for bit
    fixed = kapre.AddNoise(noises, snr_db=12.5)
    fixed(xt, training=True)
    assert np.all(to_np(fixed.last_draw)[:, 2].copy().view(np.float32) == np.float32(12.5))
    achieved = mm.achieved_snr_db(from_layout(to_np(xt), CL), from_layout(to_np(fixed(xt, training=True)), CL))
    assert np.max(np.abs(achieved - 12.5)) < 1e-3
    kapre.check_device()


def test_backend_add_noise_takes_host_and_device_arguments():
    import torch
    from kapre_amd import backend
    noises = [RNG.standard_normal(37), RNG.standard_normal(5)]
    bank, lengths, _, _ = device_bank(noises)
    x = RNG.standard_normal((BATCH, 2, 500)).astype(np.float32)
    index, offset, snr = [1, 0, 1], [4, 36, 0], [3.0, 10.0, -2.0]
    seg = mm.segments(bank, lengths, index, offset, 500)
    for fmt in (CF, CL):
        xt = torch.from_numpy(to_layout(x, fmt)).cuda()
        y_host = backend.add_noise(xt, noises, snr, index=index, offset=offset, data_format=fmt)
        y_dev = backend.add_noise(xt, noises, torch.tensor(snr, dtype=torch.float32).cuda(),
                                  index=torch.tensor(index, dtype=torch.int32).cuda(),
                                  offset=torch.tensor(offset, dtype=torch.int32).cuda(), data_format=fmt)
        assert torch.equal(y_host, y_dev)
        y64, st64 = mm.forward64(x, seg, np.array(snr, np.float32))
        assert np.max(np.abs(from_layout(to_np(y_host), fmt) - y64) / mm.forward_bound(y64, st64, seg)) <= 1.0
    y0 = backend.add_noise(torch.from_numpy(to_layout(x, CL)).cuda(), noises[0], 10.0)            # index, offset default to 0
    seg0 = mm.segments(bank, lengths, [0] * BATCH, [0] * BATCH, 500)
    y64, st64 = mm.forward64(x, seg0, np.full(BATCH, 10.0, np.float32))
    assert np.max(np.abs(from_layout(to_np(y0), CL) - y64) / mm.forward_bound(y64, st64, seg0)) <= 1.0
    # a device table is clamped by the kernels: index 9 reads noise 1, offset 99 its last sample
    far = backend.add_noise(torch.from_numpy(to_layout(x, CL)).cuda(), noises, 10.0, index=torch.full((BATCH,), 9, dtype=torch.int32).cuda(),
                            offset=torch.full((BATCH,), 99, dtype=torch.int32).cuda())
    near = backend.add_noise(torch.from_numpy(to_layout(x, CL)).cuda(), noises, 10.0, index=[1] * BATCH, offset=[4] * BATCH)
    assert torch.equal(far, near)


def test_captured_graph_draws_anew_at_every_replay():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, augmentation
    K, _ = geometry()
    noises = [RNG.standard_normal(37), RNG.standard_normal(4099), RNG.standard_normal(5)]
    bank, lengths, _, _ = device_bank(noises)
    for T, v in ((5000, 2), (2 * K + 3, 0)):                                   # (resident: one launch; streamed: two and the workspace)
        C = 1 if T == 5000 else 3
        old_variant = _ffi.set_option("addnoise_variant", v)                   # read at launch, here: at capture time
        layer = kapre.AddNoise(noises, snr_db=(0.0, 15.0))
        x = RNG.standard_normal((BATCH, C, T)).astype(np.float32)
        xt = torch.from_numpy(to_layout(x, CL)).cuda()
        augmentation.set_seed(99)
        layer(xt, training=True)                                               # warm-up: the device state and the bank exist
        torch.cuda.synchronize()
        state = augmentation.device_state(xt.device)
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        try:
            with torch.cuda.stream(side):
                layer(xt, training=True)
                assert _ffi.last_launches().startswith("k_mix_res" if v == 2 else "k_mix_sums")
                torch.cuda.synchronize()
                seed, calls = am.state_of(state)
                with torch.cuda.graph(graph, stream=side):
                    y = layer(xt, training=True)
        finally:
            _ffi.set_option("addnoise_variant", old_variant)
        torch.cuda.synchronize()
        assert (seed, calls) == (99, 2) and am.state_of(state) == (99, 2)      # capturing runs nothing
        table_t, tables = layer.last_draw, []
        for k in range(2):
            graph.replay()
            torch.cuda.synchronize()
            table = to_np(table_t).copy()
            assert np.array_equal(table, mm.noise_draw(seed, calls + k, BATCH, lengths, 0.0, 15.0)), k
            seg = mm.segments(bank, lengths, table[:, 0], table[:, 1], T)
            y64, st64 = mm.forward64(x, seg, table[:, 2].copy().view(np.float32))
            assert np.max(np.abs(from_layout(to_np(y), CL) - y64) / mm.forward_bound(y64, st64, seg)) <= 1.0, k
            tables.append(table)
        assert not np.array_equal(tables[0], tables[1])
        assert am.state_of(state) == (99, 4)
    kapre.check_device()


def test_chain_in_front_of_the_fused_mel_launch():
    import torch
    import kapre_amd as kapre
    from kapre_amd import _ffi, augmentation, backend
    from kapre_amd.keras_shim import Sequential
    rirs = RNG.standard_normal((4, 300)) * np.exp(-np.arange(300) / 60.0)
    noises = [RNG.standard_normal(4099), RNG.standard_normal(700)]
    reverb, noise = kapre.Reverb(rirs), kapre.AddNoise(noises, snr_db=(5, 20))
    mel = kapre.get_melspectrogram_layer(n_fft=512, hop_length=128, sample_rate=16000, n_mels=40, return_decibel=True)
    model = Sequential([reverb, noise, mel])
    xt = torch.from_numpy(RNG.standard_normal((3, 4096, 1)).astype(np.float32)).cuda()
    augmentation.set_seed(5)
    got = model(xt, training=True)
    wet = backend._convolve_run(xt, reverb._plan, CL, 'full', index=reverb.last_index, out_len=4096)
    bank_t, lengths_t = noise._plan.device(xt.device)
    noisy, _ = _ffi.add_noise(wet, CL, bank_t, lengths_t, noise.last_draw)
    assert not torch.equal(noisy, wet) and torch.equal(got, mel(noisy))              # bit for bit
    seen, real = [], _ffi._call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)

    _ffi._call = spy
    try:
        plain = model(xt)
        launches = _ffi.last_launches()
    finally:
        _ffi._call = real
    # (the fused mel launch does not go through _ffi._call: no other launcher ran, and the log is that of the mel call alone)
    assert seen == [] and "k_mel" in launches and "k_mix" not in launches and "k_spec_fir" not in launches
    assert torch.equal(plain, mel(xt)) and _ffi.last_launches() == launches
    kapre.check_device()
