"""tests/encode_restatement.py - the reference of tests/test_gpu_encode.py - checked on the CPU: against oracle/network.py, against
central differences of its own forward, its integer record formats against their documented error, and the crafted inputs of the
GPU test against what they claim to be."""
import numpy as np
import pytest
import torch

from oracle import loss as OL
from oracle import network as NW
from oracle import render as RD
from tests import encode_restatement as ER
from tests.conftest import load_golden
from tests.test_gpu_kernels import NETS

F32, F64 = torch.float32, torch.float64
ALL_DENSE = dict(otype="HashGrid", n_levels=2, n_features_per_level=2, log2_hashmap_size=19, base_resolution=4, per_level_scale=2.0)
HASH_NETS = {k: v[0] for k, v in NETS.items() if v[0]["otype"] == "HashGrid"}
HASH_NETS["all_dense"] = ALL_DENSE


def _oracle(enc):
    return NW.NetworkSpec.from_config(enc, dict(activation="ReLU", n_neurons=16, n_hidden_layers=1))


def _table(grid, seed, gain=3000.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(grid.n_entries * grid.n_features, generator=gen) * 2 - 1) * 1e-4 * gain


def _points(grid, seed, n=400):
    """random points inside the cube, the crafted ones, and the cube's faces (all with cells >= 0)"""
    gen = torch.Generator().manual_seed(seed)
    crafted, _ = ER.crafted_points(grid, seed, outside=False)
    return torch.cat([torch.rand(n, 3, generator=gen) * 1.98 - 0.99, crafted])


# ------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name", list(HASH_NETS))
def test_grid_geometry_and_float32_features_equal_the_oracle(name):
    enc = HASH_NETS[name]
    grid, spec = ER.make_grid(enc), _oracle(enc)
    assert [(lv.scale, lv.res, lv.size, lv.offset, lv.hashed) for lv in grid.levels] == \
           [(lv.scale, lv.res, lv.size, lv.offset, lv.hashed) for lv in spec.levels]
    table, p = _table(grid, 1), _points(grid, 2)
    ours = torch.cat(ER.encode(grid, table, p, F32)["feat"], dim=1)
    ref = NW.encode_hashgrid(spec, table.reshape(-1, grid.n_features), (p + 1) / 2)
    assert torch.equal(ours, ref)
    # beyond the far faces cells stay non-negative; below the near faces they wrap as unsigned 32-bit numbers, which the oracle's
    # hashed levels do too (its dense-indexed levels use signed cells there: excluded, see encode_restatement's docstring)
    gen = torch.Generator().manual_seed(3)
    far = torch.rand(64, 3, generator=gen) * 0.4 + 0.95
    near = -far
    F = grid.n_features
    o_far, r_far = torch.cat(ER.encode(grid, table, far, F32)["feat"], dim=1), NW.encode_hashgrid(spec, table.reshape(-1, F), (far + 1) / 2)
    o_near, r_near = torch.cat(ER.encode(grid, table, near, F32)["feat"], dim=1), NW.encode_hashgrid(spec, table.reshape(-1, F), (near + 1) / 2)
    assert torch.equal(o_far, r_far)
    for l, lv in enumerate(grid.levels):
        if lv.hashed:
            assert torch.equal(o_near[:, l * F:(l + 1) * F], r_near[:, l * F:(l + 1) * F]), l


@pytest.mark.parametrize("name", ["default", "hash_f4_2hidden", "hash_f1", "hash_f8", "all_dense"])
def test_float64_gradients_equal_autograd_through_the_oracle(name):
    """Per level: the oracle evaluated in float64 at the unit coordinate whose float64 position IS the float32-defined position, on
    the points where both then floor to the same cell; its autograd against level_table_grad / level_input_grad."""
    enc = HASH_NETS[name]
    grid, spec = ER.make_grid(enc), _oracle(enc)
    F = grid.n_features
    table, p = _table(grid, 4).double(), _points(grid, 5, 300)
    gen = torch.Generator().manual_seed(6)
    d_feat = torch.randn(p.shape[0], len(grid.levels) * F, generator=gen, dtype=F64)
    compared = 0
    for l, lv in enumerate(grid.levels):
        cell, frac = ER.locate(lv, p)
        x64 = ((cell.double() + frac.double()) - 0.5) / lv.scale
        same = (torch.floor(x64 * lv.scale + 0.5).long() == cell).all(dim=1)
        assert float(same.double().mean()) > 0.95
        cell, frac, x64, g = cell[same], frac[same].double(), x64[same].clone().requires_grad_(True), d_feat[same, l * F:(l + 1) * F]
        tab = table.clone().requires_grad_(True)
        feat = NW.encode_hashgrid(spec, tab.reshape(-1, F), x64)[:, l * F:(l + 1) * F]
        (feat * g).sum().backward()
        entries = ER.corner_entries(lv, cell)
        tab_l = ER.table_of(grid, table, l)
        tg, A, cnt = ER.level_table_grad(lv, F, entries, frac, g)
        ref_t = ER.table_of(grid, tab.grad, l)
        # (the oracle's fraction is that of a float64 position recomputed from x64: 2^-53 of a position of up to 2^19)
        assert float((tg - ref_t).abs().max()) <= 1e-9 * float(ref_t.abs().max())
        dp = ER.level_input_grad(lv, tab_l, entries, frac, g)
        assert float((dp - 0.5 * x64.grad).abs().max()) <= 1e-9 * float(x64.grad.abs().max())
        assert float((ER.level_features(lv, tab_l, entries, frac) - feat.detach()).abs().max()) <= 1e-9 * float(feat.detach().abs().max())
        assert bool((A >= tg.abs() - 1e-12).all()) and float(cnt.sum()) == float((ER.corner_weights(frac)[:, :, None] * g[:, None, :] != 0).sum())
        compared += int(same.sum())
    assert compared > 0


@pytest.mark.parametrize("name", ["default", "hash_f1"])
def test_float64_input_gradient_equals_central_differences_inside_a_cell(name):
    grid = ER.make_grid(HASH_NETS[name])
    F = grid.n_features
    table = _table(grid, 7).double()
    gen = torch.Generator().manual_seed(8)
    p = torch.rand(200, 3, generator=gen) * 1.9 - 0.95
    for l, lv in enumerate(grid.levels):
        cell, frac = ER.locate(lv, p)
        inner = ((frac > 0.01) & (frac < 0.99)).all(dim=1)
        cell, frac = cell[inner], frac[inner].double()
        entries, tab_l = ER.corner_entries(lv, cell), ER.table_of(grid, table, l)
        g = torch.randn(frac.shape[0], F, generator=gen, dtype=F64)
        dp = ER.level_input_grad(lv, tab_l, entries, frac, g)
        h = 1e-4                                                   # in cells; the function is trilinear inside a cell: no truncation error
        for axis in range(3):
            step = torch.zeros(3, dtype=F64); step[axis] = h
            hi = (ER.level_features(lv, tab_l, entries, frac + step) * g).sum(dim=1)
            lo = (ER.level_features(lv, tab_l, entries, frac - step) * g).sum(dim=1)
            # d/d(world) = d/d(fraction) * scale / 2
            fd = (hi - lo) / (2 * h) * lv.scale * 0.5
            assert float((fd - dp[:, axis]).abs().max()) <= 1e-9 * float(dp.abs().max()), (l, axis)


# ------------------------------------------------------------------------------------------- the record formats
def _value_cases():
    rng = np.random.default_rng(0)
    mag = np.exp2(rng.uniform(-126, 127, 20000)).astype(np.float32) * rng.choice([-1.0, 1.0], 20000).astype(np.float32)
    below_pow2 = (np.exp2(np.arange(-100, 100, dtype=np.float64)) * (1 - 2.0 ** -24)).astype(np.float32)     # one ulp below a power of two
    carry = ER.u2f(np.array([0x3F7FFFDF, 0x3F7FFFE0, 0x3F7FFFFF, 0x407FFFE0, 0x7F7FFFDF], np.uint32))          # around the rounding carry
    ties = ER.u2f(np.array([0x3F800020, 0x3F800060, 0x3F8000A0], np.uint32))                                     # exactly between two 26-bit values
    denormal = ER.u2f(np.array([1, 0x20, 0x3F, 0x40, 0x7FFFFF, 0x800000], np.uint32))
    zero = np.array([0.0, -0.0], np.float32)
    return np.concatenate([mag, below_pow2, -below_pow2, carry, -carry, ties, denormal, -denormal, zero])


def test_pack26_round_trip_error_and_ties():
    v = _value_cases()
    back = ER.unpack26(ER.pack26(v))
    normal = np.abs(v) >= np.float32(2.0 ** -126)
    err = np.abs(back.astype(np.float64) - v.astype(np.float64))
    assert np.all(err[normal] <= 2.0 ** -18 * np.abs(v[normal].astype(np.float64)))
    assert np.all(err[~normal] <= 2.0 ** -144)                                        # denormals: half of the kept grid's 2^-143 step
    assert np.all(np.signbit(back) == np.signbit(v)) and np.all(back[v == 0] == 0)
    assert np.all((ER.f2u(back) & 0x3F) == 0)
    # the carry into the next binade is the correct rounding, and ties go to the even 26-bit value
    assert ER.unpack26(ER.pack26(np.float32(1 - 2.0 ** -24))) == np.float32(1.0)
    assert list(ER.f2u(ER.unpack26(ER.pack26(ER.u2f(np.array([0x3F800020, 0x3F800060], np.uint32)))))) == [0x3F800000, 0x3F800080]


def test_pair_record_round_trip():
    v = _value_cases()
    rng = np.random.default_rng(1)
    w = rng.permutation(v)
    idx = rng.integers(0, 4096, v.shape[0]).astype(np.uint32)
    lo, hi = ER.pack_pair(idx, v, w)
    i2, v0, v1 = ER.unpack_pair(lo, hi)
    assert np.array_equal(i2, idx)
    assert np.array_equal(ER.f2u(v0), ER.f2u(ER.unpack26(ER.pack26(v)))) and np.array_equal(ER.f2u(v1), ER.f2u(ER.unpack26(ER.pack26(w))))


def _fx_cases():
    rng = np.random.default_rng(2)
    top = ER.u2f(np.arange(0x3F7FFFE0, 0x3F800000, dtype=np.uint32))                 # the 32 largest floats below 1
    return np.concatenate([rng.uniform(0, 1, 20000).astype(np.float32), np.exp2(rng.uniform(-40, 0, 5000)).astype(np.float32),
                           np.array([0.0, 0.5, 2.0 ** -149, 2.0 ** -126], np.float32), top])


def test_xpair_record_round_trip_and_the_fx_carry():
    fx = _fx_cases()
    rng = np.random.default_rng(3)
    v = _value_cases()
    a0, a1 = rng.choice(v, fx.shape[0]), rng.choice(v, fx.shape[0])
    idx, t = rng.integers(0, 4096, fx.shape[0]).astype(np.uint32), rng.integers(0, 12, fx.shape[0]).astype(np.uint32)
    i2, t2, b0, b1, fx2 = ER.unpack_xpair(*ER.pack_xpair(idx, t, a0, a1, fx))
    assert np.array_equal(i2, idx) and np.array_equal(t2, t)
    assert np.array_equal(ER.f2u(b0), ER.f2u(ER.unpack26(ER.pack26(a0)))) and np.array_equal(ER.f2u(b1), ER.f2u(ER.unpack26(ER.pack26(a1))))
    assert np.all(np.abs(fx2.astype(np.float64) - fx.astype(np.float64)) <= 2.0 ** -20)
    assert np.all(np.abs(fx2.astype(np.float64) - fx.astype(np.float64)) <= 2.0 ** -20 * fx.astype(np.float64) + 2.0 ** -149)   # relative, too
    assert np.all(fx2 <= 1.0) and fx2[fx == 0][0] == 0.0
    # fractions from 1 - 2^-21 up carry to exactly 1.0: the x corner gets weight 0 and the x + 1 corner all of a
    carried = fx >= np.float32(1 - 2.0 ** -21)
    assert carried.sum() == 8 and np.all(fx2[carried] == 1.0) and np.all(fx2[~carried] < 1.0)
    q = ER.xpair_fix(b0[carried], b1[carried], fx2[carried])
    assert np.all(q[0] == 0) and np.all(q[1] == 0)
    assert np.array_equal(q[2], ER.to_fix(b0[carried])) and np.array_equal(q[3], ER.to_fix(b1[carried]))


def test_fixed_point_conversions_agree_below_256_and_what_happens_above():
    """The fast conversion (an fp64 fma that leaves the integer in the mantissa) equals the generic one wherever the code uses it,
    |v| < 256 - and in fact up to |v| <= 512, where 1.5 * 2^52 + v * 2^42 leaves [2^52, 2^53) and the mantissa trick returns another
    number.  The generic branch is exact (v * 2^42 is a float32 again, and an integer from |v| >= 2^-19 on) until it saturates at
    |v| >= 2^21: a single contribution of 2.1e6 - or a sum beyond it - ends at +-2^63 / 2^42."""
    rng = np.random.default_rng(4)
    v = np.concatenate([_value_cases(), rng.uniform(-256, 256, 20000).astype(np.float32),
                        ER.u2f(np.array([0x437FFFFF, 0xC37FFFFF], np.uint32))])             # the largest floats below 256
    v = v[np.abs(v) < 256]
    assert np.array_equal(ER.to_fix_small(v), ER.to_fix_generic(v))
    exact = np.rint(v.astype(np.float64) * 2.0 ** 42)
    assert np.array_equal(ER.to_fix(v).astype(np.float64), exact)                            # (|q| < 2^50: exact as float64)
    assert np.all(np.abs(ER.to_fix(v).astype(np.float64) * 2.0 ** -42 - v.astype(np.float64)) <= 2.0 ** -43)
    mid = np.array([256.0, 300.5, 511.99997, 512.0, -256.0, -512.0], np.float32)
    assert np.array_equal(ER.to_fix_small(mid), ER.to_fix_generic(mid))
    beyond = np.array([512.00006, 513.0, 1000.0, -512.00006, -4096.0], np.float32)
    assert not np.any(ER.to_fix_small(beyond) == ER.to_fix_generic(beyond))
    big = np.array([256.0, 1e3, -65536.5, 2.0 ** 20, -(2.0 ** 21 - 0.25)], np.float32)
    assert np.array_equal(ER.to_fix(big).astype(np.float64), big.astype(np.float64) * 2.0 ** 42)
    assert ER.to_fix(np.float32(2.0 ** 21)) >= 2 ** 63 - 1024 and ER.to_fix(np.float32(-3e6)) == -2 ** 63
    # an x-pair takes the generic branch as soon as ONE of its values reaches 256, for all four products
    q = ER.xpair_fix(np.float32(300.0), np.float32(0.125), np.float32(0.25))
    assert [int(x) for x in q] == [int(225.0 * 2 ** 42), int(0.09375 * 2 ** 42), int(75.0 * 2 ** 42), int(0.03125 * 2 ** 42)]


# ------------------------------------------------------------------------------------------- the crafted inputs
def test_crafted_points_reach_every_trailing_ones_class_and_straddle_owner_slices():
    grid = ER.make_grid(HASH_NETS["default"])
    kinds = [(not lv.hashed, lv.hashed and not ER.uses_xpairs(grid, l), ER.uses_xpairs(grid, l)) for l, lv in enumerate(grid.levels)]
    assert [sum(k[i] for k in kinds) for i in range(3)] == [3, 5, 8]                 # dense-indexed, hashed pair-record, x-pair levels
    p, notes = ER.crafted_points(grid, 0)
    hit, straddles = set(), 0
    for row, l, what in notes:
        if l < 0:
            continue
        lv = grid.levels[l]
        cell, frac = ER.locate(lv, p[row:row + 1])
        t = ER.trailing_ones(int(cell[0, 0]))
        if what.startswith("t="):
            assert t == int(what[2:]), (row, l, what, t)
            assert 0.0 < float(frac[0, 0]) < 1.0
            hit.add((l, ER.t_class(t)))
            if t >= 12:                                                # e(x + 1) = e(x) ^ (2^(t+1) - 1): another 8192-float owner slice
                e = ER.corner_entries(lv, cell)[0]
                for k in (0, 2, 4, 6):
                    f0, f1 = (lv.offset + int(e[k])) * 2, (lv.offset + int(e[k + 1])) * 2
                    assert f0 // ER.SLICE_FLOATS != f1 // ER.SLICE_FLOATS and (int(e[k]) ^ int(e[k + 1])) == ((2 << t) - 1) & (lv.size - 1)
                    straddles += 1
        if what == "fx=0":
            assert float(frac[0, 0]) == 0.0
    assert straddles > 0
    for l, lv in enumerate(grid.levels):
        if lv.res > 4096:
            bits = lv.res.bit_length() - 1
            want = {ER.t_class(t) for t in (0, 5, 11, 12, 13, 15, bits) if t <= bits}
            assert want <= {c for (ll, c) in hit if ll == l}, (l, want)
            assert sum(1 for (_, ll, what) in notes if ll == l and what == "fx=0") >= 1
    # cells around x = 0: the fraction there has more significant bits than a record's fx keeps, and the x corner's weight is small
    low = [(row, l) for row, l, what in notes if what == "low"]
    inexact = 0
    for row, l in low:
        cell, frac = ER.locate(grid.levels[l], p[row:row + 1])
        assert -17 <= int(cell[0, 0]) <= 16
        fx = frac[0, 0].numpy()
        inexact += int(ER.unpack_fx(ER.pack_fx(fx)) != fx and 1.0 - float(fx) < 1.0 / 16)
    assert inexact >= 8
    # Fractions within 2^-21 of 1 need a position below 8.  A float32 world coordinate gives a unit coordinate m 2^-25, and at scale
    # 2^k - 1 the position m 2^(k-25) + 1/2 - m 2^-25 lies just below an integer only for m = 2^(24-k) x odd: the fraction is then
    # 1 - odd x 2^-(k+1), 1 - 2^-20 at best on the finest level (k = 19) - it does not carry (the carry itself is tested on the
    # record restatement above)
    near_one = [float(ER.locate(grid.levels[l], p[row:row + 1])[1][0, 0]) for row, l, what in notes if what == "fx->1"]
    assert len(near_one) >= 8 and max(near_one) >= 1 - 2.0 ** -10 and max(near_one) < 1 - 2.0 ** -21
    # faces and outside points: every face has points exactly on it and beyond it
    faces = p[[row for row, l, what in notes if what == "face"]]
    outside = p[[row for row, l, what in notes if what == "outside"]]
    for axis in range(3):
        for side in (-1.0, 1.0):
            assert int((faces[:, axis] == side).sum()) >= 6 and int((outside[:, axis] * side > 1.0).sum()) >= 6
    assert float(outside.abs().max()) <= 1.35 + 1e-6


def test_the_magnitude_sweep_has_x_pairs_with_one_value_on_either_side_of_256():
    """case e of the GPU test: with W1[0, j] = 2^-(j mod 8) the two features of a level receive d_sigma c and d_sigma c / 2, so
    a0 = wy wz g0 and a1 = a0 / 2 straddle 256 whenever 256 <= |a0| < 512"""
    grid = ER.make_grid(HASH_NETS["default"])
    p, _ = ER.crafted_points(grid, 0)
    d_sigma = ER.sweep_d_sigma(p.shape[0])
    coeff = ER.all_level_coefficients(len(grid.levels) * 2)
    split = 0
    for k in ER.SWEEP_EXPONENTS:
        for l, lv in enumerate(grid.levels):
            if not ER.uses_xpairs(grid, l):
                continue
            _, frac = ER.locate(lv, p)
            for wy in (frac[:, 1], 1 - frac[:, 1]):
                for wz in (frac[:, 2], 1 - frac[:, 2]):
                    a0 = (wy * wz * (d_sigma * 2.0 ** k * coeff[2 * l])).abs()
                    split += int(((a0 >= 256) & (a0 * 0.5 < 256)).sum())
    assert split > 0
    assert min(ER.SWEEP_EXPONENTS) == -40 and max(ER.SWEEP_EXPONENTS) == 14


def test_bunched_depths_share_cells_below_scale_3000():
    grid = ER.make_grid(HASH_NETS["default"])
    for S in (64, 100, 128):
        rays, z, live = ER.bunched_rays(S)
        assert rays.shape[0] == 8 and live < 8
        p = ER.world_points(rays, z).reshape(-1, 3)
        for l, lv in enumerate(grid.levels):
            if lv.scale >= ER.COMBINE_SCALE_MAX:
                continue
            cell, _ = ER.locate(lv, p)
            same = (cell[1:] == cell[:-1]).all(dim=1)               # sample m shares its cell with sample m - 1
            m = torch.arange(1, p.shape[0])
            assert int(same.sum()) >= 8 * 20
            inside_row = same & (m % 16 != 0)
            across_row = same & (m % 16 == 0) & (m % 64 != 0)
            across_wave = same & (m % 64 == 0) & (m % 512 != 0)
            across_batch = same & (m % 512 == 0)
            assert bool(inside_row.any()) and bool(across_row.any()), (S, l)
            if S != 64:
                assert bool(across_wave.any()) and bool(across_batch.any()), (S, l)
            # a run that ends with its ray: the last samples of a ray share a cell and the next ray starts elsewhere
            last = torch.arange(1, 8) * S
            assert bool((same[last - 2] & ~same[last - 1]).any()), (S, l)


# ------------------------------------------------------------------------------------------- where real gradients sit
def test_d_sigma_of_the_fused_loss_fixture_against_the_fixed_point_floor():
    """The table gradient is summed in fixed point at 2^-42.  A contribution w d_feature is resolved to 2^-17 of itself (the budget of
    a 26-bit record) as long as it is at least 2^-25 = 3e-8.  This prints where the d_sigma of the reference's loss (fixture G8:
    192 rays x 128 samples, loss terms as in cfg/model_config) lies relative to that, for DESIGN.md 4.3."""
    g = load_golden("g8_compute_loss")
    enc = {k: (int(v) if v.isdigit() else v) for k, v in zip(g["enc_keys"], g["enc_vals"])}
    net = dict(activation="ReLU", n_neurons=32, n_hidden_layers=1)
    spec = NW.NetworkSpec.from_config(enc, net)
    rays, z, depths = torch.from_numpy(g["rays"]), torch.from_numpy(g["z"]), torch.from_numpy(g["depths"])
    xyz = RD.sample_points(rays, z)
    sigma = NW.density(spec, torch.from_numpy(g["params"]), xyz.reshape(-1, 3)).reshape(z.shape).detach().requires_grad_(True)
    out = RD.composite(sigma, z, rays[:, 3:6], rays[:, -1:], torch.from_numpy(g["noise"]))
    loss, _ = OL.lidar_loss(out, z, rays, depths, float(g["scale"][0]), OL.LossConfig())
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-4 * float(g["loss"])
    d = torch.autograd.grad(loss, sigma)[0].abs().reshape(-1)
    live = d[d > 0]
    qs = torch.quantile(live.double(), torch.tensor([0.01, 0.1, 0.5, 0.9, 1.0], dtype=F64))
    floor = 2.0 ** -25
    below = float((live < floor).double().mean())
    print(f"FIGURES fused-loss d_sigma (G8): {live.numel()} of {d.numel()} non-zero; |d_sigma| quantiles 1% {qs[0]:.2e} 10% {qs[1]:.2e} "
          f"50% {qs[2]:.2e} 90% {qs[3]:.2e} max {qs[4]:.2e}; below 2^-25 = {floor:.2e}: {100 * below:.1f} %")
    assert float(qs[4]) > floor
