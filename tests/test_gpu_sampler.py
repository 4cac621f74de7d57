"""The ray samplers on every sort route, row length and depth span - needs an MI355X (pytest -m gpu).

lnr_sample_rays_occ / lnr_sample_rays_uniform / lnr_occ_interpolate (loner_amd/csrc/lnr_sampler.hip) against oracle/sampling.py and
oracle/occupancy.py, BIT FOR BIT (np.array_equal, no tolerance anywhere): the sampler's contract is identity with the reference,
sample indices included.  The cases and the route each ray is meant to take come from tests/sampler_restatement.py;
tests/test_sampler_host.py proves on the CPU that they take it.  With them, because they feed the same front end of an iteration:
lnr_compact_rays at its 1024-thread seams against boolean indexing, and the ray builders' keep mask exactly ON its threshold against
oracle/rays.py on inputs whose every sum is exact."""
import numpy as np
import pytest
import torch

from oracle import occupancy as OC
from oracle import rays as OR
from oracle import sampling as SP
from tests import sampler_restatement as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = -7777.0


def dv(x, dtype=torch.float32):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.array(x))                  # (a copy: the shared cases are read-only)
    return x.to(DEV, dtype).contiguous()


@pytest.fixture(scope="module")
def ops():
    from loner_amd import hip
    from loner_amd import ops as _ops
    hip.load()
    return _ops


def _same(stage, got, want, name=""):
    """np.array_equal, and on a difference the first differing ray, column and both values"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, stage, got.shape, want.shape, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~(got == want))
    ray, col = (int(v) for v in bad[0])
    raise AssertionError(f"{name}: stage `{stage}` differs first at ray {ray}, column {col}: kernel {got[ray, col]!r}, oracle {want[ray, col]!r} "
                         f"({len(bad)} of {got.size} entries differ, on rays {sorted(set(bad[:, 0].tolist()))})")


# ------------------------------------------------------------------------------------------- the occupancy sampler
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_occ_sampler_equals_the_oracle_stage_by_stage(ops, name):
    rays, grid, S, perturb, u_jitter, u_pdf = R.build_case(name)
    zo, st = R.oracle_case(name)
    z, dbg = ops.sample_rays_occ(dv(rays), dv(grid), S, perturb, u_jitter=dv(u_jitter), u_pdf=dv(u_pdf), debug=True)
    _same("probs", dbg["probs"], st["probs"], name)        # trilinear lookup of the coarse depths + correctly rounded sigmoid
    _same("cdf", dbg["cdf"], st["cdf"], name)              # cascade row sum, division, float64 running sum
    _same("inds", dbg["inds"], st["inds"], name)           # searchsorted(right=True), planted ties and the draw past cdf[K] included
    _same("z", z, zo, name)                                # inverse cdf + the sort, on the route of each ray
    z2 = ops.sample_rays_occ(dv(rays), dv(grid), S, perturb, u_jitter=dv(u_jitter), u_pdf=dv(u_pdf))
    _same("z without the debug outputs", z2, zo, name)


def test_occ_sampler_same_bytes_on_a_second_call(ops):
    rays, grid, S, perturb, u_jitter, u_pdf = R.build_case("s512_empty")
    args = (dv(rays), dv(grid), S, perturb)
    z1 = ops.sample_rays_occ(*args, u_jitter=dv(u_jitter), u_pdf=dv(u_pdf))
    z2 = ops.sample_rays_occ(*args, u_jitter=dv(u_jitter), u_pdf=dv(u_pdf))
    assert torch.equal(z1.view(torch.int32), z2.view(torch.int32))


@pytest.mark.parametrize("live", [0, 5, 12])
def test_samplers_with_a_device_side_live_count(ops, live):
    """both samplers through the raw binding, z owned by the caller and pre-filled: rows below the device-side count equal the oracle,
    every other row keeps the fill"""
    from loner_amd import hip
    from loner_amd.ops.render import linspace_table
    lib = hip.load()
    rays, grid, S, perturb, u_jitter, u_pdf = R.build_case("s512_reversed")
    n = rays.shape[0]
    assert n == 12
    zo, _ = R.oracle_case("s512_reversed")
    n_dev = torch.tensor([live], device=DEV, dtype=torch.int32)
    d_rays, d_grid, d_u1, d_u2 = dv(rays), dv(grid), dv(u_jitter), dv(u_pdf)
    z = torch.full((n, S), POISON, device=DEV)
    hip.check(lib.lnr_sample_rays_occ(hip._ptr(d_rays), n, hip._ptr(n_dev), hip._ptr(d_grid), grid.shape[0], S, float(perturb),
                                      hip._ptr(linspace_table(S // 2, d_rays.device)), hip._ptr(d_u1), hip._ptr(d_u2), 0, hip._ptr(z), None, None, None,
                                      hip._stream()), "lnr_sample_rays_occ")
    want = np.full((n, S), POISON, np.float32)
    want[:live] = zo[:live]
    _same("z", z, want, f"occupancy sampler, live count {live}")

    u_rays, u = R.uniform_case(64, 1.0)
    d_rays, d_u = dv(u_rays), dv(u)
    z = torch.full((n, 64), POISON, device=DEV)
    hip.check(lib.lnr_sample_rays_uniform(hip._ptr(d_rays), n, hip._ptr(n_dev), 64, 1.0, hip._ptr(linspace_table(64, d_rays.device)), hip._ptr(d_u), 0,
                                          hip._ptr(z), hip._stream()), "lnr_sample_rays_uniform")
    want = np.full((n, 64), POISON, np.float32)
    want[:live] = SP.sample_uniform(u_rays, 64, 1.0, u)[:live]
    _same("z", z, want, f"uniform sampler, live count {live}")


# ------------------------------------------------------------------------------------------- the uniform sampler
@pytest.mark.parametrize("perturb", R.PERTURBS)
@pytest.mark.parametrize("S", R.UNIFORM_SIZES)
def test_uniform_sampler_equals_the_oracle(ops, S, perturb):
    rays, u = R.uniform_case(S, perturb)
    assert (rays[1::3, 12] == 0).all() and (rays[2::3, 12] == rays[2::3, 11]).all()         # reversed and empty spans among the rows
    z = ops.sample_rays_uniform(dv(rays), S, perturb, u_jitter=dv(u))
    _same("z", z, SP.sample_uniform(rays, S, perturb, u), f"uniform S={S} perturb={perturb}")


# ------------------------------------------------------------------------------------------- the occupancy lookup
@pytest.mark.parametrize("V", [1, 2, 24])
def test_occ_interpolate_on_voxel_centres_faces_and_outside(ops, V):
    """the trilinear_zero_pad the sampler calls: voxel centres, the cube's faces / edges / corners at exactly -1 and +1, and points
    outside of which 4, 2, 1 and 0 of the 8 corners remain - with none, exactly 0"""
    grid = np.random.default_rng(V).standard_normal((V, V, V)).astype(np.float32) * np.float32(3.0)
    pts = R.lookup_points(V)
    out = ops.occ_interpolate(dv(grid), dv(pts)).cpu().numpy()
    want = OC.trilinear_lookup_np(grid, pts)
    bad = np.nonzero(~(out == want))[0]
    assert np.array_equal(out, want), (V, pts[bad[:4]].tolist(), out[bad[:4]].tolist(), want[bad[:4]].tolist())
    none_left = R.inside_corners(V, pts) == 0
    assert none_left.any() and (out[none_left] == 0).all()
    assert (out[~none_left] != 0).any()


# ------------------------------------------------------------------------------------------- compaction at the 1024-thread seams
def _compact_case(n, seg, keep, seed):
    gen = torch.Generator().manual_seed(seed)
    rays = torch.randn(n, 13, generator=gen)
    depths = torch.rand(n, generator=gen)
    src = torch.randint(0, 65536, (n,), generator=gen)
    return rays, depths, src, keep.to(torch.uint8), seg


def _compact_cases():
    cases = {}
    for n in (1, 1023, 1024, 1025, 2048):
        gen = torch.Generator().manual_seed(n)
        cases[f"n{n}_random"] = (n, [0, n // 3, n // 3, n], torch.rand(n, generator=gen) > 0.4)
        cases[f"n{n}_all"] = (n, [0, n], torch.ones(n, dtype=torch.bool))
        cases[f"n{n}_none"] = (n, [0, n // 2, n], torch.zeros(n, dtype=torch.bool))
        last = torch.zeros(n, dtype=torch.bool)
        last[-1] = True
        cases[f"n{n}_only_last"] = (n, [0, n // 2, n], last)
    # 64 segments (the most the kernel takes), most of them empty, starts exactly on both seams of a 3000-ray window
    starts = sorted([0] * 9 + [1, 1023] + [1024] * 12 + [1025, 1500] + [2047] * 3 + [2048] * 14 + [2049, 2999] + [3000] * 19 + [700, 701])
    assert len(starts) == 65 and starts[0] == 0 and starts[-1] == 3000
    gen = torch.Generator().manual_seed(64)
    cases["n3000_64_segments"] = (3000, starts, torch.rand(3000, generator=gen) > 0.5)
    cases["n3000_64_segments_none"] = (3000, starts, torch.zeros(3000, dtype=torch.bool))
    return cases


COMPACT = _compact_cases()


@pytest.mark.parametrize("case", list(COMPACT))
def test_compact_rays_at_the_block_seams(ops, case):
    n, seg, k = COMPACT[case]
    rays, depths, src, keep, seg = _compact_case(n, seg, k, len(case) + n)
    r, d, s, out_seg, n_out = ops.compact_rays(dv(rays), dv(depths), keep.to(DEV), src.to(DEV), seg)
    m = int(k.sum())
    assert int(n_out.item()) == m, case
    assert torch.equal(r.cpu()[:m], rays[k]) and torch.equal(d.cpu()[:m], depths[k]) and torch.equal(s.cpu()[:m], src[k]), case
    assert out_seg.cpu().tolist() == [int(k[:b].sum()) for b in seg], case


# ------------------------------------------------------------------------------------------- the keep mask exactly on its threshold
def _oracle_records(c, T, ray_range):
    idx = torch.arange(c["dirs"].shape[1])
    args = (torch.from_numpy(c["dirs"]), torch.from_numpy(c["dist"]), idx, torch.from_numpy(T), torch.tensor(ray_range, dtype=torch.float32),
            torch.tensor(c["scale"]), torch.from_numpy(c["shift"]))
    rays, depths, _ = OR.lidar_ray_records(*args, keep_all=True)
    _, _, keep = OR.lidar_ray_records(*args)
    return rays.numpy(), depths.numpy(), keep.numpy()


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("which", ["range_equal", "range_above"])
def test_ray_builders_keep_mask_at_equality_bit_for_bit(ops, which):
    """scale = 64, ray_range = (1, 2): far_range == near + 1/scale exactly, so a range-limited ray is dropped; at (1, nextafter(2, 3)) it
    is kept; from an origin outside the cube the rays that point away get far == 0 and are dropped.  Signed-permutation rotations and
    Pythagorean directions (components exactly 0 among them) make every sum exact in any order: rays, depths and keep of
    lnr_build_lidar_rays and of lnr_build_window_rays (one segment per pose) equal oracle/rays.py bit for bit."""
    c = R.exact_lidar_case()
    ray_range = c[which]
    n = c["dirs"].shape[1]
    idx = torch.arange(n, device=DEV)
    dirs, dist = dv(c["dirs"]), dv(c["dist"])
    want = [_oracle_records(c, T, ray_range) for T in c["poses"]]
    kept = 0
    for T, (rays_o, depths_o, keep_o) in zip(c["poses"], want):
        rays, depths, keep = ops.build_lidar_rays(dirs, dist, idx, dv(T[:3, :4].reshape(12)), ray_range, c["scale"], c["shift"])
        assert np.array_equal(_bits(rays), _bits(rays_o)) and np.array_equal(_bits(depths), _bits(depths_o))
        assert np.array_equal(keep.cpu().numpy().astype(bool), keep_o)
        inside = abs(float(T[0, 3])) <= 64.0
        if inside:
            assert keep_o.all() if which == "range_above" else not keep_o.any()
        else:
            away = rays_o[:, 3] >= 0
            assert away.any() and (rays_o[away, 12] == 0).all() and not keep_o[away].any()
        kept += int(keep_o.sum())
    assert (kept == 0) == (which == "range_equal")
    # the whole window in one launch: one segment per pose
    p = len(c["poses"])
    tab = ops.WindowTables([dirs] * p, [dist] * p, [0.0] * p, [n] * p, list(range(p)))
    T12 = dv(np.stack([T[:3, :4].reshape(12) for T in c["poses"]]))
    rays, depths, keep, src = ops.build_window_rays(tab, T12, ray_range, c["scale"], c["shift"], index=idx.repeat(p))
    assert np.array_equal(_bits(rays), _bits(np.concatenate([w[0] for w in want])))
    assert np.array_equal(_bits(depths), _bits(np.concatenate([w[1] for w in want])))
    assert np.array_equal(keep.cpu().numpy().astype(bool), np.concatenate([w[2] for w in want]))
    assert torch.equal(src.cpu(), torch.arange(n).repeat(p))
