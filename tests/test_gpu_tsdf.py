"""TSDF fusion on the GPU against the fp64 restatement (tests/tsdf_restatement.py): the integration's sum and count byte for byte,
the field and the masked marching cubes byte for byte, and the whole chain on simulated scans of the box room."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from loner_amd.utils import synthetic as SYN
from loner_amd.utils import synthetic_mesh as SM
from tests import tsdf_restatement as TR

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _empty(dims):
    """(sum, count) of an empty volume on the device"""
    return torch.zeros(dims, dtype=torch.int64, device=DEV), torch.zeros(dims, dtype=torch.int32, device=DEV).view(torch.uint32)


def _host(sum_, count):
    return sum_.cpu().numpy(), count.view(torch.int32).cpu().numpy().view(np.uint32)


def _integrate(rays, ranges, dims, origin, v, trunc, front, volume=None):
    from loner_amd import ops
    sum_, count = _empty(dims) if volume is None else volume
    info = ops.tsdf_integrate(_t(rays).reshape(-1, 6), _t(ranges).reshape(-1), sum_, count, origin, v, trunc, front)
    return sum_, count, info.cpu().numpy().tolist()


def _assert_same_volume(got, want, what):
    for name, g, w in zip(("sum", "count"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype} {g.shape}, want {w.dtype} {w.shape}"
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {name} differs on {len(bad)} of {g.size} nodes, first {bad[:5].tolist()}: got "
                                 f"{g[tuple(bad[0])]}, want {w[tuple(bad[0])]}")


@functools.lru_cache(maxsize=None)
def _table():
    from loner_amd import ops
    return ops.mc_case_table()


# ---------------------------------------------------------------- integration
GRID = ((9, 7, 5), (-1.0, -0.75, -0.5), 0.25)


@functools.lru_cache(maxsize=None)
def _grid_rays():
    """the ray set of tests/test_tsdf_host.py and rays the call must count and leave out"""
    dims, origin, v = GRID
    rays, ranges = TR.ray_set(dims, origin, v, 11)
    extra, extra_r = [], []
    good = [0.1, 0.05, 0.02, 0.6, 0.64, 0.48]
    for k in range(6):
        for bad in (math.nan, math.inf):
            ray = list(good)
            ray[k] = bad
            extra.append(ray); extra_r.append(1.0)
    extra.append([math.nan] * 6); extra_r.append(1.0)                   # what lnr_trajectory_rays writes outside its trajectory
    extra.append(good[:3] + [0.0, 0.0, 0.0]); extra_r.append(1.0)
    for r in (0.0, -0.5, math.nan, math.inf, -math.inf):
        extra.append(list(good)); extra_r.append(r)
    extra.append([5.0, 0.0, 0.0, 1.0, 0.0, 0.0]); extra_r.append(1.0)   # misses: starts behind the box, ends before it, passes beside it
    extra.append([-9.0, 0.0, 0.0, 1.0, 0.0, 0.0]); extra_r.append(1.0)
    extra.append([-9.0, 3.0, 0.0, 1.0, 0.0, 0.0]); extra_r.append(9.0)
    return np.concatenate([rays, np.asarray(extra)]), np.concatenate([ranges, np.asarray(extra_r)]), len(extra)


@pytest.mark.parametrize("carve", [False, True])
def test_integration_bit_for_bit(carve):
    dims, origin, v = GRID
    rays, ranges, n_extra = _grid_rays()
    trunc = 3 * v
    front = math.inf if carve else trunc
    want_sum, want_count, want_info = TR.integrate(rays, ranges, dims, origin, v, trunc, front)
    sum_, count, info = _integrate(rays, ranges, dims, origin, v, trunc, front)
    print(f"carve {carve}: {len(rays)} rays, info {info}, {int((want_count > 0).sum())} of {want_count.size} nodes written")
    assert info == want_info
    assert info[0] == 0 and info[2] == 12 + 1 + 1 + 5 and info[3] >= 3 + 5 and info[4] == int(want_count.sum()) and info[5:] == [0, 0, 0]
    assert info[1] + info[2] + info[3] <= len(rays) and info[1] >= 200
    _assert_same_volume(_host(sum_, count), (want_sum, want_count), f"carve {carve}")
    # a second call adds to the first: the same rays again double every word
    _integrate(rays, ranges, dims, origin, v, trunc, front, (sum_, count))
    _assert_same_volume(_host(sum_, count), (2 * want_sum, 2 * want_count), f"carve {carve}, twice")


def test_many_copies_of_one_ray_land_on_the_same_nodes():
    dims, origin, v = GRID
    ray, r, trunc = np.array([-1.3, -0.6, -0.4, 0.6, 0.48, 0.64]), 1.7, 0.75
    one_sum, one_count, _ = TR.integrate(ray[None], [r], dims, origin, v, trunc, math.inf)
    assert int(one_count.sum()) >= 8 and one_count.max() == 1
    n = 4096
    sum_, count, info = _integrate(np.tile(ray, (n, 1)), np.full(n, r), dims, origin, v, trunc, math.inf)
    assert info[:5] == [0, n, 0, 0, n * int(one_count.sum())]
    _assert_same_volume(_host(sum_, count), (n * one_sum, (n * one_count).astype(np.uint32)), "4096 copies")


def test_result_does_not_depend_on_the_run_or_on_the_order_of_the_rays():
    """70 000 rays: 274 workgroups of 256, more than the 256 compute units hold in one round of one workgroup each"""
    dims, origin, v = (33, 17, 9), (-4.0, -2.0, -1.0), 0.25
    rng = np.random.default_rng(21)
    n = 70000
    lo, size = np.asarray(origin) - 0.5 * v, np.asarray(dims) * v
    o = lo + rng.uniform(-0.2, 1.2, (n, 3)) * size
    d = lo + rng.uniform(0.0, 1.0, (n, 3)) * size - o
    length = np.linalg.norm(d, axis=1)
    rays = np.concatenate([o, d / length[:, None]], axis=1)
    ranges = length * rng.uniform(0.5, 1.2, n)
    first = _host(*_integrate(rays, ranges, dims, origin, v, 0.75, math.inf)[:2])
    second_sum, second_count, info = _integrate(rays, ranges, dims, origin, v, 0.75, math.inf)
    order = rng.permutation(n)
    third = _host(*_integrate(rays[order], ranges[order], dims, origin, v, 0.75, math.inf)[:2])
    # more than 700 000 updates on 5049 nodes: every node takes more than a hundred atomics on average, from many waves
    assert info[1] > 60000 and info[4] > 10 * n and int(first[1].sum()) == info[4]
    _assert_same_volume(_host(second_sum, second_count), first, "second run")
    _assert_same_volume(third, first, "permuted rays")
    # and in two halves
    halves = _empty(dims)
    _integrate(rays[: n // 2], ranges[: n // 2], dims, origin, v, 0.75, math.inf, halves)
    _integrate(rays[n // 2:], ranges[n // 2:], dims, origin, v, 0.75, math.inf, halves)
    _assert_same_volume(_host(*halves), first, "two calls")


# ---------------------------------------------------------------- field and masked marching cubes
def _mc_block_nodes():
    text = open(os.path.join(ROOT, "loner_amd", "csrc", "lnr_mesh.hip")).read()
    block, per_lane = (int(re.search(rf"#define {name} (\d+)", text).group(1)) for name in ("MC_BLOCK", "MC_PER_LANE"))
    return block * per_lane


SHAPES = [(2, 2, 2), (3, 2, 2), (5, 4, 3), (17, 9, 6), (33, 17, 9)]


def test_the_largest_shape_spans_more_than_one_marching_cubes_block():
    assert np.prod(SHAPES[-1]) > _mc_block_nodes() >= 1024


@pytest.mark.parametrize("shape", SHAPES)
def test_field_bit_for_bit(shape):
    from loner_amd import ops
    rng = np.random.default_rng(sum(shape))
    count = rng.integers(0, 5, shape).astype(np.uint32)
    count[rng.uniform(size=shape) < 0.1] = rng.integers(1 << 20, 1 << 32, dtype=np.uint64)       # large counts too
    sum_ = rng.integers(-(1 << 20), (1 << 20) + 1, shape) * count.astype(np.int64)               # |mean| <= 1 ...
    sum_ += rng.integers(-3, 4, shape) * (count > 0)                                             # ... give or take
    sum_[count == 0] = 0
    for min_count in (1, 3):
        want_f, want_v = TR.field(sum_, count, min_count)
        f, valid = ops.tsdf_field(_t(sum_, np.int64), _t(count.view(np.int32), np.int32).view(torch.uint32), min_count)
        got_f, got_v = f.cpu().numpy(), valid.cpu().numpy()
        assert got_f.dtype == np.float32 and got_v.dtype == np.uint8
        assert got_f.tobytes() == want_f.tobytes(), f"field differs on {int((got_f != want_f).sum())} nodes"
        assert got_v.tobytes() == want_v.tobytes()


@pytest.mark.parametrize("shape", SHAPES)
def test_masked_marching_cubes_bit_for_bit(shape):
    from loner_amd import ops
    rng = np.random.default_rng(7 + sum(shape))
    vol = rng.normal(size=shape).astype(np.float32)
    sp, org = (0.25, 0.5, 0.125), (-1.0, 2.0, 0.5)
    dvol = _t(vol, np.float32)
    for p_valid in (1.0, 0.9, 0.5):
        valid = (rng.uniform(size=shape) < p_valid).astype(np.uint8)
        want_v, want_f = TR.marching_cubes_masked(vol, valid, 0.1, _table(), sp, org)
        verts, faces = ops.marching_cubes(dvol, 0.1, sp, org, valid=_t(valid, np.uint8))
        got_v, got_f = verts.cpu().numpy(), faces.cpu().numpy()
        print(f"{shape}, {p_valid:.0%} valid: {got_v.shape[0]} vertices, {got_f.shape[0]} triangles")
        assert got_v.dtype == np.float32 and got_f.dtype == np.int32
        assert got_v.shape == want_v.shape and got_f.shape == want_f.shape
        assert got_v.tobytes() == want_v.tobytes() and got_f.tobytes() == want_f.tobytes()
        if p_valid == 1.0:
            plain_v, plain_f = ops.marching_cubes(dvol, 0.1, sp, org)
            assert got_v.tobytes() == plain_v.cpu().numpy().tobytes() and got_f.tobytes() == plain_f.cpu().numpy().tobytes()
            assert got_f.shape[0] > 0
            bool_v, bool_f = ops.marching_cubes(dvol, 0.1, sp, org, valid=_t(valid, np.uint8).bool())
            assert torch.equal(bool_v, verts) and torch.equal(bool_f, faces)


def test_masked_marching_cubes_refuses_a_wrong_mask():
    from loner_amd import ops
    vol = torch.zeros(3, 3, 3, device=DEV)
    with pytest.raises(ValueError):
        ops.marching_cubes(vol, valid=torch.ones(3, 3, 2, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.marching_cubes(vol, valid=torch.ones(3, 3, 3, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.marching_cubes(vol, valid=torch.ones(3, 3, 3, dtype=torch.uint8))


# ---------------------------------------------------------------- end to end
V_ROOM = 0.2


def _tum_rows():
    """five poses, 0.1 s apart, walking and turning through the middle of the room"""
    rows = []
    for k in range(5):
        h = math.radians(12.0) * k / 2.0
        rows.append([0.1 * k, -3.0 + 1.5 * k, 1.0 - 0.5 * k, 1.0 + 0.1 * k, 0.0, 0.0, math.sin(h), math.cos(h)])
    return np.asarray(rows)


@functools.lru_cache(maxsize=None)
def _room():
    """-> (scene, scans, trajectory, volume, stats): three simulated scans of the box room fused along their trajectory"""
    from loner_amd.analysis import lidar_sim
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.analysis.raycast import RaycastingScene
    from loner_amd.analysis.tsdf import fuse_scans
    scene = RaycastingScene(*SM.box_room_mesh(), device=DEV)
    traj = load_trajectory(_tum_rows(), DEV)
    dirs, times = SYN.lidar_pattern(16, 128)
    scans = [lidar_sim.simulate_scan(scene, traj, dirs, times, stamp, (1.0, 50.0), range_sigma=0.0)[0] for stamp in (0.0, 0.1, 0.2)]
    bound = (np.asarray(SYN.BOX_MIN) - 1.0, np.asarray(SYN.BOX_MAX) + 1.0)
    stats = {}
    volume = fuse_scans(scans, _tum_rows(), bound, V_ROOM, device=DEV, stats=stats)
    return scene, scans, traj, volume, stats


def test_fused_room_bit_for_bit_and_near_the_walls():
    from loner_amd import ops
    scene, scans, traj, volume, stats = _room()
    assert volume.dims == (211, 161, 51) and volume.sdf_trunc == 3 * V_ROOM and volume.front == volume.sdf_trunc
    assert stats["scans"] == 3 and stats["skipped_scans"] == 0 and stats["invalid_rays"] == 0
    assert stats["rays"] == sum(len(s) for s in scans) == volume.n_rays and stats["updated_rays"] > 0.9 * stats["rays"]
    want_sum, want_count = np.zeros(volume.dims, dtype=np.int64), np.zeros(volume.dims, dtype=np.uint32)
    for scan in scans:
        rays, _ = ops.trajectory_rays(scan.ray_directions, scan.timestamps.double(), traj)
        TR.integrate(rays.cpu().numpy(), scan.distances.double().cpu().numpy(), volume.dims, volume.origin, V_ROOM, volume.sdf_trunc,
                     volume.front, want_sum, want_count)
    _assert_same_volume(_host(volume.sum, volume.count), (want_sum, want_count), "fused room")
    assert int(want_count.sum()) == stats["node_updates"]
    mesh = volume.extract_mesh()
    want = TR.extract_mesh(want_sum, want_count, volume.origin, V_ROOM, _table())
    assert mesh is not None and want is not None
    assert mesh.vertices.dtype == np.float64 and mesh.triangles.dtype == np.int32
    assert mesh.vertices.tobytes() == want[0].tobytes() and mesh.triangles.tobytes() == want[1].tobytes()
    # (16 x 128 rays are sparse at 0.2 m in a 40 m room: only near the sensor do all eight corners of a cell get a ray)
    assert mesh.triangles.shape[0] > 0
    # An inside node (field > 0) has a ray through its voxel with -trunc <= s < 0: the node is within sqrt(trunc^2 + 0.75 v^2) of that
    # ray's hit point on the room, and a vertex is within v of an inside node: trunc + 1.87 v bounds the sum.
    dist = scene.compute_distance(torch.from_numpy(mesh.vertices).to(DEV))
    print(f"fused room: {mesh.vertices.shape[0]} vertices, {mesh.triangles.shape[0]} triangles, max distance to the room "
          f"{float(dist.max()):.4f} m, mean {float(dist.mean()):.4f} m (bound {volume.sdf_trunc + 1.87 * V_ROOM:.4f} m)")
    assert float(dist.max()) <= volume.sdf_trunc + 1.87 * V_ROOM
    # the filters: a higher min_count and a component filter only take away
    fewer = volume.extract_mesh(min_count=2, min_component_triangles=20)
    assert fewer is None or 0 < fewer.triangles.shape[0] <= mesh.triangles.shape[0]


def test_constant_trajectory_is_the_pose():
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.analysis.tsdf import TSDFVolume
    from loner_amd.common.pose_utils import quat_to_matrix
    _, scans, _, room, _ = _room()
    h = 0.4
    row = [0.0, 1.0, -2.0, 0.5, 0.0, 0.0, math.sin(h / 2), math.cos(h / 2)]
    rows = np.asarray([row, [1.0] + row[1:]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = quat_to_matrix(rows[:1, 4:])[0], rows[0, 1:4]
    lo, hi = np.asarray(room.origin), np.asarray(room.origin) + (np.asarray(room.dims) - 1) * V_ROOM
    by_pose = TSDFVolume(lo, hi, V_ROOM, device=DEV)
    by_traj = TSDFVolume(lo, hi, V_ROOM, device=DEV)
    assert by_pose.dims == room.dims
    a = by_pose.integrate_scan(scans[0], pose=torch.from_numpy(T))
    b = by_traj.integrate_scan(scans[0], trajectory=load_trajectory(rows, DEV))
    assert a == b and a["updated_rays"] > 0 and "skipped" not in b
    _assert_same_volume(_host(by_traj.sum, by_traj.count), _host(by_pose.sum, by_pose.count), "constant trajectory")
    # reset gives the empty volume back
    by_pose.reset()
    assert by_pose.n_rays == 0 and int(by_pose.sum.abs().sum()) == 0 and int(by_pose.count.view(torch.int32).abs().sum()) == 0
    assert by_pose.extract_mesh() is None
    # a scan that reaches past the trajectory's end is skipped whole, as build_lidar_map skips it
    short = load_trajectory(np.asarray([row, [0.05] + row[1:]]), DEV)
    got = by_pose.integrate_scan(scans[0], trajectory=short)
    assert got["skipped"] and got["rays"] == 0 and by_pose.n_rays == 0 and int(by_pose.count.view(torch.int32).abs().sum()) == 0


def test_volume_refusals():
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.analysis.tsdf import MAX_RAYS, TSDFVolume
    volume = TSDFVolume((0, 0, 0), (1, 1, 1), 0.25, device=DEV)
    assert volume.dims == (5, 5, 5) and volume.count.dtype == torch.uint32 and volume.sum.dtype == torch.int64
    rays, ranges = torch.zeros(2, 6, dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        volume.integrate_rays(rays, ranges)
    with pytest.raises(RuntimeError):
        volume.integrate_rays(rays.to(DEV), ranges)
    with pytest.raises(ValueError):
        volume.integrate_rays(rays.to(DEV)[:, :5], ranges.to(DEV))
    with pytest.raises(ValueError):
        volume.integrate_rays(rays.to(DEV), ranges.to(DEV)[:1])
    scan = (np.array([[1.0, 0.0, 0.0]]), np.array([0.0]))
    traj = load_trajectory(_tum_rows(), DEV)
    with pytest.raises(ValueError):
        volume.integrate_scan(scan)
    with pytest.raises(ValueError):
        volume.integrate_scan(scan, pose=np.eye(4), trajectory=traj)
    with pytest.raises(ValueError):
        volume.integrate_scan(scan, trajectory=_tum_rows())
    assert volume.n_rays == 0
    # the guard on the total, by setting the counter: 2^32 - 2 rays are in, one more fits, two do not
    volume.n_rays = MAX_RAYS - 1
    with pytest.raises(ValueError):
        volume.integrate_rays(rays.to(DEV), ranges.to(DEV))
    assert volume.n_rays == MAX_RAYS - 1 and int(volume.count.view(torch.int32).abs().sum()) == 0
    got = volume.integrate_rays(rays.to(DEV)[:1], ranges.to(DEV)[:1])
    assert got["rays"] == 1 and got["invalid_rays"] == 1 and volume.n_rays == MAX_RAYS
