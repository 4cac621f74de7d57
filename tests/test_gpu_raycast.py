"""Ray casting on the MI355X against the numpy restatement (tests/raycast_restatement.py): t_hit, ids and uvs bit for bit on soups
with every degenerate the contract names, trees that tie and trees tens of levels deep, flat scenes, the [t_min, t_max] window,
watertightness on closed meshes, the rays of a moving sensor, and the workflows built on them (simulate_scan and its inverse
ops.trajectory_transform, depth images, mesh_depth_l1, simulate_sequence)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from loner_amd.utils import synthetic as SYN
from loner_amd.utils import synthetic_mesh as SM
from tests import raycast_restatement as RR

pytestmark = pytest.mark.gpu

DEV = "cuda"
# the inscribed radius of icosphere(2) with radius 1: the smallest distance from the centre to a triangle's plane (the foot of the
# perpendicular lies inside every triangle), worked out in fp64 from the mesh; test_icosphere... recomputes it
ICOSPHERE2_INRADIUS = 0.982246946376846


def _t(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _gpu_cast(v, f, rays, t_min=0.0, t_max=math.inf, bvh=None):
    from loner_amd import ops
    bvh = ops.BVH(_t(v), _t(f, np.int32)) if bvh is None else bvh
    stats = {}
    t, ids, uvs = ops.cast_rays(bvh, _t(rays).reshape(-1, 6), t_min, t_max, stats=stats)
    return dict(t_hit=t.cpu().numpy(), primitive_ids=ids.cpu().numpy(), primitive_uvs=uvs.cpu().numpy(), stats=stats, bvh=bvh)


def _assert_equal(got, want, what=""):
    for key in ("primitive_ids", "t_hit", "primitive_uvs"):
        if not _same_bits(got[key], want[key]):
            bad = np.nonzero(np.atleast_2d((got[key] != want[key]).T).any(axis=0))[0]
            raise AssertionError(f"{what}: {key} differs on {len(bad)} rays, first {bad[:5]}: got {got[key][bad[:5]]}, want "
                                 f"{want[key][bad[:5]]}")
    n = len(want["t_hit"])
    assert got["stats"]["hits"] == int((want["primitive_ids"] >= 0).sum()), what
    assert got["stats"]["invalid_rays"] == want["invalid_rays"] and got["stats"]["capped_rays"] == 0, what
    assert got["stats"]["excluded_triangles"] == want["excluded_triangles"], what
    assert got["stats"]["depth"] < _stack(), what
    assert n == 0 or got["stats"]["node_visits"] >= 0


def _stack():
    from loner_amd import hip
    return hip.BVH_STACK


# ---------------------------------------------------------------- the soup
@functools.lru_cache(maxsize=None)
def _soup():
    """2000 triangles in a 10 m box: 1875 random, then 50 copies of earlier ones, 50 without area (25 with two corners at the same
    place, 25 with the third corner the exact midpoint of the other two), 20 with a repeated index, 5 with a NaN vertex.
    -> (vertices, triangles, the ranges of the groups)"""
    rng = np.random.default_rng(11)
    n0 = 1875
    centre = rng.uniform(0.0, 10.0, (n0, 1, 3))
    v = (centre + rng.uniform(-0.6, 0.6, (n0, 3, 3))).reshape(-1, 3)
    f = np.arange(3 * n0).reshape(n0, 3)
    dup = f[rng.choice(n0, 50, replace=False)]
    a = np.round(rng.uniform(0.0, 10.0, (50, 3)) * 1024) / 1024             # dyadic: the midpoint is exact
    b = np.round(rng.uniform(0.0, 10.0, (50, 3)) * 1024) / 1024
    c = np.concatenate([b[:25], 0.5 * (a[25:] + b[25:])])
    base = len(v)
    v = np.concatenate([v, a, b, c])
    flat = np.stack([base + np.arange(50), base + 50 + np.arange(50), base + 100 + np.arange(50)], axis=1)
    rep = f[rng.choice(n0, 20, replace=False)].copy()
    rep[:, 2] = rep[:, 0]
    nan_v = rng.uniform(0.0, 10.0, (15, 3))
    nan_v[::3, rng.integers(0, 3)] = np.nan
    nan_v[3, 1] = np.inf
    base = len(v)
    v = np.concatenate([v, nan_v])
    nan_f = base + np.arange(15).reshape(5, 3)
    f = np.concatenate([f, dup, flat, rep, nan_f]).astype(np.int32)
    assert f.shape == (2000, 3)
    groups = dict(random=(0, n0), dup=(n0, n0 + 50), flat=(n0 + 50, n0 + 100), rep=(n0 + 100, n0 + 120), nan=(n0 + 120, n0 + 125))
    return v, f, groups


@functools.lru_cache(maxsize=None)
def _soup_rays():
    """4096 rays: 2500 random; 200 from a corner of a triangle (t = 0 exactly) and 200 from a point on one; 300 with one and 200 with
    two zero direction components; 200 in a triangle's plane; 250 aimed exactly at corners and 246 at points on edges"""
    v, f, _ = _soup()
    rng = np.random.default_rng(12)
    tri = lambda n: v[f[rng.integers(0, 1875, n)]]                           # noqa: E731  [n,3,3]
    org = lambda n: rng.uniform(-1.0, 11.0, (n, 3))                          # noqa: E731
    parts = [np.concatenate([org(2500), rng.normal(size=(2500, 3))], axis=1)]
    T = tri(200)
    parts.append(np.concatenate([T[:, 0], rng.normal(size=(200, 3))], axis=1))
    T, w = tri(200), rng.dirichlet((1, 1, 1), 200)
    parts.append(np.concatenate([np.einsum("nk,nka->na", w, T), rng.normal(size=(200, 3))], axis=1))
    d = rng.normal(size=(300, 3))
    d[np.arange(300), rng.integers(0, 3, 300)] = 0.0
    parts.append(np.concatenate([org(300), d], axis=1))
    d = np.zeros((200, 3))
    d[np.arange(200), rng.integers(0, 3, 200)] = rng.choice([-1.0, 1.0, 0.37], 200)
    o = org(200)
    T = tri(200)
    o[:100] = T[:100, 1] - d[:100] * 3.0                                     # half of them through a corner
    parts.append(np.concatenate([o, d], axis=1))
    T = tri(200)
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    parts.append(np.concatenate([T[:, 0] - e1, e1 + 0.5 * e2], axis=1)[:100])
    parts.append(np.concatenate([T[:, 0], e1], axis=1)[100:])                # along an edge
    T, o = tri(250), org(250)
    parts.append(np.concatenate([o, T[:, 2] - o], axis=1))
    T, o, s = tri(246), org(246), rng.uniform(0, 1, (246, 1))
    parts.append(np.concatenate([o, (T[:, 0] + s * (T[:, 1] - T[:, 0])) - o], axis=1))
    rays = np.concatenate(parts)
    assert rays.shape == (4096, 6)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def _soup_want():
    v, f, _ = _soup()
    return RR.cast_rays(v, f, _soup_rays())


def test_soup_bit_for_bit_with_every_degenerate():
    v, f, groups = _soup()
    want = _soup_want()
    ids = want["primitive_ids"]
    assert want["excluded_triangles"] == 5 and (ids >= 0).sum() > 1500
    for name in ("dup", "flat", "rep", "nan"):                               # the restatement itself never returns them
        lo, hi = groups[name]
        assert not ((ids >= lo) & (ids < hi)).any(), name
    assert (want["t_hit"] == 0.0).sum() >= 150                               # rays that start on a surface
    got = _gpu_cast(v, f, _soup_rays())
    _assert_equal(got, want, "soup")
    assert got["bvh"].n_in_tree == 1995 and got["bvh"].n_nonfinite == 5
    print(f"soup: depth {got['stats']['depth']}, {got['stats']['node_visits'] / 4096:.1f} node visits per ray")


def test_two_runs_give_identical_bytes():
    v, f, _ = _soup()
    a, b = _gpu_cast(v, f, _soup_rays()), _gpu_cast(v, f, _soup_rays())
    for key in ("t_hit", "primitive_ids", "primitive_uvs"):
        assert _same_bits(a[key], b[key]), key
    assert a["stats"] == b["stats"]


@pytest.mark.parametrize("n_tris", [0, 1, 2, 3, 65])
def test_small_meshes_and_ray_counts(n_tris):
    v, f, _ = _soup()
    f = f[:n_tris]
    rng = np.random.default_rng(n_tris)
    o = rng.uniform(-1.0, 11.0, (1000, 3))
    target = v[f[rng.integers(0, max(n_tris, 1), 1000)]].mean(axis=1) if n_tris else rng.uniform(0, 10, (1000, 3))
    rays = np.concatenate([o, target + rng.normal(scale=0.2, size=(1000, 3)) - o], axis=1)
    want = RR.cast_rays(v, f, rays)
    assert n_tris == 0 or (want["primitive_ids"] >= 0).sum() > 100
    bvh = None
    for n in (0, 1, 63, 64, 65, 1000):
        got = _gpu_cast(v, f, rays[:n], bvh=bvh)
        bvh = got["bvh"]
        part = {k: (x[:n] if isinstance(x, np.ndarray) else x) for k, x in want.items()}
        _assert_equal(got, part, f"F = {n_tris}, n = {n}")
    assert bvh.n_in_tree == n_tris and (n_tris >= 2 or bvh.depth == 0) and bvh.n_nodes == max(2 * n_tris - 1, 0)


def test_index_out_of_range_sets_the_status_and_is_not_dereferenced():
    from loner_amd import ops
    v, f, _ = _soup()
    for bad in (len(v), -1, 2 ** 31 - 1):
        g = f[:100].copy()
        g[37, 1] = bad
        with pytest.raises(RuntimeError, match="index"):
            ops.BVH(_t(v), _t(g, np.int32))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- ties and depth
def _aimed(v, f, rng, n_random=200):
    """rays from above at every triangle's centre (slightly tilted), and random ones"""
    c = v[f].mean(axis=1)
    o = c + np.array([0.013, -0.007, 1.0])
    box_lo, box_hi = v.min(0) - 1.0, v.max(0) + 1.0
    ro = rng.uniform(box_lo, box_hi, (n_random, 3))
    return np.concatenate([np.concatenate([o, c - o], axis=1), np.concatenate([ro, rng.normal(size=(n_random, 3))], axis=1)])


def test_equal_codes_shared_centres_and_deep_trees():
    rng = np.random.default_rng(5)
    tri = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.2]])
    # 512 copies of one triangle: every code is equal, the sorted position alone shapes the tree
    v, f = tri, np.tile(np.arange(3), (512, 1))
    rays = _aimed(v, f[:1], rng)
    want = RR.cast_rays(v, f, rays)
    got = _gpu_cast(v, f, rays)
    _assert_equal(got, want, "512 copies")
    assert want["primitive_ids"][0] == 0 and set(np.unique(want["primitive_ids"])) <= {-1, 0}
    assert got["stats"]["depth"] == 9
    # concentric triangles in one plane around one centre: one box centre, one code, every ray through the middle hits them all at one t
    ring = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
    v = np.concatenate([ring * s for s in np.arange(64, 0, -1)]) + np.array([3.0, 4.0, 1.0])
    f = np.concatenate([[[4 * k, 4 * k + 1, 4 * k + 2], [4 * k, 4 * k + 2, 4 * k + 3]] for k in range(64)])
    rays = _aimed(v, f, rng)
    rays = np.concatenate([rays, [[3.1, 4.05, 5.0, 0.0, 0.0, -1.0], [3.0, 4.0, -2.0, 0.0, 0.0, 1.0]]])
    want = RR.cast_rays(v, f, rays)
    assert want["primitive_ids"][-2] == 0 and want["t_hit"][-2] == 4.0
    _assert_equal(_gpu_cast(v, f, rays), want, "concentric")
    # clusters of 8 small triangles at x = 2^-k: the codes share ever longer prefixes and the tree is tens of levels deep
    vs, fs = [], []
    for k in range(21):
        x, size = 2.0 ** -k, 2.0 ** -(k + 3)
        for j in range(8):
            p = np.array([x, 0.0, 0.0]) + size * np.array([0.1 * j, 0.05 * j, 0.02 * j])
            fs.append(len(vs) + np.arange(3))
            vs += [p, p + size * np.array([0.5, 0.0, 0.1]), p + size * np.array([0.0, 0.5, 0.0])]
    v, f = np.asarray(vs), np.asarray(fs)
    rays = _aimed(v, f, rng)
    want = RR.cast_rays(v, f, rays)
    assert (want["primitive_ids"][:168] >= 0).all()
    got = _gpu_cast(v, f, rays)
    _assert_equal(got, want, "clusters at 2^-k")
    print(f"clusters: depth {got['stats']['depth']}")
    assert 20 <= got["stats"]["depth"] < _stack()


def test_flat_scene_crossing_and_grazing_rays():
    """every triangle in the plane z = 1: boxes without thickness, a scene box without extent on one axis"""
    rng = np.random.default_rng(6)
    g = np.arange(11, dtype=np.float64)
    v = np.stack([np.repeat(g, 11), np.tile(g, 11), np.ones(121)], axis=1)
    quad = np.array([[i * 11 + j, (i + 1) * 11 + j, (i + 1) * 11 + j + 1, i * 11 + j + 1] for i in range(10) for j in range(10)])
    f = np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]])
    o = rng.uniform(-1, 11, (600, 3))
    cross = np.concatenate([o, rng.normal(size=(600, 3))], axis=1)
    graze = cross[:300].copy()
    graze[:, 2] = 1.0                                                        # in the plane ...
    graze[:, 5] = 0.0                                                        # ... and staying in it
    off = graze[:100].copy()
    off[:, 2] = 1.5                                                          # parallel to it: never meets it
    down = np.concatenate([v[:, :2], np.full((121, 1), 3.0), np.zeros((121, 2)), np.full((121, 1), -1.0)], axis=1)    # at the vertices
    rays = np.concatenate([cross, graze, off, down])
    want = RR.cast_rays(v, f, rays)
    assert (want["primitive_ids"][900:1000] == -1).all() and (want["primitive_ids"][1000:] >= 0).all()
    assert (want["t_hit"][1000:] == 2.0).all()
    _assert_equal(_gpu_cast(v, f, rays), want, "flat")


def test_window():
    v = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [0, 0, 2.3], [1, 0, 2.3], [0, 1, 2.3]], dtype=np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    rays = np.array([[0.2, 0.3, 0.0, 0.01, 0.02, 0.7], [0.1, 0.1, 0.0, 0.0, 0.0, 1.0]])
    free = RR.cast_rays(v, f, rays, 0.0, np.inf)
    assert (free["primitive_ids"] == 0).all()
    far = RR.cast_rays(v, f, rays, 2.0, np.inf)
    assert (far["primitive_ids"] == 1).all()                                 # the nearer hit lies below t_min
    _assert_equal(_gpu_cast(v, f, rays, 2.0, np.inf), far, "t_min")
    for k in range(2):
        t1 = float(far["t_hit"][k])
        at = _gpu_cast(v, f, rays[k:k + 1], 2.0, t1)
        assert at["primitive_ids"][0] == 1 and at["t_hit"][0] == t1         # exactly t_max is accepted
        below = _gpu_cast(v, f, rays[k:k + 1], 2.0, np.nextafter(t1, 0.0), bvh=at["bvh"])
        assert below["primitive_ids"][0] == -1 and np.isinf(below["t_hit"][0])
        t0 = float(free["t_hit"][k])
        exact = _gpu_cast(v, f, rays[k:k + 1], t0, t0, bvh=at["bvh"])
        assert exact["primitive_ids"][0] == 0 and exact["t_hit"][0] == t0
        above = _gpu_cast(v, f, rays[k:k + 1], np.nextafter(t0, np.inf), np.inf, bvh=at["bvh"])
        assert above["primitive_ids"][0] == 1


# ---------------------------------------------------------------- watertightness
def test_box_room_has_no_cracks():
    v, f = SM.box_room_mesh()
    rays = RR.room_rays(SYN.BOX_MIN, SYN.BOX_MAX)
    got = _gpu_cast(v, f, rays)
    want = RR.slab_distance(rays, SYN.BOX_MIN, SYN.BOX_MAX)
    misses = int((got["primitive_ids"] < 0).sum())
    rel = np.abs(got["t_hit"] - want) / want
    print(f"box room: misses {misses}, max relative difference {np.nanmax(rel):.3e}")
    assert misses == 0
    assert rel.max() <= 1e-12
    _assert_equal(got, RR.cast_rays(v, f, rays), "box room")


def test_icosphere_from_its_centre_has_no_cracks():
    r, c = 3.0, np.array([8.0, 3.0, 0.0])
    v, f = SM.icosphere(2, r, c)
    assert f.shape == (320, 3)
    a, b, cc = (v[f[:, k]] - c for k in range(3))
    n = np.cross(b - a, cc - a)
    inradius = (np.einsum("na,na->n", n, a) / np.linalg.norm(n, axis=1)).min() / r
    assert abs(inradius - ICOSPHERE2_INRADIUS) < 1e-14 and ICOSPHERE2_INRADIUS > math.cos(math.pi / 10)
    d = RR.lidar_directions(64, 1024, (-88.0, 88.0))
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.broadcast_to(c, d.shape), d], axis=1)
    got = _gpu_cast(v, f, rays)
    t = got["t_hit"]
    misses = int((got["primitive_ids"] < 0).sum())
    print(f"icosphere: misses {misses}, t / r in [{t.min() / r:.15f}, {t[np.isfinite(t)].max() / r:.15f}]")
    assert misses == 0
    assert t.min() >= r * math.cos(math.pi / 10) and t.max() <= r * (1 + 1e-12)
    assert t.min() >= r * ICOSPHERE2_INRADIUS * (1 - 1e-12)


# ---------------------------------------------------------------- trajectory rays
def _tum(yaw_step_deg=10.0, step=1.0, dt=0.1, n=3, start=(0.0, 0.0, 1.0), t0=0.0):
    rows = []
    for k in range(n):
        h = math.radians(yaw_step_deg) * k / 2.0
        rows.append([t0 + dt * k, start[0] + step * k, start[1], start[2], 0.0, 0.0, math.sin(h), math.cos(h)])
    return np.asarray(rows)


def test_trajectory_rays_bit_for_bit():
    from loner_amd import ops
    from loner_amd.analysis.gt_map import trajectory_arrays
    q = lambda ax, ang: list(np.asarray(ax) / np.linalg.norm(ax) * math.sin(ang / 2)) + [math.cos(ang / 2)]    # noqa: E731
    rows = np.array([[1.0, 0, 0, 0] + q([0, 0, 1], 0.0), [1.5, 1, 0, 0.2] + q([0, 0, 1], 0.4), [2.25, 2, 1, 0.1] + q([1, 2, 3], 1.1),
                     [2.5, 2, 2, 0.1] + q([1, 2, 3], 1.1),                   # no rotation in this segment: the 1e-9 branch
                     [3.0, 1, 3, -0.2] + q([-1, 0.5, 0.2], 2.0), [4.0, 0, 3, 0] + q([0, 1, 0], -0.7)])
    T, P, R, W = trajectory_arrays(rows)
    assert np.linalg.norm(W[2]) < 1e-9 and np.linalg.norm(W[1]) > 0.5
    rng = np.random.default_rng(3)
    dirs, _ = SYN.lidar_pattern(4, 64)
    dirs = dirs.numpy()
    stamps = rng.uniform(1.0, 4.0, dirs.shape[1])
    stamps[:8] = [1.0, 1.5, 2.25, 2.5, 3.0, 4.0, 2.3, 2.4]                   # on the poses, and in the segment without rotation
    stamps[8:12] = [3.5, 3.999, 0.999, 4.0 + 1e-9]                           # the last segment; outside
    stamps[12] = np.nan
    dirs[1, 13] = np.inf
    want, info = RR.trajectory_rays(dirs, stamps, T, P, R, W)
    traj = ops.Trajectory(T, P, R, W, DEV)
    rays, info_dev = ops.trajectory_rays(_t(dirs, np.float32), _t(stamps), traj)
    got, info_dev = rays.cpu().numpy(), info_dev.cpu().numpy()
    assert list(info_dev) == [1, info["rays"], info["outside"], info["nonfinite"], 0, 0, 0, 0]
    assert info["outside"] == 2 and info["nonfinite"] == 2
    differ = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    print(f"trajectory rays: {int(differ.sum())} of {differ.size} words differ, max |difference| "
          f"{np.nanmax(np.abs(got - want)):.3e}")
    assert _same_bits(got, want)


# ---------------------------------------------------------------- workflows
@functools.lru_cache(maxsize=None)
def _scene():
    from loner_amd.analysis.raycast import RaycastingScene
    return RaycastingScene(*SM.scene_mesh(), device=DEV)


@functools.lru_cache(maxsize=None)
def _moving_scan(frozen=False):
    from loner_amd.analysis import lidar_sim
    from loner_amd.analysis.gt_map import load_trajectory
    rows = _tum()
    if frozen:
        rows[:, 1:] = rows[0, 1:]
    dirs, times = SYN.lidar_pattern(16, 256)
    traj = load_trajectory(rows, DEV)
    scan, keep = lidar_sim.simulate_scan(_scene(), traj, dirs, times, 0.0, (1.0, 50.0))
    return scan, keep, traj, times


def test_simulated_scan_closes_the_loop_with_the_trajectory_transform():
    """dir * dist moved by the same trajectory lands on the triangle each ray hit: within 1e-4 m of its plane and inside its bounds
    grown by as much (fp32 range and point: 64 m * 2^-23 per operation over a handful of operations is about 1e-5 m)"""
    from loner_amd import ops
    scan, keep, traj, times = _moving_scan()
    assert int(keep.sum()) == len(scan) > 3500
    pts = (scan.ray_directions.double() * scan.distances.double()).T.contiguous()
    stamps = times.to(DEV)[keep].double() + 0.0
    out, info = ops.trajectory_transform(pts, stamps, traj, 0.0)
    info = info.cpu()
    assert int(info[0]) == 0 and int(info[1]) == len(scan)
    scene = _scene()
    tri = scene.triangles[scan.primitive_ids.long()].long()
    a, b, c = (scene.vertices[tri[:, k]] for k in range(3))
    n = scene.triangle_normals()[scan.primitive_ids.long()]
    plane = ((out - a) * n).sum(1).abs()
    lo, hi = torch.minimum(torch.minimum(a, b), c), torch.maximum(torch.maximum(a, b), c)
    outside = torch.maximum(lo - out, out - hi).max()
    print(f"closed loop: max plane distance {float(plane.max()):.3e} m, max excess over the bounds {float(outside):.3e} m")
    assert float(plane.max()) <= 1e-4
    assert float(outside) <= 1e-4
    assert len(torch.unique(scan.primitive_ids)) > 20 and int((scan.primitive_ids >= 12).sum()) > 50      # walls and sphere


def test_motion_is_in_the_simulated_data():
    moving, keep_m, _, _ = _moving_scan()
    frozen, keep_f, _, _ = _moving_scan(True)
    dm = torch.full(keep_m.shape, float("nan"), device=DEV)
    df = dm.clone()
    dm[keep_m], df[keep_f] = moving.distances, frozen.distances
    both = keep_m & keep_f
    diff = (dm - df)[both].abs()
    print(f"moving vs frozen: max range difference {float(diff.max()):.3f} m")
    assert float(diff.max()) > 0.1


def test_depth_image_of_the_box_room():
    from loner_amd.analysis.raycast import RaycastingScene
    from loner_amd.analysis.renderer import depth_to_rgba, lidar_only_calibration
    from loner_amd.common.ray_utils import CameraRayDirections
    scene = RaycastingScene(*SM.box_room_mesh(), device=DEV)
    cam = CameraRayDirections(lidar_only_calibration(), device=DEV)
    h = 0.3
    T = np.array([[math.cos(h), 0, math.sin(h), 0.0], [0, 1, 0, 0.0], [-math.sin(h), 0, math.cos(h), 2.0], [0, 0, 0, 1]])
    depth = scene.depth_image(torch.from_numpy(T), cam)
    assert tuple(depth.shape) == (1, 1, 384, 512) and depth.dtype == torch.float64
    d = cam.directions.cpu().numpy().astype(np.float64)
    world = (d[:, 0:1] * T[:3, 0] + d[:, 1:2] * T[:3, 1]) + d[:, 2:3] * T[:3, 2]
    rays = np.concatenate([np.broadcast_to(T[:3, 3], world.shape), world], axis=1)
    want = RR.slab_distance(rays, SYN.BOX_MIN, SYN.BOX_MAX) * np.linalg.norm(world, axis=1)
    got = depth.reshape(-1).cpu().numpy()
    rel = np.abs(got - want) / want
    print(f"depth image: max relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-12
    assert tuple(depth_to_rgba(depth.float()).shape) == (384, 512, 4)


def test_mesh_depth_l1():
    from loner_amd.analysis.mesh_eval import mesh_depth_l1
    from loner_amd.analysis.raycast import RaycastingScene
    gt = RaycastingScene(*SM.box_room_mesh(), device=DEV)
    lo, hi = np.asarray(SYN.BOX_MIN) - 0.05, np.asarray(SYN.BOX_MAX) + 0.05
    est = RaycastingScene(*SM.box_room_mesh(lo, hi), device=DEV)
    dirs, _ = SYN.lidar_pattern(16, 256)
    poses = []
    for x, y, z, h in ((0.0, 0.0, 2.0, 0.0), (5.0, -3.0, 1.0, 0.7)):
        poses.append(np.array([[math.cos(h), -math.sin(h), 0, x], [math.sin(h), math.cos(h), 0, y], [0, 0, 1, z], [0, 0, 0, 1.0]]))
    same = mesh_depth_l1(gt, gt, poses, dirs, (0.0, 100.0))
    assert same["depth_l1"] == 0.0 and same["n_valid"] == same["n_rays"] == 2 * 4096
    assert same["est_miss_ratio"] == 0.0 and same["gt_miss_ratio"] == 0.0
    got = mesh_depth_l1(est, gt, poses, dirs, (0.0, 100.0))
    d = dirs.numpy().astype(np.float64).T
    want = []
    for T in poses:
        world = (d[:, 0:1] * T[:3, 0] + d[:, 1:2] * T[:3, 1]) + d[:, 2:3] * T[:3, 2]
        rays = np.concatenate([np.broadcast_to(T[:3, 3], world.shape), world], axis=1)
        length = np.linalg.norm(world, axis=1)
        want.append(np.abs(RR.slab_distance(rays, lo, hi) * length - RR.slab_distance(rays, SYN.BOX_MIN, SYN.BOX_MAX) * length))
    want = float(np.concatenate(want).mean())
    print(f"mesh_depth_l1: {got['depth_l1']!r}, analytic {want!r}")
    assert got["n_valid"] == 2 * 4096 and abs(got["depth_l1"] - want) <= 1e-9
    near = mesh_depth_l1(est, gt, poses, dirs, (0.0, 12.0))                  # a range that cuts rays off: they count as missed
    assert 0.0 < near["gt_miss_ratio"] <= near["est_miss_ratio"] < 1.0 and near["n_valid"] < 2 * 4096


def test_simulated_sequence_goes_through_scan_ingestion(tmp_path):
    """build_scan_from_points gives the ranges back to fp32 rounding: the direction's length (1.5), the three products (1) and the
    norm (2) each within that many units of 2^-24 relative; 6 * 2^-24 * range bounds their sum"""
    from loner_amd.analysis import lidar_sim
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.common.sensors import build_scan_from_points
    rows = _tum(n=4)
    dirs, times = SYN.lidar_pattern(16, 256)
    out = str(tmp_path / "seq")
    stamps = lidar_sim.simulate_sequence(_scene(), rows, out, (dirs, times), scan_period=0.1, n_scans=2, ray_range=(1.0, 50.0))
    assert stamps == [0.0, 0.1]
    traj = load_trajectory(rows, DEV)
    for k, stamp in enumerate(stamps):
        want, keep = lidar_sim.simulate_scan(_scene(), traj, dirs, times, stamp, (1.0, 50.0), 0.0, k)
        pts = np.load(os.path.join(out, f"{k:06d}.npy"))
        assert pts.shape == (len(want), 4) and pts.dtype == np.float32
        scan, order = build_scan_from_points(pts[:, :3], pts[:, 3], float(stamp), device=DEV)
        assert len(scan) == len(want) and scan.time_sorted
        ref = want.distances[order]
        err = (scan.distances - ref).abs() / ref
        print(f"scan {k}: max relative range difference {float(err.max()):.3e}")
        assert float(err.max()) <= 6 * 2.0 ** -24
        assert float((scan.ray_directions - want.ray_directions[:, order]).abs().max()) <= 6 * 2.0 ** -24
