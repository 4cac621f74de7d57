"""Mesh sampling, the statistical outlier filter and the trajectory transform on the MI355X against the numpy restatement
(tests/cloud_tools_restatement.py): samples and neighbour means bit for bit, the outlier statistics within the summation band of
exactly rounded sums, the transform within a derived rounding bound of scipy's Slerp and interp1d, and the three workflows end to end."""
import functools

import numpy as np
import pytest
import torch

from tests import cloud_restatement as CR
from tests import cloud_tools_restatement as TR
from tests import icp_restatement as IR
from tests import test_gpu_icp as ICP_TESTS

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -53


def _t(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- sampling
SQUARE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], [3.0, 0.0, 0.0], [3.0, 1.0, 0.0],
                   [0.5, 0.0, 0.0]])
N_POINTS = [0, 1, 63, 64, 65, 100003, 2 ** 20 + 1]
SEEDS = [0, 0x9E3779B97F4A7C15]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "one":
        return SQUARE, np.array([[0, 1, 2]], dtype=np.int32)
    if name == "pair":                                  # areas 1 : 3
        return SQUARE, np.array([[0, 1, 3], [0, 4, 3]], dtype=np.int32)
    if name == "degenerate":                            # the middle triangle's vertices are collinear
        return SQUARE, np.array([[0, 1, 2], [0, 6, 1], [0, 2, 3]], dtype=np.int32)
    assert name == "random"                             # 5000 > 64^2 triangles: a three-level tree; areas over six decades
    rng = np.random.default_rng(7)
    centre = rng.uniform(-10, 10, size=(5000, 1, 3))
    size = 10.0 ** rng.uniform(-3, 0, size=(5000, 1, 1))
    v = (centre + size * rng.normal(size=(5000, 3, 3))).reshape(-1, 3)
    order = rng.permutation(len(v))                     # shared storage order, so the triangles index all over it
    inverse = np.argsort(order)
    areas = TR.triangle_areas(v[order], inverse.reshape(-1, 3))
    assert areas.max() / areas[areas > 0].min() > 1e6
    return v[order], inverse.reshape(-1, 3).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _want(name, n, seed):
    v, t = _mesh(name)
    return TR.mesh_sample(v, t, n, seed)


def _gpu_sample(v, t, n, seed):
    from loner_amd import ops
    info = {}
    p, owner = ops.mesh_sample_points(_t(v), _t(t, np.int32), n, seed, want_triangles=True, info=info)
    return p.cpu().numpy(), owner.cpu().numpy(), info


@pytest.mark.parametrize("n", N_POINTS)
@pytest.mark.parametrize("name", ["one", "pair", "degenerate", "random"])
def test_samples_are_bit_identical_to_the_restatement(name, n):
    v, t = _mesh(name)
    for seed in SEEDS:
        want_p, want_o = _want(name, n, seed)
        p, o, info = _gpu_sample(v, t, n, seed)
        assert p.shape == (n, 3) and _same_bits(o, want_o), f"{name} n={n}: {int((o != want_o).sum()) if o.shape == want_o.shape else o.shape} owners differ"
        assert _same_bits(p, want_p), f"{name} n={n} seed={seed}: {int((p != want_p).any(1).sum())} points differ"
        assert info["area"] == TR.tree_prefix(TR.triangle_areas(v, t))[-1] and info["bad_triangles"] == 0
    if n:
        assert not _same_bits(_want(name, n, SEEDS[0])[0], _want(name, n, SEEDS[1])[0])


def test_two_calls_give_the_same_bits():
    v, t = _mesh("random")
    a = _gpu_sample(v, t, 100003, 5)
    b = _gpu_sample(v, t, 100003, 5)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


@pytest.mark.parametrize("n", [100003, 2 ** 20 + 1])
def test_every_triangle_gets_its_share(n):
    """|count_t - N A_t / S| < 2: n_t and n_{t-1} are each within 1/2 (and the roundings of C / S N, far below 1/2) of N C_t / S."""
    v, t = _mesh("random")
    _, owner, info = _gpu_sample(v, t, n, 1)
    counts = np.bincount(owner, minlength=len(t))
    share = n * TR.triangle_areas(v, t) / info["area"]
    worst = float(np.abs(counts - share).max())
    print(f"n={n}: worst |count - share| = {worst:.4f}")
    assert counts.sum() == n and worst < 2


def _raw_sample(v, t, n):
    """the entry itself on buffers filled with a sentinel -> (points, owner, info)"""
    from loner_amd import hip
    from loner_amd.hip import _ptr, _stream
    lib = hip.load()
    vd, td = _t(v), _t(t, np.int32)
    need = int(lib.lnr_mesh_sample_workspace(len(t)))
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    points = torch.full((n, 3), -7.0, device=DEV, dtype=torch.float64)
    owner = torch.full((n,), -7, device=DEV, dtype=torch.int32)
    info = torch.empty(8, device=DEV, dtype=torch.int64)
    rc = lib.lnr_mesh_sample_points(_ptr(vd), len(v), _ptr(td), len(t), n, 0, _ptr(ws), need, _ptr(points), _ptr(owner), _ptr(info),
                                    _stream())
    assert rc == 0
    return points.cpu().numpy(), owner.cpu().numpy(), info.cpu().numpy()


def test_status_words_and_nothing_written():
    from loner_amd import ops
    v, t = _mesh("degenerate")
    bad_v = v.copy()
    bad_v[3, 1] = np.nan                                # used by the last triangle only
    p, o, info = _raw_sample(bad_v, t, 1000)
    assert info[0] == 1 and info[1] == 0 and info[2] == 1 and (p == -7.0).all() and (o == -7).all()
    bad_t = t.copy()
    bad_t[0, 2] = len(v)                                # one past the last vertex
    p, o, info = _raw_sample(v, bad_t, 1000)
    assert info[0] == 2 and info[1] == 0 and info[2] == 1 and (p == -7.0).all() and (o == -7).all()
    bad_t[1, 0] = -1
    bad_v[6, 0] = np.inf                                # vertex 6 is only used by triangle 1, whose index is bad already
    p, o, info = _raw_sample(bad_v, bad_t, 10)
    assert info[0] == 3 and info[2] == 3 and (p == -7.0).all()
    with pytest.raises(RuntimeError, match="non-finite vertex"):
        ops.mesh_sample_points(_t(bad_v), _t(t, np.int32), 10)
    unused = v.copy()
    unused[5, 0] = np.nan                               # no triangle uses vertex 5
    p, o, info = _raw_sample(unused, t, 64)
    assert info[0] == 0 and info[1] == 64 and _same_bits(p, TR.mesh_sample(v, t, 64, 0)[0])
    p, o, info = _raw_sample(v, np.array([[0, 6, 1]], dtype=np.int32), 64)          # no area
    assert info[0] == 0 and info[1] == 0 and (p == -7.0).all()
    p, o, info = _raw_sample(v, np.zeros((0, 3), dtype=np.int32), 64)               # no triangle
    assert info[0] == 0 and info[1] == 0 and (p == -7.0).all()


def test_triangle_mesh_methods():
    from loner_amd.analysis.mesher import TriangleMesh
    v, t = _mesh("pair")
    mesh = TriangleMesh(v, t)
    assert mesh.get_surface_area() == 2.0
    cloud, owner = mesh.sample_points_uniformly(100, seed=4, return_triangles=True)
    assert _same_bits(cloud.numpy(), TR.mesh_sample(v, t, 100, 4)[0]) and np.bincount(owner.cpu().numpy()).tolist() == [25, 75]
    assert len(TriangleMesh(v, t[:0]).sample_points_uniformly(10)) == 0
    with pytest.raises(ValueError):
        mesh.sample_points_uniformly(0)


# ---------------------------------------------------------------- outlier filter
@functools.lru_cache(maxsize=None)
def _clouds():
    return ICP_TESTS._clouds()


@functools.lru_cache(maxsize=None)
def _want_avg(name, k=20):
    return TR.knn_mean_distance(_clouds()[name], k)


def _gpu_avg(p, k=20, cell_edge=None):
    from loner_amd import ops
    g = ops.NNGrid(_t(p), cell_edge)
    stats = {}
    return g.knn_mean_distance(k, stats=stats), g, stats


@pytest.mark.parametrize("name", list(ICP_TESTS._clouds()))
def test_mean_distances_are_bit_identical_to_the_restatement(name):
    p = _clouds()[name]
    want = _want_avg(name)
    avg, g, stats = _gpu_avg(p)
    avg = avg.cpu().numpy()
    assert _same_bits(avg, want), f"{int((avg != want).sum())} of {len(p)} means differ"
    for f in (0.37, 2.0, 5.0):                          # the result does not depend on the cell edge
        assert _same_bits(_gpu_avg(p, cell_edge=g.edge * f)[0].cpu().numpy(), want), f
    print(f"{name}: {len(p)} points, edge {g.edge:.4g}, {stats}")


def test_every_point_takes_the_exact_pass():
    """the lattice at a tenth of its spacing, as tests/test_gpu_icp.py: five shells find only the point itself"""
    p = _clouds()["lattice"]
    avg, g, stats = _gpu_avg(p, cell_edge=0.05)
    assert stats["fallback"] == len(p)
    assert _same_bits(avg.cpu().numpy(), _want_avg("lattice"))
    avg5, _, _ = _gpu_avg(p, k=5, cell_edge=0.05)
    assert _same_bits(avg5.cpu().numpy(), TR.knn_mean_distance(p, 5))


STAT_CLOUDS = [name for name in ICP_TESTS._clouds() if name != "one"]       # one point: test_one_point_keeps_nothing


@pytest.mark.parametrize("name", STAT_CLOUDS)
def test_threshold_is_within_the_summation_band(name):
    """mean, std and threshold against exactly rounded sums, on every cloud of two points and more: within n 2^-53 (relative), the
    worst case of any order of summing n non-negative terms.  A sum of n terms takes n - 1 additions, so the sums are within
    (n - 1) 2^-53; the division and the square root after them, and the same on fsum's side, add a few 2^-53 more, which on the
    3-point cloud is as much as the sums' own share.  The band is held there all the same: the device's order, restated in numpy
    (test_statistics_are_bit_identical_to_the_restated_order), gives 2.3, 0 and 1.7 times 2^-53 on the 3-point cloud, 0 on the 20-point
    one, and at most 1.4 on the others."""
    p = _clouds()[name]
    n = len(p)
    avg, g, _ = _gpu_avg(p)
    got = g.outlier_threshold(avg, 1.5).cpu().numpy()
    mean, std, thr = TR.outlier_stats(_want_avg(name), 1.5)
    rel = [abs(a - b) / abs(b) if b else abs(a - b) for a, b in zip(got[:3], (mean, std, thr))]
    print(f"{name}: n={n} mean {got[0]:.17g} std {got[1]:.17g} threshold {got[2]:.17g}; relative errors {rel}, band {n * U:.3g}")
    assert got[3] == n
    assert all(r <= n * U for r in rel)


@pytest.mark.parametrize("name", STAT_CLOUDS)
def test_statistics_are_bit_identical_to_the_restated_order(name):
    """the header fixes the order of both sums (per thread, the wave's butterfly, four waves, one workgroup's fold), so mean, std and
    threshold are the restatement's bits: a term dropped or added twice in a partly filled wave or block shows at any n"""
    p = _clouds()[name]
    avg, g, _ = _gpu_avg(p)
    assert _same_bits(avg.cpu().numpy(), _want_avg(name))
    got = g.outlier_threshold(avg, 1.5).cpu().numpy()
    want = np.array(TR.outlier_stats_device_order(_want_avg(name), 1.5) + (float(len(p)),))
    assert _same_bits(got, want), f"{name}: {got.tolist()} != {want.tolist()}"


@functools.lru_cache(maxsize=None)
def _planted():
    """random 6000 and 30 points far from them; seed 0 leaves no avg_i within the summation band of the threshold (the restatement
    asserts it)"""
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.normal(size=(6000, 3)) * [3.0, 2.0, 0.5], rng.uniform(-1, 1, size=(30, 3)) * 5 + [60.0, 0, 0]])
    return p, TR.outlier_mask(TR.knn_mean_distance(p, 20), 1.5)


def test_outlier_filter_keeps_what_the_restatement_keeps():
    from loner_amd.analysis.lidar_map import PointCloud
    p, want = _planted()
    cloud = PointCloud(_t(p))
    cloud.estimate_normals(10)
    kept, index = cloud.remove_statistical_outlier(20, 1.5)
    index = index.cpu().numpy()
    assert np.array_equal(index, np.nonzero(want)[0])
    assert index.max() < 6000                           # the 30 planted points are all removed
    assert _same_bits(kept.numpy(), p[want]) and _same_bits(kept.normals.cpu().numpy(), cloud.normals.cpu().numpy()[want])
    again, index2 = cloud.remove_statistical_outlier(20, 1.5, cell_edge=0.9)
    assert np.array_equal(index2.cpu().numpy(), index)


def test_one_point_keeps_nothing():
    from loner_amd.analysis.lidar_map import PointCloud
    from loner_amd import ops
    p = _clouds()["one"]
    g = ops.NNGrid(_t(p))
    res = g.outlier_threshold(g.knn_mean_distance(20), 1.5).cpu().numpy()
    assert res[0] == 0.0 and np.isnan(res[1]) and np.isnan(res[2]) and res[3] == 1      # no avg_i > 0; 0 / 0
    kept, index = PointCloud(_t(p)).remove_statistical_outlier()
    assert len(kept) == 0 and len(index) == 0
    kept, index = PointCloud().remove_statistical_outlier()
    assert len(kept) == 0 and len(index) == 0


# ---------------------------------------------------------------- trajectory transform
@functools.lru_cache(maxsize=None)
def _trajectory():
    """40 poses 0.1 s apart on a path that moves away from the origin; neighbouring rotations up to 170 degrees apart, and one
    identity-to-identity segment (38 -> 39 repeats the rotation: the small-angle branch)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    K = 40
    T = 1.7e9 + 0.1 * np.arange(K)
    P = np.array([20.0, -10.0, 2.0]) + np.cumsum(rng.uniform(0.1, 0.6, size=(K, 3)), axis=0)
    angles = np.deg2rad(rng.uniform(1.0, 170.0, size=K - 1))
    angles[5] = np.deg2rad(170.0)
    axes = rng.normal(size=(K - 1, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    r = [Rotation.from_rotvec(rng.normal(size=3))]
    for k in range(K - 1):
        r.append(r[-1] * Rotation.from_rotvec(axes[k] * (0.0 if k == K - 2 else angles[k])))
    rows = np.concatenate([T[:, None], P, np.stack([x.as_quat() for x in r])], axis=1)
    return rows


@functools.lru_cache(maxsize=None)
def _scan():
    """10 000 points between 0.1 and 30 m, some within the 0.5 m minimum range; times over the whole trajectory including exact pose
    times, both ends, and the neighbouring doubles outside both ends"""
    rows = _trajectory()
    T = rows[:, 0]
    rng = np.random.default_rng(4)
    n = 10_000
    d = rng.normal(size=(n, 3))
    p = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.1, 30.0, size=(n, 1))
    ts = rng.uniform(T[0], T[-1], size=n)
    ts[:40] = T
    ts[40:44] = [np.nextafter(T[0], -np.inf), np.nextafter(T[-1], np.inf), T[0] - 1.0, T[-1] + 1.0]
    ts[44:46] = [np.nextafter(T[7], -np.inf), np.nextafter(T[7], np.inf)]
    p[:46] *= 2.0 / np.linalg.norm(p[:46], axis=1, keepdims=True)               # these are beyond the minimum range
    p[46] = [0.3, 0.4, 0.0]                                                      # |p| = 0.5 exactly: not > 0.5
    return p, ts


def _gpu_transform(p, ts, rows, min_range):
    from loner_amd import ops
    from loner_amd.analysis.gt_map import load_trajectory
    out, info = ops.trajectory_transform(_t(p), _t(ts), load_trajectory(rows, DEV), min_range)
    info = info.cpu().numpy()
    return out.cpu().numpy()[:info[1]], info


def test_trajectory_transform_against_scipy():
    """Bound: |out - scipy| <= 256 * 2^-53 * (|p| + |trans|) per axis, from the operations of the contract (u = 2^-53).
    Rotation, as an angle: alpha is one division of an exact difference of two times by another (<= 2 u relative; the times here are
    multiples of one ulp); w = alpha w_k adds u, the host's w_k (a quaternion product, atan2, a division and a scaling) carries <= 8 u,
    and the norm (three products, two sums, a square root) <= 3 u: theta is within 15 u relative, so with theta <= pi the rotation is
    off by at most 15 pi u < 48 u radians, which moves p by 48 u |p|.  The unit axis (a division per component) adds 4 u |p|.  sin and
    cos are within 2 u; each entry of E is then at most five operations on values <= 2: 10 u per entry, sqrt(3) 10 u |p| < 18 u |p| per
    output row.  R_k from quat_to_matrix (normalisation and four operations) carries 8 u per entry: < 14 u |p|; the products and sums
    of R_k E (5 u per entry) < 9 u |p|; those of R p (three products and two sums) < 9 u |p|.  Together 102 u |p| for this side, and
    scipy's chain (from_rotvec, a quaternion product, as_matrix, a matrix product) has the same kinds of steps: 204 u |p|.
    Translation: P_k + alpha (P_k+1 - P_k) is three operations and alpha's 2 u: <= 6 u (|P_k| + |P_k+1|) <= 12.7 u |trans| on this path,
    whose steps are at most 5 % of the poses' distance from the origin (asserted below), so that |trans| >= 0.95 max(|P_k|, |P_k+1|);
    interp1d's slope form the same: 26 u |trans|.  The last addition adds u (|p| + |trans|) on either side.
    Sum: 206 u |p| + 28 u |trans| < 256 u (|p| + |trans|)."""
    rows = _trajectory()
    p, ts = _scan()
    norms = np.linalg.norm(rows[:, 1:4], axis=1)
    steps = np.linalg.norm(np.diff(rows[:, 1:4], axis=0), axis=1)
    assert (steps <= 0.05 * np.maximum(norms[:-1], norms[1:])).all()         # |trans| >= 0.95 max(|P_k|, |P_k+1|) on every segment
    want = TR.trajectory_transform(p, ts, rows, 0.5)
    got, info = _gpu_transform(p, ts, rows, 0.5)
    assert info[0] == 0 and info[4] == 0
    assert (info[1], info[2], info[3]) == (len(want["index"]), want["below"], want["outside"])
    assert want["outside"] == 4 and want["below"] > 50 and 46 not in want["index"]
    err = np.abs(got - want["points"])
    bound = TR.transform_bound(p[want["index"]], want["trans"])[:, None]
    worst = float((err / bound).max())
    print(f"trajectory transform: {len(got)} kept; max |out - scipy| = {err.max():.3e} m, {worst * TR.TRANSFORM_BOUND_ULPS:.1f} of the "
          f"{TR.TRANSFORM_BOUND_ULPS} u (|p| + |trans|) allowed")
    assert (err <= bound).all()
    knots = np.isin(want["index"], np.arange(40))
    assert knots.sum() == 40                            # the points at the exact pose times: scipy ends a segment there, we start one
    again, _ = _gpu_transform(p, ts, rows, 0.5)
    assert _same_bits(again, got)


def test_trajectory_transform_counts_non_finite_points():
    rows = _trajectory()
    p, ts = (a.copy() for a in _scan())
    p[100, 1] = np.nan
    p[101, 0] = np.inf
    ts[102] = np.nan
    got, info = _gpu_transform(p, ts, rows, 0.5)
    ok = np.ones(len(p), dtype=bool)
    ok[100:103] = False
    want = TR.trajectory_transform(p[ok], ts[ok], rows, 0.5)
    assert info[0] == 1 and info[4] == 3 and info[1] == len(want["index"]) and np.isfinite(got).all()
    assert info[1] + info[2] + info[3] + info[4] == len(p)
    empty, info = _gpu_transform(np.zeros((0, 3)), np.zeros(0), rows, 0.5)
    assert info.tolist() == [0] * 8 and empty.shape == (0, 3)


# ---------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _scans():
    """6 scans of the box scene (1 m sampling, 1500 points each) from a sensor that moves 0.4 m per scan along x and yaws by 2 degrees
    per scan; a scan takes 0.1 s and its points carry times across it.  The trajectory has a pose every 0.05 s from the first
    scan's start to the fifth scan's end: the sixth scan runs past the last pose and is skipped whole."""
    from scipy.spatial.transform import Rotation
    world = IR.box_scene(1.0)
    K = 11
    T = 100.0 + 0.05 * np.arange(K)
    P = np.stack([-3.0 + 4.0 * (T - T[0]), np.full(K, 1.0), np.full(K, 0.5)], axis=1)
    R = Rotation.from_euler("z", 20.0 * (T - T[0]), degrees=True)
    rows = np.concatenate([T[:, None], P, R.as_quat()], axis=1)
    rng = np.random.default_rng(6)
    scans = []
    for s in range(6):
        pick = rng.permutation(len(world))[:1500]
        ts = np.sort(rng.uniform(100.0 + 0.1 * s, 100.0 + 0.1 * (s + 1), size=len(pick)))
        pose_R = Rotation.from_euler("z", 20.0 * (ts - T[0]), degrees=True).as_matrix()
        pose_t = np.stack([-3.0 + 4.0 * (ts - T[0]), np.full(len(ts), 1.0), np.full(len(ts), 0.5)], axis=1)
        scans.append((np.einsum("nba,nb->na", pose_R, world[pick] - pose_t), ts))      # R^T (p - t): the sensor frame
    return scans, rows


def test_build_lidar_map_end_to_end():
    from loner_amd.analysis.gt_map import build_lidar_map, mask_by_distance
    from loner_amd.analysis.lidar_map import PointCloud
    scans, rows = _scans()
    want, used, scale, (pop_scan, pop_merged) = TR.build_lidar_map(scans, rows, 0.25, 0.5)
    assert used == [0, 1, 2, 3, 4]                      # the sixth scan ends after the last pose
    cloud = build_lidar_map(scans, rows, voxel_size=0.25, min_range=0.5, device=DEV)
    got = cloud.numpy()
    assert got.shape == want.shape
    # the transform's bound on every input of a voxel's mean, and the two means' own roundings, which may fall differently on either
    # side: (m - 1) additions and a division, on sums of at most m points each
    bound = (TR.TRANSFORM_BOUND_ULPS + 2 * (pop_scan + pop_merged)) * U * scale
    err = float(np.abs(got - want).max())
    print(f"map: {len(got)} points from {len(used)} scans, max |got - restatement| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    filtered = build_lidar_map(scans, rows, voxel_size=0.25, run_outlier_filter=True, min_range=0.5, device=DEV)
    assert 0.8 * len(cloud) < len(filtered) < len(cloud)

    # the box scene is the ground truth here: keep its points within 0.3 m of the map
    gt = IR.box_scene(1.0)
    d = np.sqrt(CR.sq_distances(gt, got))
    assert not (np.abs(d - 0.3) < 1e-12).any()
    masked = mask_by_distance(PointCloud(_t(gt)), cloud, threshold=0.3)
    assert _same_bits(masked.numpy(), gt[d < 0.3]) and 0 < len(masked) < len(gt)


def test_mask_by_distance_carries_attributes_and_keeps_nothing_near_an_empty_reference():
    from loner_amd.analysis.gt_map import mask_by_distance
    from loner_amd.analysis.lidar_map import PointCloud
    p = _clouds()["random"][:500]
    ref = _clouds()["random"][500:560]
    d = np.sqrt(CR.sq_distances(p, ref))
    keep = d < 0.5
    assert not (np.abs(d - 0.5) < 1e-12).any() and 0 < keep.sum() < len(p)
    cloud = PointCloud(_t(p))
    cloud.estimate_normals(10)
    cloud.estimate_covariances(10)
    masked = mask_by_distance(cloud, PointCloud(_t(ref)), threshold=0.5)
    assert _same_bits(masked.numpy(), p[keep])
    assert _same_bits(masked.normals.cpu().numpy(), cloud.normals.cpu().numpy()[keep])
    assert _same_bits(masked.covariances.cpu().numpy(), cloud.covariances.cpu().numpy()[keep])
    none = mask_by_distance(cloud, PointCloud(), threshold=0.5)
    assert len(none) == 0 and none.normals.shape == (0, 3)


def test_evaluate_mesh_of_a_box_against_its_own_samples(tmp_path):
    from loner_amd.analysis.mesh_eval import evaluate_mesh, mesh_to_point_cloud
    from loner_amd.analysis.mesher import TriangleMesh
    from loner_amd.analysis.lidar_map import read_point_cloud
    lo, hi = np.array([-2.0, -1.5, 0.0]), np.array([2.0, 1.5, 2.0])
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.array([[a, b, c] for a, b, c, d in faces] + [[a, c, d] for a, b, c, d in faces], dtype=np.int32)
    mesh = TriangleMesh(corners, tris)
    assert mesh.get_surface_area() == 52.0
    gt = mesh.sample_points_uniformly(300_000, seed=1)
    stats = evaluate_mesh(mesh, gt, str(tmp_path), f_score_threshold=0.1, voxel_size=0.05, number_of_points=300_000, seed=2)
    print(stats)
    assert stats["accuracy"] < 0.05 and stats["completion"] < 0.05
    assert stats["precision"] == 1.0 and stats["recall"] == 1.0 and stats["f-score"] > 1.0 - 1e-8
    path = tmp_path / "box.ply"
    mesh.write_ply(str(path))
    cloud = mesh_to_point_cloud(str(path), 0.05, number_of_points=300_000, seed=2)
    back = read_point_cloud(str(tmp_path / "box_sampled.pcd"))
    assert len(back) == len(cloud) and np.abs(back.numpy() - cloud.numpy()).max() < 1e-6
