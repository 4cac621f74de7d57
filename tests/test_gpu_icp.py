"""Normals and point-to-plane ICP on the MI355X against the numpy restatement (tests/icp_restatement.py): covariances and
correspondences bit for bit, normals and ICP steps to tight tolerances, a known rigid motion recovered, and the refined evaluation end
to end."""
import numpy as np
import pytest
import torch

from tests import cloud_restatement as CR
from tests import icp_restatement as IR

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _gpu_normals(p, knn=30, cell_edge=None):
    from loner_amd import ops
    g = ops.NNGrid(_t(p), cell_edge)
    stats = {}
    n, C = g.normals(knn, want_covariances=True, stats=stats)
    return n.cpu().numpy(), C.cpu().numpy(), g, stats


def _clouds():
    rng = np.random.default_rng(1)
    ax = np.arange(-4, 5) * 0.5
    lattice = np.stack(np.meshgrid(ax, ax, ax[:4], indexing="ij"), -1).reshape(-1, 3)
    dup = np.concatenate([rng.uniform(-1, 1, size=(300, 3))] * 3)
    return {"random": rng.normal(size=(6000, 3)) * [3.0, 2.0, 0.5], "lattice": lattice, "box": IR.box_scene(0.5), "dup": dup,
            "one": rng.normal(size=(1, 3)), "two": rng.normal(size=(2, 3)), "three": rng.normal(size=(3, 3)),
            "twenty": rng.normal(size=(20, 3))}


@pytest.mark.parametrize("name", list(_clouds()))
def test_covariances_are_bit_identical_to_the_restatement(name):
    p = _clouds()[name]
    idx, _ = IR.knn(p, 30)
    want = IR.covariance(p, idx)
    n0, C0, g, stats = _gpu_normals(p)
    assert _same_bits(C0, want), f"{int((C0 != want).any((1, 2)).sum())} of {len(p)} covariances differ"
    for f in (0.37, 2.0, 5.0):                       # the result does not depend on the cell edge
        n1, C1, _, _ = _gpu_normals(p, cell_edge=g.edge * f)
        assert _same_bits(C1, want) and _same_bits(n1, n0), f
    print(f"{name}: {len(p)} points, edge {g.edge:.4g}, {stats}")


def test_every_point_takes_the_exact_knn_pass():
    """A cell edge of a tenth of the lattice's spacing: five shells reach at most 0.25 from a query on every axis, so a point finds only
    itself while unvisited cells remain, and all 324 points go through knn_brute."""
    p = _clouds()["lattice"]
    n0, _, _, _ = _gpu_normals(p)
    n1, C1, g, stats = _gpu_normals(p, cell_edge=0.05)
    print(f"lattice: {len(p)} points, edge {g.edge:.4g}, dims {g.dims}, {stats}")
    assert stats["fallback"] == len(p)
    want = IR.covariance(p, IR.knn(p, 30)[0])
    assert _same_bits(C1, want), f"{int((C1 != want).any((1, 2)).sum())} of {len(p)} covariances differ"
    assert _same_bits(n1, n0)


@pytest.mark.parametrize("name", list(_clouds()))
def test_normals_match_the_eigenvector(name):
    p = _clouds()[name]
    n, C, _, _ = _gpu_normals(p, 16)
    want, exact = IR.normal_rule(C)
    assert np.array_equal(n[exact], want[exact])
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-14
    good = ~exact & (IR.eigen_gap(C) > 1e-4)
    dots = np.abs((n[good] * want[good]).sum(1))
    assert np.all(dots >= 1 - 1e-12), dots.min()
    print(f"{name}: {int(exact.sum())} exact, {int(good.sum())} well conditioned of {len(p)}")


def test_correspondences_are_bit_identical_to_brute_force():
    from loner_amd import ops
    rng = np.random.default_rng(3)
    ax = np.arange(-10, 10) * 0.25
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    tgt = np.concatenate([lat, rng.uniform(-2.5, 2.5, size=(4000, 3))])
    mid = lat[rng.integers(0, len(lat), 3000)] + np.array([0.125, 0.125, 0.0])       # ties between lattice points
    exact_r = lat[rng.integers(0, len(lat), 500)] + np.array([0.0, 0.0, 0.125])      # a lattice point at exactly r
    far = rng.normal(size=(500, 3)) + [9.0, 0.0, 0.0]
    src = np.concatenate([mid, exact_r, far, rng.uniform(-3, 3, size=(6000, 3))])
    for r in (0.125, 0.3, 1.0):
        want_i, want_d = IR.correspondences(src, tgt, r)
        for edge in (None, r, 0.1, 0.5):
            i, d2 = ops.NNGrid(_t(tgt), edge).correspondences(_t(src), r)
            i, d2 = i.cpu().numpy(), d2.cpu().numpy()
            assert np.array_equal(i, want_i), (r, edge, int((i != want_i).sum()))
            assert _same_bits(d2, want_d), (r, edge)
    # a source exactly at r = 0.125 from its only target within reach gets none
    i, _ = ops.NNGrid(_t(np.array([[0.0, 0.0, 0.0], [5.0, 5.0, 5.0]])), 0.125).correspondences(_t(np.array([[0.125, 0.0, 0.0]])), 0.125)
    assert int(i[0]) == -1


def _target(step, knn=30):
    from loner_amd import ops
    tgt = IR.box_scene(step)
    normals = ops.NNGrid(_t(tgt)).normals(knn).cpu().numpy()
    return tgt, normals


def test_one_round_matches_the_restatement():
    from loner_amd import ops
    tgt, normals = _target(0.2)
    T = IR.rigid(0.2, [0.02, -0.01, 0.015])
    rng = np.random.default_rng(4)
    src = tgt[::3] @ T[:3, :3].T + T[:3, 3] + rng.normal(size=(len(tgt[::3]), 3)) * 0.005
    out = ops.icp_point_to_plane(ops.NNGrid(_t(tgt), 0.125), _t(normals), _t(src), 0.125, max_iteration=1)
    idx, _ = IR.correspondences_grid(src, tgt, 0.125)
    JTJ, JTr, k = IR.system(src, tgt, normals, idx)
    assert out["system_correspondences"] == k
    assert np.abs(out["JTJ"] - JTJ).max() <= 1e-12 * np.abs(JTJ).max()
    assert np.abs(out["JTr"] - JTr).max() <= 1e-12 * np.abs(JTr).max()
    x = IR.ldlt_solve(JTJ, -JTr)
    assert np.abs(out["x"] - x).max() <= 1e-12
    assert np.abs(out["transformation"] - IR.step_matrix(x)).max() <= 1e-12


def test_known_rigid_motion_is_recovered():
    """box and sphere at 0.05 m (target, GPU normals); source every third target point moved by 0.2 deg and 2 cm.  Noiseless: T^-1 to
    1e-8, fitness 1; two runs bit-identical.  With 5 mm noise on the 0.2 m scene: the restatement's transformation and fitness.
    First measurement: 1 449 884 targets, 483 295 sources, fitness 1, RMSE 3.9e-15 after 3 rounds."""
    from loner_amd.analysis.lidar_map import PointCloud, registration_icp
    tgt, normals = _target(0.05)
    T = IR.rigid(0.2, [0.02, -0.01, 0.015])
    src = tgt[::3] @ T[:3, :3].T + T[:3, 3]
    target = PointCloud(tgt, DEV)
    target.normals = _t(normals)
    a = registration_icp(PointCloud(src, DEV), target, 0.125, max_iteration=30)
    b = registration_icp(PointCloud(src, DEV), target, 0.125, max_iteration=30)
    print(f"{len(tgt)} targets, {len(src)} sources: fitness {a.fitness}, rmse {a.inlier_rmse:.3g}, {a.iterations} rounds")
    assert np.abs(a.transformation - np.linalg.inv(T)).max() < 1e-8
    assert a.fitness == 1.0 and a.inlier_rmse < 1e-8
    assert _same_bits(a.transformation, b.transformation) and a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse

    tgt, normals = _target(0.2)
    rng = np.random.default_rng(5)
    src = tgt[::3] @ T[:3, :3].T + T[:3, 3] + rng.normal(size=(len(tgt[::3]), 3)) * 0.005
    target = PointCloud(tgt, DEV)
    target.normals = _t(normals)
    got = registration_icp(PointCloud(src, DEV), target, 0.125, max_iteration=10, relative_fitness=1e-12, relative_rmse=1e-12)
    want = IR.icp(src, tgt, normals, 0.125, max_iteration=10, relative_fitness=1e-12, relative_rmse=1e-12, corr=IR.correspondences_grid)
    assert np.abs(got.transformation - want["transformation"]).max() < 1e-10
    assert got.fitness == want["fitness"] and abs(got.inlier_rmse - want["inlier_rmse"]) < 1e-12


def test_refined_evaluation_end_to_end(tmp_path):
    """compare_point_clouds(refine_alignment=True) with more than 2 M points per side after down-sampling (skip 2 or more), against
    the same statistics taken by cKDTree after moving the down-sampled estimate by the ICP result; the refinement brings a
    mis-aligned estimate (0.2 deg, 3 cm) back to its noise level.  First measurement: 4 016 521 samples, 3 733 219 estimate voxels
    (alignment source 1 244 407 points, skip 3); accuracy 0.0267 -> 0.0040 m, completion 0.0271 -> 0.0049 m after 6 rounds, fitness 1,
    RMSE 0.024 m (the 2 mm noise and the voxel means)."""
    from scipy.spatial import cKDTree
    from loner_amd.analysis.lidar_map import PointCloud, compare_point_clouds
    v = 0.03
    gt = IR.box_scene(v)
    rng = np.random.default_rng(6)
    T = IR.rigid(0.2, [0.03, 0.0, -0.01])
    est = gt @ T[:3, :3].T + T[:3, 3] + rng.normal(size=gt.shape) * 0.002
    plain = compare_point_clouds(PointCloud(est, DEV), PointCloud(gt, DEV), str(tmp_path), 0.1, voxel_size=v)
    align = {}
    stats = compare_point_clouds(PointCloud(est, DEV), PointCloud(gt, DEV), str(tmp_path), 0.1, voxel_size=v, refine_alignment=True,
                                 alignment=align)
    print(f"{len(gt)} points; plain {plain}; refined {stats}; alignment {align}")
    est_ds = CR.voxel_down_sample(est, v)
    gt_ds = CR.voxel_down_sample(gt, v)
    assert len(est_ds) > 2_000_000 and len(gt_ds) > 2_000_000
    moved = CR.transform(est_ds, np.array(align["transformation"]))
    acc = cKDTree(gt_ds).query(moved, workers=16)[0]
    comp = cKDTree(moved).query(gt_ds, workers=16)[0]
    ref = CR.statistics(acc, comp, 0.1)
    assert stats["num_points"] == ref["num_points"] and stats["precision"] == ref["precision"] and stats["recall"] == ref["recall"]
    for k in ("accuracy", "completion", "chamfer_distance"):
        assert abs(stats[k] - ref[k]) <= 1e-12 * abs(ref[k]), k
    assert align["iterations"] >= 1 and 0.9 < align["fitness"] <= 1.0
    assert stats["accuracy"] < 0.5 * plain["accuracy"]


def test_evaluate_lidar_map_from_files(tmp_path):
    """PCD clouds, a TUM trajectory and an initial transform in tmp_path; the statistics YAML equals the restated pipeline (fp32 start
    pose inverted in fp32, restated ICP, cKDTree distances) to 1e-9."""
    import yaml
    from scipy.spatial import cKDTree
    from loner_amd.analysis.lidar_map import evaluate_lidar_map, read_pcd, write_point_cloud
    from loner_amd.common.pose_utils import build_poses_from_df
    gt = IR.box_scene(0.25)
    rng = np.random.default_rng(7)
    est = gt[rng.permutation(len(gt))[: len(gt) // 2]] + rng.normal(size=(len(gt) // 2, 3)) * 0.01
    (tmp_path / "lidar_renders").mkdir()
    write_point_cloud(str(tmp_path / "lidar_renders" / "render_full.pcd"), est)
    write_point_cloud(str(tmp_path / "gt.pcd"), gt)
    q = np.array([0.01, -0.02, 0.015, 1.0])
    rows = np.array([[0.0, 0.05, -0.03, 0.02, *q], [1.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0]])
    np.savetxt(tmp_path / "traj.txt", rows, delimiter=" ", fmt="%.10f")
    align = {}
    stats = evaluate_lidar_map(str(tmp_path), str(tmp_path / "gt.pcd"), gt_trajectory=str(tmp_path / "traj.txt"), voxel_size=0.25,
                               alignment=align)
    assert yaml.safe_load(open(tmp_path / "metrics" / "statistics.yaml")) == stats
    start = build_poses_from_df(np.loadtxt(tmp_path / "traj.txt", ndmin=2))[0][0].inverse().numpy().astype(np.float64)
    gt_w = CR.transform(read_pcd(str(tmp_path / "gt.pcd")), start)
    est_ds = CR.voxel_down_sample(read_pcd(str(tmp_path / "lidar_renders" / "render_full.pcd")), 0.25)
    gt_ds = CR.voxel_down_sample(gt_w, 0.25)
    idx, _ = IR.knn(gt_ds, 30)
    normals, _ = IR.normal_rule(IR.covariance(gt_ds, idx))
    reg = IR.icp(est_ds, gt_ds, normals, 0.125, relative_fitness=1e-12, relative_rmse=1e-12, max_iteration=10)
    assert np.abs(np.array(align["transformation"]) - reg["transformation"]).max() < 1e-9
    moved = CR.transform(est_ds, reg["transformation"])
    ref = CR.statistics(cKDTree(gt_ds).query(moved)[0], cKDTree(moved).query(gt_ds)[0], 0.1)
    for k in ref:
        assert abs(stats[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), k
    # initial_transform: the same inverse rule on torch.tensor(list) (fp32)
    T0 = np.eye(4)
    T0[:3, 3] = [0.05, -0.03, 0.02]
    s2 = evaluate_lidar_map(str(tmp_path), str(tmp_path / "gt.pcd"), initial_transform=T0.reshape(-1).tolist(), voxel_size=0.25)
    assert s2["num_points"] == stats["num_points"]


def test_errors_and_empty_clouds():
    from loner_amd import ops
    from loner_amd.analysis.lidar_map import PointCloud, registration_icp
    tgt, normals = _target(0.5)
    target = PointCloud(tgt, DEV)
    with pytest.raises(ValueError, match="normals"):
        registration_icp(PointCloud(tgt[::5], DEV), target, 0.125)
    target.normals = _t(normals)
    bad = tgt[::5].copy()
    bad[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="non-finite source"):
        registration_icp(PointCloud(bad, DEV), target, 0.125)
    bad_n = normals.copy()
    bad_n[:, 0] = np.inf
    target_bad = PointCloud(tgt, DEV)
    target_bad.normals = _t(bad_n)
    with pytest.raises(RuntimeError, match="non-finite target normals"):
        registration_icp(PointCloud(tgt[::5], DEV), target_bad, 0.125)
    with pytest.raises(RuntimeError, match="non-finite"):
        PointCloud(bad, DEV).estimate_normals()
    r = registration_icp(PointCloud(np.zeros((0, 3)), DEV), target, 0.125)
    assert r.fitness == 0.0 and r.inlier_rmse == 0.0 and np.array_equal(r.transformation, np.eye(4))
    empty = PointCloud(np.zeros((0, 3)), DEV)
    empty.estimate_normals()
    r = registration_icp(PointCloud(tgt[::5], DEV), empty, 0.125)
    assert r.fitness == 0.0 and np.array_equal(r.transformation, np.eye(4))
    with pytest.raises(ValueError):
        ops.NNGrid(_t(tgt)).normals(0)
