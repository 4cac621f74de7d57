"""The normals / ICP restatement (tests/icp_restatement.py) on hand-worked and analytic cases, build_poses_from_df, and the alignment
subset arithmetic (CPU only)."""
import numpy as np
import pytest
import torch

from tests import icp_restatement as IR


def test_step_matrix_is_scipy_zyx():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(1)
    for _ in range(50):
        x = np.concatenate([rng.uniform(-np.pi, np.pi, 3), rng.normal(size=3)])
        U = IR.step_matrix(x)
        R = Rotation.from_euler("ZYX", [x[2], x[1], x[0]]).as_matrix()
        assert np.abs(U[:3, :3] - R).max() < 1e-15
        assert np.array_equal(U[:3, 3], x[3:]) and np.array_equal(U[3], [0, 0, 0, 1])


def test_ldlt_matches_solve_and_zeroes_singular_pivots():
    rng = np.random.default_rng(2)
    for _ in range(50):
        M = rng.normal(size=(6, 6))
        A = M @ M.T + 1e-3 * np.eye(6)
        b = rng.normal(size=6)
        want = np.linalg.solve(A, b)
        assert np.abs(IR.ldlt_solve(A, b) - want).max() <= 1e-9 * np.abs(want).max()
    # exactly singular: a zero row and column gives a zero component, the rest is the reduced solve
    A = np.diag([4.0, 0.0, 9.0, 1.0, 2.0, 0.5])
    A[0, 2] = A[2, 0] = 1.0
    b = np.array([1.0, 3.0, 2.0, -1.0, 4.0, 0.25])
    x = IR.ldlt_solve(A, b)
    assert x[1] == 0.0
    keep = [0, 2, 3, 4, 5]
    assert np.allclose(x[keep], np.linalg.solve(A[np.ix_(keep, keep)], b[keep]), rtol=1e-14)
    assert np.array_equal(IR.ldlt_solve(np.zeros((6, 6)), b), np.zeros(6))


def test_restated_icp_recovers_a_rigid_motion():
    """the box-and-sphere scene at 0.2 m with normals; every third point moved by 0.2 deg and 2 cm comes back to about 1e-9"""
    tgt = IR.box_scene(0.2)
    idx, _ = IR.knn(tgt, 30)
    C = IR.covariance(tgt, idx)
    normals, _ = IR.normal_rule(C)
    T = IR.rigid(0.2, [0.02, -0.01, 0.015])
    src = (tgt[::3] @ T[:3, :3].T) + T[:3, 3]
    out = IR.icp(src, tgt, normals, 0.125, max_iteration=30, relative_fitness=1e-12, relative_rmse=1e-12,
                 corr=IR.correspondences_grid)
    assert np.abs(out["transformation"] - np.linalg.inv(T)).max() < 1e-9
    assert out["fitness"] == 1.0 and out["inlier_rmse"] < 1e-9


def test_knn_covariance_and_normal_rules():
    # a regular grid: ties everywhere; the neighbour list is ordered by (d2, index)
    ax = np.arange(4) * 0.5
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    idx, d2 = IR.knn(g, 7)
    assert np.all(idx[:, 0] == np.arange(len(g))) and np.all(d2[:, 0] == 0)
    for i in range(len(g)):
        assert all((d2[i, j], idx[i, j]) < (d2[i, j + 1], idx[i, j + 1]) for j in range(6))
    # fewer than 3 neighbours: the identity, normal (0, 0, 1)
    C = IR.covariance(g[:2], IR.knn(g[:2], 30)[0])
    assert np.array_equal(C, np.tile(np.eye(3), (2, 1, 1)))
    n, exact = IR.normal_rule(C)
    assert exact.all() and np.array_equal(n, [[0, 0, 1], [0, 0, 1]])
    n, _ = IR.normal_rule(np.diag([2.0, 1.0, 3.0])[None])
    assert np.array_equal(n, [[0, 1, 0]])
    n, _ = IR.normal_rule(np.zeros((1, 3, 3)))
    assert np.array_equal(n, [[0, 0, 1]])


def test_build_poses_from_df_equals_scipy_and_keeps_the_fp32_inverse():
    from scipy.spatial.transform import Rotation
    from loner_amd.common.pose_utils import build_poses_from_df
    rng = np.random.default_rng(3)
    q = rng.normal(size=(40, 4)) * rng.uniform(0.1, 5.0, size=(40, 1))      # unnormalised quaternions
    rows = np.concatenate([np.arange(40.0)[:, None], rng.normal(size=(40, 3)) * 10, q], 1)
    poses, ts = build_poses_from_df(rows)
    assert poses.dtype == torch.float32 and np.array_equal(ts.numpy(), rows[:, 0])
    R = Rotation.from_quat(q).as_matrix()
    want = np.zeros((40, 4, 4))
    want[:, :3, :3] = R
    want[:, :3, 3] = rows[:, 1:4]
    want[:, 3, 3] = 1
    assert np.abs(poses.numpy().astype(np.float64) - want.astype(np.float32)).max() <= 1e-6

    class Frame:                                   # anything with .to_numpy() (a DataFrame)
        def to_numpy(self, dtype=None):
            return rows.astype(dtype)
    assert torch.equal(build_poses_from_df(Frame())[0], poses)
    inv = poses[0].inverse()                       # the rough alignment's inverse is taken in fp32, then widened
    assert inv.dtype == torch.float32
    assert not np.array_equal(inv.numpy().astype(np.float64), np.linalg.inv(want[0]))


def test_alignment_skip_and_uniform_down_sample_arithmetic():
    from loner_amd.analysis.lidar_map import alignment_skip
    assert alignment_skip(10 ** 6) == 1 and alignment_skip(10 ** 6 + 1) == 1
    assert alignment_skip(1_999_999) == 1 and alignment_skip(2 * 10 ** 6) == 2 and alignment_skip(4_100_000) == 4
    assert alignment_skip(10) == 1 and alignment_skip(0) == 1
    n = 10 ** 6 + 1
    kept = np.arange(n)[::alignment_skip(n)]
    assert len(kept) == n
    n = 4_100_000
    kept = np.arange(n)[::alignment_skip(n)]
    assert len(kept) == 1_025_000 and np.all(kept % 4 == 0)
