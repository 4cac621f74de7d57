"""Trajectory scoring (loner_amd/analysis/trajectory.py) on cases whose answers are known: a rigidly moved trajectory, a reflected
point set, stamps outside the association bound, and three poses worked out by hand."""
import numpy as np
import pytest

from tests import slam_restatement as SR


_tum = SR.tum_rows


def _yaw(deg, xyz=(0.0, 0.0, 0.0)):
    a = np.radians(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = xyz
    return T


def _path(n=30):
    s = np.linspace(0.0, 3.0, n)
    return [_yaw(25.0 * t, (2.0 * t, np.sin(t), 0.1 * t * t)) for t in s], 0.1 * np.arange(n)


def test_a_rigidly_moved_trajectory_scores_zero_when_aligned(tmp_path):
    from loner_amd.analysis.trajectory import STATS, ape
    poses, stamps = _path()
    M = _yaw(40.0, (3.0, -2.0, 0.5)) @ np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1.0]])
    gt = _tum(stamps, poses)
    est = _tum(stamps, [M @ T for T in poses])
    aligned = ape(est, gt, align=True)
    assert aligned["pairs"] == 30 and set(STATS) <= set(aligned) and set(STATS) == set(aligned["rotation_deg"])
    assert max(aligned[k] for k in STATS) <= 1e-9
    assert aligned["rotation_deg"]["max"] <= 1e-5                  # arccos near 1 resolves 1e-8 rad
    # a pure offset, not aligned: every pose is off by exactly its length, and by no angle
    shifted = _tum(stamps, [_yaw(0.0, (0.3, -0.4, 1.2)) @ T for T in poses])
    raw = ape(shifted, gt, align=False)
    for k in ("rmse", "mean", "median", "min", "max"):
        assert raw[k] == pytest.approx(1.3, abs=1e-9)
    assert raw["std"] <= 1e-9 and raw["sse"] == pytest.approx(30 * 1.69, abs=1e-8) and raw["rotation_deg"]["max"] <= 1e-5
    assert ape(shifted, gt, align=True)["max"] <= 1e-9
    # paths are read with read_tum
    np.savetxt(tmp_path / "gt.txt", gt, delimiter=" ", fmt="%.10f")
    np.savetxt(tmp_path / "est.txt", est, delimiter=" ", fmt="%.10f")
    assert ape(str(tmp_path / "est.txt"), tmp_path / "gt.txt")["max"] <= 1e-8


def test_a_reflected_point_set_does_not_yield_a_reflection():
    from loner_amd.analysis.trajectory import umeyama_alignment
    rng = np.random.default_rng(11)
    x = rng.normal(size=(50, 3)) * [3.0, 2.0, 1.0]
    R, t, c = umeyama_alignment(x, x * [1.0, 1.0, -1.0])
    assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-12) and np.allclose(R @ R.T, np.eye(3), atol=1e-12) and c == 1.0
    # a proper rigid motion is recovered, with and without scale
    T = SR.random_rigid(rng, 4.0)
    y = 2.5 * x @ T[:3, :3].T + T[:3, 3]
    R, t, c = umeyama_alignment(x, y, with_scale=True)
    assert np.allclose(R, T[:3, :3], atol=1e-10) and np.allclose(t, T[:3, 3], atol=1e-9) and c == pytest.approx(2.5, abs=1e-10)
    R, t, c = umeyama_alignment(x, x @ T[:3, :3].T + T[:3, 3])
    assert np.allclose(R, T[:3, :3], atol=1e-10) and np.allclose(t, T[:3, 3], atol=1e-9) and c == 1.0
    with pytest.raises(ValueError):
        umeyama_alignment(x, x[:10])


def test_association_keeps_the_nearest_stamp_inside_the_bound_and_uses_none_twice():
    from loner_amd.analysis.trajectory import ape, associate
    gt = [0.0, 1.0, 2.0, 3.0]
    e, g = associate([0.02, 0.95, 1.04, 2.2, 2.91, 7.0], gt, t_max_diff=0.1)
    # 0.95 and 1.04 both want 1.0: 1.04 is nearer; 2.2 and 7.0 are outside the bound
    assert e.tolist() == [0, 2, 4] and g.tolist() == [0, 1, 3]
    e, g = associate([0.5], gt, t_max_diff=1.0)                    # a tie goes to the earlier stamp
    assert g.tolist() == [0]
    e, g = associate([], gt)
    assert len(e) == 0 and len(g) == 0
    poses, stamps = _path(10)
    with pytest.raises(ValueError):
        ape(_tum(stamps + 5.0, poses), _tum(stamps, poses))
    assert ape(_tum(np.r_[stamps[:5] + 0.03, stamps[5:] + 5.0], poses), _tum(stamps, poses), align=False)["pairs"] == 5


def test_three_poses_by_hand():
    from loner_amd.analysis.trajectory import ape
    # truth: three poses along x, no rotation; the estimate is off by (0, 3, 4) at the first (5 m), exact at the second and turned by
    # 90 degrees about z at the third.  Not aligned: errors 5, 0, 0 m and 0, 0, 90 degrees
    gt = _tum([0.0, 1.0, 2.0], [_yaw(0, (0, 0, 0)), _yaw(0, (1, 0, 0)), _yaw(0, (2, 0, 0))])
    est = _tum([0.0, 1.0, 2.0], [_yaw(0, (0, 3, 4)), _yaw(0, (1, 0, 0)), _yaw(90, (2, 0, 0))])
    got = ape(est, gt, align=False)
    want = {"rmse": np.sqrt(25.0 / 3), "mean": 5.0 / 3, "median": 0.0, "std": np.sqrt(25.0 / 3 - 25.0 / 9), "min": 0.0, "max": 5.0, "sse": 25.0}
    for k, v in want.items():
        assert got[k] == pytest.approx(v, abs=1e-12), k
    rot = got["rotation_deg"]
    assert rot["max"] == pytest.approx(90.0, abs=1e-9) and rot["mean"] == pytest.approx(30.0, abs=1e-9) and rot["median"] <= 1e-6
    assert rot["rmse"] == pytest.approx(np.sqrt(8100.0 / 3), abs=1e-9) and got["pairs"] == 3
