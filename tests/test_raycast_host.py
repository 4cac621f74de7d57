"""Ray casting without a GPU: the stated hit rule has no cracks on a closed mesh (tests/raycast_restatement.py against the analytic
slab distance of the box room), the synthetic meshes are what they claim to be, the new Python entry points refuse bad arguments
before they touch a device, and simulate_sequence writes the folder examples/run_sequence.py reads."""
import math
import os

import numpy as np
import pytest
import torch

from loner_amd.utils import synthetic as SYN
from loner_amd.utils import synthetic_mesh as SM
from tests import raycast_restatement as RR


def test_the_hit_rule_is_watertight_on_the_box_room():
    """0 misses and 1e-12 relative to the slab distance from three origins: a LiDAR pattern, every corner, two points per edge, the
    face centres, points on the face diagonals, and the axes.  (Measured: 1.5e-15; the margin covers other libm and numpy builds.)"""
    v, f = SM.box_room_mesh()
    assert v.shape == (8, 3) and f.shape == (12, 3) and f.dtype == np.int32
    rays = RR.room_rays(SYN.BOX_MIN, SYN.BOX_MAX)
    assert len(rays) == 3 * (16 * 256 + 50 + 6)
    got = RR.cast_rays(v, f, rays)
    want = RR.slab_distance(rays, SYN.BOX_MIN, SYN.BOX_MAX)
    assert got["invalid_rays"] == 0 and got["excluded_triangles"] == 0 and got["bad_index"] == 0
    misses = int((got["primitive_ids"] < 0).sum())
    rel = np.abs(got["t_hit"] - want) / want
    print(f"misses {misses}, max relative difference {rel.max():.3e}")
    assert misses == 0
    assert rel.max() <= 1e-12
    u, w = got["primitive_uvs"][:, 0], got["primitive_uvs"][:, 1]
    assert (u >= 0).all() and (w >= 0).all() and (u + w <= 1 + 1e-12).all()


def test_restatement_tie_window_and_exclusions():
    v = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [0, 0, 2], [1, 0, 2], [0, 1, 2], [np.nan, 0, 0]], dtype=np.float64)
    f = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2], [0, 1, 6], [0, 1, 9], [0, 0, 1]], dtype=np.int32)
    ray = np.array([[0.25, 0.25, 0, 0, 0, 1.0]])
    got = RR.cast_rays(v, f, ray)
    assert got["t_hit"][0] == 1.0 and got["primitive_ids"][0] == 1                 # the lower index of the duplicate
    assert got["excluded_triangles"] == 1 and got["bad_index"] == 1
    assert np.allclose(got["primitive_uvs"][0], [0.5, 0.25])                        # u weighs A, v weighs B
    assert RR.cast_rays(v, f, ray, t_min=1.5)["primitive_ids"][0] == 0             # the farther hit inside the window
    assert RR.cast_rays(v, f, ray, t_max=1.0)["primitive_ids"][0] == 1             # exactly t_max is accepted
    assert RR.cast_rays(v, f, ray, t_max=np.nextafter(1.0, 0.0))["primitive_ids"][0] == -1
    bad = np.array([[0, 0, 0, 0, 0, 0], [np.nan, 0, 0, 0, 0, 1], [0, 0, 0, np.inf, 0, 1]], dtype=np.float64)
    got = RR.cast_rays(v, f, bad)
    assert got["invalid_rays"] == 3 and (got["primitive_ids"] == -1).all() and np.isinf(got["t_hit"]).all()


def test_synthetic_meshes_are_closed_and_on_their_surfaces():
    def closed(f):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        und, count = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
        directed = {(int(a), int(b)) for a, b in e}
        return (count == 2).all() and all((b, a) in directed for a, b in directed)      # every edge once each way

    v, f = SM.box_room_mesh()
    assert closed(f) and (v.min(0) == SYN.BOX_MIN).all() and (v.max(0) == SYN.BOX_MAX).all()
    for s, n_f in ((0, 20), (1, 80), (2, 320)):
        v, f = SM.icosphere(s, radius=3.0, centre=(8.0, 3.0, 0.0))
        assert f.shape == (n_f, 3) and len(v) == n_f // 2 + 2 and closed(f)
        assert np.abs(np.linalg.norm(v - np.array([8.0, 3.0, 0.0]), axis=1) - 3.0).max() < 1e-14
        a, b, c = (v[f[:, k]] for k in range(3))
        assert (np.einsum("na,na->n", np.cross(b - a, c - a), a - np.array([8.0, 3.0, 0.0])) > 0).all()    # wound outwards
    v, f = SM.scene_mesh(2)
    assert f.shape == (12 + 320, 3) and f.max() == len(v) - 1 and closed(f)
    with pytest.raises(ValueError):
        SM.icosphere(-1)
    with pytest.raises(ValueError):
        SM.icosphere(2, radius=0.0)


def test_trajectory_rays_restatement_inverts_the_trajectory_transform():
    """the ray's origin plus range times its direction, moved back by the restated transform's own pose, is the sensor-frame point"""
    from loner_amd.analysis.gt_map import trajectory_arrays
    rows = np.array([[0.0, 0, 0, 0, 0, 0, 0, 1], [1.0, 1, 2, 0.5, 0, 0, math.sin(0.3), math.cos(0.3)],
                     [2.0, 1, 2, 0.5, 0, 0, math.sin(0.3), math.cos(0.3)]])
    T, P, R, W = trajectory_arrays(rows)
    d = np.array([[1, 0, 0], [0, 1, 0], [0.6, 0, 0.8], [1, 0, 0], [np.nan, 0, 0]], dtype=np.float32).T.copy()
    stamps = np.array([0.0, 0.5, 1.5, 2.5, 1.0])
    rays, info = RR.trajectory_rays(d, stamps, T, P, R, W)
    assert info == dict(rays=3, outside=1, nonfinite=1)
    assert np.isnan(rays[3]).all() and np.isnan(rays[4]).all()
    assert (rays[0] == [0, 0, 0, 1, 0, 0]).all()
    assert np.allclose(rays[1, :3], [0.5, 1.0, 0.25]) and np.allclose(rays[1, 3:], [-math.sin(0.3), math.cos(0.3), 0], atol=1e-15)
    assert np.allclose(rays[2, :3], [1, 2, 0.5]) and np.allclose(np.linalg.norm(rays[2, 3:]), 1.0)


def test_stated_sine_and_cosine_are_within_two_ulps():
    rng = np.random.default_rng(0)
    for theta in list(rng.uniform(1e-9, math.pi, 20000)) + [1e-9, 1e-5, math.pi / 4, math.pi / 2, 3 * math.pi / 4, math.pi, 6.0]:
        s, c = RR.stated_sincos(theta)
        for got, want in ((s, math.sin(theta)), (c, math.cos(theta))):
            assert abs(got - want) <= 2 * max(np.spacing(abs(want)), 2.0 ** -70), theta


def test_new_entry_points_refuse_bad_arguments():
    from loner_amd import ops
    from loner_amd.analysis import lidar_sim, mesh_eval, raycast
    v, f = SM.box_room_mesh()
    with pytest.raises(ValueError):
        raycast.RaycastingScene(v[:, :2], f)
    with pytest.raises(ValueError):
        raycast.RaycastingScene(v, f.astype(np.float64))
    with pytest.raises(ValueError):
        raycast.RaycastingScene(v, f.astype(np.int64) + 2 ** 31)
    with pytest.raises(ValueError):
        raycast.RaycastingScene(object())
    with pytest.raises(RuntimeError):                           # host tensors: there is no CPU ray caster
        ops.BVH(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(ValueError):
        ops.cast_rays(None, torch.zeros(1, 6))
    with pytest.raises(RuntimeError):
        ops.trajectory_rays(torch.zeros(3, 4), torch.zeros(4), None)
    dirs, times = SYN.lidar_pattern(2, 4)

    class Scene:
        device = torch.device("cpu")

    for bad in (dict(directions=dirs.double()), dict(directions=dirs.T.contiguous()), dict(point_times=times[:-1]),
                dict(ray_range=(5.0, 1.0)), dict(ray_range=(-1.0, 1.0)), dict(range_sigma=-0.1), dict(range_sigma=math.nan),
                dict(seed=0.5), dict(stamp=math.inf)):
        args = dict(scene=Scene(), trajectory=None, directions=dirs, point_times=times, stamp=0.0, ray_range=(1.0, 50.0))
        args.update(bad)
        with pytest.raises(ValueError):
            lidar_sim.simulate_scan(**args)
    with pytest.raises(ValueError):
        mesh_eval.mesh_depth_l1(Scene(), Scene(), [np.eye(4)], dirs, (3.0, 1.0))
    with pytest.raises(ValueError):
        mesh_eval.mesh_depth_l1(Scene(), Scene(), [np.eye(4)], dirs.T, (1.0, 3.0))
    with pytest.raises(ValueError):
        mesh_eval.mesh_depth_l1(Scene(), Scene(), [], dirs, (1.0, 3.0))


def test_simulate_sequence_writes_the_folder_run_sequence_reads(tmp_path):
    from loner_amd.analysis import lidar_sim
    from loner_amd.common.pose_utils import read_tum
    from loner_amd.common.sensors import LidarScan
    dirs, times = SYN.lidar_pattern(2, 8)
    rows = np.array([[10.0, 0, 0, 0, 0, 0, 0, 1], [10.25, 1, 0, 0, 0, 0, math.sin(0.1), math.cos(0.1)],
                     [10.55, 1, 1, 0, 0, 0, math.sin(0.1), math.cos(0.1)]])
    calls = []

    class Scene:
        device = torch.device("cpu")

    def scan_fn(scene, trajectory, directions, point_times, stamp, ray_range, range_sigma, seed):
        calls.append((stamp, seed, trajectory.n_poses, tuple(ray_range)))
        keep = torch.ones(directions.shape[1], dtype=torch.bool)
        keep[len(calls)] = False                                 # a no-return
        dist = torch.full((int(keep.sum()),), 2.0 + len(calls))
        return LidarScan(directions[:, keep], dist, point_times[keep] + float(stamp)), keep

    out = str(tmp_path / "seq")
    stamps = lidar_sim.simulate_sequence(Scene(), rows, out, (dirs, times), scan_period=0.1, ray_range=(1.0, 50.0), seed=7, scan_fn=scan_fn)
    assert stamps == [10.0, 10.1, 10.2, 10.0 + 3 * 0.1, 10.4]    # the sweep of 0.1 s still fits before 10.55
    assert [c[1] for c in calls] == [7, 8, 9, 10, 11] and calls[0][2:] == (3, (1.0, 50.0))
    assert sorted(os.listdir(out)) == [f"{k:06d}.npy" for k in range(5)] + ["gt_tum.txt", "stamps.txt"]
    assert (np.loadtxt(os.path.join(out, "stamps.txt"), dtype=np.float64, ndmin=1) == np.asarray(stamps)).all()
    for k in range(5):
        pts = np.load(os.path.join(out, f"{k:06d}.npy"))
        keep = np.ones(16, dtype=bool)
        keep[k + 1] = False
        assert pts.dtype == np.float32 and pts.shape == (15, 4)
        assert (pts[:, :3] == (dirs.numpy().T * np.float32(3.0 + k))[keep]).all()
        assert (pts[:, 3] == times.numpy()[keep]).all()
    gt = read_tum(os.path.join(out, "gt_tum.txt"))
    assert gt.shape == (5, 8) and (gt[:, 0] == np.asarray(stamps)).all()
    assert np.allclose(gt[1, 1:4], [0.4, 0, 0]) and np.allclose(gt[4, 1:4], [1, 0.5, 0])
    assert np.allclose(np.linalg.norm(gt[:, 4:], axis=1), 1.0) and np.allclose(gt[4, 4:], rows[2, 4:])
    assert np.allclose(gt[1, 4:], [0, 0, math.sin(0.04), math.cos(0.04)])
    with pytest.raises(ValueError):                              # shorter than one sweep
        lidar_sim.simulate_sequence(Scene(), rows[:2] * [1, 1, 1, 1, 1, 1, 1, 1] - [0, 0, 0, 0, 0, 0, 0, 0], out, (dirs, times * 5), scan_fn=scan_fn)
    with pytest.raises(ValueError):
        lidar_sim.simulate_sequence(Scene(), rows, out, (dirs, times), scan_period=0.0, scan_fn=scan_fn)
    with pytest.raises(ValueError):
        lidar_sim.simulate_sequence(Scene(), rows, out, (dirs, times - 1.0), scan_fn=scan_fn)
