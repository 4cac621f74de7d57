"""Generalized ICP and the robust kernels on the MI355X against the numpy restatement (tests/gicp_restatement.py): plane covariances
bit for bit, one round's system and step for every kernel at every source size that takes another path through the sums, the full
loop, point to plane with L2 byte for byte, the source covariances' frame, outliers, degenerate inputs and the tracker's setting."""
import functools

import numpy as np
import pytest
import torch

from tests import cloud_restatement as CR
from tests import gicp_restatement as GR
from tests import icp_restatement as IR

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-3
KNN = 20
R = 0.5
KERNELS = (("l2", 1.0), ("huber", 1.0), ("cauchy", 1.0), ("tukey", 3.0))
MOVE = IR.rigid(2, (0.05, -0.03, 0.02))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _kernel(kind, k):
    from loner_amd.analysis.registration import RobustKernel
    return RobustKernel(kind, k)


def _normals_and_covariances(points):
    """GPU normals (knn 20) and their plane covariances, as numpy: the restatement takes the device's normals, as test_gpu_icp.py's"""
    from loner_amd import ops
    from loner_amd.analysis.registration import plane_covariances
    normals = ops.NNGrid(_t(points)).normals(KNN)
    return normals.cpu().numpy(), plane_covariances(normals, EPS).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene(target_step, source_step, noise_seed=None):
    """target box_scene(target_step); source box_scene(source_step) moved by MOVE (plus 5 mm noise with a seed), with the device's
    normals and covariances of both.  Computed once and shared: the arrays are read, never written.
    box_scene samples every edge of the box once per face, and the copies differ in their last bits and carry different normals.  A
    source beside an edge is then as near to one copy as to the other within rounding, and a loop of several rounds, which the device
    and numpy walk with differently rounded sums, may take the other copy.  The noisy scene, which the multi-round comparisons use,
    therefore keeps the first copy of each target only."""
    tgt = IR.box_scene(target_step)
    base = IR.box_scene(source_step)
    src = base @ MOVE[:3, :3].T + MOVE[:3, 3]
    if noise_seed is not None:
        src = src + np.random.default_rng(noise_seed).normal(size=src.shape) * 0.005
        tgt = tgt[np.sort(np.unique(np.round(tgt, 6), axis=0, return_index=True)[1])]
    tn, tc = _normals_and_covariances(tgt)
    sn, sc = _normals_and_covariances(src)
    return {"tgt": tgt, "tn": tn, "tc": tc, "src": src, "sn": sn, "sc": sc}


def test_plane_covariances_are_bit_identical_to_the_restatement():
    from loner_amd.analysis.registration import plane_covariances
    rng = np.random.default_rng(31)
    n = rng.normal(size=(10_000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:3] = np.eye(3)
    n[3:6] = -np.eye(3)
    n[6] = [np.nan, 0.0, 1.0]
    for eps in (EPS, 1e-9):
        got = plane_covariances(_t(n), eps).cpu().numpy()
        want = GR.plane_covariances(n, eps)
        ok = np.arange(len(n)) != 6                                       # a NaN's sign and payload are not part of the definition
        assert _same_bits(got[ok], want[ok]), f"{int((got[ok] != want[ok]).any((1, 2)).sum())} covariances differ"
        assert np.array_equal(np.isnan(got[6]), np.isnan(want[6])) and np.isnan(got[6]).any() and np.isfinite(got[ok]).all()
        assert np.array_equal(got[6][~np.isnan(got[6])], want[6][~np.isnan(want[6])])
        assert _same_bits(got[:3], got[3:6])                              # the sign of the normal does not matter
    assert plane_covariances(_t(np.zeros((0, 3))), EPS).shape == (0, 3, 3)


def _one_round_case(size):
    """(target, target covariances, target normals, source, source covariances): 1, 63 and 257 sources spread over the 0.46 m scene;
    "grid": 600 000 jittered copies of them against the 0.8 m scene, more than 2048 blocks of 256, so that a thread sums several."""
    if size == "grid":
        sc = _scene(0.8, 0.46)
        rng = np.random.default_rng(32)
        pick = rng.integers(0, len(sc["src"]), 600_000)
        return sc["tgt"], sc["tc"], sc["tn"], sc["src"][pick] + rng.normal(size=(len(pick), 3)) * 0.01, sc["sc"][pick]
    sc = _scene(0.4, 0.46)
    pick = ((np.arange(size) + 0.5) * len(sc["src"]) / size).astype(np.int64)
    return sc["tgt"], sc["tc"], sc["tn"], sc["src"][pick], sc["sc"][pick]


@pytest.mark.parametrize("size", [1, 63, 257, "grid"])
def test_one_round_matches_the_restatement(size):
    """max_iteration=1 from the identity: the solved system is the first round's.  JTJ and JTr to 1e-12 of their largest entry, x and
    the step matrix to 1e-12 (test_gpu_icp.py's tolerances for the same sums), for every kernel, and for point to plane with the
    three robust kernels."""
    from loner_amd import ops
    from loner_amd.analysis.registration import icp_generalized, icp_point_to_plane_robust
    tgt, tc, tn, src, sc = _one_round_case(size)
    grid = ops.NNGrid(_t(tgt), R)
    if size == "grid":                  # the search itself is test_gpu_icp.py's subject: bit-identical to brute force
        idx = grid.correspondences(_t(src), R)[0].cpu().numpy().astype(np.int64)
    else:
        idx = IR.correspondences(src, tgt, R)[0]
    assert (idx >= 0).sum() >= 1
    for kind, k in KERNELS:
        out = icp_generalized(grid, _t(tc), _t(src), _t(sc), R, max_iteration=1, kernel=_kernel(kind, k))
        JTJ, JTr, n, skipped = GR.system(src, tgt, tc, sc, np.eye(3), idx, kind, k)
        dJ, dr = np.abs(out["JTJ"] - JTJ).max() / np.abs(JTJ).max(), np.abs(out["JTr"] - JTr).max() / np.abs(JTr).max()
        x = IR.ldlt_solve(JTJ, -JTr)
        dx, dT = np.abs(out["x"] - x).max(), np.abs(out["transformation"] - IR.step_matrix(x)).max()
        print(f"{size} {kind}: {n} correspondences, JTJ {dJ:.3g}, JTr {dr:.3g}, x {dx:.3g}, step {dT:.3g}")
        assert skipped == 0 and out["system_correspondences"] == n
        assert dJ <= 1e-12 and dr <= 1e-12, (kind, dJ, dr)
        assert dx <= 1e-12 and dT <= 1e-12, (kind, dx, dT)
    if size in (1, "grid"):
        return                          # one point-to-plane row leaves five directions free; the grid case's sums are the same code
    for kind, k in (("huber", 0.01), ("cauchy", 0.01), ("tukey", 0.05)):
        out = icp_point_to_plane_robust(grid, _t(tn), _t(src), R, max_iteration=1, kernel=_kernel(kind, k))
        JTJ, JTr, n = GR.plane_system(src, tgt, tn, idx, kind, k)
        assert out["system_correspondences"] == n
        assert np.abs(out["JTJ"] - JTJ).max() <= 1e-12 * np.abs(JTJ).max() and np.abs(out["JTr"] - JTr).max() <= 1e-12 * np.abs(JTr).max()
        x = IR.ldlt_solve(JTJ, -JTr)
        assert np.abs(out["x"] - x).max() <= 1e-12 and np.abs(out["transformation"] - IR.step_matrix(x)).max() <= 1e-12, kind


@pytest.mark.parametrize("kind,k", [("l2", 1.0), ("tukey", 3.0)])
def test_full_loop_matches_the_restatement(kind, k):
    """0.4 m target, 0.46 m source with 5 mm noise, 10 rounds with criteria 1e-12: the transformation to 1e-10, equal fitness, RMSE to
    1e-12, and two runs return the same bytes."""
    from loner_amd.analysis.lidar_map import PointCloud
    from loner_amd.analysis.registration import registration_generalized_icp
    sc = _scene(0.4, 0.46, 33)
    target, source = PointCloud(sc["tgt"], DEV), PointCloud(sc["src"], DEV)
    target.covariances, source.covariances = _t(sc["tc"]), _t(sc["sc"])
    run = lambda: registration_generalized_icp(source, target, R, np.eye(4), 1e-12, 1e-12, 10, _kernel(kind, k))
    a, b = run(), run()
    want = GR.gicp(sc["src"], sc["tgt"], sc["tc"], sc["sc"], R, relative_fitness=1e-12, relative_rmse=1e-12, max_iteration=10, kind=kind, k=k,
                   corr=IR.correspondences_grid)
    dT = np.abs(a.transformation - want["transformation"]).max()
    err = np.linalg.norm(a.transformation[:3, 3] - np.linalg.inv(MOVE)[:3, 3])
    print(f"{kind}: {a.iterations} rounds, fitness {a.fitness:.6f}, rmse {a.inlier_rmse:.6g}, |dT| {dT:.3g}, translation error {err * 1e3:.3f} mm")
    assert dT < 1e-10
    assert a.fitness == want["fitness"] and abs(a.inlier_rmse - want["inlier_rmse"]) < 1e-12 and a.iterations == want["iterations"]
    assert _same_bits(a.transformation, b.transformation) and a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse


def test_point_to_plane_with_l2_returns_the_plain_entry_points_bytes():
    from loner_amd import ops
    from loner_amd.analysis import registration as RG
    sc = _scene(0.4, 0.46, 33)
    grid = ops.NNGrid(_t(sc["tgt"]), R)
    args = (grid, _t(sc["tn"]), _t(sc["src"]), None, R, np.eye(4), 1e-12, 1e-12, 10)
    res0, info0 = RG._run("plane", *args, None)
    for kernel in (RG.RobustKernel(), RG.RobustKernel("l2", 7.0)):
        res1, info1 = RG._run("plane_robust", *args, kernel)
        assert res1.shape == (64,) and _same_bits(res0, res1) and np.array_equal(info0, info1)
    assert info0[0] == 0 and info0[2] >= 2 and info0[7] == 0
    res2, _ = RG._run("plane_robust", *args, RG.RobustKernel("huber", 0.01))
    assert not _same_bits(res0[:16], res2[:16])                           # a weight does change the estimate


def test_source_covariances_follow_the_accumulated_transformation():
    """A source held in a frame rotated by 25 degrees, with its covariances in that frame: registering it with init = T0 equals
    registering the cloud moved by PointCloud.transform(T0) (points and R C R^T) from the identity, to 1e-10.  Leaving the
    covariances unrotated gives another answer, so the agreement shows that R comes from the accumulated transformation."""
    from loner_amd.analysis.lidar_map import PointCloud
    from loner_amd.analysis.registration import registration_generalized_icp
    sc = _scene(0.4, 0.46, 33)
    T0 = IR.rigid(25, (0.3, -0.2, 0.1), axis=(0.5, 0.4, -0.7))
    back = np.linalg.inv(T0)
    own = sc["src"] @ back[:3, :3].T + back[:3, 3]
    own_cov = np.einsum("ab,nbc,dc->nad", back[:3, :3], sc["sc"], back[:3, :3])
    target = PointCloud(sc["tgt"], DEV)
    target.covariances = _t(sc["tc"])

    def source(cov):
        cloud = PointCloud(own, DEV)
        cloud.covariances = _t(cov)
        return cloud

    a = registration_generalized_icp(source(own_cov), target, R, T0, 1e-12, 1e-12, 10)
    b = registration_generalized_icp(source(own_cov).transform(T0), target, R, np.eye(4), 1e-12, 1e-12, 10)
    d = np.abs(a.transformation - b.transformation @ T0).max()
    wrong = registration_generalized_icp(source(sc["sc"]), target, R, T0, 1e-12, 1e-12, 10)       # covariances of the other frame
    dw = np.abs(a.transformation - wrong.transformation).max()
    print(f"init = T0 against the pre-transformed cloud: {d:.3g}; with covariances of the wrong frame: {dw:.3g}")
    assert d < 1e-10 and a.fitness == b.fitness
    assert dw > 1e-7


def test_tukey_halves_the_error_that_outliers_cause():
    """0.2 m target, 0.23 m source with 5 mm noise, and 20 % of the source displaced by up to +-0.4 m per axis (seed 22); covariances
    from normals estimated on the contaminated source, 30 rounds.  Tukey (k = 3 on the Mahalanobis residual) ends at no more than half
    of L2's translation error.  The restatement alone, with numpy's eigenvectors for the normals: L2 1.782 mm, Tukey 0.235 mm (7.6 x),
    Huber k=1 0.532 mm, Cauchy k=1 0.135 mm; seed 21: 1.015 and 0.227 mm (4.5 x); the 0.4 m scene: 4.0 x and 4.7 x."""
    from loner_amd.analysis.lidar_map import PointCloud
    from loner_amd.analysis.registration import registration_generalized_icp
    rng = np.random.default_rng(22)
    tgt, base = IR.box_scene(0.2), IR.box_scene(0.23)
    src = base @ MOVE[:3, :3].T + MOVE[:3, 3] + rng.normal(size=base.shape) * 0.005
    hit = rng.random(len(src)) < 0.2
    src[hit] += rng.uniform(-0.4, 0.4, size=(int(hit.sum()), 3))
    source, target = PointCloud(src, DEV), PointCloud(tgt, DEV)
    truth = np.linalg.inv(MOVE)[:3, 3]
    err = {}
    for kind, k in (("l2", 1.0), ("tukey", 3.0)):
        reg = registration_generalized_icp(source, target, R, kernel=_kernel(kind, k), epsilon=EPS, knn=KNN)
        err[kind] = float(np.linalg.norm(reg.transformation[:3, 3] - truth))
        print(f"{kind}: translation error {err[kind] * 1e3:.3f} mm after {reg.iterations} rounds, fitness {reg.fitness:.4f}")
    assert source.covariances is None and source.normals is None and target.covariances is None and target.normals is None
    assert err["tukey"] <= 0.5 * err["l2"]


def test_map_alignment_takes_a_kernel():
    """refine_alignment_icp with a 10 % share of floaters (up to +-0.1 m, inside the 0.125 m reach): None is the plain call's bytes,
    L2 as a kernel too, and Tukey at 0.03 m, which ignores what lies off the surface, ends nearer the motion that was applied.  The
    floaters lie on one side (0 .. 0.1 m per axis), a mean pull of 10 % x 0.05 m per axis on L2; Tukey keeps the 30 % of them below
    0.03 m at reduced weight.  The restatement alone: L2 7.89 mm, Tukey 0.26 mm."""
    from loner_amd.analysis.lidar_map import PointCloud, refine_alignment_icp, registration_icp
    gt = IR.box_scene(0.25)
    rng = np.random.default_rng(35)
    T = IR.rigid(0.2, [0.03, 0.0, -0.01])
    est = gt @ T[:3, :3].T + T[:3, 3] + rng.normal(size=gt.shape) * 0.002
    hit = rng.random(len(est)) < 0.1
    est[hit] += rng.uniform(0.0, 0.1, size=(int(hit.sum()), 3))                   # one-sided, so that L2 is pulled along
    clouds = lambda: (PointCloud(est, DEV), PointCloud(gt, DEV))
    plain = refine_alignment_icp(*clouds())
    target = PointCloud(gt, DEV).estimate_normals(30)
    direct = registration_icp(PointCloud(est, DEV), target, 0.125, np.eye(4), 1e-12, 1e-12, 10)
    l2 = refine_alignment_icp(*clouds(), kernel=_kernel("l2", 1.0))
    tukey = refine_alignment_icp(*clouds(), kernel=_kernel("tukey", 0.03))
    assert _same_bits(plain.transformation, direct.transformation) and _same_bits(plain.transformation, l2.transformation)
    err = lambda reg: float(np.linalg.norm(reg.transformation[:3, 3] - np.linalg.inv(T)[:3, 3]))
    print(f"translation error: L2 {err(plain) * 1e3:.3f} mm, Tukey {err(tukey) * 1e3:.3f} mm")
    assert err(tukey) < err(plain)


def test_degenerate_inputs():
    from loner_amd import ops
    from loner_amd.analysis import registration as RG
    from loner_amd.analysis.lidar_map import PointCloud
    sc = _scene(0.4, 0.46)
    target, source = PointCloud(sc["tgt"], DEV), PointCloud(sc["src"][::7], DEV)
    target.covariances, source.covariances = _t(sc["tc"]), _t(sc["sc"][::7])
    empty = PointCloud(np.zeros((0, 3)), DEV)
    for a, b in ((empty, target), (source, empty)):
        reg = RG.registration_generalized_icp(a, b, R, kernel=_kernel("tukey", 3.0))
        assert reg.fitness == 0.0 and reg.inlier_rmse == 0.0 and np.array_equal(reg.transformation, np.eye(4))
    # all-zero covariances: every M is singular; the status bit, the count, the transformation stays init, nothing is NaN
    grid = ops.NNGrid(target.points, R)
    zt, zs = torch.zeros_like(target.covariances), torch.zeros_like(source.covariances)
    res, info = RG._run("generalized", grid, zt, source.points, zs, R, MOVE, 1e-6, 1e-6, 5, RG.RobustKernel())
    n_corr = int((IR.correspondences(CR.transform(sc["src"][::7], MOVE), sc["tgt"], R)[0] >= 0).sum())
    assert info[0] == 16 and info[7] == n_corr > 0 and info[2] == 0
    assert np.isfinite(res).all() and np.array_equal(res[:16].reshape(4, 4), MOVE)
    with pytest.raises(RuntimeError, match="covariance"):
        RG.icp_generalized(grid, zt, source.points, zs, R)
    nan_cov = target.covariances.clone()
    nan_cov[:, 0, 0] = float("nan")
    with pytest.raises(RuntimeError, match="covariance"):
        RG.icp_generalized(grid, nan_cov, source.points, source.covariances, R)
    bad = sc["src"][::7].copy()
    bad[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="non-finite source"):
        RG.icp_generalized(grid, target.covariances, _t(bad), source.covariances, R)
    with pytest.raises(ValueError):
        RG.registration_generalized_icp(source, target, R, kernel=_kernel("huber", 0.0))

    class Zero:                         # past RobustKernel's own check: the library refuses it too
        code, k = 1, 0.0
    with pytest.raises(RuntimeError, match="kernel_k"):
        RG._run("generalized", grid, target.covariances, source.points, source.covariances, R, None, 1e-6, 1e-6, 5, Zero)
    with pytest.raises(ValueError, match="covariances"):
        RG.icp_generalized(grid, target.covariances[:5], source.points, source.covariances, R)


def test_tracker_with_generalized_estimation():
    """Two motion-distorted 32 x 512 frames.  With icp.estimation = GENERALIZED every stage equals registration_generalized_icp called
    by hand on the frame clouds (knn 20, epsilon 1e-3, each stage from the one before), byte for byte, and the reference cloud keeps
    the covariances it was built with; with the default settings the stages are registration_icp's bytes."""
    from loner_amd.analysis.lidar_map import PointCloud, registration_icp
    from loner_amd.analysis.registration import registration_generalized_icp
    from loner_amd.common.frame import Frame
    from loner_amd.common.sensors import LidarScan
    from loner_amd.common.settings import default_tracking_settings
    from loner_amd.common.signals import Signal
    from loner_amd.tracking.tracker import Tracker
    from tests import track_restatement as TR
    scans = [TR.distorted_scan(k, 32, 512) for k in range(2)]

    def track(**icp):
        settings = default_tracking_settings()
        settings["tracker"]["icp"].update(icp)
        settings["tracker"]["motion_compensation"]["enabled"] = False
        tracker = Tracker(settings, Signal(), Signal(), Signal(), device=DEV)
        clouds = []
        for dirs, dist, ts in scans:
            frame = Frame(None, LidarScan(dirs.clone(), dist.clone(), ts.clone())).to(DEV)
            clouds.append(tracker.frame_cloud(frame).numpy())
            assert tracker.track_frame(frame)
        return tracker, clouds, settings["tracker"]["icp"]["schedule"]

    def by_hand(register, clouds, schedule, **kw):
        init, out = np.eye(4), []
        for stage in schedule:
            out.append(register(PointCloud(clouds[1], DEV), clouds[0], stage["threshold"], init, stage["relative_fitness"],
                                stage["relative_rmse"], stage["max_iterations"], **kw))
            init = out[-1].transformation.copy()
        return out

    def same(got, want):
        assert len(got) == len(want) == 2
        for g, w in zip(got, want):
            assert _same_bits(g.transformation, w.transformation) and g.fitness == w.fitness and g.inlier_rmse == w.inlier_rmse
            assert g.iterations == w.iterations >= 1

    tracker, clouds, schedule = track(estimation="GENERALIZED", robust_kernel={"type": "TUKEY", "k": 3.0})
    ref = tracker._reference_point_cloud
    assert ref.covariances is not None and ref.normals is None and _same_bits(ref.numpy(), clouds[1])
    same(tracker.last_registrations, by_hand(lambda s, t, *a, **kw: registration_generalized_icp(s, PointCloud(t, DEV), *a, **kw), clouds,
                                             schedule, kernel=_kernel("tukey", 3.0), epsilon=1e-3, knn=20))
    plain, clouds_p, _ = track()
    assert _same_bits(clouds_p[1], clouds[1]) and plain._reference_point_cloud.has_normals()
    target = PointCloud(clouds_p[0], DEV).estimate_normals(30)
    same(plain.last_registrations, by_hand(lambda s, t, *a: registration_icp(s, target, *a), clouds_p, schedule))
    assert not _same_bits(plain.last_registrations[-1].transformation, tracker.last_registrations[-1].transformation)
