"""Segmentation on the MI355X against the numpy restatement (tests/segment_restatement.py): radius counts, DBSCAN labels, the RANSAC
plane's choice, mask and hypothesis model bit for bit; the refitted model to 1e-9 (below).  The restated neighbour lists are computed
once per (scene, radius) and shared.

The refit's bound: the cumulants and the covariance are restated in the device's order, but the device's FastEigen3x3 goes through the
library's acos and cos, which are not correctly rounded, and the restatement takes numpy.linalg.eigh.  Both eigenvectors carry an
error of a few ulp of the covariance divided by the gap between the two smallest eigenvalues, here 1e-16 / 0.3; 1e-9 is the bound the
issue sets for the same normal against an SVD, and it is far above either error."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from loner_amd.analysis import segmentation as SEG
from tests import segment_restatement as SR

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _cloud(p):
    from loner_amd.analysis.lidar_map import PointCloud
    return PointCloud(_t(np.asarray(p, dtype=np.float64).reshape(-1, 3)))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def _blobs(shifted=False):
    p = SR.blobs_scene()
    return p + SR.SHIFT if shifted else p


@functools.lru_cache(maxsize=None)
def _blob_neighbours(eps, shifted=False):
    return SR.radius_neighbours(_blobs(shifted), eps)


def _dbscan(p, eps, min_points):
    info = {}
    labels = _cloud(p).cluster_dbscan(eps, min_points, info=info)
    assert labels.dtype == torch.int32 and labels.is_cuda
    return labels.cpu().numpy(), info


# ---------------------------------------------------------------- counts
@pytest.mark.parametrize("shifted", [False, True])
def test_radius_counts_equal_the_restatement_at_any_radius_and_edge(shifted):
    from loner_amd import ops
    p = _blobs(shifted)
    grid = ops.NNGrid(_t(p))
    other = ops.NNGrid(_t(p), 0.37 * grid.edge)
    wide = ops.NNGrid(_t(p), 2.9 * grid.edge)
    for f in (0.5, 1.0, 3.0):
        r = f * grid.edge
        want = SR.radius_counts(p, r)
        stats = {}
        got = SEG.radius_count(grid, r, stats=stats).cpu().numpy()
        print(f"shifted {shifted}, r = {f} x {grid.edge:.4f}: counts up to {want.max()}, mean {want.mean():.1f}, {stats['shells']} shells walked")
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert want.max() >= 64 and want.min() >= 1                 # the 64 copies count one another; every point counts itself
        assert np.array_equal(SEG.radius_count(other if f < 3 else wide, r).cpu().numpy(), want)
    own = ops.NNGrid(_t(p), grid.edge)                               # edge == radius: the wrappers' choice
    assert np.array_equal(SEG.radius_count(own, grid.edge).cpu().numpy(), SR.radius_counts(p, grid.edge))


# ---------------------------------------------------------------- DBSCAN
@pytest.mark.parametrize("eps,min_points", SR.RANDOM_SETTINGS)
def test_dbscan_labels_and_info_equal_the_sequential_algorithm(eps, min_points):
    p = _blobs()
    want, winfo = SR.dbscan(p, eps, min_points, _blob_neighbours(eps))
    got, info = _dbscan(p, eps, min_points)
    print(f"eps {eps}, min_points {min_points}: {info}")
    assert np.array_equal(got, want) and info == winfo
    again, _ = _dbscan(p, eps, min_points)
    assert got.tobytes() == again.tobytes()
    # a permuted input: the same partition, and the labels the permuted smallest-core rule implies
    perm = np.random.default_rng(5).permutation(len(p))
    got_p, info_p = _dbscan(p[perm], eps, min_points)
    want_p, winfo_p = SR.dbscan(p[perm], eps, min_points)
    assert np.array_equal(got_p, want_p) and info_p == winfo_p
    assert {k: info_p[k] for k in ("clusters", "cores", "noise")} == {k: info[k] for k in ("clusters", "cores", "noise")}
    core = np.array([len(x) >= min_points for x in _blob_neighbours(eps)])
    a, b = got[perm][core[perm]], got_p[core[perm]]                  # the cores' labels, the same points side by side
    pairs = set(zip(a.tolist(), b.tolist()))
    assert len(pairs) == info["clusters"] and len({x for x, _ in pairs}) == len({y for _, y in pairs}) == info["clusters"]
    assert np.array_equal(got[perm] == -1, got_p == -1)              # noise is noise in any order


_CHAIN = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from loner_amd.analysis.lidar_map import PointCloud
from tests import segment_restatement as SR
info = {{}}
labels = PointCloud(torch.from_numpy(SR.chain_scene()).to("cuda")).cluster_dbscan(0.1, 3, info=info)
np.save({out!r}, np.concatenate([labels.cpu().numpy(), [info[k] for k in ("clusters", "cores", "border", "noise")]]))
"""


def test_dbscan_unites_a_chain_across_many_workgroups(tmp_path):
    """3 000 points on a line in shuffled order: one cluster through a long chain of hooks between workgroups.  It runs in a process
    of its own under a time limit: a union-find that read a stale parent would not come back."""
    out = str(tmp_path / "chain.npy")
    try:
        r = subprocess.run([sys.executable, "-c", _CHAIN.format(root=ROOT, out=out)], timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.exit("the DBSCAN chain case did not come back within 120 s: nothing more is started on the device", returncode=1)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    n = 3000
    assert got[n:].tolist() == [1, n - 2, 2, 0]
    assert np.array_equal(got[:n], np.zeros(n, dtype=np.int64))
    assert np.array_equal(got[:n], SR.dbscan(SR.chain_scene(), 0.1, 3)[0])


def test_dbscan_is_strict_at_the_threshold():
    p = SR.lattice_scene()
    got, info = _dbscan(p, 0.25, 2)
    assert np.all(got == -1) and info == {"clusters": 0, "cores": 0, "border": 0, "noise": len(p)}
    got, info = _dbscan(p, float(np.nextafter(0.25, 1.0)), 2)
    assert np.all(got == 0) and info == {"clusters": 1, "cores": len(p), "border": 0, "noise": 0}


@pytest.mark.parametrize("swap", [False, True])
def test_dbscan_border_point_between_two_clusters_takes_the_lower_label(swap):
    p = SR.border_scene(swap)
    got, info = _dbscan(p, SR.BORDER_EPS, SR.BORDER_MIN_POINTS)
    want, winfo = SR.dbscan(p, SR.BORDER_EPS, SR.BORDER_MIN_POINTS)
    assert np.array_equal(got, want) and info == winfo
    assert info["clusters"] == 2 and got[-1] == 0 and got[0] == 0 and got[11] == 1


def test_dbscan_edges():
    from loner_amd.analysis.lidar_map import PointCloud
    p = _blobs()[:3000]
    got, info = _dbscan(p, 0.5, 1)                                   # min_points = 1: no noise, the labels are components
    want, winfo = SR.dbscan(p, 0.5, 1)
    assert np.array_equal(got, want) and info == winfo and info["noise"] == 0 and info["border"] == 0 and got.min() == 0
    empty = PointCloud(torch.zeros(0, 3, dtype=torch.float64, device=DEV)).cluster_dbscan(0.5, 3)
    assert empty.shape == (0,) and empty.dtype == torch.int32
    one = np.array([[1.0, 2.0, 3.0]])
    assert _dbscan(one, 0.5, 1)[0].tolist() == [0] and _dbscan(one, 0.5, 2)[0].tolist() == [-1]
    got, info = _dbscan(_blobs()[:500], 0.01, 3)                     # all noise
    assert np.all(got == -1) and info == {"clusters": 0, "cores": 0, "border": 0, "noise": 500}
    bad = p[:100].copy()
    bad[7, 1] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):            # the grid's own refusal, as for every grid user
        _cloud(bad).cluster_dbscan(0.5, 3)
    with pytest.raises(RuntimeError, match="non-finite"):
        _cloud(bad).remove_radius_outlier(3, 0.5)


# ---------------------------------------------------------------- planes
@functools.lru_cache(maxsize=None)
def _box_reference(refine):
    return SR.segment_plane(SR.box_corner_scene(), SR.BOX_T, SR.BOX_H, 0, refine)


_INFO_KEYS = ("status", "best_hypothesis", "n_inliers", "survivors", "rejected_repeated", "rejected_degenerate", "nonfinite", "n")


@pytest.mark.parametrize("refine", [True, False])
def test_plane_of_the_box_corner(refine):
    p = SR.box_corner_scene()
    want = _box_reference(refine)
    got = SEG.plane_ransac(_t(p), SR.BOX_T, SR.BOX_H, 0, refine)
    print({k: got[k] for k in _INFO_KEYS}, got["plane"], got["hypothesis_plane"])
    assert {k: got[k] for k in _INFO_KEYS} == {k: want[k] for k in _INFO_KEYS}
    assert got["nonfinite"] == 2 and got["n"] == 4173
    assert np.array_equal(got["inlier"].cpu().numpy().astype(bool), want["inlier"])
    assert _same_bits(got["hypothesis_plane"], want["hypothesis_plane"])
    if refine:
        print("refit against the restatement:", np.abs(got["plane"] - want["plane"]).max())
        assert np.abs(got["plane"] - want["plane"]).max() < 1e-9
        assert abs(np.linalg.norm(got["plane"][:3]) - 1) < 1e-14 and got["plane"][:3] @ got["hypothesis_plane"][:3] > 0
    else:
        assert _same_bits(got["plane"], want["hypothesis_plane"])
    again = SEG.plane_ransac(_t(p), SR.BOX_T, SR.BOX_H, 0, refine)
    assert _same_bits(again["plane"], got["plane"]) and torch.equal(again["inlier"], got["inlier"])
    model, index = _cloud(p).segment_plane(SR.BOX_T, SR.BOX_H, 0, refine)
    assert _same_bits(model, got["plane"]) and index.dtype == torch.int64
    assert np.array_equal(index.cpu().numpy(), np.nonzero(want["inlier"])[0])


def test_plane_ties_go_to_the_smallest_hypothesis():
    p = SR.tie_scene()
    want = SR.segment_plane(p, 0.01, 256, 0, True)
    got = SEG.plane_ransac(_t(p), 0.01, 256, 0, False)
    assert {k: got[k] for k in _INFO_KEYS} == {k: want[k] for k in _INFO_KEYS}
    assert got["best_hypothesis"] == int(want["alive"][0]) and got["n_inliers"] == 600
    assert _same_bits(got["plane"], want["hypothesis_plane"]) and bool(got["inlier"].all())


def test_plane_degenerate_inputs():
    got = SEG.plane_ransac(_t(SR.collinear_scene()), 0.01, 256, 0, True)
    assert got["status"] == 2 and got["best_hypothesis"] == -1 and got["survivors"] == 0 and got["n_inliers"] == 0
    assert got["rejected_repeated"] + got["rejected_degenerate"] == 256
    assert not got["plane"].any() and not got["hypothesis_plane"].any() and not bool(got["inlier"].any())
    two = SEG.plane_ransac(_t(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])), 0.01, 16)
    assert two["status"] == 1 and two["n"] == 2 and not two["plane"].any() and not bool(two["inlier"].any())
    model, index = _cloud(np.zeros((0, 3))).segment_plane(0.01, 16)
    assert not model.any() and index.shape == (0,)


def test_segment_planes_finds_the_three_faces_of_the_box_corner():
    from loner_amd.analysis.segmentation import segment_planes
    p = SR.box_corner_scene()
    models, labels = segment_planes(_cloud(p), SR.BOX_T, 5, 300, num_iterations=SR.BOX_H)
    want_models, want_labels = SR.segment_planes(p, SR.BOX_T, 5, 300, SR.BOX_H)
    assert models.shape == (3, 4) and labels.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), want_labels)
    assert np.abs(models - want_models).max() < 1e-9
    axes = [int(np.abs(m[:3]).argmax()) for m in models]
    assert sorted(axes) == [0, 1, 2]
    for m, a in zip(models, axes):
        assert np.abs(np.abs(m[:3]) - np.eye(3)[a]).max() < 1e-3


# ---------------------------------------------------------------- filters
def test_filters_equal_the_restated_masks():
    p = _blobs()
    cloud = _cloud(p)
    cloud.normals = _t(np.random.default_rng(1).normal(size=p.shape))
    kept, index = cloud.remove_radius_outlier(5, 0.5)
    want = np.nonzero(SR.radius_counts(p, 0.5, _blob_neighbours(0.5)) > 5)[0]
    assert np.array_equal(index.cpu().numpy(), want) and 0 < len(want) < len(p)
    assert _same_bits(kept.numpy(), p[want]) and torch.equal(kept.normals, cloud.normals[index]) and kept.covariances is None
    eps, min_points = SR.RANDOM_SETTINGS[0]
    labels, _ = SR.dbscan(p, eps, min_points, _blob_neighbours(eps))
    for floor in (0, 40, 2000):
        kept, index = cloud.remove_small_clusters(eps, min_points, floor)
        want = np.nonzero(SR.small_cluster_mask(labels, floor))[0]
        assert np.array_equal(index.cpu().numpy(), want) and _same_bits(kept.numpy(), p[want])
    assert len(np.nonzero(SR.small_cluster_mask(labels, 40))[0]) < int((labels >= 0).sum())        # a small cluster did go


def test_compare_point_clouds_removes_a_floater_only_when_asked(tmp_path):
    from scipy.spatial import cKDTree
    from loner_amd.analysis.lidar_map import PointCloud, compare_point_clouds
    from loner_amd.utils import synthetic as SY
    from tests.test_gpu_lidar_map import _gt_cloud
    v = 0.1
    gt = _gt_cloud(v)
    rng = np.random.default_rng(3)
    est = gt + rng.normal(size=gt.shape) * 0.003
    plain = compare_point_clouds(PointCloud(est, DEV), PointCloud(gt, DEV), str(tmp_path / "a"), 0.1, voxel_size=v)
    off = compare_point_clouds(PointCloud(est, DEV), PointCloud(gt, DEV), str(tmp_path / "b"), 0.1, voxel_size=v, min_cluster_points=0,
                               cluster_eps=None)
    assert off == plain and "removed_floaters" not in off
    lo, hi = np.array(SY.BOX_MIN), np.array(SY.BOX_MAX)
    centre = lo + (hi - lo) * np.array([0.3, 0.7, 0.6])
    assert cKDTree(gt).query(centre)[0] > 0.6                        # the floater hangs in free space
    blob = centre + rng.normal(size=(30, 3)) * 0.03
    both = np.concatenate([est[:1000], blob, est[1000:]])
    dirty = compare_point_clouds(PointCloud(both, DEV), PointCloud(gt, DEV), str(tmp_path / "c"), 0.1, voxel_size=v)
    clean = compare_point_clouds(PointCloud(both, DEV), PointCloud(gt, DEV), str(tmp_path / "d"), 0.1, voxel_size=v, min_cluster_points=50)
    assert clean.pop("removed_floaters") == 30
    assert clean == plain and dirty["accuracy"] > plain["accuracy"]
    kept, index = PointCloud(both, DEV).remove_small_clusters(2 * v, 4, 50)
    assert np.array_equal(index.cpu().numpy(), np.concatenate([np.arange(1000), np.arange(1030, len(both))]))
