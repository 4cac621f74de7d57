"""Segmentation on the CPU: the library's symbols, the label rule the kernels follow against the sequential algorithm the restatement
(tests/segment_restatement.py) runs, the refit against an SVD, the wrappers' argument errors, and the conditions the GPU tests'
scenes must meet."""
import os
import re

import numpy as np
import pytest
import torch

from tests import cloud_tools_restatement as TR
from tests import global_reg_restatement as GR
from tests import segment_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lnr_cloud_radius_count", "lnr_cloud_dbscan_workspace", "lnr_cloud_dbscan", "lnr_plane_workspace", "lnr_cloud_segment_plane")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from loner_amd import hip
    return hip.load()


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    from loner_amd import build, hip
    header = open(os.path.join(ROOT, "include", "loner_hip.h")).read()
    declared = set(re.findall(r"\b(lnr_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/loner_hip.h"
        assert name in hip.declared_symbols(), f"{name} is not in the ctypes table"
        assert hasattr(lib, name), f"{name} is not exported"
    plane = int(re.search(r"#define LNR_STREAM_PLANE (0x[0-9A-Fa-f]+)", header).group(1), 16)
    assert plane == hip.STREAM_PLANE == SR.STREAM_PLANE
    assert len({plane, GR.STREAM_RANSAC, TR.STREAM_MESH}) == 3
    assert "lnr_cloud_segment.hip" in build.EXACT and any(s[0] == "lnr_cloud_segment.hip" for s in build.SOURCES)
    assert lib.lnr_cloud_dbscan_workspace(-1) == 0 and lib.lnr_cloud_dbscan_workspace(1 << 31) == 0 and lib.lnr_cloud_dbscan_workspace(10) > 0
    assert lib.lnr_plane_workspace(10, 0) == 0 and lib.lnr_plane_workspace(10, (1 << 22) + 1) == 0 and lib.lnr_plane_workspace(10, 1 << 22) > 0


def test_host_entries_refuse_bad_arguments(lib):
    for r, word in ((0.0, b"radius"), (float("inf"), b"radius"), (float("nan"), b"radius")):
        assert lib.lnr_cloud_radius_count(None, 0, r, None, None, None) != 0 and word in lib.lnr_last_error()
    for eps, k, word in ((0.0, 3, b"eps"), (float("nan"), 3, b"eps"), (1.0, 0, b"min_points")):
        assert lib.lnr_cloud_dbscan(None, 0, eps, k, None, None, 0, None, None) != 0 and word in lib.lnr_last_error()
    for t, H, word in ((0.0, 8, b"distance_threshold"), (float("inf"), 8, b"distance_threshold"), (0.1, 0, b"n_hypotheses"),
                       (0.1, (1 << 22) + 1, b"n_hypotheses")):
        assert lib.lnr_cloud_segment_plane(None, 0, t, H, 0, 1, None, None, None, 0, None, None) != 0 and word in lib.lnr_last_error()


# ---------------------------------------------------------------- the label rule
def parallel_rule(nbrs, min_points):
    """What the kernels compute, written without the sequential walk: components of cores, numbered by their smallest core; a
    non-core takes the smallest number among its core neighbours; everything else is -1."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(nbrs)
    core = np.array([len(x) >= min_points for x in nbrs], dtype=bool)
    rows = np.concatenate([np.full(len(x), i) for i, x in enumerate(nbrs)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    cols = np.concatenate(list(nbrs) + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    both = core[rows] & core[cols]
    _, comp = connected_components(coo_matrix((np.ones(int(both.sum())), (rows[both], cols[both])), shape=(n, n)), directed=False)
    labels = np.full(n, -1, dtype=np.int64)
    smallest = {}
    for i in np.nonzero(core)[0]:
        smallest.setdefault(comp[i], i)
    number = {c: k for k, (c, _) in enumerate(sorted(smallest.items(), key=lambda kv: kv[1]))}
    for i in np.nonzero(core)[0]:
        labels[i] = number[comp[i]]
    for i in np.nonzero(~core)[0]:
        near = [labels[j] for j in nbrs[i] if core[j]]
        if near:
            labels[i] = min(near)
    return labels.astype(np.int32)


def _scenes():
    blobs = SR.blobs_scene()
    eps = np.nextafter(0.25, 1.0)
    return [("blobs a", blobs, *SR.RANDOM_SETTINGS[0]), ("blobs b", blobs, *SR.RANDOM_SETTINGS[1]), ("chain", SR.chain_scene(), 0.1, 3),
            ("lattice at eps", SR.lattice_scene(), 0.25, 2), ("lattice above eps", SR.lattice_scene(), eps, 2),
            ("border", SR.border_scene(), SR.BORDER_EPS, SR.BORDER_MIN_POINTS),
            ("border swapped", SR.border_scene(True), SR.BORDER_EPS, SR.BORDER_MIN_POINTS), ("components", blobs[:3000], 0.5, 1),
            ("all noise", blobs[:500], 0.01, 3)]


@pytest.mark.parametrize("k", range(9))
def test_the_parallel_rule_equals_the_sequential_walk_on_the_gpu_scenes(k):
    name, p, eps, min_points = _scenes()[k]
    nbrs = SR.radius_neighbours(p, eps)
    seq, info = SR.dbscan(p, eps, min_points, nbrs)
    assert np.array_equal(seq, parallel_rule(nbrs, min_points)), name
    print(f"{name}: {info}")
    n = len(p)
    if name == "chain":
        assert info == {"clusters": 1, "cores": n - 2, "border": 2, "noise": 0}
    if name == "lattice at eps":
        assert info["noise"] == n and info["clusters"] == 0
    if name == "lattice above eps":
        assert info["clusters"] == 1 and info["cores"] == n
    if name.startswith("border"):
        assert info["clusters"] == 2 and seq[-1] == 0 and seq[0] == 0 and seq[11] == 1 and info["border"] == 5
    if name == "components":
        assert info["noise"] == 0 and info["cores"] == n
    if name == "all noise":
        assert info["noise"] == n
    if name.startswith("blobs"):
        assert info["clusters"] >= 4 and info["border"] > 0 and info["noise"] > 1000    # blobs may touch; several stay apart


def test_the_parallel_rule_equals_the_sequential_walk_on_random_small_clouds():
    rng = np.random.default_rng(7)
    seen_border = 0
    for trial in range(200):
        n = int(rng.integers(1, 61))
        p = rng.uniform(0, 1, size=(n, 3)) * rng.uniform(0.3, 1.5)
        eps = rng.uniform(0.1, 0.4)
        min_points = int(rng.integers(1, 6))
        nbrs = SR.radius_neighbours(p, eps)
        seq, info = SR.dbscan(p, eps, min_points, nbrs)
        assert np.array_equal(seq, parallel_rule(nbrs, min_points)), trial
        seen_border += info["border"]
    assert seen_border > 100                                    # the border rule was exercised


# ---------------------------------------------------------------- scene preconditions
def test_no_pair_of_the_random_scene_lies_at_eps():
    """strictness of < cannot decide the random cases: no pair lies within 1e-9 of eps or of a radius the count test may use (the
    crafted lattice decides it)"""
    from scipy.spatial import cKDTree
    p = SR.blobs_scene()
    tree = cKDTree(p)
    for eps, _ in SR.RANDOM_SETTINGS:
        assert tree.count_neighbors(tree, eps + 1e-9) == tree.count_neighbors(tree, eps - 1e-9)


def test_the_plane_scene_has_a_clear_winner_and_the_tie_scene_only_ties():
    p = SR.box_corner_scene()
    r = SR.segment_plane(p, SR.BOX_T, SR.BOX_H, 0, True)
    top = np.sort(r["counts"])[::-1]
    print(f"box corner: best h {r['best_hypothesis']} with {r['n_inliers']} inliers, the next count {top[1]}; {r['survivors']} survivors")
    assert top[0] > top[1] and r["nonfinite"] == 2 and r["status"] == 0
    assert 1900 < r["n_inliers"] <= 2000 + 273 and r["rejected_degenerate"] > 0          # a NaN sample is degenerate
    t = SR.tie_scene()
    r = SR.segment_plane(t, 0.01, 256, 0, True)
    assert r["survivors"] > 100 and np.all(r["counts"] == 600) and np.all(r["sums"] == 0.0)
    assert r["best_hypothesis"] == r["alive"][0] and r["rejected_repeated"] + r["rejected_degenerate"] + r["survivors"] == 256
    assert np.array_equal(np.abs(r["hypothesis_plane"]), [0.0, 0.0, 1.0, 0.0])
    r = SR.segment_plane(SR.collinear_scene(), 0.01, 256, 0, True)
    assert r["status"] == 2 and r["survivors"] == 0 and not r["inlier"].any() and not r["plane"].any()
    assert SR.segment_plane(np.zeros((2, 3)), 0.01, 16)["status"] == 1


def test_the_refit_agrees_with_an_svd_of_the_centred_inliers():
    p = SR.box_corner_scene()
    r = SR.segment_plane(p, SR.BOX_T, SR.BOX_H, 0, True)
    q = p[r["inlier"]]
    c = q.mean(axis=0)
    nrm = np.linalg.svd(q - c)[2][2]
    nrm = nrm if nrm @ r["hypothesis_plane"][:3] >= 0 else -nrm
    assert np.abs(r["plane"][:3] - nrm).max() < 1e-9
    assert abs(r["plane"][3] + nrm @ c) < 1e-9
    assert np.abs(np.abs(r["plane"][:3]) - [0.0, 0.0, 1.0]).max() < 1e-3


def test_segment_planes_restated_finds_the_three_faces():
    models, labels = SR.segment_planes(SR.box_corner_scene(), SR.BOX_T, 5, 300, SR.BOX_H)
    assert len(models) == 3 and [int((labels == k).sum()) > 600 for k in range(3)] == [True] * 3
    assert sorted(int(np.abs(m[:3]).argmax()) for m in models) == [0, 1, 2]


# ---------------------------------------------------------------- wrappers
class _Fake:
    """a tensor stand-in that says it lives on the device, for the checks that run before any launch"""

    def __init__(self, t):
        self.t = t
        self.is_cuda = True

    def __getattr__(self, name):
        return getattr(self.t, name)


def _cloud(n=4):
    from loner_amd.analysis.lidar_map import PointCloud
    c = PointCloud.__new__(PointCloud)
    c.points, c.normals, c.covariances = _Fake(torch.zeros(n, 3, dtype=torch.float64)), None, None
    return c


def test_wrappers_refuse_bad_arguments_before_touching_a_device(lib):
    from loner_amd.analysis import segmentation as SEG
    c = _cloud()
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            c.cluster_dbscan(eps, 3)
        with pytest.raises(ValueError, match="eps"):
            c.remove_small_clusters(eps, 3, 10)
    for k in (0, -2, 2.5):
        with pytest.raises(ValueError, match="min_points"):
            c.cluster_dbscan(0.1, k)
    with pytest.raises(ValueError, match="min_cluster_points"):
        c.remove_small_clusters(0.1, 3, -1)
    for r in (0.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            c.remove_radius_outlier(3, r)
    with pytest.raises(ValueError, match="nb_points"):
        c.remove_radius_outlier(-1, 0.1)
    for H in (0, (1 << 22) + 1, 10.5):
        with pytest.raises(ValueError, match="num_iterations"):
            c.segment_plane(0.01, H)
        with pytest.raises(ValueError, match="num_iterations"):
            SEG.segment_planes(c, 0.01, 3, 10, num_iterations=H)
    for t in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="distance_threshold"):
            c.segment_plane(t)
        with pytest.raises(ValueError, match="distance_threshold"):
            SEG.plane_ransac(c.points, t)
    with pytest.raises(ValueError, match="max_planes"):
        SEG.segment_planes(c, 0.01, -1, 10)
    with pytest.raises(ValueError, match="min_inliers"):
        SEG.segment_planes(c, 0.01, 3, -1)
    with pytest.raises(RuntimeError, match="expected a tensor on the MI355X"):
        SEG.plane_ransac(torch.zeros(4, 3), 0.01)
