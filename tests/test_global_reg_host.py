"""Global registration on the CPU: the restatement (tests/global_reg_restatement.py) against independent formulas, the conditions the
GPU tests' scene must meet, the library's symbols and host entries, and the wrappers' argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from loner_amd.analysis import registration as REG
from tests import cloud_restatement as CR
from tests import global_reg_restatement as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lnr_cloud_orient_normals", "lnr_fpfh_bin_edges", "lnr_cloud_fpfh_workspace", "lnr_cloud_fpfh", "lnr_feature_nearest_workspace",
           "lnr_feature_nearest", "lnr_ransac_workspace", "lnr_ransac_correspondence")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from loner_amd import hip
    return hip.load()


@pytest.fixture(scope="module")
def edges(lib):
    return GR.bin_edges()


@pytest.fixture(scope="module")
def scene_features(edges):
    """the scene with CPU normals oriented towards the viewpoint, its FPFH features and its feature correspondences, computed once"""
    src, tgt, truth, view_s, view_t = GR.scene()
    ns = GR.orient(GR.host_normals(src), src, location=view_s)[0]
    nt = GR.orient(GR.host_normals(tgt), tgt, location=view_t)[0]
    fs, _ = GR.fpfh(src, ns, 5 * GR.VOXEL, 32, edges)
    ft, _ = GR.fpfh(tgt, nt, 5 * GR.VOXEL, 32, edges)
    return src, tgt, truth, fs, ft, GR.correspondences_from_features(fs, ft)


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    from loner_amd import hip
    header = open(os.path.join(ROOT, "include", "loner_hip.h")).read()
    declared = set(re.findall(r"\b(lnr_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/loner_hip.h"
        assert name in hip.declared_symbols(), f"{name} is not in the ctypes table"
        assert hasattr(lib, name), f"{name} is not exported"
    for word, value in (("LNR_FPFH_DIM", hip.FPFH_DIM), ("LNR_FEATURE_DIM_MAX", hip.FEATURE_DIM_MAX), ("LNR_RANSAC_CHUNK", hip.RANSAC_CHUNK),
                        ("LNR_KNN_MAX", hip.KNN_MAX)):
        assert int(re.search(rf"#define {word} (\d+)", header).group(1)) == value
    assert int(re.search(r"#define LNR_STREAM_RANSAC (0x[0-9A-Fa-f]+)", header).group(1), 16) == hip.STREAM_RANSAC == GR.STREAM_RANSAC
    from tests import cloud_tools_restatement as TR
    assert GR.STREAM_RANSAC != TR.STREAM_MESH
    from loner_amd import build
    assert "lnr_global_reg.hip" in build.EXACT and any(s[0] == "lnr_global_reg.hip" for s in build.SOURCES)


def test_bin_edges_are_the_cosines_and_sines_of_the_inner_edges(edges):
    theta = -np.pi + 2 * np.pi * np.arange(1, 11) / 11
    # cos and sin of a theta that carries half an ulp of 3.14 itself: 4e-16 bounds the difference from the correctly rounded literals
    assert np.abs(edges[:, 0] - np.cos(theta)).max() < 4e-16 and np.abs(edges[:, 1] - np.sin(theta)).max() < 4e-16
    assert np.array_equal(edges[:5, 0], edges[:4:-1, 0]) and np.array_equal(edges[:5, 1], -edges[:4:-1, 1])     # symmetric in y


def test_the_angle_bin_rule_matches_atan2(edges):
    rng = np.random.default_rng(0)
    y, x = rng.normal(size=200000), rng.normal(size=200000)
    want = np.minimum(np.floor(11 * (np.arctan2(y, x) + np.pi) / (2 * np.pi)), 10).astype(np.int64)
    assert np.array_equal(GR.angle_bin(y, x, edges), want)
    tiny = np.nextafter(0.0, 1.0)
    for (yy, xx), b in (((0.0, -1.0), 10), ((0.0, 1.0), 5), ((-tiny, -1.0), 0), ((0.0, 0.0), 5)):
        assert int(GR.angle_bin(np.array(yy), np.array(xx), edges)) == b, (yy, xx)
    assert list(GR.unit_bin(np.array([-1.0, -1.5, 1.0, 2.0, 0.0, np.nan]))) == [0, 0, 10, 10, 5, 0]


def _bins(edges, p1, n1, p2, n2):
    return tuple(int(b[0]) for b in GR.pair_bins(np.array([p1], dtype=np.float64), np.array([n1], dtype=np.float64),
                                                 np.array([p2], dtype=np.float64), np.array([n2], dtype=np.float64), edges))


def test_pair_features_of_known_pairs(edges):
    """the degenerate pairs count as (0, 0, 0): a duplicate, and a neighbour along the normal (|v| = 0); and one pair by hand"""
    z, o = (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
    assert _bins(edges, o, z, o, z) == (5, 5, 5)
    assert _bins(edges, o, z, (0.0, 0.0, 2.0), z) == (5, 5, 5)
    assert _bins(edges, o, (np.nan, 0.0, 1.0), (1.0, 0.0, 0.0), z) == (5, 5, 5)
    # p2 = (1, 0, 0), both normals z: a1 = a2 = 0, no swap, f2 = 0; v = d x n1 = (0, -1, 0), w = n1 x v = (1, 0, 0), f1 = v.n2 = 0,
    # y = w.n2 = 0, x = 1: atan2(0, 1) = 0 -> bin 5
    assert _bins(edges, o, z, (1.0, 0.0, 0.0), z) == (5, 5, 5)
    # n2 tilted towards +x by 45 degrees: a2 = sin 45 > |a1| = 0: swapped, d = (-1, 0, 0), f2 = -a2 = -0.707 -> bin floor(11 * 0.146) = 1;
    # v = d x n1' = (0, c, 0) / c = (0, 1, 0), w = n1' x v = (-c, 0, s), f1 = v.z = 0 -> 5; y = w.z = 0.707, x = 0.707: 45 degrees ->
    # floor(11 * (pi/4 + pi) / 2 pi) = 6
    s = np.sqrt(0.5)
    assert _bins(edges, o, z, (1.0, 0.0, 0.0), (s, 0.0, s)) == (6, 5, 1)


def test_fpfh_blocks_sum_to_200(scene_features):
    src, tgt, truth, fs, ft, corr = scene_features
    ids, d2, cnt = GR.neighbours(tgt, 5 * GR.VOXEL, 32)
    assert cnt.min() > 0                                        # every point has a neighbour, and a neighbour's SPFH sums to 100
    blocks = np.add.accumulate(ft.reshape(-1, 3, 11), axis=2)[:, :, -1]
    assert np.abs(blocks - 200.0).max() < 1e-9, np.abs(blocks - 200.0).max()
    lone, _ = GR.fpfh(np.array([[0.0, 0.0, 0.0], [9.0, 0.0, 0.0]]), np.array([[0.0, 0.0, 1.0]] * 2), 1.0, 32)
    assert not lone.any()                                       # no neighbour inside the radius: all zero


def test_feature_nearest_rules():
    t = np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0], [np.nan, 0.0]])
    idx, d2 = GR.feature_nearest(t, np.array([[0.1, 0.0], [0.9, 0.0], [np.nan, 1.0]]))
    assert list(idx) == [1, 0, -1] and d2[0] == 0.1 * 0.1 and np.isinf(d2[2])      # the lower index of a duplicate; NaN never wins
    assert list(GR.feature_nearest(np.zeros((0, 2)), np.zeros((2, 2)))[0]) == [-1, -1]
    c = GR.correspondences_from_features(np.array([[0.0], [0.2], [5.0]]), np.array([[0.1], [5.0]]), mutual_filter=True)
    assert c.tolist() == [[0, 0], [2, 1]]                       # 0 and 1 both choose target 0, which chooses 0 back (the tie's lower index)


def test_the_restated_ransac_recovers_the_scene(scene_features):
    """The conditions of the GPU tests' scene: with 4096 hypotheses at least 50 survive the edge checker, and the best pose leaves every
    source point within the first ICP distance (3 voxels) of its true place."""
    src, tgt, truth, fs, ft, corr = scene_features
    true = CR.transform(src, truth)
    near = np.linalg.norm(true[corr[:, 0]] - tgt[corr[:, 1]], axis=1) < 1.5 * GR.VOXEL
    print(f"{len(corr)} feature correspondences, {near.mean():.3f} of them within {1.5 * GR.VOXEL} m of the truth")
    for seed in (0, 1, 2):
        r = GR.ransac(src, tgt, corr, 4096, seed, 1.5 * GR.VOXEL, 0.9)
        err = np.linalg.norm(CR.transform(src, r["transformation"]) - true, axis=1).max()
        print(f"seed {seed}: {r['survivors']} survivors, best h {r['best_hypothesis']}, {r['n_inliers']} inliers, largest point error {err:.4f} m")
        assert r["status"] == 0 and r["survivors"] >= 50
        assert err < 3 * GR.VOXEL
        assert r["survivors"] + r["rejected_repeated"] + r["rejected_edge"] + r["rejected_frame"] == 4096
        R = r["transformation"][:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


def test_restated_ransac_edge_cases():
    rng = np.random.default_rng(5)
    p = rng.normal(size=(40, 3))
    corr = np.stack([np.arange(40), np.arange(40)], 1)
    for m in (0, 2):
        r = GR.ransac(p, p, corr[:m], 64, 0, 0.1, 0.9)
        assert r["status"] == 1 and np.array_equal(r["transformation"], np.eye(4)) and r["survivors"] == 0 and r["n_correspondences"] == m
    line = np.outer(np.arange(40.0), [1.0, 0.0, 0.0]) + [0.0, 2.0, -1.0]        # along an axis: every cross product is exactly zero
    r = GR.ransac(line, line, corr, 256, 0, 0.1, 0.0)
    assert r["status"] == 2 and r["survivors"] == 0 and r["rejected_frame"] + r["rejected_repeated"] == 256
    r = GR.ransac(p, p, corr[:3], 256, 0, 0.1, 0.9)
    assert r["rejected_repeated"] > 128 and r["survivors"] > 0 and r["n_inliers"] == 3           # 7 of 9 draws repeat an index
    assert np.abs(r["transformation"] - np.eye(4)).max() < 1e-12


def test_host_entries_refuse_bad_arguments(lib):
    out = (ctypes.c_double * 20)()
    assert lib.lnr_fpfh_bin_edges(out) == 0 and lib.lnr_fpfh_bin_edges(None) != 0
    assert lib.lnr_cloud_fpfh_workspace(-1) == 0 and lib.lnr_cloud_fpfh_workspace(1 << 31) == 0 and lib.lnr_cloud_fpfh_workspace(10) > 0
    assert lib.lnr_ransac_workspace(10, 0) == 0 and lib.lnr_ransac_workspace(10, (1 << 22) + 1) == 0 and lib.lnr_ransac_workspace(10, 1 << 22) > 0
    assert lib.lnr_feature_nearest_workspace(-1) == 0
    for max_nn, radius, word in ((1, 1.0, b"max_nn"), (33, 1.0, b"max_nn"), (8, 0.0, b"radius"), (8, float("nan"), b"radius")):
        assert lib.lnr_cloud_fpfh(None, 0, None, radius, max_nn, None, None, 0, None, None) != 0 and word in lib.lnr_last_error()
    for dim, split, word in ((0, 0, b"dim"), (65, 0, b"dim"), (3, -1, b"split"), (3, 513, b"split")):
        assert lib.lnr_feature_nearest(None, 0, None, 0, dim, split, None, None, None, 0, None) != 0 and word in lib.lnr_last_error()
    for H, d, e, word in ((0, 1.0, 0.5, b"n_hypotheses"), ((1 << 22) + 1, 1.0, 0.5, b"n_hypotheses"), (8, 0.0, 0.5, b"max_distance"),
                          (8, 1.0, -0.1, b"edge_similarity"), (8, 1.0, 1.5, b"edge_similarity"), (8, 1.0, float("nan"), b"edge_similarity")):
        assert lib.lnr_ransac_correspondence(None, 0, None, 0, None, 0, H, 0, d, e, None, 0, None, None, None) != 0
        assert word in lib.lnr_last_error()
    ref = (ctypes.c_double * 3)(0.0, 0.0, float("inf"))
    assert lib.lnr_cloud_orient_normals(None, 0, None, 2, ref, None, None) != 0 and b"mode" in lib.lnr_last_error()
    assert lib.lnr_cloud_orient_normals(None, 0, None, 1, ref, ctypes.c_void_p(8), None) != 0 and b"finite" in lib.lnr_last_error()


class _Fake:
    """a tensor stand-in that says it lives on the device, for the checks that run before any launch"""

    def __init__(self, t):
        self.t = t
        self.is_cuda = True

    def __getattr__(self, name):
        return getattr(self.t, name)


def test_wrapper_argument_errors(lib):
    f = _Fake(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="exactly one"):
        REG.orient_normals(f)
    with pytest.raises(ValueError, match="exactly one"):
        REG.orient_normals(f, f, location=(0, 0, 0), direction=(0, 0, 1))
    with pytest.raises(ValueError, match="needs the points"):
        REG.orient_normals(f, location=(0, 0, 0))
    with pytest.raises(ValueError, match="3 finite numbers"):
        REG.orient_normals(f, direction=(0, 0, float("nan")))
    with pytest.raises(ValueError, match="fp64"):
        REG.orient_normals(_Fake(torch.zeros(4, 3)), direction=(0, 0, 1))
    with pytest.raises(ValueError, match="dim in"):
        REG.feature_nearest(_Fake(torch.zeros(4, 65, dtype=torch.float64)), _Fake(torch.zeros(4, 65, dtype=torch.float64)))
    with pytest.raises(ValueError, match="queries of dim"):
        REG.feature_nearest(_Fake(torch.zeros(4, 3, dtype=torch.float64)), _Fake(torch.zeros(4, 2, dtype=torch.float64)))
    with pytest.raises(ValueError, match="split"):
        REG.feature_nearest(f, f, split=513)
    corr = _Fake(torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="integer"):
        REG.ransac_correspondence(f, f, _Fake(torch.zeros(4, 2)), 0.1)
    with pytest.raises(ValueError, match="max_distance"):
        REG.ransac_correspondence(f, f, corr, 0.0)
    with pytest.raises(ValueError, match="edge_similarity"):
        REG.ransac_correspondence(f, f, corr, 0.1, edge_similarity=1.1)
    with pytest.raises(ValueError, match="hypotheses"):
        REG.ransac_correspondence(f, f, corr, 0.1, hypotheses=0)
    with pytest.raises(RuntimeError, match="expected a tensor on the MI355X"):
        REG.feature_nearest(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="voxel_size"):
        REG.global_registration(None, None, 0.0)
    with pytest.raises(ValueError, match="orient"):
        REG.global_registration(None, None, 0.25, orient=(1, 2, 3))
