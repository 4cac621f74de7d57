"""Global registration on the MI355X against the numpy restatement (tests/global_reg_restatement.py): orientation, FPFH, the feature
search and RANSAC bit for bit, then the whole path on a scene whose clouds are metres and 140 degrees apart.  The scene's FPFH inputs
are the device's own normals; the references are computed once per module."""
import numpy as np
import pytest
import torch

from loner_amd.analysis import registration as REG
from tests import cloud_restatement as CR
from tests import global_reg_restatement as GR
from tests import icp_restatement as IR

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = 64                                # FN_TILE of loner_amd/csrc/lnr_global_reg.hip


def _t(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def edges():
    return GR.bin_edges()


@pytest.fixture(scope="module")
def scene(edges):
    """the scene, the device's normals of both clouds oriented towards the viewpoints, and the restated features and matches"""
    from loner_amd import ops
    src, tgt, truth, view_s, view_t = GR.scene()
    out = {"src": src, "tgt": tgt, "truth": truth, "views": (view_s, view_t)}
    for key, p, view in (("s", src, view_s), ("t", tgt, view_t)):
        n = ops.NNGrid(_t(p)).normals(30)
        REG.orient_normals(n, _t(p), location=view)
        out["n" + key] = n.cpu().numpy()
        out["f" + key], _ = GR.fpfh(p, out["n" + key], 5 * GR.VOXEL, 32, edges)
    out["corr"] = GR.correspondences_from_features(out["fs"], out["ft"])
    return out


# ---------------------------------------------------------------- orientation
def test_orientation_is_bit_identical_in_both_modes():
    rng = np.random.default_rng(11)
    p = rng.normal(size=(1000, 3)) * 3
    n = _unit(rng, 1000)
    loc = np.array([0.5, -1.0, 2.0])
    p[0], n[0] = loc + [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]             # (l - p).n = 0 exactly: left
    n[1] = [np.nan, 0.0, 1.0]                                        # left and counted
    n[2] = [0.0, np.inf, 0.0]
    n[3] = [1.0, 0.0, 0.0]                                           # direction (0, 1, 1): a zero dot product
    for how in ({"location": loc}, {"direction": np.array([0.0, 1.0, 1.0])}):
        want, bad, flipped = GR.orient(n, p, **how)
        got, stats = _t(n), {}
        REG.orient_normals(got, _t(p), stats=stats, **how)
        assert _same_bits(got.cpu().numpy(), want)
        assert stats == {"nonfinite": bad, "flipped": flipped} and bad == 2 and 400 < flipped < 600
        assert _same_bits(got.cpu().numpy()[[0, 3] if "direction" in how else [0]], n[[0, 3] if "direction" in how else [0]])


def test_point_cloud_orientation_methods():
    from loner_amd.analysis.lidar_map import PointCloud
    rng = np.random.default_rng(12)
    p, n = rng.normal(size=(300, 3)), _unit(rng, 300)
    cloud = PointCloud(_t(p))
    with pytest.raises(ValueError, match="no normals"):
        cloud.orient_normals_towards_location((0, 0, 0))
    cloud.normals = _t(n)
    assert cloud.orient_normals_towards_location((0.0, 0.0, 9.0)) is cloud
    assert _same_bits(cloud.normals.cpu().numpy(), GR.orient(n, p, location=(0.0, 0.0, 9.0))[0])
    cloud.normals = _t(n)
    cloud.orient_normals_to_align_with_direction((1.0, 0.0, 0.0))
    assert _same_bits(cloud.normals.cpu().numpy(), GR.orient(n, direction=(1.0, 0.0, 0.0))[0])


# ---------------------------------------------------------------- FPFH
def _fpfh_clouds():
    rng = np.random.default_rng(21)
    blob = rng.normal(size=(150, 3)) * [1.0, 1.0, 0.2]
    dup = np.concatenate([rng.uniform(-1, 1, size=(20, 3)) + [6.0, 0.0, 0.0]] * 3)                # 3 exact copies of 20 points
    pile = np.tile([[-6.0, 0.0, 0.0]], (40, 1))                                                   # more copies than max_nn
    far = np.array([[0.0, 40.0, 0.0]])                                                            # no neighbour inside r
    sparse = np.array([[20.0, 0.0, 0.0], [20.3, 0.0, 0.0], [20.0, 0.4, 0.0]])                     # fewer than max_nn neighbours
    pair = np.array([[0.0, -20.0, 0.0], [0.0, -20.0, 0.5]])                                       # the neighbour along the normal: |v| = 0
    mixed = np.concatenate([blob, dup, pile, far, sparse, pair, rng.normal(size=(1, 3))])
    assert len(mixed) == 257
    nm = _unit(rng, 257)
    nm[-3], nm[-2] = [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]
    nan = mixed[:60].copy()
    nn = _unit(rng, 60)
    nn[7] = [np.nan, 0.0, 0.0]
    ax = np.arange(-4, 5) * 0.5
    lattice = np.stack(np.meshgrid(ax, ax, ax[:4], indexing="ij"), -1).reshape(-1, 3)
    return {"one": (rng.normal(size=(1, 3)), _unit(rng, 1), 1.0, None), "two": (rng.normal(size=(2, 3)) * 0.3, _unit(rng, 2), 5.0, None),
            "mixed257": (mixed, nm, 1.0, None), "nan_normal": (nan, nn, 1.0, None),
            "lattice_exact_pass": (lattice, _unit(rng, len(lattice)), 1.1, 0.05)}


@pytest.mark.parametrize("name", list(_fpfh_clouds()))
@pytest.mark.parametrize("max_nn", [2, 32])
def test_fpfh_is_bit_identical_to_the_restatement(name, max_nn, edges):
    from loner_amd import ops
    p, n, radius, cell_edge = _fpfh_clouds()[name]
    want, bad = GR.fpfh(p, n, radius, max_nn, edges)
    stats = {}
    got = REG.fpfh(ops.NNGrid(_t(p), cell_edge), _t(n), radius, max_nn, stats=stats).cpu().numpy()
    print(f"{name}: {len(p)} points, max_nn {max_nn}, {stats}")
    assert got.shape == (len(p), 33) and np.isfinite(got).all()
    assert _same_bits(got, want), f"{int((got != want).any(1).sum())} of {len(p)} rows differ"
    assert stats["nonfinite_normals"] == bad == (1 if name == "nan_normal" else 0)
    if name == "lattice_exact_pass":                 # a cell edge of a tenth of the spacing: five shells find only the point itself
        assert stats["fallback"] == len(p)
    if name == "mixed257":
        ids, d2, cnt = GR.neighbours(p, radius, max_nn)
        assert cnt[250] == 0 and not got[250].any()                     # the far point
        assert cnt[251] == min(2, max_nn - 1) and (d2[150:210, 0] == 0).all()
        if max_nn == 32:
            assert cnt[249] == 32 and cnt[210] == 31                    # the pile: a late copy does not hold itself in its list
        assert 0 < cnt[:150].min() and cnt[:150].max() <= max_nn


@pytest.mark.parametrize("max_nn", [2, 32])
def test_fpfh_of_the_scene_target(scene, max_nn, edges):
    from loner_amd.analysis.lidar_map import PointCloud
    want = scene["ft"] if max_nn == 32 else GR.fpfh(scene["tgt"], scene["nt"], 5 * GR.VOXEL, max_nn, edges)[0]
    cloud = PointCloud(_t(scene["tgt"]))
    with pytest.raises(ValueError, match="no normals"):
        cloud.compute_fpfh_feature(5 * GR.VOXEL)
    cloud.normals = _t(scene["nt"])
    got = cloud.compute_fpfh_feature(5 * GR.VOXEL, max_nn).cpu().numpy()
    assert _same_bits(got, want), f"{int((got != want).any(1).sum())} of {len(want)} rows differ"
    blocks = got.reshape(-1, 3, 11).sum(2)
    assert np.abs(blocks - 200.0).max() < 1e-9
    again = cloud.compute_fpfh_feature(5 * GR.VOXEL, max_nn).cpu().numpy()
    assert _same_bits(again, got)


def test_fpfh_argument_errors():
    from loner_amd import ops
    g = ops.NNGrid(_t(np.random.default_rng(0).normal(size=(10, 3))))
    n = _t(np.zeros((10, 3)))
    for kw, word in ((dict(radius=1.0, max_nn=1), "max_nn"), (dict(radius=1.0, max_nn=33), "max_nn"), (dict(radius=0.0), "radius")):
        with pytest.raises(ValueError, match=word):
            REG.fpfh(g, n, **kw)
    with pytest.raises(ValueError, match="normals for"):
        REG.fpfh(g, n[:9], 1.0)


# ---------------------------------------------------------------- nearest neighbour in feature space
@pytest.mark.parametrize("dim", [1, 33, 64])
def test_feature_nearest_is_bit_identical(dim):
    rng = np.random.default_rng(31 + dim)
    for n_t in (0, 1, TILE - 1, TILE, TILE + 1, 5 * TILE + 7):
        t = rng.normal(size=(n_t, dim))
        if n_t > 3:
            t[3] = t[1]                                               # duplicated rows: the lower index wins
            t[2, 0] = np.nan                                          # a NaN row never wins
        for n_q in (1, 63, 257):
            q = rng.normal(size=(n_q, dim))
            if n_t > 3:
                q[0] = t[1]
            if n_q > 5:
                q[5, dim - 1] = np.nan                                # a NaN query finds nothing
            want_i, want_d = GR.feature_nearest(t, q)
            for split in ((0,) if n_t <= TILE else (0, 1, 3)):        # 0: the library's rule, which slices once there are two tiles
                idx, d2 = REG.feature_nearest(_t(t), _t(q), split=split)
                idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
                assert np.array_equal(idx, want_i), (n_t, n_q, split, int((idx != want_i).sum()))
                assert _same_bits(d2, want_d), (n_t, n_q, split)
            if n_t == 0:
                assert (want_i == -1).all() and np.isinf(want_d).all()
            elif n_t > 3:
                assert want_i[0] == 1 and want_d[0] == 0.0 and (2 not in want_i)
                assert n_q <= 5 or want_i[5] == -1


def test_correspondences_from_features(scene):
    fs, ft = _t(scene["fs"]), _t(scene["ft"])
    got = REG.correspondences_from_features(fs, ft)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), scene["corr"])
    mutual = REG.correspondences_from_features(fs, ft, mutual_filter=True).cpu().numpy()
    want = GR.correspondences_from_features(scene["fs"], scene["ft"], mutual_filter=True)
    assert np.array_equal(mutual, want) and 0 < len(want) < len(scene["corr"])


# ---------------------------------------------------------------- RANSAC
def _ransac_pair():
    rng = np.random.default_rng(41)
    src = rng.uniform(-4, 4, size=(3000, 3))
    tgt = CR.transform(src, IR.rigid(75, (1.0, 2.0, -0.5))) + rng.normal(size=src.shape) * 0.01
    corr = np.stack([np.arange(3000), np.arange(3000)], 1)
    wrong = rng.random(3000) < 0.6
    corr[wrong, 1] = rng.integers(0, 3000, int(wrong.sum()))
    return src, tgt, corr.astype(np.int32)


KEYS = ("status", "best_hypothesis", "n_inliers", "survivors", "rejected_repeated", "rejected_edge", "rejected_frame", "n_correspondences")


def _check_ransac(src, tgt, corr, H, seed, d, e):
    want = GR.ransac(src, tgt, corr, H, seed, d, e)
    got = REG.ransac_correspondence(_t(src), _t(tgt), _t(corr, np.int32).reshape(-1, 2), d, e, H, seed, strict=False)
    assert {k: got[k] for k in KEYS} == {k: want[k] for k in KEYS}
    assert _same_bits(got["transformation"], want["transformation"])
    assert _same_bits(np.array([got["fitness"], got["inlier_rmse"]]), np.array([want["fitness"], want["inlier_rmse"]]))
    return got


@pytest.mark.parametrize("m,H,e", [(0, 255, 0.9), (2, 257, 0.0), (3, 4096, 0.9), (3, 255, 0.0), (2047, 255, 0.9), (2048, 257, 0.0),
                                   (2049, 4096, 0.0), (2049, 1, 0.9), (2049, 4096, 0.9), (3000, 257, 0.9)])
def test_ransac_is_bit_identical_to_the_restatement(m, H, e):
    src, tgt, corr = _ransac_pair()
    got = _check_ransac(src, tgt, corr[:m], H, 7, 0.05, e)
    print(f"m {m}, H {H}, e {e}: {got}")
    if m < 3:
        assert got["status"] == 1 and np.array_equal(got["transformation"], np.eye(4)) and got["n_inliers"] == 0
    if m == 3 and H == 4096:
        assert got["rejected_repeated"] > H // 2                     # 7 of 9 draws repeat an index
    if e == 0.0:
        assert got["rejected_edge"] == 0
    if m == 2049 and H == 4096 and e == 0.9:
        R = got["transformation"]
        assert got["n_inliers"] > 600 and np.abs(R - IR.rigid(75, (1.0, 2.0, -0.5))).max() < 0.05


def test_ransac_on_the_scene_seeds_and_repeats(scene):
    src, tgt, corr = scene["src"], scene["tgt"], scene["corr"]
    a = _check_ransac(src, tgt, corr, 4096, 0, 1.5 * GR.VOXEL, 0.9)
    b = _check_ransac(src, tgt, corr, 4096, 1, 1.5 * GR.VOXEL, 0.9)
    assert a["best_hypothesis"] != b["best_hypothesis"] and not np.array_equal(a["transformation"], b["transformation"])
    assert a["survivors"] >= 50
    again = REG.ransac_correspondence(_t(src), _t(tgt), _t(corr, np.int32), 1.5 * GR.VOXEL, 0.9, 4096, 0)
    assert all(np.array_equal(np.asarray(again[k]), np.asarray(a[k])) for k in a)
    true = CR.transform(src, scene["truth"])
    assert np.linalg.norm(CR.transform(src, a["transformation"]) - true, axis=1).max() < 3 * GR.VOXEL


def test_ransac_collinear_and_bad_indices():
    line = np.outer(np.arange(40.0), [1.0, 0.0, 0.0]) + [0.0, 2.0, -1.0]         # along an axis: every cross product is exactly zero
    corr = np.stack([np.arange(40), np.arange(40)], 1).astype(np.int32)
    got = _check_ransac(line, line, corr, 257, 0, 0.1, 0.0)
    assert got["status"] == 2 and got["survivors"] == 0 and got["rejected_frame"] > 200 and got["best_hypothesis"] == -1
    assert np.array_equal(got["transformation"], np.eye(4))
    with pytest.raises(RuntimeError, match="no hypothesis survived"):
        REG.ransac_correspondence(_t(line), _t(line), _t(corr, np.int32), 0.1, 0.0, 257, 0)
    bad = corr.copy()
    bad[5, 1] = 40
    bad[6, 0] = -1
    out = REG.ransac_correspondence(_t(line), _t(line), _t(bad, np.int32), 0.1, 0.0, 64, 0, strict=False)
    assert out["status"] & 4


# ---------------------------------------------------------------- end to end
def _scene_clouds(scene):
    from loner_amd.analysis.lidar_map import PointCloud
    s, t = PointCloud(_t(scene["src"])), PointCloud(_t(scene["tgt"]))
    s.normals, t.normals = _t(scene["ns"]), _t(scene["nt"])
    return s, t


def test_feature_matching_returns_the_restated_transformation(scene):
    s, t = _scene_clouds(scene)
    fs, ft = s.compute_fpfh_feature(5 * GR.VOXEL, 32), t.compute_fpfh_feature(5 * GR.VOXEL, 32)
    assert _same_bits(fs.cpu().numpy(), scene["fs"])
    res = REG.registration_ransac_based_on_feature_matching(s, t, fs, ft, False, 1.5 * GR.VOXEL, 0.9, hypotheses=4096, seed=0)
    want = GR.ransac(scene["src"], scene["tgt"], scene["corr"], 4096, 0, 1.5 * GR.VOXEL, 0.9)
    assert _same_bits(res.transformation, want["transformation"])
    idx, d2 = IR.correspondences(CR.transform(scene["src"], want["transformation"]), scene["tgt"], 1.5 * GR.VOXEL)
    assert res.n_correspondences == int((idx >= 0).sum()) and res.fitness == res.n_correspondences / len(scene["src"])
    assert abs(res.inlier_rmse - np.sqrt(d2[idx >= 0].sum() / res.n_correspondences)) < 1e-12


# On the CPU the restatement of the same steps (voxel_down_sample at 0.25, eigh normals towards the viewpoints, FPFH, RANSAC with 4096
# hypotheses, icp_restatement.icp at 0.75 and 0.375) leaves the source's points within 2.48 mm of their true places (seeds 0 and 1, and
# with the centroid orientation); the bound is twice that.
GLOBAL_BOUND = 2 * 0.00248


def test_global_registration_brings_every_point_home(scene):
    from loner_amd.analysis.lidar_map import PointCloud
    s, t = PointCloud(_t(scene["src"])), PointCloud(_t(scene["tgt"]))
    true = CR.transform(scene["src"], scene["truth"])
    for orient in (scene["views"], None):
        res = REG.global_registration(s, t, GR.VOXEL, orient=orient, hypotheses=4096)
        err = np.linalg.norm(CR.transform(scene["src"], res.transformation) - true, axis=1).max()
        print(f"orient {'viewpoints' if orient else 'centroids'}: largest point error {err * 1e3:.3f} mm, fitness {res.fitness:.3f}")
        assert err < GLOBAL_BOUND
    assert len(s) == len(scene["src"]) and s.normals is None          # neither cloud is changed
    rough = REG.global_registration(s, t, GR.VOXEL, orient=scene["views"], refine=False, hypotheses=4096)
    assert np.linalg.norm(CR.transform(scene["src"], rough.transformation) - true, axis=1).max() < 3 * GR.VOXEL


def test_compare_point_clouds_with_global_alignment(scene, tmp_path):
    from loner_amd.analysis.lidar_map import PointCloud, compare_point_clouds
    home = CR.transform(scene["src"], scene["truth"])
    base_align, moved_align, plain_align = {}, {}, {}
    base = compare_point_clouds(PointCloud(_t(home)), PointCloud(_t(scene["tgt"])), str(tmp_path / "a"), 0.1, refine_alignment=True,
                                alignment=base_align)
    how = {"voxel_size": GR.VOXEL, "orient": scene["views"], "hypotheses": 4096}
    moved = compare_point_clouds(PointCloud(_t(scene["src"])), PointCloud(_t(scene["tgt"])), str(tmp_path / "b"), 0.1, refine_alignment=True,
                                 alignment=moved_align, global_alignment=how)
    print(f"accuracy: {base['accuracy']:.5f} m on the unmoved pair, {moved['accuracy']:.5f} m through global alignment")
    assert moved["accuracy"] <= 2 * base["accuracy"]                  # the margin of the bound above
    assert "global" in moved_align and "transformation" in moved_align and "global" not in base_align
    plain = compare_point_clouds(PointCloud(_t(home)), PointCloud(_t(scene["tgt"])), str(tmp_path / "d"), 0.1, refine_alignment=True,
                                 alignment=plain_align, global_alignment=False)
    assert plain == base and plain_align == base_align               # the default keeps today's outputs
