"""The numpy restatement of mesh sampling (tests/cloud_tools_restatement.py) against known answers, and the argument checks of the
ground-truth map builder: nothing here needs a GPU."""
import numpy as np
import pytest

from tests import cloud_tools_restatement as TR

# philox4x32_10(counter_lo, counter_hi, key) -> (x, y, z, w), printed by a stand-alone host build of loner_amd/csrc/lnr_common.h; the
# first row is Random123's known answer for an all-zero counter and key
PHILOX = [
    ((0x0, 0x0, 0x0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0x1, 0x4D45534800000000, 0x0), (0x9AEB5D8C, 0x157B3EEC, 0xBA51A8E9, 0xF4B6CB51)),
    ((0xFFFFFFFF, 0x4D45534800000000, 0xDEADBEEFCAFEF00D), (0xEF063B69, 0xBC8A2B53, 0xECB996CD, 0xBA69466E)),
    ((0x100000005, 0x4D45534800000000, 0x7), (0x937FE0A7, 0x5DE80DFA, 0x43043D76, 0xBF6D7F47)),
    ((0x7FFFEFFF, 0x4D45534800000000, 0xFFFFFFFFFFFFFFFF), (0x3221B0C5, 0x2D05749D, 0x4EB0D65A, 0x652BE3F3)),
]

SQUARE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], [3.0, 0.0, 0.0], [3.0, 1.0, 0.0],
                   [0.5, 0.0, 0.0]])


def test_restated_philox_equals_the_host_build():
    for (lo, hi, key), want in PHILOX:
        got = TR.philox4x32_10(np.array([lo], dtype=np.uint64), hi, key)
        assert tuple(int(g[0]) for g in got) == want
    lo = np.array([c[0][0] for c in PHILOX[1:]], dtype=np.uint64)          # vectorised over counters, one key
    got = TR.philox4x32_10(lo, TR.STREAM_MESH, 0)
    assert tuple(int(g[0]) for g in got) == PHILOX[1][1]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096, 4097, 5000, 64 ** 2 * 3 + 17])
def test_tree_prefix_of_integers_is_the_cumulative_sum(n):
    a = np.random.default_rng(n).integers(0, 1000, size=n)
    assert np.array_equal(TR.tree_prefix(a), np.cumsum(a))
    assert np.array_equal(TR.tree_prefix(a, np.maximum), np.maximum.accumulate(a))
    f = a.astype(np.float64)                                               # integers below 2^53: every order is exact
    assert np.array_equal(TR.tree_prefix(f), np.cumsum(f))


def _counts(vertices, triangles, n):
    _, owner = TR.mesh_sample(vertices, triangles, n, seed=3)
    return np.bincount(owner, minlength=len(triangles)).tolist()


def test_ownership_on_known_meshes():
    pair = [[0, 1, 3], [0, 4, 3]]                                          # areas 1 : 3
    assert TR.triangle_areas(SQUARE, pair).tolist() == [0.5, 1.5]
    assert _counts(SQUARE, pair, 8) == [2, 6]
    equal = [[0, 1, 2], [0, 2, 3]]
    assert _counts(SQUARE, equal, 1) == [1, 0]                             # round(0.5 * 1) = 1: half away from zero
    degenerate = [[0, 1, 2], [0, 6, 1], [0, 2, 3]]                         # the middle one's vertices are collinear
    assert TR.triangle_areas(SQUARE, degenerate)[1] == 0.0
    c = _counts(SQUARE, degenerate, 101)
    assert c[1] == 0 and c[0] + c[2] == 101 and abs(c[0] - c[2]) == 1
    assert len(TR.mesh_sample(SQUARE, [[0, 6, 1]], 10, seed=0)[0]) == 0    # no area: no points


def test_round_half_away_from_zero():
    x = np.array([0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 2.4999999999999996, 4503599627370497.0])
    assert TR.round_half_away(x).tolist() == [0.0, 0.0, 1.0, 2.0, 3.0, 2.0, 4503599627370497.0]


def test_uniform_over_sixteen_congruent_subtriangles():
    """One triangle, 2^16 points: the 16 congruent triangles its sides' quarter points cut it into (10 upright, 6 inverted) receive
    equal shares; chi-square with 15 degrees of freedom below its 1 - 1e-6 quantile."""
    from scipy.stats import chi2
    n = 2 ** 16
    a, b, c = TR.barycentric_weights(n, seed=11)
    i, j, k = (np.minimum(np.floor(4 * w).astype(int), 3) for w in (a, b, c))
    upright = i + j + k == 3
    assert (upright | (i + j + k == 2)).all()
    cell = (i * 4 + j) * 2 + upright
    counts = np.unique(cell, return_counts=True)[1]
    assert len(counts) == 16
    stat = float(((counts - n / 16) ** 2 / (n / 16)).sum())
    print(f"chi-square {stat:.2f}, bound {chi2.ppf(1 - 1e-6, 15):.2f}")
    assert stat < chi2.ppf(1 - 1e-6, 15)


def test_barycentrics_are_convex_weights():
    a, b, c = TR.barycentric_weights(2 ** 16, seed=5)
    for w in (a, b, c):
        assert (w >= 0).all() and (w <= 1).all()
    assert (np.abs(((a + b) + c) - 1.0) <= 2 * 2.0 ** -52).all()


def _tum(times):
    rows = np.zeros((len(times), 8))
    rows[:, 0] = times
    rows[:, 7] = 1.0
    return rows


def test_build_lidar_map_argument_errors():
    from loner_amd.analysis.gt_map import build_lidar_map
    scan = [(np.ones((4, 3)), np.full(4, 0.5))]
    with pytest.raises(ValueError, match="strictly increasing"):
        build_lidar_map(scan, _tum([0.0, 1.0, 1.0]), device="cpu")
    with pytest.raises(ValueError, match="strictly increasing"):
        build_lidar_map(scan, _tum([0.0, 2.0, 1.0]), device="cpu")
    with pytest.raises(ValueError, match="at least 2 poses"):
        build_lidar_map(scan, _tum([0.0]), device="cpu")
    with pytest.raises(ValueError, match="TUM rows"):
        build_lidar_map(scan, np.zeros((3, 7)), device="cpu")
    with pytest.raises(ValueError, match="voxel_size"):
        build_lidar_map(scan, _tum([0.0, 1.0]), voxel_size=0.0, device="cpu")
    with pytest.raises(ValueError, match="scan 0"):
        build_lidar_map([(np.ones((4, 3)), np.full(5, 0.5))], _tum([0.0, 1.0]), device="cpu")
    with pytest.raises(ValueError, match="scan 0"):
        build_lidar_map([(np.ones((4, 2)), np.full(4, 0.5))], _tum([0.0, 1.0]), device="cpu")


def test_mask_by_distance_argument_errors():
    from loner_amd.analysis.gt_map import mask_by_distance
    from loner_amd.analysis.lidar_map import PointCloud
    cloud = PointCloud(np.zeros((2, 3)), device="cpu")
    with pytest.raises(ValueError, match="PointClouds"):
        mask_by_distance(np.zeros((2, 3)), cloud)
    with pytest.raises(ValueError, match="PointClouds"):
        mask_by_distance(cloud, np.zeros((2, 3)))
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            mask_by_distance(cloud, cloud, threshold=bad)


def test_segment_rotation_vectors_match_scipy():
    from scipy.spatial.transform import Rotation
    from loner_amd.analysis.gt_map import segment_rotvecs
    q = Rotation.random(40, random_state=2).as_quat()
    q = np.concatenate([q, q[-1:], -q[-1:]])                               # an identity segment, and the same rotation with -q
    r = Rotation.from_quat(q)
    want = (r[:-1].inv() * r[1:]).as_rotvec()
    got = segment_rotvecs(q)
    assert np.abs(got - want).max() < 1e-14
    assert np.abs(got[-2:]).max() < 1e-15
