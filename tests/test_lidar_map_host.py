"""The point-cloud restatement (tests/cloud_restatement.py) on hand-worked cases, and the PCD reader / writer (CPU only)."""
import numpy as np
import pytest

from tests import cloud_restatement as CR


def test_voxel_down_sample_points_on_faces_and_negative_coordinates():
    # v = 0.5, min = -1 -> lo = -1.25: ref_coord = (p + 1.25) / 0.5; p = -1, -0.75, -0.25, 0.25 give 0.5, 1, 2, 3 (faces at 1, 2, 3)
    p = np.array([[-1.0, 0, 0], [-0.75, 0, 0], [-0.25, 0, 0], [0.25, 0, 0], [-0.5, 0, 0]])
    out = CR.voxel_down_sample(p, 0.5)
    # voxels along x: -1 -> 0; -0.75 -> 1; -0.5 -> 1 (1.5); -0.25 -> 2; 0.25 -> 3
    assert np.array_equal(out[:, 0], [-1.0, (-0.75 + -0.5) / 2, -0.25, 0.25])
    assert np.array_equal(out[:, 1:], np.zeros((4, 2)))
    q = np.array([[-3.0, -2.0, -1.0], [-3.1, -2.05, -1.2], [2.0, 1.0, 0.5]])
    out = CR.voxel_down_sample(q, 1.0)
    assert out.shape == (2, 3) and np.array_equal(out[1], q[2])
    assert np.array_equal(out[0], (q[0] + q[1]) / 2.0)


def test_voxel_down_sample_one_point_identical_points_and_empty():
    assert np.array_equal(CR.voxel_down_sample(np.array([[1.5, -2.0, 3.25]]), 0.1), [[1.5, -2.0, 3.25]])
    same = np.tile([[0.1, 0.2, 0.3]], (1000, 1))
    out = CR.voxel_down_sample(same, 0.05)
    s = 0.0
    for _ in range(1000):
        s += 0.1
    assert out.shape == (1, 3) and out[0, 0] == s / 1000.0
    assert CR.voxel_down_sample(np.zeros((0, 3)), 0.1).shape == (0, 3)


def test_voxel_down_sample_too_small_voxel_and_non_finite():
    p = np.array([[0.0, 0.0, 0.0], [1000.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="too small"):
        CR.voxel_down_sample(p, 1e-7)                 # 1e-7 * INT_MAX = 214.7 < 1000
    CR.voxel_down_sample(p, 1e-6)
    with pytest.raises(ValueError, match="non-finite"):
        CR.voxel_down_sample(np.array([[0.0, np.nan, 0.0]]), 0.1)


def test_voxel_sum_is_in_index_order_not_pairwise():
    """a voxel whose input-order sum differs from numpy's pairwise np.sum: 1, then 2^-53 many times (each lost against 1)"""
    x = np.concatenate([[1.0], np.full(200, 2.0 ** -53)])
    p = np.stack([x * 1e-3, np.zeros_like(x), np.zeros_like(x)], 1)
    seq = 0.0
    for v in p[:, 0]:
        seq += v
    assert seq != np.sum(p[:, 0])
    out = CR.voxel_down_sample(p, 1.0)
    assert out.shape == (1, 3) and out[0, 0] == seq / len(x)


def test_transform_rounds_each_operation():
    T = np.array([[0.0, -1.0, 0.0, 1.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.25], [0, 0, 0, 1]])
    p = np.array([[1.0, 2.0, 3.0], [-0.5, 0.5, 0.0]])
    assert np.array_equal(CR.transform(p, T), [[-0.5, -1.0, 3.25], [1.0, -2.5, 0.25]])
    rng = np.random.default_rng(2)
    T = np.eye(4)
    T[:3] = rng.normal(size=(3, 4))
    p = rng.normal(size=(100, 3)) * 10
    want = np.array([[((T[i, 0] * a + T[i, 1] * b) + T[i, 2] * c) + T[i, 3] for i in range(3)] for a, b, c in p.tolist()])
    assert np.array_equal(CR.transform(p, T), want)


def test_brute_force_distances_agree_with_a_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3)
    for nq, nt in ((500, 3000), (2000, 700)):
        q = rng.uniform(-5, 5, size=(nq, 3))
        t = rng.uniform(-4, 4, size=(nt, 3))
        d2 = CR.sq_distances(q, t)
        d_kd, _ = cKDTree(t).query(q)
        d = np.sqrt(d2)
        ulp = np.spacing(np.maximum(d, d_kd))
        assert (np.abs(d - d_kd) <= ulp).all()
    assert np.array_equal(CR.sq_distances(q, np.zeros((0, 3))), np.zeros(len(q)))
    assert np.array_equal(CR.sq_distances(t[:10], t), np.zeros(10))


def test_statistics_quirks_on_hand_worked_distances():
    acc = np.array([0.05, 0.2, 0.01, 0.5])          # FP = 2 (> 0.1), TP = 2
    comp = np.array([0.0, 0.3, 0.05])               # FN = 1
    s = CR.statistics(acc, comp, 0.1)
    assert s["precision"] == 2 / 4 and s["recall"] == 2 / 3
    assert s["f-score"] == 2 * (0.5 * (2 / 3)) / (0.5 + 2 / 3 + 1e-8)
    assert s["num_points"] == 4 and s["chamfer_distance"] == acc.mean() + comp.mean()
    # recall counts TP on the estimate and FN on the ground truth: it can exceed what a symmetric count would give
    s = CR.statistics(np.zeros(10), np.array([1.0, 0.0]), 0.1)
    assert s["precision"] == 1.0 and s["recall"] == 10 / 11
    # a threshold equal to a distance is not a miss (strict >)
    s = CR.statistics(np.array([0.1]), np.array([0.1]), 0.1)
    assert s["precision"] == 1.0 and s["recall"] == 1.0 and s["f-score"] == 2 / (2 + 1e-8)


def _pcd(path, fields, sizes, types, rows, data):
    head = ["# .PCD v0.7", "VERSION 0.7", "FIELDS " + " ".join(fields), "SIZE " + " ".join(map(str, sizes)),
            "TYPE " + " ".join(types), "COUNT " + " ".join("1" for _ in fields), f"WIDTH {len(rows)}", "HEIGHT 1",
            "VIEWPOINT 0 0 0 1 0 0 0", f"POINTS {len(rows)}", f"DATA {data}"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if data == "ascii":
            f.write("".join(" ".join(repr(float(v)) for v in r) + "\n" for r in rows).encode())
        else:
            code = {("F", 4): "<f4", ("F", 8): "<f8", ("U", 1): "u1", ("I", 4): "<i4"}
            dt = np.dtype([(f"f{k}", code[(t, s)]) for k, (t, s) in enumerate(zip(types, sizes))])
            rec = np.zeros(len(rows), dtype=dt)
            for k in range(len(fields)):
                rec[f"f{k}"] = [r[k] for r in rows]
            f.write(rec.tobytes())


def test_pcd_round_trips_and_extra_fields(tmp_path):
    from loner_amd.analysis.lidar_map import read_pcd, write_point_cloud
    rng = np.random.default_rng(4)
    p = rng.normal(size=(257, 3)) * 30
    p32 = p.astype(np.float32).astype(np.float64)
    for ascii_ in (False, True):
        path = str(tmp_path / f"c{int(ascii_)}.pcd")
        write_point_cloud(path, p, write_ascii=ascii_)
        head = open(path, "rb").read(300).decode("ascii", "replace")
        assert "FIELDS x y z" in head and "SIZE 4 4 4" in head and "TYPE F F F" in head
        assert np.array_equal(read_pcd(path), p32)
    write_point_cloud(str(tmp_path / "empty.pcd"), np.zeros((0, 3)))
    assert read_pcd(str(tmp_path / "empty.pcd")).shape == (0, 3)
    rows = [(float(a), int(i % 200), float(b), float(c), float(d)) for i, (a, b, c, d) in enumerate(rng.normal(size=(50, 4)))]
    for data in ("binary", "ascii"):
        # F8 x y z with an intensity (U1) and a curvature (F4) in between: x y z come back exactly, the rest is skipped
        path = str(tmp_path / f"extra_{data}.pcd")
        _pcd(path, ["rgb_like", "intensity", "x", "y", "z"], [8, 1, 8, 8, 8], ["F", "U", "F", "F", "F"],
             [(r[0], r[1], r[2], r[3], r[4]) for r in rows], data)
        assert np.array_equal(read_pcd(path), np.array([[r[2], r[3], r[4]] for r in rows]))
        path = str(tmp_path / f"f4_{data}.pcd")
        _pcd(path, ["x", "y", "z", "i"], [4, 4, 4, 4], ["F", "F", "F", "I"], [(r[2], r[3], r[4], r[1]) for r in rows], data)
        want = np.array([[r[2], r[3], r[4]] for r in rows]).astype(np.float32).astype(np.float64)
        assert np.array_equal(read_pcd(path), want)


def test_pcd_binary_compressed_is_rejected(tmp_path):
    from loner_amd.analysis.lidar_map import read_pcd
    path = str(tmp_path / "c.pcd")
    with open(path, "wb") as f:
        f.write(b"VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 1\nHEIGHT 1\nPOINTS 1\nDATA binary_compressed\n")
        f.write(b"\x00" * 20)
    with pytest.raises(ValueError, match="binary_compressed"):
        read_pcd(path)
