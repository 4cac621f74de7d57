"""The restatement of the mesh simplification and smoothing contracts (tests/mesh_filters_restatement.py) pinned with hand-made known
answers, and one sanity check of the smoothing definitions on a noisy sphere.  No GPU."""
import numpy as np
import pytest

from tests import mesh_filters_restatement as MF


def test_two_vertices_in_one_voxel_are_averaged_and_numbered_by_first_occurrence():
    # lo = -0.25: x = 1.0 -> voxel 2, x = 0.0 -> voxel 0, x = 1.1 -> voxel 2; the voxel met first is cluster 0
    v = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.1, 0.0, 0.0]])
    cluster, means = MF.vertex_clusters(v, 0.5)
    assert cluster.dtype == np.int32 and cluster.tolist() == [0, 1, 0]
    assert means.tolist() == [[(1.0 + 1.1) / 2.0, 0.0, 0.0], [0.0, 0.0, 0.0]]


def test_a_vertex_on_a_voxel_face_belongs_to_the_upper_voxel():
    # lo = -0.25, so the faces are at 0.25, 0.75, ...: (0.75 + 0.25) / 0.5 is exactly 2.0
    v = np.array([[0.0, 0.0, 0.0], [0.75, 0.0, 0.0], [0.5, 0.0, 0.0], [np.nextafter(0.75, 0.0), 0.0, 0.0]])
    cluster, means = MF.vertex_clusters(v, 0.5)
    assert cluster.tolist() == [0, 1, 2, 2]
    assert means[1].tolist() == [0.75, 0.0, 0.0] and means[2, 0] == (0.5 + np.nextafter(0.75, 0.0)) / 2.0


def test_cluster_status_rules():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    assert MF.cluster_status(v, 0.5) == 0 and MF.cluster_status(np.zeros((0, 3)), 0.5) == 0
    assert MF.cluster_status(np.array([[0.0, np.nan, 0.0]]), 0.5) == 1 and MF.cluster_status(np.array([[np.inf, 0.0, 0.0]]), 0.5) == 1
    assert MF.cluster_status(v, 1e-10) == 2                         # 1e-10 * INT_MAX = 0.21 < 3
    assert MF.cluster_status(np.array([[0.0, 0.0, 0.0], [1e6, 1e6, 1e6]]), 1e-3) == 4      # 30 bits per axis
    with pytest.raises(ValueError):
        MF.vertex_clusters(np.array([[0.0, np.nan, 0.0]]), 0.5)


def test_the_rotations_of_a_triangle_are_one_class_and_its_mirror_image_another():
    tris = [[5, 7, 9], [7, 9, 5], [9, 5, 7], [5, 9, 7], [9, 7, 5], [7, 5, 9]]
    canonical, keep, kept, degenerate = MF.unique_triangles(tris)
    assert canonical.tolist() == [[5, 7, 9]] * 3 + [[5, 9, 7]] * 3
    assert keep.tolist() == [1, 0, 0, 1, 0, 0] and kept == 2 and degenerate == 0


def test_the_tie_rule_of_the_rotation():
    # open3d compares with <=: [0,0,1] and [0,1,0] stay, [1,0,0] rotates to [0,0,1]
    assert MF.canonical_triple(0, 0, 1) == (0, 0, 1)
    assert MF.canonical_triple(0, 1, 0) == (0, 1, 0)
    assert MF.canonical_triple(1, 0, 0) == (0, 0, 1)
    assert MF.canonical_triple(2, 1, 1) == (1, 1, 2) and MF.canonical_triple(1, 2, 1) == (1, 2, 1)
    canonical, keep, kept, degenerate = MF.unique_triangles([[0, 0, 1], [1, 0, 0], [0, 1, 0], [3, 3, 3]])
    assert keep.tolist() == [1, 0, 1, 1] and kept == 3 and degenerate == 4
    assert MF.unique_triangles([[0, 0, 1], [1, 0, 0], [0, 1, 2]], drop_degenerate=True)[1].tolist() == [0, 0, 1]


def test_a_vertex_map_is_applied_before_the_rotation():
    canonical, keep, kept, degenerate = MF.unique_triangles([[0, 1, 2], [3, 4, 5], [2, 3, 0]], vertex_map=[4, 4, 1, 0, 4, 1],
                                                            drop_degenerate=True)
    assert canonical.tolist() == [[1, 4, 4], [0, 4, 1], [0, 4, 1]]
    assert keep.tolist() == [0, 1, 0] and kept == 1 and degenerate == 1


def test_adjacency_known_answers():
    # vertex 4 is in no triangle; edge 1-2 is shared by two triangles; [5, 5, 6] repeats an index: 5 is not its own neighbour
    row_start, neighbours = MF.vertex_adjacency([[0, 1, 2], [2, 1, 3], [5, 5, 6]], 7)
    assert row_start.tolist() == [0, 2, 5, 8, 10, 10, 11, 12]
    assert neighbours.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2, 6, 5]


def test_a_tetrahedron_smoothed_by_hand():
    v, t = MF.TETRAHEDRON
    # simple: every vertex has the other three as neighbours, so all become the mean of the four (the sums are exact)
    assert MF.smooth(v, t, 1, 0).tolist() == [[0.25, 0.5, 1.0]] * 4
    # Laplacian, vertex 0 at the origin: neighbours 1, 2, 3 at distances 1, 2, 4
    w1, w2, w4 = 1.0 / (1.0 + 1e-12), 1.0 / (2.0 + 1e-12), 1.0 / (4.0 + 1e-12)
    W = ((0.0 + w1) + w2) + w4
    want = [0.0 + 0.5 * ((0.0 + w1 * 1.0) / W - 0.0), 0.0 + 0.5 * (((0.0 + w1 * 0.0) + w2 * 2.0) / W - 0.0),
            0.0 + 0.5 * ((((0.0 + w1 * 0.0) + w2 * 0.0) + w4 * 4.0) / W - 0.0)]
    got = MF.smooth(v, t, 1, 1, 0.5)
    assert got[0].tolist() == want
    assert np.abs(got[0] - 2.0 / 7.0).max() < 1e-11
    # vertex 1 at (1, 0, 0): neighbours 0, 2, 3 at distances 1, sqrt 5, sqrt 17
    w = [1.0 / (1.0 + 1e-12), 1.0 / (np.sqrt(5.0) + 1e-12), 1.0 / (np.sqrt(17.0) + 1e-12)]
    W = ((0.0 + w[0]) + w[1]) + w[2]
    assert got[1, 0] == 1.0 + 0.5 * ((((0.0 + w[0] * 0.0) + w[1] * 0.0) + w[2] * 0.0) / W - 1.0)
    assert got[1, 1] == 0.0 + 0.5 * ((((0.0 + w[0] * 0.0) + w[1] * 2.0) + w[2] * 0.0) / W - 0.0)


def test_the_factor_alternates_and_zero_steps_change_nothing():
    v, t = MF.TETRAHEDRON
    assert MF.smooth(v, t, 0, 1).tobytes() == v.tobytes()
    row_start, neighbours = MF.vertex_adjacency(t, 4)
    by_hand = MF.smooth_step(MF.smooth_step(MF.smooth_step(v, row_start, neighbours, 1, 0.5), row_start, neighbours, 1, -0.53),
                             row_start, neighbours, 1, 0.5)
    assert MF.smooth(v, t, 3, 1, 0.5, -0.53).tobytes() == by_hand.tobytes()
    assert MF.taubin(v, t, 1).tobytes() == MF.smooth(v, t, 2, 1, 0.5, -0.53).tobytes()


def test_an_isolated_vertex_stays_where_it_is():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [7.0, 8.0, 9.0]])
    for kind in (0, 1):
        out = MF.smooth(v, [[0, 1, 2]], 2, kind)
        assert out[3].tolist() == [7.0, 8.0, 9.0] and np.isfinite(out).all() and not np.array_equal(out[:3], v[:3])


def test_adjacent_coincident_vertices_stay_finite():
    v = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    out = MF.smooth(v, [[0, 1, 2]], 3, 1, 0.5, -0.53)
    assert np.isfinite(out).all()


def test_simplification_of_a_square():
    # four corners of a 1 x 1 square and a centre close to corner 0: the centre merges into corner 0's voxel
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.1, 0.1, 0.0]])
    t = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], dtype=np.int32)
    sv, st = MF.simplify_vertex_clustering(v, t, 0.5)
    assert sv.tolist() == [[0.05, 0.05, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]]
    assert st.tolist() == [[0, 1, 2], [0, 2, 3]]                    # [0,1,0] and [3,0,0] are degenerate


def test_taubin_smooths_a_noisy_sphere_without_shrinking_it():
    """a 24 x 48 latitude-longitude unit sphere with 2 % radial noise, ten iterations: radial std 0.0197 -> 0.0085, mean radius
    0.9992 -> 1.0011 with Taubin and -> 0.9637 with the plain Laplacian filter"""
    v, t = MF.noisy_sphere(24, 48, 0.02)
    r0 = np.linalg.norm(v, axis=1)
    r_taubin = np.linalg.norm(MF.taubin(v, t, 10), axis=1)
    r_laplacian = np.linalg.norm(MF.smooth(v, t, 10, 1, 0.5), axis=1)
    print(f"radial std {r0.std():.4f} -> {r_taubin.std():.4f}; mean radius {r0.mean():.4f} -> Taubin {r_taubin.mean():.4f}, "
          f"Laplacian {r_laplacian.mean():.4f}")
    assert r_taubin.std() < r0.std()
    assert abs(r_taubin.mean() - r0.mean()) < 0.01 * r0.mean()
    assert r_laplacian.mean() < r_taubin.mean()


def test_the_generators_exercise_every_path():
    v, t = MF.height_field()
    cluster, means = MF.vertex_clusters(v, 0.25)
    _, keep, kept, degenerate = MF.unique_triangles(t, cluster, drop_degenerate=True)
    duplicates = len(t) - degenerate - kept
    print(f"height field: {len(v)} vertices in {len(means)} clusters; {len(t)} triangles -> {degenerate} degenerate, {duplicates} "
          f"duplicates, {kept} kept")
    assert len(v) == 1600 and len(t) == 3042 and degenerate > 0 and duplicates > 0 and kept > 0
    assert not np.array_equal(cluster, np.sort(cluster))            # shuffled: first occurrence is not spatial order
    fv, ft = MF.fan()
    row_start, _ = MF.vertex_adjacency(ft, len(fv))
    assert row_start[1] == 10000
