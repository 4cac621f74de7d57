"""The mesh-tools restatement (tests/mesh_tools_restatement.py) against independent checkers on the CPU: its labels against scipy's
connected_components on the edge-adjacency graph, its normals against TriangleMesh.compute_vertex_normals bit for bit, its tree sum
against math.fsum, and the argument checks of the new TriangleMesh methods (which fail before any device is touched)."""
import math

import numpy as np
import pytest

from tests import mesh_tools_restatement as MT


def _scipy_labels(triangles):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(triangles)
    rows, cols = [], []
    for users in MT.edge_triangles(triangles).values():
        rows += users[:-1]
        cols += users[1:]
    graph = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    return MT.first_triangle_numbering(connected_components(graph, directed=False)[1])


HAND = {
    "shared edge": ([[0, 1, 2], [2, 1, 3]], [0, 0]),
    "shared vertex": ([[0, 1, 2], [2, 3, 4]], [0, 1]),
    "three on one edge": ([[0, 1, 2], [5, 6, 7], [1, 0, 3], [0, 1, 4]], [0, 1, 0, 0]),
    "duplicate": ([[0, 1, 2], [3, 4, 5], [0, 1, 2]], [0, 1, 0]),
    "repeated index": ([[0, 0, 1], [2, 3, 4], [0, 0, 5], [1, 6, 7]], [0, 1, 0, 2]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    tris, want = HAND[name]
    labels, sizes = MT.connected_triangles(np.array(tris, dtype=np.int32))
    assert labels.tolist() == want and sizes.tolist() == np.bincount(want).tolist()


def test_labels_equal_scipy_connected_components():
    rng = np.random.default_rng(5)
    meshes = [MT.strip(2003)[0], MT.random_shared_mesh()[1], rng.integers(0, 3000, size=(1500, 3)).astype(np.int32),
              np.arange(3 * 300, dtype=np.int32).reshape(-1, 3)]
    for t in meshes:
        labels, sizes = MT.connected_triangles(t)
        assert np.array_equal(labels, _scipy_labels(t))
        assert np.array_equal(sizes, np.bincount(labels)) and sizes.sum() == len(t)
        first = [int(np.flatnonzero(labels == c)[0]) for c in range(len(sizes))]
        assert first == sorted(first)
    assert MT.connected_triangles(meshes[0])[1].tolist() == [2003]
    assert len(MT.connected_triangles(meshes[2])[1]) > 10


def test_restated_normals_equal_numpy_add_at_bit_for_bit():
    from loner_amd.analysis.mesher import TriangleMesh
    for v, t in (MT.random_shared_mesh(), MT.fan(500)):
        mesh = TriangleMesh(v, t).compute_vertex_normals()
        assert mesh.vertex_normals.tobytes() == MT.vertex_normals(v, t).tobytes()
    v, t = MT.random_shared_mesh()
    assert not MT.vertex_normals(v, t)[-7:].any() and MT.vertex_normals(v, t)[:-7].any(1).sum() > 390


def test_tree_sum_stays_within_the_summation_band_of_fsum():
    rng = np.random.default_rng(2)
    for n in (0, 1, 63, 64, 65, 4097, 10001):
        a = (10.0 ** rng.uniform(-6, 0, size=n)).tolist()
        assert abs(MT.tree_sum(a) - math.fsum(a)) <= n * 2.0 ** -53 * math.fsum(a)


def test_restated_select():
    t = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5], [6, 6, 7]], dtype=np.int32)
    out, vmap, n = MT.select(t, 9, triangle_keep=[1, 0, 1, 1], drop_unreferenced=True)
    assert out.tolist() == [[0, 1, 2], [3, 4, 5], [6, 6, 7]] and vmap.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1] and n == 8
    out, vmap, n = MT.select(t, 9, vertex_keep=[1, 1, 1, 0, 1, 1, 1, 1, 1])
    assert out.tolist() == [[0, 1, 2], [5, 5, 6]] and vmap.tolist() == [0, 1, 2, -1, 3, 4, 5, 6, 7] and n == 8


def test_select_components_follows_the_restated_rule():
    from loner_amd.analysis.mesher import select_components
    sizes = np.array([5, 9, 9, 1, 7, 9], dtype=np.int32)
    areas = np.array([1.0, 0.2, 3.0, 0.1, 2.0, 0.5])
    for kw in (dict(min_triangles=6), dict(min_area=0.4), dict(keep_largest=2), dict(min_triangles=6, min_area=0.4, keep_largest=2),
               dict(keep_largest=10), dict(min_triangles=0)):
        want = MT.small_component_keep(sizes, areas, **kw)
        got = select_components(sizes, kw.get("min_triangles"), kw.get("keep_largest"), areas, kw.get("min_area"))
        assert got.tolist() == want.tolist(), kw
    assert select_components(sizes, keep_largest=2).tolist() == [False, True, True, False, False, False]


def test_new_methods_check_their_arguments_before_touching_a_device():
    from loner_amd.analysis.mesher import Mesher, TriangleMesh
    v, t = MT.random_shared_mesh()
    mesh = TriangleMesh(v, t)
    with pytest.raises(ValueError):
        mesh.remove_triangles_by_mask(np.zeros(len(t) - 1, dtype=bool))
    with pytest.raises(ValueError):
        mesh.remove_triangles_by_mask(np.zeros(len(t), dtype=np.float64))
    with pytest.raises(ValueError):
        mesh.remove_vertices_by_mask(np.zeros(len(t), dtype=bool))
    with pytest.raises(ValueError):
        mesh.crop([0.0, 0.0], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        mesh.crop([0.0, 0.0, 2.0], [1.0, 1.0, 1.0])
    for kw in ({}, dict(min_triangles=-1), dict(min_triangles=2.5), dict(min_area=-1.0), dict(min_area=float("nan")), dict(keep_largest=0)):
        with pytest.raises(ValueError):
            mesh.remove_small_components(**kw)
    with pytest.raises(ValueError):
        Mesher.get_mesh(None, "cuda", None, min_component_triangles=-3)
    assert mesh.vertices.shape == v.shape and np.array_equal(mesh.triangles, t)
