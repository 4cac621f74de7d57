"""Mesh simplification and smoothing on the MI355X against the plain-Python restatement (tests/mesh_filters_restatement.py): cluster
labels and means, canonical triples and keep masks, the adjacency CSR and the smoothed positions, all bit for bit, and the TriangleMesh
and Mesher.get_mesh workflows built on them."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_filters_restatement as MF
from tests import mesh_tools_restatement as MT
from tests import test_gpu_mesh_tools as TOOLS
from tests.test_gpu_mesh_tools import mesher  # noqa: F401  (the module-scoped fixture: the trained synthetic map behind a Mesher)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_t, _tris, _same_bits = TOOLS._t, TOOLS._tris, TOOLS._same_bits


# ---------------------------------------------------------------- inputs, built once
@functools.lru_cache(maxsize=None)
def _grid():
    return MF.height_field()


GRID_VOXEL = 0.25           # 2.5 spacings


@functools.lru_cache(maxsize=None)
def _fan():
    return MF.fan(10000)


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(vertices fp64 [V,3], voxel_size)"""
    rng = np.random.default_rng(5)
    if name == "empty":
        return np.zeros((0, 3)), 0.5
    if name == "one":
        return np.array([[1.5, -2.0, 0.25]]), 0.5
    if name == "coincident":
        return np.tile([[0.3, 0.1, -7.0]], (300, 1)), 0.2
    if name == "faces":                                 # lo = -0.25 and faces every 0.5: every odd multiple of 0.25 lies on one
        k = np.arange(9) * 0.25
        v = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
        return v[rng.permutation(len(v))], 0.5
    if name == "grid":
        return _grid()[0], GRID_VOXEL
    if name == "long run":                              # 5 000 single-vertex voxels (more clusters than one 2 048-element scan tile)
        lattice = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), np.arange(13.0), indexing="ij"), -1).reshape(-1, 3)
        crowd = lattice[5100] + rng.uniform(-0.3, 0.3, (1000, 3))      # and one voxel holding 1 000
        v = np.concatenate([lattice[:5000], crowd])
        return v[rng.permutation(len(v))], 1.0
    assert name == "wide key"                           # 12 bits per axis: 36 key bits, five digit passes
    return rng.uniform(0.0, 4000.0, (3000, 3)), 1.0


CLOUDS = ["empty", "one", "coincident", "faces", "grid", "long run", "wide key"]


@functools.lru_cache(maxsize=None)
def _want_clusters(name):
    return MF.vertex_clusters(*_cloud(name))


def _gpu_clusters(v, voxel):
    from loner_amd import ops
    cluster, means = ops.mesh_vertex_clusters(_t(v), voxel)
    return cluster.cpu().numpy(), means.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _triangles(name):
    """(triangles int32 [F,3], n_vertices, vertex_map or None, n_mapped or None)"""
    if name == "empty":
        return np.zeros((0, 3), dtype=np.int32), 4, None, None
    if name == "rotations":
        return np.array([[5, 7, 9], [7, 9, 5], [9, 5, 7], [5, 9, 7], [9, 7, 5], [7, 5, 9], [0, 0, 1], [1, 0, 0], [0, 1, 0]],
                        dtype=np.int32), 10, None, None
    if name in ("duplicate", "repeated index", "top indices"):
        tris, n_vertices = TOOLS._topology(name)
        return tris, n_vertices, None, None
    if name == "strip":                                 # 100 003 triangles, then copies of 700 of them: as stored, rotated, mirrored
        tris, n_vertices = MT.strip(100003)
        pick = np.random.default_rng(9).choice(len(tris), 700, replace=False)
        extra = np.concatenate([tris[pick[:300]], tris[pick[300:500]][:, [1, 2, 0]], tris[pick[500:]][:, [0, 2, 1]]])
        return np.ascontiguousarray(np.concatenate([tris, extra]), dtype=np.int32), n_vertices, None, None
    assert name == "grid clusters"
    cluster, means = _want_clusters("grid")
    return _grid()[1], len(cluster), cluster, len(means)


TRIANGLES = ["empty", "rotations", "duplicate", "repeated index", "top indices", "strip", "grid clusters"]


def _gpu_unique(name, drop):
    from loner_amd import ops
    tris, n_vertices, vmap, n_mapped = _triangles(name)
    canonical, keep, kept, degenerate = ops.mesh_unique_triangles(_tris(tris), n_vertices, None if vmap is None else _t(vmap, np.int32),
                                                                  n_mapped, drop_degenerate=drop)
    return canonical.cpu().numpy(), keep.cpu().numpy(), kept, degenerate


@functools.lru_cache(maxsize=None)
def _want_unique(name, drop):
    tris, _, vmap, _ = _triangles(name)
    return MF.unique_triangles(tris, vmap, drop)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "grid":
        return _grid()
    if name == "fan":
        return _fan()
    assert name == "hand"       # vertex 4 in no triangle, edge 1-2 shared by two triangles, a repeated index
    return np.arange(21, dtype=np.float64).reshape(7, 3) ** 1.5, np.array([[0, 1, 2], [2, 1, 3], [5, 5, 6]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _want_adjacency(name):
    v, t = _mesh(name)
    return MF.vertex_adjacency(t, len(v))


def _gpu_adjacency(name):
    from loner_amd import ops
    v, t = _mesh(name)
    row_start, neighbours = ops.mesh_vertex_adjacency(_tris(t), len(v))
    return row_start.cpu().numpy(), neighbours.cpu().numpy()


KINDS = {"simple": 0, "laplacian": 1}


@functools.lru_cache(maxsize=None)
def _want_smooth(name, kind, steps):
    """the restated positions after `steps` steps with the factors 0.5 / -0.53, each step computed once"""
    v, t = _mesh(name)
    if steps == 0:
        return v
    row_start, neighbours = _want_adjacency(name)
    return MF.smooth_step(_want_smooth(name, kind, steps - 1), row_start, neighbours, KINDS[kind], 0.5 if steps % 2 == 1 else -0.53)


def _gpu_smooth(name, kind, steps, lam=0.5, mu=-0.53):
    from loner_amd import ops
    v, t = _mesh(name)
    row_start, neighbours = _want_adjacency(name)
    return ops.mesh_smooth(_t(v), _t(row_start, np.int32), _t(neighbours, np.int32), steps, kind, lam, mu).cpu().numpy()


# ---------------------------------------------------------------- clusters
@pytest.mark.parametrize("name", CLOUDS)
def test_vertex_clusters_equal_the_restatement(name):
    v, voxel = _cloud(name)
    want_cluster, want_means = _want_clusters(name)
    cluster, means = _gpu_clusters(v, voxel)
    sizes = np.bincount(want_cluster) if len(want_cluster) else np.zeros(1, dtype=np.int64)
    print(f"{name}: {len(v)} vertices, {len(want_means)} clusters, largest {sizes.max()}")
    assert cluster.dtype == np.int32 and means.dtype == np.float64
    assert means.shape == want_means.shape, f"{name}: m = {len(means)}, restated {len(want_means)}"
    assert _same_bits(cluster, want_cluster), f"{name}: {int((cluster != want_cluster).sum())} labels differ"
    assert _same_bits(means, want_means), f"{name}: {int((means != want_means).any(1).sum())} means differ"


def test_cluster_fixtures_are_what_they_claim():
    cluster, means = _want_clusters("long run")
    assert len(means) == 5001 and np.bincount(cluster).max() == 1000
    assert len(_want_clusters("coincident")[1]) == 1
    v, voxel = _cloud("wide key")
    assert sum(int(x).bit_length() for x in np.floor((v.max(0) - (v.min(0) - 0.5 * voxel)) / voxel)) > 32
    cluster, _ = _want_clusters("grid")
    assert not np.array_equal(cluster, np.sort(cluster))            # first-occurrence numbering is not the key order
    v, voxel = _cloud("faces")
    assert ((v[:, 0] + 0.25) / voxel == np.floor((v[:, 0] + 0.25) / voxel)).sum() > 100


def test_cluster_errors():
    from loner_amd import ops
    v = _grid()[0].copy()
    v[77, 1] = np.nan
    with pytest.raises(RuntimeError, match="1 vertices with non-finite"):
        ops.mesh_vertex_clusters(_t(v), 0.25)
    v[5, 0] = np.inf
    with pytest.raises(RuntimeError, match="2 vertices with non-finite"):
        ops.mesh_vertex_clusters(_t(v), 0.25)
    assert MF.cluster_status(_grid()[0], 1e-10) == 2
    with pytest.raises(RuntimeError, match="too small"):
        ops.mesh_vertex_clusters(_t(_grid()[0]), 1e-10)
    wide = np.array([[0.0, 0.0, 0.0], [1e6, 1e6, 1e6]])
    assert MF.cluster_status(wide, 1e-3) == 4
    with pytest.raises(RuntimeError, match="64 bits"):
        ops.mesh_vertex_clusters(_t(wide), 1e-3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size must be finite and > 0"):
            ops.mesh_vertex_clusters(_t(_grid()[0]), bad)


# ---------------------------------------------------------------- unique triangles
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("name", TRIANGLES)
def test_unique_triangles_equal_the_restatement(name, drop):
    want_canonical, want_keep, want_kept, want_degenerate = _want_unique(name, drop)
    canonical, keep, kept, degenerate = _gpu_unique(name, drop)
    print(f"{name}, drop_degenerate={drop}: {len(want_keep)} triangles, {want_degenerate} degenerate, {want_kept} kept")
    assert canonical.dtype == np.int32 and keep.dtype == np.uint8
    assert _same_bits(canonical, want_canonical), f"{name}: {int((canonical != want_canonical).any(1).sum())} triples differ"
    assert _same_bits(keep, want_keep), f"{name}: {int((keep != want_keep).sum())} flags differ"
    assert (kept, degenerate) == (want_kept, want_degenerate)


def test_unique_triangle_fixtures_exercise_every_path():
    _, keep, kept, degenerate = _want_unique("grid clusters", True)
    duplicates = len(keep) - degenerate - kept
    print(f"grid through its clusters: {len(keep)} triangles -> {degenerate} degenerate, {duplicates} duplicates, {kept} kept")
    assert degenerate > 0 and duplicates > 0 and kept > 0
    _, keep, kept, degenerate = _want_unique("strip", False)
    assert len(keep) == 100703 and kept == 100003 + 200 and degenerate == 0      # the mirrored copies are classes of their own
    assert _want_unique("rotations", False)[1].tolist() == [1, 0, 0, 1, 0, 0, 1, 0, 1]
    assert _want_unique("top indices", False)[0].max() == 2 ** 31 - 2


@pytest.mark.parametrize("bad", [-1, 1600, 2 ** 31 - 1])
def test_an_index_out_of_range_raises(bad):
    from loner_amd import ops
    v, t = _grid()
    t = t.copy()
    t[1234, 1] = bad
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_unique_triangles(_tris(t), len(v))
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_vertex_adjacency(_tris(t), len(v))
    cluster, means = _want_clusters("grid")
    vmap = cluster.copy()
    vmap[int(_grid()[1][0, 0])] = bad if bad < 0 else len(means)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_unique_triangles(_tris(_grid()[1]), len(v), _t(vmap, np.int32), len(means))


def test_argument_checks():
    from loner_amd import ops
    v, t = _grid()
    with pytest.raises(ValueError, match="vertex_map int32"):
        ops.mesh_unique_triangles(_tris(t), len(v), _t(np.zeros(len(v) - 1), np.int32), 5)
    with pytest.raises(ValueError, match="vertex_map int32"):
        ops.mesh_unique_triangles(_tris(t), len(v), _t(np.zeros(len(v)), np.int32))
    with pytest.raises(ValueError, match="triangles int32"):
        ops.mesh_vertex_adjacency(_t(t, np.int64), len(v))
    row_start, neighbours = (_t(a, np.int32) for a in _want_adjacency("grid"))
    with pytest.raises(ValueError, match="kind"):
        ops.mesh_smooth(_t(v), row_start, neighbours, 1, "taubin")
    with pytest.raises(ValueError, match="n_steps"):
        ops.mesh_smooth(_t(v), row_start, neighbours, -1)
    with pytest.raises(ValueError, match="row_start int32"):
        ops.mesh_smooth(_t(v), row_start[:-1], neighbours, 1)
    with pytest.raises(ValueError, match="finite"):
        ops.mesh_smooth(_t(v), row_start, neighbours, 1, "laplacian", float("nan"))
    broken = _want_adjacency("grid")[1].copy()
    broken[10] = len(v)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_smooth(_t(v), row_start, _t(broken, np.int32), 2)


# ---------------------------------------------------------------- adjacency
@pytest.mark.parametrize("name", ["hand", "grid", "fan"])
def test_adjacency_equals_the_restatement(name):
    want_rows, want_neighbours = _want_adjacency(name)
    row_start, neighbours = _gpu_adjacency(name)
    print(f"{name}: {len(want_rows) - 1} vertices, {len(want_neighbours)} neighbours, longest row {np.diff(want_rows).max()}")
    assert row_start.dtype == np.int32 and neighbours.dtype == np.int32
    assert _same_bits(row_start, want_rows) and _same_bits(neighbours, want_neighbours)


def test_adjacency_known_answers():
    row_start, neighbours = _gpu_adjacency("hand")
    assert row_start.tolist() == [0, 2, 5, 8, 10, 10, 11, 12]       # vertex 4 has no row; 5 is not its own neighbour
    assert neighbours.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2, 6, 5]
    assert np.diff(_gpu_adjacency("fan")[0])[0] == 10000
    from loner_amd import ops
    row_start, neighbours = ops.mesh_vertex_adjacency(_tris(np.zeros((0, 3))), 3)
    assert row_start.tolist() == [0, 0, 0, 0] and neighbours.shape[0] == 0


# ---------------------------------------------------------------- smoothing
@pytest.mark.parametrize("steps", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["simple", "laplacian"])
@pytest.mark.parametrize("name", ["grid", "fan"])
def test_smoothing_equals_the_restatement(name, kind, steps):
    want = _want_smooth(name, kind, steps)
    got = _gpu_smooth(name, kind, steps)
    moved = np.abs(want - _mesh(name)[0]).max()
    print(f"{name}, {kind}, {steps} steps: largest move {moved:.3g}, largest difference {np.abs(got - want).max():.3g}")
    assert (moved > 0) == (steps > 0)
    assert _same_bits(got, want), f"{int((got != want).any(1).sum())} vertices differ"


def test_the_taubin_factors_alternate_from_lambda():
    v, t = _mesh("grid")
    got = _gpu_smooth("grid", "laplacian", 2, 0.5, -0.53)
    assert _same_bits(got, MF.taubin(v, t, 1))
    assert not _same_bits(got, _gpu_smooth("grid", "laplacian", 2, -0.53, 0.5))
    from loner_amd import ops
    row_start, neighbours = (_t(a, np.int32) for a in _want_adjacency("grid"))
    same_factor = ops.mesh_smooth(_t(v), row_start, neighbours, 2, "laplacian", 0.5).cpu().numpy()      # mu defaults to lambda
    assert _same_bits(same_factor, MF.smooth(v, t, 2, 1, 0.5, 0.5))


def test_smoothing_leaves_its_input_alone():
    from loner_amd import ops
    v, t = _mesh("grid")
    dev = _t(v)
    row_start, neighbours = (_t(a, np.int32) for a in _want_adjacency("grid"))
    for steps in (0, 1, 2):
        out = ops.mesh_smooth(dev, row_start, neighbours, steps)
        assert out.data_ptr() != dev.data_ptr() and _same_bits(dev.cpu().numpy(), v)


def test_coincident_neighbours_and_an_isolated_vertex():
    from loner_amd import ops
    v = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [7.0, 8.0, 9.0]])
    t = np.array([[0, 1, 2]], dtype=np.int32)
    row_start, neighbours = ops.mesh_vertex_adjacency(_tris(t), 4)
    for kind in KINDS:
        for steps in (1, 2, 3):
            got = ops.mesh_smooth(_t(v), row_start, neighbours, steps, kind, 0.5, -0.53).cpu().numpy()
            assert np.isfinite(got).all() and got[3].tolist() == [7.0, 8.0, 9.0]
            assert _same_bits(got, MF.smooth(v, t, steps, KINDS[kind], 0.5, -0.53))


# ---------------------------------------------------------------- determinism
def test_two_runs_give_the_same_bits():
    v, voxel = _cloud("long run")
    a, b = _gpu_clusters(v, voxel), _gpu_clusters(v, voxel)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    a, b = _gpu_unique("strip", True), _gpu_unique("strip", True)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and a[2:] == b[2:]
    a, b = _gpu_adjacency("fan"), _gpu_adjacency("fan")
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    assert _same_bits(_gpu_smooth("fan", "laplacian", 3), _gpu_smooth("fan", "laplacian", 3))


# ---------------------------------------------------------------- workflows
def _triangle_mesh(name="grid"):
    from loner_amd.analysis.mesher import TriangleMesh
    return TriangleMesh(*_mesh(name))


def test_simplify_vertex_clustering_equals_the_restatement():
    mesh = _triangle_mesh().compute_vertex_normals()
    want_v, want_t = MF.simplify_vertex_clustering(*_grid(), GRID_VOXEL)
    out = mesh.simplify_vertex_clustering(GRID_VOXEL, device=DEV)
    print(f"grid at {GRID_VOXEL}: {len(mesh.vertices)} vertices, {len(mesh.triangles)} triangles -> {len(want_v)}, {len(want_t)}")
    assert out is not mesh and _same_bits(mesh.vertices, _grid()[0]) and _same_bits(mesh.triangles, _grid()[1])
    assert _same_bits(out.vertices, want_v) and _same_bits(out.triangles, want_t)
    assert 0 < len(want_t) < len(mesh.triangles) and not out.has_vertex_normals()
    t = out.triangles
    assert ((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])).all() and len(np.unique(t, axis=0)) == len(t)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size must be finite and > 0"):
            mesh.simplify_vertex_clustering(bad, device=DEV)


def test_remove_duplicated_triangles_keeps_the_first_of_each_class():
    from loner_amd.analysis.mesher import TriangleMesh
    tris, n_vertices, _, _ = _triangles("strip")
    tris = np.concatenate([tris, [[3, 3, 4], [4, 3, 3], [3, 4, 3]]]).astype(np.int32)   # degenerate ones are treated like any other
    v = np.random.default_rng(2).normal(size=(n_vertices, 3))
    mesh = TriangleMesh(v, tris).compute_vertex_normals()
    normals = mesh.vertex_normals.copy()
    keep = MF.unique_triangles(tris)[1].astype(bool)
    assert mesh.remove_duplicated_triangles(device=DEV) is mesh
    assert _same_bits(mesh.triangles, tris[keep]) and len(mesh.triangles) == 100003 + 200 + 2
    assert _same_bits(mesh.vertices, v) and _same_bits(mesh.vertex_normals, normals)


def test_the_smoothing_filters_equal_the_restatement():
    v, t = _grid()
    mesh = _triangle_mesh().compute_vertex_normals()
    for out, want in ((mesh.filter_smooth_simple(3, device=DEV), MF.smooth(v, t, 3, 0)),
                      (mesh.filter_smooth_laplacian(2, 0.4, device=DEV), MF.smooth(v, t, 2, 1, 0.4)),
                      (mesh.filter_smooth_taubin(2, device=DEV), MF.taubin(v, t, 2)),
                      (mesh.filter_smooth_taubin(1, 0.3, -0.31, device=DEV), MF.smooth(v, t, 2, 1, 0.3, -0.31)),
                      (mesh.filter_smooth_taubin(0, device=DEV), v)):
        assert out is not mesh and _same_bits(out.vertices, want) and _same_bits(out.triangles, t) and not out.has_vertex_normals()
    assert _same_bits(mesh.vertices, v) and mesh.has_vertex_normals()
    with pytest.raises(ValueError, match="number_of_iterations"):
        mesh.filter_smooth_taubin(-1, device=DEV)


def test_get_mesh_smooths_and_simplifies_on_the_device(mesher):
    raw = TOOLS._get_mesh(mesher)
    s = 1.0
    fused = TOOLS._get_mesh(mesher, smooth_iterations=2, simplify_voxel_size=s)
    smoothed = raw.filter_smooth_taubin(2, device=DEV)
    two_step = smoothed.simplify_vertex_clustering(s, device=DEV)
    print(f"trained map at 0.4 m: {len(raw.vertices)} vertices, {len(raw.triangles)} triangles -> {len(fused.vertices)}, "
          f"{len(fused.triangles)} at {s} m")
    assert _same_bits(fused.vertices, two_step.vertices) and _same_bits(fused.triangles, two_step.triangles)
    assert 0 < len(fused.triangles) < len(raw.triangles) and not fused.has_vertex_normals()
    only_smooth = TOOLS._get_mesh(mesher, smooth_iterations=2)
    assert _same_bits(only_smooth.vertices, smoothed.vertices) and _same_bits(only_smooth.triangles, raw.triangles)
    only_simplify = TOOLS._get_mesh(mesher, simplify_voxel_size=s)
    want = raw.simplify_vertex_clustering(s, device=DEV)
    assert _same_bits(only_simplify.vertices, want.vertices) and _same_bits(only_simplify.triangles, want.triangles)
    filtered = TOOLS._get_mesh(mesher, min_component_triangles=30, smooth_iterations=0)
    raw.remove_small_components(min_triangles=30)
    assert _same_bits(filtered.vertices, raw.vertices) and _same_bits(filtered.triangles, raw.triangles)
    m, sampler = mesher
    for kw in ({"smooth_iterations": -1}, {"smooth_iterations": 1.5}, {"simplify_voxel_size": 0.0}, {"simplify_voxel_size": float("nan")}):
        with pytest.raises(ValueError, match="get_mesh"):
            m.get_mesh(DEV, sampler, skip_step=1, **kw)
