"""Mesh clean-up on the MI355X against the plain-Python restatement (tests/mesh_tools_restatement.py): cluster labels, counts, the
compaction and the vertex normals bit for bit, the cluster areas within the summation band of exactly rounded sums (and equal to the
header's stated order), and the TriangleMesh / Mesher / evaluate_mesh workflows built on them."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_restatement as MR
from tests import mesh_tools_restatement as MT
from tests import test_gpu_mesh as MESH_TESTS

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -53
TOP = 2 ** 31 - 1


def _t(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _tris(a):
    return _t(np.asarray(a, dtype=np.int32).reshape(-1, 3), np.int32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _mc_mesh():
    """the welded marching-cubes mesh of two spheres and five one-voxel blobs on a 24^3 lattice: (vertices fp64, triangles)"""
    from loner_amd import ops
    v, f = MR.marching_cubes(MT.two_spheres_volume(), 0.0, ops.mc_case_table(), spacing=(0.1, 0.1, 0.1), origin=(-1.0, 0.5, 2.0))
    return v.astype(np.float64), f


@functools.lru_cache(maxsize=None)
def _topology(name):
    """(triangles int32 [F,3], n_vertices)"""
    if name == "empty":
        return np.zeros((0, 3), dtype=np.int32), 5
    if name == "one":
        return np.array([[2, 0, 1]], dtype=np.int32), 3
    if name == "shared edge":
        return np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32), 4
    if name == "shared vertex":
        return np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32), 5
    if name == "three on one edge":
        return np.array([[0, 1, 2], [5, 6, 7], [1, 0, 3], [0, 1, 4]], dtype=np.int32), 8
    if name == "duplicate":
        return np.array([[0, 1, 2], [3, 4, 5], [0, 1, 2]], dtype=np.int32), 6
    if name == "repeated index":
        return np.array([[0, 0, 1], [2, 3, 4], [0, 0, 5], [1, 6, 7]], dtype=np.int32), 8
    if name == "strip":                                 # one chain of 100 003 links in shuffled storage order
        return MT.strip(100003)
    if name == "isolated":                              # 5 000 clusters: more than one 2 048-element scan tile
        return np.random.default_rng(1).permutation(15000).astype(np.int32).reshape(-1, 3), 15000
    if name == "marching cubes":
        v, f = _mc_mesh()
        return f, len(v)
    if name == "random":
        v, f = MT.random_shared_mesh()
        return f, len(v)
    assert name == "top indices"                        # 31-bit indices: the edge key takes all eight digit passes
    m = TOP
    return np.array([[m - 1, m - 2, m - 3], [m - 3, m - 2, m - 4], [5, 6, 7], [m - 1, 0, 1], [0, 1, 2], [7, m - 5, m - 6],
                     [m - 1, m - 3, 9]], dtype=np.int32), m


TOPOLOGIES = ["empty", "one", "shared edge", "shared vertex", "three on one edge", "duplicate", "repeated index", "strip", "isolated",
              "marching cubes", "random", "top indices"]


@functools.lru_cache(maxsize=None)
def _want_clusters(name):
    return MT.connected_triangles(_topology(name)[0])


def _gpu_clusters(tris, n_vertices):
    from loner_amd import ops
    labels, sizes = ops.mesh_connected_triangles(_tris(tris), n_vertices)
    return labels.cpu().numpy(), sizes.cpu().numpy()


# ---------------------------------------------------------------- connectivity
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_clusters_equal_the_restatement(name):
    tris, n_vertices = _topology(name)
    want_labels, want_sizes = _want_clusters(name)
    labels, sizes = _gpu_clusters(tris, n_vertices)
    print(f"{name}: {len(tris)} triangles, {len(want_sizes)} clusters, largest {want_sizes.max() if len(want_sizes) else 0}")
    assert labels.dtype == np.int32 and sizes.dtype == np.int32
    assert len(sizes) == len(want_sizes), f"{name}: C = {len(sizes)}, restated {len(want_sizes)}"
    assert _same_bits(labels, want_labels), f"{name}: {int((labels != want_labels).sum())} labels differ"
    assert _same_bits(sizes, want_sizes)


def test_fixtures_are_what_they_claim():
    assert _want_clusters("strip")[1].tolist() == [100003] and len(_want_clusters("isolated")[1]) == 5000
    sizes = np.sort(_want_clusters("marching cubes")[1])
    assert len(sizes) == 7 and sizes[:5].tolist() == [8] * 5 and sizes[5] > 200
    assert _want_clusters("top indices")[0].tolist() == [0, 0, 1, 2, 2, 3, 0]


def test_two_runs_give_the_same_clusters():
    tris, n_vertices = _topology("strip")
    a, b = _gpu_clusters(tris, n_vertices), _gpu_clusters(tris, n_vertices)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


@pytest.mark.parametrize("bad", [-1, 407, TOP])
def test_an_index_out_of_range_raises_in_every_entry(bad):
    from loner_amd import ops
    v, f = MT.random_shared_mesh()
    f = f.copy()
    f[1234, 1] = bad
    labels = _t(np.zeros(len(f)), np.int32)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_connected_triangles(_tris(f), len(v))
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_cluster_area(_t(v), _tris(f), labels, 1)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_select(_tris(f), len(v), vertex_keep=_t(np.ones(len(v)), np.uint8), drop_unreferenced=True)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_vertex_normals(_t(v), _tris(f))


def test_a_cluster_id_out_of_range_raises():
    from loner_amd import ops
    v, f = MT.random_shared_mesh()
    for bad in (-1, 3):
        labels = np.zeros(len(f), dtype=np.int32)
        labels[77] = bad
        with pytest.raises(RuntimeError, match="cluster id"):
            ops.mesh_cluster_area(_t(v), _tris(f), _t(labels, np.int32), 3)


def test_too_many_triangles_for_the_sort_are_refused():
    from loner_amd import hip
    lib = hip.load()
    limit = (2 ** 31 - 4096) // 3
    assert lib.lnr_mesh_tools_workspace(10, limit) > 0 and lib.lnr_mesh_tools_workspace(10, limit + 1) == 0
    assert lib.lnr_mesh_tools_workspace(2 ** 31, 10) == 0 and lib.lnr_mesh_tools_workspace(TOP, 10) > 0


# ---------------------------------------------------------------- cluster area
@functools.lru_cache(maxsize=None)
def _area_mesh(name):
    if name == "marching cubes":                        # spheres of 1056 and 420 triangles: two tree levels; blobs of 8
        v, f = _mc_mesh()
    elif name == "random":                              # ~2500 clusters of one to a few triangles, some of zero area
        v, f = MT.random_shared_mesh()
    elif name == "small fan":                           # 60 pairs: one sort block, the scan sums sized by the count table; one level
        v, f = MT.fan(60)
    else:
        assert name == "fan"                            # one cluster of 10 000 > 64^2 triangles: three tree levels
        v, f = MT.fan(10000)
    labels, sizes = MT.connected_triangles(f)
    return v, f, labels, sizes, MT.cluster_areas_exact(v, f, labels, len(sizes)), MT.cluster_areas_tree(v, f, labels, len(sizes))


@pytest.mark.parametrize("name", ["marching cubes", "random", "fan", "small fan"])
def test_cluster_areas_within_the_summation_band_and_in_the_stated_order(name):
    """|area_c - exact_c| <= n_c 2^-53 exact_c: the worst case of any order of summing n_c non-negative terms (exact_c: math.fsum of
    the restated triangle areas).  Beyond the band, the bits are those of the header's 64-ary order, and of a second run."""
    from loner_amd import ops
    v, f, labels, sizes, exact, tree = _area_mesh(name)
    run = lambda: ops.mesh_cluster_area(_t(v), _tris(f), _t(labels, np.int32), len(sizes)).cpu().numpy()
    got, again = run(), run()
    err = np.abs(got - exact)
    print(f"{name}: {len(sizes)} clusters, largest {sizes.max()}; max |error| / (n_c u exact) = "
          f"{(err[exact > 0] / (sizes * U * exact)[exact > 0]).max():.3g}")
    assert got.dtype == np.float64 and got.shape == exact.shape and (exact > 0).sum() > 0.9 * len(exact)
    assert (err <= sizes * U * exact).all()
    assert _same_bits(got, again)
    assert _same_bits(got, tree), f"{int((got != tree).sum())} clusters differ from the stated order"


def test_cluster_area_of_a_labelling_that_is_not_connectivity():
    """any labelling in [0, C): interleaved labels, one cluster without a triangle"""
    from loner_amd import ops
    v, f = MT.random_shared_mesh()
    labels = (np.arange(len(f)) % 5).astype(np.int32)
    labels[labels == 3] = 1
    got = ops.mesh_cluster_area(_t(v), _tris(f), _t(labels, np.int32), 5).cpu().numpy()
    assert _same_bits(got, MT.cluster_areas_tree(v, f, labels, 5)) and got[3] == 0.0
    assert ops.mesh_cluster_area(_t(v), _tris(f[:0]), _t(labels[:0], np.int32), 0).shape == (0,)


# ---------------------------------------------------------------- select
def _select_case(name):
    rng = np.random.default_rng(9)
    if name == "random":
        f, n = _topology("random")
    elif name == "isolated":                            # 15 000 vertices and 5 000 triangles: several scan tiles each
        f, n = _topology("isolated")
    else:
        f, n = _topology("marching cubes")
    return f, n, rng.random(len(f)) < 0.7, rng.random(n) < 0.9


@pytest.mark.parametrize("name", ["random", "isolated", "marching cubes"])
@pytest.mark.parametrize("use", ["triangles", "vertices", "both", "both, drop unreferenced", "drop unreferenced", "nothing"])
def test_select_equals_the_restatement(name, use):
    from loner_amd import ops
    f, n, tk, vk = _select_case(name)
    tk = tk if use in ("triangles", "both", "both, drop unreferenced") else None
    vk = vk if use in ("vertices", "both", "both, drop unreferenced") else None
    drop = "drop" in use
    want_f, want_map, want_n = MT.select(f, n, tk, vk, drop)
    got_f, got_map, got_n = ops.mesh_select(_tris(f), n, None if tk is None else _t(tk, np.bool_), None if vk is None else _t(vk, np.uint8),
                                            drop)
    assert got_n == want_n and _same_bits(got_map.cpu().numpy(), want_map)
    assert _same_bits(got_f.cpu().numpy(), want_f)
    if use == "nothing":
        assert want_n == n and np.array_equal(want_f, f)


def test_select_on_empty_inputs():
    from loner_amd import ops
    out, vmap, n = ops.mesh_select(_tris(np.zeros((0, 3))), 4, drop_unreferenced=True)
    assert out.shape == (0, 3) and vmap.cpu().tolist() == [-1] * 4 and n == 0
    out, vmap, n = ops.mesh_select(_tris(np.zeros((0, 3))), 0)
    assert out.shape == (0, 3) and vmap.shape == (0,) and n == 0
    out, vmap, n = ops.mesh_select(_tris([[0, 1, 2]]), 3, triangle_keep=_t([0], np.uint8))
    assert out.shape == (0, 3) and vmap.cpu().tolist() == [0, 1, 2] and n == 3


# ---------------------------------------------------------------- vertex normals
@pytest.mark.parametrize("name", ["random", "marching cubes", "fan", "small fan"])
def test_vertex_normals_are_the_bytes_of_the_numpy_route(name):
    from loner_amd import ops
    from loner_amd.analysis.mesher import TriangleMesh
    v, f = {"random": MT.random_shared_mesh, "marching cubes": _mc_mesh, "fan": lambda: MT.fan(10000),
            "small fan": lambda: MT.fan(60)}[name]()                # 180 pairs: one sort block
    want = TriangleMesh(v, f).compute_vertex_normals().vertex_normals
    got = ops.mesh_vertex_normals(_t(v), _tris(f)).cpu().numpy()
    differ = (got.view(np.uint64) != want.view(np.uint64)).any(1)
    assert _same_bits(got, want), f"{name}: {int(differ.sum())} of {len(v)} normals differ, first at vertex {int(np.argmax(differ))}"
    if name == "random":
        assert _same_bits(got, MT.vertex_normals(v, f)) and not got[-7:].any() and np.abs(np.linalg.norm(got[:-7], axis=1) - 1).max() < 1e-12
    assert _same_bits(TriangleMesh(v, f).compute_vertex_normals(device=DEV).vertex_normals, want)


def test_vertex_normals_without_triangles_are_zeros():
    from loner_amd import ops
    v = np.random.default_rng(0).normal(size=(5, 3))
    assert not ops.mesh_vertex_normals(_t(v), _tris(np.zeros((0, 3)))).cpu().numpy().any()
    assert ops.mesh_vertex_normals(_t(v[:0]), _tris(np.zeros((0, 3)))).shape == (0, 3)


# ---------------------------------------------------------------- workflows
def _mc_triangle_mesh(normals=True):
    from loner_amd.analysis.mesher import TriangleMesh
    v, f = _mc_mesh()
    mesh = TriangleMesh(v, f)
    return mesh.compute_vertex_normals() if normals else mesh


def test_cluster_connected_triangles_returns_open3d_s_triple():
    labels, sizes, area = _mc_triangle_mesh().cluster_connected_triangles()
    v, f, want_labels, want_sizes, _, tree = _area_mesh("marching cubes")
    assert _same_bits(labels, want_labels) and _same_bits(sizes, want_sizes) and _same_bits(area, tree)


@pytest.mark.parametrize("kw", [dict(min_triangles=9), dict(keep_largest=2), dict(min_area=0.05), dict(keep_largest=1),
                                dict(min_triangles=8, keep_largest=3)])
def test_remove_small_components_leaves_the_restated_clusters(kw):
    v, f, labels, sizes, exact, tree = _area_mesh("marching cubes")
    keep = MT.small_component_keep(sizes, tree, **kw)
    want_v, want_n, want_f = MT.apply_select(v, _mc_triangle_mesh().vertex_normals, f, triangle_keep=keep[labels], drop_unreferenced=True)
    mesh = _mc_triangle_mesh()
    removed = mesh.remove_small_components(**kw)
    assert removed == len(f) - len(want_f) and 0 < removed < len(f)
    assert _same_bits(mesh.triangles, want_f) and _same_bits(mesh.vertices, want_v) and _same_bits(mesh.vertex_normals, want_n)
    left = np.sort(mesh.cluster_connected_triangles()[1])
    assert left.tolist() == np.sort(sizes[keep]).tolist()
    if kw in (dict(min_triangles=9), dict(keep_largest=2)):         # exactly the two spheres
        assert left.tolist() == np.sort(sizes)[-2:].tolist() and left[0] > 200


def test_the_remove_methods_and_crop_equal_the_restatement_with_normals_carried():
    from loner_amd.analysis.mesher import TriangleMesh
    v, f = _mc_mesh()
    normals = _mc_triangle_mesh().vertex_normals
    rng = np.random.default_rng(4)
    tmask, vmask = rng.random(len(f)) < 0.3, rng.random(len(v)) < 0.1

    def check(mesh, want, had_normals=True):
        assert _same_bits(mesh.vertices, want[0]) and _same_bits(mesh.triangles, want[2])
        assert _same_bits(mesh.vertex_normals, want[1]) if had_normals else mesh.vertex_normals.shape == (0, 3)

    mesh = _mc_triangle_mesh()
    assert mesh.remove_triangles_by_mask(tmask) is mesh
    check(mesh, MT.apply_select(v, normals, f, triangle_keep=~tmask))
    assert len(mesh.vertices) == len(v) and len(mesh.triangles) == int((~tmask).sum())
    assert mesh.remove_unreferenced_vertices() is mesh
    check(mesh, MT.apply_select(v, normals, f, triangle_keep=~tmask, drop_unreferenced=True))
    mesh = _mc_triangle_mesh(normals=False)
    assert mesh.remove_vertices_by_mask(vmask) is mesh
    check(mesh, MT.apply_select(v, None, f, vertex_keep=~vmask), had_normals=False)
    assert len(mesh.vertices) == int((~vmask).sum())
    fd = f.copy()
    fd[::5, 2] = fd[::5, 0]
    mesh = TriangleMesh(v, fd)
    mesh.vertex_normals = normals.copy()
    assert mesh.remove_degenerate_triangles() is mesh
    check(mesh, MT.apply_select(v, normals, fd, triangle_keep=np.arange(len(fd)) % 5 != 0))
    lo, hi = np.array([-0.6, 0.9, 2.4]), np.array([0.35, 2.0, 3.3])
    lo[0] = v[100, 0]                                    # a vertex exactly on the face of the closed box stays
    source = _mc_triangle_mesh()
    cropped = source.crop(lo, hi)
    inside = ((v >= lo) & (v <= hi)).all(1)
    check(cropped, MT.apply_select(v, normals, f, vertex_keep=inside))
    assert 0 < len(cropped.triangles) < len(f) and len(cropped.vertices) == int(inside.sum())
    assert cropped is not source and _same_bits(source.vertices, v) and _same_bits(source.triangles, f)


def test_evaluate_mesh_can_drop_floaters_first(tmp_path):
    """a box and one detached triangle far from it: unfiltered, the floater's samples cost precision; with min_component_triangles = 2
    the score is the box's own, and the caller's mesh is left alone"""
    from loner_amd.analysis.mesh_eval import evaluate_mesh
    from loner_amd.analysis.mesher import TriangleMesh
    lo, hi = np.array([-2.0, -1.5, 0.0]), np.array([2.0, 1.5, 2.0])
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.array([[a, b, c] for a, b, c, d in faces] + [[a, c, d] for a, b, c, d in faces], dtype=np.int32)
    box = TriangleMesh(corners, tris)
    gt = box.sample_points_uniformly(100_000, seed=1)
    dirty = TriangleMesh(np.concatenate([corners, [[9.0, 9.0, 9.0], [12.0, 9.0, 9.0], [9.0, 12.0, 9.0]]]),
                         np.concatenate([tris, [[8, 9, 10]]]).astype(np.int32))
    kw = dict(f_score_threshold=0.1, voxel_size=0.05, number_of_points=100_000, seed=2)
    raw = evaluate_mesh(dirty, gt, str(tmp_path), **kw)
    clean = evaluate_mesh(dirty, gt, str(tmp_path), min_component_triangles=2, **kw)
    assert raw["precision"] < 0.99 and clean["precision"] == 1.0
    assert dirty.triangles.shape == (13, 3) and dirty.vertices.shape == (11, 3)


@pytest.fixture(scope="module")
def mesher():
    """the trained synthetic map of tests/test_gpu_mesh.py (one keyframe, 150 iterations) behind a Mesher at 0.4 m"""
    from loner_amd.analysis.mesher import Mesher
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
    from tests.test_gpu_mapping import make_keyframes
    s = default_optimizer_settings()
    s["num_samples"]["sky"] = 0
    torch.manual_seed(0)
    wc = MESH_TESTS._world_cube()
    opt = Optimizer(s, None, wc, 0, False, True, False)
    kf = make_keyframes([SY.trajectory_pose6(1)[0]])[0]
    opt._do_iterate_optimizer([kf], [None], optimizer_settings=OptimizationSettings(150, True, False, False, True))
    mcb = [[-21.0, 21.0], [-16.0, 16.0], [-3.0, 7.0]]
    return Mesher(opt._model, {"poses": [kf.get_pose_state()]}, wc, torch.tensor([1.0, 50.0]), resolution=0.4, marching_cubes_bound=mcb,
                  level_set=0), opt._ray_sampler


def _get_mesh(mesher, **kw):
    m, sampler = mesher
    torch.manual_seed(3)
    return m.get_mesh(DEV, sampler, skip_step=1, **kw)


def test_get_mesh_without_the_argument_is_the_unfiltered_pipeline(mesher):
    """get_mesh() is what it was: the volume, marching cubes, and the float64 conversion to metres, byte for byte"""
    from loner_amd import ops
    m, sampler = mesher
    mesh = _get_mesh(mesher)
    torch.manual_seed(3)
    with torch.no_grad():
        volume, xyz = m.get_volume(DEV, sampler, 1, None)
    verts, faces = ops.marching_cubes(volume, 0.0, spacing=(xyz[0][2] - xyz[0][1], xyz[1][2] - xyz[1][1], xyz[2][2] - xyz[2][1]))
    vertices = verts.cpu().numpy() + np.array([xyz[0][0], xyz[1][0], xyz[2][0]])
    vertices *= m.world_cube_scale_factor
    vertices -= m.world_cube_shift
    assert mesh.triangles.shape[0] > 1000
    assert _same_bits(mesh.vertices, np.ascontiguousarray(vertices, dtype=np.float64)) and _same_bits(mesh.triangles, faces.cpu().numpy())
    assert mesh.vertex_normals.shape == (0, 3)


def test_get_mesh_filters_small_components_on_the_device(mesher):
    raw = _get_mesh(mesher)
    sizes = raw.cluster_connected_triangles()[1]
    k = 30
    print(f"trained map at 0.4 m: {raw.triangles.shape[0]} triangles in {len(sizes)} clusters, largest {sizes.max()}, "
          f"{int((sizes < k).sum())} clusters with {int(sizes[sizes < k].sum())} triangles below {k}")
    filtered = _get_mesh(mesher, min_component_triangles=k)
    removed = raw.remove_small_components(min_triangles=k)
    assert removed == int(sizes[sizes < k].sum()) and removed > 0     # the trained map has floaters: the filter has work to do
    assert _same_bits(filtered.vertices, raw.vertices) and _same_bits(filtered.triangles, raw.triangles)
    assert filtered.cluster_connected_triangles()[1].min() >= k
