"""Point-to-mesh queries on the MI355X against the numpy restatement (tests/mesh_distance_restatement.py): squared distances, ids,
points, uvs and crossing counts bit for bit on a soup with every degenerate the contract names, at every small size, on trees that
tie and trees tens of levels deep, far from the origin, with a reach; then the closed forms of closed meshes (occupancy and signed
distance of the box room, the icosphere within its sagitta) and evaluate_mesh_to_mesh on two parallel patches."""
import functools
import math

import numpy as np
import pytest
import torch

from loner_amd.utils import synthetic as SYN
from loner_amd.utils import synthetic_mesh as SM
from tests import mesh_distance_restatement as MR

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEYS = ("primitive_ids", "dist_sq", "points", "primitive_uvs")


def _t(a, dtype=np.float64):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)       # a copy: some inputs are read-only


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _bvh(v, f):
    from loner_amd import ops
    return ops.BVH(_t(v), _t(f, np.int32))


def _gpu_closest(v, f, points, max_distance=math.inf, bvh=None):
    from loner_amd import ops
    bvh = _bvh(v, f) if bvh is None else bvh
    stats = {}
    d2, ids, q, uvs = ops.closest_points(bvh, _t(points).reshape(-1, 3), max_distance, stats=stats)
    return dict(dist_sq=d2.cpu().numpy(), primitive_ids=ids.cpu().numpy(), points=q.cpu().numpy(), primitive_uvs=uvs.cpu().numpy(),
                stats=stats, bvh=bvh)


def _assert_equal(got, want, what=""):
    for key in KEYS:
        if not _same_bits(got[key], want[key]):
            if got[key].shape != want[key].shape:
                raise AssertionError(f"{what}: {key} has shape {got[key].shape}, want {want[key].shape}")
            bits = np.int64 if want[key].dtype == np.float64 else np.int32
            width = int(np.prod(want[key].shape[1:]))
            g, w = (np.ascontiguousarray(x).view(bits).reshape(len(x), width) for x in (got[key], want[key]))
            bad = np.nonzero((g != w).any(axis=1))[0]
            raise AssertionError(f"{what}: {key} differs on {len(bad)} queries, first {bad[:5]}: got {got[key][bad[:5]]}, want "
                                 f"{want[key][bad[:5]]}")
    s = got["stats"]
    assert s["answered"] == int((want["primitive_ids"] >= 0).sum()), what
    assert s["invalid_points"] == want["invalid_points"] and s["capped"] == 0, what
    assert s["excluded_triangles"] == want["excluded_triangles"], what


# ---------------------------------------------------------------- the soup
@functools.lru_cache(maxsize=None)
def _soup():
    """300 triangles in a 10 m box: 240 random; 20 copies of earlier ones (coincident centres); 10 collapsed to a point (5 with one
    index three times, 5 with three vertices at one place); 20 needles on dyadic coordinates (10 with two corners at one place, 10
    with the third corner the exact midpoint of the other two); 5 thin but proper ones (height a 50th of the base); 5 with a NaN or
    inf vertex -> (vertices, triangles)"""
    rng = np.random.default_rng(21)
    n0 = 240
    centre = rng.uniform(0.0, 10.0, (n0, 1, 3))
    v = [(centre + rng.uniform(-0.8, 0.8, (n0, 3, 3))).reshape(-1, 3)]
    f = [np.arange(3 * n0).reshape(n0, 3)]
    f.append(f[0][rng.choice(n0, 20, replace=False)])
    f.append(np.repeat(rng.integers(0, 3 * n0, 5), 3).reshape(5, 3))
    count = 3 * n0

    def add(corners):                                                        # [k,3,3] -> k triangles on new vertices
        nonlocal count
        k = len(corners)
        v.append(corners.reshape(-1, 3))
        f.append(count + np.arange(3 * k).reshape(k, 3))
        count += 3 * k

    dyadic = lambda k: np.round(rng.uniform(0.0, 10.0, (k, 3)) * 1024) / 1024        # noqa: E731
    a = dyadic(5)
    add(np.stack([a, a, a], axis=1))
    a, b = dyadic(20), dyadic(20)
    add(np.stack([a, b, np.concatenate([b[:10], 0.5 * (a[10:] + b[10:])])], axis=1))
    a, e = rng.uniform(2.0, 8.0, (5, 3)), rng.normal(size=(5, 3))
    side = np.cross(e, rng.normal(size=(5, 3)))
    side *= (np.linalg.norm(e, axis=1) / 50 / np.linalg.norm(side, axis=1))[:, None]
    add(np.stack([a, a + e, a + 0.4 * e + side], axis=1))
    bad = rng.uniform(0.0, 10.0, (5, 3, 3))
    bad[:4, 1, 2] = np.nan
    bad[4, 0, 0] = np.inf
    add(bad)
    v, f = np.concatenate(v), np.concatenate(f).astype(np.int32)
    assert f.shape == (300, 3)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def _soup_points(v, f, rng, scale=1.0):
    """2048 queries: 1200 random in and around the box; 200 exactly at vertices, 200 on edges, 200 at centroids; 200 about 1e6 away;
    48 with a NaN or inf coordinate"""
    usable = np.nonzero(np.isfinite(v[f]).all(axis=(1, 2)))[0]
    tri = lambda n: v[f[rng.choice(usable, n)]]                              # noqa: E731  [n,3,3]
    lo, hi = np.nanmin(v[np.isfinite(v).all(axis=1)], axis=0), np.nanmax(v[np.isfinite(v).all(axis=1)], axis=0)
    parts = [rng.uniform(lo - scale, hi + scale, (1200, 3)), tri(200)[:, 1]]
    T, s = tri(200), rng.uniform(0, 1, (200, 1))
    parts.append(T[:, 0] + s * (T[:, 2] - T[:, 0]))
    parts.append(tri(200).mean(axis=1))
    far = rng.normal(size=(200, 3))
    parts.append(0.5 * (lo + hi) + 1e6 * far / np.linalg.norm(far, axis=1, keepdims=True))
    bad = rng.uniform(lo, hi, (48, 3))
    bad[np.arange(48), rng.integers(0, 3, 48)] = np.tile([np.nan, np.inf, -np.inf], 16)
    parts.append(bad)
    p = np.concatenate(parts)
    assert p.shape == (2048, 3)
    return p


@functools.lru_cache(maxsize=None)
def _soup_case():
    v, f = _soup()
    p = _soup_points(v, f, np.random.default_rng(22))
    p.setflags(write=False)
    return p, MR.closest_points(v, f, p)


def test_soup_bit_for_bit_with_every_degenerate():
    v, f = _soup()
    p, want = _soup_case()
    ids = want["primitive_ids"]
    assert want["excluded_triangles"] == 5 and want["invalid_points"] == 48 and (ids[:2000] >= 0).all() and (ids[2000:] == -1).all()
    assert (want["dist_sq"][1200:1800] < 1e-20).all() and (want["dist_sq"][1800:2000] > 0.99e12).all()
    assert not (ids >= 295).any() and ((ids >= 260) & (ids < 295)).any()     # the degenerates answer too; the NaN ones never
    got = _gpu_closest(v, f, p)
    _assert_equal(got, want, "soup")
    assert got["bvh"].n_in_tree == 295 and got["bvh"].n_nonfinite == 5
    print(f"soup: depth {got['stats']['depth']}, {got['stats']['node_visits'] / len(p):.1f} node visits per query")


def test_two_runs_give_identical_bytes_and_nullable_outputs():
    from loner_amd import ops
    v, f = _soup()
    p, _ = _soup_case()
    a, b = _gpu_closest(v, f, p), _gpu_closest(v, f, p)
    for key in KEYS:
        assert _same_bits(a[key], b[key]), key
    assert a["stats"] == b["stats"]
    d2, ids, q, uvs = ops.closest_points(a["bvh"], _t(p), want_points=False, want_uvs=False)
    assert q is None and uvs is None and _same_bits(d2.cpu().numpy(), a["dist_sq"]) and _same_bits(ids.cpu().numpy(), a["primitive_ids"])
    rays = np.concatenate([p, np.random.default_rng(1).normal(size=p.shape)], axis=1)
    c = [ops.count_intersections(a["bvh"], _t(rays)).cpu().numpy() for _ in range(2)]
    assert _same_bits(c[0], c[1])


def test_index_out_of_range_sets_the_status_and_every_query_misses():
    """ops.BVH refuses such a mesh, so the entries are called on the built buffer directly"""
    from loner_amd import hip, ops
    from loner_amd.hip import _ptr, _stream
    v, f = _soup()
    g = f[:100].copy()
    g[37, 1] = len(v)
    with pytest.raises(RuntimeError, match="index"):
        ops.BVH(_t(v), _t(g, np.int32))
    lib = hip.load()
    vt, gt = _t(v), _t(g, np.int32)
    need, nbytes = int(lib.lnr_bvh_workspace(100)), int(lib.lnr_bvh_bytes(100))
    ws, buf = torch.empty(need, device=DEV, dtype=torch.uint8), torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    info = torch.empty(8, device=DEV, dtype=torch.int64)
    hip.check(lib.lnr_bvh_build(_ptr(vt), vt.shape[0], _ptr(gt), 100, _ptr(ws), need, _ptr(buf), nbytes, _ptr(info), _stream()))
    assert int(info.cpu()[0]) == 1
    p = _t(_soup_case()[0][:130])
    d2, ids = torch.empty(130, device=DEV, dtype=torch.float64), torch.empty(130, device=DEV, dtype=torch.int32)
    q, uv = torch.ones(130, 3, device=DEV, dtype=torch.float64), torch.ones(130, 2, device=DEV, dtype=torch.float64)
    hip.check(lib.lnr_closest_points(_ptr(buf), 100, _ptr(p), 130, math.inf, _ptr(d2), _ptr(ids), _ptr(q), _ptr(uv), _ptr(info), _stream()))
    host = info.cpu()
    assert int(host[0]) == 1 and int(host[1]) == 0 and int(host[5]) == 1
    assert bool(torch.isinf(d2).all()) and bool((ids == -1).all()) and bool((q == 0).all()) and bool((uv == 0).all())
    rays = torch.cat([p, torch.ones_like(p)], dim=1).contiguous()
    counts = torch.ones(130, device=DEV, dtype=torch.int32)
    hip.check(lib.lnr_count_intersections(_ptr(buf), 100, _ptr(rays), 130, 0.0, math.inf, _ptr(counts), _ptr(info), _stream()))
    assert int(info.cpu()[0]) == 1 and bool((counts == 0).all())


@pytest.mark.parametrize("n_tris", [0, 1, 2, 3, 65])
def test_small_meshes_and_query_counts(n_tris):
    v, f = _soup()
    f = f[:n_tris]
    p, _ = _soup_case()
    p = p[np.r_[0:50, 1200:1215]]                                            # random ones and some at vertices
    want = MR.closest_points(v, f, p)
    rays = np.concatenate([p, np.random.default_rng(n_tris).normal(size=p.shape)], axis=1)
    want_counts = MR.count_intersections(v, f, rays)
    bvh = _bvh(v, f)
    from loner_amd import ops
    for n in (0, 1, 63, 64, 65):
        got = _gpu_closest(v, f, p[:n], bvh=bvh)
        part = {k: (x[:n] if isinstance(x, np.ndarray) else x) for k, x in want.items()}
        _assert_equal(got, part, f"F = {n_tris}, n = {n}")
        stats = {}
        counts = ops.count_intersections(bvh, _t(rays[:n]).reshape(-1, 6), stats=stats).cpu().numpy()
        assert _same_bits(counts, want_counts["counts"][:n]), (n_tris, n)
        assert stats["rays_crossing"] == int((want_counts["counts"][:n] > 0).sum()) and stats["invalid_rays"] == 0
    assert bvh.n_in_tree == n_tris


# ---------------------------------------------------------------- ties and depth
def _around(v, f, rng, n_random=150):
    """queries above every triangle's centre, at it, and random ones around the mesh"""
    c = v[f].mean(axis=1)
    lo, hi = v.min(0) - 1.0, v.max(0) + 1.0
    return np.concatenate([c + np.array([0.013, -0.007, 0.5]), c, rng.uniform(lo, hi, (n_random, 3))])


def test_equal_codes_shared_centres_and_deep_trees():
    rng = np.random.default_rng(5)
    tri = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.2]])
    # 512 copies of one triangle: every code is equal, every distance ties, the answer is triangle 0
    v, f = tri, np.tile(np.arange(3), (512, 1))
    p = _around(v, f[:1], rng)
    want = MR.closest_points(v, f, p)
    assert (want["primitive_ids"] == 0).all()
    got = _gpu_closest(v, f, p)
    _assert_equal(got, want, "512 copies")
    assert got["stats"]["depth"] == 9
    # concentric squares in one plane around one centre: one box centre, one code; above the middle all 128 triangles tie at one distance
    ring = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
    v = np.concatenate([ring * s for s in np.arange(64, 0, -1)]) + np.array([3.0, 4.0, 1.0])
    f = np.concatenate([[[4 * k, 4 * k + 1, 4 * k + 2], [4 * k, 4 * k + 2, 4 * k + 3]] for k in range(64)])
    p = np.concatenate([_around(v, f, rng), [[3.25, 4.125, 5.0], [3.0, 4.0, -2.0]]])
    want = MR.closest_points(v, f, p)
    assert want["primitive_ids"][-2] == 0 and want["dist_sq"][-2] == 16.0 and want["primitive_ids"][-1] == 0
    _assert_equal(_gpu_closest(v, f, p), want, "concentric")
    # clusters of 8 small triangles at x = 2^-k: the codes share ever longer prefixes and the tree is tens of levels deep
    vs, fs = [], []
    for k in range(21):
        x, size = 2.0 ** -k, 2.0 ** -(k + 3)
        for j in range(8):
            q = np.array([x, 0.0, 0.0]) + size * np.array([0.1 * j, 0.05 * j, 0.02 * j])
            fs.append(len(vs) + np.arange(3))
            vs += [q, q + size * np.array([0.5, 0.0, 0.1]), q + size * np.array([0.0, 0.5, 0.0])]
    v, f = np.asarray(vs), np.asarray(fs)
    p = _around(v, f, rng)
    want = MR.closest_points(v, f, p)
    got = _gpu_closest(v, f, p)
    _assert_equal(got, want, "clusters at 2^-k")
    print(f"clusters: depth {got['stats']['depth']}")
    assert 20 <= got["stats"]["depth"]


def test_far_from_the_origin_with_queries_a_nanometre_off_the_surface():
    """the soup moved by 1e4 on every axis: an ulp of a coordinate is 2e-12, the relative pad of a 1e-9 gap is nothing, and the
    computed closest point can lie outside its box by more than the gap; the absolute part of the pad keeps those boxes"""
    v, f = _soup()
    v = v + 1e4
    rng = np.random.default_rng(23)
    usable = np.arange(260)                                                  # proper triangles and copies: they have a normal
    T = v[f[rng.choice(usable, 1500)]]
    w = rng.dirichlet((1, 1, 1), 1500)
    w[:300] = np.eye(3)[rng.integers(0, 3, 300)]                             # at corners
    w[300:600, 0] = 0.0                                                      # on the edge BC
    w[300:600] /= w[300:600].sum(axis=1, keepdims=True)
    on = np.einsum("nk,nka->na", w, T)
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    p = np.concatenate([on + 1e-9 * n * rng.choice([-1.0, 1.0], (1500, 1)), _soup_points(v, f, rng)[:548]])
    want = MR.closest_points(v, f, p)
    assert (want["dist_sq"][:1500] < 1e-16).all()
    _assert_equal(_gpu_closest(v, f, p), want, "offset")


def test_reach():
    v = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1], [0, 0, 3], [4, 0, 3], [0, 4, 3]], dtype=np.float64)
    f = np.array([[3, 4, 5], [0, 1, 2]])
    p = np.array([[1.0, 1.0, 0.25], [1.0, 1.0, 1.5], [1.0, 1.0, 2.5], [1.0, 1.0, 6.0], [9.0, 9.0, 2.0]])
    bvh = _bvh(v, f)
    for reach in (math.inf, 0.75, np.nextafter(0.75, 0.0), 0.5, 0.0, 3.0):
        want = MR.closest_points(v, f, p, reach * reach)
        _assert_equal(_gpu_closest(v, f, p, reach, bvh=bvh), want, f"reach {reach}")
    at = _gpu_closest(v, f, p[:1], 0.75, bvh=bvh)                            # exactly at the reach: 0.75^2 = 0.5625, both exact
    assert at["primitive_ids"][0] == 1 and at["dist_sq"][0] == 0.5625
    below = _gpu_closest(v, f, p[:1], np.nextafter(0.75, 0.0), bvh=bvh)
    assert below["primitive_ids"][0] == -1 and np.isinf(below["dist_sq"][0]) and (below["points"] == 0).all()
    half = _gpu_closest(v, f, p, 0.5, bvh=bvh)
    assert list(half["primitive_ids"]) == [-1, 1, 0, -1, -1]                 # queries on both sides of the reach


def test_counts_bit_for_bit_with_a_window():
    from loner_amd import ops
    v, f = _soup()
    p, _ = _soup_case()
    rng = np.random.default_rng(24)
    rays = np.concatenate([p[:1500], rng.normal(size=(1500, 3))], axis=1)
    rays[1200:1500, 3:] = v[f[rng.integers(0, 240, 300)]][:, 2] - rays[1200:1500, :3]       # from a vertex at another triangle's corner
    rays[100:110, 3:] = 0.0
    rays[110:120, 4] = np.nan
    bvh = _bvh(v, f)
    most = 0
    for t_min, t_max in ((0.0, math.inf), (0.5, 3.0), (-math.inf, math.inf), (1.0, 1.0)):
        want = MR.count_intersections(v, f, rays, t_min, t_max)
        most = max(most, int(want["counts"].max()))
        stats = {}
        got = ops.count_intersections(bvh, _t(rays), t_min, t_max, stats=stats).cpu().numpy()
        assert got.dtype == np.int32 and _same_bits(got, want["counts"]), (t_min, t_max, int((got != want["counts"]).sum()))
        assert stats["invalid_rays"] == want["invalid_rays"] == 20 and stats["rays_crossing"] == int((want["counts"] > 0).sum())
        assert stats["excluded_triangles"] == 5 and stats["capped"] == 0
    assert most >= 3


# ---------------------------------------------------------------- closed meshes
def test_box_room_occupancy_and_signed_distance():
    from loner_amd.analysis.raycast import RaycastingScene
    scene = RaycastingScene(*SM.box_room_mesh(), device=DEV)
    lo, hi = np.asarray(SYN.BOX_MIN), np.asarray(SYN.BOX_MAX)
    rng = np.random.default_rng(7)
    inside = rng.uniform(lo + 0.01, hi - 0.01, (3000, 3)).reshape(30, 100, 3)
    shift = rng.choice([-1.0, 1.0], (3000, 1)) * (hi - lo) * np.eye(3)[rng.integers(0, 3, 3000)]
    outside = inside.reshape(-1, 3) + shift
    for nsamples in (1, 3):
        occ = scene.compute_occupancy(inside, nsamples)
        assert tuple(occ.shape) == (30, 100) and occ.dtype == torch.float64 and bool((occ == 1.0).all())
        assert bool((scene.compute_occupancy(outside, nsamples) == 0.0).all())
    want = np.minimum(inside - lo, hi - inside).min(axis=-1)
    sd = scene.compute_signed_distance(inside).cpu().numpy()
    print(f"box room: max |signed distance + wall distance| {np.abs(sd + want).max():.3e}")
    assert np.abs(sd + want).max() <= 1e-12
    assert bool((scene.compute_signed_distance(outside) > 0).all())
    counts = scene.count_intersections(np.concatenate([inside, np.ones_like(inside)], axis=-1))
    assert tuple(counts.shape) == (30, 100) and counts.dtype == torch.int32 and bool((counts == 1).all())
    near = scene.compute_closest_points(inside)
    assert set(near) == {"points", "primitive_ids", "primitive_uvs", "primitive_normals", "distance"}
    assert tuple(near["points"].shape) == (30, 100, 3) and np.abs(near["distance"].cpu().numpy() - want).max() <= 1e-12
    step = torch.from_numpy(inside).to(DEV) - near["points"]
    along = (step * near["primitive_normals"]).sum(-1).abs()                 # the step to a wall runs along the wall's normal
    assert float((along - near["distance"]).abs().max()) <= 1e-12
    miss = scene.compute_closest_points(inside[0], max_distance=1e-3)
    assert bool((miss["primitive_ids"] == -1).all()) and bool(torch.isinf(miss["distance"]).all())
    assert bool((miss["primitive_normals"] == 0).all()) and bool((miss["points"] == 0).all())


def test_icosphere_distance_within_its_sagitta():
    """the mesh lies between the sphere and the sphere shrunk by the sagitta (the largest depth of a triangle's plane below the
    sphere, attained above its circumcentre or beyond it): r - s <= |x - c| <= r for every surface point x, so the distance from p
    to the mesh differs from ||p - c| - r| by at most s"""
    from loner_amd.analysis.mesh_eval import cloud_to_mesh_distance
    from loner_amd.analysis.raycast import RaycastingScene
    r, c = 3.0, np.asarray(SYN.SPHERE_C)
    v, f = SM.icosphere(2, r, c)
    a, b, cc = (v[f[:, k]] - c for k in range(3))
    n = np.cross(b - a, cc - a)
    sagitta = r - (np.einsum("na,na->n", n, a) / np.linalg.norm(n, axis=1)).min()
    assert 0.0 < sagitta < 0.02 * r
    rng = np.random.default_rng(8)
    u = rng.normal(size=(4000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = rng.uniform(0.0, 3 * r, 4000)
    p = c + rad[:, None] * u
    scene = RaycastingScene(v, f, device=DEV)
    d = cloud_to_mesh_distance(torch.from_numpy(p).to(DEV), scene).cpu().numpy()
    err = np.abs(d - np.abs(rad - r))
    print(f"icosphere: sagitta {sagitta:.4f}, max difference {err.max():.4f}")
    assert err.max() <= sagitta + 1e-12
    sd = scene.compute_signed_distance(p).cpu().numpy()
    clear = np.abs(rad - r) > sagitta
    assert (np.sign(sd[clear]) == np.sign(rad[clear] - r)).all()


def test_evaluate_mesh_to_mesh_on_parallel_patches():
    from loner_amd.analysis.mesh_eval import evaluate_mesh_to_mesh
    from loner_amd.analysis.mesher import TriangleMesh
    from loner_amd.analysis.raycast import RaycastingScene
    delta = 0.25                                                             # exact in fp64, as are the coordinates below

    def patch(lo, hi, z, cells):
        g = np.linspace(lo, hi, cells + 1)
        v = np.stack([np.repeat(g, cells + 1), np.tile(g, cells + 1), np.full((cells + 1) ** 2, z)], axis=1)
        quad = np.array([[i * (cells + 1) + j, (i + 1) * (cells + 1) + j, (i + 1) * (cells + 1) + j + 1, i * (cells + 1) + j + 1]
                         for i in range(cells) for j in range(cells)])
        return TriangleMesh(v, np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]]))

    est, gt = patch(2.0, 6.0, 1.0, 4), patch(0.0, 8.0, 1.0 + delta, 8)
    got = evaluate_mesh_to_mesh(est, gt, f_score_threshold=0.3, number_of_points=5000, device=DEV)
    print(f"patches: {got}")
    assert set(got) == {"accuracy", "completion", "chamfer", "precision", "recall", "f_score", "n_est", "n_gt"}
    assert got["n_est"] == got["n_gt"] == 5000
    assert abs(got["accuracy"] - delta) <= 1e-12                             # every sample of the estimate lies delta below the larger patch
    assert got["completion"] > delta and abs(got["chamfer"] - (got["accuracy"] + got["completion"])) <= 1e-15
    assert got["precision"] == 1.0 and 0.0 < got["recall"] < 1.0             # the ground truth reaches beyond the estimate
    assert abs(got["f_score"] - 2 * got["recall"] / (1 + got["recall"])) <= 1e-15
    below = evaluate_mesh_to_mesh(est, gt, f_score_threshold=0.2, number_of_points=5000, device=DEV)
    assert below["precision"] == 0.0 and below["recall"] == 0.0 and below["f_score"] == 0.0
    scene = RaycastingScene(gt, device=DEV)                                  # a ready scene is taken as it is
    same = evaluate_mesh_to_mesh(scene, scene, number_of_points=5000)
    assert same["accuracy"] <= 1e-12 and same["completion"] <= 1e-12 and same["precision"] == same["recall"] == 1.0
    again = evaluate_mesh_to_mesh(est, scene, f_score_threshold=0.3, number_of_points=5000, device=DEV)
    assert again == got
