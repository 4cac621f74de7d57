"""Point-to-mesh queries without a GPU: the numpy restatement (tests/mesh_distance_restatement.py) against closed forms - plane,
edge and corner distances, the box room from inside, crossing counts and occupancy of closed meshes - the tie rule, and the new Python
entry points refusing bad arguments before they touch a device."""
import math

import numpy as np
import pytest
import torch

from loner_amd.utils import synthetic as SYN
from loner_amd.utils import synthetic_mesh as SM
from tests import mesh_distance_restatement as MR

# coordinates of order 10 and a dozen fp64 operations per figure: about 1e-14; asserted at 1e-12
TOL = 1e-12


def _one(p, tri):
    tri = np.asarray(tri, dtype=np.float64)
    return MR.closest_points(tri, [[0, 1, 2]], np.asarray(p, dtype=np.float64).reshape(-1, 3))


def test_single_triangle_against_closed_forms():
    rng = np.random.default_rng(0)
    A, B, C = np.array([3.0, -7.0, 2.0]), np.array([11.0, -4.0, 5.0]), np.array([5.0, 6.0, -8.0])
    n = np.cross(B - A, C - A)
    n /= np.linalg.norm(n)
    # above the interior: the plane distance, and the foot as u A + v B + (1 - u - v) C
    w = rng.dirichlet((2, 2, 2), 200)
    foot = w @ np.stack([A, B, C])
    h = rng.uniform(-9.0, 9.0, 200)
    got = _one(foot + h[:, None] * n, [A, B, C])
    assert np.abs(np.sqrt(got["dist_sq"]) - np.abs(h)).max() <= TOL
    assert np.abs(got["points"] - foot).max() <= TOL and (got["primitive_ids"] == 0).all()
    u, v = got["primitive_uvs"][:, 0], got["primitive_uvs"][:, 1]
    assert np.abs(u[:, None] * A + v[:, None] * B + (1 - u - v)[:, None] * C - got["points"]).max() <= TOL
    assert np.abs(got["primitive_uvs"] - w[:, :2]).max() <= TOL
    # on the surface: 0
    got = _one(foot, [A, B, C])
    assert np.sqrt(got["dist_sq"]).max() <= TOL
    # beyond a corner: within the cone of directions that leave both edges behind, the distance to the corner
    for P, Q, R in ((A, B, C), (B, C, A), (C, A, B)):
        away = -((Q - P) / np.linalg.norm(Q - P) + (R - P) / np.linalg.norm(R - P))
        p = P + 4.0 * away / np.linalg.norm(away) + 2.5 * n
        got = _one(p, [A, B, C])
        assert abs(math.sqrt(got["dist_sq"][0]) - np.linalg.norm(p - P)) <= TOL and np.abs(got["points"][0] - P).max() == 0.0
    # beyond an edge: the distance to the segment
    for P, Q, R in ((A, B, C), (B, C, A), (C, A, B)):
        e = (Q - P) / np.linalg.norm(Q - P)
        out = np.cross(e, n)
        out = out if out @ (R - P) < 0 else -out                  # in the plane, away from the third corner
        for s in (0.1, 0.5, 0.93):
            on = P + s * (Q - P)
            p = on + 3.0 * out - 1.7 * n
            got = _one(p, [A, B, C])
            assert abs(math.sqrt(got["dist_sq"][0]) - math.hypot(3.0, 1.7)) <= TOL and np.abs(got["points"][0] - on).max() <= TOL
    # the corners themselves and the reach
    got = _one([A, B, C], [A, B, C])
    assert (got["dist_sq"] == 0.0).all() and (got["primitive_uvs"] == [[1, 0], [0, 1], [0, 0]]).all()
    p = foot[:1] + 2.0 * n
    far = MR.closest_points([A, B, C], [[0, 1, 2]], p, max_distance_sq=3.9)
    assert far["primitive_ids"][0] == -1 and np.isinf(far["dist_sq"][0]) and (far["points"] == 0).all()


def test_degenerate_triangles_and_exclusions():
    v = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0],          # a point
                  [0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [2.0, 0.0, 0.0],          # a needle: the third corner is the midpoint
                  [np.nan, 0.0, 0.0]])
    f = np.array([[0, 1, 2], [3, 4, 5], [3, 4, 6], [3, 4, 9]])
    p = np.array([[1.0, 2.0, 7.0], [3.0, 3.0, 0.0], [-1.0, 0.0, 0.0], [np.inf, 0.0, 0.0]])
    got = MR.closest_points(v, f, p)
    assert got["excluded_triangles"] == 1 and got["bad_index"] == 1 and got["invalid_points"] == 1
    assert list(got["primitive_ids"]) == [0, 1, 1, -1]
    assert list(got["dist_sq"]) == [16.0, 9.0, 1.0, np.inf]
    assert (got["points"][1] == [3.0, 0.0, 0.0]).all()


def test_box_room_from_inside_and_the_tie_on_a_shared_diagonal():
    v, f = SM.box_room_mesh()
    lo, hi = np.asarray(SYN.BOX_MIN), np.asarray(SYN.BOX_MAX)
    rng = np.random.default_rng(1)
    p = rng.uniform(lo + 0.01, hi - 0.01, (2000, 3))
    got = MR.closest_points(v, f, p)
    want = np.minimum(p - lo, hi - p).min(axis=1)
    assert np.abs(np.sqrt(got["dist_sq"]) - want).max() <= TOL
    # above the diagonal the floor's two triangles (8 and 9) share: both give the same point, the lower index wins
    on = v[0] + 0.25 * (v[3] - v[0])
    got = MR.closest_points(v, f, on + [0.0, 0.0, 2.0])
    assert got["primitive_ids"][0] == 8 and got["dist_sq"][0] == 4.0 and (got["points"][0] == on).all()
    swapped = f.copy()
    swapped[[8, 9]] = swapped[[9, 8]]
    assert MR.closest_points(v, swapped, on + [0.0, 0.0, 2.0])["primitive_ids"][0] == 8


def test_crossing_counts_and_occupancy_of_closed_meshes():
    v, f = SM.box_room_mesh()
    lo, hi = np.asarray(SYN.BOX_MIN), np.asarray(SYN.BOX_MAX)
    rng = np.random.default_rng(2)
    inside = rng.uniform(lo + 0.01, hi - 0.01, (300, 3))
    d = rng.normal(size=(300, 3))
    assert (MR.count_intersections(v, f, np.concatenate([inside, d], axis=1))["counts"] == 1).all()
    outside = inside + [50.0, 0.0, 0.0]
    counts = MR.count_intersections(v, f, np.concatenate([outside, d], axis=1))["counts"]
    assert set(np.unique(counts)) == {0, 2}
    window = MR.count_intersections(v, f, np.concatenate([outside, d], axis=1), 0.0, 1.0)["counts"]
    assert (window == 0).all()                                   # the box is 30 m away and |d| is a few units at most
    for nsamples in (1, 3):
        assert (MR.occupancy(v, f, inside, nsamples) == 1.0).all() and (MR.occupancy(v, f, outside, nsamples) == 0.0).all()
    r, c = 3.0, np.asarray(SYN.SPHERE_C)
    sv, sf = SM.icosphere(2, r, c)
    u = rng.normal(size=(400, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = np.concatenate([rng.uniform(0.0, 0.95 * r, 200), rng.uniform(1.01 * r, 3 * r, 200)])      # icosphere(2)'s inradius is 0.982 r
    occ = MR.occupancy(sv, sf, c + rad[:, None] * u, 3)
    assert (occ[:200] == 1.0).all() and (occ[200:] == 0.0).all()
    bad = MR.count_intersections(sv, sf, [[np.nan, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0]])
    assert bad["invalid_rays"] == 2 and (bad["counts"] == 0).all()


def test_new_entry_points_refuse_bad_arguments():
    from loner_amd import hip, ops
    from loner_amd.analysis import mesh_eval, raycast
    assert hip.OCCUPANCY_DIRECTIONS == MR.DIRECTIONS
    bvh = ops.BVH.__new__(ops.BVH)                               # never built: every refusal below comes before the library
    bvh.buf, bvh.n_triangles = torch.zeros(8, dtype=torch.uint8), 0
    pts, rays = torch.zeros(4, 3, dtype=torch.float64), torch.ones(4, 6, dtype=torch.float64)
    for args, kwargs in (((None, pts), {}), ((bvh, torch.zeros(4, 2)), {}), ((bvh, torch.zeros(3)), {}), ((bvh, pts.long()), {}),
                         ((bvh, pts.numpy()), {}), ((bvh, pts), dict(max_distance=math.nan)), ((bvh, pts), dict(max_distance=-1.0))):
        with pytest.raises(ValueError):
            ops.closest_points(*args, **kwargs)
    for args, kwargs in (((None, rays), {}), ((bvh, pts), {}), ((bvh, rays.int()), {}), ((bvh, rays), dict(t_min=math.nan)),
                         ((bvh, rays), dict(t_max=math.nan))):
        with pytest.raises(ValueError):
            ops.count_intersections(*args, **kwargs)
    with pytest.raises(RuntimeError):                            # host tensors: there is no CPU implementation
        ops.closest_points(bvh, pts)
    with pytest.raises(RuntimeError):
        ops.count_intersections(bvh, rays)
    scene = raycast.RaycastingScene.__new__(raycast.RaycastingScene)
    scene.vertices, scene.triangles = torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, 3, dtype=torch.int32)
    scene.bvh, scene._normals = bvh, None
    for call in (lambda: scene.compute_closest_points(torch.zeros(4, 2)), lambda: scene.compute_closest_points(pts.long()),
                 lambda: scene.compute_closest_points(pts, max_distance=math.nan), lambda: scene.compute_distance(torch.zeros(())),
                 lambda: scene.compute_distance(pts, max_distance=math.nan), lambda: scene.count_intersections(pts),
                 lambda: scene.count_intersections(rays, t_min=math.nan), lambda: scene.compute_occupancy(pts, nsamples=2),
                 lambda: scene.compute_occupancy(pts, nsamples=0), lambda: scene.compute_occupancy(pts, nsamples=True),
                 lambda: scene.compute_occupancy(rays), lambda: scene.compute_signed_distance(pts, nsamples=2),
                 lambda: scene.compute_signed_distance(torch.zeros(4, 4)),
                 lambda: mesh_eval.cloud_to_mesh_distance(pts, object()), lambda: mesh_eval.cloud_to_mesh_distance(torch.zeros(4, 2), scene),
                 lambda: mesh_eval.cloud_to_mesh_distance(pts, scene, max_distance=math.nan),
                 lambda: mesh_eval.evaluate_mesh_to_mesh(object(), scene), lambda: mesh_eval.evaluate_mesh_to_mesh(scene, 7),
                 lambda: mesh_eval.evaluate_mesh_to_mesh(scene, scene, number_of_points=0),
                 lambda: mesh_eval.evaluate_mesh_to_mesh(scene, scene, f_score_threshold=math.nan)):
        with pytest.raises(ValueError):
            call()
