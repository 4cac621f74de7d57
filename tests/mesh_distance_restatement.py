"""Plain numpy fp64 restatements of the point queries of include/loner_hip.h's "ray casting" block, operation by operation and by
brute force over every triangle: the closest point of a triangle (Ericson's region walk as np.where chains in the stated order), the
answer rule ((squared distance, index) lexicographic), the crossing count on raycast_restatement's hit rule, and occupancy along the
stated directions."""
import numpy as np

from tests import raycast_restatement as RR

INF = np.inf
# LNR_OCCUPANCY_DIRECTIONS
DIRECTIONS = ((1.0, 0.4142135623730951, 0.7320508075688772), (-0.6180339887498949, 1.0, 0.3027756377319946),
              (0.2360679774997897, -0.7071067811865476, 1.0))


def usable_triangles(vertices, triangles):
    """-> (v fp64 [V,3], f int64 [F,3], the indices of the triangles the build keeps, excluded for a non-finite vertex, bad indices)"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < len(v))).all(axis=1)
    finite = np.zeros(len(f), dtype=bool)
    finite[in_range] = np.isfinite(v[f[in_range]]).all(axis=(1, 2))
    return v, f, np.nonzero(in_range & finite)[0], int((in_range & ~finite).sum()), int((~in_range).sum())


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def triangle_closest(p, A, B, C):
    """p [n,1,3] (or [n,3]) against corners [m,3] (or [n,3]) by broadcasting -> (q [...,3], squared distance, u, v); the first
    branch that applies wins, so the chain is built from the last branch backwards"""
    with np.errstate(all="ignore"):
        ab, ac, ap = B - A, C - A, p - A
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - B
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - C
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        A, B, C = (np.broadcast_to(x, ap.shape) for x in (A, B, C))
        # inside
        den = 1.0 / ((va + vb) + vc)
        v_in, w_in = vb * den, vc * den
        q = (A + ab * v_in[..., None]) + ac * w_in[..., None]
        vB, wC = v_in, w_in
        # the edge BC
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
        q = np.where(m[..., None], B + w_bc[..., None] * (C - B), q)
        vB, wC = np.where(m, 1.0 - w_bc, vB), np.where(m, w_bc, wC)
        # the edge AC
        w_ac = d2 / (d2 - d6)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        q = np.where(m[..., None], A + w_ac[..., None] * ac, q)
        vB, wC = np.where(m, zero, vB), np.where(m, w_ac, wC)
        # the corner C
        m = (d6 >= 0) & (d5 <= d6)
        q = np.where(m[..., None], C, q)
        vB, wC = np.where(m, zero, vB), np.where(m, one, wC)
        # the edge AB
        v_ab = d1 / (d1 - d3)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        q = np.where(m[..., None], A + v_ab[..., None] * ab, q)
        vB, wC = np.where(m, v_ab, vB), np.where(m, zero, wC)
        # the corner B
        m = (d3 >= 0) & (d4 <= d3)
        q = np.where(m[..., None], B, q)
        vB, wC = np.where(m, one, vB), np.where(m, zero, wC)
        # the corner A
        m = (d1 <= 0) & (d2 <= 0)
        q = np.where(m[..., None], A, q)
        vB, wC = np.where(m, zero, vB), np.where(m, zero, wC)
        pq = p - q
        return q, dot(pq, pq), (1.0 - vB) - wC, vB


def closest_points(vertices, triangles, points, max_distance_sq=INF, chunk=512):
    """-> dict(dist_sq fp64 [n], primitive_ids int32 [n], points fp64 [n,3], primitive_uvs fp64 [n,2], invalid_points,
    excluded_triangles, bad_index): every usable triangle against every finite query; the answer is the candidate (squared distance
    <= max_distance_sq, never a NaN) with the smallest (squared distance, index)"""
    v, f, usable, excluded, bad_index = usable_triangles(vertices, triangles)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    out = dict(dist_sq=np.full(n, INF), primitive_ids=np.full(n, -1, dtype=np.int32), points=np.zeros((n, 3)),
               primitive_uvs=np.zeros((n, 2)), excluded_triangles=excluded, bad_index=bad_index)
    valid = np.isfinite(p).all(axis=1)
    out["invalid_points"] = int((~valid).sum())
    rows = np.nonzero(valid)[0]
    if len(rows) == 0 or len(usable) == 0:
        return out
    A, B, C = (v[f[usable, k]] for k in range(3))
    for start in range(0, len(rows), chunk):
        r = rows[start:start + chunk]
        q, dd, u, vv = triangle_closest(p[r][:, None, :], A[None], B[None], C[None])
        with np.errstate(invalid="ignore"):
            cand = dd <= max_distance_sq                                      # False for a NaN
        key = np.where(cand, dd, INF)
        # the smallest distance, then the smallest index: `usable` ascends, and argmin returns the first of equal keys.  A
        # candidate at +inf ties with the non-candidates, so candidates are ranked ahead of them explicitly
        best = np.lexsort((np.broadcast_to(np.arange(len(usable)), key.shape), ~cand, key), axis=1)[:, 0]
        ar = np.arange(len(r))
        found = cand[ar, best]
        rf, bf = r[found], best[found]
        out["dist_sq"][rf] = dd[ar[found], bf]
        out["primitive_ids"][rf] = usable[bf].astype(np.int32)
        out["points"][rf] = q[ar[found], bf]
        out["primitive_uvs"][rf, 0] = u[ar[found], bf]
        out["primitive_uvs"][rf, 1] = vv[ar[found], bf]
    return out


def count_intersections(vertices, triangles, rays, t_min=0.0, t_max=INF):
    """-> dict(counts int32 [n], invalid_rays, excluded_triangles): the triangles RR.cast_rays' rule accepts, one triangle at a time"""
    v, f, usable, excluded, _ = usable_triangles(vertices, triangles)
    r = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    counts = np.zeros(len(r), dtype=np.int32)
    invalid = 0
    for t in usable:
        got = RR.cast_rays(v, f[t:t + 1], r, t_min, t_max)
        counts += got["primitive_ids"] >= 0
        invalid = got["invalid_rays"]
    if len(usable) == 0:
        invalid = RR.cast_rays(v, f[:0], r, t_min, t_max)["invalid_rays"]
    return dict(counts=counts, invalid_rays=invalid, excluded_triangles=excluded)


def occupancy(vertices, triangles, points, nsamples=3):
    """1.0 where the crossing count from the point along the stated direction(s), over [0, inf], is odd (nsamples 1) or odd for at
    least two of the three (nsamples 3)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    odd = np.zeros(len(p), dtype=np.int64)
    for d in DIRECTIONS[:nsamples]:
        rays = np.concatenate([p, np.broadcast_to(np.asarray(d), p.shape)], axis=1)
        odd += count_intersections(vertices, triangles, rays)["counts"] & 1
    return (2 * odd > nsamples).astype(np.float64)
