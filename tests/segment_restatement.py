"""numpy fp64 restatement of the segmentation entries (include/loner_hip.h, "segmentation"): exact radius neighbours, open3d's
*sequential* DBSCAN, and the RANSAC plane with its Philox draws, chunked score and refit, written out step by step; then the scenes
the host and the GPU tests share.  The Philox generator and the device's order of summation are cloud_tools_restatement's."""
import numpy as np

from tests import cloud_tools_restatement as TR
from tests import global_reg_restatement as GR
from tests import icp_restatement as IR

STREAM_PLANE = 0x504C414E00000000       # LNR_STREAM_PLANE of include/loner_hip.h: "PLAN" in the counter's top word
CHUNK = GR.CHUNK                        # LNR_RANSAC_CHUNK


# ---------------------------------------------------------------- radius neighbours
def radius_neighbours(points, radius):
    """per point the ascending indices j, itself included, with d2(p_i, p_j) < radius * radius (strict, the product rounded once).
    cKDTree finds the candidates at a slightly larger radius; the test is the stated expression."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    r2 = np.float64(radius) * np.float64(radius)
    if len(p) == 0:
        return []
    balls = cKDTree(p).query_ball_point(p, radius * (1 + 1e-9) + 1e-9, workers=16)
    out = []
    for i, cand in enumerate(balls):
        cand = np.sort(np.asarray(cand, dtype=np.int64))
        out.append(cand[GR.sq_dist(p[i][None, :], p[cand]) < r2])
    return out


def radius_counts(points, radius, nbrs=None):
    nbrs = radius_neighbours(points, radius) if nbrs is None else nbrs
    return np.array([len(x) for x in nbrs], dtype=np.int64)


def radius_outlier_mask(points, nb_points, radius):
    """open3d's RemoveRadiusOutliers: kept when the count, the point included, is > nb_points"""
    return radius_counts(points, radius) > nb_points


# ---------------------------------------------------------------- DBSCAN
def dbscan(points, eps, min_points, nbrs=None):
    """open3d's ClusterDBSCAN as it runs: indices in ascending order, a breadth-first walk from every unvisited core, a noise point
    re-labelled by the first cluster that reaches it.  -> (labels int32 [n], info {clusters, cores, border, noise})"""
    nbrs = radius_neighbours(points, eps) if nbrs is None else nbrs
    n = len(nbrs)
    UNDEFINED, NOISE = -2, -1
    labels = np.full(n, UNDEFINED, dtype=np.int64)
    cluster = 0
    for i in range(n):
        if labels[i] != UNDEFINED:
            continue
        if len(nbrs[i]) < min_points:
            labels[i] = NOISE
            continue
        labels[i] = cluster
        queue = list(nbrs[i])
        seen = set(queue)
        seen.add(i)
        at = 0
        while at < len(queue):
            q = queue[at]
            at += 1
            if labels[q] == NOISE:
                labels[q] = cluster
            if labels[q] != UNDEFINED:
                continue
            labels[q] = cluster
            if len(nbrs[q]) >= min_points:
                for x in nbrs[q]:
                    if x not in seen:
                        seen.add(x)
                        queue.append(x)
        cluster += 1
    cores = int(sum(len(x) >= min_points for x in nbrs))
    noise = int((labels == NOISE).sum())
    return labels.astype(np.int32), {"clusters": cluster, "cores": cores, "border": n - cores - noise, "noise": noise}


def small_cluster_mask(labels, min_cluster_points):
    """kept: the points whose cluster has at least min_cluster_points members; noise goes"""
    labels = np.asarray(labels, dtype=np.int64)
    sizes = np.bincount(labels[labels >= 0], minlength=1)
    return (labels >= 0) & (sizes[np.maximum(labels, 0)] >= min_cluster_points)


# ---------------------------------------------------------------- the RANSAC plane
def plane_hypotheses(P, n_hypotheses, seed):
    """-> (status [H]: 0 survives, 1 repeated index, 2 degenerate; planes [H,4] = (nv, d); first [H] the first sample's index)"""
    n = len(P)
    h = np.arange(n_hypotheses, dtype=np.uint64)
    x = TR.philox4x32_10(h, STREAM_PLANE, seed)
    idx = [((x[k].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64) for k in range(3)]
    status = np.zeros(n_hypotheses, dtype=np.int64)
    status[(idx[0] == idx[1]) | (idx[0] == idx[2]) | (idx[1] == idx[2])] = 1
    a, b, c = P[idx[0]], P[idx[1]], P[idx[2]]
    with np.errstate(all="ignore"):
        nrm = GR.cross3(b - a, c - a)
        L = np.sqrt(GR.dot3(nrm, nrm))
        nv = nrm / L[:, None]
        d = -GR.dot3(nv, a)
    planes = np.concatenate([nv, d[:, None]], axis=1)
    bad = (L == 0.0) | ~np.isfinite(L) | ~np.isfinite(planes).all(axis=1)
    status[(status == 0) & bad] = 2
    return status, planes, idx[0]


def plane_residuals(planes, P):
    """[k,n]: e = dot(nv, p) + d"""
    Q = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return ((Q[:, 0, None] * P[None, :, 0] + Q[:, 1, None] * P[None, :, 1]) + Q[:, 2, None] * P[None, :, 2]) + Q[:, 3, None]


def plane_score(planes, P, t):
    """-> (inlier count [k], sum of the inliers' e*e [k]): chunks of 2048 summed left to right, then chunk by chunk"""
    k, n = len(planes), len(P)
    count = np.zeros(k, dtype=np.int64)
    total = np.zeros(k)
    step = max(1, int(4e6 // max(n, 1)))
    for r0 in range(0, k, step):
        e = plane_residuals(planes[r0:r0 + step], P)
        with np.errstate(all="ignore"):
            inl = np.abs(e) < t
            terms = np.where(inl, e * e, 0.0)                         # x + 0.0 = x: skipping a term and adding zero agree
        count[r0:r0 + step] = inl.sum(axis=1)
        acc = np.zeros(len(e))
        for c0 in range(0, n, CHUNK):
            acc = acc + np.add.accumulate(terms[:, c0:c0 + CHUNK], axis=1)[:, -1]
        total[r0:r0 + step] = acc
    return count, total


def plane_cumulants(P, mask, a):
    """the 9 means of the refit and the covariance formed from them, the sums in the device's order (a point that is no inlier adds
    0.0)"""
    with np.errstate(all="ignore"):
        q = P - a[None, :]
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        terms = [np.where(mask, v, 0.0) for v in (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)]
    s = np.array([TR._device_sum(v) for v in terms]) / float(int(mask.sum()))
    C = np.empty((3, 3))
    C[0, 0], C[1, 1], C[2, 2] = s[3] - s[0] * s[0], s[6] - s[1] * s[1], s[8] - s[2] * s[2]
    C[0, 1] = C[1, 0] = s[4] - s[0] * s[1]
    C[0, 2] = C[2, 0] = s[5] - s[0] * s[2]
    C[1, 2] = C[2, 1] = s[7] - s[1] * s[2]
    return s, C


def plane_refit(P, mask, a, nv):
    """-> the refitted (normal, d).  The eigenvector is numpy.linalg.eigh's (with lnr_cloud_normals' exact rules, IR.normal_rule): the
    device's closed form goes through the library's acos and cos, so its normal is compared to a tolerance, not bit for bit"""
    s, C = plane_cumulants(P, mask, a)
    nrm = IR.normal_rule(C)[0][0]
    if GR.dot3(nrm, nv) < 0.0:
        nrm = -nrm
    centre = a + s[:3]
    return np.array([nrm[0], nrm[1], nrm[2], -GR.dot3(nrm, centre)])


def segment_plane(points, distance_threshold, n_hypotheses, seed=0, refine=True):
    """-> the dict of analysis.segmentation.plane_ransac with inlier as a bool array, and counts / sums / alive for the tests' preconditions"""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    out = {"plane": np.zeros(4), "hypothesis_plane": np.zeros(4), "inlier": np.zeros(n, dtype=bool), "status": 0, "best_hypothesis": -1,
           "n_inliers": 0, "survivors": 0, "rejected_repeated": 0, "rejected_degenerate": 0,
           "nonfinite": int((~np.isfinite(P).all(axis=1)).sum()), "n": n}
    if n < 3:
        out["status"] = 1
        return out
    status, planes, first = plane_hypotheses(P, n_hypotheses, seed)
    out.update(rejected_repeated=int((status == 1).sum()), rejected_degenerate=int((status == 2).sum()))
    alive = np.nonzero(status == 0)[0]
    out["survivors"] = len(alive)
    if len(alive) == 0:
        out["status"] = 2
        return out
    count, total = plane_score(planes[alive], P, distance_threshold)
    best = np.lexsort((alive, total, -count))[0]
    h = int(alive[best])
    with np.errstate(all="ignore"):
        mask = np.abs(plane_residuals(planes[h], P)[0]) < distance_threshold
    assert int(mask.sum()) == int(count[best])
    out.update(best_hypothesis=h, n_inliers=int(count[best]), hypothesis_plane=planes[h].copy(), plane=planes[h].copy(), inlier=mask,
               counts=count, sums=total, alive=alive)
    if refine and out["n_inliers"] >= 3:
        out["plane"] = plane_refit(P, mask, P[first[h]], planes[h, :3])
    return out


def segment_planes(points, distance_threshold, max_planes, min_inliers, n_hypotheses, seed=0, refine=True):
    """successive segment_plane calls on what is left -> (models [k,4], labels int32 [n])"""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.full(len(P), -1, dtype=np.int32)
    left = np.arange(len(P))
    models = []
    while len(models) < max_planes and len(left) >= 3:
        r = segment_plane(P[left], distance_threshold, n_hypotheses, seed, refine)
        if r["status"] or r["n_inliers"] < max(min_inliers, 1):
            break
        labels[left[r["inlier"]]] = len(models)
        models.append(r["plane"])
        left = left[~r["inlier"]]
    return np.array(models).reshape(-1, 4), labels


# ---------------------------------------------------------------- the scenes
RANDOM_SETTINGS = ((0.3, 6), (0.5, 12))          # (eps, min_points) of the random DBSCAN cases


def blobs_scene():
    """20 000 points: 8 Gaussian blobs of 1 500, 7 936 uniform noise points and 64 exact copies of one point, shuffled"""
    rng = np.random.default_rng(101)
    centres = rng.uniform(-9, 9, size=(8, 3))
    sigma = rng.uniform(0.5, 1.2, size=8)
    parts = [centres[k] + rng.normal(size=(1500, 3)) * sigma[k] for k in range(8)]
    parts.append(rng.uniform(-12, 12, size=(7936, 3)))
    parts.append(np.tile(centres[0] + [0.3, -0.2, 0.1], (64, 1)))
    p = np.concatenate(parts)
    assert len(p) == 20000
    return p[rng.permutation(len(p))]


SHIFT = np.array([1e4, -2e4, 3e3])


def chain_scene(eps=0.1, n=3000):
    """n points on a line at spacing 0.9 eps in shuffled order: with min_points = 3 one cluster, its two ends border points"""
    rng = np.random.default_rng(102)
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n) * (0.9 * eps)
    return p[rng.permutation(n)]


def lattice_scene():
    """12 x 12 x 12 at spacing 0.25: the nearest neighbours lie at d2 == 0.25 * 0.25 exactly"""
    ax = np.arange(12) * 0.25
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


BORDER_EPS, BORDER_MIN_POINTS = 0.22, 4


def border_scene(swap=False):
    """Two lines of 11 points along y at spacing 0.1, at x = 0 and x = 0.4, and the point (0.2, 0.5, 0): within eps = 0.22 of one core
    of each line (0.2 away; their neighbours on the lines are 0.2236 away) and with 3 neighbours itself, below min_points = 4.
    -> (points [23,3] with that point last, the line that comes first in the input)"""
    y = np.arange(11) * 0.1
    a = np.stack([np.zeros(11), y, np.zeros(11)], 1)
    b = np.stack([np.full(11, 0.4), y, np.zeros(11)], 1)
    first, second = (b, a) if swap else (a, b)
    return np.concatenate([first, second, [[0.2, 0.5, 0.0]]])


BOX_T, BOX_H = 0.003, 512          # 3 sigma of the faces' noise: at 5 sigma every good hypothesis holds every point of a face and the counts tie


def box_corner_scene():
    """4 173 points (2 * 2048 + 77): three mutually orthogonal faces with 2 000 / 1 200 / 700 points in [0, 2]^2 and 1 mm noise along
    their normals, and 273 uniform rows of which two are made NaN; shuffled"""
    rng = np.random.default_rng(103)
    parts = []
    for axis, m in ((2, 2000), (0, 1200), (1, 700)):
        f = rng.uniform(0.0, 2.0, size=(m, 3))
        f[:, axis] = rng.normal(size=m) * 0.001
        parts.append(f)
    out = rng.uniform(0.0, 2.0, size=(273, 3))
    out[5] = np.nan
    out[17, 1] = np.nan
    parts.append(out)
    p = np.concatenate(parts)
    assert len(p) == 4173 == 2 * CHUNK + 77
    return p[rng.permutation(len(p))]


def tie_scene():
    """600 points with integer coordinates on z = 0: every surviving hypothesis holds every point at e = 0"""
    rng = np.random.default_rng(104)
    p = np.zeros((600, 3))
    p[:, :2] = rng.integers(-50, 51, size=(600, 2))
    return p


def collinear_scene():
    """300 points along an axis: every cross product is exactly zero"""
    return np.outer(np.arange(300.0), [1.0, 0.0, 0.0]) + [0.0, 2.0, -1.0]
