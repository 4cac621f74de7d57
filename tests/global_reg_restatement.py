"""numpy fp64 restatement of global registration (include/loner_hip.h, "global registration"): normal orientation, FPFH, the nearest
neighbour in feature space and RANSAC on correspondences, written out operation by operation: the device must give the same bits.
Every sum is an explicit left-to-right loop or np.add.accumulate, never np.sum.  The neighbour search is icp_restatement.knn, the draws
are cloud_tools_restatement.philox4x32_10, and the angle bins' literals are read from the library (lnr_fpfh_bin_edges, host only)."""
import numpy as np

from tests import cloud_restatement as CR
from tests import cloud_tools_restatement as TR
from tests import icp_restatement as IR

STREAM_RANSAC = 0x524E534300000000      # LNR_STREAM_RANSAC of include/loner_hip.h: "RNSC" in the counter's top word
KNN_MAX = 32
CHUNK = 2048                            # LNR_RANSAC_CHUNK


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def sq_dist(q, t):
    d = q - t
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ---------------------------------------------------------------- orientation
def orient(normals, points=None, location=None, direction=None):
    """-> (normals, non-finite normals, normals flipped)"""
    nrm = np.array(normals, dtype=np.float64).reshape(-1, 3)
    bad = ~np.isfinite(nrm).all(1)
    with np.errstate(all="ignore"):
        if location is not None:
            d = dot3(np.asarray(location, dtype=np.float64)[None, :] - np.asarray(points, dtype=np.float64).reshape(-1, 3), nrm)
        else:
            d = dot3(nrm, np.asarray(direction, dtype=np.float64)[None, :])
        flip = ~bad & (d < 0.0)
    nrm[flip] = -nrm[flip]
    return nrm, int(bad.sum()), int(flip.sum())


# ---------------------------------------------------------------- FPFH
def bin_edges():
    from loner_amd.analysis import registration
    return registration.fpfh_bin_edges()


def unit_bin(f):
    with np.errstate(all="ignore"):
        b = np.floor(11.0 * ((f + 1.0) * 0.5))
        b = np.where(b > 10.0, 10.0, b)
        b = np.where(b >= 0.0, b, 0.0)
    return b.astype(np.int64)


def angle_bin(y, x, edges):
    """the bin of atan2(y, x) from the signs of y c_b - x s_b, b = 1..10 (edges [10,2] = (c_b, s_b))"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    ge = [(y * edges[b - 1, 0] - x * edges[b - 1, 1]) >= 0.0 for b in range(1, 11)]
    low = np.zeros(y.shape, dtype=np.int64)
    for b in range(5):
        low = low + ge[b]
    high = np.full(y.shape, 5, dtype=np.int64)
    for b in range(5, 10):
        high = high + ge[b]
    out = np.where(y < 0.0, low, high)
    return np.where((x == 0.0) & (y == 0.0), 5, out)


def neighbours(points, radius, max_nn):
    """-> (ids [n,32] int64, d2 [n,32], count [n]): of the min(max_nn, n) smallest (d2, index) pairs those with d2 < radius*radius, less
    the point itself, in list order"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    idx, d2 = IR.knn(p, max_nn)
    r2 = radius * radius
    ids = np.zeros((n, KNN_MAX), dtype=np.int64)
    out = np.zeros((n, KNN_MAX))
    cnt = np.zeros(n, dtype=np.int64)
    for j in range(idx.shape[1]):
        keep = (d2[:, j] < r2) & (idx[:, j] != np.arange(n))
        rows = np.nonzero(keep)[0]
        ids[rows, cnt[rows]] = idx[rows, j]
        out[rows, cnt[rows]] = d2[rows, j]
        cnt[rows] += 1
    return ids, out, cnt


def pair_bins(p1, n1, p2, n2, edges):
    """(angle bin, f1 bin, f2 bin) of the pair features of (p1, n1) -> (p2, n2), row by row"""
    with np.errstate(all="ignore"):
        d = p2 - p1
        f3 = np.sqrt(dot3(d, d))
        a1, a2 = dot3(n1, d) / f3, dot3(n2, d) / f3
        swap = np.abs(a1) < np.abs(a2)
        m1 = np.where(swap[:, None], n2, n1)
        m2 = np.where(swap[:, None], n1, n2)
        ds = np.where(swap[:, None], -d, d)
        f2 = np.where(swap, -a2, a1)
        v = cross3(ds, m1)
        vn = np.sqrt(dot3(v, v))
        v = v / vn[:, None]
        w = cross3(m1, v)
        f1 = dot3(v, m2)
        y, x = dot3(w, m2), dot3(m1, m2)
        zero = (f3 == 0.0) | (vn == 0.0) | ~np.isfinite(n1).all(1) | ~np.isfinite(n2).all(1)
        ba = np.where(zero, 5, angle_bin(y, x, edges))
        b1 = np.where(zero, 5, unit_bin(f1))
        b2 = np.where(zero, 5, unit_bin(f2))
    return ba, b1, b2


def spfh(points, normals, ids, cnt, edges):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    hist = np.zeros((n, 33), dtype=np.int64)
    for s in range(KNN_MAX):
        rows = np.nonzero(s < cnt)[0]
        if len(rows) == 0:
            break
        k = ids[rows, s]
        ba, b1, b2 = pair_bins(p[rows], nrm[rows], p[k], nrm[k], edges)
        hist[rows, ba] += 1
        hist[rows, 11 + b1] += 1
        hist[rows, 22 + b2] += 1
    out = np.zeros((n, 33))
    has = cnt > 0
    out[has] = hist[has].astype(np.float64) * (100.0 / cnt[has].astype(np.float64))[:, None]
    return out


def fpfh(points, normals, radius, max_nn, edges=None):
    """-> (features [n,33], points whose own normal is not finite)"""
    edges = bin_edges() if edges is None else edges
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ids, d2, cnt = neighbours(p, radius, max_nn)
    own = spfh(p, normals, ids, cnt, edges)
    n = len(p)
    acc = np.zeros((n, 33))
    total = np.zeros((n, 3))
    for s in range(KNN_MAX):
        rows = np.nonzero((s < cnt) & (d2[:, s] != 0.0))[0]
        if len(rows) == 0:
            continue
        val = own[ids[rows, s]] / d2[rows, s][:, None]
        acc[rows] = acc[rows] + val
        for j in range(33):
            total[rows, j // 11] = total[rows, j // 11] + val[:, j]
    wide = np.repeat(total, 11, axis=1)
    with np.errstate(all="ignore"):
        scaled = np.where(wide != 0.0, acc * (100.0 / wide), acc)
    return scaled + own, int((~np.isfinite(np.asarray(normals, dtype=np.float64).reshape(-1, 3)).all(1)).sum())


# ---------------------------------------------------------------- nearest neighbour in feature space
def feature_nearest(targets, queries):
    """-> (index [n_q] int64, -1 for none; d2 [n_q], +inf for none): the smallest (d2, index) over the targets whose d2 is not NaN"""
    t = np.asarray(targets, dtype=np.float64)
    q = np.asarray(queries, dtype=np.float64)
    n_q, dim = q.shape
    index = np.full(n_q, -1, dtype=np.int64)
    best = np.full(n_q, np.inf)
    if len(t) == 0:
        return index, best
    for b in range(0, n_q, 128):
        qq = q[b:b + 128]
        d2 = np.zeros((len(qq), len(t)))
        with np.errstate(all="ignore"):
            for j in range(dim):
                df = qq[:, None, j] - t[None, :, j]
                d2 = d2 + df * df
        valid = ~np.isnan(d2)
        d2m = np.where(valid, d2, np.inf)
        lo = d2m.min(axis=1)
        first = np.argmax(valid & (d2m == lo[:, None]), axis=1)       # the first (lowest) index at the minimum
        ok = valid.any(axis=1)
        index[b:b + 128][ok] = first[ok]
        best[b:b + 128][ok] = lo[ok]
    return index, best


def correspondences_from_features(src_f, tgt_f, mutual_filter=False):
    idx, _ = feature_nearest(tgt_f, src_f)
    i = np.arange(len(idx))
    keep = idx >= 0
    if mutual_filter:
        back, _ = feature_nearest(src_f, tgt_f)
        keep = keep & (back[np.where(keep, idx, 0)] == i)
    return np.stack([i[keep], idx[keep]], axis=1).astype(np.int32)


# ---------------------------------------------------------------- RANSAC
def _frames(a, b, c):
    """[n,3,3] with F[:, k] = e_{k+1}, and which are finite"""
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        e1 = ab / np.sqrt(dot3(ab, ab))[:, None]
        nrm = cross3(e1, ac)
        e3 = nrm / np.sqrt(dot3(nrm, nrm))[:, None]
        e2 = cross3(e3, e1)
    F = np.stack([e1, e2, e3], axis=1)
    return F, np.isfinite(F).all(axis=(1, 2))


def hypotheses(S, T, n_hypotheses, seed, e):
    """S, T [m,3] the correspondences' points.  -> (status [H]: 0 survives, 1 repeated index, 2 edge checker, 3 frame; poses [H,12])"""
    m = len(S)
    h = np.arange(n_hypotheses, dtype=np.uint64)
    x = TR.philox4x32_10(h, STREAM_RANSAC, seed)
    idx = [((x[k].astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64) for k in range(3)]
    status = np.zeros(n_hypotheses, dtype=np.int64)
    status[(idx[0] == idx[1]) | (idx[0] == idx[2]) | (idx[1] == idx[2])] = 1
    s = [S[idx[k]] for k in range(3)]
    t = [T[idx[k]] for k in range(3)]
    with np.errstate(all="ignore"):
        if e != 0.0:
            bad = np.zeros(n_hypotheses, dtype=bool)
            for k in range(3):
                j = (k + 1) % 3
                ls, lt = np.sqrt(sq_dist(s[k], s[j])), np.sqrt(sq_dist(t[k], t[j]))
                bad |= ~((ls >= e * lt) & (lt >= e * ls))
            status[(status == 0) & bad] = 2
        Fs, oks = _frames(*s)
        Ft, okt = _frames(*t)
        status[(status == 0) & ~(oks & okt)] = 3
        cs = ((s[0] + s[1]) + s[2]) / 3.0
        ct = ((t[0] + t[1]) + t[2]) / 3.0
        P = np.zeros((n_hypotheses, 12))
        for a in range(3):
            for b in range(3):
                P[:, 4 * a + b] = (Ft[:, 0, a] * Fs[:, 0, b] + Ft[:, 1, a] * Fs[:, 1, b]) + Ft[:, 2, a] * Fs[:, 2, b]
            P[:, 4 * a + 3] = ct[:, a] - ((P[:, 4 * a] * cs[:, 0] + P[:, 4 * a + 1] * cs[:, 1]) + P[:, 4 * a + 2] * cs[:, 2])
    return status, P


def score(P, S, T, max_distance):
    """-> (inlier count [k], sum of the inlier d2 [k]) of the poses P [k,12]: chunks of 2048 summed left to right, then chunk by chunk"""
    dd = max_distance * max_distance
    k, m = len(P), len(S)
    count = np.zeros(k, dtype=np.int64)
    total = np.zeros(k)
    step = max(1, int(4e6 // max(m, 1)))
    for r0 in range(0, k, step):
        Q = P[r0:r0 + step]
        with np.errstate(all="ignore"):
            p = np.stack([((Q[:, 4 * a, None] * S[None, :, 0] + Q[:, 4 * a + 1, None] * S[None, :, 1]) + Q[:, 4 * a + 2, None] * S[None, :, 2])
                          + Q[:, 4 * a + 3, None] for a in range(3)], axis=-1)
            d2 = sq_dist(p, T[None, :, :])
            inl = d2 < dd
        count[r0:r0 + step] = inl.sum(axis=1)                         # integers
        terms = np.where(inl, d2, 0.0)                                # x + 0.0 = x: skipping a term and adding zero agree
        acc = np.zeros(len(Q))
        for c0 in range(0, m, CHUNK):
            acc = acc + np.add.accumulate(terms[:, c0:c0 + CHUNK], axis=1)[:, -1]
        total[r0:r0 + step] = acc
    return count, total


def ransac(source, target, corr, n_hypotheses, seed, max_distance, edge_similarity):
    """-> the dict of ops.ransac_correspondence (strict=False)"""
    src = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    tgt = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    corr = np.asarray(corr, dtype=np.int64).reshape(-1, 2)
    m = len(corr)
    out = {"transformation": np.eye(4), "fitness": 0.0, "inlier_rmse": 0.0, "status": 0, "best_hypothesis": -1, "n_inliers": 0, "survivors": 0,
           "rejected_repeated": 0, "rejected_edge": 0, "rejected_frame": 0, "n_correspondences": m}
    if m < 3:
        out["status"] = 1
        return out
    S, T = src[corr[:, 0]], tgt[corr[:, 1]]
    status, P = hypotheses(S, T, n_hypotheses, seed, float(edge_similarity))
    out.update(rejected_repeated=int((status == 1).sum()), rejected_edge=int((status == 2).sum()), rejected_frame=int((status == 3).sum()))
    alive = np.nonzero(status == 0)[0]
    out["survivors"] = len(alive)
    if len(alive) == 0:
        out["status"] = 2
        return out
    count, total = score(P[alive], S, T, max_distance)
    best = np.lexsort((alive, total, -count))[0]
    c = int(count[best])
    out["best_hypothesis"] = int(alive[best])
    out["n_inliers"] = c
    out["transformation"] = np.vstack([P[alive[best]].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
    out["fitness"] = c / m if c else 0.0
    out["inlier_rmse"] = float(np.sqrt(total[best] / c)) if c else 0.0
    return out


# ---------------------------------------------------------------- the test scene
VOXEL = 0.25
VIEWPOINT = np.array([6.0, 6.0, 30.0])
MOVE = IR.rigid(140, (3.0, -2.0, 1.5))


def height_field(seed, n=48, step=0.25):
    """a jittered n x n height field at `step`: a sum of 12 fixed sinusoids"""
    rng = np.random.default_rng(seed)
    u = np.arange(n) * step
    X, Y = np.meshgrid(u, u, indexing="ij")
    X = X + rng.uniform(-0.08, 0.08, X.shape)
    Y = Y + rng.uniform(-0.08, 0.08, Y.shape)
    waves = np.random.default_rng(4242)
    Z = np.zeros_like(X)
    for _ in range(12):
        kx, ky = waves.uniform(-2.2, 2.2, 2)
        Z = Z + waves.uniform(0.12, 0.4) * np.sin(kx * X + ky * Y + waves.uniform(0, 2 * np.pi))
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


def scene():
    """-> (source [k,3] in its own frame, target [n,3], truth 4x4 with truth @ source = the source's true place, the source's
    viewpoint, the target's viewpoint)"""
    target = height_field(1)
    other = height_field(2)
    other = other[(other[:, 0] > 2.0) & (other[:, 1] < 9.5)]
    inv = np.linalg.inv(MOVE)
    source = CR.transform(other, inv)
    view_s = inv[:3, :3] @ VIEWPOINT + inv[:3, 3]
    return source, target, MOVE, view_s, VIEWPOINT


def host_normals(points, knn=30):
    """normals of a cloud on the CPU (eigh; the GPU tests take the device's own)"""
    idx, _ = IR.knn(points, knn)
    return IR.normal_rule(IR.covariance(points, idx))[0]
