"""numpy fp64 restatement of normals and point-to-plane ICP (include/loner_hip.h, "normals and point-to-plane ICP"): open3d's
EstimateNormals, RegistrationICP and TransformationEstimationPointToPlane as this project defines them, written out step by step."""
import numpy as np

from tests import cloud_restatement as CR

DBL_MIN = np.finfo(np.float64).tiny


def knn(points, k, queries=None):
    """indices [n, min(k, n)] and d2 of the k smallest (d2, index) pairs per query (the points themselves by default), ascending;
    d2 = (dx*dx + dy*dy) + dz*dz.  cKDTree finds a candidate set (ball at the k-th distance plus a margin), the order is ours."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    q = p if queries is None else np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    m = min(k, len(p))
    tree = cKDTree(p)
    dk = tree.query(q, k=m, workers=16)[0].reshape(len(q), -1)[:, -1]
    idx = np.empty((len(q), m), dtype=np.int64)
    d2o = np.empty((len(q), m))
    balls = tree.query_ball_point(q, dk * (1 + 1e-9) + 1e-12, workers=16)
    for i, cand in enumerate(balls):
        cand = np.asarray(cand, dtype=np.int64)
        d = q[i] - p[cand]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        o = np.lexsort((cand, d2))[:m]
        idx[i], d2o[i] = cand[o], d2[o]
    return idx, d2o


def covariance(points, idx):
    """[n,3,3]: cumulants summed in neighbour order, divided by the count, C_ab = m_ab - m_a m_b; the identity below 3 neighbours"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n, m = idx.shape
    if m < 3:
        return np.tile(np.eye(3), (n, 1, 1))
    s = np.zeros((n, 9))
    for j in range(m):
        x, y, z = p[idx[:, j], 0], p[idx[:, j], 1], p[idx[:, j], 2]
        for v, t in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            s[:, v] = s[:, v] + t
    s = s / float(m)
    C = np.empty((n, 3, 3))
    C[:, 0, 0] = s[:, 3] - s[:, 0] * s[:, 0]
    C[:, 1, 1] = s[:, 6] - s[:, 1] * s[:, 1]
    C[:, 2, 2] = s[:, 8] - s[:, 2] * s[:, 2]
    C[:, 0, 1] = C[:, 1, 0] = s[:, 4] - s[:, 0] * s[:, 1]
    C[:, 0, 2] = C[:, 2, 0] = s[:, 5] - s[:, 0] * s[:, 2]
    C[:, 1, 2] = C[:, 2, 1] = s[:, 7] - s[:, 1] * s[:, 2]
    return C


def normal_rule(C):
    """-> (normals [n,3], exact [n] bool): the smallest eigenvector by numpy.linalg.eigh, except the exact rules: zero off-diagonals
    give (1,0,0) / (0,1,0) / (0,0,1) by the diagonal compares, an all-zero C gives (0,0,1)."""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 3, 3)
    w, V = np.linalg.eigh(C)
    out = V[:, :, 0].copy()
    off = (C[:, 0, 1] == 0) & (C[:, 0, 2] == 0) & (C[:, 1, 2] == 0)
    d0, d1, d2 = C[:, 0, 0], C[:, 1, 1], C[:, 2, 2]
    e = np.zeros((len(C), 3))
    x = (d0 < d1) & (d0 < d2)
    y = ~x & (d1 < d0) & (d1 < d2)
    e[x, 0] = 1
    e[y, 1] = 1
    e[~x & ~y, 2] = 1
    out[off] = e[off]
    return out, off


def eigen_gap(C):
    """the relative gap between the two smallest eigenvalues (where the eigenvector is well conditioned)"""
    w = np.linalg.eigvalsh(np.asarray(C).reshape(-1, 3, 3))
    return (w[:, 1] - w[:, 0]) / np.maximum(np.abs(w).max(1), 1e-300)


def correspondences(source, target, r):
    """brute force: the smallest (d2, index) target with d2 < r*r per source; -1 and inf for none"""
    s = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    idx = np.full(len(s), -1, dtype=np.int64)
    best = np.full(len(s), np.inf)
    r2 = r * r
    for b in range(0, len(s), 256):
        d = s[b:b + 256, None, :] - t[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2 = np.where(d2 < r2, d2, np.inf)
        j = np.argmin(d2, axis=1)               # the first (lowest) index of the minimum
        v = d2[np.arange(len(j)), j]
        ok = np.isfinite(v)
        idx[b:b + 256][ok] = j[ok]
        best[b:b + 256][ok] = v[ok]
    return idx, best


def correspondences_grid(source, target, r):
    """the same rule through a cKDTree ball query (for large clouds)"""
    from scipy.spatial import cKDTree
    s = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    idx = np.full(len(s), -1, dtype=np.int64)
    best = np.full(len(s), np.inf)
    balls = cKDTree(t).query_ball_point(s, r * (1 + 1e-9), workers=16)
    for i, cand in enumerate(balls):
        if not cand:
            continue
        cand = np.asarray(cand, dtype=np.int64)
        d = s[i] - t[cand]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = d2 < r * r
        if keep.any():
            cand, d2 = cand[keep], d2[keep]
            o = np.lexsort((cand, d2))[0]
            idx[i], best[i] = cand[o], d2[o]
    return idx, best


def system(source, target, normals, idx):
    """JTJ [6,6], JTr [6], sum d2 over the correspondences (r = (s - t).n, J = [s x n, n])"""
    s = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    ok = idx >= 0
    s = s[ok]
    t = np.asarray(target)[idx[ok]]
    n = np.asarray(normals)[idx[ok]]
    dv = s - t
    r = (dv[:, 0] * n[:, 0] + dv[:, 1] * n[:, 1]) + dv[:, 2] * n[:, 2]
    J = np.empty((len(s), 6))
    J[:, 0] = s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1]
    J[:, 1] = s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2]
    J[:, 2] = s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0]
    J[:, 3:] = n
    return J.T @ J, J.T @ r, len(s)


def ldlt_solve(A, b):
    """Eigen's LDLT with symmetric pivoting on the largest remaining |diagonal| (first on ties), left-looking; the solve zeroes the
    components whose |D_i| <= DBL_MIN"""
    A = np.array(A, dtype=np.float64)
    n = len(A)
    perm = list(range(n))
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))
        perm[k] = p
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
        if k > 0:
            temp = np.array([A[j, j] * A[k, j] for j in range(k)])
            s = 0.0
            for j in range(k):
                s = s + A[k, j] * temp[j]
            A[k, k] = A[k, k] - s
            for i in range(k + 1, n):
                t = 0.0
                for j in range(k):
                    t = t + A[i, j] * temp[j]
                A[i, k] = A[i, k] - t
        akk = A[k, k]
        if k == 0 and not abs(akk) > 0:
            perm = list(range(n))
            break
        if abs(akk) > 0:
            A[k + 1:, k] = A[k + 1:, k] / akk
    y = np.array(b, dtype=np.float64)
    for k in range(n):
        y[k], y[perm[k]] = y[perm[k]], y[k]
    for i in range(n):
        s = 0.0
        for j in range(i):
            s = s + A[i, j] * y[j]
        y[i] = y[i] - s
    for i in range(n):
        y[i] = y[i] / A[i, i] if abs(A[i, i]) > DBL_MIN else 0.0
    for i in range(n - 1, -1, -1):
        s = 0.0
        for j in range(i + 1, n):
            s = s + A[j, i] * y[j]
        y[i] = y[i] - s
    for k in range(n - 1, -1, -1):
        y[k], y[perm[k]] = y[perm[k]], y[k]
    return y


def step_matrix(x):
    """TransformVector6dToMatrix4d: [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5]"""
    ca, sa, cb, sb, cc, sc = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([[cc * cb, (cc * sb) * sa - sc * ca, (cc * sb) * ca + sc * sa, x[3]],
                     [sc * cb, (sc * sb) * sa + cc * ca, (sc * sb) * ca - cc * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def matmul4(U, T):
    out = np.empty((4, 4))
    for a in range(4):
        for c in range(4):
            out[a, c] = ((U[a, 0] * T[0, c] + U[a, 1] * T[1, c]) + U[a, 2] * T[2, c]) + U[a, 3] * T[3, c]
    return out


def icp(source, target, normals, r, init=np.eye(4), relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, corr=None):
    """RegistrationICP, point to plane -> dict(transformation, fitness, inlier_rmse, n_correspondences, iterations)"""
    corr = corr or (correspondences if len(source) * max(len(target), 1) <= 4e7 else correspondences_grid)
    pcd = CR.transform(source, init)
    T = np.array(init, dtype=np.float64)

    def result(pcd):
        idx, d2 = corr(pcd, target, r)
        k = int((idx >= 0).sum())
        fit = k / len(pcd) if k else 0.0
        rmse = float(np.sqrt(d2[idx >= 0].sum() / k)) if k else 0.0
        return idx, fit, rmse, k

    idx, fit, rmse, k = result(pcd)
    rounds = 0
    for _ in range(max_iteration):
        if k:
            JTJ, JTr, _ = system(pcd, target, normals, idx)
            U = step_matrix(ldlt_solve(JTJ, -JTr))
        else:
            U = np.eye(4)
        T = matmul4(U, T)
        pcd = CR.transform(pcd, U)
        prev = (fit, rmse)
        idx, fit, rmse, k = result(pcd)
        rounds += 1
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fit, "inlier_rmse": rmse, "n_correspondences": k, "iterations": rounds}


def box_scene(step):
    """the synthetic scene's surfaces (box walls without the window, and the sphere) sampled at about `step`"""
    from loner_amd.utils import synthetic as SY
    lo, hi = np.array(SY.BOX_MIN), np.array(SY.BOX_MAX)
    parts = []
    for a in range(3):
        b, c = [i for i in range(3) if i != a]
        u = np.arange(lo[b], hi[b] + 1e-9, step)
        w = np.arange(lo[c], hi[c] + 1e-9, step)
        U, W = np.meshgrid(u, w, indexing="ij")
        for side in (lo[a], hi[a]):
            P = np.zeros((U.size, 3))
            P[:, a], P[:, b], P[:, c] = side, U.ravel(), W.ravel()
            if a == 0 and side == hi[0]:
                window = (np.abs(P[:, 1]) < SY.WINDOW_HALF_Y) & (P[:, 2] > SY.WINDOW_Z[0]) & (P[:, 2] < SY.WINDOW_Z[1])
                P = P[~window]
            parts.append(P)
    n = int(4 * np.pi * SY.SPHERE_R ** 2 / step ** 2)
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    theta = np.pi * (1 + 5 ** 0.5) * i
    parts.append(np.array(SY.SPHERE_C) + SY.SPHERE_R * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], 1))
    return np.concatenate(parts)


def rigid(deg, shift, axis=(0.3, -0.5, 0.8)):
    """a rigid 4x4: rotation by deg about axis, then the shift"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = shift
    return T
