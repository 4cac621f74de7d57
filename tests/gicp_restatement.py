"""numpy fp64 restatement of the robust kernels and generalized ICP (include/loner_hip.h, "robust kernels and generalized ICP"): the
plane rule, the combined covariance and its cofactor inverse in the header's order, the weights, one round's system and the full loop.
The sums over correspondences are numpy's (pairwise), so systems agree with the device to rounding, not bit for bit; everything per
point is written operation by operation."""
import numpy as np

from tests import cloud_restatement as CR
from tests import icp_restatement as IR

KINDS = ("l2", "huber", "cauchy", "tukey")


def plane_covariances(normals, epsilon):
    """[n,3,3]: C_ab = delta_ab - ((1 - epsilon) n_a) n_b for a <= b, mirrored"""
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    f = 1.0 - epsilon
    C = np.empty((len(n), 3, 3))
    with np.errstate(invalid="ignore"):
        for a in range(3):
            for b in range(a, 3):
                C[:, a, b] = C[:, b, a] = (1.0 if a == b else 0.0) - (f * n[:, a]) * n[:, b]
    return C


def weight(kind, m, k):
    """w(m) of the kernel `kind` with the scale k"""
    m = np.asarray(m, dtype=np.float64)
    if kind == "l2":
        return np.ones_like(m)
    if kind == "huber":
        return k / np.maximum(m, k)
    q = m / k
    if kind == "cauchy":
        return 1.0 / (1.0 + q * q)
    if kind == "tukey":
        u = 1.0 - q * q
        return np.where(m <= k, u * u, 0.0)
    raise ValueError(kind)


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def combined_covariance(Ct, Cs, R):
    """the six entries (m00, m01, m02, m11, m12, m22) of M = C_t + R C_s R^T, from the upper triangles of Ct and Cs [n,3,3]"""
    S = [[Cs[:, min(a, b), max(a, b)] for b in range(3)] for a in range(3)]
    B = [[(R[a, 0] * S[0][b] + R[a, 1] * S[1][b]) + R[a, 2] * S[2][b] for b in range(3)] for a in range(3)]
    return [Ct[:, a, b] + _dot3(B[a], R[b]) for a in range(3) for b in range(a, 3)]


def cofactor_inverse(m):
    """(W as a 3x3 list of arrays, det) of the symmetric matrix with the entries m = (m00, m01, m02, m11, m12, m22)"""
    m00, m01, m02, m11, m12, m22 = m
    c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
    c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
    det = (m00 * c00 + m01 * c01) + m02 * c02
    with np.errstate(divide="ignore", invalid="ignore"):
        W = [[c00 / det, c01 / det, c02 / det], [c01 / det, c11 / det, c12 / det], [c02 / det, c12 / det, c22 / det]]
    return W, det


def system(source, target, Ct, Cs, R, idx, kind="l2", k=1.0):
    """-> (JTJ [6,6], JTr [6], correspondences summed, correspondences skipped): one round's normal equations.  source: the working
    copy (already moved); Cs: the source's covariances as given; R: the rotation block of the accumulated transformation."""
    s_all = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    ok = idx >= 0
    s = s_all[ok]
    t = np.asarray(target, dtype=np.float64).reshape(-1, 3)[idx[ok]]
    with np.errstate(invalid="ignore", over="ignore"):
        m = combined_covariance(np.asarray(Ct)[idx[ok]], np.asarray(Cs)[ok], np.asarray(R, dtype=np.float64))
        W, det = cofactor_inverse(m)
    good = np.isfinite(np.stack(m, 0)).all(0) & (det > 0)
    skipped = int((~good).sum())
    s, t = s[good], t[good]
    W = [[W[a][b][good] for b in range(3)] for a in range(3)]
    d = [s[:, a] - t[:, a] for a in range(3)]
    sv = [s[:, a] for a in range(3)]
    Wd = [_dot3(W[a], d) for a in range(3)]
    w = weight(kind, np.sqrt(np.maximum(_dot3(d, Wd), 0.0)), k)
    G = [_cross(sv, W[a]) for a in range(3)]
    H = [[None] * 3 for _ in range(3)]
    for b in range(3):
        h = _cross(sv, [G[0][b], G[1][b], G[2][b]])
        for a in range(3):
            H[a][b] = h[a]
    JTJ = np.zeros((6, 6))
    full = [[H[a][b] for b in range(3)] + [G[c][a] for c in range(3)] for a in range(3)] + \
           [[None] * 3 + [W[a][b] for b in range(3)] for a in range(3)]
    for a in range(6):
        for b in range(a, 6):
            term = full[a][b]
            JTJ[a, b] = JTJ[b, a] = np.sum(term if kind == "l2" else w * term)
    rhs = _cross(sv, Wd) + Wd
    JTr = np.array([np.sum(v if kind == "l2" else w * v) for v in rhs])
    return JTJ, JTr, len(s), skipped


def plane_system(source, target, normals, idx, kind, k):
    """icp_restatement.system with the weight w(|r|) on every term"""
    s = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    ok = idx >= 0
    s = s[ok]
    t = np.asarray(target)[idx[ok]]
    n = np.asarray(normals)[idx[ok]]
    dv = s - t
    r = (dv[:, 0] * n[:, 0] + dv[:, 1] * n[:, 1]) + dv[:, 2] * n[:, 2]
    J = np.empty((len(s), 6))
    J[:, :3] = np.stack(_cross([s[:, 0], s[:, 1], s[:, 2]], [n[:, 0], n[:, 1], n[:, 2]]), 1)
    J[:, 3:] = n
    w = weight(kind, np.abs(r), k)
    JTJ = np.array([[np.sum(w * (J[:, min(a, b)] * J[:, max(a, b)])) for b in range(6)] for a in range(6)])
    return JTJ, np.array([np.sum(w * (J[:, a] * r)) for a in range(6)]), len(s)


def gicp(source, target, Ct, Cs, r, init=np.eye(4), relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, kind="l2", k=1.0,
         corr=None):
    """RegistrationGeneralizedICP -> dict(transformation, fitness, inlier_rmse, n_correspondences, iterations); icp_restatement.icp's
    loop with this file's system"""
    corr = corr or (IR.correspondences if len(source) * max(len(target), 1) <= 4e7 else IR.correspondences_grid)
    pcd = CR.transform(source, init)
    T = np.array(init, dtype=np.float64)

    def result(pcd):
        idx, d2 = corr(pcd, target, r)
        n = int((idx >= 0).sum())
        fit = n / len(pcd) if n else 0.0
        rmse = float(np.sqrt(d2[idx >= 0].sum() / n)) if n else 0.0
        return idx, fit, rmse, n

    idx, fit, rmse, n = result(pcd)
    rounds = 0
    for _ in range(max_iteration):
        if n:
            JTJ, JTr, _, skipped = system(pcd, target, Ct, Cs, T[:3, :3], idx, kind, k)
            assert skipped == 0
            U = IR.step_matrix(IR.ldlt_solve(JTJ, -JTr))
        else:
            U = np.eye(4)
        T = IR.matmul4(U, T)
        pcd = CR.transform(pcd, U)
        prev = (fit, rmse)
        idx, fit, rmse, n = result(pcd)
        rounds += 1
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fit, "inlier_rmse": rmse, "n_correspondences": n, "iterations": rounds}
