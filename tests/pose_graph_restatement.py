"""numpy fp64 restatement of the pose graph (include/loner_hip.h, "pose graph"), written from the header's definitions and not from
the kernels: the information matrix of a registered pair by brute force, the residual, its analytic Jacobians through the generators
(dE = A G_c B as dense 4x4 products), the dense linear system, the Levenberg-Marquardt schedule with numpy.linalg.solve, the line
process and the pruning of global_optimization, and the scenes the host and GPU tests share."""
import numpy as np

EPS = 2.0 ** -52


# ---------------------------------------------------------------- information matrix
def transform_points(T, p):
    """((T0 x + T1 y) + T2 z) + T3 per row, as lnr_cloud_append_transformed rounds"""
    T, p = np.asarray(T, dtype=np.float64), np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], axis=1)


def correspondences(source, target, T, r):
    """index [n] (-1 for none) by lnr_icp_correspondences' rule: the smallest (d2, index) with d2 < r r, d2 = (dx dx + dy dy) + dz dz"""
    s = transform_points(T, source)
    t = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    index = np.full(len(s), -1, dtype=np.int64)
    if len(t) == 0:
        return index
    for i, q in enumerate(s):
        if not np.isfinite(q).all():
            continue
        d = q - t
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        j = int(np.argmin(d2))                              # the first of equal minima: the lower index
        if d2[j] < r * r:
            index[i] = j
    return index


def information_matrix(source, target, T, r):
    """-> (6x6, correspondences, non-finite source points, bound 6x6): the sum of G^T G over the correspondences, G = [-[q]x | I].
    Every term is formed as the header states it, ((G0a G0b + G1a G1b) + G2a G2b), so it carries the device's bits; only the order of
    the n additions differs, and n additions lose at most n 2^-52 times the sum of the absolute terms (to first order; the bound).
    With n <= 1 there is no addition to reorder: the bound is 0 and the result is the device's bit for bit."""
    index = correspondences(source, target, T, r)
    hit = index >= 0
    q = np.asarray(target, dtype=np.float64).reshape(-1, 3)[index[hit]]
    n = len(q)
    G = np.zeros((n, 3, 6))
    G[:, 0, 1], G[:, 0, 2] = q[:, 2], -q[:, 1]
    G[:, 1, 0], G[:, 1, 2] = -q[:, 2], q[:, 0]
    G[:, 2, 0], G[:, 2, 1] = q[:, 1], -q[:, 0]
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    M, A = np.zeros((6, 6)), np.zeros((6, 6))
    for a in range(6):
        for b in range(a, 6):
            term = (G[:, 0, a] * G[:, 0, b] + G[:, 1, a] * G[:, 1, b]) + G[:, 2, a] * G[:, 2, b]
            M[a, b] = M[b, a] = float(term.sum()) if n else 0.0
            A[a, b] = A[b, a] = float(np.abs(term).sum()) if n else 0.0
    bad = int((~np.isfinite(transform_points(T, source)).all(axis=1)).sum())
    return M, n, bad, (n if n > 1 else 0) * EPS * A


# ---------------------------------------------------------------- the model
def step_matrix(x):
    """TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), t = x[3:6]"""
    ca, sa, cb, sb, cc, sc = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, x[3]],
                     [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def rigid_inverse(T):
    O = np.eye(4)
    O[:3, :3] = T[:3, :3].T
    O[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return O


def vee(E):
    return np.array([(E[2, 1] - E[1, 2]) / 2.0, (E[0, 2] - E[2, 0]) / 2.0, (E[1, 0] - E[0, 1]) / 2.0, E[0, 3], E[1, 3], E[2, 3]])


def residual(Ts, Tt, X):
    return vee(rigid_inverse(X) @ rigid_inverse(Tt) @ Ts)


def generators():
    G = np.zeros((6, 4, 4))
    G[0, 1, 2], G[0, 2, 1] = -1.0, 1.0
    G[1, 0, 2], G[1, 2, 0] = 1.0, -1.0
    G[2, 0, 1], G[2, 1, 0] = -1.0, 1.0
    G[3, 0, 3] = G[4, 1, 3] = G[5, 2, 3] = 1.0
    return G


def jacobians(Ts, Tt, X):
    """(J_s, J_t) at 0: column c of J_s is vee(A G_c B), of J_t vee(-A G_c B)"""
    A, B = rigid_inverse(X) @ rigid_inverse(Tt), Ts
    Js = np.stack([vee(A @ G @ B) for G in generators()], axis=1)
    return Js, -Js


class Graph:
    """source, target int [m]; X [m,4,4]; L [m,6,6]; uncertain bool [m]; poses [n,4,4] (the initial ones)"""

    def __init__(self, poses, source, target, X, L, uncertain, truth=None):
        self.poses = np.asarray(poses, dtype=np.float64)
        self.source, self.target = np.asarray(source, dtype=np.int64), np.asarray(target, dtype=np.int64)
        self.X, self.L = np.asarray(X, dtype=np.float64).reshape(-1, 4, 4), np.asarray(L, dtype=np.float64).reshape(-1, 6, 6)
        self.uncertain = np.asarray(uncertain, dtype=bool).reshape(-1)
        self.truth = truth
        self.n, self.m = len(self.poses), len(self.source)

    def subset(self, keep):
        keep = np.asarray(keep, dtype=bool)
        return Graph(self.poses, self.source[keep], self.target[keep], self.X[keep], self.L[keep], self.uncertain[keep], self.truth)


def linearize(g, poses, line, reference=-1):
    """-> dict: e [m,6], q [m], W [m,6,6], g [m,6], H (dense [6n,6n], the reference node's rows and columns zero but for its identity
    block), H_diag [n,6,6], b [n,6], and mag_* : the sums of absolute terms each of those is made of (for the tests' bounds)"""
    n, m = g.n, g.m
    w = np.where(g.uncertain, line, 1.0)
    e, q, W, gg = np.zeros((m, 6)), np.zeros(m), np.zeros((m, 6, 6)), np.zeros((m, 6))
    magW, magg, mage, magq = np.zeros((m, 6, 6)), np.zeros((m, 6)), np.zeros((m, 6)), np.zeros(m)
    H, b = np.zeros((6 * n, 6 * n)), np.zeros((n, 6))
    magH, magb = np.zeros((n, 6, 6)), np.zeros((n, 6))
    for k in range(m):
        s, t = g.source[k], g.target[k]
        J, _ = jacobians(poses[s], poses[t], g.X[k])
        e[k] = residual(poses[s], poses[t], g.X[k])
        Le = g.L[k] @ e[k]
        q[k] = e[k] @ Le
        W[k] = J.T @ g.L[k] @ J
        gg[k] = J.T @ Le
        A = np.abs(rigid_inverse(g.X[k])) @ np.abs(rigid_inverse(poses[t])) @ np.abs(poses[s])
        mage[k] = np.array([A[2, 1] + A[1, 2], A[0, 2] + A[2, 0], A[1, 0] + A[0, 1], A[0, 3], A[1, 3], A[2, 3]])
        aL = np.abs(g.L[k])
        aJ = np.stack([vee_abs(np.abs(rigid_inverse(g.X[k])) @ np.abs(rigid_inverse(poses[t])) @ np.abs(G) @ np.abs(poses[s]))
                       for G in generators()], axis=1)
        magq[k] = mage[k] @ aL @ mage[k]
        magW[k] = aJ.T @ aL @ aJ
        magg[k] = aJ.T @ aL @ mage[k]
        for i, sign in ((s, 1.0), (t, -1.0)):
            if i == reference:
                continue
            H[6 * i:6 * i + 6, 6 * i:6 * i + 6] += w[k] * W[k]
            b[i] -= sign * w[k] * gg[k]
            magH[i] += w[k] * magW[k]
            magb[i] += w[k] * magg[k]
        if s != reference and t != reference:
            H[6 * s:6 * s + 6, 6 * t:6 * t + 6] -= w[k] * W[k]
            H[6 * t:6 * t + 6, 6 * s:6 * s + 6] -= w[k] * W[k].T
    if reference >= 0:
        H[6 * reference:6 * reference + 6, 6 * reference:6 * reference + 6] = np.eye(6)
    Hd = np.stack([H[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n)])
    return {"e": e, "q": q, "W": W, "g": gg, "H": H, "H_diag": Hd, "b": b, "mag_e": mage, "mag_q": magq, "mag_W": magW, "mag_g": magg,
            "mag_H": magH, "mag_b": magb}


def vee_abs(E):
    return np.array([(E[2, 1] + E[1, 2]) / 2.0, (E[0, 2] + E[2, 0]) / 2.0, (E[1, 0] + E[0, 1]) / 2.0, E[0, 3], E[1, 3], E[2, 3]])


def objective(g, poses, line, mu):
    q = np.array([residual(poses[g.source[k]], poses[g.target[k]], g.X[k]) @ g.L[k] @ residual(poses[g.source[k]], poses[g.target[k]], g.X[k])
                  for k in range(g.m)])
    return float(np.sum(np.where(g.uncertain, line * q + mu * (np.sqrt(line) - 1.0) ** 2, q))), q


def loop_mu(g, max_correspondence_distance, preference_loop_closure):
    if not g.uncertain.any():
        return 0.0
    return preference_loop_closure * max_correspondence_distance ** 2 * float(np.mean(g.L[g.uncertain, 5, 5]))


def optimize(g, max_correspondence_distance, preference_loop_closure=1.0, reference=-1, max_iteration=100, max_iteration_lm=20,
             min_relative_increment=1e-6, min_right_term=1e-6, min_residual=1e-6):
    """The header's Levenberg-Marquardt schedule with a dense direct solve -> dict: poses, line, history (1 accepted, 0 rejected,
    -1 the relative-increment stop), rhos, F, b_inf, lambda0, H0 (the first dense system), reason"""
    poses, line = g.poses.copy(), np.ones(g.m)
    mu = loop_mu(g, max_correspondence_distance, preference_loop_closure)
    lin = linearize(g, poses, line, reference)
    F, _ = objective(g, poses, line, mu)
    lam0 = lam = 1e-5 * float(np.max(np.diag(lin["H"]))) if g.n else 0.0
    nu, history, rhos, accepts, consecutive = 2.0, [], [], 0, 0
    b_inf = float(np.abs(lin["b"]).max())
    reason = "min_right_term" if b_inf < min_right_term else ("max_iteration" if accepts >= max_iteration else None)
    H0 = lin["H"].copy()
    trials = 0
    while reason is None and trials < max_iteration * (max_iteration_lm + 1):
        trials += 1
        delta = np.linalg.solve(lin["H"] + lam * np.eye(6 * g.n), lin["b"].reshape(-1)).reshape(g.n, 6)
        if np.linalg.norm(delta) <= min_relative_increment * (np.linalg.norm(poses[:, :3, 3]) + min_relative_increment):
            history.append(-1)
            reason = "min_relative_increment"
            break
        trial = np.stack([step_matrix(delta[i]) @ poses[i] for i in range(g.n)])
        F_new, q_new = objective(g, trial, line, mu)
        rho = (F - F_new) / float(np.sum(delta * (lam * delta + lin["b"])))
        rhos.append(rho)
        if rho > 0:
            history.append(1)
            lam, nu, accepts, consecutive = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 2.0, accepts + 1, 0
            poses = trial
            line = np.where(g.uncertain, (mu / (mu + q_new)) ** 2 if mu > 0 else 1.0, line)      # mu = 0: no line process
            lin = linearize(g, poses, line, reference)
            F, _ = objective(g, poses, line, mu)
            b_inf = float(np.abs(lin["b"]).max())
            if b_inf < min_right_term:
                reason = "min_right_term"
            elif F < min_residual:
                reason = "min_residual"
            elif accepts >= max_iteration:
                reason = "max_iteration"
        else:
            history.append(0)
            lam, nu, consecutive = lam * nu, nu * 2.0, consecutive + 1
            if consecutive >= max_iteration_lm:
                reason = "max_iteration_lm"
    return {"poses": poses, "line": line, "history": history, "rhos": rhos, "F": F, "b_inf": b_inf, "lambda0": lam0, "H0": H0,
            "reason": reason or "trials ran out", "mu": mu}


def global_optimization(g, max_correspondence_distance, edge_prune_threshold=0.25, **kw):
    """optimise, drop the uncertain edges with l < threshold, optimise again -> (first, second, pruned edge indices)"""
    first = optimize(g, max_correspondence_distance, **kw)
    keep = ~(g.uncertain & (first["line"] < edge_prune_threshold))
    g2 = g.subset(keep)
    g2.poses = first["poses"]
    second = optimize(g2, max_correspondence_distance, **kw)
    return first, second, np.nonzero(~keep)[0].tolist()


# ---------------------------------------------------------------- scenes
def _spd(rng, m, lo=0.5, hi=2.0):
    out = np.zeros((m, 6, 6))
    for k in range(m):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        out[k] = Q @ np.diag(rng.uniform(lo, hi, 6)) @ Q.T
        out[k] = (out[k] + out[k].T) / 2.0
    return out


def ring_truth(n, radius=None):
    """n poses on a circle, each turned to face along it, with a wobble in height and tilt"""
    radius = max(2.0, n / 6.0) if radius is None else radius
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / max(n, 1)
        out.append(step_matrix([0.1 * np.sin(3 * a), 0.1 * np.cos(2 * a), a, radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(2 * a)]))
    return np.stack(out)


def measure(truth, s, t):
    return rigid_inverse(truth[t]) @ truth[s]


def perturbed(truth, rng, rot, trans, keep=()):
    out = truth.copy()
    for i in range(len(truth)):
        if i not in keep:
            out[i] = step_matrix(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)])) @ truth[i]
    return out


def ring_graph(n, seed=0, chords=True, rot=0.02, trans=0.05, flip_first=False, duplicate_first=False):
    """A ring of n nodes: edges i -> i + 1 (certain, the last one closing the ring), with chords i -> i + n // 3 (uncertain) from every
    fourth node when asked; exact measurements of the ground truth, perturbed initial poses (node 0 kept).  flip_first: the first
    edge runs from the higher node to the lower one; duplicate_first: it appears twice."""
    rng = np.random.default_rng(seed)
    truth = ring_truth(n)
    pairs = [(i, (i + 1) % n, False) for i in range(n)] if n > 2 else ([(0, 1, False)] if n == 2 else [])
    if chords and n >= 8:
        pairs += [(i, (i + n // 3) % n, True) for i in range(0, n, 4)]
    if flip_first and pairs:
        pairs[0] = (pairs[0][1], pairs[0][0], pairs[0][2])
    if duplicate_first and pairs:
        pairs.append(pairs[0])
    s, t, u = (np.array([p[k] for p in pairs]) for k in range(3)) if pairs else (np.zeros(0, dtype=np.int64),) * 3
    X = np.stack([measure(truth, a, b) for a, b, _ in pairs]) if pairs else np.zeros((0, 4, 4))
    return Graph(perturbed(truth, rng, rot, trans, keep=(0,)), s, t, X, _spd(rng, len(pairs)), u, truth)


def star_graph(degree=130, seed=1):
    """A hub (node 0) with `degree` leaves, every leaf joined to the hub (alternating direction); every third edge uncertain"""
    rng = np.random.default_rng(seed)
    n = degree + 1
    truth = ring_truth(n, 4.0)
    pairs = [((0, i) if i % 2 else (i, 0)) + (i % 3 == 0,) for i in range(1, n)]
    s, t, u = (np.array([p[k] for p in pairs]) for k in range(3))
    X = np.stack([measure(truth, a, b) for a, b, _ in pairs])
    return Graph(perturbed(truth, rng, 0.02, 0.05, keep=(0,)), s, t, X, _spd(rng, len(pairs)), u, truth)


NOISY = {"n": 24, "sigma_rot": 0.002, "sigma_trans": 0.003, "max_correspondence_distance": 0.1}


def noisy_graph(seed=5):
    """A ring of 24 nodes with noisy odometry, eight true loop closures (uncertain, noisy) and three false ones (uncertain, their
    measurement wrong by about half a metre and a quarter radian); the initial poses are the odometry chain from node 0"""
    rng = np.random.default_rng(seed)
    n = NOISY["n"]
    truth = ring_truth(n)
    noise = lambda: step_matrix(np.concatenate([rng.normal(0, NOISY["sigma_rot"], 3), rng.normal(0, NOISY["sigma_trans"], 3)]))   # noqa: E731
    pairs = [(i, i + 1, False) for i in range(n - 1)] + [(i, (i + 9) % n, True) for i in range(0, n, 3)]
    X = [noise() @ measure(truth, a, b) for a, b, _ in pairs]
    false = [(2, 13), (20, 7), (5, 17)]
    for a, b in false:
        wrong = step_matrix(np.concatenate([rng.choice([-1, 1], 3) * rng.uniform(0.15, 0.3, 3), rng.choice([-1, 1], 3) * rng.uniform(0.3, 0.6, 3)]))
        pairs.append((a, b, True))
        X.append(wrong @ measure(truth, a, b))
    s, t, u = (np.array([p[k] for p in pairs]) for k in range(3))
    poses = [truth[0]]
    for k in range(n - 1):                                  # X_k takes frame k to frame k + 1: T_(k+1) = T_k X_k^-1
        poses.append(poses[-1] @ rigid_inverse(X[k]))
    g = Graph(np.stack(poses), s, t, np.stack(X), _spd(rng, len(pairs)), u, truth)
    g.false_edges = list(range(len(pairs) - len(false), len(pairs)))
    return g


def cloud_pair(n_source, seed=0, shift=0.0):
    """-> (source [n_source,3], target [1500,3], T 4x4, r): the target on three walls of a room corner, the source a noisy subset of
    it moved by inv(T); shift moves the whole scene along x"""
    rng = np.random.default_rng(seed)
    nt = 1500
    t = rng.uniform(0.0, 4.0, (nt, 3))
    t[np.arange(nt), rng.integers(0, 3, nt)] = 0.0
    t[:, 0] += shift
    T = step_matrix([0.02, -0.03, 0.05, 0.1, -0.05, 0.08])
    T[:3, 3] += shift - T[:3, :3] @ np.array([shift, 0.0, 0.0])        # T keeps the shifted scene on itself up to the small motion
    pick = rng.integers(0, nt, n_source)
    moved = t[pick] + rng.normal(0, 0.01, (n_source, 3))
    src = (moved - T[:3, 3]) @ T[:3, :3]                                # inv(T) applied
    return src, t, T, 0.08
