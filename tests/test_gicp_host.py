"""Generalized ICP and the robust kernels on the CPU: the restatement (tests/gicp_restatement.py) against what it must reduce to -
Kabsch with identity covariances, point to plane in the small-epsilon limit, numpy's inverse, the weight formulas - and the argument
errors of RobustKernel, the tracker's two settings and the entry points, which need no device."""
import ctypes
import pickle

import numpy as np
import pytest

from tests import gicp_restatement as GR
from tests import icp_restatement as IR

U = 2.0 ** -53


def test_identity_covariances_converge_to_kabsch():
    """C_s = C_t = I gives W = I / 2 for every pair: the steps minimise sum |T s - t|^2, whose minimum over rigid T is Kabsch's"""
    from loner_amd.analysis.trajectory import umeyama_alignment
    from tests import cloud_restatement as CR
    rng = np.random.default_rng(11)
    s = rng.uniform(-2, 2, size=(300, 3))
    T = IR.rigid(3.0, [0.05, -0.03, 0.02])
    t = s @ T[:3, :3].T + T[:3, 3] + rng.normal(size=s.shape) * 0.01
    eye = np.tile(np.eye(3), (len(s), 1, 1))
    idx = np.arange(len(s))
    acc, pcd = np.eye(4), s.copy()
    for _ in range(12):
        JTJ, JTr, n, skipped = GR.system(pcd, t, eye, eye, acc[:3, :3], idx)
        assert (n, skipped) == (len(s), 0)
        step = IR.step_matrix(IR.ldlt_solve(JTJ, -JTr))
        acc = IR.matmul4(step, acc)
        pcd = CR.transform(pcd, step)
    R, shift, _ = umeyama_alignment(s, t)
    err = max(np.abs(acc[:3, :3] - R).max(), np.abs(acc[:3, 3] - shift).max())
    print(f"max |T - Kabsch| = {err:.3g}")
    assert err <= 1e-9


def test_small_epsilon_limit_is_point_to_plane():
    """C_s = 0 and the plane C_t: M = I - (1 - e) n n^T, so W = (n n^T + e P) / e with P = I - n n^T, and the system is
    (A + e E) x = -(b + e f) / 1 with A, b point to plane's and E = sum J^T P J, f = sum J^T P d.  To first order in e
    x - x_plane = -e A^-1 (f + E x_plane), bounded by e |A^-1| (|f| + |E| |x_plane|); twice that covers the higher orders while
    e |A^-1| |E| < 1/2 (asserted).  The cofactor inverse adds rounding: det = e comes out of about 16 roundings of terms of size
    <= 1, a relative error of at most 16 u / e in W, one factor per correspondence, which moves x by at most
    (16 u / e) |A^-1| sum |J_i| (|r_i| + |J_i| |x_plane|)."""
    eps = 1e-9
    rng = np.random.default_rng(12)
    t = rng.uniform(-2, 2, size=(400, 3))
    n = rng.normal(size=t.shape)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    s = t + rng.normal(size=t.shape) * 0.02
    idx = np.arange(len(s))
    A, b, _ = IR.system(s, t, n, idx)
    x_plane = IR.ldlt_solve(A, -b)
    Ct = GR.plane_covariances(n, eps)
    JTJ, JTr, cnt, skipped = GR.system(s, t, Ct, np.zeros_like(Ct), np.eye(3), idx)
    assert (cnt, skipped) == (len(s), 0)
    x = IR.ldlt_solve(JTJ, -JTr)
    d = s - t
    J = np.concatenate([np.cross(s, n), n], 1)
    r = (d * n).sum(1)
    sx = np.zeros((len(s), 3, 3))
    sx[:, 0, 1], sx[:, 0, 2], sx[:, 1, 0], sx[:, 1, 2], sx[:, 2, 0], sx[:, 2, 1] = -s[:, 2], s[:, 1], s[:, 2], -s[:, 0], -s[:, 1], s[:, 0]
    J3 = np.concatenate([-sx, np.tile(np.eye(3), (len(s), 1, 1))], 2)                       # [-[s]x | I]
    P = np.eye(3) - n[:, :, None] * n[:, None, :]
    E = np.einsum("nai,nab,nbj->ij", J3, P, J3)
    f = np.einsum("nai,nab,nb->i", J3, P, d)
    inv = np.linalg.norm(np.linalg.inv(A), 2)
    assert eps * inv * np.linalg.norm(E, 2) < 0.5
    first_order = 2 * eps * inv * (np.linalg.norm(f) + np.linalg.norm(E, 2) * np.linalg.norm(x_plane))
    jn = np.linalg.norm(J, axis=1)
    rounding = (16 * U / eps) * inv * float((jn * (np.abs(r) + jn * np.linalg.norm(x_plane))).sum())
    err = np.abs(x - x_plane).max()
    print(f"|x - x_plane| = {err:.3g}; first order {first_order:.3g}, rounding {rounding:.3g}; |x| = {np.abs(x_plane).max():.3g}")
    assert err <= first_order + rounding
    assert first_order + rounding < 1e-3 * np.abs(x_plane).max()           # the bound says something


def test_cofactor_inverse_matches_numpy():
    rng = np.random.default_rng(13)
    Q = np.linalg.qr(rng.normal(size=(2000, 3, 3)))[0]
    lam = rng.uniform(0.1, 1.0, size=(2000, 3))                           # condition number <= 10
    M = np.einsum("nab,nb,ncb->nac", Q, lam, Q)
    M = (M + M.transpose(0, 2, 1)) / 2
    W, det = GR.cofactor_inverse([M[:, a, b] for a in range(3) for b in range(a, 3)])
    got = np.stack([np.stack(row, -1) for row in W], -2)
    want = np.linalg.inv(M)
    rel = np.abs(got - want).max((1, 2)) / np.abs(want).max((1, 2))
    print(f"max relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-12 and (det > 0).all()
    # a singular and a non-finite matrix are what the round skips
    _, det = GR.cofactor_inverse([np.array([0.0, np.nan])] * 6)
    assert not (det[0] > 0) and not (det[1] > 0)


def test_plane_rule():
    rng = np.random.default_rng(14)
    n = rng.normal(size=(1000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:3] = np.eye(3)
    eps = 1e-3
    C = GR.plane_covariances(n, eps)
    assert np.array_equal(C, GR.plane_covariances(-n, eps)) and np.array_equal(C, C.transpose(0, 2, 1))
    w = np.linalg.eigvalsh(C)
    assert np.abs(w - [eps, 1.0, 1.0]).max() < 1e-12
    assert np.abs(np.einsum("nab,nb->na", C, n) - eps * n).max() < 1e-12
    assert np.array_equal(C[2], np.diag([1.0, 1.0, 1.0 - (1.0 - eps)]))
    assert not np.isfinite(GR.plane_covariances([[np.nan, 0.0, 1.0]], eps)).all()


@pytest.mark.parametrize("k", [1.0, 0.3])
def test_weights_equal_their_formulas(k):
    m = np.array([0.0, k, 2 * k])
    assert np.array_equal(GR.weight("l2", m, k), [1.0, 1.0, 1.0])
    assert np.array_equal(GR.weight("huber", m, k), [1.0, 1.0, k / (2 * k)])
    assert np.array_equal(GR.weight("cauchy", m, k), [1.0, 0.5, 1.0 / (1.0 + 4.0)])
    assert np.array_equal(GR.weight("tukey", m, k), [1.0, 0.0, 0.0])
    assert GR.weight("tukey", np.array([0.5 * k]), k)[0] == (1 - 0.25) ** 2
    beyond = GR.weight("tukey", k * (1 + np.logspace(-15, 3, 50)), k)
    assert np.array_equal(beyond, np.zeros(50))                           # exactly 0 beyond k


def test_robust_kernel_argument_errors():
    from loner_amd.analysis.registration import RobustKernel
    assert (RobustKernel().kind, RobustKernel().code) == ("l2", 0)
    assert [RobustKernel(kind, 2.0).code for kind in GR.KINDS] == [0, 1, 2, 3]
    assert RobustKernel("Tukey", 3).kind == "tukey" and RobustKernel("l2", 0.0).k == 0.0
    for kind, k in (("welsch", 1.0), ("huber", 0.0), ("cauchy", -1.0), ("tukey", float("nan")), ("huber", float("inf"))):
        with pytest.raises(ValueError):
            RobustKernel(kind, k)


def _tracking_settings(**icp):
    from loner_amd.common.settings import default_tracking_settings
    s = default_tracking_settings()
    s["tracker"]["icp"].update(icp)
    return s


def test_tracker_settings_and_their_errors():
    from loner_amd.common.signals import Signal
    from loner_amd.tracking.tracker import Tracker
    plain = Tracker(_tracking_settings(), Signal(), Signal(), Signal())
    assert plain._estimation == "POINT_TO_PLANE" and plain._robust_kernel is None
    t = Tracker(_tracking_settings(estimation="GENERALIZED", robust_kernel={"type": "TUKEY", "k": 3.0}), Signal(), Signal(), Signal())
    assert t._estimation == "GENERALIZED" and (t._robust_kernel.kind, t._robust_kernel.k) == ("tukey", 3.0)
    back = pickle.loads(pickle.dumps(t))
    assert back._estimation == "GENERALIZED" and back._robust_kernel.kind == "tukey"
    for bad in (dict(estimation="POINT_TO_POINT"), dict(estimation=None), dict(robust_kernel={"type": "WELSCH", "k": 1.0}),
                dict(robust_kernel={"type": "HUBER", "k": 0.0}), dict(robust_kernel={"k": 1.0})):
        with pytest.raises(ValueError):
            Tracker(_tracking_settings(**bad), Signal(), Signal(), Signal())


def test_entry_points_refuse_a_bad_kernel_before_a_launch():
    """kernel and kernel_k are checked first, so null pointers never reach a launch"""
    import __graft_entry__ as ge
    ge.build()
    from loner_amd import hip
    lib = hip.load()
    init = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    for kernel, k in ((1, 0.0), (2, -1.0), (3, float("nan")), (1, float("inf")), (4, 1.0), (-1, 1.0)):
        rc = lib.lnr_icp_generalized(None, 0, None, None, None, 0, 0.5, init, 1e-6, 1e-6, 1, kernel, k, None, 0, None, None, None)
        assert rc != 0 and b"kernel" in lib.lnr_last_error()
        rc = lib.lnr_icp_point_to_plane_robust(None, 0, None, None, 0, 0.5, init, 1e-6, 1e-6, 1, kernel, k, None, 0, None, None, None)
        assert rc != 0 and b"kernel" in lib.lnr_last_error()
    assert lib.lnr_cloud_plane_covariances(None, 0, 0.0, None, None) != 0 and b"epsilon" in lib.lnr_last_error()
    assert lib.lnr_cloud_plane_covariances(None, 0, 1e-3, None, None) == 0
