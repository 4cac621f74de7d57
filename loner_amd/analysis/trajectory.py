"""Trajectory scoring: the absolute pose error of an estimated trajectory against ground truth, what the reference asks of
`evo_ape tum <gt> <est> --t_max_diff 0.1 -a` (analysis/compute_metrics/traj/analyze.sh).  Host only, numpy fp64; the definitions below
are the contract.

  associate   every estimate stamp is offered its nearest ground-truth stamp (the earlier one on a tie); offers farther than
              t_max_diff are dropped; the remaining offers are granted in order of increasing distance (then estimate index), and an
              offer for a ground-truth stamp already granted is dropped: no ground-truth stamp is used twice
  umeyama     the least-squares similarity (Umeyama 1991) gt ~ c R est + t through the SVD of the cross-covariance, with the
              reflection fix (the last singular direction is flipped when det(U) det(V) < 0); c = 1 unless with_scale
  ape         per associated pair E = inv(gt) @ est (est aligned first when align): the translation error is |trans(E)| in the
              trajectories' unit, the rotation error the angle of rot(E) in degrees; each summarised as rmse, mean, median, std
              (population), min, max, sse
The relative pose error over a path-length delta (evo_rpe) is not here."""
import numpy as np

from ..common.pose_utils import quat_to_matrix, read_tum

STATS = ("rmse", "mean", "median", "std", "min", "max", "sse")


def associate(est_stamps, gt_stamps, t_max_diff=0.1):
    """-> (est_idx, gt_idx) int64 arrays of equal length, ascending in est_idx"""
    est = np.asarray(est_stamps, dtype=np.float64).reshape(-1)
    gt = np.asarray(gt_stamps, dtype=np.float64).reshape(-1)
    if est.size == 0 or gt.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    order = np.argsort(gt, kind="stable")
    gs = gt[order]
    right = np.clip(np.searchsorted(gs, est), 1, len(gs) - 1) if len(gs) > 1 else np.zeros(len(est), dtype=np.int64)
    left = np.maximum(right - 1, 0)
    nearest = np.where(np.abs(est - gs[left]) <= np.abs(gs[right] - est), left, right)
    diff = np.abs(est - gs[nearest])
    used = np.zeros(len(gs), dtype=bool)
    pairs = []
    for e in np.lexsort((np.arange(len(est)), diff)):
        if diff[e] <= t_max_diff and not used[nearest[e]]:
            used[nearest[e]] = True
            pairs.append((e, order[nearest[e]]))
    pairs.sort()
    return (np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64))


def umeyama_alignment(est_xyz, gt_xyz, with_scale=False):
    """est_xyz, gt_xyz [n,3] -> (R [3,3], t [3], c): gt ~ c R est + t in the least-squares sense; R is a rotation (det +1)"""
    x = np.asarray(est_xyz, dtype=np.float64)
    y = np.asarray(gt_xyz, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 2 or x.shape[1] != 3 or len(x) == 0:
        raise ValueError(f"umeyama_alignment: two [n,3] point sets, got {x.shape} and {y.shape}")
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    cov = yc.T @ xc / len(x)
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    var_x = (xc ** 2).sum() / len(x)
    c = float(np.trace(np.diag(D) @ S) / var_x) if with_scale and var_x > 0 else 1.0
    return R, my - c * R @ mx, c


def _rows(tum):
    rows = read_tum(tum) if isinstance(tum, (str, bytes)) or hasattr(tum, "__fspath__") else np.asarray(tum, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 8:
        raise ValueError(f"ape: TUM rows [n,8] (ts x y z qx qy qz qw), got {rows.shape}")
    return rows


def summary(errors) -> dict:
    e = np.asarray(errors, dtype=np.float64)
    sse = float((e ** 2).sum())
    return {"rmse": float(np.sqrt(sse / len(e))), "mean": float(e.mean()), "median": float(np.median(e)), "std": float(e.std()),
            "min": float(e.min()), "max": float(e.max()), "sse": sse}


def ape(est_tum, gt_tum, align=True, t_max_diff=0.1, with_scale=False) -> dict:
    """est_tum, gt_tum: TUM rows [n,8] or paths -> the translation error's rmse, mean, median, std, min, max, sse, the same for the
    rotation angle under "rotation_deg", and "pairs", the number of associated poses"""
    est, gt = _rows(est_tum), _rows(gt_tum)
    ei, gi = associate(est[:, 0], gt[:, 0], t_max_diff)
    if len(ei) == 0:
        raise ValueError(f"ape: no estimate stamp lies within {t_max_diff} s of a ground-truth stamp")
    p_est, p_gt = est[ei, 1:4], gt[gi, 1:4]
    R_est, R_gt = quat_to_matrix(est[ei, 4:]), quat_to_matrix(gt[gi, 4:])
    if align:
        R, t, c = umeyama_alignment(p_est, p_gt, with_scale)
        p_est = c * p_est @ R.T + t
        R_est = R @ R_est
    E_t = np.einsum("nba,nb->na", R_gt, p_est - p_gt)              # trans(inv(gt) @ est) = R_gt^T (p_est - p_gt)
    E_R = np.einsum("nba,nbc->nac", R_gt, R_est)
    cos = np.clip((np.trace(E_R, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    out = summary(np.linalg.norm(E_t, axis=1))
    out["rotation_deg"] = summary(np.degrees(np.arccos(cos)))
    out["pairs"] = int(len(ei))
    return out
