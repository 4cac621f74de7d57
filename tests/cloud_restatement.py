"""numpy restatement of the point-cloud contract (include/loner_hip.h, "point clouds"): what the reference's open3d calls compute,
written out step by step so that the device results can be compared bit for bit."""
import numpy as np

INT_MAX = 2147483647


def scan_points(depth, variance, ray_index, directions, scale, var_threshold, depth_bound):
    """renderer_lidar.py:83-91 for the kept rays of one pose: depth and variance times the scale in fp32, the two fp32 compares
    (NaN fails them), fp32 direction times depth, widened to fp64, in ray order."""
    depth = np.asarray(depth, dtype=np.float32).reshape(-1)
    variance = np.asarray(variance, dtype=np.float32).reshape(-1)
    d = depth * np.float32(scale)
    v = variance * np.float32(scale)
    good = (v < np.float32(var_threshold)) & (d < np.float32(depth_bound))
    dirs = np.asarray(directions, dtype=np.float32)[:, np.asarray(ray_index)].T
    return (dirs * d[:, None])[good].astype(np.float64)


def voxel_down_sample(points, voxel_size):
    """open3d PointCloud::VoxelDownSample (legacy): voxel = floor((p - (min - v/2)) / v) in fp64, the voxel's points summed in input
    order (np.add.at) and divided by the count; voxels in ascending (i_x, i_y, i_z) order."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = float(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError("voxel_size must be finite and > 0")
    if p.shape[0] == 0:
        return np.zeros((0, 3))
    if not np.isfinite(p).all():
        raise ValueError(f"{int((~np.isfinite(p).all(1)).sum())} non-finite points")
    lo = p.min(0) - v * 0.5
    hi = p.max(0) + v * 0.5
    if v * INT_MAX < (hi - lo).max():
        raise ValueError("voxel_size is too small")
    idx = np.floor((p - lo) / v).astype(np.int64)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))       # stable: input order within a voxel
    key = idx[order]
    head = np.ones(len(order), dtype=bool)
    head[1:] = (key[1:] != key[:-1]).any(1)
    seg = np.cumsum(head) - 1
    sums = np.zeros((int(head.sum()), 3))
    np.add.at(sums, seg, p[order])
    counts = np.bincount(seg).astype(np.float64)
    return sums / counts[:, None]


def transform(points, T):
    """((T_i0 x + T_i1 y) + T_i2 z) + T_i3 in fp64, one rounding per operation."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64)
    out = np.empty_like(p)
    for i in range(3):
        out[:, i] = ((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3]
    return out


def sq_distances(queries, targets, block=512):
    """min over all targets of (dx*dx + dy*dy) + dz*dz in fp64, brute force in blocks of queries; 0 with no target."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(q.shape[0])
    if t.shape[0] == 0:
        return out
    for s in range(0, q.shape[0], block):
        qb = q[s:s + block]
        best = np.full(qb.shape[0], np.inf)
        for u in range(0, t.shape[0], 4096):
            tb = t[u:u + 4096]
            dx = qb[:, None, 0] - tb[None, :, 0]
            dy = qb[:, None, 1] - tb[None, :, 1]
            dz = qb[:, None, 2] - tb[None, :, 2]
            best = np.minimum(best, ((dx * dx + dy * dy) + dz * dz).min(1))
        out[s:s + block] = best
    return out


def statistics(accuracy, completion, f_score_threshold):
    """evaluate_lidar_map.py:58-80 on given distance arrays, quirks included."""
    accuracy = np.asarray(accuracy)
    completion = np.asarray(completion)
    chamfer_distance = accuracy.mean() + completion.mean()
    false_negatives = (completion > f_score_threshold).sum().item()
    false_positives = (accuracy > f_score_threshold).sum().item()
    true_positives = (len(accuracy) - false_positives)
    precision = true_positives / (true_positives + false_positives)
    recall = true_positives / (true_positives + false_negatives)
    f_score = 2 * (precision * recall) / (precision + recall + 1e-8)
    return {"accuracy": accuracy.mean().item(), "completion": completion.mean().item(), "chamfer_distance": chamfer_distance.item(),
            "recall": recall, "precision": precision, "f-score": f_score, "num_points": len(accuracy)}
