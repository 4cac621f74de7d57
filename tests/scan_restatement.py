"""CPU restatement of scan ingestion (include/loner_hip.h, "scan ingestion"): torch CPU ops following the four steps of the contract,
with the sort made stable.  No reference code, no GPU."""
import torch

NANOSECONDS, NEGATIVE_START, LOCAL, GLOBAL, CONSTANT, NO_TIMES = 1, 2, 4, 8, 16, 32      # LNR_SCAN_* flag bits


def theta_degrees(xyz):
    """step 1's angle: atan2(y, x) in degrees, plus 360 where negative (fp32)"""
    theta = torch.atan2(xyz[:, 1], xyz[:, 0]).rad2deg()
    theta[theta < 0] += 360
    return theta


def fov_mask(xyz, segments):
    theta = theta_degrees(xyz)
    mask = torch.zeros(xyz.shape[0], dtype=torch.bool)
    for lo, hi in segments:
        mask |= (theta >= lo) & (theta <= hi)
    return mask


def scan_from_points(xyz, point_times, stamp, segments=None, min_range=0.3, recompute_timestamps=False):
    """xyz [N,3] fp32 CPU, point_times [N] (any real dtype) or None, segments None (FOV off) or a list of (lo, hi) degrees
    -> dict(order int64 [M], distances, timestamps fp32 [M], directions fp32 [3,M], flags, theta, dist (both over all N points))"""
    xyz = xyz.float()
    n = xyz.shape[0]
    # 1. FOV
    passed = torch.ones(n, dtype=torch.bool) if segments is None else fov_mask(xyz, segments)
    # 2. range
    dist = xyz.norm(dim=1)
    keep = passed & (dist > min_range)
    kept = torch.nonzero(keep)[:, 0]
    # 3. times, on the kept points in input order
    flags = 0
    full = lambda: torch.full((len(kept),), stamp, dtype=torch.float64).float()
    if point_times is None:
        flags = NO_TIMES | CONSTANT
        t = full()
    else:
        if recompute_timestamps:
            t = ((torch.arange(n) % 2048) * 1.0 / 2048 * 0.1)[kept]
        else:
            t = point_times.float()[kept]
        if len(kept):
            if t.abs().max() > 1e7:
                flags |= NANOSECONDS
                t = t * 1e-9
            if t[0] < -0.001:
                flags |= NEGATIVE_START
                t = t - t[0].clone()
            if t[0] < 1e-2:
                flags |= LOCAL
                t = t + stamp
            else:
                flags |= GLOBAL
                t = t - t[0] + stamp
            if t[-1] - t[0] < 1e-3:
                flags |= CONSTANT
                t = full()
    assert t.dtype == torch.float32
    # 4. order
    t_sorted, perm = torch.sort(t, stable=True)
    order = kept[perm]
    d = dist[order]
    return dict(order=order, distances=d, timestamps=t_sorted, directions=(xyz[order] / d[:, None]).T.contiguous(), flags=flags,
                theta=theta_degrees(xyz), dist=dist)


def ulp_distance(a, b):
    """the number of fp32 values between a and b, elementwise (finite, same sign)"""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()
