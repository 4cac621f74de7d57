"""numpy fp64 restatement of mesh sampling, the statistical outlier filter and the trajectory transform (include/loner_hip.h, "mesh
sampling, outlier filter, trajectory transform"), written out step by step.  The sampling and the neighbour means are restated
operation by operation (the device must give the same bits); the outlier statistics use math.fsum and the trajectory scipy's Slerp and
interp1d, against which the device is held to a rounding bound."""
import math

import numpy as np

from tests import cloud_restatement as CR
from tests import icp_restatement as IR

STREAM_MESH = 0x4D45534800000000       # LNR_STREAM_MESH of loner_amd/csrc/lnr_common.h: "MESH" in the counter's top word
U = 2.0 ** -53


# ---------------------------------------------------------------- Philox4x32-10
def philox4x32_10(counter_lo, counter_hi, key):
    """(x, y, z, w) uint32 arrays: Philox4x32-10 of the 128-bit counter (counter_lo [n] uint64, counter_hi a 64-bit int) under the
    64-bit key, as loner_amd/csrc/lnr_common.h's philox4x32_10."""
    lo = np.asarray(counter_lo, dtype=np.uint64).reshape(-1)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = lo & m32, lo >> np.uint64(32)
    c2 = np.full_like(lo, int(counter_hi) & 0xFFFFFFFF)
    c3 = np.full_like(lo, (int(counter_hi) >> 32) & 0xFFFFFFFF)
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits, exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def u53(hi, lo):
    """(double)(((uint64) hi << 32 | lo) >> 11) * 2^-53"""
    bits = ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(11)
    return bits.astype(np.float64) * U


# ---------------------------------------------------------------- the 64-ary tree
def tree_prefix(a, op=np.add):
    """The inclusive prefix of a under op in the header's order: within a chunk of 64 left to right; across chunks the prefix of the
    chunk totals (formed by the same rule) op the sum within the chunk."""
    a = np.asarray(a)
    n = len(a)
    if n == 0:
        return a.copy()
    chunks = (n + 63) // 64
    pad = np.zeros(chunks * 64, dtype=a.dtype)
    pad[:n] = a
    pad = pad.reshape(chunks, 64)
    within = np.empty_like(pad)
    within[:, 0] = pad[:, 0]
    for j in range(1, 64):
        within[:, j] = op(within[:, j - 1], pad[:, j])
    if chunks == 1:
        return within.reshape(-1)[:n]
    last = np.minimum(63, n - 1 - 64 * np.arange(chunks))           # the short last chunk ends early
    totals = within[np.arange(chunks), last]
    before = tree_prefix(totals, op)
    out = within.copy()
    out[1:] = op(before[:-1, None], within[1:])
    return out.reshape(-1)[:n]


# ---------------------------------------------------------------- mesh sampling
def triangle_areas(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    u = v[t[:, 0]] - v[t[:, 1]]
    w = v[t[:, 0]] - v[t[:, 2]]
    cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def round_half_away(x):
    """for x >= 0: x - trunc(x) is exact, so the compare against 0.5 is"""
    t = np.trunc(x)
    return t + (x - t >= 0.5)


def mesh_bounds(vertices, triangles, n_points):
    """(n_t int64 [F], S): triangle t owns the points n_{t-1} <= i < n_t"""
    cdf = tree_prefix(triangle_areas(vertices, triangles))
    S = cdf[-1]
    if not S > 0:
        return np.zeros(len(cdf), dtype=np.int64), S
    raw = np.minimum(round_half_away((cdf / S) * float(n_points)), float(n_points)).astype(np.int64)
    return tree_prefix(raw, np.maximum), S


def mesh_sample(vertices, triangles, n_points, seed):
    """(points [n,3], owner int32 [n]); a mesh without area gives no points"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0 or n_points == 0:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
    bounds, S = mesh_bounds(v, t, n_points)
    if not S > 0:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
    i = np.arange(n_points, dtype=np.int64)
    owner = np.searchsorted(bounds, i, side="right")                # the first t with n_t > i
    x, y, z, w = philox4x32_10(i.astype(np.uint64), STREAM_MESH, seed)
    r1, r2 = u53(x, y), u53(z, w)
    s = np.sqrt(r1)
    a, b, c = 1.0 - s, s * (1.0 - r2), s * r2
    v0, v1, v2 = v[t[owner, 0]], v[t[owner, 1]], v[t[owner, 2]]
    return (a[:, None] * v0 + b[:, None] * v1) + c[:, None] * v2, owner.astype(np.int32)


def barycentric_weights(n_points, seed):
    """(a, b, c) of points 0..n-1"""
    x, y, z, w = philox4x32_10(np.arange(n_points, dtype=np.uint64), STREAM_MESH, seed)
    r1, r2 = u53(x, y), u53(z, w)
    s = np.sqrt(r1)
    return 1.0 - s, s * (1.0 - r2), s * r2


# ---------------------------------------------------------------- outlier filter
def knn_mean_distance(points, k):
    """avg [n]: sqrt(d2) of the min(k, n) nearest (d2, index) pairs summed in list order from 0.0, divided by their number"""
    _, d2 = IR.knn(points, k)
    m = d2.shape[1]
    s = np.zeros(len(d2))
    for j in range(m):
        s = s + np.sqrt(d2[:, j])
    return s / float(m)


def outlier_stats(avg, std_ratio):
    """(mean, std, threshold) with exactly rounded sums (math.fsum); valid = n"""
    avg = np.asarray(avg, dtype=np.float64)
    n = len(avg)
    pos = avg[avg > 0]
    mean = math.fsum(pos) / n
    if n < 2:
        return mean, math.nan, math.nan
    std = math.sqrt(math.fsum((pos - mean) * (pos - mean)) / (n - 1))
    return mean, std, mean + std_ratio * std


def _block_sum(v):
    """[blocks, 256] -> [blocks]: the xor butterfly of each wave of 64 (offsets 32, 16, ... 1), then the four waves left to right"""
    w = v.reshape(len(v), 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ o]
    return ((w[:, 0, 0] + w[:, 1, 0]) + w[:, 2, 0]) + w[:, 3, 0]


def _device_sum(terms):
    """The header's fixed order: thread j of block b adds its terms 256 b + j, + 256 B, ... in turn from 0.0 (B = min(ceil(n / 256),
    2048)), a block sums its threads, and one workgroup folds the B partials the same way."""
    n = len(terms)
    B = min(max((n + 255) // 256, 1), 2048)
    acc = np.zeros(256 * B)
    for start in range(0, n, 256 * B):
        part = terms[start:start + 256 * B]
        acc[:len(part)] = acc[:len(part)] + part
    partial = _block_sum(acc.reshape(B, 256))
    fold = np.zeros(256)
    for start in range(0, B, 256):
        part = partial[start:start + 256]
        fold[:len(part)] = fold[:len(part)] + part
    return float(_block_sum(fold.reshape(1, 256))[0])


def outlier_stats_device_order(avg, std_ratio):
    """(mean, std, threshold) with the sums in lnr_cloud_outlier_threshold's own order (a term that is not > 0 adds 0.0, which changes
    no bit of a sum of non-negative terms): the device must give these bits"""
    avg = np.asarray(avg, dtype=np.float64)
    n = len(avg)
    pos = avg > 0
    mean = _device_sum(np.where(pos, avg, 0.0)) / float(n)
    d = avg - mean
    with np.errstate(invalid="ignore", divide="ignore"):
        std = float(np.sqrt(np.float64(_device_sum(np.where(pos, d * d, 0.0))) / np.float64(n - 1.0)))
    return mean, std, mean + std_ratio * std


def outlier_mask(avg, std_ratio):
    """the kept mask; asserts that no avg_i lies within n * 2^-53 (relative) of the threshold, where a device sum in another order
    could decide otherwise"""
    avg = np.asarray(avg, dtype=np.float64)
    _, _, thr = outlier_stats(avg, std_ratio)
    if math.isnan(thr):
        return np.zeros(len(avg), dtype=bool)
    band = len(avg) * U * abs(thr)
    assert not (np.abs(avg - thr) <= band).any(), "an avg_i lies within the summation band of the threshold"
    return (avg > 0) & (avg < thr)


# ---------------------------------------------------------------- trajectory transform
def trajectory_transform(points, stamps, tum_rows, min_range):
    """create_lidar_map.py:77-111 with scipy -> dict(points: the kept points in order, index: their input indices, trans: their
    interpolated translations, below, outside)"""
    from scipy.interpolate import interp1d
    from scipy.spatial.transform import Rotation, Slerp
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ts = np.asarray(stamps, dtype=np.float64).reshape(-1)
    rows = np.asarray(tum_rows, dtype=np.float64)
    T = rows[:, 0]
    far = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) > min_range
    inside = (ts >= T[0]) & (ts <= T[-1])
    keep = far & inside
    index = np.nonzero(keep)[0]
    R = Slerp(T, Rotation.from_quat(rows[:, 4:]))(ts[index]).as_matrix()
    trans = interp1d(T, rows[:, 1:4], axis=0)(ts[index])
    out = np.einsum("nab,nb->na", R, p[index]) + trans
    return {"points": out, "index": index, "trans": trans, "below": int((~far).sum()), "outside": int((far & ~inside).sum())}


TRANSFORM_BOUND_ULPS = 256          # test_gpu_cloud_tools.py derives it


def transform_bound(p, trans):
    """per point: TRANSFORM_BOUND_ULPS * 2^-53 * (|p| + |trans|)"""
    return TRANSFORM_BOUND_ULPS * U * (np.linalg.norm(p, axis=-1) + np.linalg.norm(trans, axis=-1))


def max_voxel_population(points, voxel_size):
    """the largest number of points VoxelDownSample averages into one voxel"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    idx = np.floor((p - (p.min(0) - 0.5 * voxel_size)) / voxel_size).astype(np.int64)
    return int(np.unique(idx, axis=0, return_counts=True)[1].max())


def build_lidar_map(scans, tum_rows, voxel_size, min_range):
    """-> (map points, the scans used, the largest |p| + |trans| of a kept point, the voxel populations (per scan max, merged max))"""
    parts, used, scale, pop = [], [], 0.0, 0
    for k, (xyz, stamps) in enumerate(scans):
        r = trajectory_transform(xyz, stamps, tum_rows, min_range)
        if r["outside"] or len(r["index"]) == 0:
            continue
        used.append(k)
        scale = max(scale, float((np.linalg.norm(np.asarray(xyz)[r["index"]], axis=1) + np.linalg.norm(r["trans"], axis=1)).max()))
        pop = max(pop, max_voxel_population(r["points"], voxel_size))
        parts.append(CR.voxel_down_sample(r["points"], voxel_size))
    merged = np.concatenate(parts)
    return CR.voxel_down_sample(merged, voxel_size), used, scale, (pop, max_voxel_population(merged, voxel_size))
