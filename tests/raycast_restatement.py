"""Plain numpy fp64 restatements of include/loner_hip.h's "ray casting" block, operation by operation: the hit of a ray by brute
force over every triangle with the (t, index) tie rule, the rays of a moving sensor, and the ray sets and analytic distances the
host and the device tests share."""
import functools

import numpy as np

INF = np.inf


# ---------------------------------------------------------------- the hit rule
def cast_rays(vertices, triangles, rays, t_min=0.0, t_max=INF):
    """-> dict(t_hit fp64 [n], primitive_ids int32 [n], primitive_uvs fp64 [n,2], invalid_rays, excluded_triangles, bad_index).
    Every triangle is tested against every ray; a triangle with an index outside [0, V) or a non-finite vertex is left out."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    r = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    n = len(r)
    t_hit = np.full(n, INF)
    ids = np.full(n, -1, dtype=np.int32)
    uvs = np.zeros((n, 2))
    in_range = ((f >= 0) & (f < len(v))).all(axis=1)
    finite = np.zeros(len(f), dtype=bool)
    finite[in_range] = np.isfinite(v[f[in_range]]).all(axis=(1, 2))
    usable = np.nonzero(in_range & finite)[0]
    o, d = r[:, :3], r[:, 3:]
    valid = np.isfinite(r).all(axis=1) & (d != 0).any(axis=1)
    out = dict(t_hit=t_hit, primitive_ids=ids, primitive_uvs=uvs, invalid_rays=int((~valid).sum()),
               excluded_triangles=int((in_range & ~finite).sum()), bad_index=int((~in_range).sum()))
    rows = np.nonzero(valid)[0]
    if len(rows) == 0 or len(usable) == 0:
        return out
    o, d = o[rows], d[rows]
    m = len(rows)
    ar = np.arange(m)
    ad = np.abs(d)
    kz = np.zeros(m, dtype=np.int64)
    kz[ad[:, 1] > ad[:, 0]] = 1
    kz[ad[:, 2] > ad[ar, kz]] = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    swap = d[ar, kz] < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    dz = d[ar, kz]
    sx, sy, sz = d[ar, kx] / dz, d[ar, ky] / dz, 1.0 / dz
    best_t = np.full(m, INF)
    best_id = np.full(m, -1, dtype=np.int64)
    best_uv = np.zeros((m, 2))
    with np.errstate(all="ignore"):
        for t in usable:                                            # ascending index: a later triangle must be strictly nearer
            A, B, C = (v[f[t, k]][None, :] - o for k in range(3))
            akz, bkz, ckz = A[ar, kz], B[ar, kz], C[ar, kz]
            ax, ay = A[ar, kx] - sx * akz, A[ar, ky] - sy * akz
            bx, by = B[ar, kx] - sx * bkz, B[ar, ky] - sy * bkz
            cx, cy = C[ar, kx] - sx * ckz, C[ar, ky] - sy * ckz
            U = cx * by - cy * bx
            V = ax * cy - ay * cx
            W = bx * ay - by * ax
            miss = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
            det = (U + V) + W
            miss |= det == 0
            tt = ((U * (sz * akz) + V * (sz * bkz)) + W * (sz * ckz)) / det
            ok = ~miss & (tt >= t_min) & (tt <= t_max) & (tt < best_t)
            best_t[ok] = tt[ok]
            best_id[ok] = t
            best_uv[ok, 0] = (U / det)[ok]
            best_uv[ok, 1] = (V / det)[ok]
    t_hit[rows] = best_t
    ids[rows] = best_id.astype(np.int32)
    uvs[rows] = best_uv
    return out


# ---------------------------------------------------------------- trajectory rays
def stated_sincos(theta):
    """(sin, cos) of theta >= 0 by the header's stated operations: two-constant reduction by pi / 2, then the nested Taylor forms"""
    theta = float(theta)
    kf = float(np.floor(theta * 0.6366197723675814 + 0.5))
    r = (theta - kf * 1.5707963267948966) - kf * 6.123233995736766e-17
    z = r * r
    ps = pc = 1.0
    for k in range(10, 0, -1):
        ps = 1.0 - (z * ps) / float((2 * k) * (2 * k + 1))
        pc = 1.0 - (z * pc) / float((2 * k - 1) * (2 * k))
    S, C = r * ps, pc
    q = int(kf) % 4
    return (S, C, -S, -C)[q], (C, -S, -C, S)[q]


def trajectory_rays(directions, stamps, times, positions, rotations, rotvecs):
    """lnr_trajectory_rays -> (rays fp64 [n,6], info {rays, outside, nonfinite}).  directions fp32 [3,n]; the pose rule is
    lnr_cloud_trajectory_transform's, expression by expression."""
    d = np.asarray(directions)
    assert d.dtype == np.float32 and d.ndim == 2 and d.shape[0] == 3
    d = d.astype(np.float64)
    tau_all = np.asarray(stamps, dtype=np.float64)
    T, P = np.asarray(times, dtype=np.float64), np.asarray(positions, dtype=np.float64)
    R, Wv = np.asarray(rotations, dtype=np.float64).reshape(-1, 9), np.asarray(rotvecs, dtype=np.float64)
    K, n = len(T), d.shape[1]
    rays = np.full((n, 6), np.nan)
    info = dict(rays=0, outside=0, nonfinite=0)
    for i in range(n):
        x, y, z, tau = d[0, i], d[1, i], d[2, i], tau_all[i]
        if not (np.isfinite([x, y, z]).all() and np.isfinite(tau)):
            info["nonfinite"] += 1
            continue
        if tau < T[0] or tau > T[-1]:
            info["outside"] += 1
            continue
        info["rays"] += 1
        k = min(int(np.searchsorted(T, tau, side="right")) - 1, K - 2)
        alpha = (tau - T[k]) / (T[k + 1] - T[k])
        wx, wy, wz = alpha * Wv[k, 0], alpha * Wv[k, 1], alpha * Wv[k, 2]
        theta = np.sqrt((wx * wx + wy * wy) + wz * wz)
        Rk = R[k]
        if theta < 1e-9:
            Rm = Rk.copy()
        else:
            ax, ay, az = wx / theta, wy / theta, wz / theta
            s, cs = stated_sincos(theta)
            c = 1.0 - cs
            E = [1.0 - c * (ay * ay + az * az), c * ax * ay - s * az, c * ax * az + s * ay,
                 c * ax * ay + s * az, 1.0 - c * (ax * ax + az * az), c * ay * az - s * ax,
                 c * ax * az - s * ay, c * ay * az + s * ax, 1.0 - c * (ax * ax + ay * ay)]
            Rm = np.empty(9)
            for a in range(3):
                for b in range(3):
                    Rm[3 * a + b] = (Rk[3 * a] * E[b] + Rk[3 * a + 1] * E[3 + b]) + Rk[3 * a + 2] * E[6 + b]
        for a in range(3):
            rays[i, a] = P[k, a] + alpha * (P[k + 1, a] - P[k, a])
            rays[i, 3 + a] = (Rm[3 * a] * x + Rm[3 * a + 1] * y) + Rm[3 * a + 2] * z
    return rays, info


# ---------------------------------------------------------------- the box room's rays and distances
ROOM_ORIGINS = ((0.0, 0.0, 2.0), (0.3, -1.7, 0.9), (19.5, 14.0, 5.5))


def lidar_directions(beams=16, azimuths=256, fov_deg=(-22.5, 22.5)):
    """utils/synthetic.lidar_pattern's directions in numpy fp64 [n,3] (not rounded to fp32)"""
    el = np.deg2rad(np.linspace(fov_deg[0], fov_deg[1], beams))
    az = 2 * np.pi * np.arange(azimuths) / azimuths
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    return np.stack([ce * np.cos(az)[None, :], ce * np.sin(az)[None, :], np.broadcast_to(se, (beams, azimuths))], -1).reshape(-1, 3)


def box_targets(lo, hi):
    """Points of the box's surface where a crack would show: the 8 corners, two points on each of the 12 edges, the 6 face centres
    and a point on the diagonal each face's two triangles share (and one on the other diagonal) -> [50,3]"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    c = np.array([[(hi if i >> a & 1 else lo)[a] for a in range(3)] for i in range(8)])
    pts = [p for p in c]
    for i in range(8):
        for a in range(3):
            j = i | (1 << a)
            if j != i:
                pts += [c[i] + 0.25 * (c[j] - c[i]), c[i] + 0.7 * (c[j] - c[i])]
    for a in range(3):
        b, e = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            base = side << a
            p00, p01, p10, p11 = c[base], c[base | 1 << e], c[base | 1 << b], c[base | 1 << b | 1 << e]
            pts += [0.25 * (p00 + p01 + p10 + p11), p00 + 0.3 * (p11 - p00), p01 + 0.3 * (p10 - p01)]
    return np.asarray(pts)


@functools.lru_cache(maxsize=None)
def room_rays(lo, hi):
    """[3 * m, 6]: from each of ROOM_ORIGINS a 16 x 256 LiDAR pattern, rays aimed at box_targets, and the six axis directions"""
    targets = box_targets(lo, hi)
    rays = []
    for o in ROOM_ORIGINS:
        o = np.asarray(o, dtype=np.float64)
        d = np.concatenate([lidar_directions(), targets - o, np.eye(3), -np.eye(3)])
        rays.append(np.concatenate([np.broadcast_to(o, d.shape), d], axis=1))
    out = np.concatenate(rays)
    out.setflags(write=False)
    return out


def slab_distance(rays, lo, hi):
    """The exit parameter of rays that start inside the box [lo, hi]: min over the axes the ray moves along of
    max((lo - o) / d, (hi - o) / d)"""
    r = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    o, d = r[:, :3], r[:, 3:]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.maximum((np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d)
    t = np.where(d == 0, INF, t)
    return t.min(axis=1)
