"""A numpy / plain-float restatement of TSDF fusion, written from include/loner_hip.h ("TSDF fusion" and the masked marching cubes),
not from the kernels: the integration ray by ray in Python floats (IEEE fp64, every operation rounded on its own), the field, and the
masked marching cubes built on mesh_restatement.marching_cubes and the library's case table."""
import math

import numpy as np

from tests import mesh_restatement as MR

ONE = 1048576.0


def walk(o, d, r, dims, origin, v, trunc, front):
    """One ray -> ("invalid" | "miss" | "ok", [(i, j, k), ...]): the voxels the header's walk visits, in order."""
    o, d, r = [float(x) for x in o], [float(x) for x in d], float(r)
    if not all(math.isfinite(x) for x in o + d) or not any(x != 0.0 for x in d) or not math.isfinite(r) or r <= 0.0:
        return "invalid", []
    go = [(o[a] - origin[a]) / v + 0.5 for a in range(3)]
    gd = [d[a] / v for a in range(3)]
    if not all(math.isfinite(x) for x in go + gd):
        return "invalid", []
    t0, t1 = max(0.0, r - front), r + trunc
    for a in range(3):
        if gd[a] == 0.0:
            if not 0.0 <= go[a] < float(dims[a]):
                return "miss", []
        else:
            ta, tb = (0.0 - go[a]) / gd[a], (float(dims[a]) - go[a]) / gd[a]
            t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    if not t0 < t1:
        return "miss", []
    c, step, t_max, t_delta = [], [], [], []
    for a in range(3):
        e = math.floor(go[a] + t0 * gd[a])
        c.append(min(max(e, 0), dims[a] - 1))
        if gd[a] == 0.0:
            step.append(0); t_max.append(math.inf); t_delta.append(math.inf)
        else:
            step.append(1 if gd[a] > 0.0 else -1)
            t_max.append((float(c[a] + (1 if gd[a] > 0.0 else 0)) - go[a]) / gd[a])
            t_delta.append(1.0 / abs(gd[a]))
    out = []
    while True:
        out.append(tuple(c))
        a = 0 if (t_max[0] <= t_max[1] and t_max[0] <= t_max[2]) else (1 if t_max[1] <= t_max[2] else 2)
        if not t_max[a] < t1:
            break
        nxt = c[a] + step[a]
        if nxt < 0 or nxt >= dims[a]:
            break
        c[a] = nxt
        t_max[a] += t_delta[a]
    return "ok", out


def integrate(rays, ranges, dims, origin, v, trunc, front, sum_=None, count=None):
    """-> (sum int64 [nx,ny,nz], count uint32 [nx,ny,nz], info [8]): the arrays after the rays were added (to sum_ / count if given)."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1)
    origin, v, trunc, front = [float(x) for x in origin], float(v), float(trunc), float(front)
    sum_ = np.zeros(dims, dtype=np.int64) if sum_ is None else sum_
    count = np.zeros(dims, dtype=np.uint32) if count is None else count
    info = [0] * 8
    for ray, r in zip(rays.tolist(), ranges.tolist()):
        o, d = ray[:3], ray[3:]
        state, voxels = walk(o, d, r, dims, origin, v, trunc, front)
        if state == "invalid":
            info[2] += 1
            continue
        if state == "miss":
            info[3] += 1
            continue
        wrote = 0
        for c in voxels:
            p = [origin[a] + float(c[a]) * v for a in range(3)]
            s = r - (((p[0] - o[0]) * d[0] + (p[1] - o[1]) * d[1]) + (p[2] - o[2]) * d[2])
            if not s >= -trunc:
                continue
            sum_[c] += round(min(s / trunc, 1.0) * ONE)             # (Python's round: ties to even)
            count[c] += 1
            wrote += 1
        info[1] += 1 if wrote else 0
        info[4] += wrote
    return sum_, count, info


def field(sum_, count, min_count=1):
    """-> (field float32, valid uint8)"""
    c = count.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (-sum_.astype(np.float64) / (c * ONE)).astype(np.float32)
    return np.where(count > 0, f, np.float32(0.0)).astype(np.float32), (count >= min_count).astype(np.uint8)


def marching_cubes_masked(volume, valid, level, table, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """The unmasked restatement's mesh without the vertices on an edge with an end that is not valid and without the triangles of
    a cell with such a corner; the order of what stays is kept.  -> (verts float32 [V,3], faces int32 [F,3])"""
    v = np.ascontiguousarray(volume, dtype=np.float32)
    ok = np.asarray(valid) != 0
    nx, ny, nz = v.shape
    verts, faces = MR.marching_cubes(v, level, table, spacing, origin)
    inside = v > np.float32(level)
    # the unmasked vertices in their order (node, then axis), and whether both ends of their edge are valid
    cross = np.zeros((3,) + v.shape, dtype=bool)
    both = np.zeros((3,) + v.shape, dtype=bool)
    cross[0, :-1], both[0, :-1] = inside[:-1] != inside[1:], ok[:-1] & ok[1:]
    cross[1, :, :-1], both[1, :, :-1] = inside[:, :-1] != inside[:, 1:], ok[:, :-1] & ok[:, 1:]
    cross[2, :, :, :-1], both[2, :, :, :-1] = inside[:, :, :-1] != inside[:, :, 1:], ok[:, :, :-1] & ok[:, :, 1:]
    flat = cross.reshape(3, -1).T
    keep_v = both.reshape(3, -1).T[flat]                          # row-major over [N,3]: node, then axis
    assert keep_v.shape[0] == verts.shape[0]
    new_id = np.cumsum(keep_v) - 1
    # the unmasked triangles in their order (cell, then the table's), and whether the cell has eight valid corners
    cases = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    cell_ok = np.ones((nx - 1, ny - 1, nz - 1), dtype=bool)
    for c in range(8):
        dx, dy, dz = MR.corner_offset(c)
        cases |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
        cell_ok &= ok[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    ntri = (table >= 0).sum(1) // 3
    ci, cj, ck = np.nonzero(cases)
    keep_f = np.repeat(cell_ok[ci, cj, ck], ntri[cases[ci, cj, ck]])
    assert keep_f.shape[0] == faces.shape[0]
    kept = faces[keep_f]
    assert keep_v[kept].all()
    return verts[keep_v], new_id[kept].astype(np.int32).reshape(-1, 3)


def drop_unreferenced(verts, faces):
    used = np.zeros(verts.shape[0], dtype=bool)
    used[faces.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    return verts[used], new_id[faces].astype(np.int32).reshape(-1, 3)


def extract_mesh(sum_, count, origin, v, table, min_count=1):
    """TSDFVolume.extract_mesh without the component filter -> (vertices float64 [V,3], triangles int32 [F,3]) or None"""
    f, valid = field(sum_, count, min_count)
    verts, faces = marching_cubes_masked(f, valid, 0.0, table, (v, v, v), origin)
    if faces.shape[0] == 0:
        return None
    verts, faces = drop_unreferenced(verts, faces)
    return verts.astype(np.float64), faces


# ------------------------------------------------------------------------------------------------ the rays of the tests
def ray_set(dims, origin, v, seed, n_random=160):
    """Seeded rays against the lattice (dims, origin, v) -> (rays fp64 [n,6], ranges fp64 [n]): random ones starting inside and
    outside the box; axis-parallel ones (two zero components) and ones with one zero component; ones starting on a face of the
    box; and ones that run inside the planes between voxels, on dyadic coordinates when origin and v are, along an axis and along
    a diagonal of the plane (exact ties between the axes at every step)."""
    rng = np.random.default_rng(seed)
    dims, origin = np.asarray(dims), np.asarray(origin, dtype=np.float64)
    lo, hi = origin - 0.5 * v, origin + (dims - 0.5) * v
    size = hi - lo
    rays, ranges = [], []

    def add(o, d, r):
        d = np.asarray(d, dtype=np.float64)
        rays.append(np.concatenate([np.asarray(o, dtype=np.float64), d / np.sqrt((d * d).sum())]))
        ranges.append(float(r))

    for k in range(n_random):
        o = lo + rng.uniform(-0.6, 1.6, 3) * size if k % 2 else lo + rng.uniform(0.0, 1.0, 3) * size
        target = lo + rng.uniform(0.0, 1.0, 3) * size
        d = target - o
        add(o, d, np.sqrt((d * d).sum()) * rng.uniform(0.3, 1.5))
    for a in range(3):
        for sign in (1.0, -1.0):
            for _ in range(6):                                          # along an axis, from inside and from outside
                o = lo + rng.uniform(-0.3, 1.3, 3) * size
                o[(a + 1) % 3] = lo[(a + 1) % 3] + rng.uniform(0.0, 1.0) * size[(a + 1) % 3]
                o[(a + 2) % 3] = lo[(a + 2) % 3] + rng.uniform(0.0, 1.0) * size[(a + 2) % 3]
                d = np.zeros(3)
                d[a] = sign
                add(o, d, rng.uniform(0.2, 1.2) * size[a])
            for _ in range(6):                                          # one zero component
                o = lo + rng.uniform(0.0, 1.0, 3) * size
                d = rng.normal(size=3)
                d[a] = 0.0
                add(o, d, rng.uniform(0.2, 1.0) * size.max())
        for side in (lo, hi):                                           # on a face, heading in and heading out
            for _ in range(4):
                o = lo + rng.uniform(0.0, 1.0, 3) * size
                o[a] = side[a]
                add(o, rng.normal(size=3), rng.uniform(0.2, 1.0) * size.max())
        b, c = (a + 1) % 3, (a + 2) % 3
        for i in range(0, dims[a] + 1):                                 # inside the plane between voxels i - 1 and i of axis a
            o = np.empty(3)
            o[a] = origin[a] + (i - 0.5) * v
            o[b] = origin[b] + (int(rng.integers(0, dims[b])) - 0.5) * v
            o[c] = origin[c] + (int(rng.integers(0, dims[c])) - 0.5) * v
            d = np.zeros(3)
            d[b] = 1.0
            add(o, d, 0.5 * size[b])
            d[c] = -1.0 if i % 2 else 1.0
            add(o, d, 0.75 * size.max())
            d[a] = 1.0                                                  # the space diagonal from a lattice corner: a three-way tie
            add(o, d, 0.75 * size.max())
    return np.asarray(rays), np.asarray(ranges)


# ------------------------------------------------------------------------------------------------ brute force, for the walk
def voxels_crossed(o, d, r, dims, origin, v, trunc, front, grow):
    """bool [nx,ny,nz]: the voxels (cubes of edge v about the nodes) grown by `grow` metres on every side (negative: shrunk) that
    the segment t in [max(0, r - front), r + trunc] of o + t d meets, by a slab test per voxel in the world frame."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    t0 = np.full(dims, max(0.0, r - front))
    t1 = np.full(dims, r + trunc)
    hit = np.ones(dims, dtype=bool)
    for a in range(3):
        shape = [1, 1, 1]
        shape[a] = dims[a]
        centre = (origin[a] + np.arange(dims[a], dtype=np.float64) * v).reshape(shape)
        lo, hi = centre - (0.5 * v + grow), centre + (0.5 * v + grow)
        if d[a] == 0.0:
            hit &= (lo <= o[a]) & (o[a] <= hi)
        else:
            ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
            t0 = np.maximum(t0, np.minimum(ta, tb))
            t1 = np.minimum(t1, np.maximum(ta, tb))
    return hit & (t0 <= t1)
