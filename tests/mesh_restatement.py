"""CPU restatements of the meshing path (analysis/mesher.py:143-207 of the reference), the yardsticks of tests/test_*mesh*.py.

reference_accumulate   the reference's op sequence for one batch of rendered rays, literally (mesher.py:143-180), including its
                       indexed assignment `results[idx] = max(results[idx], w)` (last writer wins among duplicate indices)
restated_accumulate    the same sequence with that one assignment replaced by scatter_reduce(amax): the true max, which the HIP
                       kernel (lnr_render_mesh_accumulate) computes
marching_cubes         numpy marching cubes with the library's exported case table and the vertex rule of include/loner_hip.h
"""
import numpy as np
import torch


def _filtered(spoints, weights, depths, variance, bound, axes, ray_range, var_threshold, n_results):
    """mesher.py:143-178: -> (bucket_idx int64 [k], weights [k, 1]) of the samples that survive the filters"""
    valid_idx = depths < ray_range[1] - 0.25
    if var_threshold is not None:
        valid_idx = torch.logical_and(valid_idx, variance < var_threshold)
    spoints = spoints[valid_idx, ...]
    weights = weights[valid_idx, ...]
    spoints = spoints.view(-1, 3)
    weights = weights.view(-1, 1)
    good_idx = torch.ones_like(weights.flatten())
    for i in range(3):
        good_dim = torch.logical_and(spoints[:, i] >= bound[i][0], spoints[:, i] <= bound[i][1])
        good_idx = torch.logical_and(good_idx, good_dim)
    spoints = spoints[good_idx]
    if len(spoints) == 0:
        return None, None
    x_boundaries, y_boundaries, z_boundaries = (torch.from_numpy(np.asarray(a, dtype=np.float64)).contiguous() for a in axes)
    x = spoints[:, 0].contiguous()
    y = spoints[:, 1].contiguous()
    z = spoints[:, 2].contiguous()
    x_buck = torch.bucketize(x, x_boundaries)
    y_buck = torch.bucketize(y, y_boundaries)
    z_buck = torch.bucketize(z, z_boundaries)
    bucket_idx = x_buck * len(z_boundaries) + y_buck * len(x_boundaries) * len(z_boundaries) + z_buck
    weights = weights[good_idx]
    valid_buckets = bucket_idx < n_results
    return bucket_idx[valid_buckets], weights[valid_buckets]


def reference_accumulate(results, spoints, weights, depths, variance, bound, axes, ray_range, var_threshold=None):
    """results: float64 [ny*nx*nz] (the reference's `results`), updated in place.  bound: 0-dim-indexable float64 torch tensor [3,2]."""
    idx, w = _filtered(spoints, weights, depths, variance, bound, axes, ray_range, var_threshold, len(results))
    if idx is not None:
        results[idx] = torch.max(results[idx], w.flatten())
    return results


def restated_accumulate(results, spoints, weights, depths, variance, bound, axes, ray_range, var_threshold=None):
    """As reference_accumulate, the assignment replaced by a scatter-max."""
    idx, w = _filtered(spoints, weights, depths, variance, bound, axes, ray_range, var_threshold, len(results))
    if idx is not None:
        results.scatter_reduce_(0, idx, w.flatten().to(results.dtype), reduce="amax", include_self=True)
    return results


# ------------------------------------------------------------------------------------------------ marching cubes
def edge_corners(e):
    """edge id 4 a + q -> (lower corner, upper corner); corner c = x + 2 y + 4 z"""
    a, q = e >> 2, e & 3
    o0, o1 = (1, 2) if a == 0 else ((0, 2) if a == 1 else (0, 1))
    c0 = ((q & 1) << o0) | (((q >> 1) & 1) << o1)
    return c0, c0 | (1 << a)


def corner_offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def marching_cubes(volume, level, table, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """volume float32 [nx, ny, nz] -> (verts float32 [V,3], faces int32 [F,3]) in the library's order and arithmetic."""
    v = np.ascontiguousarray(volume, dtype=np.float32)
    nx, ny, nz = v.shape
    lev = np.float32(level)
    sp = np.asarray(spacing, dtype=np.float32)
    org = np.asarray(origin, dtype=np.float32)
    inside = v > lev
    # edge bits per node, x / y / z
    bits = np.zeros((3,) + v.shape, dtype=bool)
    bits[0, :-1] = inside[:-1] != inside[1:]
    bits[1, :, :-1] = inside[:, :-1] != inside[:, 1:]
    bits[2, :, :, :-1] = inside[:, :, :-1] != inside[:, :, 1:]
    flat_bits = bits.reshape(3, -1).T                                      # [N, 3]: node order, then axis
    count = flat_bits.sum(1)
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    node, axis = np.nonzero(flat_bits)                                     # node-major, axis-minor: the vertex order
    i, j, k = np.unravel_index(node, v.shape)
    ijk = np.stack([i, j, k], 1)
    va = v.reshape(-1)[node]
    nb = ijk.copy()
    nb[np.arange(len(node)), axis] += 1
    vb = v[nb[:, 0], nb[:, 1], nb[:, 2]]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (lev - va) / (vb - va)
    f = ijk.astype(np.float32)
    f[np.arange(len(node)), axis] = f[np.arange(len(node)), axis] + t.astype(np.float32)
    verts = (f * sp) + org
    verts = verts.astype(np.float32)
    # triangles
    cases = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = corner_offset(c)
        cases |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.nonzero(cases)                                         # C order = cell (lower node) order
    cell_case = cases[ci, cj, ck]
    faces = []
    ntri = (table >= 0).sum(1) // 3
    # expand per cell, then per table triangle
    reps = ntri[cell_case]
    cell_rep = np.repeat(np.arange(len(cell_case)), reps)
    tri_in_cell = np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps)
    if len(cell_rep) == 0:
        return verts.reshape(-1, 3), np.zeros((0, 3), dtype=np.int32)
    cc = cell_case[cell_rep]
    base = np.stack([ci[cell_rep], cj[cell_rep], ck[cell_rep]], 1)
    out = np.zeros((len(cell_rep), 3), dtype=np.int64)
    for m in range(3):
        e = table[cc, 3 * tri_in_cell + m].astype(np.int64)
        a = e >> 2
        c0 = np.array([edge_corners(x)[0] for x in range(12)])[e]
        off = np.stack([c0 & 1, (c0 >> 1) & 1, (c0 >> 2) & 1], 1)
        owner = base + off
        on = np.ravel_multi_index((owner[:, 0], owner[:, 1], owner[:, 2]), v.shape)
        # vertex id of (node, axis): first[node] + the node's crossing edges on the axes before
        out[:, m] = first[on] + np.where(a >= 1, flat_bits[on, 0], 0) + np.where(a == 2, flat_bits[on, 1], 0)
    faces = out.astype(np.int32)
    return verts.reshape(-1, 3), faces


def edges_of(faces):
    """directed edges of the triangles, [3F, 2]"""
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def closed_and_oriented(faces, n_verts=None):
    """(closed, oriented): every undirected edge is used by exactly two triangles, and then once in each direction"""
    d = edges_of(faces)
    n = int(d.max()) + 1 if n_verts is None else int(n_verts)
    key_d = d[:, 0] * n + d[:, 1]
    und = np.minimum(d[:, 0], d[:, 1]) * n + np.maximum(d[:, 0], d[:, 1])
    _, cnt = np.unique(und, return_counts=True)
    closed = bool((cnt == 2).all())
    oriented = closed and np.unique(key_d).size == key_d.size
    return closed, oriented


def euler_characteristic(faces):
    f = np.asarray(faces, dtype=np.int64)
    V = np.unique(f).size
    d = edges_of(f)
    E = np.unique(np.minimum(d[:, 0], d[:, 1]) * (f.max() + 1) + np.maximum(d[:, 0], d[:, 1])).size
    return V - E + f.shape[0]


def vertex_links_are_single_cycles(faces):
    """Manifold at the vertices: around every vertex the edges opposite it (its link, directed by the triangles' orientation) form ONE
    closed cycle - one fan of triangles, not two sheets pinched together at the vertex and no fan left open."""
    f = np.asarray(faces, dtype=np.int64)
    nxt = {}
    for a, b, c in f.tolist():
        for v, u, w in ((a, b, c), (b, c, a), (c, a, b)):
            link = nxt.setdefault(v, {})
            if u in link:
                return False                      # two link edges leave the same neighbour: not a simple cycle
            link[u] = w
    for v, link in nxt.items():
        start = next(iter(link))
        u, steps = start, 0
        while True:
            if u not in link:
                return False                      # the fan is open
            u = link[u]
            steps += 1
            if u == start:
                break
            if steps > len(link):
                return False
        if steps != len(link):
            return False                          # more than one cycle around the vertex
    return True
