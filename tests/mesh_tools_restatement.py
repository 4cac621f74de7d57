"""The mesh tools of include/loner_hip.h ("mesh tools") restated in plain Python and numpy, item by item: connected components from a
dictionary of edges and a union-find, cluster areas (exactly rounded by math.fsum, and in the header's 64-ary order), the compaction
behind the filters, and the vertex normals summed in (corner slot, triangle) order.  Every fp64 step is one numpy or Python operation,
so it rounds as the kernels compiled without contraction do."""
import math

import numpy as np

from tests import cloud_tools_restatement as TR


# ---------------------------------------------------------------- connected components
def edge_triangles(triangles):
    """{(lo, hi): [triangles using the edge, ascending]} over the three edges 0-1, 1-2, 2-0 of every triangle"""
    edges = {}
    for t, (a, b, c) in enumerate(np.asarray(triangles, dtype=np.int64).reshape(-1, 3).tolist()):
        for u, w in ((a, b), (b, c), (c, a)):
            edges.setdefault((min(u, w), max(u, w)), []).append(t)
    return edges


def first_triangle_numbering(representative):
    """labels from any per-triangle representative: clusters numbered in the order their first triangle appears"""
    ids, labels = {}, np.zeros(len(representative), dtype=np.int32)
    for t, r in enumerate(representative):
        labels[t] = ids.setdefault(int(r), len(ids))
    return labels


def connected_triangles(triangles):
    """-> (triangle_clusters int32 [F], cluster_n_triangles int32 [C]): triangles sharing an edge are united, clusters numbered by
    ascending smallest triangle"""
    n = np.asarray(triangles).reshape(-1, 3).shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for users in edge_triangles(triangles).values():
        for t in users[1:]:
            a, b = find(users[0]), find(t)
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels = first_triangle_numbering([find(t) for t in range(n)])
    return labels, np.bincount(labels, minlength=0).astype(np.int32)


# ---------------------------------------------------------------- cluster area
def cluster_areas_exact(vertices, triangles, labels, n_clusters):
    """the exactly rounded sum of every cluster's triangle areas (math.fsum over TR.triangle_areas)"""
    a = TR.triangle_areas(vertices, triangles)
    labels = np.asarray(labels)
    return np.array([math.fsum(a[labels == c].tolist()) for c in range(n_clusters)], dtype=np.float64)


def tree_sum(terms):
    """the header's order: groups of 64 consecutive entries replaced by their left-to-right sums until one entry is left"""
    level = [float(x) for x in terms]
    if not level:
        return 0.0
    while len(level) > 1:
        nxt = []
        for g in range(0, len(level), 64):
            s = level[g]
            for x in level[g + 1:g + 64]:
                s = s + x
            nxt.append(s)
        level = nxt
    return level[0]


def cluster_areas_tree(vertices, triangles, labels, n_clusters):
    a = TR.triangle_areas(vertices, triangles)
    labels = np.asarray(labels)
    return np.array([tree_sum(a[labels == c].tolist()) for c in range(n_clusters)], dtype=np.float64)


# ---------------------------------------------------------------- select
def select(triangles, n_vertices, triangle_keep=None, vertex_keep=None, drop_unreferenced=False):
    """-> (surviving triangles re-indexed int32 [F',3], vertex_map int32 [V], surviving vertices)"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    tk = np.ones(len(t), dtype=bool) if triangle_keep is None else np.asarray(triangle_keep, dtype=bool)
    vk = np.ones(n_vertices, dtype=bool) if vertex_keep is None else np.asarray(vertex_keep, dtype=bool)
    alive = [bool(tk[i]) and all(bool(vk[x]) for x in row) for i, row in enumerate(t.tolist())]
    used = np.zeros(n_vertices, dtype=bool)
    for i, row in enumerate(t.tolist()):
        if alive[i]:
            used[row] = True
    v_alive = vk & used if drop_unreferenced else vk
    vmap = np.full(n_vertices, -1, dtype=np.int32)
    vmap[v_alive] = np.arange(int(v_alive.sum()), dtype=np.int32)
    out = vmap[t[np.array(alive, dtype=bool)]].reshape(-1, 3).astype(np.int32)
    return out, vmap, int(v_alive.sum())


def apply_select(vertices, normals, triangles, **kw):
    """select on a mesh: (vertices, normals or None, triangles) of the survivors"""
    out, vmap, _ = select(triangles, len(vertices), **kw)
    kept = vmap >= 0
    return vertices[kept], None if normals is None else normals[kept], out


def small_component_keep(sizes, areas, min_triangles=None, min_area=None, keep_largest=None):
    """the clusters remove_small_components keeps: not below a threshold, then the k with the most triangles (ties: lower id)"""
    keep = [(min_triangles is None or sizes[c] >= min_triangles) and (min_area is None or areas[c] >= min_area)
            for c in range(len(sizes))]
    if keep_largest is not None:
        ranked = sorted((c for c in range(len(sizes)) if keep[c]), key=lambda c: (-int(sizes[c]), c))[:keep_largest]
        keep = [c in ranked for c in range(len(sizes))]
    return np.array(keep, dtype=bool)


# ---------------------------------------------------------------- vertex normals
def face_normals(vertices, triangles):
    """cross(v1 - v0, v2 - v0) per triangle: each component two products and one difference"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    a, b = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def vertex_normals(vertices, triangles):
    """every vertex's sum over its corners in ascending (corner slot k, triangle t), from 0.0, divided by sqrt((x x + y y) + z z) or
    by 1 where that is not > 0"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    fn = face_normals(v, t).tolist()
    sums = [[0.0, 0.0, 0.0] for _ in range(len(v))]
    for k in range(3):
        for ti, i in enumerate(t[:, k].tolist()):
            s, f = sums[i], fn[ti]
            s[0] = s[0] + f[0]
            s[1] = s[1] + f[1]
            s[2] = s[2] + f[2]
    out = np.zeros((len(v), 3), dtype=np.float64)
    for i, (x, y, z) in enumerate(sums):
        norm = math.sqrt((x * x + y * y) + z * z)
        d = norm if norm > 0.0 else 1.0
        out[i] = (x / d, y / d, z / d)
    return out


# ---------------------------------------------------------------- fixtures shared by the host and the GPU tests
def random_shared_mesh(n_vertices=400, n_triangles=3000, seed=11, spare=7):
    """a random mesh over shared vertices (valence ~ 22), some triangles degenerate, and `spare` vertices no triangle uses"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_vertices + spare, 3)) * np.array([3.0, 1.0, 0.1])
    t = rng.integers(0, n_vertices, size=(n_triangles, 3)).astype(np.int32)
    t[::97, 1] = t[::97, 0]
    return v, t


def fan(n_triangles=10000):
    """n triangles around vertex 0: one run of n corners in slot 0"""
    ang = np.linspace(0.0, 2.0 * np.pi, n_triangles + 1, endpoint=False)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.05 * np.sin(7.0 * ang)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.3]], rim])
    i = np.arange(n_triangles, dtype=np.int32)
    return v, np.stack([np.zeros_like(i), i + 1, i + 2], 1).astype(np.int32)


def strip(n_triangles=100003, seed=3):
    """a triangle strip stored in shuffled order: one chain of n_triangles links"""
    i = np.arange(n_triangles, dtype=np.int32)
    t = np.stack([i, i + 1, i + 2], 1)
    return t[np.random.default_rng(seed).permutation(n_triangles)].astype(np.int32), n_triangles + 2


def two_spheres_volume(n=24):
    """two spheres (radii 5.3 and 3.4 voxels) and five one-voxel blobs, positive inside"""
    ax = np.arange(n, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    a = 5.3 ** 2 - ((x - 7.2) ** 2 + (y - 7.6) ** 2 + (z - 8.1) ** 2)
    b = 3.4 ** 2 - ((x - 17.3) ** 2 + (y - 16.4) ** 2 + (z - 15.2) ** 2)
    vol = np.maximum(a, b).astype(np.float32)
    for p in ((2, 20, 3), (20, 3, 3), (3, 3, 20), (21, 21, 4), (12, 20, 21)):
        vol[p] = 1.0
    return vol
