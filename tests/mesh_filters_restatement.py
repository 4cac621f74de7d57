"""Plain Python / numpy restatement of the "mesh simplification and smoothing" contracts of include/loner_hip.h, item by item and in
the sequential orders stated there (dicts and sets for the bookkeeping, np.add.at for every sum: it adds one entry after the other
in the order given, never pairwise), and the small meshes the tests use."""
import numpy as np

INT_MAX = 2147483647


def _bit_length(x):
    return int(x).bit_length() if x > 0 else 0


def cluster_status(vertices, voxel_size):
    """the status word of lnr_mesh_vertex_clusters: 1 non-finite vertex, 2 voxel_size too small, 4 key wider than 64 bits"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    if len(v) == 0:
        return 0
    if not np.isfinite(v).all():
        return 1
    s = np.float64(voxel_size)
    half = s * 0.5
    lo, hi = v.min(0) - half, v.max(0) + half
    if s * np.float64(INT_MAX) < (hi - lo).max():
        return 2
    top = np.floor((v.max(0) - lo) / s)
    if not (top < 2.0 ** 62).all() or sum(_bit_length(int(f)) for f in top) > 64:
        return 4
    return 0


def vertex_clusters(vertices, voxel_size):
    """lnr_mesh_vertex_clusters -> (vertex_cluster int32 [V], cluster_vertices fp64 [m,3]); ValueError with the status otherwise"""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    status = cluster_status(v, voxel_size)
    if status:
        raise ValueError(f"status {status}")
    if len(v) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros((0, 3), dtype=np.float64)
    s = np.float64(voxel_size)
    lo = v.min(0) - s * 0.5
    voxel = np.floor((v - lo) / s).astype(np.int64)
    seen = {}
    cluster = np.zeros(len(v), dtype=np.int32)
    for i, key in enumerate(map(tuple, voxel.tolist())):        # first occurrence numbers the clusters
        cluster[i] = seen.setdefault(key, len(seen))
    m = len(seen)
    sums = np.zeros((m, 3), dtype=np.float64)
    np.add.at(sums, cluster, v)                                 # ascending vertex index, started at 0.0
    count = np.zeros(m, dtype=np.int64)
    np.add.at(count, cluster, 1)
    return cluster, sums / count.astype(np.float64)[:, None]


def canonical_triple(t0, t1, t2):
    """open3d's RemoveDuplicatedTriangles rotation"""
    if t0 <= t1:
        return (t0, t1, t2) if t0 <= t2 else (t2, t0, t1)
    return (t1, t2, t0) if t1 <= t2 else (t2, t0, t1)


def unique_triangles(triangles, vertex_map=None, drop_degenerate=False):
    """lnr_mesh_unique_triangles -> (canonical int32 [F,3], triangle_keep uint8 [F], kept, degenerate)"""
    tris = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if vertex_map is not None:
        tris = np.asarray(vertex_map, dtype=np.int64)[tris]
    canonical = np.zeros((len(tris), 3), dtype=np.int32)
    keep = np.zeros(len(tris), dtype=np.uint8)
    seen = set()
    degenerate = 0
    for t, (a, b, c) in enumerate(tris.tolist()):
        triple = canonical_triple(a, b, c)
        canonical[t] = triple
        distinct = a != b and b != c and c != a
        degenerate += 0 if distinct else 1
        if triple not in seen:
            seen.add(triple)
            keep[t] = 1 if (distinct or not drop_degenerate) else 0
    return canonical, keep, int(keep.sum()), degenerate


def vertex_adjacency(triangles, n_vertices):
    """lnr_mesh_vertex_adjacency -> (row_start int32 [V+1], neighbours int32 [row_start[V]])"""
    rows = [set() for _ in range(n_vertices)]
    for tri in np.asarray(triangles, dtype=np.int64).reshape(-1, 3).tolist():
        for k in range(3):
            i, j = tri[k], tri[(k + 1) % 3]
            if i != j:
                rows[i].add(j)
                rows[j].add(i)
    row_start = np.zeros(n_vertices + 1, dtype=np.int32)
    neighbours = []
    for i, r in enumerate(rows):
        neighbours.extend(sorted(r))
        row_start[i + 1] = len(neighbours)
    return row_start, np.asarray(neighbours, dtype=np.int32).reshape(-1)


def smooth_step(p, row_start, neighbours, kind, f):
    """one step of lnr_mesh_smooth: kind 0 simple, 1 Laplacian"""
    p = np.asarray(p, dtype=np.float64)
    counts = np.diff(row_start.astype(np.int64))
    rows = np.repeat(np.arange(len(p)), counts)                 # row-major: a vertex's neighbours in ascending order
    nb = neighbours.astype(np.int64)
    has = counts > 0
    out = p.copy()
    if kind == 0:
        s = p.copy()
        np.add.at(s, rows, p[nb])
        out[has] = (s / (1 + counts).astype(np.float64)[:, None])[has]
        return out
    d = p[rows] - p[nb]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    w = 1.0 / (dist + 1e-12)
    total = np.zeros(len(p), dtype=np.float64)
    np.add.at(total, rows, w)
    s = np.zeros_like(p)
    np.add.at(s, rows, w[:, None] * p[nb])
    with np.errstate(invalid="ignore", divide="ignore"):
        moved = p + np.float64(f) * (s / total[:, None] - p)
    out[has] = moved[has]
    return out


def smooth(vertices, triangles, n_steps, kind, lambda_filter=0.5, mu=None):
    """lnr_mesh_smooth on the adjacency of the triangles: step s uses lambda_filter when s is even, mu when s is odd"""
    p = np.array(vertices, dtype=np.float64).reshape(-1, 3)
    row_start, neighbours = vertex_adjacency(triangles, len(p))
    mu = lambda_filter if mu is None else mu
    for s in range(n_steps):
        p = smooth_step(p, row_start, neighbours, kind, lambda_filter if s % 2 == 0 else mu)
    return p


def taubin(vertices, triangles, iterations, lambda_filter=0.5, mu=-0.53):
    return smooth(vertices, triangles, 2 * iterations, 1, lambda_filter, mu)


def simplify_vertex_clustering(vertices, triangles, voxel_size):
    """TriangleMesh.simplify_vertex_clustering -> (vertices, triangles)"""
    cluster, means = vertex_clusters(vertices, voxel_size)
    canonical, keep, _, _ = unique_triangles(triangles, cluster, drop_degenerate=True)
    return means, np.ascontiguousarray(canonical[keep.astype(bool)])


# ---------------------------------------------------------------- meshes
def height_field(n=40, spacing=0.1, jitter=0.45, amplitude=2.5, seed=0, shuffle=True):
    """an n x n height-field grid of waves `amplitude` spacings high, the vertices jittered by `jitter` spacings, two triangles per
    cell; with shuffle the vertex and the triangle order are random permutations -> (vertices fp64 [n n,3], triangles int32
    [2 (n-1)^2,3])"""
    rng = np.random.default_rng(seed)
    ix, iy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([ix * spacing, iy * spacing, amplitude * spacing * np.sin(0.7 * ix) * np.cos(0.5 * iy)], -1).reshape(-1, 3)
    v = v + rng.uniform(-jitter * spacing, jitter * spacing, v.shape)
    a = (ix[:-1, :-1] * n + iy[:-1, :-1]).reshape(-1)
    tris = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
    if shuffle:
        perm = rng.permutation(len(v))                          # old index -> new index
        moved = np.empty_like(v)
        moved[perm] = v
        v, tris = moved, perm[tris][rng.permutation(len(tris))]
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(tris, dtype=np.int32)


def fan(n_rim=10000):
    """a hub (vertex 0) joined to n_rim rim vertices on a wavy circle: the hub's row has n_rim neighbours"""
    ang = 2.0 * np.pi * np.arange(n_rim) / n_rim
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(7.0 * ang)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.3]], rim])
    k = np.arange(n_rim)
    tris = np.stack([np.zeros(n_rim, dtype=np.int64), 1 + k, 1 + (k + 1) % n_rim], 1)
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(tris, dtype=np.int32)


def noisy_sphere(n_lat=24, n_lon=48, noise=0.02, seed=0):
    """a latitude-longitude unit sphere (two poles and n_lat - 1 rings of n_lon vertices), the radii scaled by 1 + noise * N(0, 1)"""
    rng = np.random.default_rng(seed)
    theta = np.pi * np.arange(1, n_lat) / n_lat
    phi = 2.0 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.sin(theta), np.sin(phi)),
                     np.outer(np.cos(theta), np.ones(n_lon))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    v = v * (1.0 + noise * rng.standard_normal(len(v)))[:, None]
    tris = []
    south = 1 + (n_lat - 1) * n_lon
    for j in range(n_lon):
        jn = (j + 1) % n_lon
        tris.append([0, 1 + j, 1 + jn])
        tris.append([south, 1 + (n_lat - 2) * n_lon + jn, 1 + (n_lat - 2) * n_lon + j])
        for i in range(n_lat - 2):
            a, b = 1 + i * n_lon + j, 1 + i * n_lon + jn
            tris.append([a, a + n_lon, b])
            tris.append([b, a + n_lon, b + n_lon])
    return np.ascontiguousarray(v, dtype=np.float64), np.asarray(tris, dtype=np.int32)


TETRAHEDRON = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 4.0]]),
               np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32))
