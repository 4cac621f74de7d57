"""Meshes: the mesher's lattice and accumulation, marching cubes, surface sampling, the mesh tools, filters and smoothing.
Offline tools: vertices are widened to fp64, triangles must be int32 [F,3], scratch is a buffer per call, and every call that reports a
status or a count reads it back once.  ValueError: an argument the caller got wrong, refused before a launch.  RuntimeError: what only
the data shows (an index out of range, a non-finite vertex, a size over the library's limit)."""
import ctypes as C
import math

import numpy as np
import torch

from .. import hip
from ..hip import _ptr, _stream, check, load, require_device
from ._common import _f32c, _f64_points, _mesh_triangles, _positive, _raise_status, _render_inputs, _scratch
from .cloud import _cloud_status

MESH_SMOOTH_KINDS = {"simple": 0, "laplacian": 1}
_MESH_STATUS = {1: "a triangle uses a non-finite vertex", 2: "a vertex index is out of range", 4: "the total area is not finite"}     # sampling
_MESH_TOOLS_STATUS = {1: "a vertex index is out of range", 2: "a cluster id is out of range"}
_MESH_FILTERS_STATUS = {1: "an index is out of range"}


class MeshLattice:
    """The mesher's lattice on a device (include/loner_hip.h: LnrMeshGrid): the three np.linspace axes (fp64, kept alive here) and
    the bound of the reference's fp32 bound check.  axes: three 1-D float64 arrays; bound: [[lo, hi]] x 3 (float64, world-cube units)."""

    def __init__(self, axes, bound, device):
        self.axes = [torch.as_tensor(np.asarray(a, dtype=np.float64)).to(device).contiguous() for a in axes]
        self.shape = tuple(int(a.numel()) for a in self.axes)            # (nx, ny, nz)
        g = hip.MeshGrid()
        for i, a in enumerate(axes):
            a = np.asarray(a, dtype=np.float64)
            g.n[i] = a.shape[0]
            g.lo[i] = float(np.float32(bound[i][0]))                     # the 0-dim fp64 bound meets fp32 points: compared in fp32
            g.hi[i] = float(np.float32(bound[i][1]))
            g.first[i] = float(a[0])
            g.inv_step[i] = float(1.0 / (a[1] - a[0])) if a.shape[0] > 1 and a[1] != a[0] else 0.0
            g.axis[i] = self.axes[i].data_ptr()
        self.grid = g

    @property
    def n_nodes(self):
        return self.shape[0] * self.shape[1] * self.shape[2]


def mesh_accumulate(sigma, z, rays, lattice: MeshLattice, volume, depth_max, var_max=None, noise=None, noise_std=0.0, seed=0,
                    n_rays_dev=None, counters=None):
    """Renders the rays (lnr_render_forward's arithmetic) and max-accumulates every sample's weight into volume [ny*nx*nz] fp32 (the
    reference's [y][x][z] order, include/loner_hip.h: lnr_render_mesh_accumulate).  counters: optional int64 [2] += {samples that
    reached the volume, atomics issued}."""
    require_device(sigma, z, rays, volume, noise, counters)
    sigma, z, rays, n, s = _render_inputs(sigma, z, rays)
    assert volume.dtype == torch.float32 and volume.is_contiguous() and volume.numel() == lattice.n_nodes
    assert counters is None or (counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() == 2)
    check(load().lnr_render_mesh_accumulate(_ptr(sigma), _ptr(z), _ptr(rays), n, _ptr(n_rays_dev), s, _ptr(_f32c(noise)), float(noise_std), int(seed),
                                            C.byref(lattice.grid), float(depth_max), 0 if var_max is None else 1,
                                            0.0 if var_max is None else float(var_max), _ptr(volume), _ptr(counters),
                                            _stream()), "lnr_render_mesh_accumulate")
    return volume


def mc_case_table():
    """The marching-cubes case table as numpy int8 [256, MC_TABLE_WIDTH] (host: no device needed)."""
    out = np.empty((256, hip.MC_TABLE_WIDTH), dtype=np.int8)
    check(load().lnr_mc_case_table(out.ctypes.data_as(C.c_void_p)), "lnr_mc_case_table")
    return out


def marching_cubes(volume, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), valid=None):
    """Marching cubes of a device volume [nx, ny, nz] at `level` (inside: v > level) -> (verts [V,3] fp32, faces [F,3] int32) on the
    device; both empty when nothing crosses the level.  Vertex i lies at index * spacing + origin (include/loner_hip.h: lnr_mc_*).
    One device -> host read of the two totals sizes the outputs.
    valid (uint8 or bool [nx, ny, nz] on the volume's device, optional): the nodes that were observed (lnr_mc_*_masked); a cell with a
    corner that is not valid emits nothing, and vertices no surviving cell uses may remain (mesh_select(drop_unreferenced=True))."""
    require_device(volume)
    vol = _f32c(volume)
    assert vol.dim() == 3, "marching_cubes: a 3-D volume [nx, ny, nz]"
    nx, ny, nz = (int(x) for x in vol.shape)
    dev = vol.device
    if valid is not None:
        require_device(valid)
        if tuple(valid.shape) != (nx, ny, nz) or valid.dtype not in (torch.uint8, torch.bool) or valid.device != dev:
            raise ValueError(f"marching_cubes: valid must be uint8 or bool [{nx},{ny},{nz}] on {dev}, got {valid.dtype} "
                             f"{tuple(valid.shape)} on {valid.device}")
        mask = valid.to(torch.uint8).contiguous()
    lib = load()
    masked = () if valid is None else (_ptr(mask),)     # the *_masked entries take the mask after the volume
    count, emit = ("lnr_mc_count", "lnr_mc_emit") if valid is None else ("lnr_mc_count_masked", "lnr_mc_emit_masked")
    ws_bytes = int(lib.lnr_mc_workspace(nx, ny, nz))    # 0 for an axis with fewer than two nodes: lnr_mc_count refuses that itself
    ws, _ = _scratch(max(ws_bytes, 1), dev)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    check(getattr(lib, count)(_ptr(vol), *masked, nx, ny, nz, float(level), _ptr(ws), ws_bytes, _ptr(totals), _stream()), count)
    n_verts, n_tris = (int(x) for x in totals.cpu())
    if n_verts >= 1 << 30:                          # lnr_mc_emit's limit: refused before the outputs are allocated
        raise RuntimeError(f"marching_cubes: {n_verts} vertices, the limit is 2^30 - 1")
    verts = torch.empty(n_verts, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(n_tris, 3, device=dev, dtype=torch.int32)
    sp = (C.c_float * 3)(*[float(x) for x in spacing])
    org = (C.c_float * 3)(*[float(x) for x in origin])
    check(getattr(lib, emit)(_ptr(vol), *masked, nx, ny, nz, float(level), sp, org, _ptr(ws), ws_bytes, n_verts, n_tris, _ptr(verts),
                             _ptr(faces), _stream()), emit)
    return verts, faces


def mesh_sample_points(vertices, triangles, n_points, seed=0, want_triangles=False, info=None):
    """open3d's sample_points_uniformly with a defined order (include/loner_hip.h: lnr_mesh_sample_points): vertices [V,3] (fp64) and
    triangles [F,3] (int32) on the device -> points [m,3] fp64 (and the owning triangle int32 [m] when asked); m = n_points, or 0 for a
    mesh without area.  info (a dict, optional) receives {"area", "bad_triangles"}.  Raises RuntimeError on a status bit.  One
    device -> host read."""
    v = _f64_points(vertices, "mesh_sample_points")
    tri = _mesh_triangles(triangles, "mesh_sample_points")
    n, seed = int(n_points), int(seed)
    if n < 0 or not 0 <= seed < 2 ** 64:
        raise ValueError(f"mesh_sample_points: n_points >= 0 and a 64-bit seed, got {n_points!r} and {seed!r}")
    dev = v.device
    lib = load()
    ws, need = _scratch(lib.lnr_mesh_sample_workspace(tri.shape[0]), dev,
                        f"mesh_sample_points: {tri.shape[0]} triangles, the limit is 2^31 - 4096")
    points = torch.empty(n, 3, device=dev, dtype=torch.float64)
    owner = torch.empty(n, device=dev, dtype=torch.int32) if want_triangles else None
    info_dev = torch.empty(8, device=dev, dtype=torch.int64)
    check(lib.lnr_mesh_sample_points(_ptr(v), v.shape[0], _ptr(tri), tri.shape[0], n, seed, _ptr(ws), need, _ptr(points), _ptr(owner), _ptr(info_dev),
                                     _stream()), "lnr_mesh_sample_points")
    host = info_dev.cpu()
    _raise_status("mesh_sample_points", int(host[0]), _MESH_STATUS, f"{int(host[2])} bad triangles: ")
    if info is not None:
        info.update(area=float(host[3:4].view(torch.float64)[0]), bad_triangles=int(host[2]))
    m = int(host[1])
    return (points[:m], owner[:m]) if want_triangles else points[:m]


def _mesh_workspace(family, what, n_vertices, n_triangles, device):
    """per-call scratch of a mesh-tools or mesh-filters entry (family: "tools" or "filters")"""
    limits = {"tools": "2^31 - 1 vertices and 3 * triangles", "filters": "2^31 - 4096 vertices and 6 * triangles"}[family]
    return _scratch(getattr(load(), f"lnr_mesh_{family}_workspace")(int(n_vertices), int(n_triangles)), device,
                    f"{what}: {n_vertices} vertices and {n_triangles} triangles, the limits are {limits} <= 2^31 - 4096")


def _mesh_tools_info(what, info_dev, messages=_MESH_TOOLS_STATUS):
    """the one device -> host read of a mesh-tools call: (a, b) of its info words; RuntimeError on a status bit"""
    host = info_dev.cpu()
    _raise_status(what, int(host[0]), messages)
    return int(host[1]), int(host[2])


def mesh_connected_triangles(triangles, n_vertices):
    """open3d's cluster_connected_triangles without the areas (include/loner_hip.h: lnr_mesh_connected_triangles): triangles [F,3]
    int32 on the device, indices in [0, n_vertices) -> (triangle_clusters int32 [F], cluster_n_triangles int32 [C]) on the device,
    clusters numbered by their smallest triangle.  Raises RuntimeError on an index out of range.  One device -> host read (C)."""
    tri = _mesh_triangles(triangles, "mesh_connected_triangles")
    f, dev = tri.shape[0], tri.device
    ws, need = _mesh_workspace("tools", "mesh_connected_triangles", 0, f, dev)
    if not 0 <= int(n_vertices) < 2 ** 31:
        raise RuntimeError(f"mesh_connected_triangles: {n_vertices} vertices, the limit is 2^31 - 1")
    clusters = torch.empty(f, device=dev, dtype=torch.int32)
    sizes = torch.empty(f, device=dev, dtype=torch.int32)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_connected_triangles(_ptr(tri), f, int(n_vertices), _ptr(ws), need, _ptr(clusters), _ptr(sizes), _ptr(info),
                                              _stream()), "lnr_mesh_connected_triangles")
    c, _ = _mesh_tools_info("mesh_connected_triangles", info)
    return clusters, sizes[:c]


def mesh_cluster_area(vertices, triangles, triangle_clusters, n_clusters):
    """The summed triangle area of every cluster in a fixed order (include/loner_hip.h: lnr_mesh_cluster_area) -> fp64 [n_clusters]
    on the device.  Raises RuntimeError on a vertex index or a cluster id out of range.  One device -> host read (the status)."""
    v = _f64_points(vertices, "mesh_cluster_area")
    tri = _mesh_triangles(triangles, "mesh_cluster_area")
    require_device(triangle_clusters)
    f, c, dev = tri.shape[0], int(n_clusters), tri.device
    if triangle_clusters.dtype != torch.int32 or tuple(triangle_clusters.shape) != (f,) or not 0 <= c <= f:
        raise ValueError(f"mesh_cluster_area: triangle_clusters int32 [{f}] and 0 <= n_clusters <= {f}, got "
                         f"{tuple(triangle_clusters.shape)} {triangle_clusters.dtype} and {n_clusters!r}")
    ws, need = _mesh_workspace("tools", "mesh_cluster_area", 0, f, dev)
    area = torch.empty(c, device=dev, dtype=torch.float64)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_cluster_area(_ptr(v), v.shape[0], _ptr(tri), f, _ptr(triangle_clusters.contiguous()), c, _ptr(ws), need, _ptr(area), _ptr(info),
                                       _stream()), "lnr_mesh_cluster_area")
    _mesh_tools_info("mesh_cluster_area", info)
    return area


def _keep_mask(mask, n, what):
    if mask is None:
        return None
    require_device(mask)
    if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (n,):
        raise ValueError(f"mesh_select: {what} bool or uint8 [{n}], got {tuple(mask.shape)} {mask.dtype}")
    return mask.to(torch.uint8).contiguous()


def mesh_select(triangles, n_vertices, triangle_keep=None, vertex_keep=None, drop_unreferenced=False):
    """The compaction behind the mesh filters (include/loner_hip.h: lnr_mesh_select): triangles [F,3] int32, optional keep masks
    (bool or uint8) per triangle and per vertex -> (the surviving triangles [F',3] int32 re-indexed, vertex_map int32 [V] with the
    new index or -1, the number of surviving vertices).  Raises RuntimeError on an index out of range.  One device -> host read."""
    tri = _mesh_triangles(triangles, "mesh_select")
    f, v, dev = tri.shape[0], int(n_vertices), tri.device
    tk, vk = _keep_mask(triangle_keep, f, "triangle_keep"), _keep_mask(vertex_keep, v, "vertex_keep")
    ws, need = _mesh_workspace("tools", "mesh_select", v, f, dev)
    out = torch.empty(f, 3, device=dev, dtype=torch.int32)
    vmap = torch.empty(v, device=dev, dtype=torch.int32)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_select(_ptr(tri), f, v, _ptr(tk), _ptr(vk), 1 if drop_unreferenced else 0, _ptr(ws), need, _ptr(out), _ptr(vmap), _ptr(info),
                                 _stream()), "lnr_mesh_select")
    n_v, n_f = _mesh_tools_info("mesh_select", info)
    return out[:n_f], vmap, n_v


def mesh_vertex_normals(vertices, triangles):
    """TriangleMesh.compute_vertex_normals on the device, bit for bit (include/loner_hip.h: lnr_mesh_vertex_normals) -> fp64 [V,3].
    Raises RuntimeError on an index out of range.  One device -> host read (the status)."""
    v = _f64_points(vertices, "mesh_vertex_normals")
    tri = _mesh_triangles(triangles, "mesh_vertex_normals")
    f, dev = tri.shape[0], tri.device
    ws, need = _mesh_workspace("tools", "mesh_vertex_normals", 0, f, dev)
    normals = torch.empty(v.shape[0], 3, device=dev, dtype=torch.float64)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_vertex_normals(_ptr(v), v.shape[0], _ptr(tri), f, _ptr(ws), need, _ptr(normals), _ptr(info),
                                         _stream()), "lnr_mesh_vertex_normals")
    _mesh_tools_info("mesh_vertex_normals", info)
    return normals


def _vertex_count(n_vertices, what):
    v = int(n_vertices)
    if v != n_vertices or not 0 <= v < 2 ** 31:
        raise ValueError(f"{what}: n_vertices must be an integer in [0, 2^31 - 1], got {n_vertices!r}")
    return v


def mesh_vertex_clusters(vertices, voxel_size):
    """The vertex half of open3d's simplify_vertex_clustering with averaging (include/loner_hip.h: lnr_mesh_vertex_clusters):
    vertices [V,3] (fp64) -> (vertex_cluster int32 [V], cluster_vertices fp64 [m,3]) on the device, clusters numbered by first
    occurrence.  Raises ValueError for a voxel_size that is not finite and > 0, RuntimeError on a non-finite vertex, a voxel_size
    that is too small or a key wider than 64 bits.  One device -> host read (the status and m)."""
    s = _positive(voxel_size, "mesh_vertex_clusters", "voxel_size")
    v = _f64_points(vertices, "mesh_vertex_clusters")
    n, dev = v.shape[0], v.device
    ws, need = _mesh_workspace("filters", "mesh_vertex_clusters", n, 0, dev)
    cluster = torch.empty(n, device=dev, dtype=torch.int32)
    means = torch.empty(n, 3, device=dev, dtype=torch.float64)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_vertex_clusters(_ptr(v), n, s, _ptr(ws), need, _ptr(cluster), _ptr(means), _ptr(info), _stream()), "lnr_mesh_vertex_clusters")
    host = info.cpu()
    _cloud_status("mesh_vertex_clusters", host, "vertices")
    return cluster, means[:int(host[1])]


def mesh_unique_triangles(triangles, n_vertices, vertex_map=None, n_mapped=None, drop_degenerate=False):
    """open3d's remove_duplicated_triangles as a mask (include/loner_hip.h: lnr_mesh_unique_triangles): triangles [F,3] int32,
    optional vertex_map int32 [n_vertices] with values in [0, n_mapped) -> (canonical int32 [F,3], the mapped corners rotated by
    open3d's rule; triangle_keep uint8 [F], 1 for the first triangle of each canonical triple, with drop_degenerate only where its
    three indices differ; the number kept; the number of degenerate triangles).  Raises RuntimeError on an index or a mapped value
    out of range.  One device -> host read."""
    tri = _mesh_triangles(triangles, "mesh_unique_triangles")
    f, dev = tri.shape[0], tri.device
    v = _vertex_count(n_vertices, "mesh_unique_triangles")
    if vertex_map is None:
        if n_mapped is not None and int(n_mapped) != v:
            raise ValueError(f"mesh_unique_triangles: n_mapped is n_vertices without a vertex_map, got {n_mapped!r}")
        m = v
    else:
        require_device(vertex_map)
        if vertex_map.dtype != torch.int32 or tuple(vertex_map.shape) != (v,) or n_mapped is None or not 0 <= int(n_mapped) < 2 ** 31:
            raise ValueError(f"mesh_unique_triangles: vertex_map int32 [{v}] and n_mapped in [0, 2^31 - 1], got "
                             f"{tuple(vertex_map.shape)} {vertex_map.dtype} and {n_mapped!r}")
        vertex_map, m = vertex_map.contiguous(), int(n_mapped)
    ws, need = _mesh_workspace("filters", "mesh_unique_triangles", 0, f, dev)
    canonical = torch.empty(f, 3, device=dev, dtype=torch.int32)
    keep = torch.empty(f, device=dev, dtype=torch.uint8)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_unique_triangles(_ptr(tri), f, v, _ptr(vertex_map), m, 1 if drop_degenerate else 0, _ptr(ws), need, _ptr(canonical), _ptr(keep),
                                           _ptr(info), _stream()), "lnr_mesh_unique_triangles")
    n_kept, n_degenerate = _mesh_tools_info("mesh_unique_triangles", info, _MESH_FILTERS_STATUS)
    return canonical, keep, n_kept, n_degenerate


def mesh_vertex_adjacency(triangles, n_vertices):
    """Every vertex's distinct neighbours as a CSR (include/loner_hip.h: lnr_mesh_vertex_adjacency): triangles [F,3] int32 ->
    (row_start int32 [V+1], neighbours int32 [row_start[V]]) on the device, each row ascending, a vertex never its own neighbour.
    Raises RuntimeError on an index out of range.  One device -> host read (the status and the number of neighbours)."""
    tri = _mesh_triangles(triangles, "mesh_vertex_adjacency")
    f, dev = tri.shape[0], tri.device
    v = _vertex_count(n_vertices, "mesh_vertex_adjacency")
    ws, need = _mesh_workspace("filters", "mesh_vertex_adjacency", 0, f, dev)
    row_start = torch.empty(v + 1, device=dev, dtype=torch.int32)
    neighbours = torch.empty(6 * f, device=dev, dtype=torch.int32)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_vertex_adjacency(_ptr(tri), f, v, _ptr(ws), need, _ptr(row_start), _ptr(neighbours), _ptr(info),
                                           _stream()), "lnr_mesh_vertex_adjacency")
    n, _ = _mesh_tools_info("mesh_vertex_adjacency", info, _MESH_FILTERS_STATUS)
    return row_start, neighbours[:n]


def mesh_smooth(vertices, row_start, neighbours, n_steps, kind="laplacian", lambda_filter=0.5, mu=None):
    """n_steps smoothing steps on the device (include/loner_hip.h: lnr_mesh_smooth): vertices [V,3] (fp64), the adjacency of
    mesh_vertex_adjacency, kind "simple" or "laplacian"; step s uses lambda_filter when s is even and mu (default: lambda_filter)
    when s is odd, so Taubin's k iterations are 2 k Laplacian steps with mu < 0 -> a new fp64 [V,3] tensor; the input is not
    changed.  Raises RuntimeError on an adjacency entry out of range.  One device -> host read (the status)."""
    if kind not in MESH_SMOOTH_KINDS:
        raise ValueError(f"mesh_smooth: kind must be one of {sorted(MESH_SMOOTH_KINDS)}, got {kind!r}")
    steps = int(n_steps)
    if steps != n_steps or not 0 <= steps < 2 ** 31:
        raise ValueError(f"mesh_smooth: n_steps must be an integer >= 0, got {n_steps!r}")
    lam = float(lambda_filter)
    m = lam if mu is None else float(mu)
    if not (math.isfinite(lam) and math.isfinite(m)):
        raise ValueError(f"mesh_smooth: the factors must be finite, got {lambda_filter!r} and {mu!r}")
    v = _f64_points(vertices, "mesh_smooth").clone()
    require_device(row_start, neighbours)
    n, dev = v.shape[0], v.device
    if row_start.dtype != torch.int32 or tuple(row_start.shape) != (n + 1,) or neighbours.dtype != torch.int32 or neighbours.dim() != 1:
        raise ValueError(f"mesh_smooth: row_start int32 [{n + 1}] and neighbours int32 [n], got {tuple(row_start.shape)} "
                         f"{row_start.dtype} and {tuple(neighbours.shape)} {neighbours.dtype}")
    row_start, neighbours = row_start.contiguous(), neighbours.contiguous()
    scratch = torch.empty_like(v)
    info = torch.empty(4, device=dev, dtype=torch.int64)
    check(load().lnr_mesh_smooth(_ptr(v), _ptr(scratch), n, _ptr(row_start), _ptr(neighbours), neighbours.shape[0], MESH_SMOOTH_KINDS[kind], steps, lam, m,
                                 _ptr(info), _stream()), "lnr_mesh_smooth")
    _mesh_tools_info("mesh_smooth", info, _MESH_FILTERS_STATUS)
    return v
