"""Mesh of a trained map (the reference's analysis/mesher.py:29-225), on HIP.

Mesher.get_mesh renders every `skip_step`-th keyframe pose with a full synthetic LiDAR scan, max-accumulates the rendered weights
of all samples into a lattice over `marching_cubes_bound` (Model.mesh_accumulate: one kernel composites and accumulates, nothing
per sample reaches memory), and runs marching cubes on the device (ops.marching_cubes).  Differences from the reference, by intent:
  * the volume holds the true max of the weights that fall into a voxel; the reference's `results[idx] = torch.max(results[idx], w)`
    (mesher.py:180) keeps the LAST writer among samples of one chunk that share a voxel;
  * marching cubes is this project's (include/loner_hip.h, "meshing"), not scikit-image's Lewiner tables: the vertices lie on the same
    lattice edges at the same interpolated positions, the triangulation of a cell can differ;
  * the result is a small TriangleMesh (vertices, triangles, vertex normals, .ply output), not an open3d object.
The reference's quirks are kept: a ray counts when its rendered depth in world-cube units is below ray_range[1] - 0.25 in metres
(mesher.py:144), the bound check compares in fp32 and the bucketing in fp64, and bucket indices that alias into the next row stay.
"""
import numpy as np
import torch

from .. import ops
from ..common.pose import Pose
from ..common.ray_utils import LidarRayDirections
from ..common.sensors import LidarScan


def build_lidar_scan(lidar_intrinsics, device=0):
    """A full synthetic scan: unit directions over vertical_fov x 360 deg at the given resolutions (mesher.py:29-50)."""
    vert_fov = lidar_intrinsics["vertical_fov"]
    vert_res = lidar_intrinsics["vertical_resolution"]
    hor_res = lidar_intrinsics["horizontal_resolution"]
    phi = torch.arange(vert_fov[0], vert_fov[1], vert_res).deg2rad()
    theta = torch.arange(0, 360, hor_res).deg2rad()
    phi_grid, theta_grid = torch.meshgrid(phi, theta, indexing="ij")
    phi_grid = torch.pi / 2 - phi_grid.reshape(-1, 1)
    theta_grid = theta_grid.reshape(-1, 1)
    x = torch.cos(theta_grid) * torch.sin(phi_grid)
    y = torch.sin(theta_grid) * torch.sin(phi_grid)
    z = torch.cos(phi_grid)
    xyz = torch.hstack((x, y, z))
    return LidarScan(xyz.T, torch.ones_like(x).flatten(), torch.zeros_like(x).flatten()).to(device)


def select_components(sizes, min_triangles=None, keep_largest=None, areas=None, min_area=None):
    """The clusters TriangleMesh.remove_small_components keeps, a bool array [C], from their triangle counts (and areas)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    keep = np.ones(sizes.shape[0], dtype=bool)
    if min_triangles is not None:
        keep &= sizes >= int(min_triangles)
    if min_area is not None:
        keep &= np.asarray(areas, dtype=np.float64) >= float(min_area)
    if keep_largest is not None:
        order = np.argsort(-sizes, kind="stable")               # most triangles first; a tie goes to the lower cluster id
        order = order[keep[order]][:int(keep_largest)]
        keep = np.zeros_like(keep)
        keep[order] = True
    return keep


def _simplify_on_device(vertices, triangles, voxel_size):
    """TriangleMesh.simplify_vertex_clustering on device tensors -> (vertices fp64 [m,3], triangles int32 [F',3])"""
    cluster, means = ops.mesh_vertex_clusters(vertices, voxel_size)
    canonical, keep, _, _ = ops.mesh_unique_triangles(triangles, vertices.shape[0], vertex_map=cluster, n_mapped=means.shape[0],
                                                      drop_degenerate=True)
    return means, ops.mesh_select(canonical, means.shape[0], triangle_keep=keep)[0]


def _smooth_on_device(vertices, triangles, n_steps, kind="laplacian", lambda_filter=0.5, mu=-0.53):
    """The TriangleMesh.filter_smooth_* calls on device tensors (the defaults: Taubin's factors) -> vertices fp64 [V,3]"""
    row_start, neighbours = ops.mesh_vertex_adjacency(triangles, vertices.shape[0])
    return ops.mesh_smooth(vertices, row_start, neighbours, n_steps, kind, lambda_filter, mu)


class TriangleMesh:
    """vertices float64 [V,3] (world frame, metres), triangles int32 [F,3]; what the reference's script uses of open3d's mesh."""

    def __init__(self, vertices, triangles):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64)
        self.triangles = np.ascontiguousarray(triangles, dtype=np.int32)
        self.vertex_normals = np.zeros((0, 3), dtype=np.float64)

    def has_vertex_normals(self):
        return self.vertex_normals.shape[0] == self.vertices.shape[0] and self.vertices.shape[0] > 0

    def compute_vertex_normals(self, device=None):
        """Area-weighted sum of the adjacent triangles' normals, normalised (triangles face lower weights: out of the surface).
        device given: the same bytes from the device (include/loner_hip.h: lnr_mesh_vertex_normals); None: numpy on the host."""
        if device is not None:
            v, t = self._device_arrays(device)
            self.vertex_normals = ops.mesh_vertex_normals(v, t).cpu().numpy()
            return self
        v, t = self.vertices, self.triangles.astype(np.int64)
        fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        n = np.zeros_like(v)
        for k in range(3):
            np.add.at(n, t[:, k], fn)
        norm = np.linalg.norm(n, axis=1, keepdims=True)
        self.vertex_normals = n / np.where(norm > 0, norm, 1.0)
        return self

    def _device_arrays(self, device):
        from .lidar_map import _device
        dev = _device(device)
        return torch.tensor(self.vertices, device=dev), torch.tensor(self.triangles, device=dev)

    # ------------------------------------------------------------ clean-up (include/loner_hip.h, "mesh tools")
    def cluster_connected_triangles(self, device=None):
        """open3d's cluster_connected_triangles: (triangle_clusters int32 [F], cluster_n_triangles int32 [C], cluster_area float64 [C])
        as numpy arrays.  Triangles sharing an edge are connected; clusters are numbered by their smallest triangle."""
        v, t = self._device_arrays(device)
        clusters, sizes = ops.mesh_connected_triangles(t, v.shape[0])
        area = ops.mesh_cluster_area(v, t, clusters, sizes.shape[0])
        return clusters.cpu().numpy(), sizes.cpu().numpy(), area.cpu().numpy()

    def _mask(self, mask, n, what):
        m = np.asarray(mask)
        if m.shape != (n,) or not (m.dtype == np.bool_ or np.issubdtype(m.dtype, np.integer)):
            raise ValueError(f"{what}: a bool mask of shape ({n},), got {m.dtype} {m.shape}")
        return m.astype(bool)

    def _select(self, triangle_keep=None, vertex_keep=None, drop_unreferenced=False, device=None):
        """lnr_mesh_select applied in place: the surviving triangles re-indexed, vertices and normals compacted in their order"""
        from .lidar_map import _device
        dev = _device(device)
        up = lambda m: None if m is None else torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8)).to(dev)
        tris, vmap, n_v = ops.mesh_select(torch.from_numpy(self.triangles).to(dev), self.vertices.shape[0], up(triangle_keep),
                                          up(vertex_keep), drop_unreferenced)
        kept = vmap.cpu().numpy() >= 0
        assert int(kept.sum()) == n_v
        normals = self.has_vertex_normals()
        self.triangles = np.ascontiguousarray(tris.cpu().numpy())
        if normals:
            self.vertex_normals = np.ascontiguousarray(self.vertex_normals[kept])
        self.vertices = np.ascontiguousarray(self.vertices[kept])
        return self

    def remove_triangles_by_mask(self, mask, device=None):
        """open3d's remove_triangles_by_mask: drops the triangles whose mask entry is set.  In place; returns self."""
        return self._select(triangle_keep=~self._mask(mask, self.triangles.shape[0], "remove_triangles_by_mask"), device=device)

    def remove_vertices_by_mask(self, mask, device=None):
        """open3d's remove_vertices_by_mask: drops the vertices whose mask entry is set and the triangles that use one.  In place."""
        return self._select(vertex_keep=~self._mask(mask, self.vertices.shape[0], "remove_vertices_by_mask"), device=device)

    def remove_unreferenced_vertices(self, device=None):
        """open3d's remove_unreferenced_vertices: drops the vertices no triangle uses.  In place; returns self."""
        return self._select(drop_unreferenced=True, device=device)

    def remove_degenerate_triangles(self, device=None):
        """open3d's remove_degenerate_triangles: drops the triangles with a repeated vertex index.  In place; returns self."""
        t = self.triangles
        return self._select(triangle_keep=(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0]), device=device)

    def crop(self, min_bound, max_bound, device=None):
        """open3d's crop with an axis-aligned box: a new mesh of the vertices inside the closed box [min_bound, max_bound] and the
        triangles whose three vertices are inside."""
        lo, hi = np.asarray(min_bound, dtype=np.float64), np.asarray(max_bound, dtype=np.float64)
        if lo.shape != (3,) or hi.shape != (3,) or not (lo <= hi).all():
            raise ValueError(f"crop: min_bound <= max_bound, three numbers each, got {min_bound!r} and {max_bound!r}")
        out = TriangleMesh(self.vertices, self.triangles)
        out.vertex_normals = self.vertex_normals.copy()
        return out._select(vertex_keep=((self.vertices >= lo) & (self.vertices <= hi)).all(1), device=device)

    def remove_small_components(self, min_triangles=None, min_area=None, keep_largest=None, device=None):
        """Drops the connected components (cluster_connected_triangles) with fewer than min_triangles triangles or less than min_area
        area, then, with keep_largest = k, all but the k remaining ones with the most triangles (ties: the lower cluster id), and the
        vertices left without a triangle.  In place; returns the number of triangles removed."""
        if min_triangles is None and min_area is None and keep_largest is None:
            raise ValueError("remove_small_components: give min_triangles, min_area or keep_largest")
        if min_triangles is not None and (int(min_triangles) != min_triangles or min_triangles < 0):
            raise ValueError(f"remove_small_components: min_triangles must be an integer >= 0, got {min_triangles!r}")
        if min_area is not None and not float(min_area) >= 0.0:
            raise ValueError(f"remove_small_components: min_area must be >= 0, got {min_area!r}")
        if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 1):
            raise ValueError(f"remove_small_components: keep_largest must be an integer >= 1, got {keep_largest!r}")
        v, t = self._device_arrays(device)
        clusters, sizes = ops.mesh_connected_triangles(t, v.shape[0])
        keep = select_components(sizes.cpu().numpy(), min_triangles, keep_largest,
                                 ops.mesh_cluster_area(v, t, clusters, sizes.shape[0]).cpu().numpy() if min_area is not None else None,
                                 min_area)
        before = self.triangles.shape[0]
        self._select(triangle_keep=keep[clusters.cpu().numpy()], drop_unreferenced=True, device=device)
        return before - self.triangles.shape[0]

    # ------------------------------------------------------------ simplification and smoothing (include/loner_hip.h)
    def simplify_vertex_clustering(self, voxel_size, device=None):
        """open3d's simplify_vertex_clustering with averaging: a new mesh whose vertices are the means of the vertices sharing a
        voxel of edge voxel_size, in the order the voxels are first met, and whose triangles are the distinct non-degenerate ones
        left after the merge, each rotated to open3d's canonical corner order, in the order of their first input triangle.  No
        vertex normals: recompute them."""
        s = float(voxel_size)
        if not (np.isfinite(s) and s > 0):
            raise ValueError(f"simplify_vertex_clustering: voxel_size must be finite and > 0, got {voxel_size!r}")
        v, t = self._device_arrays(device)
        v, t = _simplify_on_device(v, t, s)
        return TriangleMesh(v.cpu().numpy(), t.cpu().numpy())

    def remove_duplicated_triangles(self, device=None):
        """open3d's remove_duplicated_triangles: of the triangles with the same corners in the same cyclic order the first stays;
        order, corner order and vertex normals are kept, degenerate triangles are treated like any other.  In place; returns self."""
        from .lidar_map import _device
        t = torch.from_numpy(self.triangles).to(_device(device))
        _, keep, _, _ = ops.mesh_unique_triangles(t, self.vertices.shape[0])
        self.triangles = np.ascontiguousarray(self.triangles[keep.cpu().numpy().astype(bool)])
        return self

    def _smoothed(self, what, kind, number_of_iterations, steps_per_iteration, lambda_filter, mu, device):
        if int(number_of_iterations) != number_of_iterations or number_of_iterations < 0:
            raise ValueError(f"{what}: number_of_iterations must be an integer >= 0, got {number_of_iterations!r}")
        v, t = self._device_arrays(device)
        out = _smooth_on_device(v, t, steps_per_iteration * int(number_of_iterations), kind, lambda_filter, mu)
        return TriangleMesh(out.cpu().numpy(), self.triangles)

    def filter_smooth_simple(self, number_of_iterations=1, device=None):
        """open3d's filter_smooth_simple: every vertex becomes the mean of itself and its neighbours, number_of_iterations times.
        A new mesh with the same triangles and no vertex normals."""
        return self._smoothed("filter_smooth_simple", "simple", number_of_iterations, 1, 0.0, None, device)

    def filter_smooth_laplacian(self, number_of_iterations=1, lambda_filter=0.5, device=None):
        """open3d's filter_smooth_laplacian (inverse-distance weights): v + lambda_filter * (weighted mean of the neighbours - v),
        number_of_iterations times.  A new mesh with the same triangles and no vertex normals."""
        return self._smoothed("filter_smooth_laplacian", "laplacian", number_of_iterations, 1, lambda_filter, None, device)

    def filter_smooth_taubin(self, number_of_iterations=1, lambda_filter=0.5, mu=-0.53, device=None):
        """open3d's filter_smooth_taubin: per iteration one Laplacian step with lambda_filter and one with mu, which keeps the
        volume a plain Laplacian filter loses.  A new mesh with the same triangles and no vertex normals."""
        return self._smoothed("filter_smooth_taubin", "laplacian", number_of_iterations, 2, lambda_filter, mu, device)

    def sample_points_uniformly(self, number_of_points, seed=0, device=None, return_triangles=False):
        """open3d's sample_points_uniformly on the device (include/loner_hip.h: lnr_mesh_sample_points): a PointCloud of
        number_of_points points, each triangle owning its area's share of them (the stratified rule), from counter-based draws:
        the cloud depends on (mesh, number_of_points, seed) only.  return_triangles: also the owning triangle of every point (int32
        tensor on the device).  A mesh without triangles or area gives an empty cloud; open3d raises there."""
        from .lidar_map import PointCloud
        n = int(number_of_points)
        if n <= 0:
            raise ValueError(f"sample_points_uniformly: number_of_points must be > 0, got {number_of_points!r}")
        v, t = self._device_arrays(device)
        out = ops.mesh_sample_points(v, t, n, seed, want_triangles=return_triangles)
        return (PointCloud(out[0]), out[1]) if return_triangles else PointCloud(out)

    def get_surface_area(self, device=None):
        """The sum of the triangle areas in the order the sampler's cumulative area takes (include/loner_hip.h)."""
        v, t = self._device_arrays(device)
        info = {}
        ops.mesh_sample_points(v, t, 0, 0, info=info)
        return info["area"]

    def write_ply(self, path, binary=True):
        """PLY with float64 x y z (+ nx ny nz when computed) and int32 vertex_indices lists."""
        normals = self.has_vertex_normals()
        props = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else [])
        fmt = "binary_little_endian" if binary else "ascii"
        head = [f"ply", f"format {fmt} 1.0", f"element vertex {self.vertices.shape[0]}"] + [f"property double {p}" for p in props] + \
            [f"element face {self.triangles.shape[0]}", "property list uchar int vertex_indices", "end_header"]
        vdata = np.hstack([self.vertices, self.vertex_normals]) if normals else self.vertices
        with open(path, "wb") as f:
            f.write(("\n".join(head) + "\n").encode("ascii"))
            if binary:
                f.write(np.ascontiguousarray(vdata, dtype="<f8").tobytes())
                faces = np.zeros(self.triangles.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
                faces["n"] = 3
                faces["i"] = self.triangles
                f.write(faces.tobytes())
            else:
                for row in vdata:
                    f.write((" ".join(repr(float(x)) for x in row) + "\n").encode("ascii"))
                for tri in self.triangles:
                    f.write(f"3 {tri[0]} {tri[1]} {tri[2]}\n".encode("ascii"))

    @staticmethod
    def read_ply(path):
        """Reads what write_ply writes (both formats)."""
        with open(path, "rb") as f:
            lines = []
            while True:
                line = f.readline().decode("ascii").strip()
                lines.append(line)
                if line == "end_header":
                    break
            nv = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
            nf = int(next(l for l in lines if l.startswith("element face")).split()[-1])
            ncol = sum(1 for l in lines if l.startswith("property double"))
            if "format binary_little_endian 1.0" in lines:
                vdata = np.frombuffer(f.read(nv * ncol * 8), dtype="<f8").reshape(nv, ncol)
                faces = np.frombuffer(f.read(nf * 13), dtype=[("n", "u1"), ("i", "<i4", (3,))])
                tris = faces["i"].copy()
            else:
                rows = f.read().decode("ascii").split("\n")
                vdata = np.array([[float(x) for x in r.split()] for r in rows[:nv]], dtype=np.float64).reshape(nv, ncol)
                tris = np.array([[int(x) for x in r.split()[1:4]] for r in rows[nv:nv + nf]], dtype=np.int32).reshape(nf, 3)
        mesh = TriangleMesh(vdata[:, :3], tris)
        if ncol == 6:
            mesh.vertex_normals = vdata[:, 3:6].copy()
        return mesh


class Mesher(object):
    def __init__(self, model, ckpt, world_cube, ray_range, resolution=0.2, marching_cubes_bound=[[-40, 20], [0, 20], [-3, 15]],
                 level_set=0, points_batch_size=5000000, lidar_vertical_fov=[-22.5, 22.5]):
        self.marching_cubes_bound = np.array(marching_cubes_bound)
        self.world_cube_shift = world_cube.shift.cpu().numpy()
        self.world_cube_scale_factor = world_cube.scale_factor.cpu().numpy()
        self.world_cube = world_cube
        self.model = model
        self.ckpt = ckpt
        self.resolution = resolution
        self.points_batch_size = points_batch_size          # (kept for the signature: the lattice is never materialised as points)
        self.level_set = level_set
        self.ray_range = ray_range
        self.lidar_vertical_fov = lidar_vertical_fov

    def _bound(self):
        """the lattice's bound in world-cube units, float64 [3,2] (mesher.py:141)"""
        return (np.array(self.marching_cubes_bound) + np.expand_dims(self.world_cube_shift, 1)) / self.world_cube_scale_factor

    def get_grid_uniform(self, resolution):
        """{"xyz": [x, y, z]}: the lattice axes of mesher.py:60-90 (np.linspace over the bound in world-cube units).  The reference also
        returns every lattice point ("grid_points", 1.2 GB at 0.1 m); nothing here needs them."""
        bound = self._bound()
        length = self.marching_cubes_bound[:, 1] - self.marching_cubes_bound[:, 0]
        num = (length / resolution).astype(int)
        x = np.linspace(bound[0][0], bound[0][1], num[0])
        y = np.linspace(bound[1][0], bound[1][1], num[1])
        z = np.linspace(bound[2][0], bound[2][1], num[2])
        return {"xyz": [x, y, z]}

    def get_volume(self, device, ray_sampler, skip_step=15, var_threshold=None, counters=None):
        """-> (volume [nx, ny, nz] fp32 on `device`, axes): the reference's `volume` (mesher.py:182-184)."""
        device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        grid = self.get_grid_uniform(self.resolution)
        lattice = ops.MeshLattice(grid["xyz"], self._bound(), device)
        nx, ny, nz = lattice.shape
        results = torch.zeros(ny * nx * nz, device=device, dtype=torch.float32)
        scan = build_lidar_scan({"vertical_fov": self.lidar_vertical_fov, "vertical_resolution": 0.25, "horizontal_resolution": 0.25},
                                device)
        ray_directions = LidarRayDirections(scan)
        depth_max = float(self.ray_range[1]) - 0.25
        all_rays = torch.arange(len(ray_directions))
        for pose_state in self.ckpt["poses"][::skip_step]:
            lidar_pose = Pose(pose_tensor=pose_state["lidar_pose"]).to(device)
            # every ray of the scan at once: the reference's 512-ray chunks (fetch_chunk_rays) concatenated
            rays = ray_directions.build_lidar_rays(all_rays, self.ray_range, self.world_cube, lidar_pose.get_transformation_matrix())[0]
            self.model.mesh_accumulate(rays, ray_sampler, lattice, results, depth_max, var_threshold, counters=counters)
        volume = results.view(ny, nx, nz).permute(1, 0, 2).contiguous()
        return volume, grid["xyz"]

    def get_mesh(self, device, ray_sampler, skip_step=15, var_threshold=None, min_component_triangles=None, smooth_iterations=None,
                 simplify_voxel_size=None):
        """TriangleMesh in world coordinates (metres), or None when no surface crosses level_set (mesher.py:103-225).
        min_component_triangles = k: connected components of fewer than k triangles are dropped on the device before the download
        (the mesh get_mesh() followed by remove_small_components(min_triangles=k) gives).
        smooth_iterations = n, simplify_voxel_size = s (metres): after that filter the mesh is converted to metres, smoothed and
        simplified on the device and downloaded once; the result is, bit for bit, get_mesh() followed by filter_smooth_taubin(n)
        and simplify_vertex_clustering(s)."""
        if smooth_iterations is not None and (int(smooth_iterations) != smooth_iterations or smooth_iterations < 0):
            raise ValueError(f"get_mesh: smooth_iterations must be an integer >= 0, got {smooth_iterations!r}")
        if simplify_voxel_size is not None and not (np.isfinite(float(simplify_voxel_size)) and float(simplify_voxel_size) > 0):
            raise ValueError(f"get_mesh: simplify_voxel_size must be finite and > 0, got {simplify_voxel_size!r}")
        if min_component_triangles is not None and (int(min_component_triangles) != min_component_triangles or min_component_triangles < 0):
            raise ValueError(f"get_mesh: min_component_triangles must be an integer >= 0, got {min_component_triangles!r}")
        with torch.no_grad():
            volume, xyz = self.get_volume(device, ray_sampler, skip_step, var_threshold)
            spacing = (xyz[0][2] - xyz[0][1], xyz[1][2] - xyz[1][1], xyz[2][2] - xyz[2][1])
            verts, faces = ops.marching_cubes(volume, float(self.level_set), spacing=spacing)
            if faces.shape[0] == 0:
                print('marching_cubes error. Possibly no surface extracted from the level set.')
                return None
            if min_component_triangles is not None:
                clusters, sizes = ops.mesh_connected_triangles(faces, verts.shape[0])
                faces, vertex_map, _ = ops.mesh_select(faces, verts.shape[0], triangle_keep=(sizes >= int(min_component_triangles))[clusters.long()],
                                                       drop_unreferenced=True)
                verts = verts[vertex_map >= 0]
            if smooth_iterations is not None or simplify_voxel_size is not None:
                # the conversion below, on the device: the same three fp64 operations per coordinate in the same order
                vertices = verts.to(torch.float64) + torch.tensor([xyz[0][0], xyz[1][0], xyz[2][0]], device=verts.device, dtype=torch.float64)
                vertices *= torch.tensor(self.world_cube_scale_factor, device=verts.device).to(torch.float64)
                vertices -= torch.tensor(self.world_cube_shift, device=verts.device).to(torch.float64)
                if smooth_iterations is not None:
                    vertices = _smooth_on_device(vertices, faces, 2 * int(smooth_iterations))
                if simplify_voxel_size is not None:
                    vertices, faces = _simplify_on_device(vertices, faces, float(simplify_voxel_size))
                return TriangleMesh(vertices.cpu().numpy(), faces.cpu().numpy())
            # convert back to world coordinates (mesher.py:214-219), in float64 as numpy does it there
            vertices = verts.cpu().numpy() + np.array([xyz[0][0], xyz[1][0], xyz[2][0]])
            vertices *= self.world_cube_scale_factor
            vertices -= self.world_cube_shift
            return TriangleMesh(vertices, faces.cpu().numpy())
