"""Ray and point queries against triangle meshes on HIP: what a user of open3d's t.geometry.RaycastingScene calls to get the depth
of a mesh along rays - the "Depth L1" metric of the mesh-based SLAM literature, depth images of a ground-truth mesh, the scans of a
simulated LiDAR (analysis/lidar_sim.py) - and the distance from points to a mesh's surface, which is what the accuracy and the
completion of a map mean (analysis/mesh_eval.py: evaluate_mesh_to_mesh).

    scene = RaycastingScene(mesh)                       # a TriangleMesh, or (vertices, triangles)
    hit = scene.cast_rays(rays)                         # rays [...,6]: ox oy oz dx dy dz
    depth = scene.depth_image(camera_pose, CameraRayDirections(calibration))
    near = scene.compute_closest_points(points)         # points [...,3]
    d, sd = scene.compute_distance(points), scene.compute_signed_distance(points)
    inside, crossings = scene.compute_occupancy(points), scene.count_intersections(rays)

Everything is defined in include/loner_hip.h ("ray casting").  The hit of a ray: the watertight test of Woop, Benthin and Wald in
fp64, the smallest t, the smallest triangle index among equal t.  The closest point: Ericson's region walk in fp64, the smallest
squared distance, the smallest triangle index among equal ones.  Differences from open3d, by intent:
  * one mesh per scene (no add_triangles of further geometries, no instance ids);
  * fp64 throughout (open3d's Embree scene is fp32), and a [t_min, t_max] window;
  * primitive_uvs weigh the triangle's first and second corner (hit = u A + v B + (1 - u - v) C); open3d's weigh the second and third;
  * primitive_normals follow the stored winding and are zeros on a miss; a triangle without area has a zero normal;
  * compute_closest_points takes a reach (max_distance) and also returns the distance; ties go to the lower triangle index, where
    Embree's answer depends on its traversal;
  * compute_occupancy and compute_signed_distance count crossings along one or three fixed directions stated in the header, where
    open3d draws random ones: the answer is a function of the mesh and the point.  A ray through an edge two triangles share is
    counted by both; the vote of three directions exists for that case, and nsamples is 1 or 3.
"""
import math

import numpy as np
import torch

from .. import hip, ops
from .lidar_map import _device


class RaycastingScene:
    """A triangle mesh on the device with its BVH.  mesh_or_vertices: an object with .vertices and .triangles (TriangleMesh), or
    vertices [V,3] with triangles [F,3] (arrays or tensors).  .bvh is the ops.BVH; .vertices fp64 and .triangles int32 live on the
    device."""

    def __init__(self, mesh_or_vertices, triangles=None, device=None):
        if triangles is None:
            if not (hasattr(mesh_or_vertices, "vertices") and hasattr(mesh_or_vertices, "triangles")):
                raise ValueError("RaycastingScene: a mesh with .vertices and .triangles, or vertices and triangles")
            vertices, triangles = mesh_or_vertices.vertices, mesh_or_vertices.triangles
        else:
            vertices = mesh_or_vertices
        v = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.ascontiguousarray(vertices, dtype=np.float64))
        f = triangles if torch.is_tensor(triangles) else torch.from_numpy(np.ascontiguousarray(triangles))
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"RaycastingScene: vertices [V,3] and triangles [F,3], got {tuple(v.shape)} and {tuple(f.shape)}")
        if f.dtype.is_floating_point or f.dtype == torch.bool:
            raise ValueError(f"RaycastingScene: triangles must be integers, got {f.dtype}")
        if f.numel() and (int(f.max()) >= 2 ** 31 or int(f.min()) < -2 ** 31):
            raise ValueError("RaycastingScene: a triangle index does not fit int32")
        if device is None and v.is_cuda:
            dev = v.device
        else:
            dev = _device(device)
        self.vertices = v.to(device=dev, dtype=torch.float64).contiguous()
        self.triangles = f.to(device=dev, dtype=torch.int32).contiguous()
        self.bvh = ops.BVH(self.vertices, self.triangles)
        self._normals = None

    @property
    def device(self):
        return self.vertices.device

    def triangle_normals(self):
        """unit geometric normals [F,3] fp64 of the stored winding, (B - A) x (C - A) normalised; zeros for a triangle without area"""
        if self._normals is None:
            idx = self.triangles.long().clamp(0, max(self.vertices.shape[0] - 1, 0))
            if self.vertices.shape[0] == 0:
                self._normals = torch.zeros(self.triangles.shape[0], 3, dtype=torch.float64, device=self.device)
            else:
                a, b, c = (self.vertices[idx[:, k]] for k in range(3))
                n = torch.linalg.cross(b - a, c - a)
                length = torch.linalg.norm(n, dim=1, keepdim=True)
                n = torch.where(length > 0, n / length, torch.zeros_like(n))
                self._normals = torch.nan_to_num(n, nan=0.0, posinf=0.0, neginf=0.0)
        return self._normals

    def cast_rays(self, rays, t_min=0.0, t_max=math.inf, stats=None):
        """rays [...,6] (ox oy oz dx dy dz; any float dtype, host or device) -> {"t_hit" fp64 [...], +inf on a miss; "primitive_ids"
        int32 [...], -1 on a miss; "primitive_uvs" fp64 [...,2]; "primitive_normals" fp64 [...,3], zeros on a miss}, on the device.
        t is in units of the direction's length.  stats: ops.cast_rays' counters (one host read)."""
        r = rays if torch.is_tensor(rays) else torch.from_numpy(np.asarray(rays, dtype=np.float64))
        if r.dim() < 1 or r.shape[-1] != 6:
            raise ValueError(f"cast_rays: rays [...,6], got {tuple(r.shape)}")
        lead = tuple(r.shape[:-1])
        flat = r.to(device=self.device, dtype=torch.float64).reshape(-1, 6)
        t_hit, ids, uvs = ops.cast_rays(self.bvh, flat, t_min, t_max, stats=stats)
        hit = ids >= 0
        normals = self.triangle_normals()
        if normals.shape[0]:
            picked = normals[ids.long().clamp(min=0)] * hit[:, None].to(torch.float64)
        else:
            picked = torch.zeros(flat.shape[0], 3, dtype=torch.float64, device=self.device)
        return {"t_hit": t_hit.reshape(lead), "primitive_ids": ids.reshape(lead), "primitive_uvs": uvs.reshape(lead + (2,)),
                "primitive_normals": picked.reshape(lead + (3,))}

    def _points(self, points, what):
        """points [...,3] (any float dtype, host or device) -> (the leading shape, fp64 [n,3] on the device)"""
        p = points if torch.is_tensor(points) else torch.from_numpy(np.asarray(points, dtype=np.float64))
        if p.dim() < 1 or p.shape[-1] != 3 or not p.dtype.is_floating_point:
            raise ValueError(f"{what}: points [...,3] of a float dtype, got {tuple(p.shape)} {p.dtype}")
        return tuple(p.shape[:-1]), p.to(device=self.device, dtype=torch.float64).reshape(-1, 3)

    @staticmethod
    def _reach(max_distance, what):
        reach = float(max_distance)
        if math.isnan(reach) or reach < 0:
            raise ValueError(f"{what}: max_distance must be a number >= 0, got {max_distance!r}")
        return reach

    def compute_closest_points(self, points, max_distance=math.inf, stats=None):
        """points [...,3] -> {"points" fp64 [...,3]: the closest point of the surface; "primitive_ids" int32 [...]; "primitive_uvs"
        fp64 [...,2] (point = u A + v B + (1 - u - v) C); "primitive_normals" fp64 [...,3]; "distance" fp64 [...]}, on the device.
        With no triangle within max_distance: distance +inf, id -1, zeros elsewhere.  stats: ops.closest_points' counters (one host
        read)."""
        reach = self._reach(max_distance, "compute_closest_points")
        lead, flat = self._points(points, "compute_closest_points")
        dist_sq, ids, closest, uvs = ops.closest_points(self.bvh, flat, reach, stats=stats)
        found = ids >= 0
        normals = self.triangle_normals()
        if normals.shape[0]:
            picked = normals[ids.long().clamp(min=0)] * found[:, None].to(torch.float64)
        else:
            picked = torch.zeros(flat.shape[0], 3, dtype=torch.float64, device=self.device)
        return {"points": closest.reshape(lead + (3,)), "primitive_ids": ids.reshape(lead), "primitive_uvs": uvs.reshape(lead + (2,)),
                "primitive_normals": picked.reshape(lead + (3,)), "distance": dist_sq.sqrt().reshape(lead)}

    def compute_distance(self, points, max_distance=math.inf, stats=None):
        """points [...,3] -> the distance fp64 [...] to the surface, sqrt of the header's squared distance; +inf where no triangle lies
        within max_distance (and for a point that is not finite, or a mesh without usable triangles)"""
        reach = self._reach(max_distance, "compute_distance")
        lead, flat = self._points(points, "compute_distance")
        dist_sq, _, _, _ = ops.closest_points(self.bvh, flat, reach, want_points=False, want_uvs=False, stats=stats)
        return dist_sq.sqrt().reshape(lead)

    def count_intersections(self, rays, t_min=0.0, t_max=math.inf, stats=None):
        """rays [...,6] -> int32 [...]: the triangles each ray crosses with t_min <= t <= t_max (the watertight rule; a ray through a
        shared edge is counted by both triangles)"""
        r = rays if torch.is_tensor(rays) else torch.from_numpy(np.asarray(rays, dtype=np.float64))
        if r.dim() < 1 or r.shape[-1] != 6 or not r.dtype.is_floating_point:
            raise ValueError(f"count_intersections: rays [...,6] of a float dtype, got {tuple(r.shape)} {r.dtype}")
        lo, hi = float(t_min), float(t_max)
        if math.isnan(lo) or math.isnan(hi):
            raise ValueError(f"count_intersections: t_min and t_max must be numbers, got {t_min!r} and {t_max!r}")
        flat = r.to(device=self.device, dtype=torch.float64).reshape(-1, 6)
        return ops.count_intersections(self.bvh, flat, lo, hi, stats=stats).reshape(tuple(r.shape[:-1]))

    def compute_occupancy(self, points, nsamples=3, stats=None):
        """points [...,3] -> fp64 [...]: 1.0 inside the (closed) mesh, 0.0 outside.  nsamples = 1: the crossing count along the
        header's first direction is odd; 3: at least two of its three directions give an odd count.  The directions are fixed
        (hip.OCCUPANCY_DIRECTIONS), so the answer does not change from run to run.  stats: the summed counters of the casts."""
        if isinstance(nsamples, bool) or nsamples not in (1, 3):
            raise ValueError(f"compute_occupancy: nsamples must be 1 or 3, got {nsamples!r}")
        lead, flat = self._points(points, "compute_occupancy")
        odd = torch.zeros(flat.shape[0], dtype=torch.int32, device=self.device)
        for direction in hip.OCCUPANCY_DIRECTIONS[:nsamples]:
            d = torch.tensor(direction, dtype=torch.float64, device=self.device).expand_as(flat)
            part = {} if stats is not None else None
            odd += ops.count_intersections(self.bvh, torch.cat([flat, d], dim=1), 0.0, math.inf, stats=part) & 1
            if stats is not None:
                for key, value in part.items():
                    stats[key] = value if key == "depth" else stats.get(key, 0) + value
        return (2 * odd > nsamples).to(torch.float64).reshape(lead)

    def compute_signed_distance(self, points, nsamples=3):
        """points [...,3] -> fp64 [...]: compute_distance, negative where compute_occupancy(points, nsamples) is 1"""
        if isinstance(nsamples, bool) or nsamples not in (1, 3):
            raise ValueError(f"compute_signed_distance: nsamples must be 1 or 3, got {nsamples!r}")
        lead, flat = self._points(points, "compute_signed_distance")
        inside = self.compute_occupancy(flat, nsamples)
        return (self.compute_distance(flat) * (1.0 - 2.0 * inside)).reshape(lead)

    def camera_rays(self, camera_pose, ray_directions):
        """The rays [H*W,6] fp64 of a camera: origin = the pose's translation, direction = its rotation applied to the camera-frame
        direction of every pixel (CameraRayDirections.directions, widened to fp64; not re-normalised)."""
        T = camera_pose.get_transformation_matrix() if hasattr(camera_pose, "get_transformation_matrix") else torch.as_tensor(camera_pose)
        T = T.detach().to(device=self.device, dtype=torch.float64)
        if tuple(T.shape) != (4, 4):
            raise ValueError(f"depth_image: camera_pose must be a 4x4 transform, got {tuple(T.shape)}")
        d = ray_directions.directions.to(device=self.device, dtype=torch.float64)
        world = (d[:, 0:1] * T[:3, 0] + d[:, 1:2] * T[:3, 1]) + d[:, 2:3] * T[:3, 2]
        return torch.cat([T[:3, 3].expand_as(world), world], dim=1).contiguous()

    def depth_image(self, camera_pose, ray_directions):
        """-> depth [1,1,H,W] fp64 in metres: the distance from the camera centre to the mesh along every pixel's ray (t times the
        direction's length), +inf where the ray leaves the mesh untouched.  save_depth / depth_to_rgba (analysis/renderer.py) colour
        it as they colour a rendered map's."""
        rays = self.camera_rays(camera_pose, ray_directions)
        t_hit, _, _ = ops.cast_rays(self.bvh, rays, 0.0, math.inf, want_uvs=False)
        depth = t_hit * torch.linalg.norm(rays[:, 3:], dim=1)
        return depth.reshape(1, 1, ray_directions.im_height, ray_directions.im_width)
