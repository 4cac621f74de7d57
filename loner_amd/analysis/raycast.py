"""Ray casting against triangle meshes on HIP: what a user of open3d's t.geometry.RaycastingScene calls to get the depth of a mesh
along rays - the "Depth L1" metric of the mesh-based SLAM literature, depth images of a ground-truth mesh, and the scans of a
simulated LiDAR (analysis/lidar_sim.py).

    scene = RaycastingScene(mesh)                       # a TriangleMesh, or (vertices, triangles)
    hit = scene.cast_rays(rays)                         # rays [...,6]: ox oy oz dx dy dz
    depth = scene.depth_image(camera_pose, CameraRayDirections(calibration))

The hit of a ray is defined in include/loner_hip.h ("ray casting"): the watertight test of Woop, Benthin and Wald in fp64, the
smallest t, the smallest triangle index among equal t.  Differences from open3d, by intent:
  * one mesh per scene (no add_triangles of further geometries, no instance ids);
  * fp64 throughout (open3d's Embree scene is fp32), and a [t_min, t_max] window;
  * primitive_uvs weigh the triangle's first and second corner (hit = u A + v B + (1 - u - v) C); open3d's weigh the second and third;
  * primitive_normals follow the stored winding and are zeros on a miss; a triangle without area has a zero normal.
"""
import math

import numpy as np
import torch

from .. import ops
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
