"""TSDF fusion of LiDAR scans on HIP: the classical map to hold a trained one against, what a user of open3d would look for beside
RaycastingScene (open3d.pipelines.integration.UniformTSDFVolume, for range rays instead of depth images).

    volume = TSDFVolume(min_bound, max_bound, voxel_size=0.1)
    volume.integrate_scan(scan, pose=T)                       # a LidarScan or (xyz [n,3], timestamps [n]); one 4x4 pose ...
    volume.integrate_scan(scan, trajectory=traj)              # ... or an ops.Trajectory: every ray leaves from the pose at its own time
    mesh = volume.extract_mesh(min_count=2)                   # a TriangleMesh (analysis/mesher.py), or None
    volume = fuse_scans(scans, "gt_tum.txt", bound, 0.1)      # the scans and the trajectory as gt_map.build_lidar_map takes them

Fused along the ground-truth trajectory the mesh shows what geometry the scans support at that resolution; fused along an estimated
trajectory it shows what the tracking costs (examples/run_sequence.py --tsdf-baseline).

Everything is defined in include/loner_hip.h ("TSDF fusion").  Every ray walks the voxels of [max(0, r - front), r + trunc] along
itself (Amanatides and Woo) and adds its truncated projective distance to the node of each voxel, as an integer: a volume is a
function of the set of rays, whatever their order, and the same on every run.  The mesh comes from the marching cubes of the
neural mesher, restricted to cells all of whose corners were observed (ops.marching_cubes(valid=...)).  By intent there are no
per-ray weights, weight caps or decay, no colour, no hash table, and the distance is the projective one.

    volume = SparseTSDFVolume(min_bound, max_bound, voxel_size=0.1)      # the same lattice, of any size: 2^21 nodes per axis
    volume = fuse_scans(scans, "gt_tum.txt", bound, 0.1, sparse=True)

SparseTSDFVolume (open3d's ScalableTSDFVolume / VoxelBlockGrid; include/loner_hip.h, "sparse TSDF") is the dense volume of which only
the 8 x 8 x 8 blocks a ray wrote to are stored: every node has the dense volume's sum and count bit for bit, and the mesh is the
dense one's as a set of triangles.  The directory of blocks is a sorted array that is searched, not hashed; blocks are never freed;
the pool grows by copy.
"""
import math

import numpy as np
import torch

from .. import ops
from . import tsdf_sparse as sparse_ops
from .gt_map import trajectory_arrays
from .lidar_map import _device
from .mesher import TriangleMesh

MAX_RAYS = (1 << 32) - 1        # a ray updates a node at most once, so the total bounds every node's uint32 count


def _lattice_arguments(name, min_bound, max_bound, voxel_size, sdf_trunc, front):
    """the argument checks and the lattice rule both volumes share -> (min_bound fp64 [3], voxel_size, sdf_trunc, front, cells per axis)"""
    lo, hi = np.asarray(min_bound, dtype=np.float64), np.asarray(max_bound, dtype=np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError(f"{name}: min_bound < max_bound, three finite numbers each, got {min_bound!r} and {max_bound!r}")
    v = float(voxel_size)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name}: voxel_size must be finite and > 0, got {voxel_size!r}")
    trunc = 3.0 * v if sdf_trunc is None else float(sdf_trunc)
    if not (math.isfinite(trunc) and trunc > 0):
        raise ValueError(f"{name}: sdf_trunc must be finite and > 0, got {sdf_trunc!r}")
    fr = trunc if front is None else float(front)
    if not fr >= trunc:
        raise ValueError(f"{name}: front must be at least sdf_trunc ({trunc}), got {front!r}")
    return lo, v, trunc, fr, np.ceil((hi - lo) / v - 1e-9)


class _ScanFusion:
    """What the dense and the sparse volume share: a scan becomes rays [n,6] and ranges [n] for the volume's integrate_rays."""

    def _check_rays(self, rays, ranges):
        """integrate_rays' argument checks -> n"""
        for name, t in (("rays", rays), ("ranges", ranges)):
            if not torch.is_tensor(t):
                raise ValueError(f"integrate_rays: {name} must be a tensor, got {type(t).__name__}")
            if not t.is_cuda:
                raise RuntimeError(f"integrate_rays: {name} on {t.device}; TSDF fusion has no CPU implementation")
        if rays.dim() != 2 or rays.shape[1] != 6 or not rays.dtype.is_floating_point:
            raise ValueError(f"integrate_rays: rays [n,6] of a float dtype, got {tuple(rays.shape)} {rays.dtype}")
        n = int(rays.shape[0])
        if tuple(ranges.shape) != (n,) or not ranges.dtype.is_floating_point:
            raise ValueError(f"integrate_rays: ranges [{n}] of a float dtype, got {tuple(ranges.shape)} {ranges.dtype}")
        if self.n_rays + n > MAX_RAYS:
            raise ValueError(f"integrate_rays: {self.n_rays} rays integrated and {n} more, the limit is 2^32 - 1 (the counts are uint32)")
        return n

    @staticmethod
    def _check_component_filter(min_component_triangles):
        if min_component_triangles is not None and (int(min_component_triangles) != min_component_triangles or min_component_triangles < 0):
            raise ValueError(f"extract_mesh: min_component_triangles must be an integer >= 0, got {min_component_triangles!r}")

    @staticmethod
    def _finish_mesh(verts, faces, min_component_triangles):
        """marching cubes' output on the device -> extract_mesh's TriangleMesh or None"""
        if faces.shape[0] == 0:
            return None
        keep = None
        if min_component_triangles is not None:
            clusters, sizes = ops.mesh_connected_triangles(faces, verts.shape[0])
            keep = (sizes >= int(min_component_triangles))[clusters.long()]
        faces, vertex_map, _ = ops.mesh_select(faces, verts.shape[0], triangle_keep=keep, drop_unreferenced=True)
        if faces.shape[0] == 0:
            return None
        return TriangleMesh(verts[vertex_map >= 0].cpu().numpy(), faces.cpu().numpy())

    def integrate_scan(self, scan, pose=None, trajectory=None):
        """scan: a LidarScan (ray_directions fp32 [3,n], distances [n], timestamps [n]) or a pair (xyz [n,3], timestamps [n]) in the
        sensor frame, as gt_map.build_lidar_map takes its scans (absolute times; None with a pose).  Exactly one of
          pose        a 4x4 transform (tensor, array or Pose): the whole scan leaves from it;
          trajectory  an ops.Trajectory: every ray leaves from the pose at its own timestamp (ops.trajectory_rays), which undoes the
                      motion distortion; as in build_lidar_map a scan with a ray outside the trajectory's time span is skipped whole
                      ({"skipped": True} in the counters) and a direction or time that is not finite raises ValueError.
        -> integrate_rays' counters."""
        if (pose is None) == (trajectory is None):
            raise ValueError("integrate_scan: give exactly one of pose and trajectory")
        dirs, dist, stamps = self._scan_arrays(scan)
        if pose is not None:
            T = pose.get_transformation_matrix() if hasattr(pose, "get_transformation_matrix") else torch.as_tensor(pose)
            T = T.detach().to(device=self.device, dtype=torch.float64)
            if tuple(T.shape) != (4, 4) or not bool(torch.isfinite(T).all()):
                raise ValueError(f"integrate_scan: pose must be a finite 4x4 transform, got {tuple(T.shape)}")
            d = dirs.to(torch.float64)
            world = torch.stack([(T[a, 0] * d[0] + T[a, 1] * d[1]) + T[a, 2] * d[2] for a in range(3)], dim=1)
            rays = torch.cat([T[:3, 3].expand_as(world), world], dim=1).contiguous()
        else:
            if not isinstance(trajectory, ops.Trajectory):
                raise ValueError(f"integrate_scan: trajectory must be an ops.Trajectory, got {type(trajectory).__name__}")
            if stamps is None:
                raise ValueError("integrate_scan: a trajectory needs the scan's timestamps")
            rays, info = ops.trajectory_rays(dirs, stamps, trajectory)
            info = info.cpu()
            if int(info[0]):
                raise ValueError(f"integrate_scan: {int(info[3])} rays with a direction or timestamp that is not finite")
            if int(info[2]):
                return {"rays": 0, "updated_rays": 0, "invalid_rays": 0, "missed_rays": 0, "node_updates": 0, "skipped": True}
        return self.integrate_rays(rays, dist)

    def _scan_arrays(self, scan):
        """-> (directions fp32 [3,n], distances [n], timestamps fp64 [n] or None) on the device"""
        if hasattr(scan, "ray_directions") and hasattr(scan, "distances"):
            dirs, dist, stamps = scan.ray_directions, scan.distances, getattr(scan, "timestamps", None)
            if not (torch.is_tensor(dirs) and torch.is_tensor(dist)) or dirs.dim() != 2 or dirs.shape[0] != 3 or \
                    dirs.dtype != torch.float32 or tuple(dist.shape) != (dirs.shape[1],):
                raise ValueError("integrate_scan: a scan with ray_directions fp32 [3,n] and distances [n]")
            if not (dirs.is_cuda and dist.is_cuda):
                raise RuntimeError(f"integrate_scan: the scan is on {dirs.device}; TSDF fusion has no CPU implementation")
        else:
            try:
                xyz, stamps = scan
            except (TypeError, ValueError):
                raise ValueError("integrate_scan: scan must be a LidarScan or a pair (xyz [n,3], timestamps [n])") from None
            pts = xyz if torch.is_tensor(xyz) else torch.from_numpy(np.asarray(xyz, dtype=np.float64))
            if pts.dim() != 2 or pts.shape[1] != 3 or not pts.dtype.is_floating_point:
                raise ValueError(f"integrate_scan: xyz [n,3] of a float dtype, got {tuple(pts.shape)} {pts.dtype}")
            pts = pts.to(device=self.device, dtype=torch.float64)
            dist = torch.linalg.norm(pts, dim=1)
            dirs = (pts / dist[:, None]).T.to(torch.float32).contiguous()           # (a point at the sensor: NaN, an invalid ray)
        if stamps is not None:
            stamps = stamps if torch.is_tensor(stamps) else torch.from_numpy(np.asarray(stamps, dtype=np.float64))
            if tuple(stamps.shape) != (dirs.shape[1],):
                raise ValueError(f"integrate_scan: timestamps [{dirs.shape[1]}], got {tuple(stamps.shape)}")
            stamps = stamps.to(device=self.device, dtype=torch.float64)
        return dirs.to(self.device).contiguous(), dist.to(self.device), stamps


class TSDFVolume(_ScanFusion):
    """A dense TSDF volume on the device over the box [min_bound, max_bound]: node (i,j,k) lies at origin + (i,j,k) * voxel_size with
    origin = min_bound, and every axis has the fewest nodes (at least 2) that reach max_bound.  sdf_trunc (default 3 voxels) is the
    truncation distance; front (default sdf_trunc, math.inf to carve free space from the sensor on) is how far in front of a return
    a ray writes.  .sum int64 and .count uint32 [nx,ny,nz] are the device arrays of lnr_tsdf_integrate, .dims, .origin, .spacing
    the lattice, .n_rays the rays integrated so far."""

    def __init__(self, min_bound, max_bound, voxel_size, sdf_trunc=None, front=None, device=0):
        lo, v, trunc, fr, cells = _lattice_arguments("TSDFVolume", min_bound, max_bound, voxel_size, sdf_trunc, front)
        if not (cells < 2.0 ** 31).all() or float(np.prod(np.maximum(cells, 1.0) + 1.0)) >= 2.0 ** 31:
            raise ValueError(f"TSDFVolume: {' x '.join(str(int(c) + 1) for c in np.minimum(cells, 2.0 ** 40))} nodes, the limit is 2^31 - 1")
        self.dims = tuple(int(max(c, 1.0)) + 1 for c in cells)
        self.origin = tuple(float(x) for x in lo)
        self.voxel_size = v
        self.spacing = (v, v, v)
        self.sdf_trunc, self.front = trunc, fr
        self.device = _device(device)
        # (allocated as int32: torch zeroes every dtype's bytes the same way, and fills of uint32 tensors are recent)
        self._count_words = torch.zeros(self.dims, dtype=torch.int32, device=self.device)
        self.count = self._count_words.view(torch.uint32)
        self.sum = torch.zeros(self.dims, dtype=torch.int64, device=self.device)
        self.n_rays = 0

    def reset(self):
        """an empty volume again"""
        self.sum.zero_()
        self._count_words.zero_()
        self.n_rays = 0
        return self

    def integrate_rays(self, rays, ranges):
        """rays [n,6] (ox oy oz dx dy dz in the world frame, unit directions) and ranges [n] (metres) on the volume's device -> the
        call's counters {"rays", "updated_rays", "invalid_rays", "missed_rays", "node_updates"} (one device -> host read).  A ray that
        is not finite (ops.trajectory_rays writes NaN for a ray outside its trajectory), has no direction or no positive finite range
        is counted as invalid, not refused."""
        n = self._check_rays(rays, ranges)
        info = ops.tsdf_integrate(rays, ranges, self.sum, self.count, self.origin, self.voxel_size, self.sdf_trunc, self.front)
        self.n_rays += n
        host = info.cpu()
        return {"rays": n, "updated_rays": int(host[1]), "invalid_rays": int(host[2]), "missed_rays": int(host[3]),
                "node_updates": int(host[4])}

    def field(self, min_count=1):
        """-> (field fp32 [nx,ny,nz]: minus the mean truncated distance in units of sdf_trunc, > 0 behind the surface, 0 where nothing
        was observed; valid uint8 [nx,ny,nz]: at least min_count rays wrote the node), on the device"""
        return ops.tsdf_field(self.sum, self.count, min_count)

    def extract_mesh(self, min_count=1, min_component_triangles=None):
        """The zero crossing of the field over the cells whose eight corners were observed by at least min_count rays -> a
        TriangleMesh in the world frame (triangles face the side the sensor saw), or None when nothing crosses.
        min_component_triangles = k: connected components of fewer than k triangles are dropped.  Vertices no triangle uses are
        dropped, all on the device; the mesh is downloaded once."""
        self._check_component_filter(min_component_triangles)
        field, valid = self.field(min_count)
        verts, faces = ops.marching_cubes(field, 0.0, spacing=self.spacing, origin=self.origin, valid=valid)
        return self._finish_mesh(verts, faces, min_component_triangles)


class SparseTSDFVolume(_ScanFusion):
    """TSDFVolume's lattice (the same rule and argument checks) without its limit on the number of nodes: an axis may have up to 2^21
    nodes, and only the 8 x 8 x 8 blocks a ray wrote to are stored (include/loner_hip.h, "sparse TSDF").  initial_blocks: the blocks
    the pool holds before it first grows (6 KB each).  .n_blocks the blocks that exist, .store the device arrays
    (tsdf_sparse.SparseTSDFStore), .dims, .origin, .spacing the lattice, .n_rays the rays integrated so far (at most 2^32 - 1)."""

    MAX_AXIS = sparse_ops.SPARSE_MAX_AXIS

    def __init__(self, min_bound, max_bound, voxel_size, sdf_trunc=None, front=None, device=0, initial_blocks=4096):
        lo, v, trunc, fr, cells = _lattice_arguments("SparseTSDFVolume", min_bound, max_bound, voxel_size, sdf_trunc, front)
        if not (np.maximum(cells, 1.0) + 1.0 <= self.MAX_AXIS).all():
            raise ValueError(f"SparseTSDFVolume: {' x '.join(str(int(c) + 1) for c in np.minimum(cells, 2.0 ** 40))} nodes, the limit is "
                             f"2^21 per axis")
        self.dims = tuple(int(max(c, 1.0)) + 1 for c in cells)
        self.origin = tuple(float(x) for x in lo)
        self.voxel_size = v
        self.spacing = (v, v, v)
        self.sdf_trunc, self.front = trunc, fr
        self.device = _device(device)
        self.store = sparse_ops.SparseTSDFStore(self.device, initial_blocks)
        self.n_rays = 0

    @property
    def n_blocks(self):
        return self.store.n_blocks

    def reset(self):
        """an empty volume again, at its initial capacity"""
        self.store.reset()
        self.n_rays = 0
        return self

    def integrate_rays(self, rays, ranges):
        """TSDFVolume.integrate_rays on the sparse volume -> its counters and {"new_blocks", "blocks", "lost_updates"}; lost_updates
        (written voxels whose block the directory did not hold) is 0 unless the library is broken.  At most three device -> host reads,
        whatever n is: the candidate total, the number of new blocks (only when there is a candidate), and the counters."""
        n = self._check_rays(rays, ranges)
        info = sparse_ops.sparse_tsdf_integrate(rays, ranges, self.store, self.dims, self.origin, self.voxel_size, self.sdf_trunc, self.front)
        self.n_rays += n
        host = info.cpu()
        return {"rays": n, "updated_rays": int(host[1]), "invalid_rays": int(host[2]), "missed_rays": int(host[3]),
                "node_updates": int(host[4]), "new_blocks": int(host[5]), "blocks": int(host[6]), "lost_updates": int(host[7])}

    def block_indices(self):
        """-> int32 [B,3] on the device: the block coordinates (node index >> 3) of the existing blocks, in directory order (ascending
        key bx << 36 | by << 18 | bz)"""
        return sparse_ops.sparse_block_indices(self.store.keys[:self.n_blocks])

    def blocks(self):
        """-> (sum int64 [B,8,8,8], count uint32 [B,8,8,8]) on the device, copies in directory order"""
        slot = self.store.slot[:self.n_blocks].long()
        return self.store.sum[slot], self.store._count_words[slot].view(torch.uint32)

    def to_dense(self):
        """-> (sum int64 [nx,ny,nz], count uint32 [nx,ny,nz]) on the device: the arrays of the TSDFVolume over the same lattice.
        Raises ValueError where TSDFVolume would (2^31 nodes or more)."""
        if float(np.prod(np.asarray(self.dims, dtype=np.float64))) >= 2.0 ** 31:
            raise ValueError(f"to_dense: {' x '.join(str(n) for n in self.dims)} nodes, the limit is 2^31 - 1")
        padded = tuple((n + 7) // 8 for n in self.dims)
        sum_, count = self.blocks()
        idx = self.block_indices().long()
        out = []
        for blocks_, dtype in ((sum_, torch.int64), (count.view(torch.int32), torch.int32)):
            full = torch.zeros(padded + (8, 8, 8), dtype=dtype, device=self.device)
            full[idx[:, 0], idx[:, 1], idx[:, 2]] = blocks_
            full = full.permute(0, 3, 1, 4, 2, 5).reshape(padded[0] * 8, padded[1] * 8, padded[2] * 8)
            out.append(full[:self.dims[0], :self.dims[1], :self.dims[2]].contiguous())
        return out[0], out[1].view(torch.uint32)

    def memory_bytes(self):
        """the bytes of the blocks that exist: 6156 each (512 sums, 512 counts, a key and a slot)"""
        return self.n_blocks * sparse_ops.SparseTSDFStore.BLOCK_BYTES

    def allocated_bytes(self):
        """the bytes of the directory and the pool as allocated: 6156 per block of capacity, which at least doubles when it grows"""
        return self.store.capacity * sparse_ops.SparseTSDFStore.BLOCK_BYTES

    def field(self, min_count=1):
        """-> (field fp32 [B,8,8,8], valid uint8 [B,8,8,8]) in directory order: TSDFVolume.field's values for the existing blocks"""
        return sparse_ops.sparse_tsdf_field(self.store, min_count)

    def extract_mesh(self, min_count=1, min_component_triangles=None):
        """TSDFVolume.extract_mesh: the same triangles with the same coordinates, in another order (blocks in key order)."""
        self._check_component_filter(min_component_triangles)
        if self.n_blocks == 0:
            return None
        field, valid = self.field(min_count)
        verts, faces = sparse_ops.sparse_marching_cubes(self.store.keys[:self.n_blocks], field, valid, self.dims, 0.0, spacing=self.spacing,
                                                 origin=self.origin)
        return self._finish_mesh(verts, faces, min_component_triangles)


def fuse_scans(scans, trajectory, bound, voxel_size, sdf_trunc=None, front=None, device=None, stats=None, sparse=False):
    """-> the TSDFVolume of every scan fused along the trajectory.  scans: an iterable of (xyz [n,3], timestamps [n]) (sensor frame,
    absolute times) or LidarScans; trajectory: TUM rows [K,8], a TUM file or an ops.Trajectory, as gt_map.build_lidar_map takes it;
    bound: (min_bound, max_bound).  A scan with a ray outside the trajectory's time span is skipped whole.  stats (a dict, optional)
    receives the summed counters and {"scans", "skipped_scans"}.  sparse=True: a SparseTSDFVolume instead (stats then also hold
    "new_blocks" and "lost_updates" summed and the final "blocks")."""
    try:
        lo, hi = bound
    except (TypeError, ValueError):
        raise ValueError(f"fuse_scans: bound must be (min_bound, max_bound), got {bound!r}") from None
    arrays = None if isinstance(trajectory, ops.Trajectory) else trajectory_arrays(trajectory)
    volume = (SparseTSDFVolume if sparse else TSDFVolume)(lo, hi, voxel_size, sdf_trunc, front, device=device)
    traj = trajectory if arrays is None else ops.Trajectory(*arrays, volume.device)
    total = {"scans": 0, "skipped_scans": 0}
    for scan in scans:
        got = volume.integrate_scan(scan, trajectory=traj)
        total["scans"] += 1
        total["skipped_scans"] += 1 if got.pop("skipped", False) else 0
        for key, value in got.items():
            total[key] = total.get(key, 0) + value
    if sparse:
        total["blocks"] = volume.n_blocks
    if stats is not None:
        stats.update(total)
    return volume
