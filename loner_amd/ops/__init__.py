"""Tensor-level wrappers around the C ABI (one Python function per entry point).

Every function takes/returns torch tensors that live on the HIP device, allocates outputs with
torch, and enqueues the kernel on torch's current stream.  No function here computes anything
itself - the arithmetic is in libloner_hip.so.

One module per family, its rules (input dtypes, reads back from the device, error types) in its docstring: density, rays, render and
optim are the mapping loop's wrappers, where host microseconds count; mesh, cloud, raycast (with the TSDF) and scan the offline tools
and the tracker's calls.  Callers write `from loner_amd import ops; ops.X(...)`: names resolve through this package, so replacing
ops.X reaches them.
"""
from ..hip import check, load, require_device
from .cloud import (NNGrid, Trajectory, affine_f64, cloud_transform, icp_point_to_plane, lidar_scan_points, trajectory_transform,
                    voxel_down_sample)
from .density import (density_backward, density_clipped_count, density_fold_weight_grads, density_forward, density_route, profile_enable,
                      profile_read)
from .mesh import (MESH_SMOOTH_KINDS, MeshLattice, marching_cubes, mc_case_table, mesh_accumulate, mesh_cluster_area, mesh_connected_triangles,
                   mesh_sample_points, mesh_select, mesh_smooth, mesh_unique_triangles, mesh_vertex_adjacency, mesh_vertex_clusters,
                   mesh_vertex_normals)
from .optim import adam_step, occ_grid_apply, occ_grid_step, rng_draws, selftest_mfma
from .raycast import BVH, cast_rays, closest_points, count_intersections, trajectory_rays, tsdf_field, tsdf_integrate
from .rays import (WindowTables, build_camera_rays, build_lidar_rays, build_window_rays, compact_rays, first_ray_key, lidar_rays_backward,
                   pose_backward, pose_forward, shard_front_pack, shard_front_reduce)
from .render import (count_opaque, depth_colormap, ftb_composite, ftb_gather, linspace_table, logits_grad, los_loss_fused, occ_interpolate,
                     points_grad_to_rays, render_backward, render_forward, render_forward_peak, sample_rays_occ, sample_rays_uniform,
                     weights_gt)
from .scan import frame_cloud, motion_compensate, scan_from_points, sky_rays
