"""The public surface of loner_amd.ops is pinned: every public name and every signature, as recorded at the last commit where ops
was the single file loner_amd/ops.py.  Callers write `ops.X(...)`; splitting the file into a package, or moving a wrapper between
its modules, must not move, rename or re-default anything they can see.  No GPU, no library call.

API: name -> str(inspect.signature(...)) for a function; {"": the constructor's signature, method or property: signature or
"property"} for a class; None for a constant.  An annotation's module path is compared with the submodule left out
(loner_amd.ops.rays.WindowTables reads loner_amd.ops.WindowTables): where a class lives inside the package is not part of the API.
"""
import ast
import inspect
import os
import re
import types

API = {
    'BVH': {'': '(vertices, triangles)', 'device': 'property'},
    'MESH_SMOOTH_KINDS': None,
    'MeshLattice': {'': '(axes, bound, device)', 'n_nodes': 'property'},
    'NNGrid': {'': '(targets, cell_edge=None)',
               'correspondences': '(self, queries, max_distance)',
               'distance': '(self, queries, want_sq=False, stats=None)',
               'knn_mean_distance': '(self, nb_neighbors=20, stats=None)',
               'normals': '(self, knn=30, want_covariances=False, stats=None)',
               'outlier_threshold': '(self, mean_distance, std_ratio)'},
    'Trajectory': {'': '(times, positions, rotations, rotvecs, device)'},
    'WindowTables': {'': '(dirs_list, dist_list, const_dist, seg_counts, seg_pose)'},
    'adam_step': '(params, grads, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-08, grad_scale=1.0, zero_grad=True, poison=None)',
    'affine_f64': '(T, what, finite=False)',
    'build_camera_rays': '(directions, index, width, transform12, range_min, scale, shift)',
    'build_lidar_rays': '(directions, distances, index, transform12, ray_range, scale, shift)',
    'build_window_rays': '(tab: loner_amd.ops.WindowTables, transforms, ray_range, scale, shift, index=None, seed=0)',
    'cast_rays': '(bvh, rays, t_min=0.0, t_max=inf, want_uvs=True, stats=None)',
    'check': "(rc, what='')",
    'closest_points': '(bvh, points, max_distance=inf, want_points=True, want_uvs=True, stats=None)',
    'cloud_transform': '(points, T, out=None)',
    'compact_rays': '(rays, depths, keep, src_index, seg_start, n_out=None, want_counts=False, front=None)',
    'count_intersections': '(bvh, rays, t_min=0.0, t_max=inf, stats=None)',
    'count_opaque': '(rays, depth_gt, n_rays_dev=None, far0=None)',
    'density_backward': '(spec, params, d_sigma, grad_params, pts=None, rays=None, z=None, n_rays_dev=None, want_d_pts=False, reuse_features=False, '
                        'd_rays=None, table_atomics=False, report_regions=False, input_grad_event=None, '
                        'defer_weight_fold=False, overwrite_grad=False)',
    'density_clipped_count': '(device) -> int',
    'density_fold_weight_grads': '(spec, grad_params, n_points, overwrite_grad=False)',
    'density_forward': '(spec, params, pts=None, rays=None, z=None, n_rays_dev=None, forward_only=False, out=None)',
    'density_route': '(spec, n_points, backward=True)',
    'depth_colormap': '(values, table, multiplier=1.0, min_depth=1.0, max_depth=50.0)',
    'first_ray_key': '(rays, out_seg_start, seg_order)',
    'frame_cloud': '(directions, distances, start, stop, step)',
    'ftb_composite': '(sigma_c, z, rays, idx, n_alive, b0, block, noise_std, seed, transmittance, depth_acc, opacity_acc, next_idx, next_count, last, '
                     'noise=None)',
    'ftb_gather': '(rays, z, idx, n_alive, b0, block, rays_c, z_c, next_count)',
    'icp_point_to_plane': '(grid, target_normals, source, max_distance, init=None, relative_fitness=1e-06, relative_rmse=1e-06, max_iteration=30)',
    'lidar_rays_backward': '(d_rays, rays, src_index, seg_start_dev, directions_list, transforms, scale)',
    'lidar_scan_points': '(depth, variance, ray_index, directions, scale, var_max, depth_max)',
    'linspace_table': '(count: int, device) -> torch.Tensor',
    'load': '()',
    'logits_grad': '(s, g, margin=2.0, l_free=0.25, l_occ=2.5)',
    'los_loss_fused': '(sigma, z, rays, depth_gt, scale, cfg: loner_amd.hip.LossConfig, counts, noise=None, noise_std=0.0, seed=0, n_rays_dev=None, '
                      'want_stats=False, want_weights=False, loss_out=None, far0=None, poison=None, poison_tag=0, zero_dead_rows=True)',
    'marching_cubes': '(volume, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), valid=None)',
    'mc_case_table': '()',
    'mesh_accumulate': '(sigma, z, rays, lattice: loner_amd.ops.MeshLattice, volume, depth_max, var_max=None, noise=None, noise_std=0.0, seed=0, '
                       'n_rays_dev=None, counters=None)',
    'mesh_cluster_area': '(vertices, triangles, triangle_clusters, n_clusters)',
    'mesh_connected_triangles': '(triangles, n_vertices)',
    'mesh_sample_points': '(vertices, triangles, n_points, seed=0, want_triangles=False, info=None)',
    'mesh_select': '(triangles, n_vertices, triangle_keep=None, vertex_keep=None, drop_unreferenced=False)',
    'mesh_smooth': "(vertices, row_start, neighbours, n_steps, kind='laplacian', lambda_filter=0.5, mu=None)",
    'mesh_unique_triangles': '(triangles, n_vertices, vertex_map=None, n_mapped=None, drop_degenerate=False)',
    'mesh_vertex_adjacency': '(triangles, n_vertices)',
    'mesh_vertex_clusters': '(vertices, voxel_size)',
    'mesh_vertex_normals': '(vertices, triangles)',
    'motion_compensate': '(directions, distances, timestamps, t0, denom, consts)',
    'occ_grid_apply': '(grid, grad_buf, lr, zero_grad=True, poison=None)',
    'occ_grid_step': '(grid, rays, z, depth_gt, scale, lr, margin=2.0, l_free=0.25, l_occ=2.5, grad_buf=None, n_rays_dev=None)',
    'occ_interpolate': '(grid, pts)',
    'points_grad_to_rays': '(d_pts, z, d_rays, n_rays_dev=None)',
    'pose_backward': '(pose6, d_transforms, mask=None, out=None, accumulate=False, poison=None, poison_tag=0)',
    'pose_forward': '(pose6)',
    'profile_enable': '(on=True)',
    'profile_read': '()',
    'render_backward': '(sigma, z, rays, g_depth, g_weights, g_opacity, g_variance, noise=None, noise_std=0.0, seed=0, n_rays_dev=None)',
    'render_forward': '(sigma, z, rays, noise=None, noise_std=0.0, seed=0, n_rays_dev=None, want_weights=True)',
    'render_forward_peak': '(sigma, z, rays, noise=None, noise_std=0.0, seed=0, n_rays_dev=None)',
    'require_device': '(*tensors)',
    'rng_draws': "(which, seed, n_rays, n_per_ray, device='cuda')",
    'sample_rays_occ': '(rays, grid, n_samples, perturb, u_jitter=None, u_pdf=None, seed=0, n_rays_dev=None, debug=False)',
    'sample_rays_uniform': '(rays, n_samples, perturb, u_jitter=None, seed=0, n_rays_dev=None)',
    'scan_from_points': '(xyz, point_times, stamp, fov_segments=None, min_range=0.3, recompute_timestamps=False)',
    'selftest_mfma': "(device='cuda')",
    'shard_front_pack': '(rays, out_seg_start, seg_order, depths, n_rays_dev, cap, device=None)',
    'shard_front_reduce': '(records, world, stride)',
    'sky_rays': '(directions, rotation)',
    'trajectory_rays': '(directions, timestamps, trajectory)',
    'trajectory_transform': '(points, timestamps, trajectory, min_range)',
    'tsdf_field': '(sum_, count, min_count=1)',
    'tsdf_integrate': '(rays, ranges, sum_, count, origin, voxel_size, trunc, front=None)',
    'voxel_down_sample': '(points, voxel_size, count=None)',
    'weights_gt': '(s, g, eps, normalise=True)',
}


def _signature(obj):
    return re.sub(r"\bloner_amd\.ops\.\w+\.", "loner_amd.ops.", str(inspect.signature(obj)))


def _describe(ops):
    api = {}
    for name in sorted(n for n in dir(ops) if not n.startswith("_")):
        obj = getattr(ops, name)
        if isinstance(obj, types.ModuleType):
            continue
        if inspect.isclass(obj):
            api[name] = {"": _signature(obj)}
            for member, f in vars(obj).items():
                if not member.startswith("_"):
                    api[name][member] = "property" if isinstance(f, property) else _signature(f)
        else:
            api[name] = _signature(obj) if callable(obj) else None
    return api


def _top_level(path):
    """(names of the functions and classes, names assigned) at the top level of a Python file"""
    with open(path) as f:
        tree = ast.parse(f.read())
    defined = [n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef))]
    assigned = [t.id for n in tree.body if isinstance(n, ast.Assign) for t in n.targets if isinstance(t, ast.Name)]
    return defined, assigned


def test_ops_exposes_exactly_the_recorded_api():
    from loner_amd import ops
    assert len(API) == 74
    got = _describe(ops)
    assert sorted(got) == sorted(API)
    for name in API:
        assert got[name] == API[name], name


def test_ops_init_only_re_exports_and_no_name_has_two_homes():
    from loner_amd import hip, ops
    here = os.path.dirname(ops.__file__)
    assert os.path.basename(ops.__file__) == "__init__.py"
    assert _top_level(os.path.join(here, "__init__.py")) == ([], [])             # no function, no class, no state
    homes = {}
    for fn in sorted(os.listdir(here)):
        if fn.endswith(".py") and fn != "__init__.py":
            defined, assigned = _top_level(os.path.join(here, fn))
            for name in defined + assigned:
                if not name.startswith("_"):
                    homes.setdefault(name, []).append(fn)
    assert {n: h for n, h in homes.items() if len(h) != 1} == {}
    from_hip = {n for n in API if getattr(ops, n) is getattr(hip, n, None)}      # check, load, require_device
    assert sorted(homes) == sorted(set(API) - from_hip)
