"""Mesh simplification and smoothing costs (profiles/mesh_filters.txt): on the marching-cubes mesh of the trained synthetic map
(tests/test_gpu_mesh.py's scene, one keyframe) at 0.1 m, each entry of the "mesh simplification and smoothing" block on the device
against a plain numpy route to the same result: np.unique over the voxel triples and over the canonical triangle triples, a sorted
list of directed edges, and one np.add.at smoothing step; and the TriangleMesh calls and Mesher.get_mesh options for scale.

    python tools/probe_mesh_filters.py [--out FILE] [--resolution 0.1] [--iterations 150] [--voxel 0.3]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.probe_mesh_tools import timed  # noqa: E402


def host_clusters(vertices, voxel):
    """(vertex_cluster, cluster_vertices) by np.unique over the voxel triples, renumbered by first occurrence"""
    lo = vertices.min(0) - voxel * 0.5
    ijk = np.floor((vertices - lo) / voxel).astype(np.int64)
    _, first, inverse = np.unique(ijk, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    cluster = rank[inverse.reshape(-1)]
    sums = np.zeros((len(first), 3), dtype=np.float64)
    np.add.at(sums, cluster, vertices)
    return cluster.astype(np.int32), sums / np.bincount(cluster).astype(np.float64)[:, None]


def host_unique(triangles, vertex_map=None, drop_degenerate=False):
    """(canonical, triangle_keep) by the rotation in numpy and np.unique over the triples"""
    t = triangles.astype(np.int64)
    if vertex_map is not None:
        t = vertex_map.astype(np.int64)[t]
    t0, t1, t2 = t[:, 0], t[:, 1], t[:, 2]
    shift = np.where(t0 <= t1, np.where(t0 <= t2, 0, 2), np.where(t1 <= t2, 1, 2))     # the corner that comes first
    rows = np.arange(len(t))
    canonical = np.stack([t[rows, shift], t[rows, (shift + 1) % 3], t[rows, (shift + 2) % 3]], 1)
    _, first = np.unique(canonical, axis=0, return_index=True)
    keep = np.zeros(len(t), dtype=np.uint8)
    keep[first] = 1
    if drop_degenerate:
        keep &= ((t0 != t1) & (t1 != t2) & (t2 != t0)).astype(np.uint8)
    return canonical.astype(np.int32), keep


def host_adjacency(triangles, n_vertices):
    """(row_start, neighbours) by a sorted list of the distinct directed edges"""
    t = triangles.astype(np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2], t[:, 1], t[:, 2], t[:, 0]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0], t[:, 0], t[:, 1], t[:, 2]])
    keys = np.unique((a << 32 | b)[a != b])
    row_start = np.searchsorted(keys, np.arange(n_vertices + 1, dtype=np.int64) << 32)
    return row_start.astype(np.int32), (keys & 0xFFFFFFFF).astype(np.int32)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1000 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--resolution", type=float, default=0.1)
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--smooth-iterations", type=int, default=5)
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis.mesher import Mesher, TriangleMesh
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
    from tests import mesh_filters_restatement as MF
    from tests.test_gpu_mapping import make_keyframes
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    s = default_optimizer_settings()
    s["num_samples"]["sky"] = 0
    torch.manual_seed(0)
    scale, shift = SY.world_cube()
    wc = WorldCube(torch.tensor(scale), torch.from_numpy(shift))
    opt = Optimizer(s, None, wc, 0, False, True, False)
    kf = make_keyframes([SY.trajectory_pose6(1)[0]])[0]
    opt._do_iterate_optimizer([kf], [None], optimizer_settings=OptimizationSettings(args.iterations, True, False, False, True))
    mcb = [[-21.0, 21.0], [-16.0, 16.0], [-3.0, 7.0]]
    mesher = Mesher(opt._model, {"poses": [kf.get_pose_state()]}, wc, torch.tensor([1.0, 50.0]), resolution=args.resolution,
                    marching_cubes_bound=mcb, level_set=0)

    def get_mesh(**kw):
        torch.manual_seed(3)
        return mesher.get_mesh(dev, opt._ray_sampler, skip_step=1, **kw)

    mesh = get_mesh()
    V, F = mesh.vertices.shape[0], mesh.triangles.shape[0]
    voxel, k = args.voxel, args.smooth_iterations
    say(f"# mesh simplification and smoothing on one MI355X ({torch.cuda.get_device_name(0)}); device events after a warm-up call, mean of 5")
    say("# calls; each ops call includes its workspace and output allocations and its one host read; host: one process, numpy, one")
    say(f"# wall-clock run each (np.unique, np.sort and np.add.at do not thread, whatever OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')} allows)")
    say(f"mesh: synthetic room, {args.iterations} iterations, {args.resolution} m: {V} vertices, {F} triangles")
    v, t = torch.tensor(mesh.vertices, device=dev), torch.tensor(mesh.triangles, device=dev)
    reps = 5
    cluster, means = ops.mesh_vertex_clusters(v, voxel)
    m = means.shape[0]
    canonical, keep, kept, degenerate = ops.mesh_unique_triangles(t, V, cluster, m, drop_degenerate=True)
    say(f"clustering at {voxel} m: {m} clusters; {degenerate} triangles degenerate, {F - degenerate - kept} duplicates, {kept} kept")
    row_start, neighbours = ops.mesh_vertex_adjacency(t, V)
    valence = torch.diff(row_start)
    say(f"adjacency: {neighbours.shape[0]} neighbours, longest row {int(valence.max())}, {int((valence == 0).sum())} vertices without one")
    t_vc = timed(lambda: ops.mesh_vertex_clusters(v, voxel), reps)
    t_ut = timed(lambda: ops.mesh_unique_triangles(t, V, cluster, m, drop_degenerate=True), reps)
    t_ui = timed(lambda: ops.mesh_unique_triangles(t, V), reps)
    t_va = timed(lambda: ops.mesh_vertex_adjacency(t, V), reps)
    t_s1 = timed(lambda: ops.mesh_smooth(v, row_start, neighbours, 1, "laplacian"), reps)
    t_sk = timed(lambda: ops.mesh_smooth(v, row_start, neighbours, 2 * k, "laplacian", 0.5, -0.53), reps)
    t_simple = timed(lambda: ops.mesh_smooth(v, row_start, neighbours, 1, "simple"), reps)
    ops.profile_enable(True)
    ops.profile_read()
    for _ in range(reps):
        ops.mesh_vertex_clusters(v, voxel)
        ops.mesh_unique_triangles(t, V, cluster, m, drop_degenerate=True)
        ops.mesh_vertex_adjacency(t, V)
        ops.mesh_smooth(v, row_start, neighbours, 1, "laplacian")
    torch.cuda.synchronize()
    prof = {name: val["total_ms"] / reps for name, val in ops.profile_read().items() if name.startswith("mesh_")}
    ops.profile_enable(False)
    on_dev = lambda name: f"on the device alone {prof.get(name, float('nan')):.3f} ms"
    ms, (h_cluster, h_means) = clock(lambda: host_clusters(mesh.vertices, voxel))
    same = np.array_equal(h_cluster, cluster.cpu().numpy()) and h_means.tobytes() == means.cpu().numpy().tobytes()
    say(f"vertex clusters: ops.mesh_vertex_clusters {t_vc:.3f} ms ({on_dev('mesh_vertex_clusters')}); host: np.unique over the voxel triples, "
        f"np.add.at means {ms:.0f} ms (identical labels and bytes: {same})")
    ms, (h_canonical, h_keep) = clock(lambda: host_unique(mesh.triangles, h_cluster, True))
    same = np.array_equal(h_canonical, canonical.cpu().numpy()) and np.array_equal(h_keep, keep.cpu().numpy())
    say(f"unique triangles through the clusters: ops.mesh_unique_triangles {t_ut:.3f} ms ({on_dev('mesh_unique_triangles')}); without a map "
        f"{t_ui:.3f} ms; host: np.unique over the canonical triples {ms:.0f} ms (identical triples and flags: {same})")
    ms, (h_rows, h_neighbours) = clock(lambda: host_adjacency(mesh.triangles, V))
    same = np.array_equal(h_rows, row_start.cpu().numpy()) and np.array_equal(h_neighbours, neighbours.cpu().numpy())
    say(f"vertex adjacency: ops.mesh_vertex_adjacency {t_va:.3f} ms ({on_dev('mesh_vertex_adjacency')}); host: np.unique over the directed "
        f"edge keys {ms:.0f} ms (identical CSR: {same})")
    ms, h_step = clock(lambda: MF.smooth_step(mesh.vertices, h_rows, h_neighbours, 1, 0.5))
    same = h_step.tobytes() == ops.mesh_smooth(v, row_start, neighbours, 1, "laplacian").cpu().numpy().tobytes()
    say(f"smoothing: one Laplacian step, ops.mesh_smooth {t_s1:.3f} ms ({on_dev('mesh_smooth')}); one simple step {t_simple:.3f} ms; "
        f"{k} Taubin iterations ({2 * k} steps) {t_sk:.3f} ms; host: one np.add.at Laplacian step {ms:.0f} ms (identical bytes: {same})")
    host = TriangleMesh(mesh.vertices, mesh.triangles)
    ms, _ = clock(lambda: host.filter_smooth_taubin(k, device=dev))
    say(f"TriangleMesh.filter_smooth_taubin({k}, device=...) from host arrays and back: {ms:.1f} ms")
    ms, small = clock(lambda: host.simplify_vertex_clustering(voxel, device=dev))
    say(f"TriangleMesh.simplify_vertex_clustering({voxel}, device=...) from host arrays and back: {ms:.1f} ms "
        f"({small.vertices.shape[0]} vertices, {small.triangles.shape[0]} triangles)")
    t_plain = timed(lambda: get_mesh(), 3)
    t_both = timed(lambda: get_mesh(smooth_iterations=k, simplify_voxel_size=voxel), 3)
    say(f"Mesher.get_mesh: {t_plain:.1f} ms; with smooth_iterations = {k} and simplify_voxel_size = {voxel}: {t_both:.1f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
