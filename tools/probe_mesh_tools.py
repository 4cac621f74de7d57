"""Mesh clean-up costs (profiles/mesh_tools.txt): on the marching-cubes mesh of the trained synthetic map (tests/test_gpu_mesh.py's
scene, one keyframe) at 0.1 m, each step of the clean-up on the device against its host equivalent: connected components against
scipy.sparse.csgraph.connected_components on the edge-adjacency graph, vertex normals against the numpy compute_vertex_normals,
and the cluster areas, the compaction and the whole Mesher.get_mesh(min_component_triangles=k) for scale.

    python tools/probe_mesh_tools.py [--out FILE] [--resolution 0.1] [--iterations 150]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """mean ms per call by device events after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def host_components(triangles):
    """(graph build ms, connected_components ms, labels numbered by first triangle): triangles sharing an edge are linked, the links
    found by a numpy sort of the 3 F edge keys"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    t = triangles.astype(np.int64)
    n = len(t)
    a, b = t[:, [0, 1, 2]].reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    keys = (np.minimum(a, b) << 32) | np.maximum(a, b)
    owner = np.repeat(np.arange(n), 3)
    order = np.argsort(keys, kind="stable")
    same = keys[order][1:] == keys[order][:-1]
    rows, cols = owner[order][:-1][same], owner[order][1:][same]
    graph = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n, n)).tocsr()
    t1 = time.perf_counter()
    labels = connected_components(graph, directed=False)[1]
    t2 = time.perf_counter()
    first = np.full(labels.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(first, labels, np.arange(n))
    rank = np.empty_like(first)
    rank[np.argsort(first)] = np.arange(len(first))
    return 1000 * (t1 - t0), 1000 * (t2 - t1), rank[labels].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--resolution", type=float, default=0.1)
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--min-triangles", type=int, default=100)
    args = ap.parse_args()
    from loner_amd import ops
    from loner_amd.analysis.mesher import Mesher, TriangleMesh
    from loner_amd.common.pose_utils import WorldCube
    from loner_amd.common.settings import default_optimizer_settings
    from loner_amd.mapping.optimizer import OptimizationSettings, Optimizer
    from loner_amd.utils import synthetic as SY
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
    k = args.min_triangles

    def get_mesh(**kw):
        torch.manual_seed(3)
        return mesher.get_mesh(dev, opt._ray_sampler, skip_step=1, **kw)

    mesh = get_mesh()
    V, F = mesh.vertices.shape[0], mesh.triangles.shape[0]
    say(f"# mesh clean-up on one MI355X ({torch.cuda.get_device_name(0)}); device events after a warm-up call, mean of 5 calls; each ops call")
    say("# includes its workspace and output allocations (cached) and its one host read; host: one process, numpy / scipy (neither")
    say(f"# threads these routines, whatever OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')} allows)")
    say(f"mesh: synthetic room, {args.iterations} iterations, {args.resolution} m: {V} vertices, {F} triangles")
    v, t = torch.tensor(mesh.vertices, device=dev), torch.tensor(mesh.triangles, device=dev)
    reps = 5
    clusters, sizes = ops.mesh_connected_triangles(t, V)
    C = sizes.shape[0]
    hs = sizes.cpu().numpy()
    say(f"clusters: {C}, largest {hs.max()} triangles, {int((hs < k).sum())} clusters with {int(hs[hs < k].sum())} triangles below {k}")
    t_cc = timed(lambda: ops.mesh_connected_triangles(t, V), reps)
    t_area = timed(lambda: ops.mesh_cluster_area(v, t, clusters, C), reps)
    keep = (sizes >= k)[clusters.long()]
    t_sel = timed(lambda: ops.mesh_select(t, V, triangle_keep=keep, drop_unreferenced=True), reps)
    t_vn = timed(lambda: ops.mesh_vertex_normals(v, t), reps)
    ops.profile_enable(True)
    ops.profile_read()
    for _ in range(reps):
        ops.mesh_connected_triangles(t, V)
        ops.mesh_cluster_area(v, t, clusters, C)
        ops.mesh_select(t, V, triangle_keep=keep, drop_unreferenced=True)
        ops.mesh_vertex_normals(v, t)
    torch.cuda.synchronize()
    prof = {name: val["total_ms"] / reps for name, val in ops.profile_read().items() if name.startswith("mesh_")}
    ops.profile_enable(False)
    on_dev = lambda name: f"on the device alone {prof.get(name, float('nan')):.3f} ms"
    build_ms, cc_ms, host_labels = host_components(mesh.triangles)
    same = np.array_equal(host_labels, clusters.cpu().numpy())
    say(f"connected components: ops.mesh_connected_triangles {t_cc:.3f} ms ({on_dev('mesh_connected_triangles')}); host: adjacency graph by a "
        f"numpy sort {build_ms:.0f} ms + scipy connected_components {cc_ms:.0f} ms (identical labels: {same})")
    say(f"cluster areas: ops.mesh_cluster_area {t_area:.3f} ms ({on_dev('mesh_cluster_area')})")
    say(f"select (clusters of >= {k} triangles, unreferenced vertices dropped): ops.mesh_select {t_sel:.3f} ms ({on_dev('mesh_select')})")
    host = TriangleMesh(mesh.vertices, mesh.triangles)
    t0 = time.perf_counter()
    host.compute_vertex_normals()
    t_np = 1000 * (time.perf_counter() - t0)
    same = host.vertex_normals.tobytes() == ops.mesh_vertex_normals(v, t).cpu().numpy().tobytes()
    say(f"vertex normals: ops.mesh_vertex_normals {t_vn:.3f} ms ({on_dev('mesh_vertex_normals')}); host numpy compute_vertex_normals "
        f"{t_np:.0f} ms (identical bytes: {same})")
    t0 = time.perf_counter()
    host.compute_vertex_normals(device=dev)
    say(f"TriangleMesh.compute_vertex_normals(device=...) from host arrays and back: {1000 * (time.perf_counter() - t0):.1f} ms")
    t_plain = timed(lambda: get_mesh(), 3)
    t_filtered = timed(lambda: get_mesh(min_component_triangles=k), 3)
    say(f"Mesher.get_mesh: {t_plain:.1f} ms; with min_component_triangles = {k}: {t_filtered:.1f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
