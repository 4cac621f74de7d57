"""TSDF fusion on the CPU: the restated voxel walk against a brute-force slab test per voxel (so that kernel and restatement cannot
share a wrong walk), a known answer for the whole chain (a plane seen by parallel rays), the masked marching cubes of the
restatement against the unmasked one, and the TSDFVolume argument checks that need no device."""
import math

import numpy as np
import pytest
import torch

from tests import mesh_restatement as MR
from tests import tsdf_restatement as TR


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as ge
    ge.build()
    from loner_amd import ops
    return ops.mc_case_table()


# ------------------------------------------------------------------------------------------------ the walk
GRIDS = [((9, 7, 5), (-1.0, -0.75, -0.5), 0.25, 11), ((4, 4, 4), (0.5, -2.0, 1.0), 0.5, 12)]


@pytest.mark.parametrize("dims,origin,v,seed", GRIDS)
@pytest.mark.parametrize("carve", [False, True])
def test_walk_visits_what_a_slab_test_per_voxel_finds(dims, origin, v, seed, carve):
    """every voxel whose interior shrunk by 1e-9 v the segment crosses is visited, every visited voxel is met by the segment when
    grown by 1e-9 v, and no voxel is visited twice"""
    rays, ranges = TR.ray_set(dims, origin, v, seed)
    assert rays.shape[0] >= 250
    trunc = 3 * v
    front = math.inf if carve else trunc
    states = {"ok": 0, "miss": 0, "invalid": 0}
    zero_components = set()
    for ray, r in zip(rays, ranges):
        state, voxels = TR.walk(ray[:3], ray[3:], r, dims, origin, v, trunc, front)
        states[state] += 1
        must = TR.voxels_crossed(ray[:3], ray[3:], r, dims, origin, v, trunc, front, -1e-9 * v)
        may = TR.voxels_crossed(ray[:3], ray[3:], r, dims, origin, v, trunc, front, 1e-9 * v)
        visited = np.zeros(dims, dtype=bool)
        for c in voxels:
            assert not visited[c], f"voxel {c} visited twice by ray {ray} range {r}"
            visited[c] = True
        assert not (must & ~visited).any(), f"ray {ray} range {r}: crossed but not visited {np.argwhere(must & ~visited)}"
        assert not (visited & ~may).any(), f"ray {ray} range {r}: visited but not touched {np.argwhere(visited & ~may)}"
        if state == "ok":
            zero_components.add(int((ray[3:] == 0).sum()))
    assert states["invalid"] == 0 and states["miss"] >= 5 and states["ok"] >= 200
    assert zero_components == {0, 1, 2}


def test_walk_sorts_out_invalid_rays():
    dims, origin, v = (9, 7, 5), (-1.0, -0.75, -0.5), 0.25
    good = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    for k in range(6):
        for bad in (math.nan, math.inf, -math.inf):
            ray = list(good)
            ray[k] = bad
            assert TR.walk(ray[:3], ray[3:], 1.0, dims, origin, v, 0.75, 0.75)[0] == "invalid"
    assert TR.walk(good[:3], [0.0, 0.0, 0.0], 1.0, dims, origin, v, 0.75, 0.75)[0] == "invalid"
    for r in (0.0, -1.0, math.nan, math.inf):
        assert TR.walk(good[:3], good[3:], r, dims, origin, v, 0.75, 0.75)[0] == "invalid"
    assert TR.walk([5.0, 0.0, 0.0], good[3:], 1.0, dims, origin, v, 0.75, 0.75)[0] == "miss"           # starts behind the box
    assert TR.walk([-9.0, 0.0, 0.0], good[3:], 1.0, dims, origin, v, 0.75, 0.75)[0] == "miss"          # ends in front of it
    assert TR.walk([-9.0, 0.0, 0.0], good[3:], 9.0, dims, origin, v, 0.75, 0.75)[0] == "ok"
    state, voxels = TR.walk(good[:3], good[3:], 0.5, dims, origin, v, 0.75, math.inf)
    assert state == "ok" and voxels == [(i, 3, 2) for i in range(4, 9)]                                # x = 0 lies in voxel 4: [-0.125, 0.125)


# ------------------------------------------------------------------------------------------------ known answer
def test_plane_seen_by_parallel_rays(table):
    """Rays along +x from the plane x = 0 hit the plane x = X, which lies between nodes.  Every vertex has |x - X| <= 1e-5 m: q
    quantises s to trunc 2^-21, the interpolation divides by a slope of v / trunc per voxel, so the position is off by about
    trunc 2^-20 = 7e-7 m, and fp32 coordinates round by less than 2e-6 m below 8 m.  No vertex lies behind X + trunc, and the
    triangles face -x, the side the rays came from."""
    v, X = 0.25, 2.6
    trunc = 3 * v
    dims, origin = (17, 5, 6), (0.0, -0.5, 1.0)                             # x up to 4 m, the box well below 8 m
    rays, ranges = [], []
    for m in range(2 * dims[1]):
        for n in range(2 * dims[2]):                                        # four rays through every voxel column, off its axis
            rays.append([0.0, origin[1] + (0.5 * m - 0.25) * v, origin[2] + (0.5 * n - 0.25) * v, 1.0, 0.0, 0.0])
            ranges.append(X)
    sum_, count, info = TR.integrate(rays, ranges, dims, origin, v, trunc, trunc)
    assert info[1] == len(rays) and info[2] == info[3] == 0
    assert (count.reshape(dims[0], -1) == count[:, :1, 0]).all() and set(np.unique(count)) == {0, 4}
    mesh = TR.extract_mesh(sum_, count, origin, v, table)
    assert mesh is not None
    verts, faces = mesh
    assert faces.shape[0] == 2 * (dims[1] - 1) * (dims[2] - 1) and verts.shape[0] == dims[1] * dims[2]
    err = np.abs(verts[:, 0] - X).max()
    print(f"plane at x = {X}: max |x - X| {err:.3e} m over {verts.shape[0]} vertices")
    assert err <= 1e-5
    assert verts[:, 0].max() <= X + trunc
    a, b, c = (verts[faces[:, k]] for k in range(3))
    normals = np.cross(b - a, c - a)
    assert (normals[:, 0] < 0).all() and np.abs(normals[:, 1:]).max() <= 1e-6 * np.abs(normals[:, 0]).min()
    # the field itself: minus the mean of s / trunc, clipped at 1 in front, nothing behind the truncation
    field, valid = TR.field(sum_, count)
    x = origin[0] + np.arange(dims[0]) * v
    s = X - x
    want = np.where(s >= -trunc, -np.minimum(s / trunc, 1.0), 0.0)
    seen = (s >= -trunc) & (s <= trunc + 0.5 * v + 1e-12)                   # the voxels of the segment [X - trunc, X + trunc]
    assert (valid[:, 0, 0] != 0).tolist() == seen.tolist()
    assert np.abs(field[:, 0, 0] - want)[seen].max() <= 2.0 ** -20
    assert (field[~seen] == 0).all()


# ------------------------------------------------------------------------------------------------ masked marching cubes
def _volume(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=shape).astype(np.float32)


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 2, 2), (5, 4, 3), (9, 7, 5)])
def test_masked_marching_cubes_with_every_node_valid_is_the_unmasked_one(table, shape):
    vol = _volume(shape, 3)
    sp, org = (0.25, 0.5, 0.125), (-1.0, 2.0, 0.5)
    want_v, want_f = MR.marching_cubes(vol, 0.1, table, sp, org)
    got_v, got_f = TR.marching_cubes_masked(vol, np.ones(shape, dtype=np.uint8), 0.1, table, sp, org)
    assert got_v.dtype == want_v.dtype and got_f.dtype == want_f.dtype
    assert got_v.tobytes() == want_v.tobytes() and got_f.tobytes() == want_f.tobytes()
    assert want_f.shape[0] > 0


def _triangles_per_cell(vol, valid, table):
    """{cell: its triangles as sorted vertex positions}, found from the geometry: a triangle lies in the cell that holds its centroid"""
    verts, faces = TR.marching_cubes_masked(vol, valid, 0.0, table)
    out = {}
    for f in faces:
        cell = tuple(np.floor(verts[f].astype(np.float64).mean(0) + 0).astype(int))
        out.setdefault(cell, []).append(sorted(map(tuple, verts[f].tolist())))
    return {k: sorted(t) for k, t in out.items()}, verts, faces


def test_clearing_one_corner_removes_the_cells_that_share_it_and_no_other(table):
    shape = (5, 4, 4)
    vol = _volume(shape, 5)
    # (a centroid on a cell's face would be ambiguous: random values put none there)
    full, _, _ = _triangles_per_cell(vol, np.ones(shape, dtype=np.uint8), table)
    corner = (2, 2, 1)
    valid = np.ones(shape, dtype=np.uint8)
    valid[corner] = 0
    masked, verts, faces = _triangles_per_cell(vol, valid, table)
    sharing = {(corner[0] - dx, corner[1] - dy, corner[2] - dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
    assert len(sharing & set(full)) >= 4, "the cleared corner should touch cells that had triangles"
    assert set(masked) == set(full) - sharing
    for cell in masked:
        assert masked[cell] == full[cell]
    # every vertex lies on an edge with two valid ends: none on an edge of the cleared node
    on_edge = np.abs(verts - np.asarray(corner, dtype=np.float32)).sum(1) < 1.0
    assert not on_edge.any()
    assert faces.shape[0] == 0 or faces.max() < verts.shape[0]


def test_masked_marching_cubes_of_nothing_valid_is_empty(table):
    vol = _volume((3, 3, 3), 7)
    verts, faces = TR.marching_cubes_masked(vol, np.zeros((3, 3, 3), dtype=np.uint8), 0.0, table)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("kwargs", [
    dict(min_bound=(0, 0, 0), max_bound=(1, 1, 0)),                          # no extent
    dict(min_bound=(0, 0, 0), max_bound=(1, -1, 1)),
    dict(min_bound=(0, 0), max_bound=(1, 1, 1)),
    dict(min_bound=(0, 0, math.nan), max_bound=(1, 1, 1)),
    dict(max_bound=(1, 1, math.inf)),
    dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=math.nan), dict(voxel_size=math.inf),
    dict(sdf_trunc=0.0), dict(sdf_trunc=-1.0), dict(sdf_trunc=math.nan),
    dict(sdf_trunc=0.3, front=0.2), dict(front=math.nan), dict(front=0.1),
    dict(voxel_size=1e-4),                                                   # 10^12 nodes
    dict(max_bound=(1e12, 1, 1)),
])
def test_volume_refuses_bad_arguments_before_it_touches_a_device(kwargs):
    from loner_amd.analysis.tsdf import TSDFVolume
    args = dict(min_bound=(0.0, 0.0, 0.0), max_bound=(1.0, 1.0, 1.0), voxel_size=0.1)
    args.update(kwargs)
    with pytest.raises(ValueError):
        TSDFVolume(**args)


def test_fuse_scans_refuses_bad_arguments_before_it_touches_a_device():
    from loner_amd.analysis.tsdf import fuse_scans
    rows = np.array([[0.0, 0, 0, 0, 0, 0, 0, 1], [1.0, 1, 0, 0, 0, 0, 0, 1]])
    with pytest.raises(ValueError):
        fuse_scans([], rows, ((0, 0, 0),), 0.1)
    with pytest.raises(ValueError):
        fuse_scans([], rows[:1], ((0, 0, 0), (1, 1, 1)), 0.1)
    with pytest.raises(ValueError):
        fuse_scans([], rows, ((0, 0, 0), (1, 1, 1)), 0.0)


def test_ops_refuse_host_tensors_and_bad_volumes():
    from loner_amd import ops
    sum_ = torch.zeros(3, 3, 3, dtype=torch.int64)
    count = torch.zeros(3, 3, 3, dtype=torch.int32).view(torch.uint32)
    with pytest.raises(RuntimeError):
        ops.tsdf_integrate(torch.zeros(1, 6, dtype=torch.float64), torch.ones(1, dtype=torch.float64), sum_, count, (0, 0, 0), 0.1, 0.3)
    with pytest.raises(RuntimeError):
        ops.tsdf_field(sum_, count)
    with pytest.raises(RuntimeError):
        ops.marching_cubes(torch.zeros(3, 3, 3), valid=torch.ones(3, 3, 3, dtype=torch.uint8))
