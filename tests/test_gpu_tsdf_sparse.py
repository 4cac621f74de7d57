"""The sparse TSDF volume on the GPU: integration against the restatement (tests/tsdf_sparse_restatement.py) and against the dense
kernels byte for byte, the directory rule, growth, high keys, the field, and marching cubes over blocks against the masked restatement
on the full lattice.  Meshes are compared as sets of triangles through one comparator, SR.triangle_rows: bytes, never a tolerance.
The wrappers under test are loner_amd.analysis.tsdf_sparse's (SP): the public surface of loner_amd.ops is pinned by
tests/test_ops_api_host.py, so sparse_tsdf_integrate, sparse_tsdf_field and sparse_marching_cubes live beside the volume."""
import functools
import math

import numpy as np
import pytest
import torch

from loner_amd.utils import synthetic as SYN
from loner_amd.utils import synthetic_mesh as SM
from tests import tsdf_restatement as TR
from tests import tsdf_sparse_restatement as SR

pytestmark = pytest.mark.gpu

DEV = "cuda"
GRID = ((9, 7, 5), (-1.0, -0.75, -0.5), 0.25)                           # two partial blocks: the second is one node thick
GRID_BLOCKS = ((17, 9, 26), (-2.0, -1.0, -3.0), 0.25)                   # 3 x 2 x 4 blocks, all upper blocks partial
GRID_ORDER = ((33, 17, 9), (-4.0, -2.0, -1.0), 0.25)                    # the lattice of the dense order test: 5 x 3 x 2 blocks


def _t(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _volume(dims, origin, v, trunc, front, **kw):
    from loner_amd.analysis.tsdf import SparseTSDFVolume
    hi = [origin[a] + (dims[a] - 1) * v for a in range(3)]
    vol = SparseTSDFVolume(origin, hi, v, trunc, front, device=DEV, **kw)
    assert vol.dims == tuple(dims) and vol.n_blocks == 0
    return vol


def _add(vol, rays, ranges):
    """-> the eight info words of the call"""
    got = vol.integrate_rays(_t(rays).reshape(-1, 6), _t(ranges).reshape(-1))
    assert got["rays"] == len(ranges)
    return [0, got["updated_rays"], got["invalid_rays"], got["missed_rays"], got["node_updates"], got["new_blocks"], got["blocks"],
            got["lost_updates"]]


def _u32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _state(vol):
    """-> (keys int64 [B], slots int64 [B], pool sum [B,8,8,8], pool count [B,8,8,8]) on the host"""
    b = vol.n_blocks
    return (vol.store.keys[:b].cpu().numpy(), vol.store.slot[:b].cpu().numpy().astype(np.int64), vol.store.sum[:b].cpu().numpy(),
            _u32(vol.store.count[:b]))


def _ordered(vol):
    """-> (block_indices, sum, count) in directory order, on the host"""
    sum_, count = vol.blocks()
    return vol.block_indices().cpu().numpy(), sum_.cpu().numpy(), _u32(count)


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}[{k}]: {g.dtype} {g.shape}, want {w.dtype} {w.shape}"
        assert g.tobytes() == w.tobytes(), f"{what}[{k}] differs on {int((g != w).sum())} of {g.size} words"


def _assert_is_restatement(vol, ref, what):
    keys, slots, pool_sum, pool_count = _state(vol)
    _same((keys, slots), (ref.keys(), ref.slots()), f"{what}: directory")
    _same((pool_sum, pool_count), ref.pool(), f"{what}: pool")
    idx, sum_, count = _ordered(vol)
    _same((idx, sum_, count), (ref.block_indices(),) + ref.directory_order(), f"{what}: directory order")
    assert count.shape[0] == 0 or (count.reshape(count.shape[0], -1).astype(np.int64).sum(1) > 0).all(), f"{what}: a block nobody wrote to"


@functools.lru_cache(maxsize=None)
def _table():
    from loner_amd import ops
    return ops.mc_case_table()


# ---------------------------------------------------------------- 1. integration against the restatement
@functools.lru_cache(maxsize=None)
def _rays_of(grid_name):
    """the ray set of the lattice and rays the call must count and leave out (those of tests/test_gpu_tsdf.py's _grid_rays)"""
    dims, origin, v = {"grid": GRID, "blocks": GRID_BLOCKS}[grid_name]
    rays, ranges = TR.ray_set(dims, origin, v, 11)
    extra, extra_r = [], []
    good = [0.1, 0.05, 0.02, 0.6, 0.64, 0.48]
    for k in range(6):
        for bad in (math.nan, math.inf):
            ray = list(good)
            ray[k] = bad
            extra.append(ray); extra_r.append(1.0)
    extra.append([math.nan] * 6); extra_r.append(1.0)
    extra.append(good[:3] + [0.0, 0.0, 0.0]); extra_r.append(1.0)
    for r in (0.0, -0.5, math.nan, math.inf, -math.inf):
        extra.append(list(good)); extra_r.append(r)
    far = 9.0 + abs(origin[0])
    extra.append([far, 0.0, 0.0, 1.0, 0.0, 0.0]); extra_r.append(1.0)   # misses: starts behind the box, ends before it, passes beside it
    extra.append([-far, 0.0, 0.0, 1.0, 0.0, 0.0]); extra_r.append(1.0)
    extra.append([-far, far, 0.0, 1.0, 0.0, 0.0]); extra_r.append(far)
    return np.concatenate([rays, np.asarray(extra)]), np.concatenate([ranges, np.asarray(extra_r)])


@functools.lru_cache(maxsize=None)
def _reference(grid_name, carve):
    dims, origin, v = {"grid": GRID, "blocks": GRID_BLOCKS}[grid_name]
    rays, ranges = _rays_of(grid_name)
    ref = SR.SparseVolume(dims, origin, v, 3 * v, math.inf if carve else 3 * v)
    return ref, ref.integrate(rays, ranges)


@pytest.mark.parametrize("grid_name", ["grid", "blocks"])
@pytest.mark.parametrize("carve", [False, True])
def test_integration_bit_for_bit(grid_name, carve):
    dims, origin, v = {"grid": GRID, "blocks": GRID_BLOCKS}[grid_name]
    rays, ranges = _rays_of(grid_name)
    ref, want_info = _reference(grid_name, carve)
    vol = _volume(dims, origin, v, 3 * v, math.inf if carve else 3 * v)
    info = _add(vol, rays, ranges)
    print(f"{dims}, carve {carve}: {len(rays)} rays, info {info}, want {want_info}")
    assert info == want_info
    assert info[2] == 12 + 1 + 1 + 5 and info[3] >= 3 and info[5] == info[6] == vol.n_blocks >= 1 and info[7] == 0
    assert vol.n_blocks == 2 if grid_name == "grid" else vol.n_blocks > 8
    _assert_is_restatement(vol, ref, f"{dims} carve {carve}")
    dense = vol.to_dense()
    _same((dense[0].cpu().numpy(), _u32(dense[1])), tuple(ref.to_dense()), "to_dense")
    # a second identical call doubles every word and creates no block
    before = _state(vol)
    again = _add(vol, rays, ranges)
    assert again == want_info[:5] + [0, want_info[6], 0]
    after = _state(vol)
    _same(after[:2], before[:2], "directory after the second call")
    _same(after[2:], (2 * before[2], 2 * before[3]), "pool after the second call")


# ---------------------------------------------------------------- 2. equality with the dense kernels
@functools.lru_cache(maxsize=None)
def _order_rays():
    """the 70 000 random rays of the dense order test"""
    dims, origin, v = GRID_ORDER
    rng = np.random.default_rng(21)
    n = 70000
    lo, size = np.asarray(origin) - 0.5 * v, np.asarray(dims) * v
    o = lo + rng.uniform(-0.2, 1.2, (n, 3)) * size
    d = lo + rng.uniform(0.0, 1.0, (n, 3)) * size - o
    length = np.linalg.norm(d, axis=1)
    return np.concatenate([o, d / length[:, None]], axis=1), length * rng.uniform(0.5, 1.2, n), rng.permutation(n)


def test_equals_the_dense_kernels_whatever_the_order_and_the_split():
    from loner_amd import ops
    dims, origin, v = GRID_ORDER
    rays, ranges, order = _order_rays()
    n = len(ranges)
    dense_sum = torch.zeros(dims, dtype=torch.int64, device=DEV)
    dense_count = torch.zeros(dims, dtype=torch.int32, device=DEV).view(torch.uint32)
    dense_info = ops.tsdf_integrate(_t(rays), _t(ranges), dense_sum, dense_count, origin, v, 0.75, math.inf).cpu().tolist()
    first = _volume(dims, origin, v, 0.75, math.inf)
    info = _add(first, rays, ranges)
    assert info[:5] == dense_info[:5] and info[5] == info[6] == first.n_blocks and info[7] == 0 and info[4] > 10 * n
    got = first.to_dense()
    want_count = _u32(dense_count)
    _same((got[0].cpu().numpy(), _u32(got[1])), (dense_sum.cpu().numpy(), want_count), "to_dense against ops.tsdf_integrate")
    # the existing blocks are exactly the blocks holding a node with count > 0
    holding = sorted({SR.pack_key(i >> 3, j >> 3, k >> 3) for i, j, k in np.argwhere(want_count > 0).tolist()})
    assert first.store.keys[:first.n_blocks].cpu().tolist() == holding and 1 < len(holding) <= 30
    want = _ordered(first)
    second = _volume(dims, origin, v, 0.75, math.inf)
    _add(second, rays, ranges)
    _same(_ordered(second), want, "second run")
    _same(_state(second), _state(first), "second run: pool")
    permuted = _volume(dims, origin, v, 0.75, math.inf)
    _add(permuted, rays[order], ranges[order])
    _same(_ordered(permuted), want, "permuted rays")
    _same(_state(permuted), _state(first), "permuted rays: pool")        # one call, the same set: the same pool too
    # two calls, in either order: few enough rays in one of them to leave blocks for the other
    cut = 2
    ab, ba = _volume(dims, origin, v, 0.75, math.inf), _volume(dims, origin, v, 0.75, math.inf)
    info_a = _add(ab, rays[:cut], ranges[:cut])
    info_b = _add(ab, rays[cut:], ranges[cut:])
    _add(ba, rays[cut:], ranges[cut:])
    _add(ba, rays[:cut], ranges[:cut])
    assert 0 < info_a[5] < len(holding) and info_b[5] == len(holding) - info_a[5] and info_a[7] == info_b[7] == 0
    _same(_ordered(ab), want, "two calls")
    _same(_ordered(ba), want, "two calls, the other order")
    assert _state(ab)[1].tobytes() != _state(ba)[1].tobytes() and _state(ab)[3].tobytes() != _state(ba)[3].tobytes()


# ---------------------------------------------------------------- 3. growth
def test_growth_keeps_every_block():
    dims, origin, v = GRID_ORDER
    rays, ranges, _ = _order_rays()
    calls = [(rays[:4], ranges[:4]), (rays[:4], ranges[:4]), (rays[4:3000], ranges[4:3000])]
    small, roomy = _volume(dims, origin, v, 0.75, 0.75, initial_blocks=2), _volume(dims, origin, v, 0.75, 0.75)
    assert small.store.capacity == 2 and roomy.store.capacity == 4096 and small.memory_bytes() == 0
    new = []
    for call in calls:
        a, b = _add(small, *call), _add(roomy, *call)
        assert a == b and a[7] == 0
        new.append(a[5])
    print(f"growth: new blocks per call {new}, capacity {small.store.capacity}")
    assert new[0] > 2 and new[1] == 0 and new[2] > 0 and small.n_blocks == sum(new) <= small.store.capacity < 4096
    _same(_state(small), _state(roomy), "pool")
    _same(_ordered(small), _ordered(roomy), "directory order")
    assert small.memory_bytes() == roomy.memory_bytes() and small.allocated_bytes() < roomy.allocated_bytes()
    # a call of no rays changes nothing
    before = _state(small)
    empty = small.integrate_rays(torch.zeros(0, 6, dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV))
    assert empty == {"rays": 0, "updated_rays": 0, "invalid_rays": 0, "missed_rays": 0, "node_updates": 0, "new_blocks": 0,
                     "blocks": small.n_blocks, "lost_updates": 0}
    _same(_state(small), before, "after no rays")
    # reset, and the empty volume
    small.reset()
    assert small.n_blocks == 0 and small.n_rays == 0 and small.store.capacity == 2
    assert small.extract_mesh() is None
    assert small.block_indices().shape == (0, 3) and small.blocks()[0].shape == (0, 8, 8, 8) and small.field()[0].shape == (0, 8, 8, 8)
    assert int(small.to_dense()[1].view(torch.int32).abs().sum()) == 0
    assert small.integrate_rays(torch.zeros(0, 6, device=DEV), torch.zeros(0, device=DEV))["blocks"] == 0


# ---------------------------------------------------------------- 4. many copies of one ray
def test_many_copies_of_one_ray_land_on_the_same_nodes():
    dims, origin, v = GRID_BLOCKS
    ray, r, trunc = np.array([-2.3, -0.6, -2.4, 0.6, 0.48, 0.64]), 2.9, 0.75
    one = SR.SparseVolume(dims, origin, v, trunc, math.inf)
    one_info = one.integrate(ray[None], [r])
    assert one_info[4] >= 8 and one_info[5] >= 2 and max(int(c.max()) for _, c in one.blocks.values()) == 1
    n = 4096
    vol = _volume(dims, origin, v, trunc, math.inf)
    info = _add(vol, np.tile(ray, (n, 1)), np.full(n, r))
    assert info == [0, n, 0, 0, n * one_info[4], one_info[5], one_info[6], 0]
    keys, slots, pool_sum, pool_count = _state(vol)
    _same((keys, slots), (one.keys(), one.slots()), "directory")
    _same((pool_sum, pool_count), (n * one.pool()[0], (n * one.pool()[1]).astype(np.uint32)), "4096 copies")


# ---------------------------------------------------------------- 5. high keys
@functools.lru_cache(maxsize=None)
def _far_rays():
    """ray_set rays in two windows of 8 x 16 x 16 nodes of a lattice of 2^21 nodes along x at v = 0.25: one that ends at the last node
    (around x = 2^21 - 5: block coordinate 2^18 - 1) and one around x = 2^20 (block coordinates 2^17 - 1 and 2^17)"""
    v = 0.25
    rays, ranges = [], []
    for x0, seed in (((1 << 21) - 8, 31), ((1 << 20) - 4, 32)):
        a, b = TR.ray_set((8, 16, 16), (x0 * v, 0.0, 0.0), v, seed, n_random=12)
        rays.append(a[::2]); ranges.append(b[::2])                      # (every second ray: about 240 in all)
    return np.concatenate(rays), np.concatenate(ranges)


@pytest.mark.parametrize("nz", [16, 64])
def test_high_keys_on_a_lattice_of_two_million_nodes_along_x(nz):
    """(2^21, 16, 16) is the issue's lattice; its 2^29 nodes are fewer than TSDFVolume's limit of 2^31 - 1, so the dense volume's refusal
    is asserted on (2^21, 16, 64), 2^31 nodes, with the same rays (they stay below z = 16)."""
    from loner_amd.analysis.tsdf import TSDFVolume
    dims, origin, v = (1 << 21, 16, nz), (0.0, 0.0, 0.0), 0.25
    rays, ranges = _far_rays()
    assert 200 <= len(ranges) <= 260
    ref = SR.SparseVolume(dims, origin, v, 0.75, 0.75)
    want_info = ref.integrate(rays, ranges)
    vol = _volume(dims, origin, v, 0.75, 0.75)
    info = _add(vol, rays, ranges)
    print(f"{dims}: {len(ranges)} rays, info {info}")
    assert info == want_info and info[7] == 0 and info[1] > 60
    _assert_is_restatement(vol, ref, "high keys")
    bx = ref.block_indices()[:, 0]
    assert SR.sort_passes(dims) == 7 and int(ref.keys().max()) >= 1 << 53
    assert {(1 << 18) - 1, 1 << 17, (1 << 17) - 1} <= set(bx.tolist())
    again = _add(vol, rays, ranges)
    assert again[5] == 0 and again[4] == want_info[4] and again[7] == 0
    hi = [(n - 1) * v for n in dims]
    if nz == 64:
        with pytest.raises(ValueError):
            TSDFVolume(origin, hi, v, 0.75, device=DEV)
        with pytest.raises(ValueError):
            vol.to_dense()


# ---------------------------------------------------------------- 6. the field
@pytest.mark.parametrize("carve", [False, True])
def test_field_bit_for_bit(carve):
    dims, origin, v = GRID_BLOCKS
    ref, _ = _reference("blocks", carve)
    vol = _volume(dims, origin, v, 3 * v, math.inf if carve else 3 * v)
    _add(vol, *_rays_of("blocks"))
    for min_count in (1, 2):
        field, valid = vol.field(min_count)
        assert field.dtype == torch.float32 and valid.dtype == torch.uint8
        _same((field.cpu().numpy(), valid.cpu().numpy()), ref.field(min_count), f"field, min_count {min_count}")
    assert int(vol.field(1)[1].sum()) > int(vol.field(2)[1].sum()) > 0


# ---------------------------------------------------------------- 7. marching cubes over blocks
def _all_blocks(dims):
    nb = [(n + 7) // 8 for n in dims]
    return [(x, y, z) for x in range(nb[0]) for y in range(nb[1]) for z in range(nb[2])]


MC_CASES = {
    "2x2x2": ((2, 2, 2), None, 1.0),
    "one full block": ((8, 8, 8), None, 1.0),
    "second block one node thick": ((9, 8, 8), None, 1.0),
    "eight blocks": ((16, 16, 16), None, 1.0),
    "one block missing": ((16, 16, 16), [b for b in _all_blocks((16, 16, 16)) if b != (1, 0, 1)], 1.0),
    "two diagonal blocks": ((16, 16, 16), [(0, 0, 0), (1, 1, 1)], 1.0),
    "half the blocks, a tenth of the nodes invalid": ((17, 9, 10), "half", 0.9),
}
# (17, 9, 10): the seed under which the random half holds cells with eight valid corners across a block face along every axis
MC_SEEDS = {"half the blocks, a tenth of the nodes invalid": 59}


def _mc_inputs(name):
    dims, blocks, p_valid = MC_CASES[name]
    rng = np.random.default_rng(MC_SEEDS.get(name, len(name) + sum(dims)))
    if blocks is None:
        blocks = _all_blocks(dims)
    elif blocks == "half":
        every = _all_blocks(dims)
        blocks = [every[i] for i in sorted(rng.permutation(len(every))[:len(every) // 2].tolist())]
    keys = np.asarray(sorted(SR.pack_key(*b) for b in blocks), dtype=np.int64)
    field = rng.normal(size=(len(keys), 8, 8, 8)).astype(np.float32)
    valid = (rng.uniform(size=field.shape) < p_valid).astype(np.uint8)     # (set beyond dims too: those bytes must not be read)
    return dims, keys, field, valid


@pytest.mark.parametrize("name", list(MC_CASES))
def test_sparse_marching_cubes_is_the_masked_mesh_of_the_full_lattice(name):
    from loner_amd.analysis import tsdf_sparse as SP
    dims, keys, field, valid = _mc_inputs(name)
    level, sp, org = 0.1, (0.25, 0.5, 0.125), (-1.0, 2.0, 0.5)
    want_v, want_f = SR.marching_cubes(keys, field, valid, dims, level, _table(), sp, org)
    verts, faces = SP.sparse_marching_cubes(_t(keys, np.int64), _t(field, np.float32), _t(valid, np.uint8), dims, level, sp, org)
    got_v, got_f = verts.cpu().numpy(), faces.cpu().numpy()
    print(f"{name}: {len(keys)} blocks, {got_v.shape[0]} vertices, {got_f.shape[0]} triangles (want {want_v.shape[0]}, {want_f.shape[0]})")
    assert got_v.dtype == np.float32 and got_f.dtype == np.int32
    assert got_v.shape == want_v.shape and got_f.shape == want_f.shape and want_f.shape[0] > 0
    assert got_f.min() >= 0 and got_f.max() < got_v.shape[0]
    assert SR.triangle_rows(got_v, got_f) == SR.triangle_rows(want_v, want_f)
    # the vertices are the same set as well (a vertex no triangle uses included)
    assert sorted(map(bytes, got_v)) == sorted(map(bytes, want_v))
    # the case has triangles of cells that straddle a block face on every axis with a neighbour block, and so corners with edges
    # owned by a node in the +x, +y and +z neighbour
    f, ok = SR.densify(keys, (field, valid), dims, (np.float32, np.uint8))
    present = {SR.unpack_key(k) for k in keys}
    for axis in range(3):
        step = tuple(1 if a == axis else 0 for a in range(3))
        if not any(tuple(b[a] + step[a] for a in range(3)) in present for b in present):
            continue
        cells = 0
        for i, j, k in np.argwhere(ok[:-1, :-1, :-1] != 0).tolist():
            if (i, j, k)[axis] & 7 != 7:
                continue
            corners = f[i:i + 2, j:j + 2, k:k + 2] > np.float32(level)
            if ok[i:i + 2, j:j + 2, k:k + 2].all() and corners.any() and not corners.all():
                cells += 1
        assert cells > 0, f"{name}: no cell straddles a block face along axis {axis}"
    # a valid byte beyond dims changes nothing, down to the order
    masked = valid.copy()
    idx = np.asarray([SR.unpack_key(k) for k in keys])
    for b in range(len(keys)):
        for a in range(3):
            beyond = np.arange(8) + 8 * idx[b, a] >= dims[a]
            np.moveaxis(masked[b], a, 0)[beyond] = 0
    verts2, faces2 = SP.sparse_marching_cubes(_t(keys, np.int64), _t(field, np.float32), _t(masked, np.uint8).bool(), dims, level, sp, org)
    assert torch.equal(verts2, verts) and torch.equal(faces2, faces)


def test_sparse_marching_cubes_refuses_a_wrong_directory():
    from loner_amd.analysis import tsdf_sparse as SP
    field = torch.zeros(2, 8, 8, 8, device=DEV)
    valid = torch.ones(2, 8, 8, 8, dtype=torch.uint8, device=DEV)
    key = lambda *b: SR.pack_key(*b)
    for keys, dims in (([key(1, 0, 0), key(0, 0, 0)], (16, 16, 16)),            # not ascending
                       ([key(0, 0, 1), key(0, 0, 1)], (16, 16, 16)),            # not unique
                       ([key(0, 0, 0), key(2, 0, 0)], (16, 16, 16)),            # outside dims
                       ([key(0, 0, 0), key(0, 1, 0)], (16, 8, 16)),
                       ([-1, key(0, 0, 0)], (16, 16, 16))):
        with pytest.raises(ValueError):
            SP.sparse_marching_cubes(torch.tensor(keys, dtype=torch.int64, device=DEV), field, valid, dims)
    good = torch.tensor([key(0, 0, 0), key(1, 0, 0)], dtype=torch.int64, device=DEV)
    for args in ((good, field[:1], valid, (16, 16, 16)), (good, field, valid.float(), (16, 16, 16)), (good.int(), field, valid, (16, 16, 16)),
                 (good, field, valid, (16, 16)), (good, field, valid, (16, 16, 1)), (good, field, valid, ((1 << 21) + 1, 16, 16))):
        with pytest.raises(ValueError):
            SP.sparse_marching_cubes(*args)
    with pytest.raises(RuntimeError):
        SP.sparse_marching_cubes(good.cpu(), field, valid, (16, 16, 16))
    verts, faces = SP.sparse_marching_cubes(good, field, valid, (16, 16, 16))                 # a constant field: nothing crosses
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


# ---------------------------------------------------------------- 8. the room
V_ROOM = 0.2


def _tum_rows():
    """the five poses of tests/test_gpu_tsdf.py's room"""
    rows = []
    for k in range(5):
        h = math.radians(12.0) * k / 2.0
        rows.append([0.1 * k, -3.0 + 1.5 * k, 1.0 - 0.5 * k, 1.0 + 0.1 * k, 0.0, 0.0, math.sin(h), math.cos(h)])
    return np.asarray(rows)


def test_fused_room_gives_the_dense_mesh_in_less_memory():
    from loner_amd.analysis import lidar_sim
    from loner_amd.analysis.gt_map import load_trajectory
    from loner_amd.analysis.raycast import RaycastingScene
    from loner_amd.analysis.tsdf import SparseTSDFVolume, TSDFVolume, fuse_scans
    scene = RaycastingScene(*SM.box_room_mesh(), device=DEV)
    traj = load_trajectory(_tum_rows(), DEV)
    dirs, times = SYN.lidar_pattern(16, 128)
    scans = [lidar_sim.simulate_scan(scene, traj, dirs, times, stamp, (1.0, 50.0), range_sigma=0.0)[0] for stamp in (0.0, 0.1, 0.2)]
    bound = (np.asarray(SYN.BOX_MIN) - 1.0, np.asarray(SYN.BOX_MAX) + 1.0)
    dense_stats, sparse_stats = {}, {}
    dense = fuse_scans(scans, _tum_rows(), bound, V_ROOM, device=DEV, stats=dense_stats)
    sparse = fuse_scans(scans, _tum_rows(), bound, V_ROOM, device=DEV, stats=sparse_stats, sparse=True)
    assert type(dense) is TSDFVolume and type(sparse) is SparseTSDFVolume and sparse.dims == dense.dims == (211, 161, 51)
    assert sparse_stats["lost_updates"] == 0 and sparse_stats["blocks"] == sparse.n_blocks == sparse_stats["new_blocks"] > 0
    assert {k: sparse_stats[k] for k in dense_stats} == dense_stats
    got = sparse.to_dense()
    _same((got[0].cpu().numpy(), _u32(got[1])), (dense.sum.cpu().numpy(), _u32(dense.count)), "fused room")
    dense_bytes = 12 * math.prod(dense.dims)
    print(f"fused room: {sparse.n_blocks} blocks, {sparse.memory_bytes()} bytes in blocks ({sparse.allocated_bytes()} allocated), "
          f"dense {dense_bytes}")
    assert sparse.memory_bytes() < dense_bytes
    meshes = 0
    for min_count in (2, 1):
        a, b = sparse.extract_mesh(min_count), dense.extract_mesh(min_count)
        assert (a is None) == (b is None)
        if b is not None:
            print(f"fused room, min_count {min_count}: {b.triangles.shape[0]} triangles")
            assert a.vertices.shape == b.vertices.shape and a.triangles.shape == b.triangles.shape
            assert SR.triangle_rows(a.vertices, a.triangles) == SR.triangle_rows(b.vertices, b.triangles)
            meshes += 1
    assert meshes >= 1
    a, b = sparse.extract_mesh(1, min_component_triangles=20), dense.extract_mesh(1, min_component_triangles=20)
    assert (a is None) == (b is None) and (b is None or SR.triangle_rows(a.vertices, a.triangles) == SR.triangle_rows(b.vertices, b.triangles))


# ---------------------------------------------------------------- 9. refusals
def test_volume_refusals():
    from loner_amd.analysis import tsdf_sparse as SP
    from loner_amd.analysis.tsdf import MAX_RAYS, SparseTSDFVolume
    vol = SparseTSDFVolume((0, 0, 0), (1, 1, 1), 0.25, device=DEV)
    assert vol.dims == (5, 5, 5) and vol.store.count.dtype == torch.uint32 and vol.store.sum.dtype == torch.int64
    rays, ranges = torch.zeros(2, 6, dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        vol.integrate_rays(rays, ranges)
    with pytest.raises(RuntimeError):
        vol.integrate_rays(rays.to(DEV), ranges)
    with pytest.raises(ValueError):
        vol.integrate_rays(rays.to(DEV)[:, :5], ranges.to(DEV))
    with pytest.raises(ValueError):
        vol.integrate_rays(rays.to(DEV), ranges.to(DEV)[:1])
    with pytest.raises(ValueError):
        SparseTSDFVolume((0, 0, 0), (1, 1, 1), 0.25, sdf_trunc=0.5, front=0.25, device=DEV)
    with pytest.raises(ValueError):
        SparseTSDFVolume((0, 0, 0), ((1 << 21) * 0.25, 1, 1), 0.25, device=DEV)                # 2^21 + 1 nodes along x
    assert SparseTSDFVolume((0, 0, 0), (((1 << 21) - 1) * 0.25, 1, 1), 0.25, device=DEV, initial_blocks=1).dims == (1 << 21, 5, 5)
    with pytest.raises(ValueError):
        SparseTSDFVolume((0, 0, 0), (1, 1, 1), 0.25, device=DEV, initial_blocks=0)
    store = SP.SparseTSDFStore(DEV, 4)
    for args in ((rays.to(DEV), ranges.to(DEV), store, (5, 5, 1), (0, 0, 0), 0.25, 0.75),
                 (rays.to(DEV), ranges.to(DEV), store, ((1 << 21) + 1, 5, 5), (0, 0, 0), 0.25, 0.75),
                 (rays.to(DEV), ranges.to(DEV), store, (5, 5, 5), (0, 0, 0), 0.25, 0.75, 0.5),
                 (rays.to(DEV), ranges.to(DEV), store, (5, 5, 5), (0, 0, math.nan), 0.25, 0.75),
                 (rays.to(DEV), ranges.to(DEV), (vol.store.sum, vol.store.count), (5, 5, 5), (0, 0, 0), 0.25, 0.75)):
        with pytest.raises(ValueError):
            SP.sparse_tsdf_integrate(*args)
    with pytest.raises(ValueError):
        SP.sparse_tsdf_field(store, 0)
    assert vol.n_rays == 0 and vol.n_blocks == 0 and store.n_blocks == 0
    vol.n_rays = MAX_RAYS - 1
    with pytest.raises(ValueError):
        vol.integrate_rays(rays.to(DEV), ranges.to(DEV))
    got = vol.integrate_rays(rays.to(DEV)[:1], ranges.to(DEV)[:1])
    assert got["rays"] == 1 and got["invalid_rays"] == 1 and got["blocks"] == 0 and vol.n_rays == MAX_RAYS
