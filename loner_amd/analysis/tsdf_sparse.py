"""The device side of the sparse TSDF volume (analysis/tsdf.py: SparseTSDFVolume): the store of a volume's directory and pool, and
the wrappers of the header's "sparse TSDF" entry points - integration in its four calls, the field, marching cubes over blocks.
They live here, beside the volume, and not in loner_amd.ops, whose public surface is pinned (tests/test_ops_api_host.py).
Offline tools: rays and ranges of a float dtype are widened to fp64.  ValueError: an argument the caller got wrong, refused before a
launch.  RuntimeError: what only the data shows, and a tensor that is not on the device."""
import ctypes as C
import math
import time

import torch

from ..hip import _ptr, _stream, check, load, require_device
from ..ops._common import _float_rows, _positive, _scratch

SPARSE_MAX_AXIS = 1 << 21           # nodes per axis: 18 bits of block coordinate
_SORT_LIMIT = (1 << 31) - 4096      # pairs one sort takes


def sparse_block_keys(block_indices):
    """block coordinates int [B,3] (tensor) -> keys int64 [B]: bx << 36 | by << 18 | bz (include/loner_hip.h, "sparse TSDF")"""
    b = block_indices.to(torch.int64)
    return (b[:, 0] << 36) | (b[:, 1] << 18) | b[:, 2]


def sparse_block_indices(keys):
    """keys int64 [B] -> block coordinates int32 [B,3]"""
    k = keys.to(torch.int64)
    return torch.stack([k >> 36, (k >> 18) & 0x3FFFF, k & 0x3FFFF], dim=1).to(torch.int32)


class SparseTSDFStore:
    """The device arrays of a sparse TSDF volume (include/loner_hip.h, "sparse TSDF"): the directory .keys int64 [capacity] (ascending
    over the first .n_blocks) with .slot int32 [capacity], and the pool .sum int64 and .count uint32 [capacity,8,8,8].  The arrays
    grow by copy (amortised doubling): a block keeps its slot, so tensors taken before a growth are stale afterwards."""

    BLOCK_BYTES = 8 + 4 + 512 * (8 + 4)     # a key, a slot, 512 sums and 512 counts

    def __init__(self, device, initial_blocks=4096):
        if isinstance(initial_blocks, bool) or int(initial_blocks) != initial_blocks or not 1 <= initial_blocks < 1 << 31:
            raise ValueError(f"SparseTSDFStore: initial_blocks must be an integer in [1, 2^31), got {initial_blocks!r}")
        self.device = torch.device(device)
        self._initial = int(initial_blocks)
        self.reset()

    def _allocate(self, capacity):
        self.keys = torch.zeros(capacity, dtype=torch.int64, device=self.device)
        self.slot = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self.sum = torch.zeros(capacity, 8, 8, 8, dtype=torch.int64, device=self.device)
        self._count_words = torch.zeros(capacity, 8, 8, 8, dtype=torch.int32, device=self.device)
        self.count = self._count_words.view(torch.uint32)
        self.device = self.keys.device                      # (with its index: what the tensors of a call are compared against)

    @property
    def capacity(self):
        return int(self.keys.shape[0])

    def reset(self):
        """no block again, at the initial capacity"""
        self.n_blocks = 0
        self._allocate(self._initial)
        return self

    def reserve(self, n_blocks):
        """room for n_blocks blocks: grows once, to the larger of twice the capacity and n_blocks; old slots copied, new ones zero"""
        if n_blocks <= self.capacity:
            return
        old, b = (self.keys, self.slot, self.sum, self._count_words), self.n_blocks
        self._allocate(max(2 * self.capacity, int(n_blocks)))
        for new, was in zip((self.keys, self.slot, self.sum, self._count_words), old):
            new[:b].copy_(was[:b])


class _Laps:
    """lap(name): with a dict, waits for the device and stores the milliseconds since the last lap under name; without, nothing"""

    def __init__(self, out):
        self.out = out
        if out is not None:
            out.update(touch=0.0, insert=0.0, integrate=0.0)
            torch.cuda.synchronize()
            self.t = time.perf_counter()

    def __call__(self, name):
        if self.out is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.out[name] = (now - self.t) * 1e3
            self.t = now


def _sparse_dims(dims, what):
    try:
        nx, ny, nz = (int(x) for x in dims)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: dims must be three integers, got {dims!r}") from None
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) > SPARSE_MAX_AXIS:
        raise ValueError(f"{what}: every axis needs 2 to 2^21 nodes, got {nx} x {ny} x {nz}")
    return nx, ny, nz


def sparse_tsdf_integrate(rays, ranges, store, dims, origin, voxel_size, trunc, front=None, timings=None):
    """Adds rays to a sparse TSDF volume (include/loner_hip.h, "sparse TSDF": lnr_tsdf_sparse_touch, _insert, _merge, _integrate):
    rays [n,6] and ranges [n] as ops.tsdf_integrate takes them, store a SparseTSDFStore on their device, dims the lattice's (nx, ny, nz)
    (2 to 2^21 nodes per axis, no limit on the product).  New blocks enter the directory and the pool grows as needed.
    -> info int64 [8] on the device: {status, rays that updated a node, invalid rays, rays that miss the volume, node updates, new
    blocks, blocks, lost updates}.
    Device -> host reads, whatever n is: one, the candidate total, for a call that meets no new block; two for a call that creates
    blocks (then the number of new blocks, which sizes the pool).  The info words stay on the device for the caller to read.
    timings (a dict, optional, for measurements): receives the host-clock milliseconds of {"touch", "insert", "integrate"}, each ended
    by a device synchronisation, and the call's "candidates"."""
    what = "sparse_tsdf_integrate"
    if not isinstance(store, SparseTSDFStore):
        raise ValueError(f"{what}: store must be a SparseTSDFStore, got {type(store).__name__}")
    nx, ny, nz = _sparse_dims(dims, what)
    require_device(rays, ranges)
    _float_rows(rays, 6, what, "rays")
    n = rays.shape[0]
    if tuple(ranges.shape) != (n,) or not ranges.dtype.is_floating_point:
        raise ValueError(f"{what}: ranges [{n}] of a float dtype, got {tuple(ranges.shape)} {ranges.dtype}")
    if rays.device != store.device or ranges.device != store.device:
        raise ValueError(f"{what}: rays on {rays.device}, ranges on {ranges.device}, the volume on {store.device}")
    org = [float(x) for x in origin]
    if len(org) != 3 or not all(math.isfinite(x) for x in org):
        raise ValueError(f"{what}: origin must be three finite numbers, got {origin!r}")
    v, tr = _positive(voxel_size, what, "voxel_size"), _positive(trunc, what, "trunc")
    fr = tr if front is None else float(front)
    if not fr >= tr:
        raise ValueError(f"{what}: front must be at least trunc ({tr}), got {front!r}")
    r = rays.to(torch.float64).contiguous()
    rng = ranges.to(torch.float64).contiguous()
    dev, lib = store.device, load()
    lattice = (nx, ny, nz, (C.c_double * 3)(*org), v, tr, fr)
    n_new, candidates = 0, 0
    lap = _Laps(timings)
    if n > 0:
        offsets = torch.empty(n + 1, device=dev, dtype=torch.int32)
        counts = torch.empty(2, device=dev, dtype=torch.int64)
        ws, need = _scratch(lib.lnr_tsdf_sparse_workspace(n, 0), dev, f"{what}: {n} rays, the limit is 2^32 - 257")
        b_old = store.n_blocks
        check(lib.lnr_tsdf_sparse_touch(_ptr(r), _ptr(rng), n, *lattice, _ptr(store.keys), b_old, _ptr(offsets), _ptr(ws), need, _ptr(counts),
                                        _stream()), "lnr_tsdf_sparse_touch")
        candidates = int(counts[0].cpu())
        lap("touch")
        if candidates > 0:
            if b_old + candidates > _SORT_LIMIT:
                raise RuntimeError(f"{what}: {candidates} candidate blocks beside {b_old} blocks, one sort takes 2^31 - 4096: split the call")
            ws, need = _scratch(lib.lnr_tsdf_sparse_workspace(0, b_old + candidates), dev)
            check(lib.lnr_tsdf_sparse_insert(_ptr(r), _ptr(rng), n, *lattice, _ptr(store.keys), b_old, _ptr(offsets), candidates, _ptr(ws), need,
                                             _ptr(counts), _stream()), "lnr_tsdf_sparse_insert")
            n_new = int(counts[1].cpu())
            store.reserve(b_old + n_new)
            check(lib.lnr_tsdf_sparse_merge(_ptr(store.keys), _ptr(store.slot), b_old, n_new, candidates, nx, ny, nz, _ptr(ws), need,
                                            _ptr(store.keys), _ptr(store.slot), _stream()), "lnr_tsdf_sparse_merge")
            store.n_blocks = b_old + n_new
        lap("insert")
    info = torch.empty(8, device=dev, dtype=torch.int64)
    check(lib.lnr_tsdf_sparse_integrate(_ptr(r), _ptr(rng), n, *lattice, _ptr(store.keys), _ptr(store.slot), store.n_blocks, n_new,
                                        store.capacity, _ptr(store.sum), _ptr(store.count), _ptr(info), _stream()), "lnr_tsdf_sparse_integrate")
    lap("integrate")
    if timings is not None:
        timings["candidates"] = candidates
    return info


def sparse_tsdf_field(store, min_count=1):
    """A sparse TSDF volume's mean (include/loner_hip.h: lnr_tsdf_sparse_field) -> (field fp32 [B,8,8,8], valid uint8 [B,8,8,8]) in
    directory order (ascending key), with tsdf_field's expression and min_count rule; both empty for a volume without a block."""
    if not isinstance(store, SparseTSDFStore):
        raise ValueError(f"sparse_tsdf_field: store must be a SparseTSDFStore, got {type(store).__name__}")
    if isinstance(min_count, bool) or int(min_count) != min_count or not 1 <= min_count < 1 << 32:
        raise ValueError(f"sparse_tsdf_field: min_count must be an integer in [1, 2^32), got {min_count!r}")
    b = store.n_blocks
    field = torch.empty(b, 8, 8, 8, device=store.device, dtype=torch.float32)
    valid = torch.empty(b, 8, 8, 8, device=store.device, dtype=torch.uint8)
    if b > 0:
        check(load().lnr_tsdf_sparse_field(_ptr(store.sum), _ptr(store.count), _ptr(store.slot), b, store.capacity, int(min_count), _ptr(field),
                                           _ptr(valid), _stream()), "lnr_tsdf_sparse_field")
    return field, valid


def sparse_marching_cubes(block_keys, field, valid, dims, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """Marching cubes over the 8 x 8 x 8 blocks of a sparse volume (include/loner_hip.h: lnr_mc_sparse_*): block_keys int64 [B]
    (bx << 36 | by << 18 | bz, ascending), field fp32 and valid uint8 or bool [B,8,8,8] in that order, dims the lattice's (nx, ny, nz).
    -> (verts [V,3] fp32, faces [F,3] int32) on the device: the mesh of ops.marching_cubes(valid=...) over the whole lattice with the
    nodes of every missing block not valid, as a set of triangles (blocks in key order, not lattice order).  Keys that are not
    ascending, not unique or outside dims are refused (ValueError) before a launch.  Two device -> host reads: the key check and
    the two totals."""
    what = "sparse_marching_cubes"
    require_device(block_keys, field, valid)
    try:
        nx, ny, nz = (int(x) for x in dims)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: dims must be three integers, got {dims!r}") from None
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) > 1 << 21:
        raise ValueError(f"{what}: every axis needs 2 to 2^21 nodes, got {nx} x {ny} x {nz}")
    if block_keys.dim() != 1 or block_keys.dtype != torch.int64:
        raise ValueError(f"{what}: block_keys int64 [B], got {block_keys.dtype} {tuple(block_keys.shape)}")
    b, dev = int(block_keys.shape[0]), block_keys.device
    if tuple(field.shape) != (b, 8, 8, 8) or field.dtype != torch.float32 or field.device != dev:
        raise ValueError(f"{what}: field fp32 [{b},8,8,8] on {dev}, got {field.dtype} {tuple(field.shape)} on {field.device}")
    if tuple(valid.shape) != (b, 8, 8, 8) or valid.dtype not in (torch.uint8, torch.bool) or valid.device != dev:
        raise ValueError(f"{what}: valid uint8 or bool [{b},8,8,8] on {dev}, got {valid.dtype} {tuple(valid.shape)} on {valid.device}")
    if b >= 1 << 22:
        raise ValueError(f"{what}: {b} blocks, the limit is 2^22 - 1")
    verts = torch.empty(0, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(0, 3, device=dev, dtype=torch.int32)
    if b == 0:
        return verts, faces
    keys = block_keys.contiguous()
    nb = [(n + 7) >> 3 for n in (nx, ny, nz)]
    inside = (keys >= 0) & ((keys >> 36) < nb[0]) & (((keys >> 18) & 0x3FFFF) < nb[1]) & ((keys & 0x3FFFF) < nb[2])
    if not bool((inside.all() & (keys[1:] > keys[:-1]).all()).cpu()):
        raise ValueError(f"{what}: block_keys must be ascending, unique and inside the {nb[0]} x {nb[1]} x {nb[2]} blocks of dims")
    vol, mask = field.contiguous(), valid.to(torch.uint8).contiguous()
    lib = load()
    ws, need = _scratch(lib.lnr_mc_sparse_workspace(b), dev)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    check(lib.lnr_mc_sparse_count(_ptr(keys), b, _ptr(vol), _ptr(mask), nx, ny, nz, float(level), _ptr(ws), need, _ptr(totals), _stream()),
          "lnr_mc_sparse_count")
    n_verts, n_tris = (int(x) for x in totals.cpu())
    if n_verts >= 1 << 30:
        raise RuntimeError(f"{what}: {n_verts} vertices, the limit is 2^30 - 1")
    verts = torch.empty(n_verts, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(n_tris, 3, device=dev, dtype=torch.int32)
    sp = (C.c_float * 3)(*[float(x) for x in spacing])
    org = (C.c_float * 3)(*[float(x) for x in origin])
    check(lib.lnr_mc_sparse_emit(_ptr(keys), b, _ptr(vol), _ptr(mask), nx, ny, nz, float(level), sp, org, _ptr(ws), need, n_verts, n_tris,
                                 _ptr(verts), _ptr(faces), _stream()), "lnr_mc_sparse_emit")
    return verts, faces
