"""A numpy / plain-float restatement of the sparse TSDF volume, written from include/loner_hip.h ("sparse TSDF"), not from the kernels:
a dict of 8 x 8 x 8 blocks filled ray by ray through tests.tsdf_restatement.walk (which takes any dims), the directory and slot rule,
the field, the densified volume, and the mesh as the masked marching cubes of the densified field with the missing blocks not valid.
Meshes are compared as sets of triangles through one comparator, triangle_rows."""
import numpy as np

from tests import tsdf_restatement as TR

BLOCK = 8


def pack_key(bx, by, bz):
    return (int(bx) << 36) | (int(by) << 18) | int(bz)


def unpack_key(key):
    key = int(key)
    return key >> 36, (key >> 18) & 0x3FFFF, key & 0x3FFFF


def sort_passes(dims):
    """8-bit digit passes that sort the keys of a lattice: 18 bits per axis below the highest axis with more than one block"""
    bits = [((n - 1) >> 3).bit_length() for n in dims]
    total = 36 + bits[0] if bits[0] else (18 + bits[1] if bits[1] else bits[2])
    return max((total + 7) // 8, 1)


class SparseVolume:
    """blocks: key -> (sum int64 [8,8,8], count uint32 [8,8,8]); slot: key -> the block's slot in the pool"""

    def __init__(self, dims, origin, v, trunc, front):
        self.dims, self.origin = tuple(int(n) for n in dims), [float(x) for x in origin]
        self.v, self.trunc, self.front = float(v), float(trunc), float(front)
        self.blocks, self.slot = {}, {}

    def integrate(self, rays, ranges):
        """-> the call's eight info words"""
        rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
        ranges = np.asarray(ranges, dtype=np.float64).reshape(-1)
        origin, v, trunc = self.origin, self.v, self.trunc
        info = [0] * 8
        created = set()
        for ray, r in zip(rays.tolist(), ranges.tolist()):
            o, d = ray[:3], ray[3:]
            state, voxels = TR.walk(o, d, r, self.dims, origin, v, trunc, self.front)
            if state == "invalid":
                info[2] += 1
                continue
            if state == "miss":
                info[3] += 1
                continue
            wrote = 0
            for c in voxels:
                p = [origin[a] + float(c[a]) * v for a in range(3)]
                s = r - (((p[0] - o[0]) * d[0] + (p[1] - o[1]) * d[1]) + (p[2] - o[2]) * d[2])
                if not s >= -trunc:
                    continue                                            # visited only: no block comes of it
                key = pack_key(c[0] >> 3, c[1] >> 3, c[2] >> 3)
                if key not in self.blocks:
                    self.blocks[key] = (np.zeros((8, 8, 8), dtype=np.int64), np.zeros((8, 8, 8), dtype=np.uint32))
                    created.add(key)
                sum_, count = self.blocks[key]
                local = (c[0] & 7, c[1] & 7, c[2] & 7)
                sum_[local] += round(min(s / trunc, 1.0) * TR.ONE)     # (Python's round: ties to even)
                count[local] += 1
                wrote += 1
            info[1] += 1 if wrote else 0
            info[4] += wrote
        first = len(self.slot)
        for rank, key in enumerate(sorted(created)):                    # the call's new blocks: slots B_old, B_old + 1, ... in key order
            self.slot[key] = first + rank
        info[5], info[6] = len(created), len(self.blocks)
        return info

    def keys(self):
        return np.asarray(sorted(self.blocks), dtype=np.int64)

    def slots(self):
        return np.asarray([self.slot[k] for k in sorted(self.blocks)], dtype=np.int64)

    def block_indices(self):
        return np.asarray([unpack_key(k) for k in sorted(self.blocks)], dtype=np.int32).reshape(-1, 3)

    def directory_order(self):
        """-> (sum int64 [B,8,8,8], count uint32 [B,8,8,8]) in ascending key order"""
        order = sorted(self.blocks)
        if not order:
            return np.zeros((0, 8, 8, 8), dtype=np.int64), np.zeros((0, 8, 8, 8), dtype=np.uint32)
        return np.stack([self.blocks[k][0] for k in order]), np.stack([self.blocks[k][1] for k in order])

    def pool(self):
        """-> (sum, count) [B,8,8,8] in slot order"""
        sum_, count = self.directory_order()
        out_s, out_c = np.zeros_like(sum_), np.zeros_like(count)
        slots = self.slots()
        out_s[slots], out_c[slots] = sum_, count
        return out_s, out_c

    def to_dense(self):
        return densify(self.keys(), self.directory_order(), self.dims, (np.int64, np.uint32))

    def field(self, min_count=1):
        """-> (field float32 [B,8,8,8], valid uint8 [B,8,8,8]) in directory order"""
        return TR.field(*self.directory_order(), min_count)


def densify(keys, arrays, dims, dtypes):
    """blocks [B,8,8,8] in key order -> arrays of the lattice's shape, zero outside the blocks; what lies beyond dims is cut off"""
    padded = tuple((n + 7) // 8 * 8 for n in dims)
    out = []
    for blocks, dtype in zip(arrays, dtypes):
        full = np.zeros(padded, dtype=dtype)
        for key, block in zip(keys, blocks):
            bx, by, bz = unpack_key(key)
            full[8 * bx:8 * bx + 8, 8 * by:8 * by + 8, 8 * bz:8 * bz + 8] = block
        out.append(np.ascontiguousarray(full[:dims[0], :dims[1], :dims[2]]))
    return out


def marching_cubes(keys, field, valid, dims, level, table, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """The definition: lnr_mc_*_masked on the full lattice with every node of a missing block not valid -> (verts, faces)"""
    f, ok = densify(keys, (field, valid), dims, (np.float32, np.uint8))
    return TR.marching_cubes_masked(f, ok, level, table, spacing, origin)


def triangle_rows(verts, faces):
    """The comparator of every mesh comparison: the [F,9] fp32 array of each triangle's three vertex coordinates in emitted order, rows
    sorted lexicographically (on their bit patterns, so that the order is total) -> bytes"""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows = np.ascontiguousarray(verts[faces].reshape(-1, 9))
    bits = rows.view(np.uint32)
    order = np.lexsort(tuple(bits[:, c] for c in range(8, -1, -1)))
    return rows[order].tobytes()
