"""The synthetic scene of utils/synthetic.py as triangle meshes, for the ray caster (analysis/raycast.py) and the scan simulator
(analysis/lidar_sim.py): the box room as 12 triangles, the sphere as a subdivided icosahedron.  Everything is numpy fp64 / int32 on
the host: (vertices [V,3], triangles [F,3]).  The room's window (synthetic.py's transparent rays) is not modelled: the mesh is closed.
"""
import numpy as np

from .synthetic import BOX_MAX, BOX_MIN, SPHERE_C, SPHERE_R


def box_room_mesh(lo=BOX_MIN, hi=BOX_MAX):
    """The closed box [lo, hi] as 8 vertices and 12 triangles (two per face, sharing the face's diagonal; the ray caster does not cull by winding).
    Vertex i has x = hi when i & 1, y = hi when i & 2, z = hi when i & 4."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if i >> a & 1 else lo)[a] for a in range(3)] for i in range(8)], dtype=np.float64)
    f = np.array([[0, 4, 6], [0, 6, 2],         # x = lo
                  [1, 3, 7], [1, 7, 5],         # x = hi
                  [0, 1, 5], [0, 5, 4],         # y = lo
                  [2, 6, 7], [2, 7, 3],         # y = hi
                  [0, 2, 3], [0, 3, 1],         # z = lo
                  [4, 5, 7], [4, 7, 6]], dtype=np.int32)
    return v, f


def icosphere(subdivisions=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """The icosahedron with every triangle split in four `subdivisions` times, every vertex pushed onto the sphere: 20 * 4^s
    triangles, 10 * 4^s + 2 vertices, wound outwards, closed (shared vertices are shared indices)."""
    s = int(subdivisions)
    if s != subdivisions or not 0 <= s <= 8:
        raise ValueError(f"icosphere: subdivisions must be an integer in [0, 8], got {subdivisions!r}")
    r = float(radius)
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"icosphere: radius must be finite and > 0, got {radius!r}")
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.sqrt(1.0 + p * p) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(s):
        mid, out = {}, []

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.sqrt((m * m).sum()))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, dtype=np.float64) * r + np.asarray(centre, dtype=np.float64), np.asarray(f, dtype=np.int32)


def scene_mesh(sphere_subdivisions=4):
    """Room plus sphere: box_room_mesh() and icosphere(sphere_subdivisions, SPHERE_R, SPHERE_C) in one mesh (the room's 12 triangles
    first)."""
    bv, bf = box_room_mesh()
    sv, sf = icosphere(sphere_subdivisions, SPHERE_R, SPHERE_C)
    return np.concatenate([bv, sv]), np.concatenate([bf, sf + len(bv)]).astype(np.int32)
