"""Meshing on the CPU: the marching-cubes case table checked from first principles, the restatement of the reference's weight
accumulation against its literal op sequence (dtype rules of mesher.py:143-180), and the numpy marching cubes on analytic fields."""
import numpy as np
import pytest
import torch

from tests import mesh_restatement as MR


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as ge
    ge.build()
    from loner_amd import ops
    return ops.mc_case_table()


# ------------------------------------------------------------------------------------------------ case table
CORNERS = np.array([MR.corner_offset(c) for c in range(8)], dtype=np.float64)
EDGE_CORNERS = [MR.edge_corners(e) for e in range(12)]
MID = np.array([(CORNERS[a] + CORNERS[b]) / 2 for a, b in EDGE_CORNERS])


def _faces():
    """the six cube faces: (axis, side, the four corners in cyclic order)"""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for s in (0, 1):
            cyc = [(s << a) | (u << b) | (w << c) for u, w in ((0, 0), (1, 0), (1, 1), (0, 1))]
            out.append((a, s, cyc))
    return out


def _edge(c0, c1):
    return next(e for e, (a, b) in enumerate(EDGE_CORNERS) if {a, b} == {c0, c1})


def _triangles(table, case):
    row = table[case]
    n = int((row >= 0).sum())
    assert n % 3 == 0 and (row[:n] >= 0).all() and (row[n:] == -1).all()
    return row[:n].reshape(-1, 3).astype(int)


def test_case_table_uses_exactly_the_sign_change_edges(table):
    assert table.shape == (256, 16) and table.dtype == np.int8
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        crossing = {e for e, (a, b) in enumerate(EDGE_CORNERS) if inside[a] != inside[b]}
        tris = _triangles(table, case)
        assert set(tris.reshape(-1).tolist()) == crossing, case
        assert all(len(set(t)) == 3 for t in tris.tolist()), case
    assert _triangles(table, 0).size == 0 and _triangles(table, 255).size == 0


def test_case_table_face_boundaries_follow_the_separation_rule(table):
    """The triangles' boundary (edges used once) on every face is the segment set the face rule prescribes: the crossing edges of the
    face joined pairwise, and on an ambiguous face (inside corners diagonal) each inside corner cut off on its own."""
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        tris = _triangles(table, case)
        seg_count = {}
        for t in tris.tolist():
            for u, w in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                key = (min(u, w), max(u, w))
                seg_count[key] = seg_count.get(key, 0) + 1
        boundary = {k for k, n in seg_count.items() if n == 1}
        assert all(n in (1, 2) for n in seg_count.values()), case
        expected = set()
        for a, s, cyc in _faces():
            fe = [(cyc[i], cyc[(i + 1) % 4]) for i in range(4)]
            cross = [i for i in range(4) if inside[fe[i][0]] != inside[fe[i][1]]]
            if len(cross) == 2:
                e1, e2 = _edge(*fe[cross[0]]), _edge(*fe[cross[1]])
                expected.add((min(e1, e2), max(e1, e2)))
            elif len(cross) == 4:
                for i in range(4):
                    if inside[cyc[i]]:
                        e1, e2 = _edge(*fe[(i - 1) % 4]), _edge(*fe[i])
                        expected.add((min(e1, e2), max(e1, e2)))
        assert boundary == expected, (case, sorted(boundary), sorted(expected))


def test_case_table_triangles_face_the_outside_corners(table):
    """Taken at the edge midpoints, every triangle's normal has a positive component along its corners' inside -> outside edge
    directions (summed over the three corners): normals point toward lower values, as scikit-image's 'descent' gradient does."""
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        for t in _triangles(table, case).tolist():
            p = MID[t]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            s = 0.0
            for e in t:
                a, b = EDGE_CORNERS[e]
                d = CORNERS[b] - CORNERS[a]
                s += -n @ d if inside[b] else n @ d
            assert s > 0, (case, t)


# ------------------------------------------------------------------------------------------------ accumulation restatement
def _setup(nx=7, ny=6, nz=5):
    mcb = np.array([[-3.0, 4.0], [-2.0, 3.0], [-1.5, 1.0]])
    shift = np.array([0.5, -0.25, 0.125], dtype=np.float32)
    scale = np.float32(5.3)
    bound = torch.from_numpy((mcb + np.expand_dims(shift, 1)) / scale)
    b = bound.numpy()
    axes = [np.linspace(b[i][0], b[i][1], n) for i, n in enumerate((nx, ny, nz))]
    return bound, axes


def _samples(bound, axes, n_rays=40, S=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    lo = bound[:, 0].float() - 0.05
    hi = bound[:, 1].float() + 0.05
    pts = lo + (hi - lo) * torch.rand(n_rays, S, 3, generator=g)
    special = []
    for i in range(3):
        f32_lo, f32_hi = np.float32(bound[i][0]), np.float32(bound[i][1])
        special += [(i, float(f32_lo)), (i, float(f32_hi)), (i, float(np.float32(axes[i][2]))), (i, float(np.float32(axes[i][3])))]
        # between bound[i][1] and its fp32 rounding (when they differ): passes the fp32 check, bucket n in fp64 -> next row
        up = np.nextafter(f32_hi, np.float32(np.inf)) if float(f32_hi) < float(bound[i][1]) else f32_hi
        special.append((i, float(up)))
        special.append((i, float(np.nextafter(np.float32(axes[i][1]), np.float32(-np.inf)))))
    for r, (i, val) in enumerate(special):
        pts[r, :, i] = val
    w = torch.rand(n_rays, S, generator=g)
    w[w < 0.3] = 0
    depths = torch.rand(n_rays, generator=g) * 60
    var = torch.rand(n_rays, generator=g)
    return pts, w, depths, var


def test_restatement_equals_the_reference_sequence_without_duplicates():
    bound, axes = _setup()
    n = len(axes[0]) * len(axes[1]) * len(axes[2])
    pts, w, depths, var = _samples(bound, axes)
    # one sample per ray, rays whose buckets are all distinct (incl. the specials, placed on rows 0..)
    flat = pts[:, :1, :].contiguous()
    wf = w[:, :1].contiguous()
    for vt in (None, 0.5):
        seen, keep = set(), []
        for r in range(flat.shape[0]):
            idx, _ = MR._filtered(flat[r:r + 1], wf[r:r + 1], torch.zeros(1), torch.zeros(1), bound, axes, [0.0, 50.0], None, n)
            key = None if idx is None or idx.numel() == 0 else int(idx[0])
            if key is None or key not in seen:
                keep.append(r)
                if key is not None:
                    seen.add(key)
        keep = torch.tensor(keep)
        a = MR.reference_accumulate(torch.zeros(n, dtype=torch.float64), flat[keep], wf[keep], depths[keep], var[keep], bound, axes,
                                    torch.tensor([1.0, 50.0]), vt)
        b = MR.restated_accumulate(torch.zeros(n, dtype=torch.float64), flat[keep], wf[keep], depths[keep], var[keep], bound, axes,
                                   torch.tensor([1.0, 50.0]), vt)
        assert torch.equal(a, b) and float(a.sum()) > 0


def test_the_dtype_rules_the_kernel_restates():
    """The facts the HIP kernel is built on, pinned here: the bound check compares fp32 points in fp32, bucketize compares them in
    fp64, and a point above the fp64 top of an axis that passes the fp32 check takes bucket n (aliasing into the next row)."""
    x = torch.tensor([0.7], dtype=torch.float32)
    assert bool(x >= torch.tensor(0.7, dtype=torch.float64)) and not bool(x.double() >= 0.7)
    bound, axes = _setup()
    for i in range(3):
        b = torch.from_numpy(axes[i])
        pts = torch.from_numpy(np.array([np.float32(axes[i][2]), np.nextafter(np.float32(axes[i][1]), np.float32(-1e9)),
                                         np.float32(axes[i][-1])], dtype=np.float32))
        assert torch.equal(torch.bucketize(pts, b), torch.bucketize(pts.double(), b))
        ref = np.array([np.searchsorted(axes[i], float(p), side="left") for p in pts.numpy()])
        assert (torch.bucketize(pts, b).numpy() == ref).all()
    # a value in (bound_hi, fp32(bound_hi)] passes the check yet lands one past the last node
    for i in range(3):
        hi32 = np.float32(bound[i][1])
        if float(hi32) > float(bound[i][1]):
            p = torch.tensor([float(hi32)], dtype=torch.float32)
            assert bool(p <= bound[i][1]) and int(torch.bucketize(p, torch.from_numpy(axes[i]))) == len(axes[i])
            return
    pytest.fail("no axis of the fixture rounds its upper bound up in fp32")


def test_literal_sequence_is_last_writer_wins_on_duplicates():
    """Why the restatement replaces the assignment: two samples in one voxel, the larger first."""
    bound, axes = _setup()
    n = len(axes[0]) * len(axes[1]) * len(axes[2])
    c = torch.tensor([float(np.float32((axes[0][2] + axes[0][3]) / 2)), float(np.float32((axes[1][2] + axes[1][3]) / 2)),
                      float(np.float32((axes[2][2] + axes[2][3]) / 2))])
    pts = c.expand(1, 2, 3).contiguous()
    w = torch.tensor([[0.9, 0.2]])
    args = (pts, w, torch.tensor([1.0]), torch.tensor([0.0]), bound, axes, torch.tensor([1.0, 50.0]))
    a = MR.reference_accumulate(torch.zeros(n, dtype=torch.float64), *args)
    b = MR.restated_accumulate(torch.zeros(n, dtype=torch.float64), *args)
    assert float(a.max()) == pytest.approx(0.2) and float(b.max()) == pytest.approx(0.9)


# ------------------------------------------------------------------------------------------------ numpy marching cubes
def _grid(n):
    ax = np.arange(n, dtype=np.float64)
    return np.meshgrid(ax, ax, ax, indexing="ij")


def test_sphere_is_closed_oriented_with_euler_characteristic_two(table):
    x, y, z = _grid(24)
    vol = (9.3 ** 2 - ((x - 11.4) ** 2 + (y - 12.1) ** 2 + (z - 11.7) ** 2)).astype(np.float32)
    verts, faces = MR.marching_cubes(vol, 0.0, table)
    assert faces.shape[0] > 500
    closed, oriented = MR.closed_and_oriented(faces, len(verts))
    assert closed and oriented and MR.euler_characteristic(faces) == 2 and MR.vertex_links_are_single_cycles(faces)
    # normals point toward lower values: outward on a field that is positive inside the sphere
    p = verts[faces.astype(np.int64)].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    out = p.mean(1) - np.array([11.4, 12.1, 11.7])
    assert ((n * out).sum(1) > 0).mean() > 0.99


def test_torus_has_euler_characteristic_zero(table):
    x, y, z = _grid(32)
    R, r = 9.0, 3.7
    q = np.sqrt((x - 15.6) ** 2 + (y - 15.3) ** 2) - R
    vol = (r ** 2 - (q ** 2 + (z - 15.8) ** 2)).astype(np.float32)
    verts, faces = MR.marching_cubes(vol, 0.0, table)
    closed, oriented = MR.closed_and_oriented(faces, len(verts))
    assert closed and oriented and MR.euler_characteristic(faces) == 0 and MR.vertex_links_are_single_cycles(faces)


def test_noise_volume_gives_a_closed_manifold(table):
    """Random values: ambiguous faces everywhere.  Surrounded by an outside layer the surface must be closed, every edge used once in
    each direction, no vertex left without a triangle, and the triangles around every vertex one closed fan."""
    rng = np.random.default_rng(3)
    vol = np.full((21, 19, 17), -1.0, dtype=np.float32)
    vol[1:-1, 1:-1, 1:-1] = rng.standard_normal((19, 17, 15)).astype(np.float32)
    verts, faces = MR.marching_cubes(vol, 0.0, table)
    closed, oriented = MR.closed_and_oriented(faces, len(verts))
    assert closed and oriented
    assert np.unique(faces).size == len(verts)
    assert MR.vertex_links_are_single_cycles(faces)


def test_linear_field_puts_vertices_on_its_plane(table):
    x, y, z = _grid(12)
    vol = (x - 5.5).astype(np.float32)                          # level 0: the plane x = 5.5, half way along every crossing edge
    verts, faces = MR.marching_cubes(vol, 0.0, table, spacing=(0.5, 2.0, 1.0), origin=(1.0, -3.0, 0.25))
    assert verts.shape[0] == 12 * 12 and (verts[:, 0] == np.float32(5.5 * 0.5 + 1.0)).all()
    vol2 = (0.25 * x + 0.5 * y - 0.75 * z - 1.0).astype(np.float32)
    verts2, faces2 = MR.marching_cubes(vol2, 0.0, table)
    res = 0.25 * verts2[:, 0] + 0.5 * verts2[:, 1] - 0.75 * verts2[:, 2] - 1.0
    assert np.abs(res).max() < 1e-5 and faces2.shape[0] > 0
