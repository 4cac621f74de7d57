"""The ray samplers' test cases and the route each one is meant to take through loner_amd/csrc/lnr_sampler.hip - numpy / torch on the
CPU only.  tests/test_sampler_host.py proves that every case is what it claims (inversions, ties, planted draws, saturation, the
sort network's index arithmetic); tests/test_gpu_sampler.py runs the same cases through the kernels, bit for bit against
oracle/sampling.py.

A case is (rays [n,13], grid [V,V,V], S, perturb, u_jitter [n,S/2], u_pdf [n,S/2]), all float32; seeds are fixed and nothing is drawn
at import time.  The rays are those of the G4 fixture (one origin inside the cube, near 0.0117, far 0.583), edited where a case says so:
  reversed   far = 0                               (a camera ray from outside the cube that points away: cube_exit returns 0)
  empty      far = near                            (near (1 - s) + far s is not constant in float32)
  narrow     far = near + 2e-5 * (0.5 .. 1.5)      (with perturb = 0: the same rounding with no jitter on top)
Edited rays take the ODD rows, unedited ones the even rows: neighbouring workgroups of one launch take different sort routes.
"""
import functools
import os

import numpy as np

from oracle import sampling as SP

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U_MAX = f32(1.0) - f32(2.0 ** -24)          # the largest draw of a 24-bit uniform generator
N_PLANTED = 20
RAY_STRIDE = 13


# ------------------------------------------------------------------------------------------------ the sort routes
def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def sort_form(n_pow2):
    """bitonic_sort_lds, lnr_sampler.hip:148 (`if (n_pow2 < 256)`): the plain network below 256 elements, above it the form in which
    each wave owns a quarter of the array"""
    return "plain" if n_pow2 < 256 else "wave_local"


def sort_route(S, has_inversion):
    """-> (route, forms): the route of sample_occ_kernel's final sort for a ray of S samples, and the form of every bitonic_sort_lds
    call on it, in call order.

    lnr_sampler.hip:282 `if (__syncthreads_or(unsorted ? 1 : 0) == 0 && P2 == S && H >= 64)`: "merge" - the importance half
    (H = S/2 elements) is sorted descending, then the last stage of the P2 network merges the halves: forms (form(H), form(P2)) -
    when S is a power of two, H >= 64 and the ray's coarse depths hold no inversion; otherwise "full": one ascending sort of P2
    elements, forms (form(P2),).  lnr_sampler.hip:148 `if (n_pow2 < 256)` picks the form of each call (sort_form)."""
    P2, H = next_pow2(S), S // 2
    if not has_inversion and P2 == S and H >= 64:
        return "merge", (sort_form(H), sort_form(P2))
    return "full", (sort_form(P2),)


def bitonic(a, n, descending=False, k_first=2):
    """bitonic_sort_lds(a, n, descending, k_first) of lnr_sampler.hip, restated pass by pass with the kernel's own `exchange` index
    arithmetic and its two loop forms; -> the first n elements after the network, as a new array.  The pairs of one pass are disjoint,
    so a pass is evaluated at once; in the wave-local form the pairs of a pass that runs without a workgroup barrier are asserted to
    stay inside the quarter of the wave that handles them (what makes the missing barrier legal)."""
    a = np.array(a[:n], dtype=f32, copy=True)
    assert n >= 2 and n & (n - 1) == 0

    def exchange(t, j, k):
        i = ((t & ~(j - 1)) << 1) | (t & (j - 1))
        p = i | j
        up = ((i & k) == 0) != descending
        x, y = a[i], a[p]
        swap = (x > y) == up
        a[i], a[p] = np.where(swap, y, x), np.where(swap, x, y)
        return i, p

    k = k_first
    while k <= n:
        j = k >> 1
        while j > 0:
            if sort_form(n) == "wave_local" and 8 * j <= n:
                quarter_pairs = n // 8
                for wave in range(4):
                    t = np.concatenate([np.arange(wave * quarter_pairs + lane, (wave + 1) * quarter_pairs, 64) for lane in range(64)])
                    i, p = exchange(t, j, k)
                    lo, hi = wave * (n // 4), (wave + 1) * (n // 4)
                    assert i.min() >= lo and p.max() < hi and len(np.unique(np.concatenate([i, p]))) == n // 4
            else:
                t = np.concatenate([np.arange(thread, n // 2, 256) for thread in range(min(256, n // 2))])
                i, p = exchange(t, j, k)
                assert len(np.unique(np.concatenate([i, p]))) == n
            j >>= 1
        k <<= 1
    return a


def sort_as_kernel(merged, S, route):
    """The kernel's final sort of `merged` = [coarse (H) | importance (H)] on the given route -> the S sorted depths"""
    P2, H = next_pow2(S), S // 2
    buf = np.full(P2, np.inf, f32)
    buf[:S] = merged
    if route == "merge":
        assert P2 == S and H >= 64
        buf[H:] = bitonic(buf[H:], H, True)
        return bitonic(buf, P2, False, P2)[:S]
    return bitonic(buf, P2)[:S]


def coarse_inversions(z):
    """coarse depths [n,H] -> (inversions [n], ties [n]) between neighbours: `unsorted |= zc[j] > zc[j + 1]` of the kernel"""
    z = np.asarray(z, f32)
    return (z[:, :-1] > z[:, 1:]).sum(axis=1), (z[:, :-1] == z[:, 1:]).sum(axis=1)


# ------------------------------------------------------------------------------------------------ the case table
def _case(S, n, perturb=1.0, edit=None, grid="trained", cls=""):
    return dict(S=S, n=n, perturb=perturb, edit=edit, grid=grid, cls=cls)


def _table():
    t = {}
    for S in (8, 10, 12, 14, 16, 18):
        t[f"s{S}"] = _case(S, 8, cls="plain full sort, row sum V = 1")
    for S in (20, 22, 36, 38, 100, 126):
        t[f"s{S}"] = _case(S, 8, cls="plain full sort, K >= 8")
    t["s128"] = _case(128, 8, cls="merge, both sorts plain")
    t["s128_zero_grid"] = _case(128, 8, grid="zero", cls="merge, both sorts plain")
    t["s256"] = _case(256, 8, cls="merge, plain half + wave-local merge")
    t["s512"] = _case(512, 8, cls="merge, wave-local")
    t["s1024"] = _case(1024, 8, cls="merge, wave-local")
    t["s4096"] = _case(4096, 4, cls="merge, wave-local")
    t["s8192"] = _case(8192, 3, cls="merge, wave-local")
    t["s8192_saturated"] = _case(8192, 3, grid="saturated", cls="merge, wave-local")
    for S, n in ((130, 8), (200, 8), (258, 8), (300, 8), (1000, 8), (3000, 4), (8190, 3)):
        t[f"s{S}"] = _case(S, n, cls="full wave-local sort, S no power of two")
    for S, n in ((256, 12), (512, 12), (2048, 8)):
        t[f"s{S}_reversed"] = _case(S, n, edit="reversed", cls="mixed launch: full wave-local sort by inversion + merge")
        t[f"s{S}_empty"] = _case(S, n, edit="empty", cls="mixed launch: full wave-local sort by inversion + merge")
        t[f"s{S}_narrow"] = _case(S, n, perturb=0.0, edit="narrow", cls="mixed launch: full wave-local sort by inversion + merge")
    for S in (20, 512, 1000):                       # perturb changes the arithmetic (and, on narrow spans, the route): not a full product
        for p, tag in ((0.0, "p0"), (0.5, "p05")):
            t[f"s{S}_{tag}"] = _case(S, 8, perturb=p, cls="perturb 0 / 0.5")
    return t


CASES = _table()
CASE_NAMES = tuple(CASES)
UNIFORM_SIZES = (2, 3, 64, 257, 8192)
PERTURBS = (0.0, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def _g4():
    return dict(np.load(os.path.join(GOLDEN, "g4_samplers.npz"), allow_pickle=False))


def _seed(name):
    return 1000 + CASE_NAMES.index(name)


def saturated_grid():
    """V = 16 logits: +100 everywhere (exp(-100) vanishes beside 1: p = 1 exactly) except a slab two voxels thick across x of -100
    (exp(100) overflows float32 to inf: p = 0 exactly); the slab's faces interpolate between the two"""
    grid = np.full((16, 16, 16), 100.0, f32)
    grid[:, :, 9:11] = -100.0
    return grid


def edited_rows(name):
    """-> bool [n]: the rows of the case whose span is edited (the odd ones of a mixed case)"""
    c = CASES[name]
    rows = np.zeros(c["n"], bool)
    if c["edit"] is not None:
        rows[1::2] = True
    return rows


def _jitter(rng, n, H):
    u = rng.random((n, H), dtype=f32)
    u[:, 1 % H] = U_MAX                                # the largest draw next to the smallest: ties on ordinary spans, never inversions
    u[:, 2 % H] = 0.0
    if H >= 8:
        u[:, 5], u[:, 6] = 0.0, U_MAX
    return u


def _edit_spans(rays, rows, kind, H, perturb, u_jitter, rng):
    """`empty` and `narrow` invert on most / some values of near only: near is drawn (seeded) until the row's coarse depths hold an
    inversion, 2000 draws at the most; test_sampler_host.py asserts what came of it.  A narrow span inverts where a step of the span,
    2e-5 / H, comes near the spacing of float32 at `near`: at H = 128 that takes near > 0.5 (about 3 draws in 100 invert), so near is
    drawn from the whole (0.02, 1.9) - the cube's diagonal is 3.46 long."""
    for i in np.nonzero(rows)[0]:
        if kind == "reversed":
            rays[i, 12] = 0.0
            continue
        for _ in range(2000):
            near = f32(rng.uniform(0.02, 0.5 if kind == "empty" else 1.9))
            far = near if kind == "empty" else f32(near + f32(2e-5 * rng.uniform(0.5, 1.5)))
            z = SP.stratified_depths(np.array([near]), np.array([far]), H, perturb, u_jitter[i:i + 1])
            if coarse_inversions(z)[0][0] > 0:
                break
        rays[i, 11], rays[i, 12] = near, far


@functools.lru_cache(maxsize=None)
def build_case(name):
    """-> (rays, grid, S, perturb, u_jitter, u_pdf).  u_jitter holds columns of exact 0 and of 1 - 2^-24.  u_pdf is uniform except
    for the planted columns (planted_columns): after one oracle pass u_pdf[:, c] = cdf[:, c + 1] for c < min(20, K) - a draw exactly
    on cdf entry k must give ind = k + 1, the tie rule of searchsorted(right=True) - and one more column = cdf[:, K], which gives
    ind = K + 1: the `above` clamp and the `denom < 1e-5` branch."""
    c = CASES[name]
    g = _g4()
    S, n, perturb = c["S"], c["n"], float(c["perturb"])
    H, K = S // 2, S // 2 - 2
    rng = np.random.default_rng(_seed(name))
    if c["grid"] == "saturated":
        grid = saturated_grid()
        pool = g["rays"][g["rays"][:, 3] > 0.5]        # rays that cross the slab
    else:
        grid = g["trained_grid"] if c["grid"] == "trained" else g["zero_grid"]
        pool = g["rays"]
    rays = np.array(pool[rng.permutation(len(pool))[:n]], f32)
    assert rays.shape == (n, RAY_STRIDE)
    u_jitter = _jitter(rng, n, H)
    if c["edit"] is not None:
        _edit_spans(rays, edited_rows(name), c["edit"], H, perturb, u_jitter, rng)
    u_pdf = rng.random((n, H), dtype=f32)
    with np.errstate(over="ignore"):                   # (the saturated grid: exp overflows float32 on purpose)
        _, st = SP.sample_occupancy(rays, grid, S, perturb, u_jitter, u_pdf, return_stages=True)
    cols, last = planted_columns(S)
    u_pdf[:, cols] = st["cdf"][:, cols + 1]
    u_pdf[:, last] = st["cdf"][:, K]
    for a in (rays, grid, u_jitter, u_pdf):
        a.setflags(write=False)
    return rays, grid, S, perturb, u_jitter, u_pdf


def planted_columns(S):
    """-> (cols, last): u_pdf[:, cols] sit exactly on cdf[:, cols + 1], u_pdf[:, last] on cdf[:, K]"""
    K = S // 2 - 2
    m = min(N_PLANTED, K)
    return np.arange(m), m


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """-> (z [n,S], stages) of oracle.sampling.sample_occupancy on the case; computed once, shared, read-only"""
    rays, grid, S, perturb, u_jitter, u_pdf = build_case(name)
    with np.errstate(over="ignore"):
        z, st = SP.sample_occupancy(rays, grid, S, perturb, u_jitter, u_pdf, return_stages=True)
    z.setflags(write=False)
    for a in st.values():
        a.setflags(write=False)
    return z, st


def case_routes(name):
    """-> list of sort_route(S, inversion) per ray of the case, from the oracle's coarse depths"""
    S = CASES[name]["S"]
    inv, _ = coarse_inversions(oracle_case(name)[1]["coarse"])
    return [sort_route(S, bool(v)) for v in inv]


@functools.lru_cache(maxsize=None)
def uniform_case(S, perturb):
    """-> (rays [12,13], u_jitter [12,S]) for the uniform sampler: rows 1, 4, 7, 10 reversed, rows 2, 5, 8, 11 empty"""
    rng = np.random.default_rng(77 + S)
    rays = np.array(_g4()["rays"][:12], f32)
    rays[1::3, 12] = 0.0
    rays[2::3, 11] = rng.uniform(0.02, 0.5, 4).astype(f32)
    rays[2::3, 12] = rays[2::3, 11]
    u = _jitter(rng, 12, S)
    rays.setflags(write=False)
    u.setflags(write=False)
    return rays, u


# ------------------------------------------------------------------------------------------------ occupancy lookup points
def lookup_points(V):
    """Points for occ_interpolate on a [V,V,V] grid -> pts [m,3] float32: voxel centres (ix an integer: the weights of the upper
    corners vanish), the faces / edges / corners of the cube at exactly -1 and +1 on one, two and three axes, and points outside it by
    less than a voxel (one plane of corners of that axis remains) and by more (none remains) on one, two and three axes.
    inside_corners counts what remains of the 8 corners."""
    centre = lambda i: f32((2 * i + 1) / V - 1)                    # ix = i exactly
    inside = centre(V // 2)
    out_half = f32(-1.0 - 1.0 / (2 * V))                           # ix = -0.75: x0 = -1 outside, x1 = 0 inside
    out_far = f32(-1.0 - 4.0 / V)                                  # ix = -2.5: both outside
    pts = [(f32(-0.2), f32(0.1), f32(0.3))]                        # an ordinary point: all 8 corners inside when V >= 2
    for i in range(min(V, 3)):
        for k in range(min(V, 3)):
            pts.append((centre(i), centre(V - 1 - k), centre((i + k) % V)))
    for on in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)):
        for sign in (-1.0, 1.0):
            pts.append(tuple(f32(sign) if a else f32(0.3 * sign) for a in on))
    for n_out in (1, 2, 3):
        pts.append(tuple(out_half if a < n_out else inside for a in range(3)))
        pts.append(tuple(out_far if a < n_out else inside for a in range(3)))
    return np.array(pts, f32)


def inside_corners(V, pts):
    """The number of the 8 trilinear corners of each point that lie inside a [V,V,V] volume, counted from the point itself"""
    fV = f32(V)
    count = np.ones(len(pts), np.int64)
    for a in range(3):
        i0 = np.floor(((pts[:, a] + f32(1)) * fV - f32(1)) / f32(2))
        count = count * (((i0 >= 0) & (i0 < V)).astype(np.int64) + ((i0 + 1 >= 0) & (i0 + 1 < V)).astype(np.int64))
    return count


# ------------------------------------------------------------------------------------------------ exact lidar rays
def signed_permutations():
    """Six proper rotations with entries in {0, +1, -1}: R l has one non-zero product per row, so it is exact in any order, with or
    without fused multiply-adds"""
    mats = [[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]],
            [[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]]]
    return [np.array(m, f32) for m in mats]


def exact_lidar_case():
    """Poses and sensor-frame directions on which every sum of the ray builders is exact -> dict.  scale = 64 and ray_range = (1, 2)
    make far_range == near + 1/scale exactly (1/64 + 1/64 = 2/64): a ray limited by the range is DROPPED at (1, 2) and kept at
    (1, nextafter(2, 3)).  Directions are Pythagorean - (3, 4, 0) and (1, 2, 2) have norms 5 and 3, their squares sum exactly - with
    components exactly 0.  Origins: inside the cube (translation (8, -16, 24) / 64), and outside it at x = 1.5 (translation 96 / 64),
    from where the rays with a world direction of x >= 0 exit at 0: far == 0, dropped."""
    dirs = np.array([[3, 4, 0], [-3, 4, 0], [0, 3, 4], [4, 0, -3], [1, 2, 2], [-2, 1, 2], [2, -2, 1], [0, 0, 1], [0, -1, 0], [1, 0, 0],
                     [-1, 0, 0], [-4, -3, 0], [0, 0, -1], [2, 2, -1], [-1, -2, -2], [0, 4, 3]], f32).T.copy()       # [3,16]
    dist = (np.arange(16, dtype=f32) + f32(1)) * f32(4)
    poses = []
    for r, rot in enumerate(signed_permutations()):
        T = np.eye(4, dtype=f32)
        T[:3, :3] = rot
        T[:3, 3] = (96.0, 0.0, 0.0) if r % 2 else (8.0, -16.0, 24.0)
        poses.append(T)
    return dict(dirs=dirs, dist=dist, poses=poses, scale=64.0, shift=np.zeros(3, f32),
                range_equal=(1.0, 2.0), range_above=(1.0, float(np.nextafter(f32(2), f32(3)))))
