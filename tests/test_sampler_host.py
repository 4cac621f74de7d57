"""The sampler cases of tests/sampler_restatement.py are what they claim - no GPU.  tests/test_gpu_sampler.py compares the kernels with
the oracle on these cases; here the cases themselves are taken apart, so that the comparison cannot pass vacuously: which rays hold
inversions and so leave the merge route, that the planted draws land on the searchsorted tie rule and the `above` clamp, that the
saturated grid saturates, that the oracle's sum / cumsum equal torch's at every row length used, and that the restated sort network
sorts on every route - and does NOT sort a reversed coarse half on the merge route, which is what the kernel's fallback is for."""
import numpy as np
import pytest
import torch

from oracle import sampling as SP
from oracle.torch_rounding import cumsum_lastdim_f32, sum_lastdim_f32
from tests import sampler_restatement as R

f32 = np.float32


def test_the_table_covers_every_route_and_form():
    """every (route, forms) combination the kernel has is taken by some ray of the table"""
    seen = set()
    for name in R.CASE_NAMES:
        seen.update(R.case_routes(name))
    assert seen == {("full", ("plain",)), ("full", ("wave_local",)), ("merge", ("plain", "plain")), ("merge", ("plain", "wave_local")),
                    ("merge", ("wave_local", "wave_local"))}
    assert R.sort_route(128, False) == ("merge", ("plain", "plain")) and R.sort_route(64, False) == ("full", ("plain",))
    assert R.sort_route(256, False) == ("merge", ("plain", "wave_local")) and R.sort_route(256, True) == ("full", ("wave_local",))
    assert R.sort_route(130, False) == ("full", ("wave_local",)) and R.sort_route(126, False) == ("full", ("plain",))
    sizes = sorted({c["S"] for c in R.CASES.values()})
    assert {8, 10, 12, 14, 16, 18, 20, 22, 36, 38, 100, 126, 128, 256, 1024, 4096, 8192, 130, 200, 258, 300, 1000, 3000, 8190, 512, 2048} == set(sizes)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_takes_the_routes_it_is_meant_to(name):
    c = R.CASES[name]
    rays, grid, S, perturb, u_jitter, u_pdf = R.build_case(name)
    assert all(a.dtype == f32 for a in (rays, grid, u_jitter, u_pdf)) and rays.shape == (c["n"], 13)
    assert u_jitter.shape == u_pdf.shape == (c["n"], S // 2) and np.isfinite(rays).all()
    assert (u_jitter == 0).all(axis=0).any() and (u_jitter == R.U_MAX).all(axis=0).any() and float(u_jitter.max()) < 1.0
    _, st = R.oracle_case(name)
    inv, ties = R.coarse_inversions(st["coarse"])
    routes = R.case_routes(name)
    edited = R.edited_rows(name)
    n_full, n_merge = sum(r[0] == "full" for r in routes), sum(r[0] == "merge" for r in routes)
    print(f"{name:18s} [{c['cls']}] S={S} perturb={perturb}: {n_merge} rays merge, {n_full} rays full sort {sorted(set(routes))}; "
          f"inversions per ray {inv.tolist()}, ties {ties.tolist()}")
    assert (inv[~edited] == 0).all()                                   # ordinary spans tie at the most
    if c["edit"] is None:
        want = R.sort_route(S, False)
        assert all(r == want for r in routes)
        return
    assert edited[1::2].all() and not edited[0::2].any()              # interleaved: neighbouring workgroups differ
    if c["edit"] == "reversed":
        # every pair of a reversed span inverts, but for the pair whose jitters 1 - 2^-24 and 0 were planted to meet: a tie
        assert (rays[edited, 12] == 0).all() and (inv[edited] + ties[edited] == S // 2 - 1).all() and (inv[edited] >= S // 2 - 3).all()
        assert all(routes[i][0] == "full" for i in np.nonzero(edited)[0])
    elif c["edit"] == "empty":
        assert (rays[edited, 12] == rays[edited, 11]).all()
    else:
        span = (rays[edited, 12] - rays[edited, 11]).astype(np.float64)
        assert perturb == 0.0 and (span > 0.9e-5).all() and (span < 3.1e-5).all()
    assert n_full >= 3 and n_merge >= 3
    assert all(r == R.sort_route(S, True) for r in routes if r[0] == "full") and R.sort_route(S, True)[1] == ("wave_local",)


def test_an_empty_span_at_the_fixture_near_holds_no_inversion():
    """why the `empty` builder searches for its near values: near = far = 0.01166026 (the fixture's own near) gives a row without an
    inversion at perturb = 1, whatever the jitter - an empty span is not on the full route by itself"""
    near = R._g4()["rays"][:1, 11]
    assert abs(float(near[0]) - 0.01166026) < 1e-8
    for H in (128, 256, 1024):
        for seed in range(8):
            u = np.random.default_rng(seed).random((1, H), dtype=f32)
            assert R.coarse_inversions(SP.stratified_depths(near, near, H, 1.0, u))[0][0] == 0


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_planted_draws_hit_the_tie_rule_and_the_clamp(name):
    rays, grid, S, perturb, u_jitter, u_pdf = R.build_case(name)
    _, st = R.oracle_case(name)
    K = S // 2 - 2
    cols, last = R.planted_columns(S)
    assert len(cols) == min(20, K) and st["cdf"].shape == (len(rays), K + 1)
    assert np.array_equal(u_pdf[:, cols], st["cdf"][:, cols + 1]) and np.array_equal(u_pdf[:, last], st["cdf"][:, K])
    assert (st["inds"][:, cols] == cols[None, :] + 2).all()           # u == cdf[k] -> ind = k + 1, here k = column + 1
    assert (st["inds"][:, last] == K + 1).all()                       # u >= cdf[K]: past the last bin
    assert (np.diff(st["cdf"][:, :len(cols) + 2].astype(np.float64), axis=1) > 0).all()


def test_some_ray_ends_its_cdf_below_one():
    """cdf[K] < 1 on some ray: then a draw in [cdf[K], 1) is an ordinary draw, and ind = K + 1 an ordinary result"""
    short = {name: int((R.oracle_case(name)[1]["cdf"][:, -1] < 1).sum()) for name in R.CASE_NAMES}
    print("rays with cdf[K] < 1 per case:", {k: v for k, v in short.items() if v})
    assert sum(short.values()) >= 1


def test_the_saturated_grid_saturates_within_the_exactness_precondition():
    rays, grid, S, perturb, u_jitter, u_pdf = R.build_case("s8192_saturated")
    _, st = R.oracle_case("s8192_saturated")
    assert S == 8192 and grid.shape == (16, 16, 16)
    probs = st["probs"]
    assert (probs == 0).any(axis=1).all() and (probs == 1).any(axis=1).all()       # exp overflowed to inf / vanished beside 1, on every ray
    assert ((probs > 0) & (probs < 1)).any()                                          # and the slab's faces lie between
    K = S // 2 - 2
    w = probs[:, 1:-1] + f32(1e-5)
    pdf = w / sum_lastdim_f32(w)[:, None]
    print(f"saturated, S = 8192: min pdf {float(pdf.min()):.4e}; 1e-5 / K = {1e-5 / K:.4e}; 2^-29 = {2.0 ** -29:.4e}")
    assert float(pdf.min()) > 2.0 ** -29                    # lnr_sampler.hip: "every pdf value ... > 2^-29 for K <= 4094"
    assert float(pdf.min()) < 2.0 * 1e-5 / K                # and close to the smallest a row of this length can hold
    # the float64 running sum of such a row is exact: any order of the additions gives the oracle's cdf
    assert np.array_equal(np.cumsum(pdf.astype(np.float64), axis=1).astype(f32), st["cdf"][:, 1:])
    assert np.array_equal(np.cumsum(pdf[:, ::-1].astype(np.float64), axis=1)[:, -1].astype(f32), st["cdf"][:, -1])


def test_oracle_sum_and_cumsum_equal_torch_at_every_row_length_of_the_table():
    ks = sorted({c["S"] // 2 - 2 for c in R.CASES.values()})
    assert ks[0] == 2 and ks[-1] == 4094
    rng = np.random.default_rng(9)
    for K in ks:
        x = (rng.random((6, K), dtype=f32) + f32(1e-5)).astype(f32)
        x[1] = f32(1e-5)                                                            # an all-free ray
        x[2, ::3] = f32(1.0) + f32(1e-5)                                            # saturated bins
        t = torch.from_numpy(x)
        assert np.array_equal(sum_lastdim_f32(x), torch.sum(t, -1).numpy()), K
        pdf = x / sum_lastdim_f32(x)[:, None]
        assert np.array_equal(cumsum_lastdim_f32(pdf), torch.cumsum(torch.from_numpy(pdf), -1).numpy()), K


def _sort_inputs(S, seed):
    H = S // 2
    rng = np.random.default_rng(seed)
    coarse = np.sort(rng.random(H, dtype=f32))
    coarse[H // 3] = coarse[H // 3 + 1]                                             # a tie
    fine = rng.random(H, dtype=f32)
    fine[:3] = coarse[:3]                                                           # importance samples equal to coarse ones
    return coarse, fine


@pytest.mark.parametrize("S", sorted({c["S"] for c in R.CASES.values()}))
def test_restated_network_sorts_on_every_route(S):
    """bitonic() - the kernel's exchange arithmetic and loop forms - returns np.sort on the full route for an ascending and for a
    reversed coarse half (+inf padding up to P2), and on the merge route for an ascending one.  Forced onto the merge route, a reversed
    coarse half does NOT come out sorted: the per-ray fallback is needed, not decorative."""
    coarse, fine = _sort_inputs(S, S)
    asc, rev = np.concatenate([coarse, fine]), np.concatenate([coarse[::-1], fine])
    assert np.array_equal(R.sort_as_kernel(asc, S, "full"), np.sort(asc))
    assert np.array_equal(R.sort_as_kernel(rev, S, "full"), np.sort(rev))
    if R.sort_route(S, False)[0] == "merge":
        assert np.array_equal(R.sort_as_kernel(asc, S, "merge"), np.sort(asc))
        assert not np.array_equal(R.sort_as_kernel(rev, S, "merge"), np.sort(rev))
    # the descending half on its own (H elements, the form sort_route names)
    H = S // 2
    if H & (H - 1) == 0:
        assert np.array_equal(R.bitonic(fine, H, True), np.sort(fine)[::-1])


@pytest.mark.parametrize("name", [n for n in R.CASE_NAMES if R.CASES[n]["edit"] is not None])
def test_restated_network_on_the_mixed_cases_themselves(name):
    """on the oracle's own [coarse | importance] rows of every mixed case: each ray sorted on the route sort_route gives it equals the
    oracle's z; every reversed ray forced onto the merge route differs, and so do the printed number of the empty and narrow ones
    (a few inversions between neighbours can still come out of the merge in order)"""
    z, st = R.oracle_case(name)
    S = R.CASES[name]["S"]
    n_full = wrong = 0
    for i, (route, _) in enumerate(R.case_routes(name)):
        merged = np.concatenate([st["coarse"][i], st["fine"][i]])
        assert np.array_equal(R.sort_as_kernel(merged, S, route), z[i]), (name, i, route)
        if route == "full":
            n_full += 1
            wrong += not np.array_equal(R.sort_as_kernel(merged, S, "merge"), z[i])
    print(f"{name}: {wrong} of the {n_full} inverted rays come out of the merge route unsorted")
    if R.CASES[name]["edit"] == "reversed":
        assert wrong == n_full


def test_lookup_points_cover_the_padding_cases():
    for V in (1, 2, 24):
        pts = R.lookup_points(V)
        count = R.inside_corners(V, pts)
        # (a volume of one voxel has one corner inside per axis at the most)
        assert set(count.tolist()) == ({0, 1} if V == 1 else {0, 1, 2, 4, 8}), (V, sorted(set(count.tolist())))
        ix = ((pts[:, 0] + f32(1)) * f32(V) - f32(1)) / f32(2)
        assert (ix == np.floor(ix)).any() and (np.abs(pts) == 1).all(axis=1).any()


def test_exact_lidar_case_is_exact_and_sits_on_the_threshold():
    """every rotated direction is an integer vector with an integer norm, near + 1/scale == far_range bit for bit, and the oracle keeps
    no range-limited ray at (1, 2) but every one of them at (1, nextafter(2, 3))"""
    from oracle import rays as OR
    c = R.exact_lidar_case()
    scale = f32(c["scale"])
    assert f32(1.0) / scale + f32(1.0) / scale == f32(2.0) / scale
    norms = np.sqrt((c["dirs"].astype(np.float64) ** 2).sum(axis=0))
    assert (norms == np.round(norms)).all() and (c["dirs"] == 0).any(axis=0).sum() >= 8
    idx = torch.arange(c["dirs"].shape[1])
    kept = {}
    for key in ("range_equal", "range_above"):
        kept[key] = []
        for T in c["poses"]:
            assert sorted(np.abs(T[:3, :3]).sum(axis=0).tolist()) == [1, 1, 1] and np.isclose(np.linalg.det(T[:3, :3].astype(np.float64)), 1.0)
            rays, _, keep = OR.lidar_ray_records(torch.from_numpy(c["dirs"]), torch.from_numpy(c["dist"]), idx, torch.from_numpy(T),
                                                 torch.tensor(c[key], dtype=torch.float32), torch.tensor(c["scale"]), torch.from_numpy(c["shift"]),
                                                 keep_all=True)
            far, near = rays[:, 12].numpy(), rays[:, 11].numpy()
            k = far > near + f32(1.0) / scale
            kept[key].append(k)
            outside = abs(float(T[0, 3])) > 64.0
            if outside:
                away = rays[:, 3].numpy() >= 0
                assert away.any() and (far[away] == 0).all() and not k[away].any()
            elif key == "range_equal":
                assert (far == near + f32(1.0) / scale).all() and not k.any()      # inside, every ray range-limited: exactly ON the threshold
            else:
                assert k.all()
    print("kept per pose at (1, 2):", [int(k.sum()) for k in kept["range_equal"]], " at (1, nextafter(2, 3)):", [int(k.sum()) for k in kept["range_above"]])
