"""tests/mlp_restatement.py - the reference of tests/test_gpu_mlp_default.py - checked on the CPU: against oracle/network.py in float32
and float64, its lattice against a rational evaluation of the published algorithm, and the preconditions of every exact GPU case
recomputed from the builders the GPU test calls (an edit of an alphabet that breaks exactness fails here, not on the GPU)."""
from fractions import Fraction as Fr
from math import ceil

import pytest
import torch

from oracle import network as NW
from tests import encode_restatement as ER
from tests import known_answer as K
from tests import mlp_restatement as MR
from tests.test_gpu_kernels import NETS

F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -23
DEFAULT_CLASS = {64: "default", 32: "default_n32", 16: "default_n16"}
N_POINTS = 300


@pytest.fixture(scope="module")
def library():
    import __graft_entry__ as ge
    ge.build()


def _random_network(H):
    enc = NETS[DEFAULT_CLASS[H]][0]
    spec = NW.NetworkSpec.from_config(enc, dict(activation="ReLU", n_neurons=H, n_hidden_layers=1))
    params = NW.init_params(spec, seed=H)
    params[spec.n_mlp_params:] *= 3000.0
    gen = torch.Generator().manual_seed(H + 1)
    p = torch.rand(N_POINTS, 3, generator=gen) * 1.9 - 0.95
    d_sigma = torch.randn(N_POINTS, generator=gen)
    d_sigma[::10] = 0.0
    return enc, spec, params, p, d_sigma


# ------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("H", MR.WIDTHS)
def test_float32_restatement_agrees_with_the_oracle_to_rounding(H):
    """forward and autograd gradients to the float32 rounding of another summation order: at most 8 ulp of the entry's A"""
    enc, spec, params, p, d_sigma = _random_network(H)
    grid = ER.make_grid(enc)
    feat = torch.cat(ER.encode(grid, params[spec.n_mlp_params:], p, F32)["feat"], dim=1)
    W1, Wout = MR.unpack(params, H)
    ours = MR.backward(feat, W1, Wout[0], d_sigma)
    q = params.clone().requires_grad_(True)
    sigma = NW.density(spec, q, p)
    (sigma * d_sigma).sum().backward()
    gW1, gWout = MR.unpack(q.grad, H)
    assert not bool(gWout[1:].any())
    worst = {}
    for name, got, ref, A in (("sigma", ours["sigma"], sigma.detach(), ours["A_sigma"]), ("dW1", ours["dW1"], gW1, ours["A_dW1"]),
                              ("dWo", ours["dWo"], gWout[0], ours["A_dWo"])):
        assert bool((A > 0).all())
        worst[name] = float(((got.double() - ref.double()).abs() / (ULP * A)).max())
    print("FIGURES float32 restatement against the oracle, largest deviation in ulp of A:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 8.0, worst
    # d_feature: the float32 run against the float64 run (which the next test ties to the oracle's autograd)
    r64 = MR.backward(feat.double(), W1.double(), Wout[0].double(), d_sigma.double())
    live = ours["A_d_feature"] > 0
    assert float(((ours["d_feature"].double() - r64["d_feature"]).abs()[live] / (ULP * ours["A_d_feature"][live])).max()) <= 8.0
    assert not bool(ours["d_feature"][~live].any())


@pytest.mark.parametrize("H", MR.WIDTHS)
def test_float64_restatement_equals_the_oracles_autograd(H):
    """on the oracle's own float64 features: sigma, dW1, dWo, and d_feature through the oracle's encoding (the table gradient)"""
    enc, spec, params, p, d_sigma = _random_network(H)
    params, x, d_sigma = params.double(), (p.double() + 1) / 2, d_sigma.double()
    q = params.clone().requires_grad_(True)
    sigma = NW.density_unit(spec, q, x)
    (sigma * d_sigma).sum().backward()
    table = params[spec.n_mlp_params:].clone().requires_grad_(True)
    feat = NW.encode_hashgrid(spec, table.reshape(-1, spec.n_features), x)
    W1, Wout = MR.unpack(params, H)
    ours = MR.backward(feat.detach(), W1, Wout[0], d_sigma)
    feat.backward(ours["d_feature"])
    gW1, gWout = MR.unpack(q.grad, H)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(ours["sigma"], sigma.detach()) <= 1e-12 and rel(ours["dW1"], gW1) <= 1e-12 and rel(ours["dWo"], gWout[0]) <= 1e-12
    assert rel(table.grad, q.grad[spec.n_mlp_params:]) <= 1e-12
    # the sequential sums are the same function
    seq = MR.backward(feat.detach(), W1, Wout[0], d_sigma, sequential=True)
    assert all(rel(seq[k], ours[k]) <= 1e-12 for k in ("sigma", "dW1", "dWo", "d_feature"))


# ------------------------------------------------------------------------------------------- the lattice against the published algorithm
def _levels(enc):
    """tests/known_answer.py levels() for another config"""
    out, offset = [], 0
    for l in range(enc["n_levels"]):
        scale = Fr(2) ** l * enc["base_resolution"] - 1
        res = ceil(scale) + 1
        entries = min((res ** 3 + 7) // 8 * 8, 2 ** enc["log2_hashmap_size"])
        out.append(dict(scale=scale, res=res, entries=entries, offset=offset))
        offset += entries
    return out


def test_lattice_reference_equals_a_rational_evaluation_of_the_published_algorithm():
    """three coarse-lattice points (one on a face of the cube), 16 neurons: features, sigma and the three gradients with Fractions,
    written as tests/known_answer.evaluate on this file's 16-level config with its corner_terms / grid_index"""
    H, lat = 16, MR.COARSE
    pts_fr = [(Fr(-1, 2), Fr(0), Fr(1, 2)), (Fr(1), Fr(-1), Fr(1, 2)), (Fr(0), Fr(1, 2), Fr(-1, 2))]
    ds_fr = [Fr(1), Fr(1, 2), Fr(-1)]
    grid = MR.lattice_grid()
    table = MR.lattice_table(lat["table_alphabet"], lat["table_den"], MR.TABLE_SEED)
    W1, wo = MR.lattice_weights(H, lat["weight_alphabet"], lat["weight_den"], MR.WEIGHT_SEED)
    lv = _levels(MR.LATTICE_ENC)
    assert [(float(l["scale"]), l["res"], l["entries"], l["offset"]) for l in lv] == [(g.scale, g.res, g.size, g.offset) for g in grid.levels]
    tab = [Fr(float(v)) for v in table]
    w1 = [[Fr(float(v)) for v in row] for row in W1]
    w2 = [Fr(float(v)) for v in wo]
    feats, sigmas = [], []
    dW1 = [[Fr(0)] * 32 for _ in range(H)]
    dWo = [Fr(0)] * H
    d_feat = []
    for pw, ds in zip(pts_fr, ds_fr):
        x = [(c + 1) / 2 for c in pw]
        inp = [sum(w * tab[(l["offset"] + e) * 2 + f] for e, w in K.corner_terms(l, x)) for l in lv for f in range(2)]
        zpre = [sum(w1[j][i] * inp[i] for i in range(32)) for j in range(H)]
        hid = [max(z, Fr(0)) for z in zpre]
        feats.append(inp)
        sigmas.append(sum(w2[j] * hid[j] for j in range(H)))
        for j in range(H):
            dWo[j] += ds * hid[j]
            if zpre[j] > 0:
                for i in range(32):
                    dW1[j][i] += ds * w2[j] * inp[i]
        d_feat.append([sum(ds * w2[j] * w1[j][i] for j in range(H) if zpre[j] > 0) for i in range(32)])
    t64 = lambda rows: torch.tensor([[float(v) for v in row] for row in rows], dtype=F64)
    pts = t64(pts_fr).float()
    for dtype in (F32, F64):
        feat = torch.cat(ER.encode(grid, table, pts, dtype)["feat"], dim=1)
        assert torch.equal(feat.double(), t64(feats))
        r = MR.backward(feat, W1.to(dtype), wo.to(dtype), t64([ds_fr])[0].to(dtype))
        assert torch.equal(r["sigma"].double(), t64([sigmas])[0])
        assert torch.equal(r["dW1"].double(), t64(dW1)) and torch.equal(r["dWo"].double(), t64([dWo])[0])
        assert torch.equal(r["d_feature"].double(), t64(d_feat))
    assert any(s != 0 for s in sigmas) and any(v != 0 for v in dWo)


# ------------------------------------------------------------------------------------------- builders
def test_lattice_builders_deliver_what_they_promise():
    grid = MR.lattice_grid()
    assert [lv.scale for lv in grid.levels] == [float(2 ** (l + 1) - 1) for l in range(16)]
    for lat, count in ((MR.FINE, 729), (MR.COARSE, 125)):
        pts = MR.lattice_points(3 * count + 11, lat["denominator"], 7)
        assert torch.unique(pts, dim=0).shape[0] == count and not bool((pts[1:] == pts[:-1]).all(dim=1).any())
        assert torch.equal(pts * lat["denominator"], torch.round(pts * lat["denominator"])) and float(pts.abs().max()) == 1.0
        table = MR.lattice_table(lat["table_alphabet"], lat["table_den"], 3)
        assert table.numel() == grid.n_entries * 2
        assert set((table * lat["table_den"]).tolist()) == set(float(a) for a in lat["table_alphabet"])
    d = MR.lattice_d_sigma(5000, 1, dead=(70, 1500))
    assert set(d.tolist()) == set(MR.D_SIGMA_ALPHABET) | {0.0} and not bool(d[70:1500].any())
    assert 0.10 < float((d[1500:] != 0).double().mean()) < 0.16
    dead = MR.dead_tiles(d, 16)
    assert not bool(dead[:5].any()) and bool(dead[5:93].all()) and not bool(dead[93:].any())          # tiles 4 and 93 are cut by the stretch
    for S in MR.RAY_SAMPLES:
        rays, z = MR.lattice_rays(40, S, 2, 5)
        p = ER.world_points(rays, z)
        exact = rays[:, None, 0:3].double() + rays[:, None, 3:6].double() * z[:, :, None].double()
        assert torch.equal(p.double(), exact) and torch.equal(p * 2, torch.round(p * 2)) and float(p.abs().max()) == 1.0
        assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((rays[:, 3:6].abs().sum(dim=1) == 1).all())
        assert torch.unique(p.reshape(-1, 3), dim=0).shape[0] > 60


# ------------------------------------------------------------------------------------------- preconditions of the exact GPU cases
@pytest.mark.parametrize("route", list(MR.ROUTES))
def test_launch_shapes_give_every_case_three_steps_and_a_ragged_tile(library, route):
    for backward in (False, True):
        shapes = [MR.launch(route, H, backward) for H in MR.WIDTHS]
        assert all(s == shapes[0] for s in shapes)
        s = shapes[0]
        # 5 tiles + 17 samples beyond two rounds: 32-sample tiles 6 waves with a third step and 17 samples in the last, 16-sample tiles 7 and 1
        assert (s["tile"], MR.waves_with_three_steps(s), s["n"] % s["tile"]) in ((32, 6, 17), (16, 7, 1)) and s["n"] % 2 == 1
        last = MR.coordinates(s["n"] - 1, s)
        assert (last["step"], last["wave"], last["pair"]) == ((2, 5, 8) if s["tile"] == 32 else (2, 6, 0))
        lo, hi = MR.dead_stretch(s)
        assert hi - lo > s["R"] and lo % s["tile"] and hi % s["tile"] and lo % 2 and hi < 2 * s["R"]
    print(f"FIGURES {route}: forward n = {MR.launch(route, 64, False)['n']}, backward n = {MR.launch(route, 64, True)['n']}")


@pytest.mark.parametrize("H", MR.WIDTHS)
@pytest.mark.parametrize("route", list(MR.ROUTES))
def test_forward_cases_are_exact_in_float32(library, route, H):
    lat = MR.FORWARD_LATTICE[route]
    n = MR.launch(route, H, False)["n"]
    c = MR.forward_case(lat["name"], n, H)
    f32 = MR.lattice_features(c["grid"], c["table"], c["pts"], F32)
    assert torch.equal(f32.double(), c["feat64"])
    bits = MR.significant_bits(f32)
    budget = MR.exact_budget(c["feat64"], c["W1"], c["wo"])
    print(f"FIGURES forward {route} H={H} {lat['name']} lattice, n = {n}: features {bits} significant bits; {MR.log2_figures(budget)}; "
          f"pre-activations {c['z_share'][0]:.3f} positive, {c['z_share'][1]:.3f} negative, {c['z_share'][2]:.4f} zero")
    assert bits <= (16 if lat is MR.FINE else 11)          # bf16 x 2 holds 16 bits (the third term is zero), fp16 holds 11
    assert max(budget.values()) < 2.0 ** 24
    assert c["z_share"][0] >= 0.2 and c["z_share"][1] >= 0.2 and c["z_share"][2] > 0
    assert torch.unique(c["pts"], dim=0).shape[0] == (2 * lat["denominator"] + 1) ** 3
    if route == "f16_fast":
        s16, _ = MR.mlp(MR.round_f16(f32), MR.round_f16(c["W1"]), MR.round_f16(c["wo"]))
        assert torch.equal(s16.double(), c["sigma64"])
    assert torch.equal(c["sigma64"].float().double(), c["sigma64"])


@pytest.mark.parametrize("H", MR.WIDTHS)
@pytest.mark.parametrize("route", ["bf3", "fast32"])          # (f16_fast has bf3's launch shape: the same case)
def test_backward_cases_are_exact_in_float32_and_in_fp16_storage(library, route, H):
    s = MR.launch(route, H, True)
    assert route != "bf3" or MR.launch("f16_fast", H, True) == s
    c = MR.backward_case(s["n"], s["tile"], s["R"], H)
    f32 = MR.lattice_features(c["grid"], c["table"], c["pts"], F32)
    assert torch.equal(f32.double(), c["feat64"])
    budget = MR.exact_budget(c["feat64"], c["W1"], c["wo"], c["d_sigma"])
    live = c["d_sigma"] != 0
    lo, hi = c["dead"]
    dead_tiles = MR.dead_tiles(c["d_sigma"], s["tile"])
    kinds = MR.pair_kinds(c["d_sigma"])
    print(f"FIGURES backward {route} H={H} coarse lattice, n = {s['n']}: {int(live.sum())} live samples, dead stretch [{lo}, {hi}), "
          f"{int(dead_tiles.sum())} of {dead_tiles.numel()} steps skipped; pairs both / even / odd live {kinds}; features "
          f"{MR.significant_bits(f32)} significant bits; {MR.log2_figures(budget)}; pre-activations {c['z_share'][0]:.3f} positive, "
          f"{c['z_share'][1]:.3f} negative, {c['z_share'][2]:.4f} zero")
    assert max(budget.values()) < 2.0 ** 24
    assert c["z_share"][0] >= 0.2 and c["z_share"][1] >= 0.2 and c["z_share"][2] > 0
    # every step outside the dead stretch holds a live sample; all three kinds of pair occur
    outside = torch.ones(dead_tiles.numel(), dtype=torch.bool)
    outside[(lo + s["tile"] - 1) // s["tile"]:hi // s["tile"]] = False
    assert not bool(dead_tiles[outside].any()) and bool(dead_tiles[~outside].all()) and not bool(live[lo:hi].any())
    assert min(kinds) > 0
    # float32 (sequential) and the fp16 storage model reproduce the float64 run bit for bit
    r64 = MR.backward(c["feat64"], c["W1"].double(), c["wo"].double(), c["d_sigma"].double())
    assert all(torch.equal(r64[k], c["r64"][k]) for k in ("sigma", "dW1", "dWo", "d_feature"))
    for name, r in (("float32", MR.backward(f32, c["W1"], c["wo"], c["d_sigma"])), ("fp16 storage", MR.backward_f16_storage(f32, c["W1"], c["wo"], c["d_sigma"]))):
        for k in ("sigma", "Z", "dZ", "dW1", "dWo", "d_feature"):
            assert torch.equal(r[k].double(), r64[k]), (name, k)
    assert torch.equal(MR.round_f16(r64["Z"]), r64["Z"]) and torch.equal(MR.round_f16(r64["dZ"]), r64["dZ"])
    assert bool(r64["dW1"].any(dim=1).all()) and bool(r64["dWo"].any())


@pytest.mark.parametrize("S", MR.RAY_SAMPLES)
def test_rays_cases_end_ragged_where_the_sample_count_allows(library, S):
    for route in ("bf3", "fast32"):
        s = MR.launch(route, 64, True)
        c = MR.rays_case(s["n"], S)
        assert c["live"] < c["n_rays"] and 2 * s["R"] + s["tile"] < c["M"] <= s["n"] and c["M"] % 2 == S % 2
        assert (c["M"] % 32 != 0) == (S % 32 != 0)
        assert torch.equal(c["pts"] * 2, torch.round(c["pts"] * 2)) and float(c["pts"].abs().max()) == 1.0
