"""Every encode-backward kernel lnr_encode_backward can select is launched here (pytest -m gpu): the record partition for 1, 2, 4 and 8
features per level and the x-pair form, each in the three input-gradient modes (per-ray sums, d/dx planes, none).  The hashed levels
of f2, f4 and f8 span 64 owner slices; f2 has one level of 8-byte records and one of x-pair records.  The all-atomics route
(LNR_BWD_TABLE_ATOMICS) must give the same bits as the default one, as test_record_partition_equals_global_accumulation requires of
the rays form.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import network as NW

DEV = "cuda"
MLP = dict(activation="ReLU", n_neurons=32, n_hidden_layers=1)
# name -> (encoding, level kinds the net is meant to have: x-pair records per level)
NETS = {
    "f1": (dict(otype="HashGrid", n_levels=2, n_features_per_level=1, log2_hashmap_size=13, base_resolution=8), [False, False]),
    "f2": (dict(otype="HashGrid", n_levels=2, n_features_per_level=2, log2_hashmap_size=18, base_resolution=2048), [False, True]),
    "f4": (dict(otype="HashGrid", n_levels=2, n_features_per_level=4, log2_hashmap_size=17, base_resolution=64), [False, False]),
    "f8": (dict(otype="HashGrid", n_levels=2, n_features_per_level=8, log2_hashmap_size=16, base_resolution=64), [False, False]),
}
ROUTES = {"default": {}, "table_atomics": dict(table_atomics=True)}
MODES = ("d_rays", "d_pts", "none")
N_RAYS, N_SAMPLES = 64, 64          # one wave per ray: the per-ray input-gradient mode applies

SLICE_SHIFT, XPAIR_SCALE_MIN = 13, 3000.0          # lnr_density_api.h


def _level_kinds(spec):
    """x-pair records per level, restated from the NetSpec: lnr_level_can_use_xpairs"""
    F, kinds = spec.n_features, []
    for l in range(spec.n_levels):
        size, off, hashed = int(spec.level_size[l]), int(spec.level_offset[l]), spec.level_hashed[l] != 0
        xp = F == 2 and hashed and size & (size - 1) == 0 and spec.level_scale[l] >= XPAIR_SCALE_MIN and (off * 2) & ((1 << SLICE_SHIFT) - 1) == 0
        kinds.append(bool(xp))
    return kinds


@functools.lru_cache(maxsize=None)
def _setup(net):
    from loner_amd import hip
    enc, want = NETS[net]
    spec = hip.make_net_spec(enc, MLP)
    assert _level_kinds(spec) == want, (net, _level_kinds(spec))
    gen = torch.Generator().manual_seed(17)
    params = NW.init_params(NW.NetworkSpec.from_config(enc, MLP), 5).to(DEV)
    params[spec.n_mlp_params:] *= 500
    o = torch.rand(N_RAYS, 3, generator=gen) * 0.2 - 0.1
    d = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, generator=gen), dim=1)
    rays = torch.zeros(N_RAYS, 13); rays[:, 0:3] = o; rays[:, 3:6] = d; rays[:, 6:9] = -d; rays[:, 11] = 0.01; rays[:, 12] = 0.8
    z = torch.sort(torch.rand(N_RAYS, N_SAMPLES, generator=gen) * 0.75 + 0.01, dim=1).values
    d_sigma = torch.randn(N_RAYS, N_SAMPLES, generator=gen)
    return spec, params, rays.to(DEV), z.to(DEV), d_sigma.to(DEV)


def _backward(ops, net, route, frozen=False):
    """-> {mode: (grad_params, d_rays, d_pts)} of one route"""
    spec, params, rays, z, d_sigma = _setup(net)
    out = {}
    for mode in MODES if not frozen else ("d_rays",):
        grad = None if frozen else torch.zeros(int(spec.n_params), device=DEV)
        d_rays = torch.zeros(N_RAYS, 13, device=DEV) if mode == "d_rays" else None
        d_pts = ops.density_backward(spec, params, d_sigma, grad, rays=rays, z=z, d_rays=d_rays, want_d_pts=mode == "d_pts", **ROUTES[route])
        out[mode] = (grad, d_rays, d_pts)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _reference(ops, net):
    return _backward(ops, net, "default")


@pytest.fixture(scope="module")
def ops():
    from loner_amd import ops as _ops
    from loner_amd import hip
    hip.load()
    return _ops


@pytest.mark.parametrize("net", list(NETS))
def test_default_route_in_every_input_gradient_mode(ops, net):
    spec = _setup(net)[0]
    ref = _reference(ops, net)
    table = slice(int(spec.n_mlp_params), int(spec.n_params))
    for mode in MODES:
        assert float(ref[mode][0][table].abs().max()) > 0 and bool(torch.isfinite(ref[mode][0]).all())
        assert torch.equal(ref[mode][0], ref["d_rays"][0]), mode                    # the parameter gradient does not depend on the mode
    assert float(ref["d_rays"][1][:, 0:6].abs().max()) > 0 and float(ref["d_pts"][2].abs().max()) > 0
    # frozen parameters (grad_params=None): no regions, the same input gradient
    frozen = _backward(ops, net, "default", frozen=True)
    assert torch.equal(frozen["d_rays"][1], ref["d_rays"][1])


@pytest.mark.parametrize("net,route", [(n, r) for n in NETS for r in ROUTES if r != "default"])
def test_route_equals_the_default_route_bit_for_bit(ops, net, route):
    ref, got = _reference(ops, net), _backward(ops, net, route)
    for mode in MODES:
        for what, a, b in zip(("grad_params", "d_rays", "d_pts"), got[mode], ref[mode]):
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(a, b), (net, route, mode, what, int((a != b).sum()))
