"""The density workspace layout and route, pinned (no GPU): lnr_density_workspace, lnr_density_workspace_forward and every field of
lnr_density_route (forward and backward) for every network of tests/test_gpu_kernels.py NETS plus the benchmark's default table
size, at the point counts where make_layout and lnr_route change what they do.  tests/golden/density_layout.json holds the values the
library gave when the binned partition's region headroom went (docs/HISTORY.md 14); host code that only moves must reproduce them.

    python tests/test_density_layout_host.py --record      rewrites the file from the library as built (a deliberate layout change)
"""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "density_layout.json")

# 1, 63..65: the 64-sample plane padding; 2047..2049: one more batch group of 512 samples x 4 batches (before the rounding to 4 groups);
# 16384, 32768: a plane stride that is a multiple of 64 KiB (the skew applies), 16385: just past it; 76800: several reduce workgroups
# per owner; 2^21: the benchmark's window; 2^25 - 2048 and the next: the register-resident kernels' 32-bit plane offsets end there
COUNTS = [1, 63, 64, 65, 2047, 2048, 2049, 16384, 16385, 32768, 76800, 1 << 21, (1 << 25) - 2048, (1 << 25) - 2047]
ROUTE_FIELDS = ("kind", "w_lds", "waves", "dw64", "f16_part", "grid", "tile")


def _nets():
    from tests.test_gpu_kernels import NETS
    nets = dict(NETS)
    nets["bench_default"] = (dict(otype="HashGrid", n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16),
                             dict(activation="ReLU", n_neurons=64, n_hidden_layers=1))
    return nets


def _measure():
    from loner_amd import hip, ops
    lib = hip.load()
    out = {}
    for name, (enc, net) in _nets().items():
        spec = hip.make_net_spec(enc, net)
        rows = []
        for n in COUNTS:
            routes = [[int(getattr(ops.density_route(spec, n, backward), f)) for f in ROUTE_FIELDS] for backward in (False, True)]
            rows.append([int(lib.lnr_density_workspace(C.byref(spec), n)), int(lib.lnr_density_workspace_forward(C.byref(spec), n))] + routes)
        out[name] = rows
    return dict(counts=COUNTS, route_fields=list(ROUTE_FIELDS), nets=out)


@pytest.fixture(scope="module")
def measured():
    import __graft_entry__ as ge
    ge.build()
    return _measure()


def test_workspace_sizes_and_routes_are_the_recorded_ones(measured):
    want = json.load(open(GOLDEN))
    assert want["counts"] == COUNTS and want["route_fields"] == list(ROUTE_FIELDS)
    assert sorted(want["nets"]) == sorted(measured["nets"])
    for name, rows in want["nets"].items():
        for n, w, g in zip(COUNTS, rows, measured["nets"][name]):
            assert g[0] == w[0], (name, n, "lnr_density_workspace")
            assert g[1] == w[1], (name, n, "lnr_density_workspace_forward")
            assert g[2] == w[2], (name, n, "forward route", ROUTE_FIELDS)
            assert g[3] == w[3], (name, n, "backward route", ROUTE_FIELDS)


def test_recorded_layout_has_the_seams_it_is_there_for(measured):
    """The cases are worth their place only if the layout does change across them: the padding step, the skew, the 2^25 - 2048 limit."""
    rows = dict(zip(COUNTS, measured["nets"]["default"]))
    assert rows[1][1] == rows[63][1] == rows[64][1] < rows[65][1]                      # planes padded to 64 samples
    per_sample = (rows[16385][1] - rows[65][1]) / (16448 - 128)                         # bytes of feature planes per padded sample
    assert rows[16384][1] - rows[65][1] > per_sample * (16384 - 128)                   # 16384 x 4 B = 64 KiB: the skew is on top
    assert rows[2047][0] <= rows[2048][0] < rows[2049][0]
    kind = ROUTE_FIELDS.index("kind")
    assert rows[(1 << 25) - 2048][3][kind] != rows[(1 << 25) - 2047][3][kind]          # bf16x3 ends, the general kernels take over


if __name__ == "__main__" and "--record" in sys.argv:
    from loner_amd.build import build
    build(verbose=False)
    with open(GOLDEN, "w") as f:
        f.write(json.dumps(_measure(), separators=(",", ":")).replace('],"', '],\n"').replace("]],[", "]],\n[") + "\n")
    print("wrote", GOLDEN)
