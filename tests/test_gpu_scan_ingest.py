"""Scan ingestion on the device (loner_amd.common.sensors.build_scan_from_points, include/loner_hip.h "scan ingestion") against
tests/scan_restatement.py: the order, the times bit for bit, the distances to 2 ulps (the two may differ only in how the sum of squares
rounds), the directions bit for bit against the host's own division by the returned distance, and the flag bits."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import scan_restatement as SR

pytestmark = pytest.mark.gpu

MIN_RANGE = 0.3
SEGMENTS = [[5.0, 180.0], [185.0, 355.0]]
# below one wave, across one sort block (4096), above 65 536 (a third digit of the rank is live), and 128 beams x 512 columns in
# row-major beam order: 128 sorted runs
SHAPES = {"n1": 1, "n63": 63, "n4099": 4099, "n70001": 70001, "beams128x512": 128 * 512}
TIME_CASES = ["none", "local", "nanoseconds", "negative_start", "global", "short_span", "recompute", "sorted", "reversed", "duplicates"]

_inputs = {}


def points_and_base_times(shape):
    """(xyz [N,3] fp32, base times [N] fp64 in [0, 0.1)) of one shape, built once.  Point 0 is kept by both filters and fires at 0;
    from 63 points on, point 1 lies outside both FOV segments and point 2 inside min_range; of the others 3 % lie outside the FOV and
    2 % inside min_range.  No azimuth lies within 0.01 degree of a segment edge, no range within 1 % of min_range."""
    if shape in _inputs:
        return _inputs[shape]
    n = SHAPES[shape]
    gen = torch.Generator().manual_seed(1000 + n)
    u = torch.rand(n, 4, generator=gen, dtype=torch.float64)
    inside = 5.02 + u[:, 0] * 349.96                              # [5.02, 354.98]
    inside = torch.where((inside > 179.98) & (inside < 185.02), inside - 10.0, inside)
    outside = torch.where(u[:, 0] < 0.5, 180.02 + u[:, 0] * 9.92, 355.02 + (u[:, 0] - 0.5) * 19.92)      # (180, 185) or (355, 365)
    theta = torch.where(u[:, 1] < 0.03, outside, inside)
    r = torch.where(u[:, 2] < 0.02, 0.05 + 0.2 * u[:, 3], 1.0 + 40.0 * u[:, 3])
    theta[0], r[0] = 90.0, 7.0
    if n >= 63:
        theta[1], r[1] = 182.5, 9.0
        theta[2], r[2] = 40.0, 0.1
    elev = torch.deg2rad(-20.0 + 40.0 * torch.rand(n, generator=gen, dtype=torch.float64))
    az = torch.deg2rad(theta)
    xyz = torch.stack([r * torch.cos(elev) * torch.cos(az), r * torch.cos(elev) * torch.sin(az), r * torch.sin(elev)], 1).float()
    if shape == "beams128x512":
        base = (torch.arange(512, dtype=torch.float64) / 512 * 0.1).repeat(128)
    else:
        base = torch.rand(n, generator=gen, dtype=torch.float64) * 0.1
        base[0] = 0.0
    _inputs[shape] = (xyz.contiguous(), base)
    return _inputs[shape]


def times_of(case, base):
    """-> (point_times or None, recompute_timestamps)"""
    if case == "none":
        return None, False
    if case == "local":
        return base.clone(), False
    if case == "nanoseconds":
        return (base * 1e9).to(torch.int64), False
    if case == "negative_start":
        return base - 0.05, False
    if case == "global":
        return (base + 1000.0).float(), False
    if case == "short_span":
        return base * 0.004, False
    if case == "recompute":
        return base.clone(), True
    if case == "sorted":
        return torch.sort(base)[0], False
    if case == "reversed":
        return torch.sort(base, descending=True)[0], False
    if case == "duplicates":
        t = base.clone()
        t[3::4] = t[2::4][:len(t[3::4])]
        return t, False
    raise KeyError(case)


EXPECTED_FLAGS = {"none": SR.NO_TIMES | SR.CONSTANT, "local": SR.LOCAL, "nanoseconds": SR.NANOSECONDS | SR.LOCAL,
                  "negative_start": SR.NEGATIVE_START | SR.LOCAL, "global": SR.GLOBAL, "short_span": SR.LOCAL | SR.CONSTANT,
                  "recompute": SR.LOCAL, "sorted": SR.LOCAL, "reversed": SR.GLOBAL | SR.CONSTANT, "duplicates": SR.LOCAL}


@pytest.mark.parametrize("fov_on", [False, True], ids=["fov_off", "fov_two_segments"])
@pytest.mark.parametrize("case", TIME_CASES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scan_matches_the_restatement(shape, case, fov_on):
    from loner_amd.common.sensors import LidarScan, build_scan_from_points
    xyz, base = points_and_base_times(shape)
    n = xyz.shape[0]
    point_times, recompute = times_of(case, base)
    stamp = 1234.5 if n % 2 else 12.25
    fov = SimpleNamespace(enabled=fov_on, range=SEGMENTS)
    want = SR.scan_from_points(xyz, point_times, stamp, SEGMENTS if fov_on else None, MIN_RANGE, recompute)

    # conditions on the inputs, on the restatement's own theta and dist: no point at an edge (atan2f on the device is not torch's)
    if fov_on:
        edges = torch.tensor([e for s in SEGMENTS for e in s])
        assert float((want["theta"][:, None] - edges[None, :]).abs().min()) > 1e-3
    assert float((want["dist"] / MIN_RANGE - 1).abs().min()) > 1e-4
    m = len(want["order"])
    if n >= 63:
        assert bool((want["dist"] <= MIN_RANGE).any())                                          # the range filter drops a point
        if fov_on:
            assert bool((~SR.fov_mask(xyz, SEGMENTS)).any())                                    # and so does the FOV
        assert m >= 0.9 * n
    if n >= 63 and case != "recompute":                                                     # (recompute: the last index decides)
        assert want["flags"] == EXPECTED_FLAGS[case]
    if shape == "n70001" and not want["flags"] & SR.CONSTANT:
        assert m > 65536

    scan, order = build_scan_from_points(xyz, point_times, stamp, fov=fov, min_range=MIN_RANGE, recompute_timestamps=recompute,
                                         device="cuda")
    assert isinstance(scan, LidarScan) and all(t.is_cuda for t in (scan.ray_directions, scan.distances, scan.timestamps, order))
    assert order.dtype == torch.int64 and scan.ray_directions.shape == (3, m) and scan.ray_directions.is_contiguous()
    got_order, got_t, got_d, got_dirs = order.cpu(), scan.timestamps.cpu(), scan.distances.cpu(), scan.ray_directions.cpu()
    assert torch.equal(got_order, want["order"])
    assert torch.equal(got_t.view(torch.int32), want["timestamps"].view(torch.int32))
    assert int(SR.ulp_distance(got_d, want["distances"]).max()) <= 2
    assert torch.equal(got_dirs.view(torch.int32), (xyz[got_order] / got_d[:, None]).T.contiguous().view(torch.int32))
    assert scan.ingest_flags == want["flags"]
    assert scan.time_sorted and bool((got_t[1:] >= got_t[:-1]).all())


def test_device_inputs_are_used_in_place_and_host_arrays_are_accepted():
    from loner_amd.common.sensors import build_scan_from_points
    xyz, base = points_and_base_times("n4099")
    want = SR.scan_from_points(xyz, base, 3.5, None, MIN_RANGE)
    for a, t in ((xyz.cuda(), base.cuda()), (xyz.numpy(), base.numpy().astype(np.float32))):
        scan, order = build_scan_from_points(a, t, 3.5, min_range=MIN_RANGE)
        assert torch.equal(order.cpu(), want["order"]) and torch.equal(scan.timestamps.cpu(), want["timestamps"])


def test_errors():
    from loner_amd.common.sensors import build_scan_from_points
    xyz, base = points_and_base_times("n4099")
    with pytest.raises(ValueError, match="none of the"):
        build_scan_from_points(xyz, base, 1.0, min_range=1e6, device="cuda")
    bad = base.clone()
    bad[0] = math.nan                                            # point 0 is kept
    with pytest.raises(ValueError, match="non-finite time"):
        build_scan_from_points(xyz, bad, 1.0, device="cuda")
    dropped = base.clone()
    dropped[2] = math.nan                                        # point 2 is inside min_range: its time is never looked at
    build_scan_from_points(xyz, dropped, 1.0, device="cuda")
    with pytest.raises(ValueError, match="at most 8"):
        build_scan_from_points(xyz, base, 1.0, fov=SimpleNamespace(enabled=True, range=[[k, k + 1.0] for k in range(9)]), device="cuda")
    with pytest.raises(ValueError, match=r"xyz \[N,3\]"):
        build_scan_from_points(xyz.T.contiguous(), base, 1.0, device="cuda")
