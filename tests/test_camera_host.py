"""Camera rendering, the host side (CPU only): the restatement of the camera ray records against the reference's capture (G17),
CameraRayDirections' directions and the distortion round trip, the restated peak and colour map on hand-listed cases and against
matplotlib, the fly-through poses against scipy, and the PNG writer."""
import numpy as np
import pytest
import torch

from tests import camera_restatement as CM


def _calibration(h, w, k, distortion=None, new_k=None):
    from loner_amd.common.settings import Settings
    k = torch.as_tensor(k, dtype=torch.float32)
    return Settings({"camera_intrinsic": {"width": w, "height": h, "k": k, "new_k": k.clone() if new_k is None else new_k,
                                          "distortion": torch.zeros(4) if distortion is None else torch.as_tensor(distortion)}})


# ---------------------------------------------------------------- rays
def test_directions_and_meshgrids_equal_the_reference_bit_for_bit():
    from loner_amd.common.ray_utils import CameraRayDirections
    g = CM.g17()
    h, w = int(g["height"]), int(g["width"])
    crd = CameraRayDirections(_calibration(h, w, g["k"]), device="cpu", chunk_size=50)
    assert len(crd) == h * w and crd.num_chunks == 4 and (crd.im_height, crd.im_width) == (h, w)
    for name in ("directions", "i_meshgrid", "j_meshgrid"):
        got = getattr(crd, name).numpy()
        assert got.dtype == np.float32 and got.shape == g[name].shape
        assert np.array_equal(got.view(np.uint32), g[name].view(np.uint32)), name
    idx = torch.arange(h * w)
    assert torch.equal(crd.i_meshgrid[:, 0], (idx % w).float()) and torch.equal(crd.j_meshgrid[:, 0], (idx // w).float())
    with pytest.raises(AssertionError):
        CameraRayDirections(_calibration(h, w, g["k"]), samples_per_pixel=2, device="cpu")


def test_restated_ray_records_match_the_reference():
    g = CM.g17()
    w = int(g["width"])
    worst = 0.0
    for i in range(3):
        got = CM.camera_rays(g["directions"], None, w, g[f"T{i}"], g["ray_range"][0], g["scale"], g["shift"]).numpy()
        want = g[f"rays{i}"]
        assert got.shape == want.shape == (192, 13)
        for lo, hi in ((0, 3), (3, 9), (9, 11), (11, 12), (12, 13)):        # per block of columns: far is 100 times smaller than x, y
            worst = max(worst, CM.rel_err(got[:, lo:hi], want[:, lo:hi]))
        assert np.array_equal(got[:, 9:11], want[:, 9:11])
    got = CM.camera_rays(g["directions"], g["scattered"], w, g["T1"], g["ray_range"][0], g["scale"], g["shift"]).numpy()
    worst = max(worst, CM.rel_err(got, g["rays_scattered"]))
    # (the reference's own two captures differ in the last bit: its matmul rounds differently for 10 rows and for 192)
    assert CM.rel_err(g["rays_scattered"], g["rays1"][g["scattered"]]) < 1e-6
    print(f"restated camera rays against G17: worst relative error {worst:.3g}")
    assert worst < 1e-6
    # the capture itself: two cube faces within one image for the pose near the wall, every exit point on the cube
    r = g["rays2"]
    p = r[:, :3] + r[:, 3:6] * r[:, 12:13]
    assert len(np.unique(np.abs(p).argmax(1))) >= 2 and np.abs(np.abs(p).max(1) - 1).max() < 1e-5


def test_zero_distortion_returns_the_grid_and_distortion_round_trips():
    from loner_amd.common.ray_utils import get_ray_directions, undistort_points
    h, w = 48, 64
    k = np.array([[55.0, 0.0, 31.5], [0.0, 54.0, 23.5], [0.0, 0.0, 1.0]])
    new_k = np.array([[50.0, 0.0, 32.0], [0.0, 50.0, 24.0], [0.0, 0.0, 1.0]])
    kt = torch.tensor(k, dtype=torch.float32)
    plain, gx, gy = get_ray_directions(h, w, kt, with_indices=True)
    zero = get_ray_directions(h, w, kt, dist=torch.zeros(4), K=kt)
    assert torch.equal(plain, zero)                                              # the grid itself, exactly
    assert torch.equal(plain[:, 0:1], (gx - 31.5) / 55.0) and torch.equal(plain[:, 1:2], (gy - 23.5) / 54.0)
    pix = np.stack([gx[:, 0].numpy(), gy[:, 0].numpy()], axis=1).astype(np.float64)
    worst = 0.0
    for dist in ([0.3, -0.1, 0.01, -0.01], [-0.3, 0.2, -0.008, 0.005], [-0.25, 0.08, 0.003, -0.002, -0.01], [0.0, 0.0, 0.0, 0.0]):
        und = undistort_points(pix, k, dist, new_k)
        norm = np.stack([(und[:, 0] - new_k[0, 2]) / new_k[0, 0], (und[:, 1] - new_k[1, 2]) / new_k[1, 1]], axis=1)
        err = float(np.abs(CM.distort_points(norm, k, dist) - pix).max())
        worst = max(worst, err)
        # and through the fp32 directions CameraRayDirections keeps
        d = get_ray_directions(h, w, torch.tensor(new_k, dtype=torch.float32), dist=dist, K=kt).double().numpy()
        err32 = float(np.abs(CM.distort_points(d[:, :2], k, dist) - pix).max())
        worst = max(worst, err32)
        assert np.all(d[:, 2] == 1.0)
    print(f"distortion round trip over {h} x {w}: worst {worst:.3g} px")
    assert worst < 1e-3
    with pytest.raises(ValueError):
        undistort_points(pix, k, [0.1, 0.2], new_k)


# ---------------------------------------------------------------- peak
def test_restated_peak_follows_argmax():
    nan = float("nan")
    w = torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.1, 0.7, 0.7, 0.2], [0.3, nan, 0.9, nan], [0.0, 0.1, 0.2, 0.3]])
    z = torch.arange(16.0).reshape(4, 4)
    pz, pi = CM.peak(w, z)
    assert pi.tolist() == [0, 1, 1, 3] and pz.tolist() == [0.0, 5.0, 9.0, 15.0]


# ---------------------------------------------------------------- colour map
def test_turbo_table_is_matplotlibs():
    mpl = pytest.importorskip("matplotlib")
    from loner_amd.analysis.turbo import turbo_u8
    t = turbo_u8()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    x = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(256)
    assert np.array_equal(t, (mpl.colormaps["turbo"](x) * 255).astype(np.uint8)[:, :3])


def test_restated_colour_map_equals_matplotlib():
    mpl = pytest.importorskip("matplotlib")
    from loner_amd.analysis.turbo import turbo_u8
    img = np.concatenate([CM.colour_image(100, 100).reshape(-1), np.linspace(0.9, 50.1, 20000, dtype=np.float32)])
    for lo, hi in ((1, 50), (1, 75), (0.5, 12.25)):
        t = torch.from_numpy(img)                                               # save_depth, render_utils.py:116-127
        mask = (t >= hi)
        x = torch.clip((torch.clip(t, lo, hi) - lo) / (hi - lo), 0, 1).numpy()
        coloured = mpl.colormaps["turbo"](x)
        coloured[mask.numpy()] = np.array([0, 0, 0, 1])
        want = (coloured * 255).astype(np.uint8)
        got = CM.depth_colormap(img, turbo_u8(), 1.0, lo, hi)
        assert np.array_equal(got, want), (lo, hi, int((got != want).any(-1).sum()))


def test_restated_colour_map_hand_listed_cases():
    from loner_amd.analysis.turbo import turbo_u8
    t = turbo_u8()
    px = lambda v, **kw: CM.depth_colormap(np.array([v], dtype=np.float32), t, **kw)[0].tolist()
    assert px(1.0) == t[0].tolist() + [255]                        # exactly min_depth: the first colour
    assert px(0.0) == px(-3.0) == px(float("-inf")) == t[0].tolist() + [255]
    assert px(50.0) == [0, 0, 0, 255] and px(1e30) == [0, 0, 0, 255] and px(float("inf")) == [0, 0, 0, 255]      # masked
    assert px(49.999996) == t[255].tolist() + [255]
    assert px(float("nan")) == [0, 0, 0, 0]
    for k in (1, 2, 127, 128, 255):                                # x = k / 256 exactly: the bin edge belongs to bin k
        v = np.float32(k) / np.float32(256)
        assert px(v, min_depth=0, max_depth=1) == t[k].tolist() + [255]
        assert px(np.nextafter(v, np.float32(0)), min_depth=0, max_depth=1) == t[k - 1].tolist() + [255]
    assert px(0.5, multiplier=42.5, min_depth=1, max_depth=50) == px(21.25)     # the multiplier comes first


# ---------------------------------------------------------------- fly-through
def test_slerp_and_linear_interpolation_match_scipy():
    pytest.importorskip("scipy")
    from scipy.interpolate import interp1d
    from scipy.spatial.transform import Rotation, Slerp as ScipySlerp
    from loner_amd.analysis.renderer import Slerp, _interp_linear
    rng = np.random.default_rng(5)
    rots = Rotation.from_rotvec(rng.normal(size=(12, 3)) * np.array([[0.0], [1e-9], [1e-4], [0.3], [1.0], [3.1], [2.0], [0.5], [1.5], [3.0], [0.1], [2.5]]))
    times = np.cumsum(rng.uniform(0.1, 2.0, size=12))
    mine, theirs = Slerp(times, rots.as_matrix()), ScipySlerp(times, rots)
    xyz = rng.normal(size=(12, 3)) * 10
    lin = interp1d(times, xyz, axis=0)
    worst = 0.0
    for t in np.concatenate([times, rng.uniform(times[0], times[-1], 300)]):
        worst = max(worst, float(np.abs(mine(t) - theirs(t).as_matrix()).max()), float(np.abs(_interp_linear(times, xyz, t) - lin(t)).max()))
    print(f"slerp / linear interpolation against scipy: worst {worst:.3g}")
    assert worst < 1e-9
    with pytest.raises(ValueError):
        Slerp([0.0, 0.0, 1.0], rots.as_matrix()[:3])


@pytest.mark.parametrize("render_global", [False, True])
def test_flythrough_poses_match_the_reference_loop(render_global, tmp_path):
    """30 poses over 25 m at 1 m/s and 5 fps: int(length * fps) images and two spins of 75 steps.  fp64 against the transcription of the
    fly-through written on scipy's Slerp and interp1d (tests/camera_restatement.py) to 1e-9; spin indices and pose counts equal."""
    pytest.importorskip("scipy")
    from loner_amd.analysis.renderer import flythrough_poses, flythrough_poses_f64
    rows = CM.trajectory_rows(30, 25.0)
    want, want_spins = CM.flythrough_reference(rows, render_global=render_global)
    got, spins = flythrough_poses_f64(rows, render_global=render_global)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert spins == want_spins and len(spins) == 2 * 2 * 75 and len(want) - 2 * 75 in (124, 125)     # int(length * fps) images
    err = float(np.abs(got - want).max())
    print(f"fly-through poses against the scipy transcription, fp64: worst {err:.3g}")
    assert err < 1e-9
    got32, spins32 = flythrough_poses(rows, render_global=render_global)
    assert got32.dtype == torch.float32 and spins32 == spins and np.array_equal(got32.numpy(), got.astype(np.float32))
    # through a TUM file, with other settings
    path = tmp_path / "traj.txt"
    np.savetxt(path, rows, fmt="%.17g", delimiter=" ")
    got2, spins2 = flythrough_poses_f64(str(path), velocity=2.0, fps=3, spin_spacing_m=7.0, spin_duration_s=2.0, render_global=render_global)
    want2, want_spins2 = CM.flythrough_reference(rows, 2.0, 3, 7.0, 2.0, render_global)
    assert got2.shape == want2.shape and spins2 == want_spins2 and len(spins2) > 0 and float(np.abs(got2 - want2).max()) < 1e-9
    plain, none = flythrough_poses_f64(rows, interpolate=False, render_global=render_global)
    assert none == [] and np.abs(plain - CM.flythrough_reference(rows, render_global=render_global, interpolate=False)[0]).max() < 1e-9


def test_flythrough_poses_hand_computed_straight_line():
    """Three identity poses 2 m apart along x at 1 m/s, 2 images per second, a spin of 2 steps after more than 1.5 m: 4 s give
    int(4 * 2) = 8 images at x = 4 k / 7.  The distance passes 1.5 m at k = 3 (12 / 7 = 1.71) and again at k = 6, so two spin poses
    follow images 3 and 6: 12 poses, spins at [4, 5] and [9, 10], each listed twice.  In the global frame with the line starting at
    x = 10 the first image is already 10 m from the origin the distance is first measured from (the reference's prev_pose starts as
    the identity): a spin follows image 0 as well - 14 poses."""
    from loner_amd.analysis.renderer import flythrough_poses_f64
    quat = [0.0, 0.0, 0.0, 1.0]
    rows = np.array([[0.0, 0.0, 0.0, 0.0] + quat, [1.0, 2.0, 0.0, 0.0] + quat, [2.0, 4.0, 0.0, 0.0] + quat])
    kw = dict(velocity=1.0, fps=2, spin_spacing_m=1.5, spin_duration_s=1.0)
    poses, spins = flythrough_poses_f64(rows, **kw)
    xs = [4.0 * k / 7.0 for k in range(8)]
    want_x = xs[:4] + [xs[3]] * 2 + xs[4:7] + [xs[6]] * 2 + xs[7:]
    assert poses.shape == (12, 4, 4) and spins == [4, 4, 5, 5, 9, 9, 10, 10]
    assert np.abs(poses[:, 0, 3] - np.array(want_x)).max() < 1e-14 and not poses[:, 1:3, 3].any()
    assert np.abs(poses[:, :3, :3] - np.eye(3)).max() < 1e-15                # identity, and turns by 0 and 2 pi
    shifted = rows.copy()
    shifted[:, 1] += 10.0
    poses, spins = flythrough_poses_f64(shifted, render_global=True, **kw)
    want_x = [10.0 + x for x in [xs[0]] * 3 + xs[1:4] + [xs[3]] * 2 + xs[4:7] + [xs[6]] * 2 + xs[7:]]
    assert poses.shape == (14, 4, 4) and spins == [1, 1, 2, 2, 6, 6, 7, 7, 11, 11, 12, 12]
    assert np.abs(poses[:, 0, 3] - np.array(want_x)).max() < 1e-14
    same, spins = flythrough_poses_f64(shifted, render_global=False, **kw)     # relative to the first pose: the first case again
    assert same.shape == (12, 4, 4) and spins == [4, 4, 5, 5, 9, 9, 10, 10]
    # a quarter turn about z between two poses 4 m apart, one image per second: 4 images, the second a third of the way
    half = np.sqrt(0.5)
    rows = np.array([[0.0, 0.0, 0.0, 0.0] + quat, [1.0, 0.0, 4.0, 0.0, 0.0, 0.0, half, half]])
    poses, spins = flythrough_poses_f64(rows, fps=1, spin_spacing_m=100.0)
    a = np.pi / 6
    assert poses.shape == (4, 4, 4) and spins == []
    assert np.abs(poses[1, :3, :3] - np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])).max() < 1e-15
    assert np.abs(poses[1, :3, 3] - np.array([0.0, 4.0 / 3.0, 0.0])).max() < 1e-15 and np.abs(poses[3, :3, 3] - [0, 4, 0]).max() < 1e-15


# ---------------------------------------------------------------- PNG
@pytest.mark.parametrize("shape", [(37, 53, 4), (5, 7, 3), (9, 4), (1, 1, 4)])
def test_png_round_trip(shape, tmp_path):
    from loner_amd.analysis.renderer import write_png
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    write_png(path, img)
    back = CM.read_png(path)
    assert np.array_equal(back.reshape(shape), img)
    write_png(path, torch.from_numpy(img))
    assert np.array_equal(CM.read_png(path).reshape(shape), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert np.array_equal(np.asarray(im).reshape(shape), img)
    for bad in (img.astype(np.float32), np.zeros((2, 2, 2), dtype=np.uint8), np.zeros((0, 4, 4), dtype=np.uint8)):
        with pytest.raises(ValueError):
            write_png(path, bad)


def test_timestamp_names_follow_the_reference_rule():
    from loner_amd.analysis.renderer import lidar_only_calibration, timestamp_name
    assert timestamp_name(torch.tensor(12.3456)) == str(torch.tensor(12.3456).item()).replace(".", "_")[:5] == "12_34"
    assert timestamp_name(torch.tensor(0.0)) == "0_0" and timestamp_name(torch.tensor(3.5, dtype=torch.float64)) == "3_5"
    c = lidar_only_calibration()
    assert (c.camera_intrinsic.width, c.camera_intrinsic.height) == (512, 384)
    assert c.camera_intrinsic.k.tolist() == [[302, 0, 260], [0, 302, 197], [0, 0, 1]] and not bool(c.camera_intrinsic.distortion.any())
    assert list(c.lidar_to_camera.orientation) == [0.5, -0.5, 0.5, -0.5]
