"""Helpers shared by the GPU tests and the fixture generators (tests/golden/make_golden*.py).  No reference code, no GPU."""
import torch

SMALL_ENC = dict(otype="HashGrid", n_levels=4, n_features_per_level=2, log2_hashmap_size=12, base_resolution=8)
SMALL_NET = dict(activation="ReLU", n_neurons=32, n_hidden_layers=1, otype="FullyFusedMLP", output_activation="None")


def small_settings(n_rays, n_samples, voxel=32, n_test=None):
    """default_optimizer_settings() with the small density network of the G8/G9/G11/G12 fixtures"""
    from loner_amd.common.settings import default_optimizer_settings
    s = default_optimizer_settings()
    mc = s["model_config"]
    mc["model"]["nerf_config"]["pos_encoding_sigma"] = dict(SMALL_ENC)
    mc["model"]["nerf_config"]["sigma_network"] = dict(SMALL_NET)
    mc["model"]["nerf_config"]["pos_encoding_intensity"]["log2_hashmap_size"] = 10
    mc["model"]["render"]["N_samples_train"] = n_samples
    if n_test is not None:
        mc["model"]["render"]["N_samples_test"] = n_test
    mc["model"]["occ_model"]["voxel_size"] = voxel
    s["num_samples"]["lidar"] = n_rays
    s["num_samples"]["sky"] = 0
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# Which MLP kernels a density network runs on, so that a test can assert the route its shape is meant to cover (a change to the dispatch
# then fails a test instead of silently moving coverage elsewhere).  The decision lives in one place, lnr_route of
# loner_amd/csrc/lnr_density.hip, which the launch path reads; this asks the library for it (lnr_density_route).  No GPU.
# ---------------------------------------------------------------------------------------------------------------------------
def density_route(enc, net, n_points, backward=True, shape=False):
    """-> dict(route=..., ...) for the tinycudann-style configs `enc`, `net` at `n_points` samples; shape: with the launch shape of the MLP
    kernels as well, `grid` workgroups and `tile` samples per wave step (wave w of workgroup b runs tiles 4 b + w, + 4 grid, ...).
    routes: "wide" (256 x 2..3 layer by layer, both precisions); fp32: "bf3" / "fast32" (the default shape class), "regs" (register-
    accumulating backward, `w_lds` 1 all weights / 2 hidden matrices / 0 none in LDS), "lds" (LDS-accumulating kernels, tier `w_lds`,
    `waves`, `dw64`); fp16: "f16_fast" (the default shape class), "f16_freq" (fused frequency kernels) and "f16_gen" (features from pair
    planes), the last two with `obj` = the object the run-time-activation kernels live in (backward 1: <= 64 neurons, 2: 128 and 256;
    forward 1; None: the compile-time ReLU / Sine kernels)."""
    from loner_amd import hip, ops
    r = ops.density_route(hip.make_net_spec(enc, net), n_points, backward)
    route = hip.ROUTE_KINDS[r.kind]
    more = dict(grid=r.grid, tile=r.tile) if shape else {}
    if route in ("f16_freq", "f16_gen"):
        return dict(route=route, obj=r.f16_part or None, **more)
    if route == "regs":
        return dict(route=route, w_lds=r.w_lds, **more)
    if route == "lds":
        return dict(route=route, w_lds=r.w_lds, waves=r.waves, dw64=r.dw64, **more)
    return dict(route=route, **more)


ACTIVATION_NAMES = ["None", "ReLU", "Sine", "LeakyReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh"]   # loner_amd/hip.py


def _freq(nf):
    return dict(otype="Frequency", n_frequencies=nf)


def _hash(levels, features=2):
    return dict(otype="HashGrid", n_levels=levels, n_features_per_level=features, log2_hashmap_size=10, base_resolution=4, per_level_scale=1.3)


# One network per MLP route, the smallest shape that reaches it (tests/test_gpu_activations.py runs every activation on each):
# name -> (encoding config, network config without the activation, the route density_route must name for its backward).  More than 128
# inputs come from a hash grid: a frequency encoding that wide reaches 2^23 pi x, whose fp32 input gradient is noise.
ACTIVATION_ROUTES = {
    "f32_lds_n16": (_hash(4), dict(n_neurons=16, n_hidden_layers=1), dict(route="lds", w_lds=1, waves=4, dw64=1)),
    "f32_lds_n32x2": (_freq(4), dict(n_neurons=32, n_hidden_layers=2), dict(route="lds", w_lds=1, waves=4, dw64=1)),
    "f32_lds_in144": (_hash(18, 8), dict(n_neurons=32, n_hidden_layers=1), dict(route="lds", w_lds=1, waves=4, dw64=1)),
    "f32_lds_2waves": (_hash(18, 8), dict(n_neurons=64, n_hidden_layers=2), dict(route="lds", w_lds=1, waves=2, dw64=0)),
    "f32_lds_global_w": (_hash(18, 8), dict(n_neurons=128, n_hidden_layers=1), dict(route="lds", w_lds=0, waves=4, dw64=0)),
    "f32_regs_all": (_freq(8), dict(n_neurons=64, n_hidden_layers=1), dict(route="regs", w_lds=1)),
    "f32_regs_hidden": (_freq(8), dict(n_neurons=128, n_hidden_layers=2), dict(route="regs", w_lds=2)),
    "f32_regs_none": (_freq(8), dict(n_neurons=128, n_hidden_layers=3), dict(route="regs", w_lds=0)),
    "f32_regs_256x1": (_freq(6), dict(n_neurons=256, n_hidden_layers=1), dict(route="regs", w_lds=1)),
    "f32_wide_256x2": (_freq(6), dict(n_neurons=256, n_hidden_layers=2), dict(route="wide")),
    "f16_gen_n64": (_hash(4), dict(n_neurons=64, n_hidden_layers=2, precision="fp16"), dict(route="f16_gen", obj=1)),
    "f16_gen_n128": (_hash(4), dict(n_neurons=128, n_hidden_layers=2, precision="fp16"), dict(route="f16_gen", obj=2)),
    "f16_freq_n64": (_freq(8), dict(n_neurons=64, n_hidden_layers=2, precision="fp16"), dict(route="f16_freq", obj=1)),
    "f16_wide_256x2": (_freq(6), dict(n_neurons=256, n_hidden_layers=2, precision="fp16"), dict(route="wide")),
}


def route_of(name, activation, n_points):
    """density_route of ACTIVATION_ROUTES[name] with `activation`, without the object number of ReLU / Sine (compile-time kernels)"""
    enc, net, _ = ACTIVATION_ROUTES[name]
    return density_route(enc, dict(net, activation=activation), n_points)


# G13 (tests/golden/make_golden3.py): the reduced window of the matched-L1 fixture
G13 = dict(n_rays=256, n_samples=128, n_test=256, n_l1_rays=512, pose_noise_seed=41, init_seed=1234)


class SeededReplay:
    """The random draws of a recorded reference run, regenerated from its seed: every draw of the reference came from torch's
    global CPU generator in a fixed order, so a private generator with the same seed issuing the same calls yields the same values
    (make_golden3.py verified that for the recorded run).  Interface of the `draws` hook (Optimizer.set_draws / sampler.set_draws);
    `kinds` / `args` are the recorded call signatures, checked call by call; `checksum` accumulates the values handed out."""

    def __init__(self, seed, kinds, args):
        self.gen = torch.Generator().manual_seed(int(seed))
        self.kinds, self.args, self.i, self.checksum = [int(k) for k in kinds], [tuple(int(v) for v in a) for a in args], 0, 0.0

    def _next(self, kind, a):
        assert self.i < len(self.kinds), "more draws than the reference made"
        assert (self.kinds[self.i], self.args[self.i]) == (kind, a), (self.i, self.kinds[self.i], self.args[self.i], kind, a)
        self.i += 1

    def _out(self, t):
        self.checksum += float(t.double().sum())
        return t

    def ray_index(self, n_points, count):
        self._next(0, (int(n_points), int(count), 0))
        return self._out(torch.randint(0, int(n_points), (int(count),), generator=self.gen))

    sky_index = ray_index

    def jitter(self, n, h):
        self._next(1, (0, int(n), int(h)))
        return self._out(torch.rand(int(n), int(h), generator=self.gen))

    pdf = jitter

    def noise(self, n, s):
        self._next(2, (0, int(n), int(s)))
        return self._out(torch.randn(int(n), int(s), generator=self.gen))


def sky_directions(n=40, seed=3):
    """unit vectors pointing up and outwards, sensor frame [3,n] (what the sky segmentation hands to LidarScan.sky_rays)"""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(3, n, generator=gen)
    v[2] = v[2].abs() + 0.5
    return torch.nn.functional.normalize(v, dim=0)


def l1_scan_subset(n=512, total=65536):
    """ray indices of the synthetic scan used by the compute_l1_depth fixture (every 128th ray, offset 7)"""
    return torch.arange(7, total, total // n)[:n]


def write_repo_checkpoint(path, seed=5):
    """A checkpoint as the reference's Mapper.build_ckpt would write it (mapper.py:161-175), with the state_dicts of THIS
    repo's Model / OccupancyGridModel: "trained-like" parameters (tables x3000, random occupancy logits) from fixed seeds.
    Building a state_dict needs no GPU.  -> dict(sigma_params, occ_grid)"""
    from loner_amd.models.model_tcnn import Model, OccupancyGridModel
    s = small_settings(48, 64, n_test=256)
    mc = s.model_config.model
    torch.manual_seed(seed)
    model = Model(mc)
    occ = OccupancyGridModel(mc.occ_model)
    gen = torch.Generator().manual_seed(seed + 1)
    sig = model.nerf_model._model_sigma
    with torch.no_grad():
        sig.params[sig.spec.n_mlp_params:] *= 3000.0
        occ.occupancy_grid.copy_(torch.randn(occ.occupancy_grid.shape, generator=gen) * 2.0)
    adam = torch.optim.Adam([{"params": [sig.params], "lr": 1e-2}])
    sgd = torch.optim.SGD([occ.occupancy_grid], lr=1e-4)
    ckpt = {"global_step": 0, "network_state_dict": model.state_dict(), "optimizer_state_dict": adam.state_dict(), "poses": [],
            "occ_model_state_dict": occ.state_dict(), "occ_optimizer_state_dict": sgd.state_dict()}
    torch.save(ckpt, path)
    return dict(sigma_params=sig.params.detach().clone(), occ_grid=occ.occupancy_grid.detach().clone())


# ---------------------------------------------------------------------------------------------------------------------------
# Reference-shaped callers (boundary test).  In an integration the Optimizer is handed the REFERENCE's own
# KeyFrame / Frame / Pose / LidarScan / Settings objects.  The stand-ins below expose exactly the members
# those classes expose - written from the member list of SURVEY 8b and the class summaries in INTEGRATION.md, with the behaviours the
# hot path depends on (CPU tensors; list -> tuple on attribute access of the settings; a Pose whose matrix is cached at construction
# and recomputed from the 6-vector only while that vector requires a gradient) - and REFUSE every other attribute: setting a member
# the reference class does not have raises, reading one raises AttributeError as usual.  If loner_amd touches anything beyond the
# reference's surface, the boundary test fails.
# ---------------------------------------------------------------------------------------------------------------------------
class _Surface:
    _MEMBERS = ()

    def __setattr__(self, name, value):
        assert name in self._MEMBERS, f"{type(self).__name__} has no member '{name}' in the reference: loner_amd must not set it"
        object.__setattr__(self, name, value)


def _aa_to_matrix(p6):
    """[t, axis-angle] -> 4x4 (the quaternion route of pytorch3d 0.7.2), differentiable"""
    aa = p6[3:6]
    theta = torch.linalg.norm(aa)
    half = theta * 0.5
    k = torch.where(theta.abs() < 1e-6, 0.5 - theta * theta / 48.0, torch.sin(half) / torch.where(theta.abs() < 1e-6, torch.ones_like(theta), theta))
    q = torch.cat([torch.cos(half)[None], aa * k])
    r, i, j, kk = q[0], q[1], q[2], q[3]
    two_s = 2.0 / (q * q).sum()
    R = torch.stack([1 - two_s * (j * j + kk * kk), two_s * (i * j - kk * r), two_s * (i * kk + j * r),
                     two_s * (i * j + kk * r), 1 - two_s * (i * i + kk * kk), two_s * (j * kk - i * r),
                     two_s * (i * kk - j * r), two_s * (j * kk + i * r), 1 - two_s * (i * i + j * j)]).reshape(3, 3)
    T = torch.eye(4, dtype=p6.dtype)
    T = T.clone()
    T[:3, :3] = R
    T[:3, 3] = p6[0:3]
    return T


class RefShapedPose(_Surface):
    """src/common/pose.py:23-166 by member name.  The quirk that matters at the boundary: get_transformation_matrix() returns the
    matrix CACHED AT CONSTRUCTION unless the 6-vector currently requires a gradient (pose.py:140-144)."""
    _MEMBERS = ("_pose_tensor", "_transformation_matrix")

    def __init__(self, transformation_matrix=None, pose_tensor=None, fixed=None, requires_tensor=False):
        if transformation_matrix is None and pose_tensor is None:
            transformation_matrix = torch.eye(4)
        if fixed is None:
            fixed = not (pose_tensor if transformation_matrix is None else transformation_matrix).requires_grad
        if pose_tensor is not None:
            self._pose_tensor = pose_tensor
            self._pose_tensor.requires_grad_(not fixed)
            transformation_matrix = _aa_to_matrix(self._pose_tensor).float()
        else:
            assert not requires_tensor, "not needed by the boundary test"
            self._pose_tensor = None
            transformation_matrix = transformation_matrix.float()
        self._transformation_matrix = transformation_matrix.detach()
        self._transformation_matrix.requires_grad_(not fixed)

    def set_fixed(self, fixed=True):
        self._pose_tensor.requires_grad_(not fixed)

    def to(self, device):
        if self._pose_tensor is not None:
            self._pose_tensor = self._pose_tensor.to(device)
        self._transformation_matrix = self._transformation_matrix.to(device)
        return self

    def detach(self):
        return RefShapedPose(self.get_transformation_matrix().detach())

    def clone(self, fixed=None, requires_tensor=False):
        m = self.get_transformation_matrix()
        return RefShapedPose(m.detach().clone(), fixed=(not m.requires_grad) if fixed is None else fixed)

    def get_transformation_matrix(self):
        if self._pose_tensor is None or not self._pose_tensor.requires_grad:
            return self._transformation_matrix
        return _aa_to_matrix(self._pose_tensor)

    def get_pose_tensor(self):
        assert self._pose_tensor is not None, "the boundary test builds its poses from 6-vectors"
        return self._pose_tensor

    def get_translation(self):
        return self._pose_tensor[:3] if self._pose_tensor is not None else self._transformation_matrix[:3, 3]

    def get_rotation(self):
        return self.get_transformation_matrix()[:3, :3]

    def get_axis_angle(self):
        return self._pose_tensor[3:]


class RefShapedLidarScan(_Surface):
    """src/common/sensors.py:57-167 by member name: SoA CPU tensors, `len()` = number of timestamps."""
    _MEMBERS = ("ray_directions", "distances", "timestamps", "sky_rays")

    def __init__(self, ray_directions, distances, timestamps, sky_rays=None):
        self.ray_directions, self.distances, self.timestamps, self.sky_rays = ray_directions, distances, timestamps, sky_rays

    def __len__(self):
        return self.timestamps.shape[0]

    def get_start_time(self):
        return self.timestamps[0]

    def get_end_time(self):
        return self.timestamps[-1]

    def to(self, device):
        self.ray_directions, self.distances, self.timestamps = (t.to(device) for t in (self.ray_directions, self.distances, self.timestamps))
        return self


class RefShapedFrame(_Surface):
    """src/common/frame.py:22-156 by member name."""
    _MEMBERS = ("image", "lidar_points", "_lidar_to_camera", "_lidar_pose", "_gt_lidar_pose", "_id")

    def __init__(self, image=None, lidar_points=None, T_lidar_to_camera=None):
        self.image, self.lidar_points, self._lidar_to_camera = image, lidar_points, T_lidar_to_camera
        self._lidar_pose, self._gt_lidar_pose, self._id = None, None, -1

    def to(self, device):
        self.lidar_points.to(device)
        for p in (self._lidar_to_camera, self._lidar_pose, self._gt_lidar_pose):
            if p is not None:
                p.to(device)
        return self

    def get_time(self):
        return self.lidar_points.get_start_time()

    def get_lidar_pose(self):
        return self._lidar_pose


class RefShapedKeyFrame(_Surface):
    """src/mapping/keyframe.py:24-69,126-135 by member name (build_lidar_rays / build_camera_rays are the reference's CPU ray
    builders: the optimiser under test must not need them)."""
    _MEMBERS = ("_frame", "_device", "_tracked_lidar_pose", "is_anchored", "lidar_loss_distribution")

    def __init__(self, frame, device=None):
        self._frame = frame.to(device) if device is not None else frame
        self._device = device
        self._tracked_lidar_pose = frame.get_lidar_pose().clone()
        self.is_anchored = False
        self.lidar_loss_distribution = None

    def get_lidar_pose(self):
        return self._frame.get_lidar_pose()

    def get_lidar_scan(self):
        return self._frame.lidar_points

    def get_time(self):
        return self._frame.get_time()

    def build_lidar_rays(self, *a, **k):
        raise AssertionError("the HIP optimiser builds its rays on the device from the scan buffers")

    def get_pose_state(self):
        return {"timestamp": self.get_time().detach().cpu().clone(),
                "lidar_pose": self._frame.get_lidar_pose().get_pose_tensor().detach().cpu().clone(),
                "gt_lidar_pose": self._frame._gt_lidar_pose.get_pose_tensor().detach().cpu().clone(),
                "tracked_pose": self._tracked_lidar_pose.get_transformation_matrix().detach().cpu().clone()}


class RefShapedSettings(dict):
    """attrdict.AttrDict as the reference's Settings uses it (src/common/settings.py:51-75): attribute access, nested dicts wrapped on
    access, LISTS BECOME TUPLES on attribute access (and stay lists on item access); unknown keys raise."""

    def __getattr__(self, key):
        if key not in self:
            raise AttributeError(key)
        return self._build(self[key])

    def __setattr__(self, key, value):
        self[key] = value

    @classmethod
    def _build(cls, obj):
        if isinstance(obj, dict):
            return cls(obj)
        if isinstance(obj, (list, tuple)):
            return tuple(cls._build(v) for v in obj)
        return obj


class RefShapedWorldCube(_Surface):
    """src/common/pose_utils.py:24-57 by member name."""
    _MEMBERS = ("scale_factor", "shift")

    def __init__(self, scale_factor, shift):
        self.scale_factor, self.shift = scale_factor, shift

    def to(self, device, clone=False):
        if clone:
            return RefShapedWorldCube(self.scale_factor.to(device), self.shift.to(device))
        self.scale_factor, self.shift = self.scale_factor.to(device), self.shift.to(device)
        return self
