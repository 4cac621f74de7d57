#!/usr/bin/env python3
"""Seventh batch of golden fixtures, produced by IMPORTING THE REFERENCE in the build container.

    python tests/golden/make_golden7.py

G17  camera rays.  The reference's CameraRayDirections (src/common/ray_utils.py:128-225) for a 12 x 16 image: `directions`, the two
     meshgrids, and the records of fetch_chunk_rays (one chunk of 192 rays) for three camera poses - the identity, a general pose,
     and one 0.4 m from a cube wall, so that different cube faces give the far value within one image - and one build_rays call
     with scattered indices.

The stand-ins of make_golden.py apply.  kornia is not installed, so make_golden.install_stubs() mocks it; this script replaces the
mocked kornia.geometry.calibration.undistort_points by the identity on the points.  That is valid EXACTLY for the case captured
here - all distortion coefficients zero and new_k == k, where undistorting is the identity (the reference's lidar-only default,
analysis/renderer.py:113-120) - and for nothing else: distortion is tested by round trip, not against a capture.  Everything else
executing below is the reference's own code.  The fixture is data; nothing reads the reference at test time.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as MG                      # noqa: E402  (stubs, save)

H, W = 12, 16
K = [[14.0, 0.0, 7.5], [0.0, 13.0, 6.25], [0.0, 0.0, 1.0]]
SCALE, SHIFT = 42.5, [1.5, -2.0, 0.75]
RAY_RANGE = [1.0, 50.0]
# translation + axis-angle: the identity, a general pose, and one 0.4 m from the +x wall of the cube (x = SCALE - SHIFT[0] = 41 m)
POSES6 = [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [3.0, -4.5, 1.25, 0.3, -0.7, 1.9], [40.6, 38.0, -5.0, -1.1, 0.4, 0.2]]
SCATTERED = [191, 0, 17, 17, 100, 5, 160, 31, 32, 48]


def main():
    MG.install_stubs()
    from kornia.geometry import calibration
    calibration.undistort_points = lambda points, k, dist, new_k: points          # zero distortion, new_k == k: the identity
    from common.pose import Pose
    from common.pose_utils import WorldCube
    from common.ray_utils import CameraRayDirections
    from common.settings import Settings

    k = torch.tensor(K)
    calib = Settings({"camera_intrinsic": {"width": W, "height": H, "k": k, "new_k": k.clone(), "distortion": torch.zeros(4)}})
    wc = WorldCube(torch.tensor(SCALE), torch.tensor(SHIFT))
    crd = CameraRayDirections(calib, chunk_size=H * W, device="cpu")
    assert crd.num_chunks == 1
    out = dict(height=np.int64(H), width=np.int64(W), k=k, scale=np.float32(SCALE), shift=np.float32(SHIFT),
               ray_range=np.float32(RAY_RANGE), poses6=np.float32(POSES6), scattered=np.int64(SCATTERED),
               directions=crd.directions, i_meshgrid=crd.i_meshgrid, j_meshgrid=crd.j_meshgrid)
    for i, p6 in enumerate(POSES6):
        pose = Pose(pose_tensor=torch.tensor(p6))
        T = pose.get_transformation_matrix().detach().clone()
        rays = crd.fetch_chunk_rays(0, pose.clone(), wc, torch.tensor(RAY_RANGE))
        assert rays.shape == (H * W, 13) and rays.dtype == torch.float32 and bool(torch.isfinite(rays).all())
        out[f"T{i}"] = T
        out[f"rays{i}"] = rays
        print(i, "far", float(rays[:, 12].min()), float(rays[:, 12].max()))
    pose = Pose(pose_tensor=torch.tensor(POSES6[1]))
    out["rays_scattered"] = crd.build_rays(torch.tensor(SCATTERED), pose.clone(), None, wc, torch.tensor(RAY_RANGE))[0]
    MG.save("g17_camera_rays", **out)


if __name__ == "__main__":
    main()
