"""Plain restatements of the SLAM loop's host arithmetic in numpy fp64 (loner_amd/mapping/keyframe_manager.py,
loner_amd/logging/default_logger.py): one pose at a time, no batching.  No reference code, no GPU."""
import numpy as np


def random_rigid(rng, spread=1.0):
    """a random rigid 4x4 (fp64): rotation from a normalised random quaternion, translation uniform in [-spread, spread]^3"""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.uniform(-spread, spread, size=3)
    return T


def propagated_pose(optimised_reference, tracked_reference, tracked_new):
    return optimised_reference @ np.linalg.inv(tracked_reference) @ tracked_new


def reconstruct_trajectory(tracked, kf_poses, kf_frames):
    """tracked [n,4,4], keyframe poses [k,4,4], kf_frames [k] the (ascending) frame index each keyframe was made from -> [n,4,4]:
    every pose hung off the last keyframe at or before it; a pose behind the last keyframe hangs off the last keyframe"""
    out = []
    for p, pose in enumerate(tracked):
        r = 0
        for k, f in enumerate(kf_frames):
            if f <= p:
                r = k
        out.append(kf_poses[r] @ np.linalg.inv(tracked[kf_frames[r]]) @ pose)
    return np.stack(out)


def quat_of(R):
    """(x, y, z, w) of a rotation matrix (trace branch; the test rotations are far from 180 degrees)"""
    w = np.sqrt(1.0 + np.trace(R)) / 2.0
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 4 * w * w]) / (4 * w)


def tum_rows(stamps, poses):
    """TUM rows [n,8] (ts x y z qx qy qz qw) of stamps and 4x4 poses"""
    return np.array([[t, *T[:3, 3], *quat_of(T[:3, :3])] for t, T in zip(stamps, poses)])
