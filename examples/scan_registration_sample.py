#!/usr/bin/env python3
"""match -> register -> integrate: mapping with odometry that drifts, the matched pose refined before the scan goes into the map.

The robot, the room, the sensor and the drift are those of examples/scan_matching_sample.py.  At every step the scan is first placed
by tools.match_scan — the best integer voxel shift and the best of seven headings around the prior — and then handed to
tools.register_scan, which refines that pose by damped Gauss-Newton steps on the trilinear interpolation of the map's score table: a
sub-voxel translation, a continuous yaw, and a covariance that says how well each direction is held.  The scan is integrated at the
registered pose.  Printed per step: the error of the prior, of the matched pose and of the registered pose against the truth — in
metres and degrees — and the registration's status and the standard deviations its covariance gives.

    python examples/scan_registration_sample.py [--steps 8]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from closed_loop_exploration_sample import GEOMETRY  # noqa: E402
from scan_matching_sample import DRIFT, WINDOW, YAW, place, quat_yaw, sense, true_path, world_points, yaw_quat  # noqa: E402
from trajectory_optimization_amd import ops  # noqa: E402
from trajectory_optimization_amd.tools import evidence_map, match_scan, occupancy_grid, register_scan  # noqa: E402

DOF = "xyzw"          # the robot drives on a floor: roll and pitch stay the odometry's
MAX_MOVE = 1.5        # voxels a registration may move the matched pose; more is outside its basin and not taken


def pose_error(p, yaw, true_p, true_yaw):
    d = (yaw - true_yaw + np.pi) % (2.0 * np.pi) - np.pi
    return float(np.linalg.norm(np.asarray(p) - true_p)), float(abs(np.rad2deg(d)))


def run(steps=8, device="cuda:0", verbose=True):
    """-> dict(errors: per step ((m, deg) of the prior, of the matched pose, of the registered pose), statuses)."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    map = evidence_map(occupancy_grid(device=device, **GEOMETRY))
    matcher = ops.ScanMatcher(map)
    r = float(map.resolution)
    truth, yaws = true_path(steps)
    est_p, est_yaw = truth[0].copy(), float(yaws[0])
    errors, statuses = [], []
    for i in range(steps):
        odom_p = truth[i] + i * np.asarray(DRIFT["step"])
        odom_yaw = yaws[i] + i * DRIFT["yaw"]
        pts = sense(world, truth[i], yaws[i], device)
        if i > 0:
            prior_p = est_p + (odom_p - last_odom_p)
            prior_yaw = est_yaw + (odom_yaw - last_odom_yaw)
            m = match_scan(matcher.refresh(), pts, prior_p, yaw_quat(prior_yaw), window=WINDOW, yaw=YAW, refine=False)
            if m.ties == 1 and 2 * m.known >= m.used:
                match_p, match_yaw = m.pose.astype(np.float64), quat_yaw(m.quat)
            else:
                match_p, match_yaw = prior_p, prior_yaw
            reg = register_scan(matcher, pts, match_p, yaw_quat(match_yaw), dof=DOF)
            moved = np.abs(reg.pose - match_p).max() / r
            if reg.status in ("CONVERGED", "STALLED", "RUNNING") and moved <= MAX_MOVE:
                est_p, est_yaw = reg.pose, quat_yaw(reg.quat)
            else:
                est_p, est_yaw = match_p, match_yaw
            errors.append((pose_error(prior_p, prior_yaw, truth[i], yaws[i]), pose_error(match_p, match_yaw, truth[i], yaws[i]),
                           pose_error(est_p, est_yaw, truth[i], yaws[i])))
            statuses.append(reg.status)
            if verbose:
                sd = np.sqrt(np.diag(reg.covariance))
                (pe, pa), (me, ma), (re_, ra) = errors[-1]
                print(f"step {i}: {pts.shape[0]} returns  prior {pe:.3f} m {pa:.2f} deg  matched {me:.3f} m {ma:.2f} deg  registered {re_:.3f} m "
                      f"{ra:.2f} deg  [{reg.status} after {reg.iterations}, rms {reg.rms:.1f} byte, sd x {1e3 * sd[0]:.2f} y {1e3 * sd[1]:.2f} mm "
                      f"yaw {np.rad2deg(sd[5]):.3f} deg]")
        map.integrate(torch.as_tensor(est_p, dtype=torch.float32, device=device)[None, :], place(pts, est_p, est_yaw))
        last_odom_p, last_odom_yaw = odom_p, odom_yaw
    return dict(errors=errors, statuses=statuses)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map, the matcher and the registration have no CPU fallback")
    result = run(args.steps)
    e = np.asarray(result["errors"])
    print(f"mean error over {len(e)} steps: prior {e[:, 0, 0].mean():.3f} m {e[:, 0, 1].mean():.2f} deg, matched {e[:, 1, 0].mean():.3f} m "
          f"{e[:, 1, 1].mean():.2f} deg, registered {e[:, 2, 0].mean():.3f} m {e[:, 2, 1].mean():.2f} deg")
    return result


if __name__ == "__main__":
    main()
