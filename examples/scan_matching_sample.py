#!/usr/bin/env python3
"""Mapping with odometry that drifts, with and without scan matching.

A robot circles the room of examples/closed_loop_exploration_sample.py (the doorway room and the hall behind it, hidden in a
ground-truth grid) and scans all round at every step.  Its odometry drifts: every step adds a few centimetres and most of a degree
of error, so the pose it believes in walks away from the truth.  The scans come from tools.depth_scan against the ground truth at
the TRUE pose and are handed over in the sensor frame, as a real sensor hands them over.

Two evidence maps are built from the same scans: one places each scan at the raw odometry pose; the other first asks
tools.match_scan where the scan fits the map built so far — the prior is the last matched pose moved by the odometry's increment —
and places it there.  Printed: for both maps the number of voxels whose occupied bit disagrees with the ground truth.

    python examples/scan_matching_sample.py [--steps 8]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from closed_loop_exploration_sample import GEOMETRY, SENSOR, all_round, world_points  # noqa: E402
from trajectory_optimization_amd import ops, synth  # noqa: E402
from trajectory_optimization_amd.tools import depth_scan, evidence_map, match_scan, occupancy_grid  # noqa: E402

CENTRE, RADIUS, HEIGHT = (1.0, 1.0), 0.45, 0.52
DRIFT = dict(step=(0.05, -0.03, 0.0), yaw=np.deg2rad(0.7))   # the odometry's error per step, accumulating
WINDOW, YAW = (3, 3, 1), (np.deg2rad(2.1), 7)                # what the matcher searches around each prior


def yaw_quat(a):
    return np.array([np.cos(0.5 * a), 0.0, 0.0, np.sin(0.5 * a)], dtype=np.float64)


def quat_yaw(q):
    return 2.0 * np.arctan2(q[3], q[0])


def true_path(steps):
    """The robot's true poses on a circle -> (positions (steps,3), yaws (steps,)): heading along the tangent."""
    a = np.linspace(0.0, 1.5 * np.pi, steps)
    pos = np.stack([CENTRE[0] + RADIUS * np.cos(a), CENTRE[1] + RADIUS * np.sin(a), np.full(steps, HEIGHT)], axis=1)
    return pos, a + 0.5 * np.pi


def sense(world, position, yaw, device):
    """One all-round scan at the true pose -> the returns in the SENSOR frame, (N,3) f32 on the device."""
    poses, quats = all_round(position, synth.quat_mul(yaw_quat(yaw), synth.Q_OPTICAL))
    cam = {k: v for k, v in SENSOR.items() if k != "intrins"}
    scan = depth_scan(world, torch.from_numpy(poses).to(device), torch.from_numpy(quats).to(device), points=True,
                      intrins=torch.from_numpy(SENSOR["intrins"]), **cam)
    hits = scan.points[scan.flags == 0].double()
    R = torch.from_numpy(synth.scan_rotation(yaw_quat(yaw)).astype(np.float64)).to(device)
    return ((hits - torch.as_tensor(position, dtype=torch.float64, device=device)) @ R).float()


def place(points, position, yaw):
    """Sensor-frame points at a believed pose -> world points, f32 on the points' device."""
    R = torch.from_numpy(synth.scan_rotation(yaw_quat(yaw))).to(points.device)
    return points @ R.T + torch.as_tensor(np.asarray(position, dtype=np.float32), device=points.device)


def disagreement(map, world):
    return int((map.occupied.dense() != world.dense()).sum())


def run(steps=8, device="cuda:0", verbose=True):
    """-> dict(raw, matched: voxels whose occupied bit disagrees with the ground truth; errors: per step the distance in metres of
    the odometry pose and of the matched pose from the truth)."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    raw, matched = (evidence_map(occupancy_grid(device=device, **GEOMETRY)) for _ in range(2))
    matcher = ops.ScanMatcher(matched)
    truth, yaws = true_path(steps)
    est_p, est_yaw = truth[0].copy(), float(yaws[0])
    errors = []
    for i in range(steps):
        odom_p = truth[i] + i * np.asarray(DRIFT["step"])
        odom_yaw = yaws[i] + i * DRIFT["yaw"]
        pts = sense(world, truth[i], yaws[i], device)
        raw.integrate(torch.as_tensor(odom_p, dtype=torch.float32, device=device)[None, :], place(pts, odom_p, odom_yaw))
        if i > 0:
            # the prior: the last matched pose moved by what the odometry says happened since
            prior_p = est_p + (odom_p - last_odom_p)
            prior_yaw = est_yaw + (odom_yaw - last_odom_yaw)
            m = match_scan(matcher.refresh(), pts, prior_p, yaw_quat(prior_yaw), window=WINDOW, yaw=YAW)
            if m.ties == 1 and 2 * m.known >= m.used:
                est_p, est_yaw = m.pose_refined, quat_yaw(m.quat)
            else:
                est_p, est_yaw = prior_p, prior_yaw
        matched.integrate(torch.as_tensor(est_p, dtype=torch.float32, device=device)[None, :], place(pts, est_p, est_yaw))
        last_odom_p, last_odom_yaw = odom_p, odom_yaw
        errors.append((float(np.linalg.norm(odom_p - truth[i])), float(np.linalg.norm(est_p - truth[i]))))
        if verbose:
            print(f"step {i}: {pts.shape[0]} returns  odometry off by {errors[-1][0]:.3f} m  matched pose off by {errors[-1][1]:.3f} m")
    return dict(raw=disagreement(raw, world), matched=disagreement(matched, world), errors=errors)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the matcher have no CPU fallback")
    result = run(args.steps)
    print(f"occupied voxels that disagree with the ground truth: {result['raw']} with raw odometry, {result['matched']} with scan matching")
    return result


if __name__ == "__main__":
    main()
