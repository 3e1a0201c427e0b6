#!/usr/bin/env python3
"""Close a loop: two laps of the small room, the second one on drifting odometry, then a pose graph puts the trajectory and the map right.

The robot, the room and the sensor are those of examples/scan_matching_sample.py (tools.depth_scan is the sensor).

Lap 1.  Every scan is placed by match -> register against the map so far (tools.match_scan, tools.register_scan) and integrated: the
        front end of examples/scan_registration_sample.py.  The first lap's map is kept.
Lap 2.  The front end has lost its lock (as after a long corridor with nothing to match): the robot dead-reckons on its biased
        odometry and integrates every scan where the odometry says it is.  The walls stand twice in the map.
Close.  tools.relocalise_scan places every few scans of the second lap in the FIRST lap's map, tools.register_scan refines the
        answer, and PoseGraph.add_registration turns it into an edge with the registration's own information matrix.
Graph.  One node per scan; consecutive nodes are joined by what was measured between them (PoseGraph.relative of the registered poses
        on lap 1, the odometry's increments on lap 2); node 0 is fixed.  PoseGraph.optimize runs on the device.
Map.    The evidence map is rebuilt from the corrected poses with EvidenceMap.integrate.

Printed: the trajectory's mean error against the truth before and after the optimisation, and the occupied voxels of both maps:
doubled walls merge, so the count falls.

    python examples/loop_closure_sample.py [--scans 12]
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
from scan_matching_sample import CENTRE, HEIGHT, RADIUS, WINDOW, YAW, place, quat_yaw, sense, world_points, yaw_quat  # noqa: E402
from trajectory_optimization_amd import ops  # noqa: E402
from trajectory_optimization_amd.tools import evidence_map, match_scan, occupancy_grid, register_scan, relocalise_scan  # noqa: E402

DOF = "xyzw"                                            # the robot drives on a floor: roll and pitch stay the odometry's
BIAS = dict(step=(0.025, -0.015, 0.0), yaw=np.deg2rad(0.5))   # the odometry's error per step, accumulating
HEADINGS = (np.deg2rad(12.0), 13)                       # relocalisation's candidate headings: +-12 degrees in steps of 2
EVERY = 3                                               # every third scan of the second lap is relocalised
ODOMETRY_SIGMA = (0.05, 0.02)                           # metres and radians: what an odometry edge is trusted to


def two_laps(scans):
    """The true poses -> (positions (2 scans, 3), yaws): twice round the circle, heading along the tangent."""
    a = 2.0 * np.pi * np.arange(2 * scans) / scans
    pos = np.stack([CENTRE[0] + RADIUS * np.cos(a), CENTRE[1] + RADIUS * np.sin(a), np.full(2 * scans, HEIGHT)], axis=1)
    return pos, a + 0.5 * np.pi


def diag_information(sigma_t, sigma_r):
    return np.diag([1.0 / sigma_t ** 2] * 3 + [1.0 / sigma_r ** 2] * 3)


def build_map(device, positions, yaws, scans):
    m = evidence_map(occupancy_grid(device=device, **GEOMETRY))
    for p, yaw, pts in zip(positions, yaws, scans):
        m.integrate(torch.as_tensor(np.asarray(p), dtype=torch.float32, device=device)[None, :], place(pts, p, yaw))
    return m


def run(scans=12, device="cuda:0", verbose=True):
    """-> dict(error_before, error_after: the mean distance of the 2 `scans` poses from the truth in metres; occupied_before,
    occupied_after: occupied voxels of the map as driven and of the map rebuilt; closures, result: the PoseGraphResult)."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    truth, yaws = two_laps(scans)
    n = 2 * scans
    odom_p = truth + np.arange(n)[:, None] * np.asarray(BIAS["step"])
    odom_yaw = yaws + np.arange(n) * BIAS["yaw"]
    clouds = [sense(world, truth[i], yaws[i], device) for i in range(n)]

    # ---- lap 1: match -> register -> integrate
    first = evidence_map(occupancy_grid(device=device, **GEOMETRY))
    matcher = ops.ScanMatcher(first)
    est_p, est_yaw = [truth[0].copy()], [float(yaws[0])]
    first.integrate(torch.as_tensor(est_p[0], dtype=torch.float32, device=device)[None, :], place(clouds[0], est_p[0], est_yaw[0]))
    for i in range(1, scans):
        prior_p = est_p[-1] + (odom_p[i] - odom_p[i - 1])
        prior_yaw = est_yaw[-1] + (odom_yaw[i] - odom_yaw[i - 1])
        m = match_scan(matcher.refresh(), clouds[i], prior_p, yaw_quat(prior_yaw), window=WINDOW, yaw=YAW, refine=False)
        p, yaw = (m.pose.astype(np.float64), quat_yaw(m.quat)) if m.ties == 1 and 2 * m.known >= m.used else (prior_p, prior_yaw)
        reg = register_scan(matcher, clouds[i], p, yaw_quat(yaw), dof=DOF)
        if reg.status in ("CONVERGED", "STALLED", "RUNNING") and np.abs(reg.pose - p).max() <= 1.5 * first.resolution:
            p, yaw = reg.pose, quat_yaw(reg.quat)
        est_p.append(np.asarray(p, dtype=np.float64))
        est_yaw.append(float(yaw))
        first.integrate(torch.as_tensor(est_p[-1], dtype=torch.float32, device=device)[None, :], place(clouds[i], est_p[-1], est_yaw[-1]))
    matcher.refresh()

    # ---- lap 2: dead reckoning from the last good pose
    for i in range(scans, n):
        est_p.append(est_p[-1] + (odom_p[i] - odom_p[i - 1]))
        est_yaw.append(est_yaw[-1] + (odom_yaw[i] - odom_yaw[i - 1]))
    est_p, est_yaw = np.asarray(est_p), np.asarray(est_yaw)
    driven = build_map(device, est_p, est_yaw, clouds)

    # ---- the graph: odometry edges, then a registration against the first lap's map for every few scans of the second
    quats = np.stack([yaw_quat(a) for a in est_yaw])
    graph = ops.PoseGraph(est_p, quats, fixed=[0], device=device)
    for i in range(n - 1):
        tight = i + 1 < scans                                           # (lap 1: between registered poses)
        info = diag_information(*(s / 10.0 for s in ODOMETRY_SIGMA)) if tight else diag_information(*ODOMETRY_SIGMA)
        graph.add_edges([i], [i + 1], *graph.relative(i, i + 1), info)
    closures = []
    for j in range(scans, n, EVERY):
        found = relocalise_scan(matcher, clouds[j], est_p[j], quats[j], yaw=HEADINGS)
        reg = register_scan(matcher, clouds[j], found.pose, found.quat, dof=DOF)
        if found.ties == 1 and reg.status in ("CONVERGED", "STALLED", "RUNNING"):
            graph.add_registration(j, reg)
            closures.append(j)
            if verbose:
                print(f"scan {j}: believed {np.linalg.norm(est_p[j] - truth[j]):.3f} m off, relocalised and registered "
                      f"{np.linalg.norm(reg.pose - truth[j]):.3f} m off [{reg.status}]")
    # (no robust= here: a registration's information is so large that, from a start 0.3 m off, Geman-McClure would silence every
    # closure alike; the guard against a wrong one is `ties == 1` above)
    result = graph.optimize(dof=DOF)

    # ---- the map again, from the corrected poses
    new_yaw = np.asarray([quat_yaw(q) for q in result.quats])
    rebuilt = build_map(device, result.poses, new_yaw, clouds)
    error = lambda p: float(np.linalg.norm(np.asarray(p) - truth, axis=1).mean())   # noqa: E731
    out = dict(error_before=error(est_p), error_after=error(result.poses), occupied_before=int(driven.occupied.dense().sum()),
               occupied_after=int(rebuilt.occupied.dense().sum()), closures=closures, result=result)
    if verbose:
        print(f"pose graph: {n} nodes, {graph.n_edges} edges, {len(closures)} closures: {result.status} after {result.iterations} iterations, "
              f"{result.cg_iterations} CG iterations, cost {result.initial_cost:.4g} -> {result.cost:.4g}")
        print(f"mean trajectory error: {out['error_before']:.3f} m before, {out['error_after']:.3f} m after")
        print(f"occupied voxels: {out['occupied_before']} as driven, {out['occupied_after']} rebuilt from the corrected poses")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=12, help="scans per lap")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map, the matcher and the optimiser have no CPU fallback")
    return run(args.scans)


if __name__ == "__main__":
    main()
