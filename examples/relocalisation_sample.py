#!/usr/bin/env python3
"""A robot is switched on somewhere in a map it already has.

The map is that of examples/closed_loop_exploration_sample.py — the doorway room and the hall behind it — known from an earlier
survey: an evidence map that holds lmax in the occupied voxels and lmin in the rest.  The robot stands in the room, but the pose it
believes in is 20 voxels (2.5 m, in the hall) and 30 degrees off.  One all-round scan, taken by tools.depth_scan against the ground
truth at the TRUE pose and handed over in the sensor frame, is all it has.

tools.relocalise_scan searches the whole map — every voxel shift in x and y that keeps the prior inside it, 17 headings over +-40
degrees — by branch and bound, and names the exhaustive search's winner after bounding a small fraction of its candidates;
tools.match_scan then refines the pose around it with finer headings.  Printed: the errors of the prior, the relocalised and the
refined pose, and how many nodes each level of the search held.

    python examples/relocalisation_sample.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from closed_loop_exploration_sample import GEOMETRY, START, world_points  # noqa: E402
from scan_matching_sample import quat_yaw, sense, yaw_quat  # noqa: E402
from trajectory_optimization_amd import ops  # noqa: E402
from trajectory_optimization_amd.tools import evidence_map, match_scan, occupancy_grid, relocalise_scan  # noqa: E402

TRUE_YAW = 0.4
PRIOR_OFF = dict(voxels=(20, -3, 0), yaw=np.deg2rad(30.0))   # what the believed pose is off by
HEADINGS = (np.deg2rad(40.0), 17)                            # the search's candidate headings: +-40 degrees in steps of 5
FINE = dict(window=(2, 2, 1), yaw=(np.deg2rad(4.0), 9))      # the refinement around the relocalised pose


def known_map(world, device):
    """The survey's map: lmax where the ground truth is occupied, lmin elsewhere."""
    m = evidence_map(occupancy_grid(device=device, **GEOMETRY))
    _, _, lmin, lmax, _ = m.params
    occ = world.dense()
    return m.load(torch.where(occ, torch.full_like(occ, lmax, dtype=torch.int64), torch.full_like(occ, lmin, dtype=torch.int64)))


def run(device="cuda:0", verbose=True):
    """-> dict(prior_error, relocalised_error, refined_error in metres; shift, rotation, ties, levels, nodes, evaluated, candidates)."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    matcher = ops.ScanMatcher(known_map(world, device))
    truth = np.asarray(START, dtype=np.float64)
    pts = sense(world, truth, TRUE_YAW, device)
    prior_p = truth + GEOMETRY["resolution"] * np.asarray(PRIOR_OFF["voxels"], dtype=np.float64)
    prior_yaw = TRUE_YAW + PRIOR_OFF["yaw"]
    found = relocalise_scan(matcher, pts, prior_p, yaw_quat(prior_yaw), yaw=HEADINGS)
    fine = match_scan(matcher, pts, found.pose, found.quat, **FINE)
    result = dict(prior_error=float(np.linalg.norm(prior_p - truth)), relocalised_error=float(np.linalg.norm(found.pose - truth)),
                  refined_error=float(np.linalg.norm(fine.pose_refined - truth)), shift=found.shift, rotation=found.rotation, ties=found.ties,
                  levels=found.levels, nodes=found.nodes, evaluated=found.evaluated, candidates=found.candidates,
                  yaw_error=float(abs(quat_yaw(fine.quat) - TRUE_YAW)))
    if verbose:
        print(f"{pts.shape[0]} returns; the prior is off by {result['prior_error']:.2f} m and {np.rad2deg(PRIOR_OFF['yaw']):.0f} degrees")
        print(f"relocalised: shift {found.shift}, heading {found.rotation} of {HEADINGS[1]}, score {found.score}, ties {found.ties}: off by "
              f"{result['relocalised_error']:.3f} m")
        print(f"  {found.levels} levels held {found.nodes[::-1]} nodes (top first); {found.evaluated} bounds for {found.candidates} candidates")
        print(f"refined by match_scan: off by {result['refined_error']:.3f} m and {np.rad2deg(result['yaw_error']):.2f} degrees")
    return result


def main():
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the matcher have no CPU fallback")
    return run()


if __name__ == "__main__":
    main()
