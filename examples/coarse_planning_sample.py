#!/usr/bin/env python3
"""Plan on a coarse level of a map kept at a fine resolution, and fold a second robot's finer map into a coarse team map.

The room is that of examples/closed_loop_exploration_sample.py.  Robot A takes two all-round scans into an evidence map at the fine
resolution.  tools.map_pyramid keeps that map at four scales; each level is the one before it at twice the voxel edge under the rule
'cover' — occupied if a child is occupied, else unknown if a child is unknown, else free — so a coarse level never loses a wall and
never calls anything free that is not.

A route is planned on level 1, at an eighth of the voxels: tools.clearance_field, tools.travel_field and tools.travel_path run over
the coarse map exactly as over any map.  The legs of that route are then put to the clearance field of the FINE map
(tools.edge_clearance): every one of them keeps the robot's radius there too, which is what 'cover' promises (DESIGN.md 10,
"Coarsening maps").

Robot B maps the hall behind the doorway at the fine resolution, in a box of its own on the same fine lattice.  The team map is A's
map at twice the voxel edge (anchor='world': its lattice is the world's); B's fine map goes into it with merge_fine, which reduces
2 x 2 x 2 of B's voxels per team voxel and fuses the result as merge does.

    python examples/coarse_planning_sample.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from closed_loop_exploration_sample import GEOMETRY, SENSOR, START, all_round, world_points  # noqa: E402
from scan_matching_sample import yaw_quat  # noqa: E402
from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import (clearance_field, coarsen_map, depth_scan, edge_clearance, evidence_map, map_pyramid,  # noqa: E402
                                               occupancy_grid, travel_field, travel_path)

SMALL = dict(GEOMETRY)                                                                   # the room at 0.125 m: the test's size
FINE = dict(origin=GEOMETRY["origin"], dims=tuple(2 * n for n in GEOMETRY["dims"]), resolution=GEOMETRY["resolution"] / 2)
A_STANDS = ((START, 0.0), ((0.6, 1.4, 0.52), 1.0))                                       # where A scans from: (position, yaw)
B_STANDS = (((3.0, 1.0, 0.52), 0.5),)                                                    # B stands in the hall
B_BOX = (17, 3, 1)                                                                       # B's box starts this many fine voxels into A's
GOAL = (0.5, 1.5, 0.52)
RADIUS, MAX_DIST, LEVELS, PLAN_LEVEL = 0.1, 0.5, 3, 1


def scan_into(map, truth, position, yaw, device):
    """One all-round scan of the ground truth `truth` from (position, yaw) folded into `map`."""
    poses, quats = all_round(position, synth.quat_mul(yaw_quat(yaw), synth.Q_OPTICAL))
    cam = {k: v for k, v in SENSOR.items() if k != "intrins"}
    depth_scan(truth, torch.from_numpy(poses).to(device), torch.from_numpy(quats).to(device), into=map, intrins=torch.from_numpy(SENSOR["intrins"]), **cam)


def known(map):
    return int((map.dense() != synth.EVID_UNKNOWN).sum())


def run(device="cuda:0", verbose=True, small=False):
    """-> dict(levels, level_dims, level_known; reachable, path_rows, path_length, fine_legs_clear; coarse_known, merged_known,
    newly_known, team_dims)."""
    device = torch.device(device)
    geometry = SMALL if small else FINE
    world = occupancy_grid(device=device, **geometry)
    world.insert(torch.from_numpy(world_points()).to(device))
    map_a = evidence_map(world)
    for position, yaw in A_STANDS:
        scan_into(map_a, world, position, yaw, device)

    # the map at four scales, and a route on level 1
    pyramid = map_pyramid(map_a, LEVELS)
    coarse = pyramid[PLAN_LEVEL]
    field = clearance_field(coarse.space, MAX_DIST)
    tf = travel_field(field, torch.tensor(START, dtype=torch.float32, device=device), RADIUS)
    path = travel_path(tf, GOAL)
    fine_field = clearance_field(map_a.space, MAX_DIST)
    if path.poses.shape[0] >= 2:
        _, idx, _ = edge_clearance(fine_field, path.poses[:-1], path.poses[1:], RADIUS)
        fine_clear = bool((idx == -1).all())
    else:
        fine_clear = False

    # B's finer map of the hall, in its own box of the fine lattice, folded into the team map at twice the voxel edge
    b_dims = tuple(n - s for n, s in zip(geometry["dims"], B_BOX))
    world_b = world.reframed(shift=B_BOX, dims=b_dims)
    map_b = evidence_map(world_b)
    for position, yaw in B_STANDS:
        scan_into(map_b, world_b, position, yaw, device)
    team = coarsen_map(map_a, 2, anchor="world")
    coarse_known = known(team)
    team.merge_fine(map_b, mode="confident")
    newly = team.last_counts()[1]

    result = dict(levels=LEVELS, level_dims=[tuple(m.dims) for m in pyramid], level_known=[known(m) for m in pyramid], reachable=bool(path.reachable),
                  path_rows=int(path.poses.shape[0]), path_length=float(path.length), fine_legs_clear=fine_clear, coarse_known=coarse_known,
                  merged_known=known(team), newly_known=int(newly), team_dims=tuple(team.dims))
    if verbose:
        for l, m in enumerate(pyramid):
            print(f"level {l}: {tuple(m.dims)} voxels of {m.resolution:g} m, {result['level_known'][l]} known, {m.occupied.count()} occupied")
        print(f"route on level {PLAN_LEVEL}: {'reachable' if path.reachable else 'NOT reachable'}, {result['path_rows']} rows, {path.length:.2f} m; "
              f"its legs keep {RADIUS} m in the fine map's field: {fine_clear}")
        print(f"team map {result['team_dims']}: {coarse_known} known voxels from A, {result['merged_known']} after B's fine map ({newly} newly known)")
    return result


def main():
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the maps have no CPU fallback")
    return run()


if __name__ == "__main__":
    main()
