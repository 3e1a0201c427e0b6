#!/usr/bin/env python3
"""Closed-loop next-best-view exploration: the chain of examples/volume_exploration_sample.py run round after round, because the scan
at the pose the robot just chose is no longer written by hand — a depth sensor is simulated against a hidden ground-truth grid.

The WORLD is an occupancy grid the planner never reads: the doorway room (synth.box_room, a 2 x 2 x 1 m box with a doorway in the
wall x = 2) plus a closed hall of the same size behind that wall.  The robot's MAP is an empty ops.SpaceMap of the same geometry.
Every round: tools.depth_scan(world, four views all round the current position, into=map) marks what the sensor hits and passes;
the frontier of the map and the lattice positions known to be free give tools.propose_views its candidates; tools.select_views_volume
chooses the one view that reveals the most unknown voxels; the robot moves there.  Prints the unknown count per round.

    python examples/closed_loop_exploration_sample.py [--rounds 4]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import depth_scan, known_free, occupancy_grid, propose_views, select_views_volume, space_map  # noqa: E402

GEOMETRY = dict(origin=(-0.5, -0.5, -0.5), dims=(40, 24, 16), resolution=0.125)   # the room and the hall, half a metre around them
START = (1.03, 0.97, 0.52)
# a 64 x 48 sensor with a 90 degree horizontal field of view: four views 90 degrees apart look all round
SENSOR = dict(intrins=np.float32([[32.0, 0.0, 31.5], [0.0, 32.0, 23.5], [0.0, 0.0, 1.0]]), img_width=64, img_height=48, min_dist=0.05, max_dist=4.0)
HALL_X = 2.25   # voxel centres beyond this lie in the hall


def world_points():
    """The room with its doorway and the hall behind it: the hall is the closed box moved 2 m along x, without its face x = 2 (the
    room's wall, doorway included, stands there)."""
    hall = synth.box_room(doorway=False) + np.float32([2.0, 0.0, 0.0])
    return np.concatenate([synth.box_room(doorway=True), hall[hall[:, 0] > 2.0]]).astype(np.float32)


def all_round(position, quat):
    """Four views from `position`: `quat` and its three rotations by 90 degrees about +z -> (poses (4,3), quats (4,4)) f32."""
    turns = [[np.cos(a / 2.0), 0.0, 0.0, np.sin(a / 2.0)] for a in np.deg2rad([0.0, 90.0, 180.0, 270.0])]
    return np.tile(np.float32(position), (4, 1)), synth.quat_mul(np.array(turns), np.asarray(quat, dtype=np.float64)).astype(np.float32)


def explore(rounds=4, device="cuda:0", verbose=True, on_round=None):
    """-> (per-round records, the world grid, the robot's map).  A record: unknown (voxels of state 0 after the round's scan),
    returns (pixels with a return), position (where the scan was taken), gain (what the chosen next view promised, None when none
    was chosen).  on_round(r, world, robot) is called behind every round's scan."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    robot = space_map(occupancy_grid(device=device, **GEOMETRY))
    lattice = torch.from_numpy(synth.roadmap_lattice([0.25, 0.25, 0.5], [3.75, 1.75, 0.5], 0.25)).to(device)
    K = torch.from_numpy(SENSOR["intrins"])
    cam = {k: v for k, v in SENSOR.items() if k != "intrins"}
    position, quat = np.float32(START), synth.Q_OPTICAL
    records = []
    for r in range(rounds):
        poses, quats = all_round(position, quat)
        scan = depth_scan(world, torch.from_numpy(poses).to(device), torch.from_numpy(quats).to(device), into=robot, intrins=K, **cam)
        rec = dict(unknown=robot.unknown().count(), returns=int((scan.flags == 0).sum()), position=[float(v) for v in position], gain=None)
        records.append(rec)
        if on_round is not None:
            on_round(r, world, robot)
        frontier = robot.frontier()
        if verbose:
            print(f"round {r}: at ({position[0]:.2f}, {position[1]:.2f}, {position[2]:.2f})  {rec['returns']} returns  "
                  f"{robot.occupied.count()} occupied voxels  {frontier.n} frontier voxels  {rec['unknown']} unknown voxels")
        if frontier.n == 0:
            break
        free = known_free(robot, lattice)
        if not bool(free.any()):
            break
        prop = propose_views(frontier.points, lattice[free], n_per_position=2, sectors=32, max_views=64, K=K, **cam)
        if prop.n_views == 0:
            break
        sel = select_views_volume(robot, prop.poses, prop.quats, 1, intrins=K, **cam)
        if sel.n_selected == 0:
            break
        rec["gain"] = int(sel.gains[0])
        position, quat = sel.poses[0].cpu().numpy(), sel.quats[0].cpu().numpy()
        if verbose:
            print(f"         next: view {int(sel.order[0])} of {prop.n_views} proposals promises {rec['gain']} unknown voxels")
    return records, world, robot


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the planning chain have no CPU fallback")
    records, _, _ = explore(args.rounds)
    print("unknown voxels per round:", [r["unknown"] for r in records])
    return records


if __name__ == "__main__":
    main()
