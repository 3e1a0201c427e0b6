#!/usr/bin/env python3
"""Closed-loop exploration that prices the trip: examples/closed_loop_exploration_sample.py's world — the room and the hall behind its
wall x = 2 — but the wall has a SLIT one voxel wide instead of a doorway.  The sensor sees the hall through the slit, so lattice
positions in the hall become "known free"; the robot (radius 0.15 m) cannot pass it.

Every round: tools.depth_scan(world, four views all round, into=map); the clearance field of the map is rebuilt and a travel field
from the robot's position says which lattice positions it can reach and how far they are (tools.travel_field, tf.reachable);
propose_views takes only those; select_views_volume(..., travel=tf, travel_weight=w) maximises revealed voxels minus w voxels per
metre travelled; the robot moves along tools.travel_path.  Prints the metres travelled per round.  It never moves into the hall.

    python examples/travel_exploration_sample.py [--rounds 4] [--travel-weight 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from closed_loop_exploration_sample import GEOMETRY, HALL_X, SENSOR, START, all_round  # noqa: E402
from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import (clearance_field, depth_scan, known_free, occupancy_grid, propose_views,  # noqa: E402
                                                select_views_volume, space_map, travel_field, travel_path)

ROBOT_RADIUS = 0.15
SLIT_Y, SLIT_HALF_WIDTH = 1.0625, 0.0675   # metres: the slit spans the one voxel column y in [1, 1.125)


def world_points():
    """The closed room and the closed hall behind it; the shared wall x = 2 has a floor-to-ceiling slit one voxel wide."""
    room = synth.box_room(doorway=False)
    slit = (room[:, 0] > 1.99) & (np.abs(room[:, 1] - SLIT_Y) < SLIT_HALF_WIDTH) & (room[:, 2] > 0.05) & (room[:, 2] < 0.95)
    hall = synth.box_room(doorway=False) + np.float32([2.0, 0.0, 0.0])
    return np.concatenate([room[~slit], hall[hall[:, 0] > 2.0]]).astype(np.float32)


def explore(rounds=4, travel_weight=20.0, device="cuda:0", verbose=True):
    """-> per-round records: position, unknown (voxels of state 0 after the scan), known_free / reachable (lattice positions), gain
    and travel (metres to the chosen view; None when none was chosen)."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    robot = space_map(occupancy_grid(device=device, **GEOMETRY))
    lattice = torch.from_numpy(synth.roadmap_lattice([0.25, 0.25, 0.5], [3.75, 1.75, 0.5], 0.25)).to(device)
    K = torch.from_numpy(SENSOR["intrins"])
    cam = {k: v for k, v in SENSOR.items() if k != "intrins"}
    position, quat = np.float32(START), synth.Q_OPTICAL
    field = tf = None
    records = []
    for r in range(rounds):
        poses, quats = all_round(position, quat)
        depth_scan(world, torch.from_numpy(poses).to(device), torch.from_numpy(quats).to(device), into=robot, intrins=K, **cam)
        field = clearance_field(robot, 0.5) if field is None else field.rebuild()
        here = torch.from_numpy(position).to(device)
        tf = travel_field(field, here, ROBOT_RADIUS, space=robot) if tf is None else tf.rebuild(here)
        free, reach = known_free(robot, lattice), tf.reachable(lattice)
        rec = dict(position=[float(v) for v in position], unknown=robot.unknown().count(), known_free=int(free.sum()),
                   reachable=int(reach.sum()), gain=None, travel=None)
        records.append(rec)
        if verbose:
            print(f"round {r}: at ({position[0]:.2f}, {position[1]:.2f}, {position[2]:.2f})  {rec['unknown']} unknown voxels  "
                  f"{rec['known_free']} lattice positions known free, {rec['reachable']} reachable "
                  f"({int((free & (lattice[:, 0] > HALL_X)).sum())} known free in the hall)")
        frontier = robot.frontier()
        if frontier.n == 0 or not bool(reach.any()):
            break
        prop = propose_views(frontier.points, lattice[reach], n_per_position=2, sectors=32, max_views=64, K=K, **cam)
        if prop.n_views == 0:
            break
        sel = select_views_volume(robot, prop.poses, prop.quats, 1, travel=tf, travel_weight=travel_weight, intrins=K, **cam)
        if sel.n_selected == 0:
            break
        path = travel_path(tf, sel.poses[0])
        assert path.reachable and float(sel.poses[0, 0]) < HALL_X, "the chosen view must be one the robot can reach"
        rec["gain"], rec["travel"] = int(sel.gains[0]), float(sel.travel[0])
        position, quat = sel.poses[0].cpu().numpy(), sel.quats[0].cpu().numpy()
        if verbose:
            print(f"         next: view {int(sel.order[0])} of {prop.n_views} proposals promises {rec['gain']} unknown voxels, "
                  f"{rec['travel']:.2f} m away over {path.poses.shape[0]} voxels")
    return records


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--travel-weight", type=float, default=20.0)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the planning chain have no CPU fallback")
    records = explore(args.rounds, args.travel_weight)
    print("metres travelled per round:", [None if r["travel"] is None else round(r["travel"], 3) for r in records])
    return records


if __name__ == "__main__":
    main()
