#!/usr/bin/env python3
"""Frontier-based exploration with goals taken from the openings themselves: examples/travel_exploration_sample.py's world — the room
and the hall behind its wall x = 2, joined by a SLIT one voxel wide that the sensor sees through and the robot (radius 0.15 m) cannot
pass — plus a few stray rays that leaked through the ceiling and each left one free voxel in never-scanned space.

Every round: tools.depth_scan(world, four views all round, into=map), and the space the robot's own body fills is marked free; the
clearance field and the travel field from the robot's position are rebuilt; tools.frontier_clusters(map, travel=tf) groups the frontier voxels into connected openings and prices each by
its nearest voxel.  The round prints every cluster with its size, cost and reachability, shows that min_size drops exactly the
one-voxel clusters the stray rays made, checks that the clusters on the hall's side stay unreachable, and moves the robot to the
`approach` of the nearest reachable cluster it does not already stand in, along tools.travel_path.

    python examples/frontier_cluster_sample.py [--rounds 4] [--min-size 4]
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
from travel_exploration_sample import ROBOT_RADIUS, world_points  # noqa: E402
from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import (clearance_field, depth_scan, frontier_clusters, occupancy_grid, space_map,  # noqa: E402
                                                travel_field, travel_path)

# three stray rays: each starts above the ceiling (z = 1.3, never scanned) and ends in the next voxel, so it frees exactly one voxel
STRAYS = np.float32([[0.55, 0.45, 1.3], [1.3, 1.55, 1.3], [3.05, 0.95, 1.3]])


def body_points(position, n=200):
    """n points on the sphere of twice the robot's radius around `position` (a Fibonacci lattice): rays to them, truncated at the
    robot's radius, mark the space the robot's own body fills as free — the sensor's cone starts outside it."""
    k = np.arange(n) + 0.5
    phi, z = np.pi * (1.0 + 5.0 ** 0.5) * k, 1.0 - 2.0 * k / n
    rho = np.sqrt(1.0 - z * z)
    return (np.float32(position) + 2.0 * ROBOT_RADIUS * np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)).astype(np.float32)


def explore(rounds=4, min_size=4, device="cuda:0", verbose=True):
    """-> per-round records: position, clusters (all), kept (size >= min_size), singletons, reachable (of the kept), goal, cost."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    robot = space_map(occupancy_grid(device=device, **GEOMETRY))
    strays = torch.from_numpy(STRAYS).to(device)
    robot.free.carve(strays, strays + torch.tensor([GEOMETRY["resolution"], 0.0, 0.0], device=device))
    K = torch.from_numpy(SENSOR["intrins"])
    cam = {k: v for k, v in SENSOR.items() if k != "intrins"}
    position, quat = np.float32(START), synth.Q_OPTICAL
    field = tf = None
    records = []
    for r in range(rounds):
        poses, quats = all_round(position, quat)
        depth_scan(world, torch.from_numpy(poses).to(device), torch.from_numpy(quats).to(device), into=robot, intrins=K, **cam)
        robot.free.carve(torch.from_numpy(position).to(device), torch.from_numpy(body_points(position)).to(device), max_range=ROBOT_RADIUS)
        field = clearance_field(robot, 0.5) if field is None else field.rebuild()     # unknown='free': a frontier voxel can be a goal
        here = torch.from_numpy(position).to(device)
        tf = travel_field(field, here, ROBOT_RADIUS, space=robot) if tf is None else tf.rebuild(here)
        every = frontier_clusters(robot, travel=tf)
        kept = frontier_clusters(robot, min_size=min_size, travel=tf)
        singles = int((every.sizes == 1).sum())
        hall = kept.centroids[:, 0] > HALL_X
        rec = dict(position=[float(v) for v in position], clusters=every.n, kept=kept.n, singletons=singles,
                   reachable=int(kept.reachable.sum()), hall=int(hall.sum()), goal=None, cost=None)
        records.append(rec)
        if verbose:
            print(f"round {r}: at ({position[0]:.2f}, {position[1]:.2f}, {position[2]:.2f})  {every.frontier.n} frontier voxels in "
                  f"{every.n} clusters; min_size={min_size} keeps {kept.n} and drops {every.n - kept.n} ({singles} of one voxel)")
            for i in range(kept.n):
                c = kept.centroids[i].tolist()
                where = "hall" if bool(hall[i]) else "room"
                cost = f"{float(kept.cost[i]):.2f} m" if bool(kept.reachable[i]) else "unreachable"
                print(f"         cluster {int(kept.ids[i]):3d}: {int(kept.sizes[i]):4d} voxels around ({c[0]:.2f}, {c[1]:.2f}, {c[2]:.2f}) [{where}]  {cost}")
        assert every.n - kept.n >= len(STRAYS) and singles >= len(STRAYS), "the stray rays' one-voxel clusters fall to min_size"
        assert not bool(kept.reachable[hall].any()), "a cluster on the hall's side must stay unreachable: the slit is narrower than the robot"
        # the rows come nearest first: the goal is the first reachable opening the robot does not already stand in.  What the four
        # views leave unknown inside the room are the cones above and below the sensor's field of view: the robot moves to where
        # the nearest of them begins and looks again from there
        away = torch.nonzero(kept.reachable & (kept.cost > 0.0)).reshape(-1)
        if away.numel() == 0:
            if verbose:
                print("         no reachable opening is left to go to: what remains unknown lies behind the slit")
            break
        k = int(away[0])
        goal = kept.approach[k]
        path = travel_path(tf, goal)
        assert path.reachable and float(goal[0]) < HALL_X and abs(path.length - float(kept.cost[k])) < 1e-4
        rec["goal"], rec["cost"] = goal.tolist(), float(kept.cost[k])
        if verbose:
            print(f"         goal: the approach voxel of cluster {int(kept.ids[k])} at ({goal[0]:.2f}, {goal[1]:.2f}, {goal[2]:.2f}), "
                  f"{rec['cost']:.2f} m away over {path.poses.shape[0]} voxels")
        position = goal.cpu().numpy()
    return records


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--min-size", type=int, default=4)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the planning chain have no CPU fallback")
    records = explore(args.rounds, args.min_size)
    print("goals per round:", [None if r["goal"] is None else [round(v, 2) for v in r["goal"]] for r in records])
    return records


if __name__ == "__main__":
    main()
