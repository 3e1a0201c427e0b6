#!/usr/bin/env python3
"""A team divides the openings of one map: examples/frontier_cluster_sample.py's world — the room and the hall behind its wall,
joined by a slit the sensor sees through and the robot cannot pass — explored by TWO robots that start in the same room.

Every round: each robot scans into its own map (tools.depth_scan, four views all round; the space its body fills is marked free),
tools.merge_maps fuses the two maps, the clearance field of the merged map is built, tools.travel_fields builds one travel field per
robot in the same worklist rounds, and tools.assign_frontiers hands the frontier clusters out: the cheapest (robot, opening) pair
first, no robot and no opening twice, min_cost just above 0 so that no robot is sent to the opening it stands in.  The round checks
that the two goals are different clusters, that neither lies behind the slit, and that each robot's tools.travel_path(fields[b],
goal) has exactly the assigned cost; then both robots move.  At the end tools.plan_tour(field, views, travel=True) orders the four
places the robots have stood in — all in the room — by what a robot must travel over the map.

    python examples/team_frontier_sample.py [--rounds 3] [--min-size 4]
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
from frontier_cluster_sample import body_points  # noqa: E402
from travel_exploration_sample import ROBOT_RADIUS, world_points  # noqa: E402
from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import (assign_frontiers, clearance_field, depth_scan, merge_maps, occupancy_grid, plan_tour,  # noqa: E402
                                                space_map, travel_fields, travel_path)

STARTS = np.float32([START, (0.53, 1.47, 0.52)])        # both in the room


def explore(rounds=3, min_size=4, device="cuda:0", verbose=True):
    """-> (per-round records: positions, clusters, goals (rows of the clusters, -1 none), costs in metres; the tour)."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    own = [space_map(occupancy_grid(device=device, **GEOMETRY)) for _ in STARTS]
    K = torch.from_numpy(SENSOR["intrins"])
    cam = {k: v for k, v in SENSOR.items() if k != "intrins"}
    positions, quat = STARTS.copy(), synth.Q_OPTICAL
    records, field, stood = [], None, [p.copy() for p in STARTS]
    for r in range(rounds):
        for b, m in enumerate(own):
            poses, quats = all_round(positions[b], quat)
            depth_scan(world, torch.from_numpy(poses).to(device), torch.from_numpy(quats).to(device), into=m, intrins=K, **cam)
            m.free.carve(torch.from_numpy(positions[b]).to(device), torch.from_numpy(body_points(positions[b])).to(device),
                         max_range=ROBOT_RADIUS)
        merged = merge_maps(own)
        field = clearance_field(merged, 0.5)                    # unknown='free': a frontier voxel can be a goal
        fields = travel_fields(field, torch.from_numpy(positions).to(device), ROBOT_RADIUS, space=merged)
        assert fields.seeded.tolist() == [1, 1], "both robots stand in traversable voxels"
        plan = assign_frontiers(merged, fields, min_size=min_size, min_cost=1e-6)
        goals = plan.goal.tolist()
        rec = dict(positions=positions.tolist(), clusters=plan.clusters.n, goals=goals, costs=plan.goal_cost.tolist())
        records.append(rec)
        if verbose:
            print(f"round {r}: {plan.clusters.n} openings of at least {min_size} voxels, {fields.rounds} worklist rounds for both fields")
        if min(goals) < 0:
            if verbose:
                print("         fewer reachable openings than robots are left: what remains unknown lies behind the slit")
            break
        assert goals[0] != goals[1], "the two robots are sent to different openings"
        for b, k in enumerate(goals):
            goal = plan.goal_position[b]
            assert float(goal[0]) < HALL_X, "no robot is sent behind the slit: it is narrower than the robot"
            path = travel_path(fields[b], goal)
            assert path.reachable and path.cost == int(plan.cost_fixed[b, k]), "the path has exactly the assigned cost"
            if verbose:
                c = plan.clusters.centroids[k].tolist()
                print(f"         robot {b} at ({positions[b][0]:.2f}, {positions[b][1]:.2f}, {positions[b][2]:.2f}) -> opening {k} "
                      f"({int(plan.clusters.sizes[k])} voxels around ({c[0]:.2f}, {c[1]:.2f}, {c[2]:.2f})), {float(plan.goal_cost[b]):.2f} m "
                      f"over {path.poses.shape[0]} voxels")
            positions[b] = goal.cpu().numpy()
            stood.append(positions[b].copy())
    # the first four places the robots stood in, ordered by what a robot must travel over the map
    views = np.float32(stood[:4])
    tour = plan_tour(field, torch.from_numpy(views).to(device), clearance_radius=ROBOT_RADIUS, travel=True, space=merged)
    assert not bool(tour.unreachable.any()), "every place a robot stood in is reachable over the map"
    if verbose:
        legs = sum(bool(tour.via_flag[u, v]) for u, v in zip(tour.walk, tour.walk[1:]))
        print(f"tour through {len(views)} views: order {tour.order.tolist()}, {tour.length:.2f} m, {legs} legs over the map, "
              f"{tour.poses.shape[0]} rows")
    return records, tour


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-size", type=int, default=4)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the planning chain have no CPU fallback")
    records, _ = explore(args.rounds, args.min_size)
    print("goals per round:", [r["goals"] for r in records])
    return records


if __name__ == "__main__":
    main()
