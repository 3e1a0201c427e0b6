#!/usr/bin/env python3
"""Plan against the MAP instead of the current cloud: a path through a doorway over free-space nodes nobody supplied.

A synthetic room (synth.box_room: a 2 x 2 x 1 m box with a doorway in the wall x = 2) is scanned as two messages
(synth.doorway_messages): from inside, where the cone through the opening returns nothing and stays unknown, and from just beyond the
door, with a range of 1.4 m.  Both are integrated into one ops.SpaceMap.  tools.clearance_field(space, unknown='obstacle') then holds,
per voxel, a conservative distance to the nearest occupied OR never-seen voxel; tools.free_nodes lists the voxels that keep the
clearance radius — the roadmap's nodes come from the map itself — and tools.plan_path(field, ...) finds the route through the doorway:
every leg is certified against everything either message measured, and nothing is planned through space no ray has crossed.  A goal
in the corner no scan reached is refused.

    python examples/map_planning_sample.py [--radius 0.15] [--stride 2] [--max-dist 0.4]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import clearance_field, free_nodes, occupancy_grid, plan_path, refine_path, space_map  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=0.15, help="the clearance radius in metres")
    ap.add_argument("--stride", type=int, default=2, help="one node per stride^3 voxels")
    ap.add_argument("--max-dist", type=float, default=0.4, help="how far the field measures, in metres")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the planning chain have no CPU fallback")
    device = torch.device("cuda:0")
    scene = synth.FIELD_DOORWAY
    space = space_map(occupancy_grid(origin=scene["origin"], dims=scene["dims"], resolution=scene["resolution"], device=device))
    for k, (scanner, rows, max_range) in enumerate(synth.doorway_messages()):
        skipped = space.integrate(torch.from_numpy(scanner).to(device), torch.from_numpy(rows).to(device), max_range)
        print(f"message {k}: {len(rows)} rays ({skipped} skipped) -> {space.occupied.count()} occupied voxels, {space.free.count()} free bits")

    field = clearance_field(space, args.max_dist, unknown="obstacle")
    nodes = free_nodes(field, args.radius, stride=args.stride, space=space)
    print(f"field truncated at {field.D} voxels; {nodes.n} free-space nodes keep {args.radius} m (need2 = {field.need2(args.radius)})")

    start, goal, corner = [0.5, 0.5, 0.5], [2.6, 1.0, 0.5], [3.3, 2.3, 1.3]
    path = plan_path(field, start, goal, nodes.points, args.radius)
    d2, _ = field.segments(path.poses[:-1].contiguous(), path.poses[1:].contiguous())
    print(f"path to {goal}: {len(path.walk)} rows, {path.length:.3f} m, smallest squared gap along it {int(d2.min())} voxels")
    refined = refine_path(field, path, clearance_radius=args.radius, spacing=0.1)
    print(f"refined: {refined.poses.shape[0]} rows, {refined.length:.3f} m, {len(refined.corners)} corners")
    try:
        plan_path(field, start, corner, nodes.points, args.radius)
        refused = None
    except ValueError as e:
        refused = str(e)
    print(f"goal {corner} (never scanned): {refused}")
    return {"n_nodes": nodes.n, "length": path.length, "refined_length": refined.length, "rows": len(path.walk), "refused": refused}


if __name__ == "__main__":
    main()
