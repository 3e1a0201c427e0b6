#!/usr/bin/env python3
"""One round of next-best-view exploration, scored by volume: from where would the robot see the most unknown space?

The doorway room of examples/exploration_sample.py (synth.box_room: a 2 x 2 x 1 m box scanned from inside, a doorway in the wall
x = 2) integrated into an ops.SpaceMap, and the same proposals — tools.propose_views over the frontier, from the lattice positions
that are known to be free.  The last link is replaced: instead of covering frontier POINTS, tools.select_views_volume counts, per
candidate, the unknown VOXELS inside its frustum that the occupied map does not hide, and chooses greedily so that no voxel is
counted twice.  A view that grazes the frontier of a shallow alcove and one that looks through the doorway into an unscanned hall no
longer score alike.  Prints each chosen view and the voxels it adds.

    python examples/volume_exploration_sample.py [--beams] [--max-range 1.5] [-k 3]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import known_free, occupancy_grid, propose_views, select_views_volume, space_map  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", action="store_true", help="add the no-return beams through the doorway (far points 6 m out)")
    ap.add_argument("--max-range", type=float, default=None, help="the scanner's range in metres (needed with --beams)")
    ap.add_argument("-k", type=int, default=3)
    ap.add_argument("--min-gain", type=int, default=1, help="stop when the best view adds fewer unknown voxels than this")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the planning chain have no CPU fallback")
    if args.beams and args.max_range is None:
        args.max_range = 1.5
    device = torch.device("cuda:0")
    scanner = np.float32([1.03, 0.97, 0.52])
    rows = synth.box_room(doorway=True)
    if args.beams:
        rows = np.concatenate([rows, synth.doorway_beams(scanner)])

    space = space_map(occupancy_grid(origin=(-0.5, -0.5, -0.5), dims=(28, 24, 16), resolution=0.125, device=device))
    skipped = space.integrate(torch.from_numpy(scanner).to(device), torch.from_numpy(rows).to(device), args.max_range)
    frontier = space.frontier()
    n_unknown = space.unknown().count()
    print(f"{len(rows)} rays ({skipped} skipped): {space.occupied.count()} occupied voxels, {space.free.count()} free bits, "
          f"{frontier.n} frontier voxels, {n_unknown} unknown voxels")
    if frontier.n == 0:
        print("the map is closed: nothing left to explore")
        return {"n_frontier": 0, "order": []}

    lattice = torch.from_numpy(synth.roadmap_lattice([-0.25, -0.25, 0.5], [2.75, 2.25, 0.5], 0.25)).to(device)
    free = known_free(space, lattice)
    K = torch.from_numpy(synth.K_INTRINS)
    cam = dict(img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT, min_dist=0.5, max_dist=5.0)
    prop = propose_views(frontier.points, lattice[free], n_per_position=2, sectors=32, max_views=64, K=K, **cam)
    sel = select_views_volume(space, prop.poses, prop.quats, args.k, min_gain=args.min_gain, intrins=K, **cam)
    print(f"{int(free.sum())} of {len(lattice)} lattice positions are known free; {prop.n_views} proposals; chosen:")
    for j in range(sel.n_selected):
        p = sel.poses[j].tolist()
        print(f"  view {int(sel.order[j])} at ({p[0]:.2f}, {p[1]:.2f}, {p[2]:.2f})  adds {int(sel.gains[j])} unknown voxels")
    print(f"together {sel.total} of the {n_unknown} unknown voxels ({sel.revealed.count()} bits in the revealed plane)")
    return {"n_frontier": frontier.n, "n_unknown": n_unknown, "order": sel.order.tolist(), "gains": sel.gains.tolist(), "total": sel.total}


if __name__ == "__main__":
    main()
