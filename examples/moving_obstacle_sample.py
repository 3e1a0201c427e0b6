#!/usr/bin/env python3
"""A map that forgets what moved away: a pillar stands in a room for two scans and is gone for the rest.

A synthetic room (synth.box_room: a 2 x 2 x 1 m box) is scanned from one place.  In the first two scans a pillar stands between the
scanner and the far wall (synth.pillar_scan moves the returns of the rays it blocks to its face); then the room is scanned empty.
Every scan goes into an ops.EvidenceMap — per voxel an integer log-odds value, + hit where a return fell, - miss where a ray passed,
the occupied and free planes derived from it — and into a plain ops.SpaceMap, whose bits are only ever set.  After each scan the
sample asks both maps the two questions a planner asks: is there line of sight through the pillar's place, and does the clearance
field (rebuilt in place) open the leg through it.  The evidence map changes its mind once the misses outweigh the hits; the plain map
never does.

    python examples/moving_obstacle_sample.py [--scans 8] [--radius 0.09] [--hit 17] [--miss 8]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import clearance_field, evidence_map, occupancy_grid, space_map  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=8, help="scans of the empty room after the two with the pillar")
    ap.add_argument("--radius", type=float, default=0.09, help="the clearance radius of the leg in metres")
    ap.add_argument("--hit", type=int, default=17)
    ap.add_argument("--miss", type=int, default=8)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map layer has no CPU fallback")
    device = torch.device("cuda:0")
    S = synth.EVID_SCENE
    scanner = torch.tensor(S["scanner"], device=device)
    room = synth.box_room(step=S["step"])
    with_pillar = synth.pillar_scan(room, S["scanner"], *S["pillar"])
    a, b = (torch.tensor([p], device=device) for p in S["leg"])

    box = dict(origin=S["origin"], dims=S["dims"], resolution=S["resolution"], device=device)
    evidence = evidence_map(occupancy_grid(**box), hit=args.hit, miss=args.miss)
    plain = space_map(occupancy_grid(**box))
    fields = {"evidence": clearance_field(evidence.space, 0.5), "plain": clearance_field(plain, 0.5)}
    maps = {"evidence": evidence, "plain": plain}
    first = {name: {"sight": None, "leg": None} for name in maps}
    for k in range(2 + args.scans):
        rows = torch.from_numpy(with_pillar if k < 2 else room).to(device)
        line = f"scan {k + 1} ({'pillar' if k < 2 else 'empty '}):"
        for name, m in maps.items():
            m.integrate(scanner, rows)
            grid = m.occupied
            sight = int(grid.line_of_sight(a, b)[0]) == 1
            leg_open = int(fields[name].rebuild().edges(a, b, args.radius)[1][0]) == -1
            if k >= 2:
                for what, now in (("sight", sight), ("leg", leg_open)):
                    if now and first[name][what] is None:
                        first[name][what] = k + 1
            line += f"  {name}: sight {'clear' if sight else 'blocked'}, leg {'open' if leg_open else 'blocked'}"
        updated, known, appeared, vanished = evidence.last_counts()
        print(f"{line}  [evidence: {updated} voxels updated, {known} newly known, +{appeared} / -{vanished} occupied]")
    for name in maps:
        s, leg = first[name]["sight"], first[name]["leg"]
        print(f"{name} map: line of sight through the pillar's place clear after scan {s if s else 'none'}; "
              f"the leg open at {args.radius} m after scan {leg if leg else 'none'}")
    values, _ = evidence.log_odds(torch.tensor([[1.05, 1.0, 0.35]], device=device))
    print(f"log-odds at the pillar's face now: {int(values[0])} (x 0.05)")
    return {name: first[name] for name in maps}


if __name__ == "__main__":
    main()
