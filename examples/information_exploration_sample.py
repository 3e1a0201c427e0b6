#!/usr/bin/env python3
"""Exploration by information: where should the robot look when nothing is unknown any more but little is certain?

A closed 2 x 2 x 1 m room (synth.box_room) swept ONCE from a corner by the door into an ops.EvidenceMap.  After that one sweep
every voxel a view from inside could reach has been observed, so tools.select_views_volume — whose gain is the number of voxels
never observed — stops with nothing to gain, although each free voxel holds one miss (L = -8, p = 0.40) and each wall voxel one hit
(L = 17, p = 0.70).  tools.select_views_information weighs every voxel by the entropy observation can still remove from it
(tools.information_table) and chooses views; tools.depth_scan from the chosen views against the ground truth, folded into the map,
lowers m.information().  Prints both selections and the information before and after.

    python examples/information_exploration_sample.py [-k 3] [--rounds 2]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.tools import (depth_scan, evidence_map, information_table, known_free, occupancy_grid,  # noqa: E402
                                               select_views_information, select_views_volume)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="select-and-scan rounds")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the planning chain have no CPU fallback")
    device = torch.device("cuda:0")
    box = dict(origin=(-0.5, -0.5, -0.5), dims=(28, 24, 16), resolution=0.125)
    rows = torch.from_numpy(synth.box_room(doorway=False)).to(device)
    truth = occupancy_grid(device=device, **box)     # the world the simulated sensor scans
    truth.insert(rows)
    scanner = torch.tensor([1.78, 0.97, 0.52], device=device)   # just inside the wall x = 2, where a door would be

    m = evidence_map(occupancy_grid(device=device, **box))
    m.integrate(scanner, rows)
    table = information_table(m)
    bit = 4096.0   # the table's scale: weights are 1/4096 bit
    before = int(m.information(table))
    print(f"one sweep of {len(rows)} rays: {m.occupied.count()} occupied and {m.free.count()} free voxels, "
          f"{m.space.unknown().count()} never observed; information left {before / bit:.0f} bits")

    P, Q = synth.candidate_grid(np.linspace(0.3, 1.7, 5), np.linspace(0.3, 1.7, 5), 0.5, 4)
    P, Q = torch.from_numpy(P).to(device), torch.from_numpy(Q).to(device)
    free = known_free(m.space, P)
    P, Q = P[free], Q[free]
    K = torch.from_numpy(synth.K_INTRINS)
    cam = dict(intrins=K, img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT, min_dist=0.25, max_dist=5.0)

    vol = select_views_volume(m, P, Q, args.k, **cam)
    print(f"by volume: {vol.n_selected} views of {len(P)} candidates (every voxel in reach has been observed once)")
    history, chosen = [before], []
    for r in range(args.rounds):
        sel = select_views_information(m, P, Q, args.k, table=table, **cam)
        chosen.append(sel.order.tolist())
        print(f"by information, round {r}: {sel.n_selected} views")
        for j in range(sel.n_selected):
            p = sel.poses[j].tolist()
            print(f"  view {int(sel.order[j])} at ({p[0]:.2f}, {p[1]:.2f}, {p[2]:.2f})  gains {int(sel.gains[j]) / bit:.0f} bits")
        if sel.n_selected == 0:
            break
        depth_scan(truth, sel.poses, sel.quats, into=m, **cam)
        history.append(int(m.information(table)))
        print(f"  scanned from them: information left {history[-1] / bit:.0f} bits (was {history[-2] / bit:.0f})")
    return {"volume_views": vol.n_selected, "information_views": [len(c) for c in chosen], "order": chosen, "information": history}


if __name__ == "__main__":
    main()
