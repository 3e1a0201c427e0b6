#!/usr/bin/env python3
"""The optimiser keeps its path off what the MAP holds, not off the cloud in hand — and lets go when the map forgets.

A synthetic room (synth.box_room) is scanned twice with a pillar in it (synth.pillar_scan) into an ops.EvidenceMap.  A path runs 0.2 m
in front of the pillar's face.  The model's visibility cloud is the EMPTY room — the message in hand does not contain the pillar — so
the cloud's clearance term sees nothing to avoid.  With clearance_map=m the term asks the map: it is positive, and optimize_trajectory
pushes the waypoints away from the pillar's voxels.  Then the room is scanned empty until the map drops the pillar; the same model's
next evaluation gives a clearance of exactly 0 — the map's buffers are read at every step, nothing is re-packed.

    python examples/map_clearance_sample.py [--radius 0.3] [--weight 20] [--steps 30] [--mode waypoints|segments]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.model import ModelTraj  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_trajectory  # noqa: E402
from trajectory_optimization_amd.tools import evidence_map, occupancy_grid, trajectory_clearance  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--weight", type=float, default=20.0)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--mode", default="waypoints", choices=("waypoints", "segments"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map layer has no CPU fallback")
    device = torch.device("cuda:0")
    S = synth.EVID_SCENE
    scanner = torch.tensor(S["scanner"], device=device)
    room_np = synth.box_room(step=S["step"])
    with_pillar = torch.from_numpy(synth.pillar_scan(room_np, S["scanner"], *S["pillar"])).to(device)
    room = torch.from_numpy(room_np).to(device)

    m = evidence_map(occupancy_grid(origin=S["origin"], dims=S["dims"], resolution=S["resolution"], device=device))
    for _ in range(2):
        m.integrate(scanner, with_pillar)

    # eight waypoints along y, 0.2 m in front of the pillar's face at x = 1.0, half a metre from the floor, the ceiling and every wall
    poses = torch.tensor([[0.8, 0.65 + 0.1 * k, 0.5] for k in range(8)])
    quats = torch.from_numpy(synth.make_path(8, optical=True)[1])
    K = torch.from_numpy(synth.K_INTRINS)
    kw = dict(device=device, clearance_radius=args.radius, clearance_weight=args.weight, clearance_mode=args.mode)
    segments = args.mode == "segments"

    def nearest(model):
        d = trajectory_clearance(m, model.poses.data, args.radius, segments=segments)[0]
        return float(d.min())

    cloud_only = ModelTraj(room, poses, quats, K, synth.IMG_WIDTH, synth.IMG_HEIGHT, **kw)
    cloud_only(vis_wps_dist=0.0)
    print(f"the cloud's term (the empty room is the cloud in hand): clearance = {float(cloud_only.loss['clearance'].detach()):.4f}")

    model = ModelTraj(room, poses, quats, K, synth.IMG_WIDTH, synth.IMG_HEIGHT, clearance_map=m, **kw)
    model(vis_wps_dist=0.0)
    before = float(model.loss["clearance"].detach())
    print(f"the map's term, the pillar scanned twice: clearance = {before:.4f}, nearest occupied voxel centre {nearest(model):.3f} m")
    optimize_trajectory(model, args.steps, 0.01, 0.0, 1e9, 1e9, 0.0)
    after = float(model.loss["clearance"])
    print(f"after {args.steps} steps of optimize_trajectory: clearance = {after:.4f}, nearest occupied voxel centre {nearest(model):.3f} m")

    scans = 0
    probe = torch.tensor([[x, y, 0.45] for x in (0.95, 1.05) for y in (0.85, 1.0, 1.15)], device=device)
    while bool((m.log_odds(probe)[1] == 2).any()) and scans < 8:
        m.integrate(scanner, room)
        scans += 1
    model(vis_wps_dist=0.0)   # the same model: the map's buffers are read as they are now
    gone = float(model.loss["clearance"].detach())
    print(f"after {scans} scans of the empty room the map has dropped the pillar: clearance = {gone:.4f} (nearest {nearest(model)})")
    return {"cloud_only": float(cloud_only.loss["clearance"].detach()), "before": before, "after": after, "forgotten": gone, "scans": scans}


if __name__ == "__main__":
    main()
