#!/usr/bin/env python3
"""From chosen views to a path: the planning chain on the bundled sample.

tools.select_views picks eight of a 6 x 6 x 4 grid of candidate views; it returns them in order of gain, which is not a path.
tools.plan_tour orders them from the bundled path's first waypoint so that every straight leg keeps the clearance radius from the
cloud (a leg that does not is routed through other views), and optimize_trajectory bends the result locally with the swept
clearance term (clearance_mode='segments').  Prints the tour's length in selection order against the planned order, how many legs
the swept query blocks, and the fused mean reward before and after the optimiser.

The bundled cloud holds the ground the bundled path runs on, 9 mm below its first waypoint, so the radius here is 8 mm: with a
larger one the start itself would be too close to the cloud and no leg could leave it.

    python examples/view_tour_sample.py [--opt-steps 40] [--radius 0.008]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.model import ModelTraj  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_trajectory  # noqa: E402
from trajectory_optimization_amd.tools import load_intrinsics, plan_tour, select_views  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt-steps", type=int, default=40)
    ap.add_argument("--radius", type=float, default=0.008)
    ap.add_argument("--views", type=int, default=8)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the visibility path has no CPU fallback")
    device = torch.device("cuda:0")
    d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
    pts_np = np.ascontiguousarray(d["pts"], dtype=np.float32)
    path = np.ascontiguousarray(d["poses"], dtype=np.float32)
    K, img_width, img_height = load_intrinsics(device=device)
    quats = torch.from_numpy(np.tile(np.float32([1.0, 0.0, 0.0, 0.0]), (len(path), 1)))
    on_path = ModelTraj(torch.from_numpy(pts_np), torch.from_numpy(path), quats, K, img_width, img_height, device=device)

    cand_poses, cand_quats = synth.bundled_candidate_grid(pts_np, path)
    sel = select_views(on_path, torch.from_numpy(cand_poses), torch.from_numpy(cand_quats), args.views)
    poses = torch.cat([on_path.poses.data[:1], sel.poses])   # node 0: where the robot is
    qs = torch.cat([on_path.quats.data[:1], sel.quats])
    tour = plan_tour(on_path, poses, qs, clearance_radius=args.radius)

    clr = dict(clearance_radius=args.radius, clearance_weight=5.0, clearance_mode="segments")
    planned = ModelTraj.sharing_cloud_of(on_path, tour.poses, tour.quats, **clr)
    in_selection_order = ModelTraj.sharing_cloud_of(on_path, poses, qs, **clr)

    def fused_mean(model):
        return float(torch.sigmoid(model.coverage_log_odds(vis_wps_dist=0.0)).mean())

    planned(vis_wps_dist=0.0)
    in_selection_order(vis_wps_dist=0.0)
    out = {"n_nodes": len(poses), "n_walk": len(tour.walk), "walk": tour.walk, "unreachable": int(tour.unreachable.sum()),
           "blocked_legs": int(tour.blocked.sum()) // 2, "moves": tour.moves,
           "selection_length": float((poses[1:] - poses[:-1]).norm(dim=1).sum()), "nn_length": tour.nn_length,
           "planned_length": tour.length, "clearance_selection_start": float(in_selection_order.loss["clearance"]),
           "clearance_planned_start": float(planned.loss["clearance"]), "reward_before": fused_mean(planned)}
    optimize_trajectory(planned, n_opt_steps=args.opt_steps, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
    out["reward_after"] = fused_mean(planned)
    print(f"{len(poses) - 1} views from the start: {out['blocked_legs']} of {len(poses) * (len(poses) - 1) // 2} legs come within "
          f"{args.radius} m of the cloud, {out['unreachable']} views unreachable; walk {tour.walk} ({tour.moves} 2-opt moves)")
    print(f"length: selection order {out['selection_length']:.3f} m (swept clearance term {out['clearance_selection_start']:.3g}), "
          f"nearest neighbour {out['nn_length']:.3f} m, planned {out['planned_length']:.3f} m (term {out['clearance_planned_start']:.3g})")
    print(f"fused mean reward of the planned path: {out['reward_before']:.6f}, after {args.opt_steps} optimiser steps "
          f"{out['reward_after']:.6f}")
    return out


if __name__ == "__main__":
    main()
