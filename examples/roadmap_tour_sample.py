#!/usr/bin/env python3
"""Views behind obstacles: the planning chain on the bundled sample with a free-space roadmap behind the tour's legs.

tools.select_views picks eight of a 6 x 6 x 4 grid of candidate views.  tools.plan_tour alone joins them by straight legs and routes
a blocked leg through other views only; a view no such route reaches is reported unreachable.  With via= it also builds a roadmap
(tools.build_roadmap) over the views and a lattice of free-space nodes (synth.roadmap_lattice, two layers 1 m apart over the cloud's
footprint), collision-checks its edges with the swept clearance query, and lets a leg run over it wherever that is shorter than the
straight leg or the straight leg is blocked.  optimize_trajectory then bends the walk locally with the swept clearance term.  Prints
both tours side by side and the fused mean reward before and after the optimiser.

The bundled cloud holds the ground the bundled path runs on, 9 mm below its first waypoint, so the radius here is 8 mm.

    python examples/roadmap_tour_sample.py [--opt-steps 40] [--radius 0.008] [--spacing 1.0]
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
    ap.add_argument("--spacing", type=float, default=1.0)
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
    lo, hi = pts_np.min(axis=0).astype(np.float64), pts_np.max(axis=0).astype(np.float64)
    z = float(path[:, 2].astype(np.float64).mean())
    lattice = torch.from_numpy(synth.roadmap_lattice((lo[0], lo[1], z), (hi[0], hi[1], z + args.spacing), args.spacing))
    plain = plan_tour(on_path, poses, qs, clearance_radius=args.radius)
    tour = plan_tour(on_path, poses, qs, clearance_radius=args.radius, via=lattice)
    rm = tour.roadmap

    planned = ModelTraj.sharing_cloud_of(on_path, tour.poses, tour.quats, clearance_radius=args.radius, clearance_weight=5.0,
                                         clearance_mode="segments")

    def fused_mean(model):
        return float(torch.sigmoid(model.coverage_log_odds(vis_wps_dist=0.0)).mean())

    planned(vis_wps_dist=0.0)
    out = {"n_nodes": len(poses), "n_lattice": len(lattice), "open_edges": rm.n_open, "isolated_nodes": int(rm.isolated.sum()),
           "n_walk": len(tour.walk), "n_walk_nodes": len(tour.walk_nodes), "walk": tour.walk, "legs_over_roadmap": int(tour.via_flag.sum()) // 2,
           "unreachable_without": int(plain.unreachable.sum()), "unreachable_with_roadmap": int(tour.unreachable.sum()),
           "blocked_legs": int(tour.blocked.sum()) // 2, "plain_length": plain.length, "planned_length": tour.length,
           "clearance_planned_start": float(planned.loss["clearance"]), "reward_before": fused_mean(planned)}
    optimize_trajectory(planned, n_opt_steps=args.opt_steps, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
    out["reward_after"] = fused_mean(planned)
    print(f"roadmap: {len(poses)} views + {len(lattice)} lattice nodes, {rm.n_open} open edges, {out['isolated_nodes']} nodes without one")
    print(f"straight legs only: {out['blocked_legs']} of {len(poses) * (len(poses) - 1) // 2} legs blocked, {out['unreachable_without']} "
          f"views unreachable, {len(plain.order)} visited over {plain.length:.3f} m")
    print(f"with the roadmap: {out['legs_over_roadmap']} pairs of views are closer over it, {out['unreachable_with_roadmap']} views "
          f"unreachable, {len(tour.order)} visited over {tour.length:.3f} m through {len(tour.walk_nodes)} nodes "
          f"(swept clearance term {out['clearance_planned_start']:.3g})")
    print(f"fused mean reward of the planned path: {out['reward_before']:.6f}, after {args.opt_steps} optimiser steps "
          f"{out['reward_after']:.6f}")
    return out


if __name__ == "__main__":
    main()
