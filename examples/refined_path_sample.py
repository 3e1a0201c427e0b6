#!/usr/bin/env python3
"""From a roadmap's walk to a trajectory: the planning chain of roadmap_tour_sample.py with tools.refine_path between the tour and
the optimiser.

tools.plan_tour(via=lattice) visits the selected views over a free-space roadmap, so its walk moves along the lattice's directions:
it zigzags, its legs are a mix of long straight ones and short roadmap pieces, and a pass-through node copies the quaternion of the
view its leg leads to.  tools.refine_path shortcuts the walk under the same clearance radius (every view stays on it), cuts the
result into pieces of even length and turns the camera evenly between the views.  Prints, for the walk and for the refined path:
the number of nodes, the length, the mean turning angle (model.mean_angle_calc: pi is a straight path), the ratio of the longest to
the shortest leg, the swept clearance term at the start, and the fused mean reward after the same number of optimiser steps from
both starts.

    python examples/refined_path_sample.py [--opt-steps 40] [--radius 0.008] [--spacing 1.0] [--resample 0.5]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.model import ModelTraj, mean_angle_calc  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_trajectory  # noqa: E402
from trajectory_optimization_amd.tools import load_intrinsics, plan_tour, refine_path, select_views  # noqa: E402


def leg_ratio(poses):
    """The longest leg over the shortest one that is not a point."""
    legs = torch.linalg.norm((poses[1:] - poses[:-1]).to(torch.float64), dim=1)
    legs = legs[legs > 0]
    return float(legs.max() / legs.min())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt-steps", type=int, default=40)
    ap.add_argument("--radius", type=float, default=0.008)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--spacing", type=float, default=1.0, help="of the roadmap's lattice")
    ap.add_argument("--resample", type=float, default=0.5, help="the refined path's waypoint spacing")
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
    tour = plan_tour(on_path, poses, qs, clearance_radius=args.radius, via=lattice)
    refined = refine_path(on_path, tour, clearance_radius=args.radius, spacing=args.resample)

    def fused_mean(model):
        return float(torch.sigmoid(model.coverage_log_odds(vis_wps_dist=0.0)).mean())

    out = {"n_corners": len(refined.corners), "n_open_chords": refined.n_open, "blocked_input_legs": int(refined.leg_blocked.sum())}
    for name, p, q, length in (("walk", tour.poses, tour.quats, tour.length), ("refined", refined.poses, refined.quats, refined.length)):
        model = ModelTraj.sharing_cloud_of(on_path, p, q, clearance_radius=args.radius, clearance_weight=5.0, clearance_mode="segments")
        model(vis_wps_dist=0.0)
        out[f"{name}_nodes"] = int(p.shape[0])
        out[f"{name}_length"] = float(length)
        out[f"{name}_mean_angle"] = float(mean_angle_calc(p.detach().cpu()))
        out[f"{name}_leg_ratio"] = leg_ratio(p.detach().cpu())
        out[f"{name}_clearance_start"] = float(model.loss["clearance"].detach())
        out[f"{name}_reward_before"] = fused_mean(model)
        optimize_trajectory(model, n_opt_steps=args.opt_steps, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
        out[f"{name}_reward_after"] = fused_mean(model)
    print(f"the walk has {out['walk_nodes']} nodes; {out['n_open_chords']} chords over them are open and {out['blocked_input_legs']} of "
          f"its own legs are blocked; the refined path turns at {out['n_corners']} of them")
    for name in ("walk", "refined"):
        print(f"{name:8s}: {out[name + '_nodes']:4d} nodes, {out[name + '_length']:8.3f} m, mean angle {out[name + '_mean_angle']:.4f} rad, "
              f"longest / shortest leg {out[name + '_leg_ratio']:8.2f}, swept clearance term {out[name + '_clearance_start']:.3g}, "
              f"fused mean reward {out[name + '_reward_before']:.6f} -> {out[name + '_reward_after']:.6f} after {args.opt_steps} steps")
    return out


if __name__ == "__main__":
    main()
