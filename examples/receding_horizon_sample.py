#!/usr/bin/env python3
"""Receding-horizon planning against what has already been seen, on the bundled sample.

Each plan optimises a window of `--horizon` waypoints with ModelTraj over the shared cloud, starting from the map committed so far
(prior_log_odds).  The robot then flies the plan's first `--commit` waypoints: their coverage is fused into the map
(coverage_log_odds(upto=commit), clamped at OctoMap's upper threshold), and the window moves on — the rest of the optimised plan
followed by the next waypoints of the original path.  The next plan rewards the points the robot has not looked at yet.

    python examples/receding_horizon_sample.py [--plans 4] [--horizon 12] [--commit 4] [--opt-steps 40]

Prints each plan's mean reward (its own view: the map plus its waypoints) and the committed map's mean, sigmoid(map) over all points.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd.model import ModelTraj  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_trajectory  # noqa: E402
from trajectory_optimization_amd.tools import load_intrinsics  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=4)
    ap.add_argument("--horizon", type=int, default=12, help="waypoints per plan (>= 3)")
    ap.add_argument("--commit", type=int, default=4, help="waypoints flown (and committed to the map) per plan")
    ap.add_argument("--opt-steps", type=int, default=40)
    ap.add_argument("--clamp-max", type=float, default=3.5, help="OctoMap's upper clamping threshold (log-odds)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the visibility path has no CPU fallback")
    if args.horizon < 3 or not 0 < args.commit < args.horizon:
        raise SystemExit("need horizon >= 3 and 0 < commit < horizon")
    device = torch.device("cuda:0")
    d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
    pts = torch.from_numpy(np.ascontiguousarray(d["pts"], dtype=np.float32))
    path = np.ascontiguousarray(d["poses"], dtype=np.float32)
    K, img_width, img_height = load_intrinsics(device=device)
    ident = np.array([1.0, 0.0, 0.0, 0.0], dtype=np.float32)

    window_p = path[:args.horizon].copy()
    window_q = np.tile(ident, (len(window_p), 1))
    nxt = len(window_p)   # the next waypoint of the original path to enter the window
    first, prior = None, None
    out = {"plan_mean_reward": [], "committed_mean_reward": []}
    for i in range(args.plans):
        kw = dict(prior_log_odds=prior)
        model = (ModelTraj(pts, torch.from_numpy(window_p), torch.from_numpy(window_q), K, img_width, img_height, device=device, **kw)
                 if first is None else ModelTraj.sharing_cloud_of(first, torch.from_numpy(window_p), torch.from_numpy(window_q), **kw))
        if first is None:
            first = model
        optimize_trajectory(model, n_opt_steps=args.opt_steps, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
        plan_mean = float(model.mean_reward)
        # fly the first `commit` waypoints: their coverage joins the map
        prior = model.coverage_log_odds(upto=args.commit, clamp_max=args.clamp_max, vis_wps_dist=0.0)
        committed = float(torch.sigmoid(prior).mean())
        out["plan_mean_reward"].append(plan_mean)
        out["committed_mean_reward"].append(committed)
        print(f"plan {i}: waypoints {len(window_p)}, mean reward of the plan {plan_mean:.6f}, committed map {committed:.6f} "
              f"({int((prior > 0).sum())} of {len(pts)} points seen)")
        # the window moves on: the rest of the optimised plan, then the next waypoints of the original path
        rest_p = model.poses.detach()[args.commit:].cpu().numpy()
        rest_q = model.quats.detach()[args.commit:].cpu().numpy()
        new_p = path[nxt:nxt + args.commit]
        nxt += len(new_p)
        window_p = np.ascontiguousarray(np.concatenate([rest_p, new_p]), dtype=np.float32)
        window_q = np.ascontiguousarray(np.concatenate([rest_q, np.tile(ident, (len(new_p), 1))]), dtype=np.float32)
        if len(window_p) < 3:
            break
    return out


if __name__ == "__main__":
    main()
