#!/usr/bin/env python3
"""Where to look from: greedy view selection on the bundled sample.

Candidates: a 6 x 6 grid of positions over the bundled cloud at the bundled path's height, four headings each (144 views).
tools.select_views chooses as many of them as the bundled path has evaluated waypoints.  Prints the fused mean reward — sigmoid of
the fused log-odds map over all points — of
  (a) the bundled path's evaluated views,
  (b) the selected views,
  (c) both after optimize_trajectory (the selection is a start for the local optimiser, not a replacement).

    python examples/view_selection_sample.py [--opt-steps 40]
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
from trajectory_optimization_amd.tools import load_intrinsics, select_views  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt-steps", type=int, default=40)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the visibility path has no CPU fallback")
    device = torch.device("cuda:0")
    d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
    pts_np = np.ascontiguousarray(d["pts"], dtype=np.float32)
    path = np.ascontiguousarray(d["poses"], dtype=np.float32)
    pts = torch.from_numpy(pts_np)
    K, img_width, img_height = load_intrinsics(device=device)
    quats = torch.from_numpy(np.tile(np.float32([1.0, 0.0, 0.0, 0.0]), (len(path), 1)))

    on_path = ModelTraj(pts, torch.from_numpy(path), quats, K, img_width, img_height, device=device)   # packs the cloud once
    n_views = -(-len(path) // on_path._wps_step(0.5))     # the waypoints the path's visibility term evaluates

    def fused_mean(model, vis_wps_dist):
        return float(torch.sigmoid(model.coverage_log_odds(vis_wps_dist=vis_wps_dist)).mean())

    cand_poses, cand_quats = synth.bundled_candidate_grid(pts_np, path)
    sel = select_views(on_path, torch.from_numpy(cand_poses), torch.from_numpy(cand_quats), n_views)
    chosen = ModelTraj.sharing_cloud_of(on_path, sel.poses, sel.quats)
    out = {"n_views": n_views, "n_selected": sel.n_selected, "order": sel.order.tolist(), "path": fused_mean(on_path, 0.5),
           "selected": fused_mean(chosen, 0.0)}
    assert abs(out["selected"] - sel.mean_reward) < 1e-5   # the selection reports what a model on its views rewards
    kw = dict(n_opt_steps=args.opt_steps, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9)
    optimize_trajectory(on_path, **kw)
    optimize_trajectory(chosen, vis_wps_dist=0.0, **kw)
    out["path_optimised"], out["selected_optimised"] = fused_mean(on_path, 0.5), fused_mean(chosen, 0.0)
    print(f"{n_views} views of {len(cand_poses)} candidates ({sel.nnz} sparse entries, {int(sel.absent.sum())} absent): {out['order']}")
    print(f"fused mean reward: bundled path {out['path']:.6f}, selected views {out['selected']:.6f}; after {args.opt_steps} optimiser "
          f"steps: path {out['path_optimised']:.6f}, selected views {out['selected_optimised']:.6f}")
    return out


if __name__ == "__main__":
    main()
