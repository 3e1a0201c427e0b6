#!/usr/bin/env python3
"""Where to stand and which way to look: view proposals on the bundled sample.

Positions: a lattice (synth.roadmap_lattice) over the bundled cloud's footprint at the bundled path's height.  tools.propose_views
keeps the positions at least --radius from the cloud and proposes each one's two best headings, ranked by how many points lie
inside the camera's range shell and field of view.  tools.select_views then chooses k = 8 views out of the proposals, and, for
comparison, k = 8 out of the fixed 6 x 6 x 4 grid (synth.bundled_candidate_grid).  Prints both fused mean rewards.  The proposal is a
heuristic pre-filter (range, not depth; no occlusion): neither result is guaranteed to be the larger.

    python examples/view_proposal_sample.py [--spacing 1.0] [--radius 0.3] [--max-views 256]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import ops, synth  # noqa: E402
from trajectory_optimization_amd.tools import load_intrinsics, propose_views, select_views  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--max-views", type=int, default=256)
    ap.add_argument("-k", type=int, default=8)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the visibility path has no CPU fallback")
    device = torch.device("cuda:0")
    d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
    pts_np = np.ascontiguousarray(d["pts"], dtype=np.float32)
    path = np.ascontiguousarray(d["poses"], dtype=np.float32)
    K, img_width, img_height = load_intrinsics(device=device)
    cam = dict(intrins=K, img_width=img_width, img_height=img_height)
    cloud = ops.PackedCloud(torch.from_numpy(pts_np).to(device))   # packed once, shared by every call below

    z = float(path[:, 2].astype(np.float64).mean())
    lo, hi = pts_np.min(axis=0).astype(np.float64), pts_np.max(axis=0).astype(np.float64)
    lattice = synth.roadmap_lattice([lo[0], lo[1], z], [hi[0], hi[1], z], args.spacing)
    prop = propose_views(cloud, torch.from_numpy(lattice), n_per_position=2, sectors=32, clearance_radius=args.radius,
                         max_views=args.max_views, K=K, img_width=img_width, img_height=img_height)
    out = {"n_positions": len(lattice), "n_open": int(prop.open.sum()), "n_proposals": prop.n_views}
    sel = select_views(cloud, prop.poses, prop.quats, args.k, **cam)
    out["proposals"], out["proposals_order"] = sel.mean_reward, sel.order.tolist()

    grid_poses, grid_quats = synth.bundled_candidate_grid(pts_np, path)
    ref = select_views(cloud, torch.from_numpy(grid_poses), torch.from_numpy(grid_quats), args.k, **cam)
    out["grid"], out["n_grid"] = ref.mean_reward, len(grid_poses)
    print(f"{out['n_open']} of {out['n_positions']} lattice positions are open; {out['n_proposals']} proposals, top score "
          f"{int(prop.score[0]) if prop.n_views else 0} points")
    print(f"fused mean reward of k = {args.k} selected views: out of the proposals {out['proposals']:.6f}, out of the fixed grid of "
          f"{out['n_grid']} {out['grid']:.6f}")
    return out


if __name__ == "__main__":
    main()
