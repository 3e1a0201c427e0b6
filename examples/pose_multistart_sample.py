#!/usr/bin/env python3
"""The camera pose sample (examples/pose_optimization_sample.py) with several starts at once: B orientations drawn from seeds
0..B-1 at the start (6, 2, 0), optimised together by optimizer.optimize_poses (one pass over the cloud per step for all of them,
Adam with constant learning rates), the start with the lowest final loss kept.  Writes the single sample's .npz (trans, quat_wxyz,
observations, losses of the kept start) plus every start's final loss and pose.

    python examples/pose_multistart_sample.py --starts 64 [--points point_cloud_10.npz] [--hpr]
"""
import argparse
import os
import sys
from time import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "examples"))

from pose_optimization_sample import random_quaternion  # noqa: E402
from trajectory_optimization_amd.model import ModelPose  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_poses  # noqa: E402
from trajectory_optimization_amd.samples import load_data  # noqa: E402
from trajectory_optimization_amd.tools import load_intrinsics  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default=None, help="point_cloud_<i>.npz (key 'pts')")
    ap.add_argument("--starts", type=int, default=16, help="number of random starting orientations (seeds 0..starts-1)")
    ap.add_argument("--opt-steps", type=int, default=400)
    ap.add_argument("--lr-pose", type=float, default=0.1)
    ap.add_argument("--lr-quat", type=float, default=0.1)
    ap.add_argument("--hpr", action="store_true", help="multiply the observations by the world-frame HPR mask (model.py:114)")
    ap.add_argument("--out", default="pose_multistart_result.npz")
    args = ap.parse_args(argv)
    if args.starts < 1:
        raise SystemExit("--starts must be at least 1")

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the visibility path has no CPU fallback")
    device = torch.device("cuda:0")
    if args.points is None:
        pts_np = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))["pts"]
    else:
        pts_np, _, _ = load_data(args.points)
    K, img_width, img_height = load_intrinsics(device=device)
    trans0 = torch.tensor([[6.0, 2.0, 0.0]])
    first = ModelPose(points=torch.from_numpy(pts_np), trans0=trans0, q0=random_quaternion(0), intrins=K, img_width=img_width,
                      img_height=img_height, min_dist=1.0, max_dist=5.0, device=device)
    models = [first] + [ModelPose.sharing_cloud_of(first, trans0, random_quaternion(s)) for s in range(1, args.starts)]
    t0 = time()
    results = optimize_poses(models, n_opt_steps=args.opt_steps, lr_pose=args.lr_pose, lr_quat=args.lr_quat, hpr=args.hpr)
    elapsed = time() - t0
    final = np.asarray([r.losses[-1] for r in results], dtype=np.float32)
    best = int(np.argmin(final))
    m = models[best]
    quat = F.normalize(m.quat.detach())
    np.savez_compressed(args.out, trans=m.trans.detach().cpu().numpy(), quat_wxyz=quat.cpu().numpy(),
                        observations=m.observations.detach().cpu().numpy(), losses=np.asarray(results[best].losses, dtype=np.float32),
                        final_losses=final, best_start=np.int64(best),
                        all_trans=torch.cat([x.trans.detach() for x in models]).cpu().numpy(),
                        all_quat_wxyz=F.normalize(torch.cat([x.quat.detach() for x in models])).cpu().numpy())
    print(f"{args.starts} starts x {args.opt_steps} steps in {elapsed:.2f} s ({1e3 * elapsed / max(args.opt_steps, 1):.3f} ms/step); "
          f"best start {best}: loss {results[best].losses[0]:.3e} -> {final[best]:.3e}; worst final loss {final.max():.3e}; wrote {args.out}")
    return results


if __name__ == "__main__":
    main()
