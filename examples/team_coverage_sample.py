#!/usr/bin/env python3
"""Two robots, one map: team coverage on the bundled sample.

Both robots start on the bundled path, the second shifted one metre sideways.  Prints the fused mean reward — sigmoid of the fused
log-odds map over all points — of
  (a) the start,
  (b) each robot optimised alone (optimize_trajectory), their coverage_log_odds fused with tools.fuse_log_odds,
  (c) the two optimised as a team (optimize_team: one shared reward, so they divide the scene),
and what each member adds to the team of (c) (TeamTraj.member_gains).

    python examples/team_coverage_sample.py [--opt-steps 40] [--shift 1.0]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd.model import ModelTraj, TeamTraj  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_team, optimize_trajectory  # noqa: E402
from trajectory_optimization_amd.tools import fuse_log_odds, load_intrinsics  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt-steps", type=int, default=40)
    ap.add_argument("--shift", type=float, default=1.0, help="sideways offset of the second robot's start, metres")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the visibility path has no CPU fallback")
    device = torch.device("cuda:0")
    d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
    pts = torch.from_numpy(np.ascontiguousarray(d["pts"], dtype=np.float32))
    path = np.ascontiguousarray(d["poses"], dtype=np.float32)
    K, img_width, img_height = load_intrinsics(device=device)
    quats = torch.from_numpy(np.tile(np.float32([1.0, 0.0, 0.0, 0.0]), (len(path), 1)))
    starts = [torch.from_numpy(path), torch.from_numpy((path + np.float32([0.0, args.shift, 0.0])).astype(np.float32))]

    first = ModelTraj(pts, starts[0], quats, K, img_width, img_height, device=device)   # packs the cloud once, for every model below

    def robots():
        return [ModelTraj.sharing_cloud_of(first, p, quats) for p in starts]

    def fused_mean(models):
        return float(torch.sigmoid(fuse_log_odds(*[m.coverage_log_odds() for m in models])).mean())

    kw = dict(n_opt_steps=args.opt_steps, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9)
    out = {"start": fused_mean(robots())}
    alone = robots()
    for m in alone:
        optimize_trajectory(m, **kw)
    out["alone_fused"] = fused_mean(alone)
    members = robots()
    res = optimize_team(members, **kw)
    team = TeamTraj(members)
    out["team"] = float(torch.sigmoid(team.coverage_log_odds()).mean())
    gain, count = team.member_gains()
    out["member_gain"], out["member_count"] = gain.tolist(), count.tolist()
    print(f"fused mean reward: start {out['start']:.6f}, optimised alone then fused {out['alone_fused']:.6f}, "
          f"optimised as a team {out['team']:.6f} ({res.steps_taken} steps)")
    for b in range(len(members)):
        print(f"  robot {b}: adds {out['member_gain'][b]:.6f} to the team's mean reward, sees {out['member_count'][b]} of {len(pts)} points")
    return out


if __name__ == "__main__":
    main()
