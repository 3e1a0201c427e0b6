"""What team coverage costs (team_kernels.hip, optimizer.optimize_team), in one process, on bench.py's cloud (synth seed 0):

  step    optimize_team of B members x W waypoints per step, next to optimize_trajectory's separate-calls path on ONE model of the same
          B W waypoints with a zero prior — the same visibility work, a tail of B blocks instead of one — every waypoint evaluated,
          alternating: whole runs at two step counts, the difference over the extra steps, medians of --reps
  gains   tohip_team_member_gains over B per-member log-odds rows, event-timed over back-to-back calls, next to the HBM time of the
          B x Npad x 4 bytes it streams (rocprofv3 --kernel-trace --stats gives the kernel alone: --only-gains)

    python tools/time_team.py [--points 1000000] [--teams 2x64,8x128] [--reps 5] [--steps 20,120] [--json out.json]
    python tools/time_team.py --only-gains [--gain-members 8]        # under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from trajectory_optimization_amd import ops, synth  # noqa: E402
from trajectory_optimization_amd.model import ModelTraj  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_team, optimize_trajectory  # noqa: E402

K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
HBM_BYTES_PER_US = 8.0e6   # MI355X: 8 TB/s peak


def run_ms(factory, steps, team):
    models = factory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if team:   # thresholds out of reach: every step is taken
        optimize_team(models, steps, 0.05, 0.01, 1e9, 1e9, 0.0)
    else:
        optimize_trajectory(models[0], steps, 0.05, 0.01, 1e9, 1e9, 0.0)
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0)


def step_case(base, n, B, W, steps, reps, dev):
    p, q = synth.make_path(B * W, optical=True)
    zeros = torch.zeros(n, device=dev)

    def one():   # ONE model of B W waypoints; the zero prior sends it through the separate calls
        return [ModelTraj.sharing_cloud_of(base, torch.from_numpy(p), torch.from_numpy(q), prior_log_odds=zeros)]

    def members():   # the same rows as B members of W waypoints
        return [ModelTraj.sharing_cloud_of(base, torch.from_numpy(p[b * W:(b + 1) * W].copy()), torch.from_numpy(q[b * W:(b + 1) * W].copy()),
                                           prior_log_odds=zeros if b == 0 else None) for b in range(B)]
    variants = {"one_model": (one, False), "team": (members, True)}
    for f, team in variants.values():   # warm-up: workspaces, code objects
        run_ms(f, 3, team)
    per = {k: [] for k in variants}
    for _ in range(reps):
        for k, (f, team) in variants.items():   # alternating
            lo, hi = run_ms(f, steps[0], team), run_ms(f, steps[1], team)
            per[k].append((hi - lo) / (steps[1] - steps[0]))
    out = {f"{k}_ms_per_step_median": float(np.median(v)) for k, v in per.items()}
    out.update({f"{k}_ms_per_step_min": min(v) for k, v in per.items()})
    out["within_10pct_plus_2us"] = out["team_ms_per_step_median"] <= 1.1 * out["one_model_ms_per_step_median"] + 0.002
    return out


def gains_case(base, n, B, W, reps, calls, dev):
    p, q = synth.make_path(B * W, optical=True)
    cloud = base._cloud
    toff = (torch.arange(B + 1, dtype=torch.int32) * W).to(dev)
    lo, _ = ops.traj_forward(cloud, torch.from_numpy(p).to(dev), torch.from_numpy(q).to(dev), base._cam, ops.TrajWorkspace(cloud, B * W, B),
                             traj_offsets=toff)
    ops.team_member_gains(cloud, lo)
    best = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            ops.team_member_gains(cloud, lo)   # (each call ends with its small device-to-host read)
        b.record()
        b.synchronize()
        best.append(1000.0 * a.elapsed_time(b) / calls)
    nbytes = B * cloud.npad * 4
    return {"members": B, "bytes": nbytes, "hbm_us": nbytes / HBM_BYTES_PER_US, "call_us_median": float(np.median(best)),
            "call_us_min": min(best)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--teams", default="2x64,8x128", help="members x waypoints, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", default="20,120")
    ap.add_argument("--gain-members", type=int, default=8)
    ap.add_argument("--only-gains", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.points
    p, q = synth.make_path(8, optical=True)
    base = ModelTraj(torch.from_numpy(synth.make_cloud(n, seed=0)), torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(K), IW, IH,
                     device=dev)   # packs the cloud once
    out = {"points": n, "gains": gains_case(base, n, args.gain_members, 16, args.reps, args.calls, dev)}
    if not args.only_gains:
        steps = [int(s) for s in args.steps.split(",")]
        for team in args.teams.split(","):
            B, W = (int(x) for x in team.split("x"))
            out[f"step_{team}"] = step_case(base, n, B, W, steps, args.reps, dev)
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
