"""What the log-odds prior costs (prior_kernels.hip, ModelTraj(prior_log_odds=...)), in one process, on bench.py's inputs
(1 M points x 128 waypoints, synth seed 0):

  kernels   each prior-aware entry point next to its no-prior twin, over the state of one forward, event-timed over back-to-back calls
            (what the GPU takes per call; rocprofv3 --kernel-trace --stats gives the kernels alone):
              reward            tohip_traj_reward (prefilled 0, and 1 for reference)  | tohip_traj_reward_prior
              reward_backward   tohip_traj_reward_backward (prefilled 0, and 1)       | tohip_traj_reward_backward_prior
              backward          tohip_traj_backward (scalars, gout)                    | tohip_traj_backward_prior
            and the prior's own two: tohip_traj_prior_build (once per prior), tohip_traj_coverage
  step      optimize_trajectory per step, default mode, for the same model with no prior (the one-call step), with no prior through
            the separate calls (what the routing costs alone), a zero prior and a random prior (the separate calls), alternating:
            whole runs at two step counts, the difference over the extra steps

    python tools/time_prior.py [--points 1000000] [--wps 128] [--reps 5] [--steps 20,120] [--json out.json]
    python tools/time_prior.py --only-kernels        # under rocprofv3 --kernel-trace --stats
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
from trajectory_optimization_amd import _lib, ops, synth  # noqa: E402
from trajectory_optimization_amd._lib import check, ptr, stream_ptr  # noqa: E402
from trajectory_optimization_amd.model import ModelTraj  # noqa: E402
from trajectory_optimization_amd.optimizer import _optimize_trajectory_split, optimize_trajectory  # noqa: E402

K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT


def event_us(fn, reps, calls):
    fn()
    best = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        best.append(1000.0 * a.elapsed_time(b) / calls)
    return {"us_min": min(best), "us_median": float(np.median(best))}


def kernels(n, W, reps, calls, dev):
    L = _lib.lib()
    pts = torch.from_numpy(synth.make_cloud(n, seed=0)).to(dev)
    poses, quats = synth.make_path(W, optical=True)
    cloud = ops.PackedCloud(pts)
    cam = ops.Camera(K, IW, IH)
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    ws = ops.TrajWorkspace(cloud, W)
    half = torch.full((n,), 0.5, dtype=torch.float32, device=dev)
    lo_sum, _ = ops.traj_forward(cloud, p, q, cam, ws)
    values = torch.from_numpy(np.random.default_rng(3).uniform(0.0, 3.0, n).astype(np.float32)).to(dev)
    prior = ops.LogOddsPrior(cloud, values)
    f32 = dict(dtype=torch.float32, device=dev)
    rewards, scalars, gout = torch.empty(n, **f32), torch.empty(4, **f32), torch.ones(1, **f32)
    pg, qg = torch.empty((W, 3), **f32), torch.empty((W, 4), **f32)
    out_map = torch.empty(n, **f32)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    blob, wsb, st, rig = ptr(cloud.blob), ws.bytes, stream_ptr(), ops._NULL_RIG
    pb = ptr(prior.buf)

    def reward(pre, with_prior):
        if with_prior:
            return lambda: check(L.tohip_traj_reward_prior(blob, ptr(lo_sum), n, cam.eps, 0, ptr(rewards), ptr(scalars), ptr(ws.buf), wsb, pb, st), "r")
        return lambda: check(L.tohip_traj_reward(blob, ptr(lo_sum), n, cam.eps, pre, ptr(half if pre else rewards), ptr(scalars), ptr(ws.buf), wsb,
                                                 st), "r")

    def reward_backward(pre, with_prior):
        if with_prior:
            return lambda: check(L.tohip_traj_reward_backward_prior(blob, n, W, cam.ref(), rig, 0, None, ptr(lo_sum), cam.eps, 0, ptr(rewards),
                                                                    ptr(scalars), ptr(gout), ptr(pg), ptr(qg), ptr(ws.buf), wsb, pb, st), "rb")
        return lambda: check(L.tohip_traj_reward_backward(blob, n, W, cam.ref(), rig, 0, None, ptr(lo_sum), cam.eps, pre,
                                                          ptr(half if pre else rewards), ptr(scalars), ptr(gout), ptr(pg), ptr(qg), ptr(ws.buf),
                                                          wsb, st), "rb")

    def backward(with_prior):
        if with_prior:
            return lambda: check(L.tohip_traj_backward_prior(blob, n, W, cam.ref(), rig, 0, None, ptr(lo_sum), None, ptr(scalars), ptr(gout),
                                                             ptr(pg), ptr(qg), ptr(ws.buf), wsb, pb, st), "b")
        return lambda: check(L.tohip_traj_backward(blob, n, W, cam.ref(), rig, 0, None, ptr(lo_sum), None, ptr(scalars), ptr(gout), ptr(pg),
                                                   ptr(qg), ptr(ws.buf), wsb, st), "b")

    out = {"points": n, "waypoints": W, "touched_points": int((lo_sum[:n] != 0).sum())}
    with torch.cuda.device(dev):
        rows = {"reward": (reward(0, False), reward(0, True), reward(1, False)),
                "reward_backward": (reward_backward(0, False), reward_backward(0, True), reward_backward(1, False)),
                "backward": (backward(False), backward(True), None)}
        for name, (twin, with_p, prefilled) in rows.items():   # alternating, twin first
            t, w = [], []
            for _ in range(reps):
                t.append(event_us(twin, 1, calls)["us_median"])
                w.append(event_us(with_p, 1, calls)["us_median"])
            out[name] = {"no_prior_us": float(np.median(t)), "prior_us": float(np.median(w))}
            out[name]["delta_us"] = out[name]["prior_us"] - out[name]["no_prior_us"]
            out[name]["within_10pct_plus_2us"] = out[name]["prior_us"] <= 1.1 * out[name]["no_prior_us"] + 2.0
            if prefilled is not None:
                out[name]["no_prior_prefilled_us"] = event_us(prefilled, reps, calls)["us_median"]
        out["prior_build"] = event_us(lambda: check(L.tohip_traj_prior_build(blob, n, ptr(values), pb, prior.bytes, ptr(status), st), "pb"),
                                      reps, calls)
        out["coverage"] = event_us(lambda: check(L.tohip_traj_coverage(blob, n, ptr(lo_sum), pb, 3.5, ptr(out_map), st), "c"), reps, calls)
    torch.cuda.synchronize()
    return out


def run_ms(model_factory, steps, split=False):
    m = model_factory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if split:   # the separate calls without a prior: what the routing costs by itself
        _optimize_trajectory_split(m, steps, 0.05, 0.01, 1e9, 1e9, 0.5, (0.9, 0.999), 1e-8)
    else:
        optimize_trajectory(m, steps, 0.05, 0.01, 1e9, 1e9, 0.5)   # thresholds out of reach: every step is taken
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0)


def step_case(n, W, steps, reps, dev):
    pts = torch.from_numpy(synth.make_cloud(n, seed=0))
    p, q = synth.make_path(W, optical=True)
    base = ModelTraj(pts, torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev)
    variants = {"no_prior": None, "no_prior_split": None, "zero_prior": torch.zeros(n, device=dev),
                "random_prior": torch.from_numpy(np.random.default_rng(3).uniform(0.0, 3.0, n).astype(np.float32)).to(dev)}

    def factory(prior):
        return lambda: ModelTraj.sharing_cloud_of(base, torch.from_numpy(p), torch.from_numpy(q), prior_log_odds=prior)
    for k, prior in variants.items():   # warm-up: plans, workspaces, code objects
        run_ms(factory(prior), 3, k == "no_prior_split")
    per = {k: [] for k in variants}
    for _ in range(reps):
        for k, prior in variants.items():   # alternating
            sp = k == "no_prior_split"
            lo, hi = run_ms(factory(prior), steps[0], sp), run_ms(factory(prior), steps[1], sp)
            per[k].append((hi - lo) / (steps[1] - steps[0]))
    out = {f"{k}_ms_per_step_median": float(np.median(v)) for k, v in per.items()}
    out.update({f"{k}_ms_per_step_min": min(v) for k, v in per.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--wps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", default="20,120")
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"kernels": kernels(args.points, args.wps, args.reps, args.calls, dev)}
    if not args.only_kernels:
        out["step"] = step_case(args.points, args.wps, [int(s) for s in args.steps.split(",")], args.reps, dev)
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
