#!/usr/bin/env python3
"""Time greedy view selection against the brute force the dense calls allow.

    python tools/time_views.py [--points 1000000] [--grid 16] [--headings 4] [--k 32] [--runs 5] [--json out.json]

Medians of `--runs` whole runs, each bracketed by a device synchronisation:
  build        ops.ViewSet.append of all M candidates (the forwards in chunks + the compaction)
  forwards     the same chunks' forwards alone (what the compaction is added to)
  sparse_round tohip_views_select's k rounds / k
  brute_round  per round one f32 add of S to the M dense rows kept resident and tohip_traj_reward_multi over them (what the library
               could do before the sparse path), k rounds / k; the two (M, npad) buffers are allocated once
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from trajectory_optimization_amd import ops, synth  # noqa: E402


def timed(fn, runs):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--headings", type=int, default=4)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-brute", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    cloud = ops.PackedCloud(torch.from_numpy(synth.make_cloud(args.points, 0)).to(dev))
    cam = ops.Camera(synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT, 1.0, 5.0)
    lin = np.linspace(-15, 15, args.grid)
    p, q = [torch.from_numpy(a).to(dev) for a in synth.candidate_grid(lin, lin, 0.0, args.headings)]
    M, k = p.shape[0], args.k
    vs = ops.ViewSet(cloud, cam, M)
    vs.append(p, q)          # warm-up, and the capacity check
    stored, needed, fits = vs.status()
    if not fits:
        vs = ops.ViewSet(cloud, cam, M, nnz_capacity=needed)
        vs.append(p, q)
        stored = vs.nnz

    def build():
        vs.appended = 0
        vs.append(p, q)

    def forwards():
        for w0 in range(0, M, vs.chunk):
            t = min(vs.chunk, M - w0)
            ws, off = vs._ws[t]
            ops.traj_forward(cloud, p[w0:w0 + t], q[w0:w0 + t], cam, ws, lo_sum=vs._dense[:t], traj_offsets=off)

    res = {"points": args.points, "candidates": M, "k": k, "chunk": vs.chunk, "nnz": stored, "nnz_share_per_row": stored / M / args.points}
    res["build_ms"], res["build_runs"] = timed(build, args.runs)
    res["forwards_ms"], res["forwards_runs"] = timed(forwards, args.runs)
    ops.views_select(vs, k)   # warm-up
    ms, runs = timed(lambda: ops.views_select(vs, k), args.runs)
    order, gain, n_sel, _ = ops.views_select(vs, k)
    res["n_selected"] = int(n_sel.item())
    res["sparse_round_ms"], res["sparse_round_runs"] = ms / k, [r / k for r in runs]
    if not args.no_brute:
        rows = torch.empty((M, cloud.npad), dtype=torch.float32, device=dev)     # allocated once, reused by every run
        X = torch.empty_like(rows)
        for w0 in range(0, M, vs.chunk):
            t = min(vs.chunk, M - w0)
            ws, off = vs._ws[t]
            ops.traj_forward(cloud, p[w0:w0 + t], q[w0:w0 + t], cam, ws, lo_sum=rows[w0:w0 + t], traj_offsets=off)
        S = torch.zeros(cloud.npad, dtype=torch.float32, device=dev)
        rewards = torch.empty((M, cloud.n), dtype=torch.float32, device=dev)
        scalars = torch.empty((M, 4), dtype=torch.float32, device=dev)
        ws = ops.TrajWorkspace(cloud, M, M)

        def brute():
            for _ in range(k):
                torch.add(rows, S[None, :], out=X)
                ops.traj_reward(cloud, X, cam, ws, rewards=rewards, scalars=scalars)

        brute()   # warm-up
        ms, runs = timed(brute, args.runs)
        res["brute_round_ms"], res["brute_round_runs"] = ms / k, [r / k for r in runs]
        res["brute_over_sparse"] = res["brute_round_ms"] / res["sparse_round_ms"]
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
