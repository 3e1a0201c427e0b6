"""optimize_poses (B starts in one pass per step) against B sequential optimize_pose runs of the same starts, in one process,
alternating, on the bundled 40 452-point cloud and a 1 M-point synthetic cloud.  The final poses must be torch.equal.

Whole runs are timed with a synchronised host clock at two step counts; the difference over the extra steps is the steady-state
cost of one step (`*_ms_per_step`), what remains at the shorter count is the run's fixed cost (`*_fixed_ms`: setup, the
write-back and the one host synchronisation; for the sequential side, B runs' worth).

    python tools/time_pose_multi.py [--steps 20,220] [--reps 3] [--starts 1,8,64,256] [--clouds bundled,1m] [--json out.json]
    python tools/time_pose_multi.py --only-multi --starts 64 --clouds 1m      # under rocprofv3 (--kernel-trace --stats, or --pmc)
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
from trajectory_optimization_amd import synth  # noqa: E402
from trajectory_optimization_amd.model import ModelPose  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses  # noqa: E402


def starts(B, centre):
    rng = np.random.default_rng(B)
    out = []
    for _ in range(B):
        q = rng.standard_normal(4).astype(np.float32)
        q = q / np.linalg.norm(q) * (1 if q[0] >= 0 else -1)
        t = np.float32(centre) + rng.uniform(-1, 1, 3).astype(np.float32)
        out.append((torch.from_numpy(t[None, :]), torch.from_numpy(q[None, :])))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="20,220", help="two step counts: the per-step cost is the slope between them")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--starts", default="1,8,64,256")
    ap.add_argument("--clouds", default="bundled,1m")
    ap.add_argument("--only-multi", action="store_true", help="run optimize_poses only, at the larger step count (for profilers)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    s1, s2 = (int(s) for s in args.steps.split(","))
    dev = torch.device("cuda:0")
    K = torch.from_numpy(synth.K_INTRINS)
    clouds = {"bundled": (lambda: np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))["pts"], (6.0, 2.0, 0.0)),
              "1m": (lambda: synth.make_cloud(1_000_000, 0), (0.0, 0.0, 0.0))}
    rows = []
    for name in args.clouds.split(","):
        make, centre = clouds[name]
        pts_np = make()
        base = ModelPose(torch.from_numpy(pts_np), torch.zeros(1, 3), torch.tensor([[1.0, 0, 0, 0]]), K, synth.IMG_WIDTH, synth.IMG_HEIGHT,
                         device=dev)
        for B in (int(b) for b in args.starts.split(",")):
            st = starts(B, centre)

            def models():
                return [ModelPose.sharing_cloud_of(base, t, q) for t, q in st]

            def kw(steps):
                return dict(n_opt_steps=steps, lr_pose=0.1, lr_quat=0.1)
            if args.only_multi:
                optimize_poses(models(), **kw(s2))   # warm-up
                t = timed(lambda: optimize_poses(models(), **kw(s2)))
                print(f"{name} n={len(pts_np)} B={B} optimize_poses {s2} steps {t:.3f} ms", flush=True)
                continue
            optimize_pose(models()[0], **kw(s1))   # warm-up
            optimize_poses(models(), **kw(s1))
            tm = {(side, s): [] for side in ("seq", "multi") for s in (s1, s2)}
            for _ in range(args.reps):   # alternating
                for s in (s1, s2):
                    ms, mb = models(), models()
                    tm[("seq", s)].append(timed(lambda: [optimize_pose(m, **kw(s)) for m in ms]))
                    tm[("multi", s)].append(timed(lambda: optimize_poses(mb, **kw(s))))
                    if not all(torch.equal(a.trans, b.trans) and torch.equal(a.quat, b.quat) for a, b in zip(ms, mb)):
                        raise SystemExit(f"{name} B={B}: the batch's final poses differ from the sequential runs")
            row = dict(cloud=name, n=int(len(pts_np)), B=B, steps=[s1, s2], equal=True)
            for side in ("seq", "multi"):
                a, b = min(tm[(side, s1)]), min(tm[(side, s2)])
                per = (b - a) / (s2 - s1)
                row[f"{side}_ms_per_step"], row[f"{side}_fixed_ms"] = per, a - s1 * per
                row[f"{side}_run_ms"] = {str(s1): a, str(s2): b}
            row["speedup"] = row["seq_ms_per_step"] / row["multi_ms_per_step"]
            rows.append(row)
            print(f"{name:8s} n={row['n']:8d} B={B:4d}  per step: sequential {row['seq_ms_per_step']:8.4f} ms  multi {row['multi_ms_per_step']:8.4f} ms"
                  f"  x{row['speedup']:.1f}  | fixed per run: sequential {row['seq_fixed_ms']:7.3f} ms  multi {row['multi_fixed_ms']:7.3f} ms"
                  f"  (bitwise equal)", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
