"""Per-pose occlusion bit rows in the pose kernels against the float mask, in one process, alternating the variants.

  (a) k_pose_stream_multi at 1 M points and B = 64: each pose's own bit row (tohip_pose_forward_backward_multi_bits) against one
      float mask shared by every pose (tohip_pose_forward_backward_multi);
  (b) k_pose_stream at 16 M points: a bit row (tohip_pose_forward_backward_bits) against a float mask (tohip_pose_forward_backward);
  (c) optimize_poses with 64 starts and occlusion='hpr' at occlusion_refresh_every = 1 and 10, on the bundled cloud and on 1 M points,
      split into the refresh (one batched hull pass for the 64 poses, timed alone) and the step (the run less its refreshes, per step).

(a) and (b) time the library calls with device events over `--iters` back-to-back calls (outputs preallocated), after a warm-up;
the figure is the best of `--reps` alternating rounds, per call (the two launches: the pass and its finish).

    python tools/time_pose_occlusion.py [--iters 50] [--reps 5] [--parts a,b,c] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from trajectory_optimization_amd import _lib, ops, synth  # noqa: E402
from trajectory_optimization_amd.model import ModelPose  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_poses  # noqa: E402


def starts(B, centre, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        q = rng.standard_normal(4).astype(np.float32)
        q = q / np.linalg.norm(q) * (1 if q[0] >= 0 else -1)
        t = np.float32(centre) + rng.uniform(-1, 1, 3).astype(np.float32)
        out.append((torch.from_numpy(t[None, :]), torch.from_numpy(q[None, :])))
    return out


def event_ms(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(variants, iters, reps):
    """{name: call} -> {name: best ms per call}, the variants alternating round by round after one warm-up round."""
    for call in variants.values():
        event_ms(call, max(iters // 5, 2))
    best = {k: float("inf") for k in variants}
    for _ in range(reps):
        for k, call in variants.items():
            best[k] = min(best[k], event_ms(call, iters))
    return best


def check(rc, what):
    if rc:
        _lib.check(rc, what)


def part_a(dev, K, iters, reps):
    L = _lib.lib()
    n, B = 1_000_000, 64
    pts = torch.from_numpy(synth.make_cloud(n, 0)).to(dev)
    base = ModelPose(pts, torch.zeros(1, 3), torch.tensor([[1.0, 0, 0, 0]]), K, synth.IMG_WIDTH, synth.IMG_HEIGHT, device=dev, occlusion="hpr")
    cloud, cam = base._cloud, base._cam
    st = starts(B, (0.0, 0.0, 0.0))
    trans = torch.cat([t for t, _ in st]).to(dev).contiguous()
    quat = torch.cat([q for _, q in st]).to(dev).contiguous()
    rows = base._build_occlusion_rows(trans, quat)   # the 64 poses' own rows
    mask = ops.unpack_occlusion_rows(cloud, rows[:1])[0].contiguous()   # one of them, as the float mask every pose shares
    ws = ops.PoseWorkspace(cloud, B)
    f32 = dict(dtype=torch.float32, device=dev)
    scalars, tg, qg = torch.empty((B, 4), **f32), torch.empty((B, 3), **f32), torch.empty((B, 4), **f32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    common = (cloud.blob.data_ptr(), cloud.n, trans.data_ptr(), quat.data_ptr(), B, cam.ref())
    tail = (None, scalars.data_ptr(), None, tg.data_ptr(), qg.data_ptr(), ws.buf.data_ptr(), ws.bytes, stream)
    best = alternate({"bits_per_pose": lambda: check(L.tohip_pose_forward_backward_multi_bits(*common, rows.data_ptr(), *tail), "bits"),
                      "float_shared": lambda: check(L.tohip_pose_forward_backward_multi(*common, mask.data_ptr(), *tail), "float")}, iters, reps)
    row = dict(part="a", n=n, B=B, bits_ms=best["bits_per_pose"], float_ms=best["float_shared"],
               overhead=best["bits_per_pose"] / best["float_shared"] - 1.0)
    print(f"(a) multi n={n} B={B}: per-pose bit rows {row['bits_ms']:.4f} ms  shared float mask {row['float_ms']:.4f} ms  "
          f"({100 * row['overhead']:+.1f} %)", flush=True)
    return row


def part_b(dev, K, iters, reps):
    L = _lib.lib()
    n = 16_000_000
    pts = torch.from_numpy(synth.make_cloud(n, 1)).to(dev)
    cloud = ops.PackedCloud(pts, sort=False)
    cam = ops.Camera(K, synth.IMG_WIDTH, synth.IMG_HEIGHT, 1.0, 5.0)
    g = torch.Generator().manual_seed(0)
    rows = torch.randint(-2 ** 31, 2 ** 31 - 1, (1, cloud.npad // 32), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
    mask = ops.unpack_occlusion_rows(cloud, rows)[0].contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    trans, quat = torch.zeros((1, 3), **f32), torch.tensor([[1.0, 0, 0, 0]], **f32)
    obs, scalars, grads = torch.empty(n, **f32), torch.empty(4, **f32), torch.empty(8, **f32)
    ws = ops.PoseWorkspace(cloud)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    common = (cloud.blob.data_ptr(), cloud.n, trans.data_ptr(), quat.data_ptr(), cam.ref())
    tail = (obs.data_ptr(), scalars.data_ptr(), None, grads.data_ptr(), grads.data_ptr() + 16, ws.buf.data_ptr(), ws.bytes, stream)
    best = alternate({"bits": lambda: check(L.tohip_pose_forward_backward_bits(*common, rows.data_ptr(), *tail), "bits"),
                      "float": lambda: check(L.tohip_pose_forward_backward(*common, mask.data_ptr(), *tail), "float")}, iters, reps)
    row = dict(part="b", n=n, bits_ms=best["bits"], float_ms=best["float"], ratio=best["bits"] / best["float"])
    print(f"(b) single n={n}: bit row {row['bits_ms']:.4f} ms  float mask {row['float_ms']:.4f} ms  (x{row['ratio']:.3f})", flush=True)
    return row


def part_c(dev, K, reps, steps=30):
    out = []
    clouds = {"bundled": (lambda: np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))["pts"], (6.0, 2.0, 0.0)),
              "1m": (lambda: synth.make_cloud(1_000_000, 0), (0.0, 0.0, 0.0))}
    B = 64
    for name, (make, centre) in clouds.items():
        pts = torch.from_numpy(make())
        st = starts(B, centre)
        for k in (1, 10):
            base = ModelPose(pts, torch.zeros(1, 3), torch.tensor([[1.0, 0, 0, 0]]), K, synth.IMG_WIDTH, synth.IMG_HEIGHT, device=dev,
                             occlusion="hpr", occlusion_refresh_every=k)

            def models():
                return [ModelPose.sharing_cloud_of(base, t, q) for t, q in st]
            trans = torch.cat([t for t, _ in st]).to(dev).contiguous()
            quat = torch.cat([q for _, q in st]).to(dev).contiguous()
            optimize_poses(models(), n_opt_steps=k + 1)   # warm-up (scratch buffers, code objects)
            refresh, run = float("inf"), float("inf")
            for _ in range(reps):   # alternating: one refresh alone, then one whole run
                refresh = min(refresh, timed(lambda: base._build_occlusion_rows(trans, quat)))
                ms = models()
                run = min(run, timed(lambda: optimize_poses(ms, n_opt_steps=steps)))
            n_ref = (steps + k - 1) // k
            step = (run - n_ref * refresh) / steps
            row = dict(part="c", cloud=name, n=int(pts.shape[0]), B=B, k=k, steps=steps, run_ms=run, refresh_ms=refresh, refreshes=n_ref,
                       step_ms=step, ms_per_step_amortised=run / steps)
            out.append(row)
            print(f"(c) optimize_poses {name} n={row['n']} B={B} k={k}: run {run:.2f} ms / {steps} steps = {run / steps:.3f} ms per step;"
                  f" refresh {refresh:.3f} ms x {n_ref}; step without refresh {step:.4f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = torch.from_numpy(synth.K_INTRINS)
    rows = []
    parts = args.parts.split(",")
    if "a" in parts:
        rows.append(part_a(dev, K, args.iters, args.reps))
    if "b" in parts:
        rows.append(part_b(dev, K, args.iters, args.reps))
    if "c" in parts:
        rows += part_c(dev, K, min(args.reps, 3))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
