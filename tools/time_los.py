"""What the 'voxel' occlusion refresh costs beside the two it joins ("Voxel line of sight"), in one process on the
same inputs: ops.occlusion_bits over synth.make_cloud(1 M) x synth.make_path(128, optical=True), limits (1, 15), voxels of 0.1 m.
Medians of --reps event-timed runs after a warm-up.

  refresh      'voxel' (tohip_los_rows, one launch, nothing read back), 'zbuffer' and 'hpr' (cull, one host read, splat or hull,
               bit rows), the two ratios, 'voxel' with prune = 0, the walk's rays and its mean voxels visited per ray
  step         the amortised optimize_trajectory step (--steps steps, wall clock) at occlusion_refresh_every = 1 and 10, per method
  agreement    the share of kept (point, waypoint) pairs on which 'voxel' gives the bit of 'zbuffer' / of 'hpr' (tests/golden/
               bundled.npz): recorded, not asserted — the three methods answer different questions

    python tools/time_los.py [--reps 5] [--steps 20] [--only refresh|step|agreement] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trajectory_optimization_amd import ops, synth  # noqa: E402
from trajectory_optimization_amd.model import ModelTraj  # noqa: E402
from trajectory_optimization_amd.optimizer import optimize_trajectory  # noqa: E402
from time_tour import event_ms, wall_ms  # noqa: E402

LIMITS = (1.0, 15.0)
METHODS = ("voxel", "zbuffer", "hpr")


def refresh(a, dev):
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    poses, quats = synth.make_path(a.waypoints, optical=True)
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    cloud = ops.PackedCloud(pts)
    cam = ops.Camera(torch.from_numpy(synth.K_INTRINS), synth.IMG_WIDTH, synth.IMG_HEIGHT)
    grid = ops.OccupancyGrid.from_points(cloud, resolution=a.voxel)
    res = {"points": int(cloud.n), "waypoints": a.waypoints, "voxel_m": a.voxel, "grid_dims": list(grid.dims),
           "grid_MB": grid.buf.numel() / 2 ** 20, "occupied_voxels": int(grid.dense().sum()) if np.prod(grid.dims) <= 1 << 26 else None}
    res["insert_ms"] = event_ms(lambda: grid.insert(pts), a.reps, 1)
    call = lambda m, **kw: ops.occlusion_bits(cloud, pts, p, q, cam, *LIMITS, method=m, **kw)
    rows = call("voxel", grid=grid)
    assert torch.equal(rows, ops.los_rows(cloud, p, q, cam, *LIMITS, grid, prune=False)), "the prune changed a bit"
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    ops.los_rows(cloud, p, q, cam, *LIMITS, grid, stats=stats)
    rays, visits = (int(v) for v in stats.tolist())
    kept = int(ops.unpack_occlusion_rows(cloud, ops.los_rows(cloud, p, q, cam, *LIMITS, ops.OccupancyGrid(grid.origin, a.voxel, grid.dims, device=dev))).sum())
    res.update(kept_pairs=kept, rays_walked=rays, voxels_visited_per_ray=visits / max(rays, 1), clear_pairs=int(ops.unpack_occlusion_rows(cloud, rows).sum()))
    res["voxel_ms"] = event_ms(lambda: call("voxel", grid=grid), a.reps, 3)
    res["voxel_noprune_ms"] = event_ms(lambda: ops.los_rows(cloud, p, q, cam, *LIMITS, grid, prune=False), a.reps, 3)
    res["voxel_empty_grid_ms"] = event_ms(lambda: ops.los_rows(cloud, p, q, cam, *LIMITS, ops.OccupancyGrid(grid.origin, a.voxel, grid.dims, device=dev)),
                                          a.reps, 1)
    for m in ("zbuffer", "hpr"):
        res[f"{m}_ms"] = event_ms(lambda: call(m), a.reps, 1)
        res[f"{m}_over_voxel"] = res[f"{m}_ms"] / res["voxel_ms"]
    return res


def step(a, dev):
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    poses, quats = synth.make_path(a.waypoints, optical=True)
    K = torch.from_numpy(synth.K_INTRINS)
    base = ModelTraj(pts, torch.from_numpy(poses), torch.from_numpy(quats), K, synth.IMG_WIDTH, synth.IMG_HEIGHT, device=dev)
    grid = ops.OccupancyGrid.from_points(base._cloud, resolution=a.voxel)
    res = {}
    for m in METHODS:
        for every in (1, 10):
            kw = dict(occlusion=m, occlusion_limits=LIMITS, occlusion_refresh_every=every)
            if m == "voxel":
                kw["occlusion_grid"] = grid

            def run():
                model = ModelTraj.sharing_cloud_of(base, torch.from_numpy(poses), torch.from_numpy(quats), **kw)
                return optimize_trajectory(model, n_opt_steps=a.steps, rewards_th=float("inf"), smoothness_th=float("-inf"))
            steps = run().steps_taken
            res[f"{m}_every{every}_step_ms"] = wall_ms(run, max(1, a.reps // 2)) / max(steps, 1)
            res[f"{m}_every{every}_steps"] = steps
    return res


def agreement(a, dev):
    d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
    pts = torch.from_numpy(d["pts"]).to(dev)
    poses, quats = synth.make_path(16, optical=True, scale=0.5)
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    cloud = ops.PackedCloud(pts)
    cam = ops.Camera(torch.from_numpy(synth.K_INTRINS), synth.IMG_WIDTH, synth.IMG_HEIGHT)
    grid = ops.OccupancyGrid.from_points(cloud, resolution=a.voxel)
    empty = ops.OccupancyGrid(grid.origin, a.voxel, grid.dims, device=dev)
    un = lambda rows: ops.unpack_occlusion_rows(cloud, rows) != 0
    kept = un(ops.los_rows(cloud, p, q, cam, *LIMITS, empty))
    vox = un(ops.los_rows(cloud, p, q, cam, *LIMITS, grid))
    res = {"points": int(cloud.n), "waypoints": 16, "kept_pairs": int(kept.sum()), "voxel_visible_share": float(vox[kept].float().mean())}
    for m in ("zbuffer", "hpr"):
        other = un(ops.occlusion_bits(cloud, pts, p, q, cam, *LIMITS, method=m))
        res[f"{m}_visible_share"] = float(other[kept].float().mean())
        res[f"agrees_with_{m}"] = float((other[kept] == vox[kept]).float().mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--waypoints", type=int, default=128)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--only", choices=("refresh", "step", "agreement"), default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for name, fn in (("refresh", refresh), ("step", step), ("agreement", agreement)):
        if a.only in (None, name):
            res[name] = fn(a, dev)
            print(json.dumps({name: res[name]}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
