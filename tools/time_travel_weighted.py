"""What a weighted travel field costs ("Weighted travel fields"), in one process, over the room of tools/time_travel.py
(405 x 405 x 45 voxels of 0.1 m, two partition walls, the robot of --radius 0.3 m in one corner, a clearance field of D = 5).  Every
figure is the median of --windows windows, each window the median of --reps wall-clock runs; the spread is the smallest and the
largest window.

  unweighted            TravelField.rebuild() without weights, and its rounds
  neutral               the weighted build over kappa = 16 everywhere: the same work plus the kappa traffic and the multiply (the
                        result is compared with the unweighted one bit for bit)
  default               the weighted build over tools.travel_weights(field, radius, --soft-radius), with its rounds
  weights               the gather k_travel_weights alone (event-timed)
  paths                 --paths weighted paths() to random reachable goals
  batch                 --batch fields over the default layer in one build, beside the same batch unweighted
  unweighted_again      the unweighted build once more at the end, against the figure profiles/time_travel.json holds for the parent
                        commit and — with --parent-json, the output of the parent commit's tools/time_travel.py on the same machine —
                        against that run; the margin is the spread of the windows

    python tools/time_travel_weighted.py [--windows 5] [--reps 5] [--paths 1000] [--batch 8] [--parent-json parent.json] [--json out.json]
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
from trajectory_optimization_amd import ops, synth, tools  # noqa: E402
from time_raycast import room_points  # noqa: E402
from time_tour import event_ms, wall_ms  # noqa: E402
from time_travel import partition_points  # noqa: E402


def windows(fn, n_windows, reps, timer=wall_ms):
    """-> {"ms": the median of the windows' medians, "lo": the smallest window, "hi": the largest, "windows": all of them}."""
    w = [float(timer(fn, reps)) for _ in range(n_windows)]
    return {"ms": float(np.median(w)), "lo": min(w), "hi": max(w), "windows": w}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--soft-radius", type=float, default=0.5)
    ap.add_argument("--gain", type=float, default=4.0)
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    grid = ops.OccupancyGrid.from_points(pts, resolution=a.voxel).empty_like()
    grid.insert(room_points(dev))
    grid.insert(partition_points(dev))
    field = ops.ClearanceField(grid, D=max(5, int(np.ceil(a.soft_radius / a.voxel - 1e-9))))   # (5: tools/time_travel.py's field)
    start = torch.tensor([[-18.0, -18.0, 0.0]], device=dev)
    W, R = a.windows, a.reps
    res = {"grid_dims": list(grid.dims), "voxels": int(np.prod(grid.dims)), "radius_m": a.radius, "soft_radius_m": a.soft_radius, "gain": a.gain,
           "field_D": field.D, "windows": W, "reps": R}

    plain = ops.TravelField(field, a.radius, start)
    assert plain.seeded.tolist() == [1]
    res["unweighted_rounds"] = plain.rounds
    res["unweighted"] = windows(plain.rebuild, W, R)

    neutral = ops.TravelField(field, a.radius, start, weights=ops.TravelWeights(field))
    res["neutral_equals_unweighted"] = bool(torch.equal(neutral.buf, plain.buf))
    res["neutral_rounds"] = neutral.rounds
    res["neutral"] = windows(neutral.rebuild, W, R)

    layer = tools.travel_weights(field, a.radius, a.soft_radius, gain=a.gain)
    kappa = layer.dense()
    res["layer_table"] = layer.lut.tolist()
    res["layer_share_above_neutral"] = float((kappa > 16).float().mean())
    res["weights"] = windows(layer.rebuild, W, R, timer=lambda fn, reps: event_ms(fn, reps, 1))
    weighted = ops.TravelField(field, a.radius, start, weights=layer)
    res["default_rounds"] = weighted.rounds
    res["default"] = windows(weighted.rebuild, W, R)
    dense = weighted.dense()
    res["reachable_voxels"] = int((dense >= 0).sum())
    res["reachable_equal"] = bool(torch.equal(dense >= 0, plain.dense() >= 0))

    rng = np.random.default_rng(1)
    lo, hi = np.array([-20.0, -20.0, -2.0]), np.array([20.0, 20.0, 2.0])
    Q = torch.from_numpy(rng.uniform(lo, hi, (8 * a.paths, 3)).astype(np.float32)).to(dev)
    goals = Q[weighted.reachable(Q)][:a.paths].contiguous()
    res["paths"] = int(goals.shape[0])
    res["paths_weighted"] = windows(lambda: weighted.paths(goals), W, R)
    res["paths_unweighted"] = windows(lambda: plain.paths(goals), W, R)
    res["path_rows_mean_weighted"] = float(np.mean([len(p) for p in weighted.paths(goals)]))
    res["path_rows_mean_unweighted"] = float(np.mean([len(p) for p in plain.paths(goals)]))
    # what the layer buys: the smallest clearance along one long route, with and without it
    far = torch.nonzero(dense == dense.max())[0]
    goal = (torch.tensor(grid.origin.tolist(), device=dev) + (far.float() + 0.5) * grid.resolution).reshape(3).cpu()
    for name, tf in (("unweighted", plain), ("weighted", weighted)):
        p = tools.travel_path(tf, goal)
        gap = field.distance(p.poses)
        res[f"far_path_{name}"] = {"rows": int(p.poses.shape[0]), "length_m": p.length, "cost": p.cost, "min_clearance_m": float(gap.min()),
                                   "mean_clearance_m": float(gap[torch.isfinite(gap)].mean())}

    starts = torch.from_numpy(rng.uniform([-19.0, -19.0, -0.5], [19.0, 19.0, 0.5], (a.batch, 3)).astype(np.float32)).to(dev)
    for name, w in (("batch_unweighted", None), ("batch_weighted", layer)):
        tfs = ops.TravelFields(field, a.radius, starts, weights=w)
        res[name] = dict(windows(tfs.rebuild, W, R), fields=a.batch, seeded=int(tfs.seeded.sum()), rounds=tfs.rounds)

    res["unweighted_again"] = windows(plain.rebuild, W, R)
    recorded = os.path.join(REPO, "profiles", "time_travel.json")
    if os.path.exists(recorded):
        with open(recorded) as fh:
            res["parent_recorded_build_rpc16_ms"] = json.load(fh).get("build_rpc16_ms")
    if a.parent_json:
        with open(a.parent_json) as fh:
            res["parent_same_machine_build_rpc16_ms"] = json.load(fh).get("build_rpc16_ms")
    u = res["unweighted"]["ms"]
    res["ratio_neutral"] = res["neutral"]["ms"] / u
    res["ratio_default"] = res["default"]["ms"] / u
    res["ratio_batch"] = res["batch_weighted"]["ms"] / res["batch_unweighted"]["ms"]
    res["ratio_paths"] = res["paths_weighted"]["ms"] / res["paths_unweighted"]["ms"]
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
