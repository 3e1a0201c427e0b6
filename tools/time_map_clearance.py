"""What the clearance term costs when it asks the MAP ("Clearance from the map"), against the cloud query over the same
map's exported voxel centres, in one process: the 128 waypoints of synth.make_path (and its 127 segments), r = 0.5 m, over the grid of
tools/time_field.py — synth.make_cloud(1 M, seed 0) at voxels of 0.1 m, 405 x 405 x 45 — filled with the first 10 k, 100 k and all
1 M points and with 4 M points of the same slab, so the number of occupied voxels varies over two orders while the box stays.  The
expectation to confirm or refute: the map query scans the bricks within the radius, so it does not grow with the occupied voxels;
the cloud query walks the tile spheres of all of them.  Event-timed, --calls back-to-back raw C calls per repetition, the median and
the minimum of --reps repetitions, in microseconds per call.

    python tools/time_map_clearance.py [--reps 7] [--calls 2000] [--radius 0.5] [--waypoints 128] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from trajectory_optimization_amd import _lib, ops, synth  # noqa: E402
from trajectory_optimization_amd._lib import check, ptr, stream_ptr  # noqa: E402


def timed(call, reps, calls):
    """call(): one raw library call -> its return code.  -> (median, minimum) microseconds per call."""
    check(call(), "the timed call")
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            call()
        b.record()
        b.synchronize()
        per.append(1000.0 * a.elapsed_time(b) / calls)
    return float(np.median(per)), float(min(per))


def case(grid, poses, radius, reps, calls, unknown_plane=None):
    """Both modes over the map and over PackedCloud(the map's exported centres) -> dict of microseconds and hit counts."""
    L, dev, n = _lib.lib(), poses.device, poses.shape[0]
    st = stream_ptr()
    d, idx, s = (torch.empty(n, dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.float32))
    g = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(max(L.tohip_clearance_workspace_bytes(n), L.tohip_clearance_segments_workspace_bytes(n, 1)), dtype=torch.uint8, device=dev)
    head_map = (ptr(grid.buf), ptr(unknown_plane.buf) if unknown_plane is not None else None, grid.buf.numel(), ctypes.byref(grid.geom))
    out = {"occupied_voxels": grid.count()}
    tail_p = (ptr(poses), n, radius, 1.0, ptr(d), ptr(idx), None, ptr(g), 0, ptr(ws), ws.numel(), st)
    tail_s = (ptr(poses), n, 1, radius, 1.0, ptr(d), ptr(idx), ptr(s), None, ptr(g), ptr(ws), ws.numel(), st)
    out["map_point_us"], out["map_point_us_min"] = timed(lambda: L.tohip_clearance_map(*head_map, *tail_p), reps, calls)
    out["map_point_hits"] = int((idx >= 0).sum())
    out["map_segments_us"], out["map_segments_us_min"] = timed(lambda: L.tohip_clearance_map_segments(*head_map, *tail_s), reps, calls)
    out["map_segments_hits"] = int((idx[:n - 1] >= 0).sum())
    if unknown_plane is None:
        cloud = ops.PackedCloud(grid.export()[1])
        head_cloud = (cloud.blob.data_ptr(), cloud.n)
        out["cloud_point_us"], out["cloud_point_us_min"] = timed(lambda: L.tohip_clearance(*head_cloud, *tail_p), reps, calls)
        assert int((idx >= 0).sum()) == out["map_point_hits"]
        out["cloud_segments_us"], out["cloud_segments_us_min"] = timed(lambda: L.tohip_clearance_segments(*head_cloud, *tail_s), reps, calls)
        assert int((idx[:n - 1] >= 0).sum()) == out["map_segments_hits"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--waypoints", type=int, default=128)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(1_000_000, seed=0)).to(dev)
    box = ops.OccupancyGrid.from_points(pts, resolution=0.1)
    poses = torch.from_numpy(synth.make_path(a.waypoints, optical=True, jitter_seed=1)[0]).to(dev).contiguous()
    res = {"grid_dims": list(box.dims), "voxels": int(np.prod(box.dims)), "waypoints": a.waypoints, "radius_m": a.radius, "cases": {}}
    fills = {"10k": pts[:10_000], "100k": pts[:100_000], "1m": pts, "4m": torch.from_numpy(synth.make_cloud(4_000_000, seed=2)).to(dev)}
    for name, rows in fills.items():
        grid = box.empty_like()
        grid.insert(rows)
        res["cases"][name] = case(grid, poses, a.radius, a.reps, a.calls)
    # unknown = 'obstacle' over a map nobody has looked at: every voxel inside dims within the radius is an obstacle — the most a window holds
    res["cases"]["all_unknown"] = case(box.empty_like(), poses, a.radius, a.reps, a.calls, unknown_plane=box.empty_like())
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
