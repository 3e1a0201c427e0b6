"""What free-space carving, the frontier and the listing cost ("Free space and frontiers"), in one process:
synth.make_cloud(1 M, seed 0) as the returns of one scan from one origin, voxels of 0.1 m, the grid of OccupancyGrid.from_points.
Medians of --reps event-timed runs after a warm-up.

  carve_empty     the rays carved into an EMPTY free plane (a fresh plane per run, its allocation outside the timed window): every
                  brick a ray crosses costs a load, and an atomic where a bit is new
  carve_again     the same carve into the plane that already holds every bit — a mapper's steady state: loads only (stats: 0 atomics)
  walk_only       tohip_los_segments over the same rays through an empty grid with skip = (0, 0): the same walk with no stores — the
                  yardstick for what the stores cost
  frontier        tohip_occ_frontier over the two planes (the mask alone, nothing read back)
  export          count + export of the frontier mask and of the free plane (one host read each)
  visits / atomics per ray, from the kernels' own counters

    python tools/time_carve.py [--reps 5] [--points 1000000] [--voxel 0.1] [--max-range M] [--json out.json]
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
from trajectory_optimization_amd import _lib, ops, synth  # noqa: E402
from time_tour import event_ms  # noqa: E402


def timed_ms(setup, fn, reps):
    """Median of `reps` event-timed fn(setup()) runs after one warm-up; setup runs outside the timed window."""
    fn(setup())
    out = []
    for _ in range(reps):
        x = setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(x)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--max-range", type=float, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    origin = torch.zeros(3, device=dev)
    occupied = ops.OccupancyGrid.from_points(pts, resolution=a.voxel)
    res = {"rays": a.points, "voxel_m": a.voxel, "max_range_m": a.max_range, "grid_dims": list(occupied.dims),
           "grid_MB": occupied.buf.numel() / 2 ** 20}

    free = occupied.empty_like()
    stats = torch.zeros(3, dtype=torch.int64, device=dev)
    res["rays_skipped"] = free.carve(origin, pts, a.max_range, stats=stats)
    rays, visits, atomics = (int(v) for v in stats.tolist())
    again = torch.zeros(3, dtype=torch.int64, device=dev)
    free.carve(origin, pts, a.max_range, stats=again)
    assert again.tolist()[:2] == [rays, visits]
    res.update(rays_walked=rays, visits_per_ray=visits / max(rays, 1), atomics_per_ray_empty=atomics / max(rays, 1),
               atomics_per_ray_again=int(again[2]) / max(rays, 1), free_voxels=free.count())

    res["carve_empty_ms"] = timed_ms(occupied.empty_like, lambda g: g.carve(origin, pts, a.max_range), a.reps)
    res["carve_again_ms"] = event_ms(lambda: free.carve(origin, pts, a.max_range), a.reps, 1)
    empty = occupied.empty_like()
    o_rows = origin[None, :].expand(pts.shape[0], 3).contiguous()
    walk = torch.zeros(2, dtype=torch.int64, device=dev)
    empty.line_of_sight(o_rows, pts, skip=(0, 0), stats=walk)
    res["walk_only_visits_per_ray"] = int(walk[1]) / max(int(walk[0]), 1)
    res["walk_only_ms"] = event_ms(lambda: empty.line_of_sight(o_rows, pts, skip=(0, 0)), a.reps, 1)
    res["stores_over_walk_empty"] = res["carve_empty_ms"] / res["walk_only_ms"]
    res["stores_over_walk_again"] = res["carve_again_ms"] / res["walk_only_ms"]

    space = ops.SpaceMap(occupied, free)
    mask = free.empty_like()
    L = _lib.lib()
    res["frontier_ms"] = event_ms(lambda: _lib.check(L.tohip_occ_frontier(_lib.ptr(occupied.buf), _lib.ptr(free.buf), *mask._sizes(), 1, _lib.stream_ptr()),
                                                    "tohip_occ_frontier"), a.reps, 5)
    fr = space.frontier()
    res["frontier_voxels"] = fr.n
    res["frontier_and_export_ms"] = event_ms(lambda: space.frontier(), a.reps, 1)
    res["export_frontier_ms"] = event_ms(lambda: fr.grid.export(), a.reps, 1)
    res["export_free_ms"] = event_ms(lambda: free.export(), a.reps, 1)
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
