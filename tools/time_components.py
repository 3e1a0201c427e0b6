"""What connected components cost ("Connected components"), in one process: tools/time_travel.py's room — the 405 x 405
x 45 grid at 0.1 m holding the six faces and the two partition walls — scanned from the robot's corner: every wall point within
--max-range metres is a ray that carves the free plane.  Three planes of that map are labelled at connectivity 26:

  frontier       space.frontier().grid: sparse, many components
  occupied       the walls
  known_free     free and not occupied: millions of voxels in a few components — the worst case for the propagation distance; its
                 round count is reported

  build_ms       Components.rebuild() — the count of set bits that sizes roots, init, the worklist rounds and their read-backs, the
                 ordered roots, the relabel and the stats — wall-clock medians of --reps runs after a warm-up
  scipy_ms / transfer_ms   scipy.ndimage.label over plane.dense() on the host, and the device -> host copy it needs, separately
  sweeps_ms      the same fixed point by whole-grid sweeps of shifted minima in torch ops on the device (a convergence test every 16
                 sweeps), once; the roots are compared with the build's
  stats / min_over a travel field / --lookups at() queries (event-timed), and tools.frontier_clusters end to end (wall-clock)

    python tools/time_components.py [--reps 5] [--lookups 1000000] [--json profiles/time_components.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trajectory_optimization_amd import ops, synth, tools  # noqa: E402
from time_raycast import room_points  # noqa: E402
from time_tour import event_ms, wall_ms  # noqa: E402
from time_travel import _shift, partition_points  # noqa: E402


def torch_sweeps(plane, connectivity, check_every=16):
    """The root of every set voxel of plane (nx,ny,nz bool, on the device) by whole-grid sweeps -> (roots sorted, sweeps)."""
    nx, ny, nz = plane.shape
    big = (1 << 31) - 1
    x, y, z = torch.meshgrid(*[torch.arange(n, device=plane.device, dtype=torch.int32) for n in plane.shape], indexing="ij")
    lab = torch.where(plane, (z * ny + y) * nx + x, torch.full_like(x, big))
    offsets = synth.components_offsets(connectivity)
    sweeps = 0
    while True:
        before = lab.clone()
        for _ in range(check_every):
            for d in offsets:
                lab = torch.where(plane, torch.minimum(lab, _shift(lab, d, big)), lab)
            sweeps += 1
        if torch.equal(lab, before):
            break
    return torch.unique(lab[plane]), sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--lookups", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--max-range", type=float, default=25.0)
    ap.add_argument("--connectivity", type=int, default=26)
    ap.add_argument("--no-sweeps", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    c = a.connectivity
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    grid = ops.OccupancyGrid.from_points(pts, resolution=a.voxel).empty_like()
    walls = torch.cat([room_points(dev), partition_points(dev)])
    grid.insert(walls)
    space = ops.SpaceMap(grid)
    start = torch.tensor([[-18.0, -18.0, 0.0]], device=dev)
    space.free.carve(start[0], walls, a.max_range)
    frontier = space.frontier()
    known_free = grid.empty_like()
    known_free.buf[256:].view(torch.int32).copy_(space.free.buf[256:].view(torch.int32) & ~grid.buf[256:].view(torch.int32))
    res = {"grid_dims": list(grid.dims), "voxels": int(np.prod(grid.dims)), "connectivity": c, "max_range_m": a.max_range, "reps": a.reps,
           "planes": {}}

    comps = {}
    for name, plane in (("frontier", frontier.grid), ("occupied", grid), ("known_free", known_free)):
        comp = ops.Components(plane, c)
        comps[name] = comp
        p = {"set_voxels": plane.count(), "components": comp.n, "rounds": comp.rounds, "largest": int(comp.sizes.max()) if comp.n else 0,
             "labels_MB": comp._buf.numel() / 2 ** 20, "build_ms": wall_ms(comp.rebuild, a.reps)}
        comp.rounds_per_check = 64
        p["build_rpc64_ms"] = wall_ms(comp.rebuild, a.reps)
        comp.rounds_per_check = 16
        comp.rebuild()
        p["stats_ms"] = event_ms(lambda: ops._map_call(dev, "tohip_components_stats", *comp._labels(), comp.n, ops.ptr(comp.sizes), ops.ptr(comp.sums),
                                                       ops.ptr(comp.bbox)), a.reps, 1)
        dense = plane.dense()
        if not a.no_scipy:
            from scipy import ndimage
            p["transfer_ms"] = wall_ms(lambda: dense.cpu(), a.reps)
            host = dense.cpu().numpy()
            structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[c])
            p["scipy_ms"] = wall_ms(lambda: ndimage.label(host, structure=structure), a.reps)
            p["scipy_components"] = int(ndimage.label(host, structure=structure)[1])
        if not a.no_sweeps:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            roots, sweeps = torch_sweeps(dense, c)
            torch.cuda.synchronize()
            p["sweeps_ms"], p["sweeps"] = (time.perf_counter() - t0) * 1e3, sweeps
            p["sweeps_equal"] = bool(torch.equal(roots.to(torch.int32), comp.roots))
            del roots
        del dense
        res["planes"][name] = p
        print(json.dumps({name: p}), flush=True)

    # the queries, on the frontier's components
    comp = comps["frontier"]
    field = ops.ClearanceField(space, D=5)
    tf = ops.TravelField(field, a.radius, start, space=space)
    res["travel_rounds"], res["travel_reachable_voxels"] = tf.rounds, int((tf.dense() >= 0).sum())
    res["min_over_ms"] = event_ms(lambda: comp.min_over(tf), a.reps, 1)
    value, _ = comp.min_over(tf)
    res["frontier_components_reachable"] = int((value >= 0).sum())
    rng = np.random.default_rng(1)
    Q = torch.from_numpy(rng.uniform([-20.0, -20.0, -2.0], [20.0, 20.0, 2.0], (a.lookups, 3)).astype(np.float32)).to(dev)
    res["lookups"], res["lookups_ms"] = a.lookups, event_ms(lambda: comp.at(Q), a.reps, 1)
    res["frontier_clusters_ms"] = wall_ms(lambda: tools.frontier_clusters(space, min_size=4, travel=tf), a.reps)
    fc = tools.frontier_clusters(space, min_size=4, travel=tf)
    res["clusters_kept"], res["clusters_reachable"] = fc.n, int(fc.reachable.sum())
    res["nearest_cluster"] = {"size": int(fc.sizes[0]), "cost_m": float(fc.cost[0])} if fc.n else None
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
