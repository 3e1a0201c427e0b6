"""What travel fields in batches cost ("Travel fields in batches"), in one process, on tools/time_travel.py's room: the
405 x 405 x 45 grid with the scanned room and its two partitions, radius 0.3 m over a clearance field of D = 5.  The sources are
spread evenly over the voxels a single field reaches from the corner.

  batched / sequential  ops.TravelFields.rebuild() with B = 1, 2, 8 and 64 against B ops.TravelField.rebuild()s one after the other
                        (each with its own workspace, as B separate fields have): wall-clock medians of --reps windows after a warm-
                        up, synchronised, the two alternating window by window.  spread: the range of the sequential leg's windows.
                        Per B: the rounds, the mean and the largest number of (field, tile) items in one round (the worklist's header
                        keeps them), the ratio batched / sequential.
  single                the single build's own time (tools/time_travel.py's number), for the comparison across two library builds
  travel_matrix         tools.travel_matrix at M = 64
  assign_frontiers      4 robots end to end — travel_fields and assign_frontiers — over a map whose far third is unknown
  plan_tour             tools.plan_tour(travel=True) at n = 32 against plan_tour(via=free_nodes(stride=8)), the only stride whose
                        lattice fits the roadmap's 16 384 nodes: times and tour lengths

    python tools/time_travel_batch.py [--reps 7] [--json profiles/time_travel_batch.json] [--only-build B]
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
from time_tour import wall_ms  # noqa: E402
from time_travel import partition_points  # noqa: E402


def window_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0)


def items(ws):
    """(the most items of one round, the items of all rounds) from a worklist's header."""
    h = ws[:32].cpu().view(torch.int32)
    return int(h[5]) & 0xFFFFFFFF, int(ws[24:32].cpu().view(torch.int64)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--only-build", type=int, default=0, help="build one batch of this many fields once and stop (for a kernel trace)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    grid = ops.OccupancyGrid.from_points(pts, resolution=a.voxel).empty_like()
    grid.insert(room_points(dev))
    grid.insert(partition_points(dev))
    field = ops.ClearanceField(grid, D=5)
    start = torch.tensor([[-18.0, -18.0, 0.0]], device=dev)
    single = ops.TravelField(field, a.radius, start)
    dense = single.dense()
    reach = torch.nonzero(dense >= 0)
    origin = torch.tensor(grid.origin.tolist(), device=dev)
    centres = lambda v: (origin + (v.float() + 0.5) * float(np.float32(grid.resolution))).contiguous()   # noqa: E731
    spread_over = lambda n: centres(reach[torch.linspace(0, len(reach) - 1, n).long()])                   # noqa: E731
    res = {"grid_dims": list(grid.dims), "voxels": int(np.prod(grid.dims)), "tiles": ops.travel_tiles(grid.dims), "radius_m": a.radius,
           "reachable_voxels": int(len(reach)), "reps": a.reps, "single_rounds": single.rounds}
    if a.only_build:
        tfs = ops.TravelFields(field, a.radius, spread_over(a.only_build))
        print(json.dumps({"only_build": a.only_build, "rounds": tfs.rounds}), flush=True)
        return
    res["single_build_ms"] = wall_ms(single.rebuild, a.reps)
    most, total = items(single._ws)
    res["single_items_mean"], res["single_items_max"] = total / max(single.rounds, 1), most

    res["batches"] = {}
    for B in (1, 2, 8, 64):
        src = spread_over(B)
        tfs = ops.TravelFields(field, a.radius, src)
        assert bool(tfs.seeded.all())
        alone = [ops.TravelField(field, a.radius, src[b:b + 1]) for b in range(B)]
        assert all(torch.equal(tfs[b].buf, alone[b].buf) for b in range(B))

        def sequential():
            for tf in alone:
                tf.rebuild()

        tfs.rebuild(), sequential()   # the warm-up
        batched_ms, sequential_ms = [], []
        for _ in range(a.reps):
            batched_ms.append(window_ms(tfs.rebuild))
            sequential_ms.append(window_ms(sequential))
        most, total = items(tfs._ws)
        r = {"rounds": tfs.rounds, "sequential_rounds": [tf.rounds for tf in alone][:8], "sequential_rounds_sum": sum(tf.rounds for tf in alone),
             "items_mean": total / max(tfs.rounds, 1), "items_max": most, "batched_ms": float(np.median(batched_ms)),
             "sequential_ms": float(np.median(sequential_ms)), "sequential_spread_ms": float(max(sequential_ms) - min(sequential_ms)),
             "batched_spread_ms": float(max(batched_ms) - min(batched_ms)), "cost_MB": tfs.buf.numel() / 2 ** 20}
        r["ratio"] = r["batched_ms"] / r["sequential_ms"]
        res["batches"][str(B)] = r
        print(json.dumps({B: r}), flush=True)
        del tfs, alone

    # the consumers
    P64 = spread_over(64)
    res["travel_matrix_M64_ms"] = wall_ms(lambda: tools.travel_matrix(field, P64, a.radius), max(3, a.reps // 2))
    free = grid.empty_like()   # everything inside the room with x < 7 m is known free, the far third is unknown
    v = torch.nonzero(torch.ones(grid.dims, dtype=torch.bool, device=dev))
    c = centres(v)
    free.insert(c[(c[:, 0] < 7.0) & (c[:, 0].abs() < 20.0) & (c[:, 1].abs() < 20.0) & (c[:, 2].abs() < 2.0)].contiguous())
    del v, c
    space = ops.SpaceMap(grid, free)
    sfield = ops.ClearanceField(space, D=5)
    robots = torch.tensor([[-18.0, -18.0, 0.0], [-18.0, 10.0, 0.0], [0.0, 0.0, 0.0], [0.0, -15.0, 0.5]], device=dev)

    def assign():
        return tools.assign_frontiers(space, tools.travel_fields(sfield, robots, a.radius, space=space), min_size=8, min_cost=1e-3)

    got = assign()
    res["assign_robots"], res["assign_clusters"], res["assign_goals"] = 4, got.clusters.n, got.goal.tolist()
    res["assign_goal_cost_m"] = got.goal_cost.tolist()
    res["assign_frontiers_ms"] = wall_ms(assign, max(3, a.reps // 2))

    def one_by_one():   # the route that works today: a field and a priced clustering per robot, the rule left to the caller
        return [tools.frontier_clusters(space, min_size=8, travel=tools.travel_field(sfield, robots[b], a.radius, space=space)) for b in range(4)]

    one_by_one()
    res["assign_one_by_one_ms"] = wall_ms(one_by_one, max(3, a.reps // 2))

    views = spread_over(32)
    t = tools.plan_tour(field, views, clearance_radius=a.radius, travel=True)
    res["tour_travel_ms"] = wall_ms(lambda: tools.plan_tour(field, views, clearance_radius=a.radius, travel=True), max(3, a.reps // 2))
    res["tour_travel_length_m"], res["tour_travel_reached"], res["tour_travel_rows"] = t.length, int(len(t.order)), int(t.poses.shape[0])
    res["tour_travel_map_legs"] = int(sum(bool(t.via_flag[u, v]) for u, v in zip(t.walk, t.walk[1:])))
    nodes = field.free_nodes(a.radius, stride=8)
    res["tour_via_nodes"] = nodes.n
    try:
        via = lambda: tools.plan_tour(field, views, clearance_radius=a.radius, via=nodes.points)   # noqa: E731
        t = via()
        res["tour_via_ms"] = wall_ms(via, max(3, a.reps // 2))
        res["tour_via_length_m"], res["tour_via_reached"] = t.length, int(len(t.order))
    except ValueError as e:
        res["tour_via_refused"] = str(e)
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
