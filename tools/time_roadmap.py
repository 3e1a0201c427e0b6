"""What a free-space roadmap costs (tools.build_roadmap / plan_tour(via=...): roadmap_kernels.hip, clearance_kernels.hip's edge stage),
in one process, medians of --reps event-timed runs, at M = 1 024, 4 096 and 16 384 nodes, k = 12:

  (a) knn        tohip_roadmap_knn (exact f64 keys, ties by index) beside torch.cdist + topk on the same device and nodes — f32 and
                 approximate, so a yardstick for time only
  (b) edges      the edge stage: tohip_clearance_edges over all M k slots
  (c) routes     ops.roadmap_routes (the batch loop, its read-backs included: wall clock) for S = 1 and S = 256 sources beside
                 scipy.sparse.csgraph.dijkstra on the host over the same open graph
  (d) plan_tour  the whole public call with via= at n = 33 and n = 256 tour nodes (wall clock), M - n lattice nodes behind them

over the bundled cloud and 1 M synthetic points (synth.make_cloud).  The nodes are a lattice over the cloud's footprint, from 0.3 m
below its top to 3 m above it, so that some edges are open and some are not.

    python tools/time_roadmap.py [--reps 5] [--radius 0.5] [--json out.json]
    python tools/time_roadmap.py --once        # each stage once at M = 4 096 on the 1 M cloud: under rocprofv3 --kernel-trace --stats
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
from time_tour import event_ms, wall_ms  # noqa: E402

K = 12


def lattice_over(pts, M):
    """M lattice nodes over the cloud's footprint in three layers around its top: the spacing that gives at least M, cut to M."""
    lo, hi = np.nanmin(pts, axis=0).astype(np.float64), np.nanmax(pts, axis=0).astype(np.float64)
    h = np.sqrt((hi[0] - lo[0]) * (hi[1] - lo[1]) * 3.0 / M)
    while True:
        Q = synth.roadmap_lattice((lo[0], lo[1], hi[2] - 0.3), (hi[0], hi[1], hi[2] - 0.3 + 2.0 * h), h)
        if len(Q) >= M:
            return np.ascontiguousarray(Q[np.random.default_rng(M).permutation(len(Q))[:M]]), h
        h *= 0.97


def host_dijkstra_ms(rm, sources, reps):
    import time
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    u, v, L = synth.roadmap_edges(rm.nbr.cpu().numpy(), rm.length_fixed.cpu().numpy(), rm.open.cpu().numpy())
    M = rm.nodes.shape[0]
    g = csr_matrix((np.maximum(L, 1).astype(np.float64), (u, v)), shape=(M, M))   # (duplicates add up: time only)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dijkstra(g, directed=True, indices=sources)
        out.append(1000.0 * (time.perf_counter() - t0))
    return float(np.median(out))


def case(name, pts, radius, reps, dev, sizes, once=False):
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    res = {"points": int(cloud.n), "radius": radius, "k": K}
    for M in sizes:
        Qn, h = lattice_over(pts, M)
        Q = torch.from_numpy(Qn).to(dev)
        rm = tools.build_roadmap(cloud, Q, radius, k=K)
        r = {"spacing_m": h, "open_edges": rm.n_open, "isolated": int(rm.isolated.sum()), "slots": M * K}
        i = torch.arange(M, device=dev)[:, None].expand(M, K)
        j = torch.where(rm.nbr >= 0, rm.nbr.long(), i)
        a, b = Q[torch.minimum(i, j).reshape(-1)], Q[torch.maximum(i, j).reshape(-1)]
        for S in (1, 256):
            src = np.random.default_rng(S).permutation(M)[:S].tolist()
            routes = rm.routes(src)
            r[f"routes_S{S}_sweeps"] = routes.sweeps
            r[f"routes_S{S}_reached"] = float((routes.D < ops.ROADMAP_INF).float().mean())
            if not once:
                r[f"routes_S{S}_ms"] = wall_ms(lambda: rm.routes(src), reps)
                r[f"host_dijkstra_S{S}_ms"] = host_dijkstra_ms(rm, src, reps)
        if not once:
            r["knn_ms"] = event_ms(lambda: ops.roadmap_knn(Q, K), reps, 5)
            r["cdist_topk_ms"] = event_ms(lambda: torch.cdist(Q, Q).topk(K + 1, dim=1, largest=False), reps, 5)
            r["edges_ms"] = event_ms(lambda: ops.clearance_edges(cloud, a, b, radius), reps, 5)
            r["build_roadmap_ms"] = wall_ms(lambda: tools.build_roadmap(cloud, Q, radius, k=K), reps)
        for n in (33, 256):
            t = tools.plan_tour(cloud, Q[:n], clearance_radius=radius, via=Q[n:])
            r[f"tour_n{n}"] = {"visited": len(t.order), "legs_over_roadmap": int(t.via_flag.sum()) // 2, "walk_nodes": len(t.walk_nodes),
                               "length_m": t.length}
            if not once:
                r[f"tour_n{n}"]["plan_tour_via_ms"] = wall_ms(lambda: tools.plan_tour(cloud, Q[:n], clearance_radius=radius, via=Q[n:]), reps)
                r[f"tour_n{n}"]["plan_tour_ms"] = wall_ms(lambda: tools.plan_tour(cloud, Q[:n], clearance_radius=radius), reps)
        res[f"M{M}"] = r
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = (4096,) if a.once else (1024, 4096, 16384)
    res = {"synthetic_1m": case("synthetic_1m", synth.make_cloud(1_000_000, seed=1), a.radius, a.reps, dev, sizes, a.once)}
    if not a.once:
        d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
        res["bundled"] = case("bundled", np.ascontiguousarray(d["pts"], dtype=np.float32), a.radius, a.reps, dev, sizes)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
