"""What a tour costs (tools.plan_tour: clearance_kernels.hip's edge stage, tour_kernels.hip), in one process, medians of --reps runs:

  (a) edges_segments  the edge stage through tohip_clearance_segments with n_wps = 2: one 16-wave block per edge
  (b) edges_wave      the edge stage through tohip_clearance_edges: one wave per edge
  (c) tour            tohip_tour_plan alone (lengths, Floyd-Warshall, nearest neighbour, 2-opt) on the edge stage's answer
  (d) plan_tour       the whole public call, host copy and walk included (wall clock)

over 1 M synthetic points (synth.make_cloud) and the bundled cloud, for all pairs of n = 33 and n = 257 nodes in (a) and (b) and for
n = 33 and n = 256 — the cap — in (c) and (d).  (a) and (b) are checked to agree bit for bit before they are timed.

    python tools/time_tour.py [--reps 5] [--radius 0.5] [--json out.json]
    python tools/time_tour.py --sweep       # n = 33, 46, 65, 91, 129, 182, 257: where the two edge stages cross
    python tools/time_tour.py --once        # each stage once at n = 256 / 257 on the 1 M cloud: under rocprofv3 --kernel-trace --stats
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
from trajectory_optimization_amd import ops, synth, tools  # noqa: E402


def nodes_over(pts, n, seed, above=False):
    """n nodes spread over the cloud's extent, 1.5 m above its lowest point at least: some legs run through free space, some do not.
    above: from 0.3 m below the cloud's top to 3 m above it instead — for a cloud that fills its box, where no leg inside is open."""
    lo, hi = np.nanmin(pts, axis=0), np.nanmax(pts, axis=0)
    rng = np.random.default_rng(seed)
    P = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    P[:, 2] = hi[2] + rng.uniform(-0.3, 3.0, n) if above else np.maximum(P[:, 2], lo[2] + 1.5)
    return P


def event_ms(fn, reps, calls):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return float(np.median(out))


def wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1000.0 * (time.perf_counter() - t0))
    return float(np.median(out))


def case(name, pts, radius, reps, dev, once=False, above=False, sizes=(33, 257)):
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    res = {"points": int(cloud.n), "radius": radius}
    for n in ((257,) if once else sizes):
        P = torch.from_numpy(nodes_over(pts, n, n, above)).to(dev)
        a = tools.tour_edge_query(cloud, P, radius, "segments")
        b = tools.tour_edge_query(cloud, P, radius, "edges")
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "the two edge stages disagree"
        r = {"edges": n * (n - 1) // 2, "blocked": int((b[1] >= 0).sum())}
        if not once:
            r["edges_segments_ms"] = event_ms(lambda: tools.tour_edge_query(cloud, P, radius, "segments"), reps, 5)
            r["edges_wave_ms"] = event_ms(lambda: tools.tour_edge_query(cloud, P, radius, "edges"), reps, 5)
        res[f"n{n}"] = r
        nt = min(n, ops.TOUR_MAX_NODES)
        Pt = P[:nt].contiguous()
        idx = tools.tour_edge_query(cloud, Pt, radius, "edges")[1]
        buf = ops.tour_plan(Pt, idx)
        hdr = buf[:64].view(torch.int64).cpu().tolist()
        t = {"m": hdr[0], "moves": hdr[1], "converged": hdr[2], "length_m": hdr[3] * ops.TOUR_UNIT, "nn_length_m": hdr[4] * ops.TOUR_UNIT}
        if not once:
            t["tour_ms"] = event_ms(lambda: ops.tour_plan(Pt, idx), reps, 5)
            t["tour_no_moves_ms"] = event_ms(lambda: ops.tour_plan(Pt, idx, False, 0), reps, 5)
            t["plan_tour_ms"] = wall_ms(lambda: tools.plan_tour(cloud, Pt, clearance_radius=radius), reps)
        else:
            tools.plan_tour(cloud, Pt, clearance_radius=radius)
        res[f"tour_n{nt}"] = t
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="n = 33 .. 257 in steps of about sqrt(2): where the two edge stages cross")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = (33, 46, 65, 91, 129, 182, 257) if a.sweep else (33, 257)
    res = {"synthetic_1m": case("synthetic_1m", synth.make_cloud(1_000_000, seed=1), a.radius, a.reps, dev, a.once, True, sizes)}
    if not a.once:
        d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
        res["bundled"] = case("bundled", np.ascontiguousarray(d["pts"], dtype=np.float32), a.radius, a.reps, dev, sizes=sizes)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
