"""What refining a path costs (tools.refine_path: clearance_kernels.hip's edge stage, path_kernels.hip), in one process, medians of
--reps event-timed runs, at L = 128, 512 and 1 024 nodes with a full window (L (L - 1) / 2 chords):

  (a) chords     the chord stage: the admissible slots gathered on the device and put to tohip_clearance_edges
  (b) search     tohip_path_refine without a spacing: the search, the corners and one row per corner
  (c) resample   the same call with a spacing that fills most of the 4 096 rows; (c) - (b) is the emission
  (d) host       synth.path_refine_ref on the same inputs, on the host (wall clock): for scale only
  (e) refine     the whole public call behind plan_tour(via=) at n = 33 views (wall clock, its one read-back included)

over the bundled cloud and 1 M synthetic points (synth.make_cloud).  The walk zigzags over the cloud's footprint at the height of
its top, so that some chords are open and some are not.

    python tools/time_path.py [--reps 5] [--radius 0.5] [--json out.json]
    python tools/time_path.py --once        # each stage once at L = 1 024 on the 1 M cloud: under rocprofv3 --kernel-trace --stats
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
from time_roadmap import lattice_over  # noqa: E402
from time_tour import event_ms, wall_ms  # noqa: E402


def zigzag_over(pts, L):
    """L nodes that sweep the cloud's footprint in rows, every other node offset sideways, at the height of the cloud's top."""
    lo, hi = np.nanmin(pts, axis=0).astype(np.float64), np.nanmax(pts, axis=0).astype(np.float64)
    rows = max(2, int(np.sqrt(L / 8)))
    per = -(-L // rows)
    P = []
    for r in range(rows):
        xs = np.linspace(lo[0], hi[0], per)
        if r % 2:
            xs = xs[::-1]
        y = lo[1] + (hi[1] - lo[1]) * (r + 0.5) / rows
        for k, x in enumerate(xs):
            P.append((x, y + (0.3 if k % 2 else -0.3), hi[2] + (0.2 if k % 3 else -0.2)))
    return np.ascontiguousarray(np.float32(P[:L]))


def case(name, pts, radius, reps, dev, sizes, once=False):
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    res = {"points": int(cloud.n), "radius": radius}
    for L in sizes:
        Pn = zigzag_over(pts, L)
        P = torch.from_numpy(Pn).to(dev)
        W = L - 1
        kept = torch.zeros(L, dtype=torch.bool, device=dev)
        kept[0] = kept[-1] = True
        band = tools._path_chord_band(cloud, P, kept, W, radius)
        length = float(np.linalg.norm(np.diff(Pn.astype(np.float64), axis=0), axis=1).sum())
        h = length / 3000.0   # fewer than 4 096 rows whatever the search shortens
        hdr = ops.path_refine(P, None, kept, band, W, h)[:256].view(torch.int64).cpu().tolist()
        r = {"chords": L * (L - 1) // 2, "open_chords": hdr[5], "corners": hdr[0] + 1, "rows": hdr[1], "length_m": hdr[2] * ops.TOUR_UNIT,
             "input_length_m": hdr[3] * ops.TOUR_UNIT, "status": hdr[4]}
        if not once:
            r["chords_ms"] = event_ms(lambda: tools._path_chord_band(cloud, P, kept, W, radius), reps, 3)
            r["search_ms"] = event_ms(lambda: ops.path_refine(P, None, kept, band, W, None), reps, 5)
            r["resample_ms"] = event_ms(lambda: ops.path_refine(P, None, kept, band, W, h), reps, 5)
            bh = band.cpu().numpy()
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                synth.path_refine_ref(Pn, None, bh, W, h)
                t.append(1000.0 * (time.perf_counter() - t0))
            r["host_restatement_ms"] = float(np.median(t))
            r["refine_path_ms"] = wall_ms(lambda: tools.refine_path(cloud, P, clearance_radius=radius, spacing=h), reps)
        res[f"L{L}"] = r
    # the whole call behind a tour over a lattice
    Qn, _ = lattice_over(pts, 1024)
    Q = torch.from_numpy(Qn).to(dev)
    tour = tools.plan_tour(cloud, Q[:33], clearance_radius=radius, via=Q[33:])
    rp = tools.refine_path(cloud, tour, clearance_radius=radius, spacing=0.5)
    res["tour_n33"] = {"walk_nodes": len(tour.walk_nodes), "corners": len(rp.corners), "rows": int(rp.poses.shape[0]), "walk_length_m": tour.length,
                       "length_m": rp.length, "open_chords": rp.n_open}
    if not once:
        res["tour_n33"]["refine_path_ms"] = wall_ms(lambda: tools.refine_path(cloud, tour, clearance_radius=radius, spacing=0.5), reps)
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
    sizes = (1024,) if a.once else (128, 512, 1024)
    res = {"synthetic_1m": case("synthetic_1m", synth.make_cloud(1_000_000, seed=1), a.radius, a.reps, dev, sizes, a.once)}
    if not a.once:
        d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
        res["bundled"] = case("bundled", np.ascontiguousarray(d["pts"], dtype=np.float32), a.radius, a.reps, dev, sizes)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
