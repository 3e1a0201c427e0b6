"""What the evidence map costs ("Evidence map"), in one process: synth.make_cloud(1 M, seed 0) as the returns of one scan
from the origin, voxels of 0.1 m, the grid of OccupancyGrid.from_points (405 x 405 x 45).  Medians of --reps event-timed runs after a
warm-up.

  fold            tohip_evid_fold alone over that scan's two planes (hit: the inserted returns; pass: the carved rays), the planes kept:
                  beside it the time its counted bytes — 8 per brick word, 64 of values and 8 of planes per touched brick — would take
                  at --stream-tbs, the rate a streaming kernel reaches on this chip
  fold_clear      the same with clear_scan (8 more bytes per touched brick; the planes are copied back outside the timed window)
  fold_empty      the fold over two empty planes: the floor of 8 bytes per word
  integrate       EvidenceMap.integrate of the scan beside SpaceMap.integrate of the same scan into a map that already holds it, in the
                  same process: the price of forgetting
  from_space      EvidenceMap.from_space over the SpaceMap holding the scan (allocation and init included)
  log_odds        --queries positions

    python tools/time_evidence.py [--reps 5] [--points 1000000] [--queries 1000000] [--voxel 0.1] [--stream-tbs 6.3] [--json out.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trajectory_optimization_amd import _lib, ops, synth  # noqa: E402
from time_carve import timed_ms  # noqa: E402
from time_tour import event_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts_h = synth.make_cloud(a.points, seed=0)
    pts = torch.from_numpy(pts_h).to(dev)
    origin = torch.zeros(3, device=dev)
    hit = ops.OccupancyGrid.from_points(pts, resolution=a.voxel)   # the scan's hit plane
    pas = hit.empty_like()
    pas.carve(origin, pts)                                         # ... and its pass plane
    m = ops.EvidenceMap.like(hit)
    words = (m.buf.numel() - 256) // 32
    touched = int(((hit.buf[256:].view(torch.int32) | pas.buf[256:].view(torch.int32)) != 0).sum())
    res = {"rays": a.points, "voxel_m": a.voxel, "grid_dims": list(m.dims), "voxels": int(np.prod(m.dims)), "brick_words": words,
           "touched_bricks": touched, "evidence_MB": m.buf.numel() / 2 ** 20, "stream_TBs": a.stream_tbs}

    L = _lib.lib()
    counts = torch.zeros(4, dtype=torch.int64, device=dev)

    def fold(h, p, clear):
        _lib.check(L.tohip_evid_fold(_lib.ptr(m.buf), m.buf.numel(), _lib.ptr(h.buf), _lib.ptr(p.buf), _lib.ptr(m.occupied.buf), _lib.ptr(m.free.buf),
                                     h.buf.numel(), ctypes.byref(m.geom), *m.params, int(clear), _lib.ptr(counts), _lib.stream_ptr()),
                   "tohip_evid_fold")

    fold(hit, pas, False)
    res["first_fold_counts"] = counts.tolist()
    for name, clear, extra in (("fold", False, 0), ("fold_clear", True, 8)):
        nbytes = 8 * words + (72 + extra) * touched
        if clear:
            h2, p2 = hit.empty_like(), hit.empty_like()

            def refill():
                h2.buf.copy_(hit.buf)
                p2.buf.copy_(pas.buf)
                return h2, p2
            ms = timed_ms(refill, lambda hp: fold(hp[0], hp[1], True), a.reps)
        else:
            ms = event_ms(lambda: fold(hit, pas, False), a.reps, 1)
        res[f"{name}_ms"] = ms
        res[f"{name}_bytes"] = nbytes
        res[f"{name}_at_stream_rate_ms"] = nbytes / (a.stream_tbs * 1e12) * 1e3
        res[f"{name}_over_stream_rate"] = ms / res[f"{name}_at_stream_rate_ms"]
    e1, e2 = hit.empty_like(), hit.empty_like()
    res["fold_empty_ms"] = event_ms(lambda: fold(e1, e2, False), a.reps, 1)
    res["fold_empty_at_stream_rate_ms"] = 8 * words / (a.stream_tbs * 1e12) * 1e3

    scan_map = ops.EvidenceMap.like(hit)
    res["evidence_integrate_ms"] = event_ms(lambda: scan_map.integrate(origin, pts), a.reps, 1)
    res["last_counts"] = list(scan_map.last_counts())
    space = ops.SpaceMap(hit.empty_like())
    space.integrate(origin, pts)
    res["space_integrate_ms"] = event_ms(lambda: space.integrate(origin, pts), a.reps, 1)
    res["space_integrate_fresh_ms"] = timed_ms(lambda: ops.SpaceMap(hit.empty_like()), lambda s: s.integrate(origin, pts), a.reps)
    res["from_space_ms"] = event_ms(lambda: ops.EvidenceMap.from_space(space), a.reps, 1)

    rng = np.random.default_rng(1)
    lo, hi = pts_h.min(axis=0), pts_h.max(axis=0)
    Q = torch.from_numpy(rng.uniform(lo, hi, (a.queries, 3)).astype(np.float32)).to(dev)
    res["log_odds_ms"] = event_ms(lambda: scan_map.log_odds(Q), a.reps, 1)
    res["queries"] = a.queries
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
