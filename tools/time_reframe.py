"""What re-framing and merging maps cost ("Re-framing and merging maps"), in one process: synth.make_cloud(1 M, seed 0) as
the returns of one scan from the origin, voxels of 0.1 m, the grid of OccupancyGrid.from_points (405 x 405 x 45) — the room of the
other map timings.  Medians of --reps event-timed windows of --calls calls each, after a warm-up.

  plane / space / evidence, aligned and unaligned
                  the kernel alone (tohip_occ_transfer / tohip_evid_transfer COPY into a destination that exists) and the public
                  method (.reframed(): allocation and init of the new map included), for a brick-aligned shift and for one that is
                  unaligned on every axis.  Beside each kernel: the bytes it must move — every source word or brick read once, every
                  destination word or brick written once, the two derived words of an evidence brick — and the share of --hbm-tbs
                  (the chip's peak) and of --stream-tbs (what a streaming copy reaches on it) that the measured time amounts to.
  merge_confident / merge_add
                  EvidenceMap.merge of a map one unaligned shift away (the destination is read as well: 32 more bytes per brick)
  *_old_ms        the only route there was before, in the same process: dense() -> slice or combine with torch ops -> a new map ->
                  insert of the set voxels' centres (a plane) or load() (evidence)

    python tools/time_reframe.py [--reps 5] [--calls 200] [--points 1000000] [--voxel 0.1] [--json profiles/time_reframe.json]
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
from time_tour import event_ms  # noqa: E402

ALIGNED, UNALIGNED = (8, -4, 2), (7, -5, 1)


def window(src, shift, fill):
    """The old route's slice: a dense tensor of src's shape, voxel v = src[v + shift] inside, `fill` elsewhere."""
    out = torch.full_like(src, fill)
    to, frm = [], []
    for n, s in zip(src.shape, shift):
        lo, hi = max(0, -s), min(n, n - s)
        to.append(slice(lo, hi))
        frm.append(slice(lo + s, hi + s))
    out[tuple(to)] = src[tuple(frm)]
    return out


def plane_old(g, shift):
    """A plane re-framed without the kernel: dense() -> slice -> a new grid -> insert of the set voxels' centres."""
    bits = window(g.dense(), shift, False)
    origin = ops.reframed_origin(g.origin, g.resolution, shift)
    out = ops.OccupancyGrid(origin, g.resolution, g.dims, device=g.device)
    centres = torch.from_numpy(origin).to(g.device) + (torch.nonzero(bits).to(torch.float32) + 0.5) * g.resolution
    out.insert(centres)
    return out


def evidence_old(m, shift):
    out = ops.EvidenceMap(ops.reframed_origin(m.origin, m.resolution, shift), m.resolution, m.dims, *m.params, device=m.device)
    return out.load(window(m.dense(), shift, -128))


def merge_old(a, b, shift, mode):
    """a.merge(b, mode) without the kernel: both dense, the combine in torch, load()."""
    _, _, lmin, lmax, _ = a.params
    D, S = a.dense().to(torch.int64), window(b.dense(), shift, -128).to(torch.int64)
    known = S != -128
    if mode == "add":
        new = torch.where(known, (torch.where(D == -128, 0, D) + S).clamp(lmin, lmax), D)
    else:
        C = torch.where(known, S.clamp(lmin, lmax), S)
        key = lambda L: torch.where(L == -128, -1, 2 * L.abs() + (L > 0))   # noqa: E731
        new = torch.where(key(C) > key(D), C, D)
    return a.load(new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    origin = torch.zeros(3, device=dev)
    m = ops.EvidenceMap.like(ops.OccupancyGrid.from_points(pts, resolution=a.voxel))
    m.integrate(origin, pts)
    space = ops.SpaceMap(m.occupied, m.free)
    words = (m.occupied.buf.numel() - 256) // 4
    res = {"rays": a.points, "voxel_m": a.voxel, "grid_dims": list(m.dims), "voxels": int(np.prod(m.dims)), "brick_words": words,
           "plane_KB": m.occupied.buf.numel() / 1024, "evidence_MB": m.buf.numel() / 2 ** 20, "known_voxels": int((m.dense() != -128).sum()),
           "hbm_TBs": a.hbm_tbs, "stream_TBs": a.stream_tbs, "calls_per_window": a.calls, "shifts": {"aligned": ALIGNED, "unaligned": UNALIGNED}}

    def rate(name, ms, nbytes):
        res[f"{name}_ms"] = ms
        res[f"{name}_bytes"] = nbytes
        res[f"{name}_share_of_hbm_peak"] = nbytes / (a.hbm_tbs * 1e12) / (ms * 1e-3)
        res[f"{name}_share_of_stream_rate"] = nbytes / (a.stream_tbs * 1e12) / (ms * 1e-3)

    plane_dst, evid_dst = m.occupied.empty_like(), ops.EvidenceMap.like(m.occupied)
    for tag, shift in (("aligned", ALIGNED), ("unaligned", UNALIGNED)):
        rate(f"plane_{tag}_kernel", event_ms(lambda: ops._map_call(dev, "tohip_occ_transfer", *m.occupied._sizes(), *plane_dst._sizes(), *shift, 0, None),
                                             a.reps, a.calls), 8 * words)
        rate(f"evidence_{tag}_kernel", event_ms(lambda: evid_dst._transfer(m, shift, "copy", None), a.reps, a.calls), 72 * words)
        res[f"plane_{tag}_reframed_ms"] = event_ms(lambda: m.occupied.reframed(shift=shift), a.reps, a.calls)
        res[f"space_{tag}_reframed_ms"] = event_ms(lambda: space.reframed(shift=shift), a.reps, a.calls)
        res[f"evidence_{tag}_reframed_ms"] = event_ms(lambda: m.reframed(shift=shift), a.reps, a.calls)
        res[f"plane_{tag}_old_ms"] = event_ms(lambda: plane_old(m.occupied, shift), a.reps, 1)
        res[f"space_{tag}_old_ms"] = event_ms(lambda: (plane_old(space.occupied, shift), plane_old(space.free, shift)), a.reps, 1)
        res[f"evidence_{tag}_old_ms"] = event_ms(lambda: evidence_old(m, shift), a.reps, 1)
        # the new route and the old one give the same map
        new, old = m.reframed(shift=shift), evidence_old(m, shift)
        assert torch.equal(new.buf, old.buf) and torch.equal(new.occupied.buf[256:], old.occupied.buf[256:]) and torch.equal(new.free.buf[256:], old.free.buf[256:])
        assert torch.equal(m.occupied.reframed(shift=shift).buf[256:], plane_old(m.occupied, shift).buf[256:])

    # a second robot's map of the same room, one unaligned shift away, from the scan's other half
    other = ops.EvidenceMap(ops.reframed_origin(m.origin, m.resolution, UNALIGNED), m.resolution, m.dims, *m.params, device=dev)
    other.integrate(origin, pts[a.points // 2:])
    target = ops.EvidenceMap.like(m.occupied)
    target.integrate(origin, pts[:a.points // 2])
    shift = ops.check_merge(target, other, "add")[0]
    # (ADD moves the target at every call and CONFIDENT after the first does not; the traffic is the same: every overlapped brick is
    # read twice and written once)
    for mode in ("confident", "add"):
        rate(f"merge_{mode}", event_ms(lambda: target.merge(other, mode=mode), a.reps, a.calls), 104 * words)
        res[f"merge_{mode}_old_ms"] = event_ms(lambda: merge_old(target, other, shift, mode), a.reps, 1)
    x, y = ops.EvidenceMap.like(m.occupied), ops.EvidenceMap.like(m.occupied)
    for t in (x, y):
        t.integrate(origin, pts[:a.points // 2])
    for mode in ("confident", "add"):
        x.merge(other, mode=mode)
        merge_old(y, other, shift, mode)
        assert torch.equal(x.buf, y.buf) and torch.equal(x.occupied.buf[256:], y.occupied.buf[256:]) and torch.equal(x.free.buf[256:], y.free.buf[256:])
    res["old_and_new_routes_agree"] = True
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
