"""What coarsening a map costs ("Coarsening maps"), in one process: synth.make_cloud(1 M, seed 0) as the returns of one
scan from the origin, voxels of 0.1 m, the grid of OccupancyGrid.from_points (405 x 405 x 45) — the room of the other map timings.
Medians of --reps event-timed windows of --calls calls each, after a warm-up.  Run it twice and hand both files to --combine for the
spread between the runs.

  evidence_<rule>_f<f>_<offset>_ms   the kernel alone (tohip_evid_coarsen COPY into a destination that holds the source's whole image)
  plane_<rule>_f<f>_<offset>_ms      its plane twin (tohip_occ_coarsen COPY) on the occupied plane
                                     for f = 2, 4, 8, rules cover / max and any / all, a brick-aligned offset (4, -8, 2) and an odd one
                                     (-1, -3, -1)
  floor_ms / plane_floor_ms          tohip_evid_transfer / tohip_occ_transfer COPY over the same source into a box of its own size at an
                                     unaligned shift: the same bytes read, no reduction — the floor the *_over_floor ratios are quoted
                                     against (it also writes as much as it reads, which a coarsening does not)
  *_torch_ms                         the same map by torch ops on the device: dense() -> pad to whole groups -> reshape -> key maximum
                                     -> load(); asserted bit-equal to the kernel's map
  pyramid_ms                         tools.map_pyramid(levels=3) end to end (three launches, nine new buffers)
  merge_fine_ms                      level1.merge_fine(map, 'confident') in place
  fields_fine_ms / fields_level2_ms  tools.clearance_field + tools.travel_field (wall clock, with allocation) over the room of
                                     tools/time_travel.py in the same box and over its level-2 grid, with what each reaches
  reframed_kernel_ms                 EvidenceMap.reframed's kernel as tools/time_resample.py times it; --parent-profile names that
                                     tool's committed output, whose figure is quoted beside it

    python tools/time_coarsen.py [--reps 5] [--calls 50] [--json run1.json]
    python tools/time_coarsen.py --combine run1.json run2.json --json profiles/time_coarsen.json
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
from time_travel import partition_points, room_points  # noqa: E402

UNALIGNED = (7, -5, 1)
OFFSETS = {"aligned": (4, -8, 2), "odd": (-1, -3, -1)}
FACTORS = (2, 4, 8)
U = synth.EVID_UNKNOWN


def coarse_frame(m, f, o):
    """The coarse box that holds the whole image of map m at offset o."""
    dims = tuple(max(-((oa - n) // f), 1) for n, oa in zip(m.dims, o))
    return ops.MapFrame(ops.reframed_origin(m.origin, m.resolution, o), float(np.float32(f * m.resolution)), dims)


def sample_torch(L, dims, f, o, rule, thr):
    """The coarse values of a box of `dims` by torch ops: the dense values padded with -128 to f dims, grouped, reduced by the key."""
    win = torch.full([f * n for n in dims], U, dtype=torch.int16, device=L.device)
    ns = tuple(L.shape)
    to = [slice(max(0, -oa), min(f * n, k - oa)) for oa, n, k in zip(o, dims, ns)]
    frm = [slice(t.start + oa, t.stop + oa) for t, oa in zip(to, o)]
    win[to[0], to[1], to[2]] = L[frm[0], frm[1], frm[2]].to(torch.int16)
    C = win.reshape(dims[0], f, dims[1], f, dims[2], f).permute(0, 2, 4, 1, 3, 5).reshape(*dims, f ** 3)
    if rule == "max":
        return C.amax(dim=-1)
    key = torch.where(C == U, torch.full_like(C, 256), torch.where(C > thr, 640 + C, 128 + C)).amax(dim=-1)
    return torch.where(key > 512, key - 640, torch.where(key == 256, torch.full_like(key, U), key - 128))


def combine(paths, out):
    runs = [json.load(open(p)) for p in paths]
    spread = {k: abs(runs[0][k] - runs[1][k]) / min(runs[0][k], runs[1][k]) for k in runs[0]
              if k.endswith("_ms") and isinstance(runs[0][k], float) and k in runs[1] and min(runs[0][k], runs[1][k]) > 0}
    res = {"runs": runs, "relative_spread_between_runs": spread, "largest_spread": max(spread.values()), "median_spread": float(np.median(list(spread.values())))}
    print(json.dumps({k: res[k] for k in ("largest_spread", "median_spread")}), flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    ap.add_argument("--parent-profile", default=os.path.join(REPO, "profiles", "time_resample.json"))
    ap.add_argument("--combine", nargs=2, default=None)
    a = ap.parse_args()
    if a.combine:
        return combine(a.combine, a.json or os.path.join(REPO, "profiles", "time_coarsen.json"))
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    origin = torch.zeros(3, device=dev)
    m = ops.EvidenceMap.like(ops.OccupancyGrid.from_points(pts, resolution=a.voxel))
    m.integrate(origin, pts)
    L = m.dense()
    res = {"rays": a.points, "voxel_m": a.voxel, "grid_dims": list(m.dims), "voxels": int(np.prod(m.dims)), "evidence_MB": m.buf.numel() / 2 ** 20,
           "known_voxels": int((L != U).sum()), "calls_per_window": a.calls}
    slow = max(a.calls // 10, 1)

    same, plane_same = ops.EvidenceMap.like(m.occupied), m.occupied.empty_like()
    res["floor_ms"] = res["reframed_kernel_ms"] = event_ms(lambda: same._transfer(m, UNALIGNED, "copy", None), a.reps, a.calls)
    res["plane_floor_ms"] = event_ms(lambda: ops._map_call(dev, "tohip_occ_transfer", *m.occupied._sizes(), *plane_same._sizes(), *UNALIGNED, 0, None),
                                     a.reps, a.calls)
    if os.path.exists(a.parent_profile):
        res["reframed_kernel_parent_ms"] = json.load(open(a.parent_profile)).get("reframed_kernel_ms")

    params = dict(zip(("hit", "miss", "lmin", "lmax", "threshold"), m.params))
    for f in FACTORS:
        for tag, o in OFFSETS.items():
            frame = coarse_frame(m, f, o)
            dst = ops.EvidenceMap(frame.origin, frame.resolution, frame.dims, device=dev, **params)
            res[f"dims_f{f}_{tag}"] = list(frame.dims)
            for rule in ("cover", "max"):
                key = f"evidence_{rule}_f{f}_{tag}"
                res[key + "_ms"] = event_ms(lambda: dst._coarsen(m, f, o, rule, "copy", None), a.reps, a.calls)
                res[key + "_over_floor"] = res[key + "_ms"] / res["floor_ms"]
                route = lambda: ops.EvidenceMap(frame.origin, frame.resolution, frame.dims, device=dev, **params).load(   # noqa: E731
                    sample_torch(m.dense(), frame.dims, f, o, rule, m.threshold))
                res[key + "_torch_ms"] = event_ms(route, a.reps, slow)
                res[key + "_torch_over_kernel"] = res[key + "_torch_ms"] / res[key + "_ms"]
                # the kernel and the torch route give the same map
                dst._coarsen(m, f, o, rule, "copy", None)
                old = route()
                assert torch.equal(dst.buf, old.buf) and torch.equal(dst.occupied.buf[256:], old.occupied.buf[256:]) and torch.equal(dst.free.buf[256:], old.free.buf[256:])
            for rule in ("any", "all"):
                key = f"plane_{rule}_f{f}_{tag}"
                res[key + "_ms"] = event_ms(lambda: dst.free._coarsen(m.occupied, f, o, rule, "copy", None), a.reps, a.calls)
                res[key + "_over_floor"] = res[key + "_ms"] / res["plane_floor_ms"]
    res["torch_and_kernel_agree"] = True

    res["pyramid_ms"] = event_ms(lambda: tools.map_pyramid(m, 3), a.reps, slow)
    pyramid = tools.map_pyramid(m, 3)
    res["pyramid_dims"] = [list(p.dims) for p in pyramid]
    level1 = pyramid[1]
    res["merge_fine_ms"] = event_ms(lambda: level1.merge_fine(m, mode="confident"), a.reps, a.calls)
    # planning: tools/time_travel.py's room (walls and partitions in the same box, a robot of 0.3 m in one corner) as a grid, and its
    # level-2 grid (rule 'any': no wall is lost); the scanned cloud above has no free space to travel through
    room = m.occupied.empty_like()
    room.insert(room_points(dev))
    room.insert(partition_points(dev))
    start, radius, max_dist = torch.tensor([[-18.0, -18.0, 0.0]], device=dev), 0.3, 0.5
    fields = lambda g: tools.travel_field(tools.clearance_field(g, max_dist), start, radius)   # noqa: E731
    level2 = tools.map_pyramid(room, 2)[2]
    res["fields_fine_ms"] = wall_ms(lambda: fields(room), a.reps)
    res["fields_level2_ms"] = wall_ms(lambda: fields(level2), a.reps)
    res["fields_fine_over_level2"] = res["fields_fine_ms"] / res["fields_level2_ms"]
    for tag, g in (("fine", room), ("level2", level2)):
        tf = fields(g)
        res[f"fields_{tag}_reachable_voxels"], res[f"fields_{tag}_rounds"] = int((tf.dense() >= 0).sum()), int(tf.rounds)
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
