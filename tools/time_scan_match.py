"""What scan matching costs ("Scan matching"), in one process: the 405 x 405 x 45 grid of the other map timings
(synth.make_cloud(1 M, seed 0)'s box at voxels of 0.1 m) holding the scanned ROOM, seen once by an all-round depth sensor near its
middle — the evidence map the matcher reads — and that scan's first --points returns, in the sensor frame, offered at a prior two
voxels and two yaw steps off: K = 41 headings, window (10, 10, 2), 41 x 2205 = 90 405 candidates.  Medians of --reps windows.

  prepare       ScanMatcher.refresh(): evidence bytes -> score table (event-timed, 10 calls per window)
  correlate     the window search from the table, one launch behind two clears (event-timed, 3 calls per window)
  best          the arg-max over the K S scores, one block (event-timed, 10 calls per window)
  match_scan    tools.match_scan end to end on a kept matcher: host rotations, correlate, best, the winner's counters, one read-back
                and the parabola (wall-clock)
  explicit      the same K S scores by tohip_scan_score over the explicit candidates, from the evidence bytes (event-timed, 1 call);
                asserted equal to correlate's, score for score, before anything is timed
  torch         one rotation's S scores by torch-op gathers on dense(): per shift an index add, a gather and a sum over the points
                (event-timed, 1 call); asserted equal; torch_ms is that time x K

    python tools/time_scan_match.py [--reps 5] [--points 100000] [--json out.json]
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
from time_raycast import room_points  # noqa: E402
from time_tour import event_ms, wall_ms  # noqa: E402

K, WINDOW, HALF_RANGE = 41, (10, 10, 2), np.deg2rad(5.0)
TRUE_T = (0.53, -0.31, 0.04)
SIDE = 160                                     # four SIDE x SIDE views, 90 degrees each: 102 400 rays
PLANTED = (2, -1, 1)


def torch_scores(dense, unknown_value, floor, origin, r, pts, R, t, window):
    """One rotation's window by torch ops: the value volume padded by the window, the points' voxels by torch's own f32 arithmetic
    (asserted against the kernel's by the caller), then per shift one gather and one sum -> (2wz+1, 2wy+1, 2wx+1) int64."""
    wx, wy, wz = window
    V = torch.where(dense == -128, torch.full_like(dense, unknown_value), torch.clamp(dense, min=floor)).long()
    pad = torch.full((dense.shape[0] + 2 * wx, dense.shape[1] + 2 * wy, dense.shape[2] + 2 * wz), unknown_value, dtype=torch.int64, device=dense.device)
    pad[wx:wx + dense.shape[0], wy:wy + dense.shape[1], wz:wz + dense.shape[2]] = V
    w = (R[:, 0] * pts[:, 0:1] + R[:, 1] * pts[:, 1:2]) + R[:, 2] * pts[:, 2:3] + t
    v = torch.floor((w - origin) / r).long()
    ok = ((v >= 0) & (v < torch.tensor(dense.shape, device=dense.device))).all(dim=1)   # (every return of this scan lies inside dims)
    assert bool(ok.all())
    sy, sz = pad.shape[1], pad.shape[2]
    base = ((v[:, 0] + wx) * sy + (v[:, 1] + wy)) * sz + (v[:, 2] + wz)
    flat = pad.reshape(-1)
    out = torch.empty((2 * wz + 1, 2 * wy + 1, 2 * wx + 1), dtype=torch.int64, device=dense.device)
    for dz in range(-wz, wz + 1):
        for dy in range(-wy, wy + 1):
            for dx in range(-wx, wx + 1):
                out[dz + wz, dy + wy, dx + wx] = flat[base + ((dx * sy + dy) * sz + dz)].sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    cloud = torch.from_numpy(synth.make_cloud(1_000_000, seed=0)).to(dev)
    world = ops.OccupancyGrid.from_points(cloud, resolution=a.voxel).empty_like()
    world.insert(room_points(dev))
    emap = ops.EvidenceMap.like(world)
    # the all-round scan at the true pose, folded into the map and kept as the scan to match
    turns = np.stack([[np.cos(h / 2.0), 0.0, 0.0, np.sin(h / 2.0)] for h in np.deg2rad([0.0, 90.0, 180.0, 270.0])])
    quats = synth.quat_mul(turns, synth.Q_OPTICAL).astype(np.float32)
    poses = np.tile(np.float32(TRUE_T), (4, 1))
    f = SIDE / 2.0
    intrins = torch.tensor([[f, 0.0, f - 0.5], [0.0, f, f - 0.5], [0.0, 0.0, 1.0]])
    scan = tools.depth_scan(world, torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev), into=emap, points=True, intrins=intrins,
                            img_width=SIDE, img_height=SIDE, min_dist=0.05, max_dist=40.0)
    hits = scan.points[scan.flags == 0]
    assert hits.shape[0] >= a.points, f"the scan returned {hits.shape[0]} points, fewer than --points"
    pts = (hits[:a.points] - torch.tensor(TRUE_T, device=dev)).contiguous()
    r = float(emap.resolution)
    prior_t = np.asarray(TRUE_T, dtype=np.float64) - r * np.asarray(PLANTED)
    step = HALF_RANGE / (K // 2)
    prior_q = np.array([np.cos(-step), 0.0, 0.0, np.sin(-step)])                        # two yaw steps off
    cands = tools.yaw_candidates(prior_q, HALF_RANGE, K)
    matcher = ops.ScanMatcher(emap)
    S = int(np.prod([2 * w + 1 for w in WINDOW]))
    res = {"grid_dims": list(emap.dims), "voxels": int(np.prod(emap.dims)), "table_MB": matcher.table.numel() / 2 ** 20, "points": a.points,
           "K": K, "window": list(WINDOW), "S": S, "candidates": K * S, "lookups": K * S * a.points}

    scores, used = matcher.correlate(pts, prior_t, cands, WINDOW)
    m = tools.match_scan(matcher, pts, prior_t, prior_q, window=WINDOW, yaw=(HALF_RANGE, K))
    res.update(found_shift=list(m.shift), found_rotation=m.rotation, ties=m.ties, score=m.score, used=m.used, known=m.known)
    assert m.shift == PLANTED and m.rotation == K // 2 + 2, (m.shift, m.rotation)

    # the explicit candidates: equal before anything is timed
    poses12 = matcher.poses(prior_t, cands).repeat_interleave(S, dim=0)
    dz, dy, dx = np.meshgrid(*(np.arange(-w, w + 1) for w in WINDOW[::-1]), indexing="ij")
    shifts = torch.from_numpy(np.tile(np.stack([dx.ravel(), dy.ravel(), dz.ravel()], axis=1), (K, 1)).astype(np.int32)).to(dev)
    explicit = lambda: matcher.score(pts, None, None, shifts=shifts, poses12=poses12)   # noqa: E731
    assert torch.equal(explicit()[0], scores.reshape(-1)), "the explicit candidates and the window search disagree"
    res["explicit_equal"] = True

    k0 = K // 2 + 2
    tR = torch.from_numpy(ops.scan_rotations(cands[k0:k0 + 1])[0]).to(dev)
    tt = torch.tensor(prior_t.astype(np.float32), device=dev)
    dense, origin = emap.dense(), torch.tensor(emap.origin.tolist(), device=dev)
    by_torch = lambda: torch_scores(dense, matcher.unknown_value, matcher.floor, origin, emap.resolution, pts, tR, tt, WINDOW)   # noqa: E731
    assert torch.equal(by_torch(), scores[k0].long()), "the torch gathers and the window search disagree"
    res["torch_equal"] = True

    res["prepare_ms"] = event_ms(matcher.refresh, a.reps, 10)
    res["correlate_ms"] = event_ms(lambda: matcher.correlate(pts, prior_t, cands, WINDOW, poses12=poses12[::S].contiguous()), a.reps, 3)
    res["best_ms"] = event_ms(lambda: matcher.best(scores), a.reps, 10)
    res["match_scan_ms"] = wall_ms(lambda: tools.match_scan(matcher, pts, prior_t, prior_q, window=WINDOW, yaw=(HALF_RANGE, K)), a.reps)
    res["explicit_ms"] = event_ms(explicit, a.reps, 1)
    res["torch_one_rotation_ms"] = event_ms(by_torch, a.reps, 1)
    res["torch_ms"] = res["torch_one_rotation_ms"] * K
    res["correlate_Glookups_per_s"] = res["lookups"] / res["correlate_ms"] / 1e6
    res["explicit_over_correlate"] = res["explicit_ms"] / res["correlate_ms"]
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
