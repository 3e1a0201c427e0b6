"""What scan registration costs ("Scan registration"), in one process: the room and the scan of tools/time_scan_match.py —
the 405 x 405 x 45 grid at voxels of 0.1 m, seen once by an all-round depth sensor near its middle, and that scan's first --points
returns in the sensor frame — offered at poses a fraction of a voxel and of a degree off the truth.  Medians of --reps windows.

  normal        ScanMatcher.normal at B = 1, 8, 64 poses: one clear and one launch; eight gathers and 28 products per point and pose
                (event-timed, 200 calls per window)
  score         ScanMatcher.score at the same B: one gather per point and pose, the floor for this access pattern (event-timed, 200)
  step          ScanMatcher.step at B = 64 on the records of those poses, with the clones of the state and the poses it writes
                (event-timed, 200 calls per window; clone: the two clones alone)
  register      ScanMatcher.register at B = 1 and 8, 30 iterations with tolerances of 0 — no pose freezes as converged, every
                iteration does its work unless a pose stalls — launches only (event-timed, 10 calls per window)
  register_scan tools.register_scan end to end at B = 1, 30 iterations: the copy of the start, 30 x (clear, normal, step), one
                read-back and the host's covariance (wall-clock)
  torch         one iteration's normal equations for ONE pose restated in torch ops — the eight corner gathers on dense(), the
                weights, J and the 6 x 6 products in int64 — for scale (event-timed, 1 call); whether it equals the kernel's record
                is recorded before anything is timed

    python tools/time_scan_register.py [--reps 5] [--points 100000] [--json out.json]
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
from time_scan_match import SIDE, TRUE_T  # noqa: E402
from time_tour import event_ms, wall_ms  # noqa: E402

BATCHES = (1, 8, 64)


def torch_record(dense, unknown_value, floor, origin, r, pts, pose12):
    """One pose's record by torch ops -> (32,) int64: the definitions of DESIGN.md 10 "Scan registration" on the dense volume; the
    points' fixed-point coordinates by torch's own f32 arithmetic (the caller asserts the result against the kernel's)."""
    dev = dense.device
    T = torch.where(dense == -128, torch.full_like(dense, unknown_value), torch.clamp(dense, min=floor)).long() + 128
    R, t = pose12[:9].reshape(3, 3), pose12[9:]
    w = (R[:, 0] * pts[:, 0:1] + R[:, 1] * pts[:, 1:2]) + R[:, 2] * pts[:, 2:3] + t
    r = torch.full((), float(r), dtype=torch.float32, device=dev)   # (a tensor: torch divides by a Python scalar through its reciprocal)
    q = torch.floor(((w - origin) / r) * 256.0).long()
    qt = torch.floor(((t - origin) / r) * 256.0).long()
    c = q - 128
    b, f = c >> 8, c & 255
    dims = torch.tensor(dense.shape, device=dev)
    wts = [torch.stack([256 - f[:, k], f[:, k]]) for k in range(3)]
    V = {}
    inside = torch.ones(len(pts), dtype=torch.bool, device=dev)
    for i in range(2):
        for j in range(2):
            for k in range(2):
                v = b + torch.tensor([i, j, k], device=dev)
                ok = ((v >= 0) & (v < dims)).all(dim=1)
                vc = torch.minimum(torch.clamp(v, min=0), dims - 1)
                V[i, j, k] = torch.where(ok, T[vc[:, 0], vc[:, 1], vc[:, 2]], torch.full_like(vc[:, 0], 128 + unknown_value))
                inside &= ok
    M24 = sum(V[i, j, k] * wts[0][i] * wts[1][j] * wts[2][k] for i in range(2) for j in range(2) for k in range(2))
    G = torch.stack([sum(wts[1][j] * wts[2][k] * (V[1, j, k] - V[0, j, k]) for j in range(2) for k in range(2)),
                     sum(wts[0][i] * wts[2][k] * (V[i, 1, k] - V[i, 0, k]) for i in range(2) for k in range(2)),
                     sum(wts[0][i] * wts[1][j] * (V[i, j, 1] - V[i, j, 0]) for i in range(2) for j in range(2))], dim=1)
    e = (255 * (1 << 24) - M24 + (1 << 11)) >> 12
    g = (G + 128) >> 8
    a = (q - qt + 32) >> 6
    cr = torch.stack([a[:, 1] * g[:, 2] - a[:, 2] * g[:, 1], a[:, 2] * g[:, 0] - a[:, 0] * g[:, 2], a[:, 0] * g[:, 1] - a[:, 1] * g[:, 0]], dim=1)
    J = torch.cat([g, (cr + (1 << 11)) >> 12], dim=1)
    iu = torch.triu_indices(6, 6, device=dev)
    out = torch.zeros(32, dtype=torch.int64, device=dev)
    out[:21] = (J[:, iu[0]] * J[:, iu[1]]).sum(dim=0)
    out[21:27] = (J * e[:, None]).sum(dim=0)
    out[27], out[28], out[29] = (e * e).sum(), len(pts), inside.sum()
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
    matcher = ops.ScanMatcher(emap)
    rng = np.random.default_rng(0)
    B = max(BATCHES)
    start_t = np.asarray(TRUE_T, dtype=np.float64) + r * rng.uniform(-0.4, 0.4, (B, 3))
    h = 0.5 * np.deg2rad(rng.uniform(-0.5, 0.5, (B, 3)))
    start_q = np.concatenate([np.ones((B, 1)), h], axis=1)
    res = {"grid_dims": list(emap.dims), "voxels": int(np.prod(emap.dims)), "table_MB": matcher.table.numel() / 2 ** 20, "points": a.points,
           "iterations": 30}

    # what the registration does with these starts, and the torch restatement of one record: before anything is timed
    out = tools.register_scan(matcher, pts, start_t[:8], start_q[:8])
    res["statuses"] = [o.status for o in out]
    res["iterations_run"] = [o.iterations for o in out]
    res["end_error_voxels"] = [float(np.abs(o.pose - np.asarray(TRUE_T)).max() / r) for o in out]
    res["end_error_degrees"] = [float(np.rad2deg(2.0 * np.arccos(min(1.0, abs(o.quat[0]))))) for o in out]
    res["start_error_voxels"] = [float(np.abs(t - np.asarray(TRUE_T)).max() / r) for t in start_t[:8]]
    poses12 = matcher.poses(start_t, start_q)
    dense, origin = emap.dense(), torch.tensor(emap.origin.tolist(), device=dev)
    by_torch = lambda: torch_record(dense, matcher.unknown_value, matcher.floor, origin, emap.resolution, pts, poses12[0])   # noqa: E731
    records = matcher.normal(pts, poses12=poses12)
    res["torch_equal"] = bool(torch.equal(by_torch(), records[0]))   # (torch's own f32 transform: recorded, not asserted)

    for b in BATCHES:
        p12 = poses12[:b].contiguous()
        res[f"normal_B{b}_ms"] = event_ms(lambda: matcher.normal(pts, poses12=p12), a.reps, 200)
        res[f"score_B{b}_ms"] = event_ms(lambda: matcher.score(pts, None, None, poses12=p12), a.reps, 200)
        res[f"normal_over_score_B{b}"] = res[f"normal_B{b}_ms"] / res[f"score_B{b}_ms"]
        res[f"normal_B{b}_Gpoints_per_s"] = b * a.points / res[f"normal_B{b}_ms"] / 1e6
    st, _ = ops.scan_register_start(start_t, start_q)
    st = torch.from_numpy(st).to(dev)
    res["step_B64_ms"] = event_ms(lambda: matcher.step(records, st.clone(), poses12.clone()), a.reps, 200)
    res["clone_B64_ms"] = event_ms(lambda: (st.clone(), poses12.clone()), a.reps, 200)
    for b in (1, 8):
        sb, pb = st[:b].contiguous(), poses12[:b].contiguous()
        res[f"register_B{b}_ms"] = event_ms(lambda: matcher.register(pts, iterations=30, tol_t=0.0, tol_r=0.0, state=sb, poses12=pb), a.reps, 10)
        res[f"register_B{b}_iterations_run"] = [int(v) for v in matcher.register(pts, iterations=30, tol_t=0.0, tol_r=0.0, state=sb, poses12=pb)[:, 15].cpu()]
    res["register_scan_ms"] = wall_ms(lambda: tools.register_scan(matcher, pts, start_t[0], start_q[0]), a.reps)
    res["torch_one_record_ms"] = event_ms(by_torch, a.reps, 1)
    res["torch_over_normal_B1"] = res["torch_one_record_ms"] / res["normal_B1_ms"]
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
