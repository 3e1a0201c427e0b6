"""What resampling a map under a rigid transform costs ("Resampling maps"), in one process: synth.make_cloud(1 M, seed 0)
as the returns of one scan from the origin, voxels of 0.1 m, the grid of OccupancyGrid.from_points (405 x 405 x 45) — the room of the
other map timings.  Medians of --reps event-timed windows of --calls calls each (a fifth as many for COVER), after a warm-up.

  evidence_* / plane_*   the kernel alone (tohip_evid_resample / tohip_occ_resample COPY into a destination of the map's own box) for
                         NEAREST and COVER (planes: ANY) at the identity, at yaw 30 degrees and at a general roll / pitch / yaw, each
                         about the box's centre plus a fraction of a voxel
  reframed_kernel_ms     EvidenceMap.reframed's kernel (tohip_evid_transfer COPY, an unaligned shift) on the same map: the same bytes
                         with no gather, the floor the ratios are quoted against; plane_reframed_kernel_ms its plane twin
  *_torch_ms             the same map by torch ops on the device: index arithmetic in int64, a gather from dense(), load()
  merge_maps_ms          tools.merge_maps of two posed evidence maps end to end (union box, re-frame of the first, resample-merge)
  align_maps_ms          tools.align_maps end to end (export, relocalise_scan over a (16, 16, 0) window and 9 headings, register_scan)

    python tools/time_resample.py [--reps 5] [--calls 50] [--points 1000000] [--voxel 0.1] [--json profiles/time_resample.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trajectory_optimization_amd import ops, synth, tools  # noqa: E402
from time_tour import event_ms  # noqa: E402

UNALIGNED = (7, -5, 1)


def rpy_quat(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = (f(0.5 * a) for a in (roll, pitch, yaw) for f in (math.cos, math.sin))
    return (cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy)


def about_centre(m, quat, shift):
    """The pose that turns the map's box about its own centre and then moves it by `shift` metres."""
    c = np.asarray(m.origin, dtype=np.float64) + 0.5 * float(m.resolution) * np.asarray(m.dims, dtype=np.float64)
    return c - ops.quat_matrix(quat) @ c + np.asarray(shift, dtype=np.float64)


def nearest_torch(m, affine, dims):
    """The NEAREST source values of a box of `dims` by torch ops: u and n in int64, a gather from the dense values."""
    dev = m.device
    a = [int(v) for v in affine]
    i, j, k = (2 * torch.arange(n, device=dev, dtype=torch.int64) + 1 for n in dims)
    n = [(a[3 * r] * i[:, None, None] + a[3 * r + 1] * j[None, :, None] + a[3 * r + 2] * k[None, None, :] + a[9 + r]) >> 20 for r in range(3)]
    inside = torch.ones(dims, dtype=torch.bool, device=dev)
    for r in range(3):
        inside &= (n[r] >= 0) & (n[r] < m.dims[r])
    lin = (n[0].clamp(0, m.dims[0] - 1) * m.dims[1] + n[1].clamp(0, m.dims[1] - 1)) * m.dims[2] + n[2].clamp(0, m.dims[2] - 1)
    return torch.where(inside, m.dense().reshape(-1)[lin.reshape(-1)].reshape(dims), torch.full((), -128, dtype=torch.int8, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    origin = torch.zeros(3, device=dev)
    m = ops.EvidenceMap.like(ops.OccupancyGrid.from_points(pts, resolution=a.voxel))
    m.integrate(origin, pts)
    words = (m.occupied.buf.numel() - 256) // 4
    res = {"rays": a.points, "voxel_m": a.voxel, "grid_dims": list(m.dims), "voxels": int(np.prod(m.dims)), "brick_words": words,
           "evidence_MB": m.buf.numel() / 2 ** 20, "known_voxels": int((m.dense() != -128).sum()), "calls_per_window": a.calls}
    slow = max(a.calls // 5, 1)

    evid_dst, plane_dst = ops.EvidenceMap.like(m.occupied), m.occupied.empty_like()
    res["reframed_kernel_ms"] = event_ms(lambda: evid_dst._transfer(m, UNALIGNED, "copy", None), a.reps, a.calls)
    res["plane_reframed_kernel_ms"] = event_ms(lambda: ops._map_call(dev, "tohip_occ_transfer", *m.occupied._sizes(), *plane_dst._sizes(), *UNALIGNED, 0, None),
                                               a.reps, a.calls)
    r = float(m.resolution)
    transforms = {"identity": ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), "yaw30": (rpy_quat(0.0, 0.0, math.radians(30.0)), (0.37 * r, -0.21 * r, 0.0)),
                  "general": (rpy_quat(0.2, -0.15, 1.1), (0.37 * r, -0.21 * r, 0.43 * r))}
    for tag, (quat, shift) in transforms.items():
        pose = about_centre(m, quat, shift)
        affine = ops.resample_affine(m, m, pose, quat)
        for rule, calls in (("nearest", a.calls), ("cover", slow)):
            ms = event_ms(lambda: evid_dst._resample(m, affine, rule, "copy", None), a.reps, calls)
            res[f"evidence_{rule}_{tag}_ms"] = ms
            res[f"evidence_{rule}_{tag}_over_reframed"] = ms / res["reframed_kernel_ms"]
        for rule, calls in (("nearest", a.calls), ("any", slow)):
            ms = event_ms(lambda: plane_dst._resample(m.occupied, affine, rule, "copy", None), a.reps, calls)
            res[f"plane_{rule}_{tag}_ms"] = ms
            res[f"plane_{rule}_{tag}_over_reframed"] = ms / res["plane_reframed_kernel_ms"]
        gather = event_ms(lambda: nearest_torch(m, affine, m.dims), a.reps, 2)
        whole = event_ms(lambda: ops.EvidenceMap.like(m.occupied).load(nearest_torch(m, affine, m.dims)), a.reps, 2)
        res[f"evidence_nearest_{tag}_torch_gather_ms"], res[f"evidence_nearest_{tag}_torch_ms"] = gather, whole
        res[f"evidence_nearest_{tag}_torch_over_kernel"] = whole / res[f"evidence_nearest_{tag}_ms"]
        # the kernel and the torch route give the same map
        evid_dst._resample(m, affine, "nearest", "copy", None)
        old = ops.EvidenceMap.like(m.occupied).load(nearest_torch(m, affine, m.dims))
        assert torch.equal(evid_dst.buf, old.buf) and torch.equal(evid_dst.occupied.buf[256:], old.occupied.buf[256:]) and torch.equal(evid_dst.free.buf[256:], old.free.buf[256:])
        res[f"evidence_nearest_{tag}_known_voxels"] = int((evid_dst.dense() != -128).sum())
    res["torch_and_kernel_agree"] = True

    # a second robot's map of the same room, in a frame turned by 30 degrees and a fraction of a voxel away
    quat, shift = transforms["yaw30"]
    pose = about_centre(m, quat, shift)
    first = m
    R = ops.quat_matrix(quat)
    inv_q = (quat[0], -quat[1], -quat[2], -quat[3])
    second = m.transformed(-R.T @ pose, inv_q)             # the same room in its own frame: world_second = R^T (world - pose)
    res["second_map_dims"] = list(second.dims)
    res["merge_maps_ms"] = event_ms(lambda: tools.merge_maps([first, second], poses=[(0.0, 0.0, 0.0), pose], quats=[(1.0, 0.0, 0.0, 0.0), quat]), a.reps, slow)
    res["merge_maps_dims"] = list(tools.merge_maps([first, second], poses=[(0.0, 0.0, 0.0), pose], quats=[(1.0, 0.0, 0.0, 0.0), quat]).dims)
    matcher = ops.ScanMatcher(first)
    prior_q = rpy_quat(0.0, 0.0, math.radians(30.0) + 0.1)
    prior_t = pose + (3 * r, -2 * r, 0.0)
    align = lambda: tools.align_maps(matcher, second, prior_t, prior_q, window=(16, 16, 0), yaw=(0.2, 9), dof="xyw")   # noqa: E731
    res["align_maps_ms"] = event_ms(align, a.reps, 1)
    got = align()
    res["align_maps_scan_points"] = int(second.occupied.count())
    res["align_maps_pose_error_voxels"] = (np.abs(got.pose - pose) / r).tolist()
    res["align_maps_yaw_error_rad"] = abs(math.remainder(2.0 * math.atan2(got.quat[3], got.quat[0]) - math.radians(30.0), 2.0 * math.pi))
    res["align_maps_status"] = got.status
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
