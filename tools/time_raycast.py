"""What a depth scan costs ("Ray casts and depth scans"), in one process: the 405 x 405 x 45 grid of tools/time_los.py
(synth.make_cloud(1 M, seed 0), voxels of 0.1 m) as two worlds of one geometry — the FOG (the 1 M points themselves: 13 % of the
voxels are occupied, a walk ends after a few voxels) and a scanned ROOM (the six faces of the cloud's box: a walk runs to a wall) —
seen from the first 1 and 8 poses of synth.make_path(8, optical=True), limits (1, 15), at 640 x 480 and at the library's default
image size (synth.IMG_WIDTH x IMG_HEIGHT, synth.K_INTRINS).  Medians of --reps event-timed runs after a warm-up.

  scan / scan_planes   tohip_depth_scan without and with a hit and a pass plane (the planes emptied before every timed run is not
                       done: a plane that already holds the bits costs loads only, which is the steady state of a map; the first,
                       cold run is reported as scan_planes_first)
  los                  the yardstick, existing code: tohip_los_segments over the same (t, far) rays with skip (1, 0) — the same
                       walks with a one-byte verdict; scan_over_los is the ratio
  integrate            the composition that into= replaces: the scan with points=True, then SpaceMap.integrate of the rays that
                       reported a point (flags 0 and 1) from their poses
  rays / visits per ray / plane atomics, from the kernel's own counters

    python tools/time_raycast.py [--reps 5] [--json out.json]
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
from time_tour import event_ms  # noqa: E402

LIMITS = (1.0, 15.0)


def room_points(dev, step=0.05):
    """The six faces of the cloud's box [-20, 20] x [-20, 20] x [-2, 2], sampled every `step` metres."""
    ax = [torch.arange(-h, h + step / 2, step, device=dev, dtype=torch.float32) for h in (20.0, 20.0, 2.0)]
    faces = []
    for a in range(3):
        u, v = [ax[b] for b in range(3) if b != a]
        U, V = torch.meshgrid(u, v, indexing="ij")
        for side in (ax[a][0], ax[a][-1]):
            cols = [U.reshape(-1), V.reshape(-1)]
            cols.insert(a, torch.full_like(cols[0], float(side)))
            faces.append(torch.stack(cols, dim=1))
    return torch.cat(faces)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    fog = ops.OccupancyGrid.from_points(pts, resolution=a.voxel)
    room = fog.empty_like()
    room.insert(room_points(dev))
    poses, quats = synth.make_path(8, optical=True)
    P, Q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    cameras = {"640x480": (np.float32([[320.0, 0, 319.5], [0, 320.0, 239.5], [0, 0, 1]]), 640, 480),
               "default": (synth.K_INTRINS, int(synth.IMG_WIDTH), int(synth.IMG_HEIGHT))}
    res = {"grid_dims": list(fog.dims), "limits": list(LIMITS), "fog_voxels": fog.count(), "room_voxels": room.count(), "cases": {}}
    for world_name, world in (("fog", fog), ("room", room)):
        for cam_name, (K, W, H) in cameras.items():
            cam = ops.Camera(K, W, H, *LIMITS)
            for V in (1, 8):
                p, q = P[:V].contiguous(), Q[:V].contiguous()
                stats = torch.zeros(3, dtype=torch.int64, device=dev)
                hit, free = world.empty_like(), world.empty_like()
                a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ops.depth_scan(world, p, q, cam, *LIMITS)   # (warm)
                a0.record()
                voxel, depth, flags, _ = ops.depth_scan(world, p, q, cam, *LIMITS, hit, free, stats=stats)
                b0.record()
                b0.synchronize()
                rays, visits, atomics = (int(v) for v in stats.tolist())
                c = {"pixels": V * W * H, "rays": rays, "visits_per_ray": visits / max(rays, 1), "plane_atomics_first": atomics,
                     "returns": int((flags == 0).sum()), "no_return": int((flags == 1).sum()), "too_near": int((flags == 3).sum()),
                     "skipped": int((flags == 2).sum()), "hit_voxels": hit.count(), "pass_voxels": free.count(),
                     "scan_planes_first_ms": a0.elapsed_time(b0)}
                c["scan_ms"] = event_ms(lambda: ops.depth_scan(world, p, q, cam, *LIMITS), a.reps, 1)
                c["scan_points_ms"] = event_ms(lambda: ops.depth_scan(world, p, q, cam, *LIMITS, points=True), a.reps, 1)
                c["scan_planes_ms"] = event_ms(lambda: ops.depth_scan(world, p, q, cam, *LIMITS, hit, free), a.reps, 1)
                scan = tools.depth_scan(world, p, q, intrins=K, img_width=W, img_height=H, min_dist=LIMITS[0], max_dist=LIMITS[1])
                far = scan.far.reshape(-1, 3)
                org = p[:, None, :].expand(V, H * W, 3).reshape(-1, 3).contiguous()
                los = world.line_of_sight(org, far, skip=(1, 0))
                assert torch.equal(los.view(V, H, W) == 1, flags == 1) and torch.equal(los.view(V, H, W) == 2, flags == 2)
                c["los_ms"] = event_ms(lambda: world.line_of_sight(org, far, skip=(1, 0)), a.reps, 1)
                c["scan_over_los"] = c["scan_ms"] / c["los_ms"]
                c["scan_planes_over_scan"] = c["scan_planes_ms"] / c["scan_ms"]

                def composition():
                    _, _, fl, pp = ops.depth_scan(world, p, q, cam, *LIMITS, points=True)
                    keep = (fl <= 1).reshape(-1)
                    space = ops.SpaceMap(hit, free)   # (the planes of above: already filled, as for scan_planes_ms)
                    space.integrate(org[keep], pp.reshape(-1, 3)[keep])
                c["integrate_ms"] = event_ms(composition, a.reps, 1)
                c["integrate_over_scan_planes"] = c["integrate_ms"] / c["scan_planes_ms"]
                res["cases"][f"{world_name}_{cam_name}_V{V}"] = c
                print(json.dumps({f"{world_name}_{cam_name}_V{V}": c}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
