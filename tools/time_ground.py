"""What the ground layer costs ("Ground layer"), in one process: the 405 x 405 x 45 grid of tools/time_travel.py
(synth.make_cloud(1 M, seed 0)'s box at voxels of 0.1 m) holding the scanned ROOM — its floor, walls and ceiling — with a mezzanine
1.5 m above the floor over a third of it and a solid 1 : 1 ramp that leads up to it.  The robot is 0.5 m tall (H = 5), climbs one
voxel (s = 1) and has --radius 0.3 m.  Medians of --reps windows.

  build                 GroundLayer.rebuild(): four header clears and three launches (event-timed, 10 calls per window)
  torch                 the same four planes by whole-grid torch ops on dense bool volumes on the device, in the same process; the
                        planes are asserted equal, bit for bit, before anything is timed
  snap                  --rows positions over the box to their standing voxels (event-timed)
  field / travel        ClearanceField.rebuild() and TravelField.rebuild() over the layer (obstacles; obstacles + drive) beside the
                        plain ones over the same map (wall-clock: the travel build reads back once per 16 rounds)

    python tools/time_ground.py [--reps 5] [--rows 1000000] [--json out.json]
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

H, STEP = 5, 1
RISE = 15                                    # voxels from the room's floor to the mezzanine's slab
MEZZ = (slice(250, 400), slice(50, 350))     # the mezzanine's columns
RAMP_X, RAMP_Y = (235, 250), slice(150, 200)  # the ramp rises one voxel per voxel along x, up to the mezzanine


def furniture(grid, floor_z):
    """The mezzanine and the ramp over the floor's voxel level floor_z, as voxel centres (N,3) f32 on the grid's device."""
    bits = torch.zeros(grid.dims, dtype=torch.bool, device=grid.device)
    bits[MEZZ[0], MEZZ[1], floor_z + RISE] = True
    for x in range(*RAMP_X):
        bits[x, RAMP_Y, floor_z + 1:floor_z + 2 + (x - RAMP_X[0])] = True
    ijk = torch.nonzero(bits).float()
    return torch.tensor(grid.origin.tolist(), device=grid.device) + (ijk + 0.5) * grid.resolution


def _up(a, k, fill):
    """out[..., z] = a[..., z + k] where z + k lies inside, else fill."""
    out = torch.full_like(a, fill)
    n = a.shape[2]
    if abs(k) < n:
        out[:, :, max(-k, 0):n + min(-k, 0)] = a[:, :, max(k, 0):n + min(k, 0)]
    return out


def _side(a, dx, dy):
    out = torch.zeros_like(a)
    nx, ny = a.shape[:2]
    out[max(-dx, 0):nx + min(-dx, 0), max(-dy, 0):ny + min(-dy, 0)] = a[max(dx, 0):nx + min(dx, 0), max(dy, 0):ny + min(dy, 0)]
    return out


def torch_ground(occ, H, s):
    """synth.ground_ref (unknown = 'free') in torch ops over dense bool volumes -> (support, ground, obstacles, drive)."""
    clear = ~occ
    support = occ.clone()
    wall = torch.zeros_like(occ)
    for k in range(1, H + 1):
        support &= _up(clear, k, True)
        wall |= _up(occ, k, False)
    fine = wall
    for k in range(-s, s + 1):
        fine = fine | _up(support, k, False)
    ground = support.clone()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            if dx or dy:
                ground &= _side(fine, dx, dy)
    floor = torch.zeros_like(occ)
    for z in range(occ.shape[2] - 1, -1, -1):
        floor[:, :, z] = occ[:, :, z] & (ground[:, :, z] | (floor[:, :, z + 1] if z + 1 < occ.shape[2] else False))
    drive = torch.zeros_like(occ)
    for k in range(1, s + 2):
        drive |= _up(ground, -k, False)
    return support, ground, occ & ~floor, drive & ~occ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    grid = ops.OccupancyGrid.from_points(pts, resolution=a.voxel).empty_like()
    grid.insert(room_points(dev))
    floor_z = int(torch.nonzero(grid.dense()[200, 200])[0])   # the voxel level of the box's face z = -2 m
    grid.insert(furniture(grid, floor_z))
    layer = ops.GroundLayer(grid, H=H, step=STEP)
    res = {"grid_dims": list(grid.dims), "voxels": int(np.prod(grid.dims)), "occupied_voxels": grid.count(), "H": H, "step": STEP,
           "radius_m": a.radius, "plane_MB": grid.buf.numel() / 2 ** 20}
    for k in ("support", "ground", "obstacles", "drive"):
        res[f"{k}_voxels"] = getattr(layer, k).count()

    # the comparison: the same planes by torch ops, equal before anything is timed
    occ = grid.dense()
    want = torch_ground(occ, H, STEP)
    for k, w in zip(("support", "ground", "obstacles", "drive"), want):
        assert torch.equal(getattr(layer, k).dense(), w), f"{k}: the kernels and the torch ops disagree"
    res["planes_equal_torch"] = True
    assert bool(want[1][:, :, floor_z + RISE].any()) and bool(want[1][RAMP_X[0] + 5, RAMP_Y, floor_z + 6].any()), "the mezzanine and the ramp carry ground"
    res["build_ms"] = event_ms(layer.rebuild, a.reps, 10)
    res["torch_ms"] = event_ms(lambda: torch_ground(occ, H, STEP), a.reps, 1)
    del want

    rng = np.random.default_rng(1)
    lo, hi = np.array([-20.0, -20.0, -2.0]), np.array([20.0, 20.0, 2.0])
    Q = torch.from_numpy(rng.uniform(lo, hi, (a.rows, 3)).astype(np.float32)).to(dev)
    res["snap_rows"] = a.rows
    res["snap_ms"] = event_ms(lambda: layer.snap(Q, H), a.reps, 5)
    res["snap_found"] = int((layer.snap(Q, H)[1] >= 0).sum())

    # the field and the travel field over the layer, beside the plain ones over the same map
    sensor = torch.tensor([[-18.0, -18.0, -1.5]], device=dev)   # half a metre above the floor: within H voxels of the standing voxel
    ground_field = layer.field(D=5)
    tf = tools.ground_travel(layer, sensor, a.radius, field=ground_field)
    assert tf.seeded.tolist() == [1]
    plain_field = ops.ClearanceField(grid, D=5)
    plain_tf = ops.TravelField(plain_field, a.radius, torch.tensor([[-18.0, -18.0, 0.0]], device=dev))
    assert plain_tf.seeded.tolist() == [1]
    for name, field, travel in (("ground", ground_field, tf), ("plain", plain_field, plain_tf)):
        dense = travel.dense()
        res[f"{name}_field_ms"] = wall_ms(field.rebuild, a.reps)
        res[f"{name}_travel_ms"] = wall_ms(travel.rebuild, a.reps)
        res[f"{name}_travel_rounds"] = travel.rounds
        res[f"{name}_reachable_voxels"] = int((dense >= 0).sum())
    on_top = torch.tensor(grid.origin.tolist(), device=dev) + (torch.tensor([[300.0, 200.0, floor_z + RISE + 1.0]], device=dev) + 0.5) * grid.resolution
    reached = float(tf.distance(on_top)[0])   # (metres driven from the start to the middle of the mezzanine, up the ramp)
    res["mezzanine_reached_m"] = reached if np.isfinite(reached) else None
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
