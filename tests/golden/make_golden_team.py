#!/usr/bin/env python3
"""Generate tests/golden/team_bundled_2.npz: the reference's own numbers for a team of two on its bundled sample.

Imports make_golden.py for its stubs and its import of the UNMODIFIED reference (nothing there is edited, and none of its fixtures
is written again), and runs the reference's ModelTraj on the CPU:
  * on E = the two members' waypoints laid end to end (20 rows) at vis_wps_dist = 0: loss['vis'], the rewards and the gradient rows
    of loss['vis'] — what the team's one reward must be;
  * on each member alone: criterion's l2 / length / smooth — what stays per member.
Members: the first 10 waypoints of the bundled path, and the same shifted one metre sideways (+y); both moved off their starting
positions by a small seeded jitter (poses0 stays the start), so that l2 and length are not trivially zero.

Usage:  python tests/golden/make_golden_team.py      (needs the reference beside the repository, as make_golden.py does)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (the stubs and `ref_model`)

W_MEMBER, SHIFT, JITTER, SEED = 10, (0.0, 1.0, 0.0), 0.05, 23


def _ref(pts, poses0, quats, poses):
    m = G.ref_model.ModelTraj(points=torch.from_numpy(pts), wps_poses=torch.from_numpy(poses0), wps_quats=torch.from_numpy(quats),
                              intrins=G.K, img_width=G.IMG_W, img_height=G.IMG_H, device=G.CPU)
    with torch.no_grad():
        m.poses.copy_(torch.from_numpy(poses))
    return m


def main():
    b = np.load(os.path.join(HERE, "bundled.npz"))
    pts, path = b["pts"], b["poses"]
    rng = np.random.default_rng(SEED)
    start = [path[:W_MEMBER].copy(), (path[:W_MEMBER] + np.float32(SHIFT)).astype(np.float32)]
    now = [(p + JITTER * rng.standard_normal(p.shape)).astype(np.float32) for p in start]
    quats = np.tile(np.float32([[1, 0, 0, 0]]), (W_MEMBER, 1))
    # the team's one reward: the reference on E
    E0, E, Eq = np.concatenate(start), np.concatenate(now), np.concatenate([quats, quats])
    m = _ref(pts, E0, Eq, E)
    m(vis_wps_dist=0.0)
    m.loss["vis"].backward()
    out = dict(poses0=np.stack(start), poses=np.stack(now), quats=np.stack([quats, quats]), loss_vis=m.loss["vis"].detach().numpy(),
               rewards=m.rewards.detach().numpy(), vis_poses_grad=m.poses.grad.numpy(), vis_quats_grad=m.quats.grad.numpy())
    # what stays per member: criterion on each member alone
    terms = []
    for p0, p in zip(start, now):
        mb = _ref(pts, p0, quats, p)
        mb(vis_wps_dist=0.0)
        terms.append([float(mb.loss["l2"]), float(mb.loss["length"]), float(mb.loss["smooth"])])
    out["member_terms"] = np.float64(terms)   # (2, 3): l2, length, smooth
    out["recipe"] = np.asarray("reference ModelTraj (CPU, f32) on bundled.npz's cloud; members = first 10 waypoints of its path and "
                               "their +1 m y shift, each + 0.05 N(0,1) jitter (seed 23) over poses0; E = both end to end, "
                               "vis_wps_dist=0; member_terms = l2, length, smooth of criterion per member alone")
    path_out = os.path.join(HERE, "team_bundled_2.npz")
    np.savez_compressed(path_out, **out)
    print(f"team_bundled_2.npz  {os.path.getsize(path_out) / 1024:.1f} KiB  keys={sorted(out)}")


if __name__ == "__main__":
    main()
