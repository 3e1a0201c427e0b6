#!/usr/bin/env python3
"""Generate tests/golden/views_bundled_144.npz: the reference's own numbers for a greedy view selection on its bundled sample.

Imports make_golden.py for its stubs and its import of the UNMODIFIED reference (nothing there is edited, and none of its fixtures
is written again).  Candidates: the 6 x 6 x 4 grid over the bundled cloud (synth.bundled_candidate_grid), k = 8.  Per candidate the
log-odds row is computed with the reference's own to_camera_frame / get_dist_mask / get_fov_mask and its lines model.py:226-230
(CPU, f32); the greedy order is taken from those rows in f64 (gain = mean sigmoid(S + lo_c) - mean sigmoid(S), ties to the lowest
index); every round's margin (best minus second-best gain) is stored, and the reference ModelTraj's rewards on the chosen views
(vis_wps_dist = 0).  The rows themselves are 144 x N floats — too large to commit — so the fixture keeps their digest: each
candidate's number of non-zero entries and its f64 sum.

The fixture is only written when every margin is at least 100 x the rounding bound 2 (nnz_max / N) 4 2^-24 (two rewards per
entry, four ulps each at r < 1): below that an f32 implementation may legitimately choose differently.

Usage:  python tests/golden/make_golden_views.py      (needs the reference beside the repository, as make_golden.py does)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G  # noqa: E402  (the stubs and `ref_model`)
from trajectory_optimization_amd import synth  # noqa: E402

GRID, HEADINGS, K_VIEWS = 6, 4, 8


def reference_row(points, pose, quat, eps=1e-6):
    cam = G.ref_model.to_camera_frame(points, quat.unsqueeze(0), pose.unsqueeze(0))
    p = G.ref_model.get_dist_mask(cam, 1.0, 5.0) * G.ref_model.get_fov_mask(cam, G.IMG_H, G.IMG_W, G.K, eps=eps)
    p = p - p.min()
    p = p / p.max()
    p = torch.clip(p, 0.5, 1. - eps)
    return torch.log(p / (1. - p))


def greedy_f64(rows, k):
    """rows (M, N) -> (order, gains, margins) of the greedy rule in f64; a NaN row is absent."""
    M, N = rows.shape
    absent = np.isnan(rows).any(axis=1)
    S = np.zeros(N)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    order, gains, margins = [], [], []
    for _ in range(k):
        g = np.full(M, -np.inf)
        for c in range(M):
            if c in order or absent[c]:
                continue
            nz = rows[c] > 0
            g[c] = (sig(S[nz] + rows[c][nz]) - sig(S[nz])).sum() / N
        best = int(np.argmax(g))   # (the first maximum: ties to the lowest index)
        if not g[best] > 0:
            break
        second = np.partition(g, -2)[-2]
        order.append(best); gains.append(g[best]); margins.append(g[best] - second)
        S = S + rows[best]
    return order, np.asarray(gains), np.asarray(margins)


def main():
    b = np.load(os.path.join(HERE, "bundled.npz"))
    pts, path = b["pts"], b["poses"]
    N = len(pts)
    poses, quats = synth.bundled_candidate_grid(pts, path, GRID, HEADINGS)
    tp = torch.from_numpy(pts)
    with torch.no_grad():
        rows = np.stack([reference_row(tp, torch.from_numpy(poses[c]), torch.from_numpy(quats[c])).numpy() for c in range(len(poses))])
    nnz = (rows > 0).sum(axis=1)
    order, gains, margins = greedy_f64(rows.astype(np.float64), K_VIEWS)
    bound = 2.0 * (nnz.max() / N) * 4.0 * 2.0 ** -24
    print(f"order {order}  smallest margin {margins.min():.3e}  bound {bound:.3e}  ({margins.min() / bound:.0f} x)  "
          f"absent {int(np.isnan(rows).any(axis=1).sum())}  nnz share up to {nnz.max() / N:.4f}")
    assert len(order) == K_VIEWS, "the grid has fewer useful views than k"
    assert (margins >= 100.0 * bound).all(), (margins, bound)   # refuse: an f32 implementation could choose differently
    m = G.ref_model.ModelTraj(points=tp, wps_poses=torch.from_numpy(poses[order]), wps_quats=torch.from_numpy(quats[order]),
                              intrins=G.K, img_width=G.IMG_W, img_height=G.IMG_H, device=G.CPU)
    with torch.no_grad():
        m(vis_wps_dist=0.0)
    out = dict(cand_poses=poses, cand_quats=quats, order=np.int64(order), gains=gains, margins=margins, bound=np.float64(bound),
               row_nnz=np.int64(nnz), row_sum=rows.astype(np.float64).sum(axis=1), rewards=m.rewards.detach().numpy(),
               mean_reward=np.float64(m.rewards.detach().double().mean()),
               recipe=np.asarray("bundled.npz's cloud; candidates: x, y in linspace(min + 3, max - 3, 6), z = mean z of the bundled path, "
                                 "headings 2 pi j / 4 + 0.1, quat = r_z(heading) (x) synth.Q_OPTICAL, index (ix 6 + iy) 4 + j; rows by the "
                                 "reference's to_camera_frame / get_dist_mask / get_fov_mask + model.py:226-230 (f32); greedy in f64, k = 8; "
                                 "rewards = reference ModelTraj on the chosen views, vis_wps_dist = 0"))
    path_out = os.path.join(HERE, "views_bundled_144.npz")
    np.savez_compressed(path_out, **out)
    print(f"views_bundled_144.npz  {os.path.getsize(path_out) / 1024:.1f} KiB  keys={sorted(out)}")


if __name__ == "__main__":
    main()
