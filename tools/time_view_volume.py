"""What scoring views by the unknown volume they reveal costs ("Unknown volume"), in one process: the map of
tools/time_carve.py — synth.make_cloud(1 M, seed 0) as one scan from the origin, voxels of 0.1 m, the 405 x 405 x 45 grid of
OccupancyGrid.from_points — M = 256 views from tools.propose_views over that map's frontier (from the known-free nodes of a 1 m
lattice), limits (0.5, 5).  Medians of --reps event-timed runs after a warm-up.

  gain_window / gain_all   tohip_view_volume over the M views, window on and off (the same gains; checked)
  mark                     one launch that scores one view and sets its voxels in a plane
  select_k8                tools.select_views_volume, k = 8, end to end (3 k launches and the one read-back)
  composition              for scale, what the public calls cost for the same M views: unknown().export(), cull_waypoints over the
                           centres (16 views at a time: its outputs are (views, centres) sized) and one line_of_sight per view
  centres / rays / visits per ray, from the kernel's own counters

    python tools/time_view_volume.py [--reps 5] [--views 256] [--json out.json]
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


def composition(space, p, q, cam, limits, chunk=16):
    """The oracle of the tests as a cost: every unknown voxel's centre as a cloud, culled per view, one walk per kept centre."""
    _, centres = space.unknown().export()
    gains = []
    for w0 in range(0, p.shape[0], chunk):
        kept, _, counts, _ = ops.cull_waypoints(centres, p[w0:w0 + chunk], q[w0:w0 + chunk], cam, limits[0], limits[1], normalize=True)
        for j, n in enumerate(counts):
            c = centres[kept[j, :n].long()]
            gains.append(int((space.occupied.line_of_sight(p[w0 + j].expand_as(c).contiguous(), c, skip=(1, 0)) == 1).sum()))
    return gains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    occupied = ops.OccupancyGrid.from_points(pts, resolution=a.voxel)
    space = ops.SpaceMap(occupied)
    space.free.carve(torch.zeros(3, device=dev), pts)
    frontier = space.frontier()
    lattice = torch.from_numpy(synth.roadmap_lattice([-19.0, -19.0, 0.0], [19.0, 19.0, 0.0], 1.0)).to(dev)
    nodes = lattice[tools.known_free(space, lattice)]
    limits = (0.5, 5.0)
    K = torch.from_numpy(synth.K_INTRINS)
    prop = tools.propose_views(frontier.points, nodes, n_per_position=2, sectors=32, max_views=a.views, K=K, img_width=synth.IMG_WIDTH,
                               img_height=synth.IMG_HEIGHT, min_dist=limits[0], max_dist=limits[1])
    p, q = prop.poses, prop.quats
    cam = ops.Camera(K, synth.IMG_WIDTH, synth.IMG_HEIGHT, *limits)
    res = {"grid_dims": list(occupied.dims), "voxels": int(np.prod(occupied.dims)), "unknown_voxels": space.unknown().count(),
           "frontier_voxels": frontier.n, "free_nodes": int(nodes.shape[0]), "views": int(p.shape[0]), "limits": list(limits)}

    stats, stats_all = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    gains = ops.view_volume(space, p, q, cam, *limits, stats=stats)
    assert torch.equal(gains, ops.view_volume(space, p, q, cam, *limits, window=False, stats=stats_all))
    for name, s in (("window", stats), ("all", stats_all)):
        c, r, v = (int(x) for x in s.tolist())
        res.update({f"centres_tested_{name}": c, f"rays_{name}": r, f"visits_per_ray_{name}": v / max(r, 1)})
    res.update(gain_sum=int(gains.sum()), gain_max=int(gains.max()), views_with_gain=int((gains > 0).sum()))
    res["gain_window_ms"] = event_ms(lambda: ops.view_volume(space, p, q, cam, *limits), a.reps, 1)
    res["gain_all_ms"] = event_ms(lambda: ops.view_volume(space, p, q, cam, *limits, window=False), a.reps, 1)
    best = int(torch.argmax(gains))
    plane = space.free.empty_like()
    res["mark_ms"] = event_ms(lambda: ops.view_volume(space, p[best:best + 1], q[best:best + 1], cam, *limits, mark=plane), a.reps, 1)
    camera = dict(intrins=K, img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT, min_dist=limits[0], max_dist=limits[1])
    sel = tools.select_views_volume(space, p, q, 8, **camera)
    res.update(select_order=sel.order.tolist(), select_gains=sel.gains.tolist())
    res["select_k8_ms"] = event_ms(lambda: tools.select_views_volume(space, p, q, 8, **camera), a.reps, 1)
    assert composition(space, p, q, cam, limits) == gains.tolist()
    res["composition_ms"] = event_ms(lambda: composition(space, p, q, cam, limits), a.reps, 1)
    res["composition_over_fused"] = res["composition_ms"] / res["gain_window_ms"]
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
