"""What scoring views by information gain costs ("Information gain"), in one process: the map of
tools/time_view_volume.py — synth.make_cloud(1 M, seed 0) as one scan from the origin, voxels of 0.1 m, the 405 x 405 x 45 grid of
OccupancyGrid.from_points — integrated ONCE into an ops.EvidenceMap (the once-swept room), and that tool's M = 256 views from
tools.propose_views over the map's frontier, limits (0.5, 5).  Every figure is the median of --windows event-timed windows of
--calls calls after a warm-up, with the windows' minimum and maximum beside it.

  (a) weight_plane / fold      tohip_evid_weight_plane over the map, beside tohip_evid_fold of a pass plane that touches every brick
                               of a copy of it: the same 32 bytes per brick word read
  (b) volume / info_unit       tohip_view_volume and tohip_view_information with the unit table (W[0] = 1, else 0) over the same 256
                               views, alternating in the same windows: the walks are the same, the ratio is the price of the byte
                               gather.  info_unit_call is ops.view_information as a caller pays for it: + the candidate plane
  (c) info_default             the default table (tools.information_table) on the same map, with the kernel's centres and rays
  (d) select_k8                tools.select_views_information, k = 8, end to end (the plane, 3 k launches and the one read-back),
                               beside tools.select_views_volume
  (e) composition              the same gains by existing ops: the candidates' export(), cull_waypoints over their centres (16 views
                               at a time), one line_of_sight per view, log_odds of the seen centres, a table gather and a sum

    python tools/time_view_information.py [--windows 5] [--calls 20] [--views 256] [--json profiles/time_view_information.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from trajectory_optimization_amd import ops, synth, tools  # noqa: E402


def windows_ms(fns, windows, calls):
    """Per-call milliseconds of each of `fns`, alternating inside every window -> [(median, min, max)] in their order."""
    for fn in fns:
        fn()
    out = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b) / calls)
    return [(float(np.median(v)), float(min(v)), float(max(v))) for v in out]


def composition(m, table_dev, p, q, cam, limits, chunk=16):
    """The oracle of the tests as a cost -> the gains as a list."""
    weights = table_dev[m.dense().long() + 128]
    plane = m.occupied.empty_like()
    nx, ny, nz = m.dims
    v = torch.nonzero(weights.reshape(-1) > 0).reshape(-1)            # linear index (x ny + y) nz + z of dense()'s layout
    x, y, z = v // (ny * nz), (v // nz) % ny, v % nz
    nbx, nby = (nx + 3) // 4, (ny + 3) // 4
    word = ((z >> 1) * nby + (y >> 2)) * nbx + (x >> 2)
    bit = (x & 3) | ((y & 3) << 2) | ((z & 1) << 4)
    acc = torch.zeros(plane.buf.numel() - 256, dtype=torch.int32, device=m.device)
    acc.index_add_(0, word * 4 + (bit >> 3), (1 << (bit & 7)).to(torch.int32))   # distinct voxels are distinct bits
    plane.buf[256:] = acc.to(torch.uint8)
    _, centres = plane.export()
    gains = []
    for w0 in range(0, p.shape[0], chunk):
        kept, _, counts, _ = ops.cull_waypoints(centres, p[w0:w0 + chunk], q[w0:w0 + chunk], cam, limits[0], limits[1], normalize=True)
        for j, n in enumerate(counts):
            c = centres[kept[j, :n].long()]
            see = m.occupied.line_of_sight(p[w0 + j].expand_as(c).contiguous(), c, skip=(1, 0)) == 1
            if not bool(see.any()):
                gains.append(0)
                continue
            values, _ = m.log_odds(c[see].contiguous())
            gains.append(int(table_dev[values.long() + 128].sum()))
    return gains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing without one is no timing")
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_cloud(a.points, seed=0)).to(dev)
    m = ops.EvidenceMap.like(ops.OccupancyGrid.from_points(pts, resolution=a.voxel))
    m.integrate(torch.zeros(3, device=dev), pts)
    space = m.space
    frontier = space.frontier()
    lattice = torch.from_numpy(synth.roadmap_lattice([-19.0, -19.0, 0.0], [19.0, 19.0, 0.0], 1.0)).to(dev)
    nodes = lattice[tools.known_free(space, lattice)]
    limits = (0.5, 5.0)
    K = torch.from_numpy(synth.K_INTRINS)
    prop = tools.propose_views(frontier.points, nodes, n_per_position=2, sectors=32, max_views=a.views, K=K, img_width=synth.IMG_WIDTH,
                               img_height=synth.IMG_HEIGHT, min_dist=limits[0], max_dist=limits[1])
    p, q = prop.poses, prop.quats
    cam = ops.Camera(K, synth.IMG_WIDTH, synth.IMG_HEIGHT, *limits)
    M = int(p.shape[0])
    unit = np.zeros(256, dtype=np.int64)
    unit[0] = 1
    unit_dev = ops.check_information_table(unit, dev)
    default = tools.information_table(m)
    default_dev = ops.check_information_table(default, dev)
    res = {"grid_dims": list(m.dims), "voxels": int(np.prod(m.dims)), "brick_words": (m.buf.numel() - 256) // 32,
           "unknown_voxels": space.unknown().count(), "occupied_voxels": m.occupied.count(), "free_voxels": m.free.count(),
           "frontier_voxels": frontier.n, "views": M, "limits": list(limits), "windows": a.windows, "calls": a.calls,
           "information_default": int(m.information(default_dev)), "candidates_default": m.uncertain(default_dev).count(),
           "candidates_unit": m.uncertain(unit_dev).count()}

    def put(name, t):
        res[name + "_ms"], res[name + "_ms_min"], res[name + "_ms_max"] = t

    # (a) the weight plane beside a fold that touches every brick
    copy = m.reframed(shift=(0, 0, 0))
    hit, pas = copy.occupied.empty_like(), copy.occupied.empty_like()
    pas.buf[256:] = 0xFF
    plane = m.occupied.empty_like()
    total = torch.zeros((), dtype=torch.int64, device=dev)

    def weight_plane():
        ops._map_call0(dev, "tohip_evid_weight_plane", *m._sizes(), ops.ptr(default_dev), ops.ptr(plane.buf), plane.buf.numel(), ops.ptr(total))
    t_plane, t_fold = windows_ms([weight_plane, lambda: copy._fold(hit, pas, False)], a.windows, a.calls)
    put("weight_plane", t_plane)
    put("fold_every_brick", t_fold)

    # (b) the unit table against the volume, (c) the default table
    gains_v, gains_u, gains_d = (torch.empty(M, dtype=torch.int64, device=dev) for _ in range(3))
    plane_u, plane_d = m.uncertain(unit_dev), m.uncertain(default_dev)
    stats = {k: torch.zeros(3, dtype=torch.int64, device=dev) for k in ("volume", "unit", "default")}
    ops._view_volume_call(space, p, q, M, None, cam, *limits, None, None, True, gains_v, None, stats["volume"])
    ops._view_information_call(m, unit_dev, plane_u, p, q, M, None, cam, *limits, None, None, True, gains_u, None, stats["unit"])
    ops._view_information_call(m, default_dev, plane_d, p, q, M, None, cam, *limits, None, None, True, gains_d, None, stats["default"])
    assert torch.equal(gains_u, gains_v) and stats["unit"].tolist() == stats["volume"].tolist()
    for name, s in stats.items():
        c, r, v = (int(x) for x in s.tolist())
        res.update({f"centres_tested_{name}": c, f"rays_{name}": r, f"visits_per_ray_{name}": v / max(r, 1)})
    res.update(gain_sum_volume=int(gains_v.sum()), gain_sum_default=int(gains_d.sum()), gain_max_default=int(gains_d.max()),
               views_with_gain_default=int((gains_d > 0).sum()))
    t_v, t_u, t_d, t_call = windows_ms([
        lambda: ops._view_volume_call(space, p, q, M, None, cam, *limits, None, None, True, gains_v, None, None),
        lambda: ops._view_information_call(m, unit_dev, plane_u, p, q, M, None, cam, *limits, None, None, True, gains_u, None, None),
        lambda: ops._view_information_call(m, default_dev, plane_d, p, q, M, None, cam, *limits, None, None, True, gains_d, None, None),
        lambda: ops.view_information(m, p, q, cam, *limits, table=unit_dev)], a.windows, a.calls)
    put("volume", t_v)
    put("info_unit", t_u)
    put("info_default", t_d)
    put("info_unit_call", t_call)
    res["info_unit_over_volume"] = t_u[0] / t_v[0]
    res["info_default_over_unit"] = t_d[0] / t_u[0]

    # (d) selections end to end
    camera = dict(intrins=K, img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT, min_dist=limits[0], max_dist=limits[1])
    sel = tools.select_views_information(m, p, q, 8, table=default_dev, **camera)
    res.update(select_order=sel.order.tolist(), select_gains=sel.gains.tolist())
    t_si, t_sv = windows_ms([lambda: tools.select_views_information(m, p, q, 8, table=default_dev, **camera),
                             lambda: tools.select_views_volume(m, p, q, 8, **camera)], a.windows, max(1, a.calls // 10))
    put("select_information_k8", t_si)
    put("select_volume_k8", t_sv)

    # (e) the composition
    table_long = default.to(torch.int64).to(dev)
    assert composition(m, table_long, p, q, cam, limits) == gains_d.tolist()
    put("composition", windows_ms([lambda: composition(m, table_long, p, q, cam, limits)], a.windows, 1)[0])
    res["composition_over_fused"] = res["composition_ms"] / (res["info_default_ms"] + res["weight_plane_ms"])
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
