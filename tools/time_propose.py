"""What proposing views costs (tools.propose_views: propose_kernels.hip), in one process, medians of --reps event-timed runs, for
M = 4 096 positions (a 64 x 64 lattice at z = 0) over N = 1 M synthetic points (synth.make_cloud), S = 32 sectors, the bundled camera:

  (a) hist          tohip_view_histogram with the prune (the product path)
  (b) hist_dense    the same call with prune = 0: every tile against every position (the same bits, asserted)
  (c) headings      tohip_view_headings, two per position
  (d) propose       the whole public call, no clearance radius: inside the synthetic slab no position is clear (wall clock)
  (e) viewset       what the same question costs without the kernels: select_views (k = 1) over --base-positions positions x S
                    headings as candidates, one forward row per candidate (wall clock); x M / base-positions is the estimate for
                    all M positions — the forward's cost is linear in the number of rows

at max_dist = 10 and 5 m, and the fraction of (position, tile) pairs the prune drops, recomputed on the host from the tile spheres.

    python tools/time_propose.py [--reps 5] [--json out.json]
    python tools/time_propose.py --once        # (a) and (c) once: under rocprofv3 --kernel-trace --stats
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

S = 32


def dropped_fraction(cloud, pos, mn, mx):
    """The share of (position, tile) pairs whose sphere lies wholly outside the shell, by the kernel's test in numpy f32."""
    f32 = np.float32
    o = 16 * cloud.npad
    b = cloud.blob[o:o + 16 * (cloud.npad // 256)].view(torch.float32).view(-1, 4).cpu().numpy()
    kept = 0
    for t in pos:
        d = b[:, :3] - t[None, :]
        dc = np.sqrt((d * d).sum(axis=1, dtype=f32))
        slack = f32(1e-5) * np.maximum(np.abs(t).max(), np.abs(b[:, :3]).max(axis=1)) + f32(1e-6)
        drop = (dc > (b[:, 3] + f32(mx)) * f32(1.0001) + slack) | ((dc + b[:, 3]) * f32(1.0001) + slack < f32(mn))
        kept += int((~drop).sum())
    return 1.0 - kept / (len(pos) * len(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--base-positions", type=int, default=16)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pts = synth.make_cloud(a.points, seed=1)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    g = np.linspace(-19.0, 19.0, a.side)
    pos_np = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    pos = torch.from_numpy(pos_np).to(dev)
    K, iw, ih = torch.from_numpy(synth.K_INTRINS), synth.IMG_WIDTH, synth.IMG_HEIGHT
    tan_v = float((ih / 2) / synth.K_INTRINS[1, 1])
    res = {"points": int(cloud.n), "positions": len(pos_np), "sectors": S}
    for mx in (10.0, 5.0):
        hist = lambda prune=True: ops.view_histogram(cloud, pos, None, None, S, 1.0, mx, tan_v, prune=prune)
        h = hist()
        r = {"pairs_counted": int(h.sum())}
        if a.once:
            ops.view_headings(h, 3, 2)
            torch.cuda.synchronize()
            res[f"max{mx:g}"] = r
            continue
        assert torch.equal(h, hist(False)), "the prune changed a bin"
        r["dropped_pairs_fraction"] = dropped_fraction(cloud, pos_np, 1.0, mx)
        r["hist_ms"] = event_ms(hist, a.reps, 3)
        r["hist_dense_ms"] = event_ms(lambda: hist(False), a.reps, 1)
        r["headings_ms"] = event_ms(lambda: ops.view_headings(h, 3, 2), a.reps, 5)
        cam = dict(K=K, img_width=iw, img_height=ih, min_dist=1.0, max_dist=mx)
        r["propose_views_ms"] = wall_ms(lambda: tools.propose_views(cloud, pos, sectors=S, **cam), a.reps)
        # the parent's way: every (position, heading) a candidate row of a view set
        nb = a.base_positions
        sub = pos_np[np.linspace(0, len(pos_np) - 1, nb).astype(int)]
        cq = synth.propose_tables(S)[1]
        cp, cq = torch.from_numpy(np.repeat(sub, S, axis=0)), torch.from_numpy(np.tile(cq, (nb, 1)))
        sel = lambda: tools.select_views(cloud, cp, cq, 1, intrins=K, img_width=iw, img_height=ih, min_dist=1.0, max_dist=mx)
        r["viewset_base_ms"] = wall_ms(sel, max(1, a.reps // 2))
        r["viewset_base_candidates"] = nb * S
        r["viewset_scaled_ms"] = r["viewset_base_ms"] * len(pos_np) / nb
        res[f"max{mx:g}"] = r
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
