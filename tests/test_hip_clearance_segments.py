"""The swept clearance term (clearance_mode='segments', clearance_kernels.hip): the segment query against a numpy f32 brute force of
its definition, its edge cases, the term's value and gradient, trajectories laid end to end, every ModelTraj path and optimiser loop
that carries it, and a row of pillars it keeps the path's segments off while the waypoint term passes between them."""
import numpy as np
import pytest
import torch

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def brute(pts, poses, r, n_traj=1):
    """numpy restatement of the segment query: f32 without contraction, finite rows only, d2 < fl(r*r), ties to the lowest row; s in
    f64 from the f32 coordinates.  -> (d, idx, s, d2) of the n_traj (W - 1) segments."""
    pts, P = np.asarray(pts, f32), np.asarray(poses, f32)
    W = len(P) // n_traj
    r2 = f32(r) * f32(r)
    fin = np.isfinite(pts).all(axis=1)
    d_out, i_out, s_out, d2_out = [], [], [], []
    for b in range(n_traj):
        for w in range(W - 1):
            a, bb = P[b * W + w], P[b * W + w + 1]
            d_out.append(f32(np.inf)), i_out.append(-1), s_out.append(f32(0.0)), d2_out.append(f32(np.inf))
            if not (np.isfinite(a).all() and np.isfinite(bb).all()):
                continue
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                e = (bb - a).astype(f32)
                ee = f32(f32(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
                inv = f32(1.0) / ee if ee > 0 else f32(0.0)
                ux, uy, uz = (pts[:, 0] - a[0]).astype(f32), (pts[:, 1] - a[1]).astype(f32), (pts[:, 2] - a[2]).astype(f32)
                dot = ((ux * e[0] + uy * e[1]) + uz * e[2]).astype(f32)
                s = np.fmin(np.fmax((dot * inv).astype(f32), f32(0.0)), f32(1.0)).astype(f32)
                qx, qy, qz = (ux - s * e[0]).astype(f32), (uy - s * e[1]).astype(f32), (uz - s * e[2]).astype(f32)
                d2 = ((qx * qx + qy * qy) + qz * qz).astype(f32)
            d2 = np.where(fin, d2, np.inf).astype(f32)
            i = int(np.argmin(d2))
            if d2[i] < r2:
                a64, e64, x64 = a.astype(f64), bb.astype(f64) - a.astype(f64), pts[i].astype(f64)
                ee64 = e64 @ e64
                i_out[-1], d_out[-1], d2_out[-1] = i, f32(np.sqrt(f64(d2[i]))), d2[i]
                s_out[-1] = f32(min(max(((x64 - a64) @ e64) / ee64, 0.0), 1.0)) if ee64 > 0 else f32(0.0)
    return np.array(d_out, f32), np.array(i_out, np.int32), np.array(s_out, f32), np.array(d2_out, f32)


def seg_dist64(pts, poses):
    """f64 distance from every segment between consecutive rows of `poses` to its nearest finite point of `pts` -> (d (W-1), idx, s)."""
    x = np.asarray(pts, f64)
    x = np.where(np.isfinite(x).all(axis=1)[:, None], x, 1e30)
    P = np.asarray(poses, f64)
    d, idx, ss = [], [], []
    for a, b in zip(P[:-1], P[1:]):
        e = b - a
        ee = e @ e
        s = np.clip(((x - a) @ e) / ee, 0.0, 1.0) if ee > 0 else np.zeros(len(x))
        dist = np.linalg.norm(x - a - s[:, None] * e, axis=1)
        i = int(np.argmin(dist))
        d.append(dist[i]), idx.append(i), ss.append(s[i])
    return np.array(d), np.array(idx), np.array(ss)


def term64(pts, poses, r, w, n_traj=1):
    """f64 restatement of the term: weight x sum over the segments within r of (r - d)^2, per trajectory."""
    P = np.asarray(poses, f64).reshape(n_traj, -1, 3)
    out = []
    for p in P:
        d = seg_dist64(pts, p)[0]
        out.append(w * np.sum(np.where(d < r, (r - d) ** 2, 0.0)))
    return np.array(out)


def parts64(pts, poses, idx, d2, r, w):
    """The f64 finish given the query's winners (idx, and d2 as the f32 it was): g_a, g_b of every segment of ONE trajectory, (W-1, 3)
    each; r and w as the f32 the library takes."""
    r, w = f64(f32(r)), f64(f32(w))
    P, x = np.asarray(poses, f32).astype(f64), np.asarray(pts, f32).astype(f64)
    ga, gb = np.zeros((len(P) - 1, 3)), np.zeros((len(P) - 1, 3))
    for k in range(len(P) - 1):
        if idx[k] < 0:
            continue
        a, e, u = P[k], P[k + 1] - P[k], x[idx[k]] - P[k]
        ee, dot = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], u[0] * e[0] + u[1] * e[1] + u[2] * e[2]
        t = min(max(dot / ee, 0.0), 1.0) if ee > 0 else 0.0
        v = t * e - u
        vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        if vv > 0:
            c = -2.0 * w * (r - np.sqrt(f64(d2[k]))) / np.sqrt(vv)
            ga[k], gb[k] = c * (1.0 - t) * v, c * t * v
    return ga, gb


def rows64(ga, gb):
    """Per-waypoint rows: (float)(g_b of segment w - 1 + g_a of segment w)."""
    z = np.zeros((1, 3))
    return (np.concatenate([z, gb]) + np.concatenate([ga, z])).astype(f32)


def seg_query(cloud, poses, r, dev, n_traj=1, **kw):
    from trajectory_optimization_amd import ops
    out = ops.clearance_segments(cloud, torch.as_tensor(np.asarray(poses, f32), device=dev), r, n_traj=n_traj, **kw)
    return [None if t is None else t.cpu().numpy() for t in out]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


# ---- 1. the query equals the brute force ------------------------------------------------------------------------------------------------

def _segments(pts, rng, r):
    """(nseg, 2, 3): 24 short segments inside the cloud, one about 10 m long, four each whose nearest point lies beyond a, beyond b
    and beside the interior, four far away."""
    lo, hi = pts.min(0), pts.max(0)
    a = rng.uniform(lo, hi, (24, 3))
    short = np.stack([a, a + rng.uniform(-0.6, 0.6, (24, 3))], 1)
    long = np.array([[[-5.0, -3.0, 0.0], [4.5, 0.1, 0.6]]])
    x = pts[rng.integers(0, len(pts), 12)].astype(f64)
    dirs = rng.standard_normal((12, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    perp = np.cross(dirs, [0.0, 0.0, 1.0]) * 0.02 * r
    start = np.concatenate([np.full(4, 0.2 * r), np.full(4, -0.2 * r - 1.0), np.full(4, -0.5)])   # a = x + start * dir: beyond a, beyond b, interior
    aa = x + perp + start[:, None] * dirs
    near = np.stack([aa, aa + dirs], 1)
    fa = hi + 50.0 + rng.uniform(0, 5, (4, 3))
    far = np.stack([fa, fa + rng.uniform(-1, 1, (4, 3))], 1)
    return np.concatenate([short, long, near, far]).astype(f32)


@pytest.mark.parametrize("n", [1000, 20_000, 300_000])
def test_query_equals_brute_force(dev, n):
    """1 000 points: one wave, one group of tile spheres; 20 000: a second wave; 300 000: more than 16 x 64 tiles, so a wave takes a
    second group with the radius its first one left."""
    rng = np.random.default_rng(n)
    pts = synth.make_cloud(n, seed=5)
    r = {1000: 2.5, 20_000: 1.0}.get(n, 0.5)
    segs = _segments(pts, rng, r)
    nseg = len(segs)
    d, idx, s = seg_query(_cloud(pts, dev), segs.reshape(-1, 3), r, dev, n_traj=nseg)   # every segment a trajectory of two waypoints
    d_ref, i_ref, s_ref, _ = brute(pts, segs.reshape(-1, 3), r, n_traj=nseg)
    print(n, "found", int((i_ref >= 0).sum()), "of", nseg, "s=0:", int(((s_ref == 0) & (i_ref >= 0)).sum()), "s=1:", int((s_ref == 1).sum()))
    assert np.array_equal(idx, i_ref)
    assert same_bits(d, d_ref)
    assert np.abs(s - s_ref).max() <= 1e-6
    found = i_ref >= 0
    assert found.sum() >= nseg // 3 and (idx[-4:] == -1).all() and idx[24] >= 0
    assert (found & (s_ref == 0)).any() and (found & (s_ref == 1)).any() and (found & (s_ref > 0) & (s_ref < 1)).any()


def _cloud(pts, dev, sort=True):
    from trajectory_optimization_amd import ops
    return ops.PackedCloud(torch.from_numpy(np.asarray(pts, f32)).to(dev), sort=sort)


# ---- 2. edge cases ------------------------------------------------------------------------------------------------------------------------

def _edge_points():
    pts = synth.make_cloud(4096, seed=9)
    pts[100] = (100.5, 100.5, 100.0)                       # at exactly d2 == r*r = 0.25 from the segment (100..101, 100, 100)
    pts[3000] = (60.5, 60.125, 60.0)                       # mirrored about the segment (60..61, 60, 60): the lowest row wins
    pts[200] = (60.5, 59.875, 60.0)
    pts[520] = (70.1, 70.0, 70.3)                          # the winner of (70, 70, 70..71), a NaN row and inf rows in its tile of the
    pts[530] = (np.nan, 70.0, 70.0)                        # unsorted pack (rows 512..767)
    pts[540] = (np.inf, 70.0, 70.0)
    pts[541] = (70.0, -np.inf, 70.0)
    pts[3500] = (80.0, 80.0, 80.2)
    pts[3501] = (80.0, np.nan, 80.0)
    return pts


@pytest.mark.parametrize("sort", [True, False])
def test_query_edge_cases(dev, sort):
    from trajectory_optimization_amd import tools
    pts, r = _edge_points(), 0.5
    cloud = _cloud(pts, dev, sort)
    segs = np.array([[[100, 100, 100], [101, 100, 100]], [[60, 60, 60], [61, 60, 60]], [[70, 70, 70], [70, 70, 71]],
                     [[80, 80, 79.5], [80, 80, 80.1]]], f32)
    d, idx, s = seg_query(cloud, segs.reshape(-1, 3), r, dev, n_traj=len(segs))
    d_ref, i_ref, s_ref, _ = brute(pts, segs.reshape(-1, 3), r, n_traj=len(segs))
    assert list(i_ref) == [-1, 200, 520, 3500]
    assert np.array_equal(idx, i_ref) and same_bits(d, d_ref) and np.abs(s - s_ref).max() <= 1e-6
    assert np.isinf(d[0]) and s[0] == 0.0 and s[1] == 0.5
    # a degenerate segment is the point query, bit for bit
    rng = np.random.default_rng(7)
    inside = rng.uniform((-20, -20, -2), (20, 20, 2), (24, 3))   # the slab synth.make_cloud fills
    q = np.concatenate([inside, [[60.5, 60, 60], [70, 70, 70.2], [100, 100, 100], [500, 0, 0]]]).astype(f32)
    for rq in (r, 1.5):   # (1.5: most of the random positions find a point)
        dp, ip = tools.trajectory_clearance(cloud, torch.from_numpy(q).to(dev), rq)
        dd, ii, ss = seg_query(cloud, np.repeat(q, 2, axis=0), rq, dev, n_traj=len(q))
        assert np.array_equal(ii, ip.cpu().numpy()) and same_bits(dd, dp.cpu().numpy()) and (ss == 0).all()
        assert (ii >= 0).sum() >= (2 if rq == r else 12) and ii[-1] == -1
    # tools.trajectory_clearance(segments=True) is the same query over one path
    path = np.cumsum(rng.uniform(-0.4, 0.4, (9, 3)), axis=0).astype(f32)
    got = tools.trajectory_clearance(cloud, torch.from_numpy(path).to(dev), 1.5, segments=True)
    ref = brute(pts, path, 1.5)
    assert np.array_equal(got[1].cpu().numpy(), ref[1]) and same_bits(got[0].cpu().numpy(), ref[0]) and (ref[1] >= 0).any()


def test_a_waypoint_that_is_not_finite(dev):
    """Both segments touching it: -1 and no gradient; the others as without it."""
    rng = np.random.default_rng(3)
    pts = rng.uniform(-4, 4, (3000, 3)).astype(f32)
    cloud = _cloud(pts, dev)
    r, w = 0.875, 1.25
    path = (np.linspace(-3, 3, 7)[:, None] * np.array([1.0, 0.3, 0.1]) + rng.uniform(-0.2, 0.2, (7, 3))).astype(f32)
    for bad in (np.nan, np.inf):
        p = path.copy()
        p[3, 1] = bad
        g = torch.full((7, 3), 9.0, device=dev)
        d, idx, s, val = seg_query(cloud, p, r, dev, weight=w, grad=g, want_value=True)
        d_ref, i_ref, _, d2_ref = brute(pts, p, r)
        assert np.array_equal(idx, i_ref) and same_bits(d, d_ref)
        assert idx[2] == -1 and idx[3] == -1 and (idx[[0, 1, 4, 5]] >= 0).all()
        ga, gb = parts64(pts, np.nan_to_num(p, nan=0.0, posinf=0.0), idx, d2_ref, r, w)
        rows = g.cpu().numpy()
        assert np.array_equal(rows[3], np.zeros(3, f32)) and np.isfinite(rows).all()
        np.testing.assert_allclose(rows, rows64(ga, gb), rtol=1e-6, atol=1e-7)
        assert np.abs(rows[[2, 4]]).max() > 0
        ref = w * np.sum((r - d[idx >= 0].astype(f64)) ** 2)
        assert abs(float(val[0]) - ref) <= 1e-6 * ref


# ---- 3. value and gradient ------------------------------------------------------------------------------------------------------------------

def _walk(rng, W, step=0.7, start=(-2.5, -2.0, -1.0)):
    d = rng.standard_normal((W - 1, 3)) * 0.3 + np.array([0.6, 0.45, 0.2])
    d *= step / np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([[start], np.asarray(start) + np.cumsum(d, axis=0)]).astype(f32)


def test_value_and_gradient(dev):
    rng = np.random.default_rng(11)
    pts = rng.uniform(-4, 4, (3000, 3)).astype(f32)
    cloud = _cloud(pts, dev)
    r, w, W = 0.75, 1.75, 12   # (exact in f32: the f64 restatements take the same numbers)
    path = _walk(rng, W)
    # no near-tie: every segment's nearest point beats its runner-up by a margin the finite differences never cross
    x64 = pts.astype(f64)
    for a, b in zip(path[:-1].astype(f64), path[1:].astype(f64)):
        e = b - a
        t = np.clip(((x64 - a) @ e) / (e @ e), 0, 1)
        dist = np.sort(np.linalg.norm(x64 - a - t[:, None] * e, axis=1))
        assert dist[1] - dist[0] > 2e-4 and abs(dist[0] - r) > 1e-3   # (the differences step 1e-6)
    g = torch.empty((W, 3), dtype=torch.float32, device=dev)
    d, idx, s, val = seg_query(cloud, path, r, dev, weight=w, grad=g, want_value=True)
    rows = g.cpu().numpy()
    d64, i64, s64 = seg_dist64(pts, path)
    on = d64 < r
    assert on.sum() >= 6 and np.array_equal(idx, np.where(on, i64, -1))
    assert ((s64[on] > 0.05) & (s64[on] < 0.95)).any() and ((s64[on] == 0) | (s64[on] == 1)).any()
    # the value against the f64 restatement
    v_ref = term64(pts, path, r, w)[0]
    print("value", float(val[0]), v_ref)
    assert abs(float(val[0]) - v_ref) <= 1e-6 * v_ref
    # a waypoint's row is the f64 sum of its two segments' parts, rounded once
    ga, gb = parts64(pts, path, idx, brute(pts, path, r)[3], r, w)
    assert same_bits(rows, rows64(ga, gb))
    both = [k for k in range(1, W - 1) if idx[k - 1] >= 0 and idx[k] >= 0 and np.abs(gb[k - 1]).max() > 0 and np.abs(ga[k]).max() > 0]
    assert both, "a middle waypoint with a part from each side"
    # central differences of the f64 restatement
    h, scale = 1e-6, np.abs(rows).max()
    worst = 0.0
    for k in range(W):
        for c in range(3):
            pp, pm = path.astype(f64), path.astype(f64)
            pp[k, c] += h
            pm[k, c] -= h
            fd = (term64(pts, pp, r, w)[0] - term64(pts, pm, r, w)[0]) / (2 * h)
            worst = max(worst, abs(fd - rows[k, c]) / scale)
    print("central differences: worst error relative to the largest entry", worst)
    assert worst <= 1e-4


def _pillar_scene():
    """A thin pillar (a column of points) 0.1 m beside the midpoint of the segment between the waypoints at x = 0 and x = 2, and a few
    points far away."""
    z = np.arange(-1.0, 1.0001, 0.05)
    pillar = np.stack([np.full_like(z, 1.0), np.full_like(z, 0.1), z], 1)
    far = np.random.default_rng(1).uniform(30, 40, (500, 3))
    return np.concatenate([pillar, far]).astype(f32), len(z)


def test_a_pillar_between_two_waypoints(dev):
    from trajectory_optimization_amd import ops
    pts, n_pillar = _pillar_scene()
    cloud = _cloud(pts, dev)
    r, w = 0.5, 3.0
    path = np.stack([np.arange(-4.0, 6.1, 2.0), np.zeros(6), np.zeros(6)], 1).astype(f32)   # x = -4, -2, 0, 2, 4, 6
    pt = torch.from_numpy(path).to(dev)
    g = torch.full((6, 3), 7.0, device=dev)
    _, idx, val = ops.clearance(cloud, pt, r, w, grad=g, want_value=True)
    assert float(val) == 0.0 and (idx == -1).all() and not g.any()
    g = torch.full((6, 3), 7.0, device=dev)
    d, idx, s, val = ops.clearance_segments(cloud, pt, r, w, grad=g, want_value=True)
    rows = g.cpu().numpy()
    assert float(val[0]) > 0.0 and idx.cpu().tolist()[:2] == [-1, -1] and 0 <= int(idx[2]) < n_pillar and idx.cpu().tolist()[3:] == [-1, -1]
    assert abs(float(d[2]) - 0.1) < 1e-6 and abs(float(s[2]) - 0.5) < 1e-6
    assert abs(float(val[0]) - w * (r - 0.1) ** 2) <= 1e-5 * float(val[0])
    toward = pts[int(idx[2])].astype(f64) - np.array([1.0, 0.0, pts[int(idx[2]), 2]])   # from the closest point of the segment to the pillar
    for k in (2, 3):   # both neighbours' rows point toward the pillar: a descent step moves them away from it
        assert rows[k] @ toward > 0 and rows[k, 1] > 0.5 * w * (r - 0.1)
    assert not rows[[0, 1, 4, 5]].any()


# ---- 4. trajectories end to end -----------------------------------------------------------------------------------------------------------

def test_no_segment_joins_two_trajectories(dev):
    from trajectory_optimization_amd import ops
    pts, _ = _pillar_scene()
    cloud = _cloud(pts, dev)
    x = np.array([-6.0, -4.0, -2.0, 0.0, 2.0, 4.0, 6.0, 8.0])   # rows 3 and 4 straddle the pillar, and belong to two trajectories
    pt = torch.from_numpy(np.stack([x, np.zeros(8), np.zeros(8)], 1).astype(f32)).to(dev)
    g = torch.full((8, 3), 7.0, device=dev)
    d, idx, s, val = ops.clearance_segments(cloud, pt, 0.5, 3.0, n_traj=2, grad=g, want_value=True)
    assert d.shape == (6,) and (idx == -1).all() and torch.isinf(d).all() and not g.any() and val.tolist() == [0.0, 0.0]
    _, idx1, _ = ops.clearance_segments(cloud, pt, 0.5, 3.0, n_traj=1)   # as ONE trajectory the same rows do meet it
    assert idx1.cpu().tolist()[3] >= 0


def test_every_trajectory_equals_its_own_call(dev):
    rng = np.random.default_rng(21)
    pts = rng.uniform(-4, 4, (3000, 3)).astype(f32)
    cloud = _cloud(pts, dev)
    r, w, W, B = 0.75, 1.75, 6, 3
    paths = [_walk(np.random.default_rng(30 + b), W, start=(-2.5 + b, -2.0, -1.0 + 0.5 * b)) for b in range(B)]
    g = torch.empty((B * W, 3), dtype=torch.float32, device=dev)
    d, idx, s, val = seg_query(cloud, np.concatenate(paths), r, dev, n_traj=B, weight=w, grad=g, want_value=True)
    assert (idx >= 0).sum() >= B and val.shape == (B,)
    for b in range(B):
        g1 = torch.empty((W, 3), dtype=torch.float32, device=dev)
        d1, i1, s1, v1 = seg_query(cloud, paths[b], r, dev, weight=w, grad=g1, want_value=True)
        sl = slice(b * (W - 1), (b + 1) * (W - 1))
        assert np.array_equal(idx[sl], i1) and same_bits(d[sl], d1) and same_bits(s[sl], s1) and same_bits(val[b], v1[0])
        assert torch.equal(g[b * W:(b + 1) * W], g1)


# ---- 5. every path that carries the term ------------------------------------------------------------------------------------------------

def _model(dev, n=90_000, W=23, seed=31, cls=None, **kw):
    from trajectory_optimization_amd.model import ModelTraj
    pts = torch.from_numpy(synth.make_cloud(n, seed=seed))
    p, q = synth.make_path(W, optical=True, jitter_seed=seed)
    return (cls or ModelTraj)(pts, torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev, **kw)


CLR = dict(clearance_radius=0.6, clearance_weight=2.0)
SEG = dict(CLR, clearance_mode="segments")
TERMS = ("vis", "l2", "length", "smooth", "clearance")


@pytest.mark.parametrize("vwd,rig", [(0.0, False), (1.1, False), (0.0, True)])
def test_model_paths_agree(dev, vwd, rig):
    """The fused plan, the separate calls (_TrajLoss: the split / WaypointShard path) and the op-by-op criterion: loss['clearance'] to
    the bit and its gradient on all three, the total and every term to the bit on the two fused ones; and the term is the swept one."""
    from trajectory_optimization_amd import tools
    from trajectory_optimization_amd.model import ModelTraj, _TrajLoss

    class OpByOp(ModelTraj):
        def criterion(self, rewards):
            return super().criterion(rewards)

    kw = dict(SEG, rig=synth.camera_rig(3)) if rig else dict(SEG)
    a, b, c = _model(dev, **kw), _model(dev, **kw), _model(dev, cls=OpByOp, **kw)
    la = a(vis_wps_dist=vwd)
    step = b._wps_step(vwd)
    assert (step > 1) == (vwd > 0.0)
    lb, _, *terms_b = _TrajLoss.apply(b.poses, b.quats, b, step)
    lc = c(vis_wps_dist=vwd)
    assert [float(a.loss[k]) for k in TERMS] == [float(t) for t in terms_b] and float(la) == float(lb)
    assert float(c.loss["clearance"]) == float(a.loss["clearance"]) > 0.0
    parts = sum(float(c.loss[k]) for k in TERMS)
    assert abs(float(lc) - parts) <= 1e-5 * abs(parts) and abs(float(lc) - float(la)) <= 1e-5 * abs(parts)
    # the swept term: all W waypoints whatever the waypoint step, and not the waypoint term
    d, idx, _ = tools.trajectory_clearance(a, a.poses.data, CLR["clearance_radius"], segments=True)
    ref = CLR["clearance_weight"] * float(((float(f32(CLR["clearance_radius"])) - d[idx >= 0].double()) ** 2).sum())
    assert abs(float(a.loss["clearance"]) - ref) <= 1e-6 * ref
    w = _model(dev, **dict(kw, clearance_mode="waypoints"))
    w(vis_wps_dist=vwd)
    assert float(w.loss["clearance"]) != float(a.loss["clearance"])
    grads = []
    for m, t in ((a, a.loss["clearance"]), (b, terms_b[4]), (c, c.loss["clearance"])):
        t.backward()
        grads.append(m.poses.grad.clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2]) and grads[0].abs().sum() > 0


def test_backward_equals_the_one_call_step_gradient(dev):
    from trajectory_optimization_amd import optimizer as O
    a, b = _model(dev, **SEG), _model(dev, **SEG)
    a(vis_wps_dist=0.0).backward()
    run = O._OptRun([b], 1, 0.05, 0.01, 1e9, 1e9, 0.0, (0.9, 0.999), 1e-8)
    run.run(1)
    torch.cuda.synchronize()
    assert torch.equal(a.poses.grad, run.pg.view_as(a.poses.grad)) and a.poses.grad.abs().sum() > 0


@pytest.mark.parametrize("vwd,rig", [(0.0, False), (1.1, False), (0.0, True)])
def test_one_call_step_equals_the_split_step(dev, vwd, rig):
    from trajectory_optimization_amd import optimizer as O
    kw = dict(SEG, rig=synth.camera_rig(3)) if rig else dict(SEG)
    runs = []
    for split in (False, True):
        m = _model(dev, **kw)
        args = (m, 10, 0.05, 0.01, 1.003, 0.5, vwd, (0.9, 0.999), 1e-8)
        res = O._optimize_trajectory_split(*args) if split else O.optimize_trajectory(m, *args[1:7])
        runs.append((m, res))
    (ma, ra), (mb, rb) = runs
    assert torch.equal(ma.poses.data, mb.poses.data) and torch.equal(ma.quats.data, mb.quats.data)
    assert torch.equal(ma.rewards, mb.rewards)
    assert (ra.steps_taken, ra.stopped, ra.losses) == (rb.steps_taken, rb.stopped, rb.losses)
    for k in TERMS:
        assert float(ma.loss[k]) == float(mb.loss[k])
    assert float(ma.loss["clearance"]) > 0.0
    # and not the waypoint term's run
    mw = _model(dev, **dict(kw, clearance_mode="waypoints"))
    O.optimize_trajectory(mw, *args[1:7])
    assert not torch.equal(mw.poses.data, ma.poses.data)


def test_optimize_trajectories_equals_independent_runs(dev):
    from trajectory_optimization_amd import optimizer as O
    from trajectory_optimization_amd.model import ModelTraj
    base = _model(dev, **SEG)
    p0 = base.poses0.cpu().numpy()
    q0 = base.quats0.cpu()

    def make(j, **kw):
        p = torch.from_numpy(p0 + np.float32(0.3 * j) * np.array([0.0, 1.0, 0.1], f32))
        return ModelTraj.sharing_cloud_of(base, p, q0, **dict(SEG, **kw))
    together = [make(j) for j in range(3)]
    res = O.optimize_trajectories(together, 9, 0.05, 0.01, 1e9, 1e9, 0.0)
    for j in range(3):
        m = make(j)
        r1 = O.optimize_trajectory(m, 9, 0.05, 0.01, 1e9, 1e9, 0.0)
        assert torch.equal(m.poses.data, together[j].poses.data)
        assert r1.losses == res[j].losses
        assert float(m.loss["clearance"]) == float(together[j].loss["clearance"]) > 0.0
    with pytest.raises(ValueError, match="clearance"):   # the models must share the mode
        O.optimize_trajectories([make(0), make(1, clearance_mode="waypoints")], 1)


def test_team_of_one_is_optimize_trajectory(dev):
    from trajectory_optimization_amd.model import TeamTraj
    from trajectory_optimization_amd.optimizer import optimize_team, optimize_trajectory
    zeros = torch.zeros(90_000, device=dev)   # a zero prior: optimize_trajectory takes the separate calls as well
    a, b = _model(dev, prior_log_odds=zeros, **SEG), _model(dev, prior_log_odds=zeros, **SEG)
    # TeamTraj's forward carries the swept term: a team of one has the model's loss['clearance']
    team = TeamTraj([_model(dev, **SEG)])
    team(vis_wps_dist=0.0)
    single = _model(dev, **SEG)
    single(vis_wps_dist=0.0)
    assert float(team.loss["clearance"][0]) == float(single.loss["clearance"]) > 0.0
    run = dict(n_opt_steps=10, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, smoothness_th=1e9, vis_wps_dist=0.0)
    ra, rb = optimize_trajectory(a, **run), optimize_team([b], **run)
    assert ra.steps_taken == rb.steps_taken == 10 and ra.losses == rb.losses
    assert torch.equal(a.poses.data, b.poses.data) and torch.equal(a.quats.data, b.quats.data) and torch.equal(a.rewards, b.rewards)
    for k in TERMS:
        assert float(a.loss[k]) == float(b.loss[k]), k


@pytest.mark.parametrize("mode", ["waypoints", "segments"])
def test_weight_zero_is_the_model_without_the_term(dev, mode):
    from trajectory_optimization_amd import optimizer as O
    a, b = _model(dev), _model(dev, clearance_weight=0.0, clearance_radius=0.6, clearance_mode=mode)
    la, lb = a(vis_wps_dist=0.0), b(vis_wps_dist=0.0)
    assert "clearance" not in b.loss and float(la) == float(lb) and torch.equal(a.rewards, b.rewards)
    la.backward()
    lb.backward()
    assert torch.equal(a.poses.grad, b.poses.grad) and torch.equal(a.quats.grad, b.quats.grad)
    ra = O.optimize_trajectory(a, 5, 0.05, 0.01, 1e9, 1e9, 0.0)
    rb = O.optimize_trajectory(b, 5, 0.05, 0.01, 1e9, 1e9, 0.0)
    assert ra.losses == rb.losses and torch.equal(a.poses.data, b.poses.data) and "clearance" not in b.loss


def test_the_default_mode_is_the_model_without_the_keyword(dev):
    from trajectory_optimization_amd import optimizer as O
    a, b = _model(dev, **CLR), _model(dev, clearance_mode="waypoints", **CLR)
    assert a.clearance_mode == "waypoints"
    la, lb = a(vis_wps_dist=0.0), b(vis_wps_dist=0.0)
    assert torch.equal(la, lb) and torch.equal(a.rewards, b.rewards)
    for k in TERMS:
        assert torch.equal(a.loss[k], b.loss[k])
    la.backward()
    lb.backward()
    assert torch.equal(a.poses.grad, b.poses.grad) and torch.equal(a.quats.grad, b.quats.grad)
    ra = O.optimize_trajectory(a, 5, 0.05, 0.01, 1e9, 1e9, 0.0)
    rb = O.optimize_trajectory(b, 5, 0.05, 0.01, 1e9, 1e9, 0.0)
    assert ra.losses == rb.losses and torch.equal(a.poses.data, b.poses.data) and torch.equal(a.rewards, b.rewards)


def test_the_mode_follows_the_attribute(dev):
    a, s, w = _model(dev, **CLR), _model(dev, **SEG), _model(dev, **CLR)
    a(vis_wps_dist=0.0)
    plan = a._plan_obj
    a.clearance_mode = "segments"
    la, ls = a(vis_wps_dist=0.0), s(vis_wps_dist=0.0)
    assert a._plan_obj is not plan
    assert torch.equal(la, ls) and torch.equal(a.loss["clearance"], s.loss["clearance"])
    a.clearance_mode = "waypoints"
    la, lw = a(vis_wps_dist=0.0), w(vis_wps_dist=0.0)
    assert torch.equal(la, lw) and torch.equal(a.loss["clearance"], w.loss["clearance"])
    assert float(s.loss["clearance"]) != float(w.loss["clearance"])
    with pytest.raises(ValueError):
        a.clearance_mode = "edges"
    assert a.clearance_mode == "waypoints"
    a.set_clearance(0.6, 2.0, "segments")
    assert a.clearance_mode == "segments" and torch.equal(a(vis_wps_dist=0.0), ls)


# ---- 6. behaviour ---------------------------------------------------------------------------------------------------------------------------

BEHAVIOUR_WEIGHT = 50.0


def _pillar_row_scene():
    """tests/test_hip_clearance.py's wall case — a wall of points (the plane y = 0) with a denser block behind it that the cameras
    face — with a row of thin pillars (columns of points) across the path's corridor: the path runs 0.6 m in front of the wall, its 11
    waypoints 1 m apart, and a pillar stands 0.05 m beside the midpoint of every segment, 0.5 m from both of its waypoints.  With
    r = 0.4 no waypoint is within r of anything at the start.  -> (points, poses, quats, r, number of pillar points: the last rows)."""
    xs, zs = np.arange(-4.0, 14.0, 0.1), np.arange(-2.0, 2.0, 0.1)
    X, Z = np.meshgrid(xs, zs)
    wall = np.stack([X.ravel(), np.zeros(X.size), Z.ravel()], 1)
    block = np.random.default_rng(3).uniform((-2.0, 1.5, -1.5), (12.0, 4.0, 1.5), (60_000, 3))
    W, y0, r = 11, -0.6, 0.4
    px = np.linspace(0.0, 10.0, W)
    z = np.arange(-2.0, 2.0001, 0.05)
    pillars = np.concatenate([np.stack([np.full_like(z, m), np.full_like(z, y0 + 0.05), z], 1) for m in 0.5 * (px[:-1] + px[1:])])
    pts = np.concatenate([wall, block, pillars]).astype(f32)
    p = np.stack([px, np.full(W, y0), np.zeros(W)], 1).astype(f32)
    q = np.tile(np.array([np.sqrt(0.5), -np.sqrt(0.5), 0.0, 0.0], f32), (W, 1))   # camera z (optical axis) along world +y
    return pts, p, q, r, len(pillars)


def test_the_swept_term_keeps_the_segments_off_a_row_of_pillars(dev):
    """150 steps of tests/test_hip_clearance.py's wall run (lr 0.02, weight 50).  The waypoint term ends with every waypoint at least
    0.9 r from the cloud and a segment within r / 2 of a pillar: it passes between its waypoints (measured: waypoints 1.01 r, segments
    0.056 m = 0.14 r, the same on the commit before the mode existed).  The swept term ends with every segment further from the cloud
    than that and at least r / 2 from it (measured: 0.396 m = 0.99 r).  Distances: an f64 numpy restatement, not the library's query."""
    from trajectory_optimization_amd import optimizer as O, tools
    from trajectory_optimization_amd.model import ModelTraj
    pts, p, q, r, n_pillar = _pillar_row_scene()
    ends = {}
    for mode in ("waypoints", "segments"):
        m = ModelTraj(torch.from_numpy(pts), torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev,
                      clearance_radius=r, clearance_weight=BEHAVIOUR_WEIGHT, clearance_mode=mode)
        O.optimize_trajectory(m, 150, 0.02, 0.0, 1e9, 1e9, 0.0)
        P = m.poses.data.cpu().numpy()
        d, _ = tools.trajectory_clearance(m, m.poses.data, 10.0)
        ends[mode] = (float(d.min()), float(seg_dist64(pts, P)[0].min()), float(seg_dist64(pts[-n_pillar:], P)[0].min()))
        print(mode, "min waypoint distance %.4f, min segment distance %.4f (to a pillar %.4f), r = %.1f" % (*ends[mode], r))
    assert ends["waypoints"][0] >= 0.9 * r and ends["waypoints"][2] < 0.5 * r, ends
    assert ends["segments"][1] > ends["waypoints"][1] and ends["segments"][1] >= 0.5 * r, ends
