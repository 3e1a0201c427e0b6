"""The yardsticks far from the origin (no GPU).  tests/test_hip_far_from_origin.py compares every kernel at a translation T with
itself at the origin, bit for bit; that proves something only if the references it leans on are themselves invariant.  With every
input on a 2^-10 m grid within +-32 m and |T_k| in {2^12, 2^13}, every translated coordinate is representable in float32 and every
difference x - t, b - a, x - origin has the bits of the untranslated one — so the f32 oracle, the numpy brute forces of the three
clearance queries, synth.tour_plan and the coverage map's restatement must each return the same bits at T as at the origin."""
import numpy as np

from trajectory_optimization_amd import synth

K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
f32 = np.float32
T = np.array([8192.0, -8192.0, 4096.0], dtype=f32)
GRID = 1024.0   # 2^10 steps per metre


def snap(a):
    """round(a 2^10) / 2^10 as float32: the nearest point of the 2^-10 m grid (+ 0.0: a -0.0 becomes +0.0, which is what
    (a + T) - T gives back)."""
    return (np.rint(np.asarray(a, dtype=np.float64) * GRID) / GRID + 0.0).astype(f32)


def shifted(a, t=T):
    """a + t in float32, checked to be exact: (a + t) - t gives back a's bits, so the translated run sees the same differences."""
    a = np.asarray(a, dtype=f32)
    out = (a + np.asarray(t, dtype=f32)).astype(f32)
    back = (out - np.asarray(t, dtype=f32)).astype(f32)
    ok = np.isfinite(a)
    assert np.array_equal(back[ok].view(np.uint32), (a[ok] + f32(0.0)).view(np.uint32)), "the translation is not exact on this fixture"
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def cloud(n=20_000, seed=3):
    return snap(synth.make_cloud(n, seed=seed))


def path(W=9, seed=3):
    p, q = synth.make_path(W, optical=True, jitter_seed=seed)
    return snap(p), q


def queries(pts, seed, n_in=40, snapped=True):
    """Point queries (on the grid unless snapped=False): inside the slab, 2^-10 m off a cloud point, exactly on one, and far away."""
    rng = np.random.default_rng(seed)
    lo, hi = pts.min(0), pts.max(0)
    inside = rng.uniform(lo, hi, (n_in, 3))
    near = pts[rng.integers(0, len(pts), 4)] + f32(1.0 / GRID)
    on = pts[rng.integers(0, len(pts), 2)]
    far = hi + 8.0 + rng.uniform(0, 2, (3, 3))
    out = np.concatenate([inside, near, on, far])
    return snap(out) if snapped else out.astype(f32)


def segments(pts, seed, n_short=24, snapped=True):
    """(E, 2, 3) segments (on the grid unless snapped=False): short ones inside the slab, a long one, a zero-length one and one far
    from every point."""
    rng = np.random.default_rng(seed)
    lo, hi = pts.min(0), pts.max(0)
    a = rng.uniform(lo, hi, (n_short, 3))
    short = np.stack([a, a + rng.uniform(-0.6, 0.6, (n_short, 3))], 1)
    long = np.array([[[-5.0, -3.0, 0.0], [4.5, 0.125, 0.625]]])
    z = rng.uniform(lo, hi, (1, 3))
    zero = np.stack([z, z], 1)
    fa = hi + 8.0 + rng.uniform(0, 2, (1, 3))
    far = np.stack([fa, fa + 0.5], 1)
    out = np.concatenate([short, long, zero, far])
    return snap(out) if snapped else out.astype(f32)


def walled_scene():
    """tests/test_hip_tour.py's walled scene on the grid (the doorway, the detour and the enclosed node survive the snapping: the
    CPU test below asserts it)."""
    from test_hip_tour import walled_scene as scene
    pts, nodes, r = scene()
    return snap(pts), snap(nodes), r


def test_snap_and_translation_are_exact():
    """Every fixture the GPU tests translate: on the grid, within +-32 m, and (a + T) - T == a bitwise."""
    pts, (p, _) = cloud(), path()
    wall, nodes, _ = walled_scene()
    for name, a in (("cloud", pts), ("cloud 300k", cloud(300_000, 5)), ("path", p), ("path 33", path(33, 7)[0]), ("queries", queries(pts, 1)),
                    ("segments", segments(pts, 2)), ("wall", wall), ("nodes", nodes)):
        assert a.dtype == f32 and np.array_equal(snap(a), a), name
        assert float(np.abs(a).max()) <= 32.0, name
        for t in (T, -T, T[[2, 0, 1]]):
            s = shifted(a, t)
            assert np.array_equal((s - t).astype(f32), a), name
            assert np.array_equal(s.astype(np.float64), a.astype(np.float64) + t.astype(np.float64)), name
    assert np.array_equal(np.abs(T), f32([2 ** 13, 2 ** 13, 2 ** 12]))
    assert len(np.unique(pts, axis=0)) == len(pts)   # snapping made no duplicate rows


def test_f32_oracle_is_translation_invariant():
    from oracle import oracle
    pts, (p, q) = cloud(), path()
    out = []
    for t in (None, T):
        x, w = (pts, p) if t is None else (shifted(pts, t), shifted(p, t))
        f = oracle.traj_forward(x, w, q, K, IW, IH, prec="f32")
        pg, qg = oracle.traj_backward(x, w, q, K, IW, IH, f, prec="f32")
        out.append(dict(lo_sum=f["lo_sum"], rewards=f["rewards"], pmin=f["pmin"], pmax=f["pmax"], mean=np.float64(f["mean_reward"]),
                        loss=np.float64(f["loss_vis"]), poses_grad=pg, quats_grad=qg))
    for k in out[0]:
        assert same(out[0][k], out[1][k]), k
    assert int((out[0]["rewards"] > 0.5).sum()) > 100 and float(np.abs(out[0]["poses_grad"]).max()) > 1e-4   # the case is live


def test_pose_oracle_is_translation_invariant():
    from oracle import oracle
    pts, (p, q) = cloud(), path()
    out = []
    for t in (None, T):
        x, w = (pts, p) if t is None else (shifted(pts, t), shifted(p, t))
        obs, loss = oracle.pose_forward(x, w[4:5], q[4:5], K, IW, IH, prec="f32")
        tg, qg = oracle.pose_backward(x, w[4:5], q[4:5], K, IW, IH, loss, prec="f32")
        out.append(dict(observations=obs, loss=np.float64(loss), trans_grad=tg, quat_grad=qg))
    for k in out[0]:
        assert same(out[0][k], out[1][k]), k
    assert float(out[0]["observations"].sum()) > 1.0


def test_clearance_brute_forces_are_translation_invariant():
    from test_hip_clearance import brute as brute_points
    from test_hip_clearance_segments import brute as brute_segments
    from test_hip_tour import brute_edges
    pts = cloud()
    q, segs, r = queries(pts, 1), segments(pts, 2), 1.0
    A, B = segs[:, 0], segs[:, 1]
    want = (brute_points(pts, q, r), brute_segments(pts, segs.reshape(-1, 3), r, n_traj=len(segs)), brute_edges(pts, A, B, r))
    X = shifted(pts)
    got = (brute_points(X, shifted(q), r), brute_segments(X, shifted(segs.reshape(-1, 3)), r, n_traj=len(segs)),
           brute_edges(X, shifted(A), shifted(B), r))
    for name, w, g in zip(("points", "segments", "edges"), want, got):
        for j, (a, b) in enumerate(zip(w, g)):
            assert same(a, b), (name, j)
        assert int((w[1] >= 0).sum()) >= len(w[1]) // 3, name   # the radius finds a point for a third of them or more
    assert want[0][1][-1] == -1 and want[1][1][-1] == -1 and want[2][1][-1] == -1   # the far ones find none
    assert float(want[0][0][44:46].max()) == 0.0   # the queries that sit on a cloud point


def test_tour_restatement_is_translation_invariant():
    from test_hip_tour import all_pairs, brute_edges
    pts, P, r = walled_scene()
    n = len(P)
    out = []
    for t in (None, T):
        x, nodes = (pts, P) if t is None else (shifted(pts, t), shifted(P, t))
        A, B = all_pairs(nodes)
        i, j = np.triu_indices(n, 1)
        blocked = np.zeros((n, n), dtype=bool)
        blocked[i, j] = blocked[j, i] = brute_edges(x, A, B, r)[1] >= 0
        out.append((blocked, {closed: synth.tour_plan(nodes, blocked, closed) for closed in (False, True)}))
    assert np.array_equal(out[0][0], out[1][0]), "blocked"
    for closed in (False, True):
        a, b = out[0][1][closed], out[1][1][closed]
        for k in a:
            assert a[k] == b[k] if not isinstance(a[k], np.ndarray) else np.array_equal(a[k], b[k]), (closed, k)
        # the snapped scene is still the one tests/test_hip_tour.py describes: a blocked pair, a detour, the enclosed node left out
        assert out[0][0].any() and ((a["D"] < synth.TOUR_INF) & (a["D"] > a["w"])).any() and a["unreachable"].tolist() == [False] * 6 + [True]
        assert a["walk"].count(3) == 2


COVMAP_ORIGIN, COVMAP_R = f32([0.25, -0.5, 0.125]), 0.5   # (index + 1/2) r lies on the grid: the translated centres are exact


def covmap_rows(n=20_000):
    rng = np.random.default_rng(17)
    row = (rng.random(n) * 5.0).astype(f32)
    row[rng.random(n) < 0.2] = 0.0
    return row


def test_covmap_restatement_is_translation_invariant():
    from test_hip_covmap import RefMap
    pts, other, row = cloud(), cloud(5_000, 8), covmap_rows()
    out = []
    for t in (None, T):
        x, y, o = (pts, other, COVMAP_ORIGIN) if t is None else (shifted(pts, t), shifted(other, t), shifted(COVMAP_ORIGIN, t))
        ref = RefMap(o, COVMAP_R, clamp=4.0)
        ref.integrate(x, row, "max")
        ref.integrate(x[::3], row[::3], "add")
        out.append((ref.export(), ref.lookup(y), ref.lookup(x), ref.skipped))
    (c0, v0, k0), (c1, v1, k1) = out[0][0], out[1][0]
    assert np.array_equal(k0, k1), "keys"
    assert same(v0, v1), "values"
    assert same(shifted(c0), c1), "centres"
    assert same(out[0][1], out[1][1]) and same(out[0][2], out[1][2]), "lookup"
    assert out[0][3] == out[1][3] == 0 and 1000 < len(k0) < len(pts) and float(out[0][1].max()) > 0.0
