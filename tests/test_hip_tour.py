"""The tour planner on the GPU (tools.plan_tour, tour_kernels.hip; the edge stage tohip_clearance_edges, clearance_kernels.hip): the
edge query against the 16-wave segment query and a numpy brute force of the definition, bit for bit; the tour against the numpy
restatement of its definition (synth.tour_plan), element for element; a walled scene with a doorway and an enclosed node; the
circle and the line; and the chain select_views -> plan_tour -> ModelTraj(clearance_mode='segments') on the bundled cloud."""
import os

import numpy as np
import pytest
import torch

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def brute_edges(pts, A, B, r):
    """numpy restatement of the segment query for the edges A[e] -> B[e]: f32 without contraction, finite rows only, d2 < fl(r r), ties
    to the lowest row; d = (float)sqrt((double)d2); s in f64 from the f32 coordinates, summed in x, y, z order -> (d, idx, s)."""
    pts, A, B = np.asarray(pts, f32), np.asarray(A, f32), np.asarray(B, f32)
    r2 = f32(r) * f32(r)
    fin = np.isfinite(pts).all(axis=1)
    E = len(A)
    d_out, i_out, s_out = np.full(E, np.inf, f32), np.full(E, -1, np.int32), np.zeros(E, f32)
    for k in range(E):
        a, b = A[k], B[k]
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            e = (b - a).astype(f32)
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
            a64, b64, x64 = a.astype(f64), b.astype(f64), pts[i].astype(f64)
            ee64 = dot64 = 0.0
            for c in range(3):
                ek, uk = b64[c] - a64[c], x64[c] - a64[c]
                ee64 += ek * ek
                dot64 += uk * ek
            i_out[k], d_out[k] = i, f32(np.sqrt(f64(d2[i])))
            s_out[k] = f32(min(max(dot64 / ee64, 0.0), 1.0)) if ee64 > 0 else f32(0.0)
    return d_out, i_out, s_out


def all_pairs(P):
    i, j = np.triu_indices(len(P), 1)
    return P[i], P[j]


def edge_case(N, E):
    """A cloud with NaN rows and E edges among it: all pairs of 33 nodes at E = 528, else random ends; a zero-length edge, an edge with
    a non-finite end and (whenever E allows) an edge far from every point."""
    rng = np.random.default_rng(1000 * E + N)
    pts = synth.make_cloud(N, seed=N).astype(f32)
    pts[rng.choice(N, max(1, N // 50), replace=False), rng.integers(0, 3)] = np.nan
    lo, hi = np.nanmin(pts, axis=0), np.nanmax(pts, axis=0)
    if E == 528:
        A, B = all_pairs(rng.uniform(lo, hi, (33, 3)).astype(f32))
        A, B = A.copy(), B.copy()
    else:
        A, B = rng.uniform(lo, hi, (E, 3)).astype(f32), rng.uniform(lo, hi, (E, 3)).astype(f32)
        short = rng.random(E) < 0.5   # half of them short: only a few tiles survive the prune
        B[short] = A[short] + rng.normal(0, 0.5, (int(short.sum()), 3)).astype(f32)
    if E == 1:
        B[0] = A[0]                   # the zero-length edge
    else:
        B[E // 2] = A[E // 2]
        A[E - 1, 1] = np.inf          # a non-finite end
    if E > 2:
        A[1], B[1] = hi + f32(50.0), hi + f32(60.0)   # no point within the radius
    return pts, A, B


EDGE_CASES = [(200, 1), (257, 7), (5_000, 300), (20_000, 528)]
_edge_refs = {}


def edge_ref(N, E, r):
    key = (N, E)
    if key not in _edge_refs:
        pts, A, B = edge_case(N, E)
        _edge_refs[key] = (pts, A, B, brute_edges(pts, A, B, r))
    return _edge_refs[key]


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("N,E", EDGE_CASES)
def test_edge_query_equals_the_segment_query_and_the_definition(dev, N, E, sort):
    from trajectory_optimization_amd import ops, tools
    r = 4.0 if N <= 257 else 0.4
    pts, A, B, want = edge_ref(N, E, r)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=sort)
    a, b = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    got = ops.clearance_edges(cloud, a, b, r)
    base = ops.clearance_segments(cloud, torch.stack([a, b], dim=1).reshape(-1, 3), r, n_traj=E)
    for g, s, w, name in zip(got, base, want, ("d", "idx", "s")):
        assert torch.equal(g, s), name
        assert np.array_equal(g.cpu().numpy(), w), name
    idx = got[1].cpu().numpy()
    assert idx[E // 2] == brute_edges(pts, A[E // 2:E // 2 + 1], A[E // 2:E // 2 + 1], r)[1][0]   # the zero-length edge: the point query
    if E > 1:
        assert idx[E - 1] == -1 and np.isinf(got[0][E - 1].item()) and got[2][E - 1].item() == 0.0
        assert (idx >= 0).any()
    if E > 2:
        assert idx[1] == -1
    again = tools.edge_clearance(cloud, a, b, r)
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    # a radius no point is within; outputs left out
    far = ops.clearance_edges(cloud, a, b, 1e-7)
    assert bool((far[1] == -1).all()) and bool(torch.isinf(far[0]).all()) and bool((far[2] == 0).all())


def tour_case(n):
    """n nodes with two identical ones and (n >= 12) one that is not finite, and a random symmetric set of blocked pairs — dense
    enough at the larger n for detours and unreachable nodes."""
    rng = np.random.default_rng(n)
    P = rng.uniform(-10, 10, (n, 3)).astype(f32)
    if n >= 3:
        P[n - 1] = P[1]
    if n >= 12:
        P[5, 2] = np.nan
    E = n * (n - 1) // 2
    p_block = {2: 0.0, 3: 0.0, 12: 0.5, 64: 0.9, 256: 0.97}[n]
    hit = rng.random(E) < p_block
    i, j = np.triu_indices(n, 1)
    blocked = np.zeros((n, n), dtype=bool)
    blocked[i, j] = blocked[j, i] = hit
    return P, blocked, np.where(hit, rng.integers(0, 1000, E), -1).astype(np.int32)


_tour_refs = {}


def tour_ref(n, closed, max_moves):
    key = (n, closed, max_moves)
    if key not in _tour_refs:
        P, blocked, _ = tour_case(n)
        _tour_refs[key] = synth.tour_plan(P, blocked, closed, max_moves)
    return _tour_refs[key]


def read_tour(buf, n):
    from trajectory_optimization_amd import ops
    lay, h = ops.tour_layout(n), buf.cpu()
    hdr = h[:64].view(torch.int64).tolist()
    return dict(m=hdr[0], moves=hdr[1], converged=bool(hdr[2]), length_fixed=hdr[3], nn_length_fixed=hdr[4], status=hdr[5],
                order=h[lay["order"]:lay["order"] + 4 * n].view(torch.int32).numpy(),
                unreachable=h[lay["unreachable"]:lay["unreachable"] + n].numpy() != 0,
                D=h[lay["D"]:lay["D"] + 8 * n * n].view(torch.int64).numpy().reshape(n, n),
                nxt=h[lay["nxt"]:lay["nxt"] + 4 * n * n].view(torch.int32).numpy().reshape(n, n))


def check_tour_entry(dev, n, closed, max_moves, via):
    """One entry's buffer against the restatement.  via: through ops.tour_plan_via with routes that beat no leg — all 2^62, in a
    table wider than n — so the legs, and with them the whole buffer, are those of ops.tour_plan, and no flag is set."""
    from trajectory_optimization_amd import ops
    P, _, edge_idx = tour_case(n)
    want = tour_ref(n, closed, max_moves)
    nodes, idx = torch.from_numpy(P).to(dev), torch.from_numpy(edge_idx).to(dev)
    via_D = torch.full((n, n + 3), synth.TOUR_INF, dtype=torch.int64, device=dev) if via else None
    for run in range(2):
        if via:
            buf, flag = ops.tour_plan_via(nodes, idx, via_D, closed, max_moves)
            assert flag.dtype == torch.uint8 and tuple(flag.shape) == (n, n) and not bool(flag.any())
        else:
            buf = ops.tour_plan(nodes, idx, closed, max_moves)
        got = read_tour(buf, n)
        for k in ("m", "moves", "converged", "length_fixed", "nn_length_fixed"):
            assert got[k] == want[k], (k, run)
        for k in ("order", "unreachable", "D", "nxt"):
            assert np.array_equal(got[k], want[k]), (k, run)
        assert got["status"] == 0
    if max_moves == 0:
        assert want["moves"] == 0 and want["length_fixed"] == want["nn_length_fixed"]
    if n == 256 and max_moves is None:   # the case is not a trivial one
        assert want["moves"] > 1 and want["converged"] and want["unreachable"].sum() >= 1 and want["m"] > 200
        assert (want["D"][want["D"] < synth.TOUR_INF] > np.where(want["w"] >= 0, want["w"], 0)[want["D"] < synth.TOUR_INF]).any()


@pytest.mark.parametrize("max_moves", [0, 1, None])
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("n", [2, 3, 12, 64, 256])
def test_tour_equals_the_restatement(dev, n, closed, max_moves):
    check_tour_entry(dev, n, closed, max_moves, via=False)


@pytest.mark.parametrize("max_moves", [0, 1, None])
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("n", [2, 3, 12, 64, 256])
def test_tour_via_entry_equals_the_restatement(dev, n, closed, max_moves):
    """Both entries launch one init kernel: the second one's null-free arguments and its leading dimension, against the CPU
    restatement (not against the other entry, which would compare the kernel with itself)."""
    check_tour_entry(dev, n, closed, max_moves, via=True)


def walled_scene():
    """A wall in the plane x = 0 with a doorway (|y| < 0.8) and a node in it, nodes on both sides of the wall, and node 6 inside a
    shell of points.  -> (pts, nodes, radius)"""
    y, z = np.meshgrid(np.arange(-3.0, 3.0001, 0.1), np.arange(-1.0, 1.0001, 0.1), indexing="ij")
    wall = np.stack([np.zeros(y.size), y.ravel(), z.ravel()], axis=1)
    wall = wall[np.abs(wall[:, 1]) > 0.75]
    k = np.arange(400) + 0.5
    phi, th = np.arccos(1 - 2 * k / 400), np.pi * (1 + 5 ** 0.5) * k
    shell = np.float64([5.0, 5.0, 0.0]) + 0.5 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    nodes = f32([[-3, 0, 0], [1, -2.5, 0], [-2, 2.5, 0], [0, 0, 0], [1, 2.5, 0], [-2, -2.5, 0], [5, 5, 0]])
    return np.concatenate([wall, shell]).astype(f32), nodes, 0.25


@pytest.mark.parametrize("closed", [False, True])
def test_walled_scene_detours_through_the_doorway(dev, closed):
    from trajectory_optimization_amd import tools
    pts, P, r = walled_scene()
    n = len(P)
    A, B = all_pairs(P)
    i, j = np.triu_indices(n, 1)
    blocked = np.zeros((n, n), dtype=bool)
    blocked[i, j] = blocked[j, i] = brute_edges(pts, A, B, r)[1] >= 0
    ref = synth.tour_plan(P, blocked, closed)
    # the scene is not vacuous, by the restatement's own account
    w, D = ref["w"], ref["D"]
    assert blocked.any() and ((D < synth.TOUR_INF) & (D > w)).any() and ref["unreachable"].tolist() == [False] * 6 + [True]
    cloud = torch.from_numpy(pts).to(dev)
    t = tools.plan_tour(cloud, torch.from_numpy(P), clearance_radius=r, closed=closed)
    assert t.order.tolist() == ref["order"][:ref["m"]].tolist() and t.walk == ref["walk"] and t.unreachable.tolist() == ref["unreachable"].tolist()
    assert np.array_equal(t.blocked.numpy(), blocked) and np.array_equal(t.D.numpy(), D) and np.array_equal(t.nxt.numpy(), ref["nxt"])
    assert (t.length_fixed, t.nn_length_fixed, t.moves, t.converged) == (ref["length_fixed"], ref["nn_length_fixed"], ref["moves"], ref["converged"])
    # every leg of the walk keeps the radius, the walk holds every reachable node and no other, and its length is the sum of its legs
    a, b = t.poses[:-1], t.poses[1:]
    assert torch.equal(t.poses.cpu(), torch.from_numpy(P)[t.walk]) and t.quats is None
    d, idx, _ = tools.edge_clearance(cloud, a, b, r)
    assert bool((idx == -1).all()) and bool(torch.isinf(d).all())
    assert set(t.walk) == set(range(6)) and t.walk[0] == 0 and (t.walk[-1] == 0) == closed
    assert t.length_fixed == sum(int(w[u, v]) for u, v in zip(t.walk, t.walk[1:])) and len(t.walk) > len(t.order) + closed
    assert t.walk.count(3) == 2   # a detour: the doorway is passed a second time
    assert t.length <= t.nn_length and t.length == t.length_fixed * 2.0 ** -20
    assert t.converged and int(synth.tour_two_opt_changes(D, t.order.numpy(), closed).min()) >= 0
    ed = t.edge_distance.cpu().numpy()
    assert np.array_equal(np.isfinite(ed), blocked) and np.array_equal(ed, ed.T)


def test_circle_and_line_through_the_public_call(dev):
    from trajectory_optimization_amd import tools
    cloud = torch.from_numpy(synth.make_cloud(3_000, seed=3) + f32([500.0, 0.0, 0.0])).to(dev)   # far from every node
    th = 2 * np.pi * np.arange(16) / 16
    ring = np.stack([5 * np.cos(th), 5 * np.sin(th), np.zeros(16)], axis=1).astype(f32)
    perm = np.random.default_rng(5).permutation(16)
    x = np.concatenate([[-3.0], np.random.default_rng(6).permutation(40)[:12] * 0.75])
    line = (f32([[1.0, 2.0, 0.5]]) + x[:, None] * f32([[0.6, 0.0, 0.8]])).astype(f32)
    quats = torch.nn.functional.normalize(torch.from_numpy(np.random.default_rng(7).normal(size=(16, 4)).astype(f32)), dim=1)
    for P, closed, q in ((ring[perm], True, quats), (line, False, None)):
        free = tools.plan_tour(cloud, torch.from_numpy(P), q, clearance_radius=None, closed=closed)
        kept = tools.plan_tour(cloud, torch.from_numpy(P), q, clearance_radius=2.0, closed=closed)
        ref = synth.tour_plan(P, None, closed)
        for t in (free, kept):
            assert t.order.tolist() == ref["order"].tolist() and t.walk == ref["walk"] and not t.unreachable.any() and not t.blocked.any()
            assert (t.length_fixed, t.nn_length_fixed, t.moves, t.converged) == (ref["length_fixed"], ref["nn_length_fixed"], ref["moves"], True)
            assert np.array_equal(t.D.numpy(), ref["D"]) and np.array_equal(t.nxt.numpy(), ref["nxt"])
            assert bool(torch.isinf(t.edge_distance).all())
            if q is not None:
                assert torch.equal(t.quats.cpu(), q[t.walk])
    ring_t = tools.plan_tour(cloud, torch.from_numpy(ring[perm]), closed=True)
    step = np.diff(np.append(perm[ring_t.order.numpy()], perm[ring_t.order[0]])) % 16
    assert (step == 1).all() or (step == 15).all()
    assert abs(ring_t.length - 16 * 2 * 5 * np.sin(np.pi / 16)) < 1e-4
    line_t = tools.plan_tour(cloud, torch.from_numpy(line))
    assert line_t.order.tolist() == np.argsort(x, kind="stable").tolist()


BUNDLED_RADIUS = 0.008   # the bundled cloud holds the ground the bundled path runs on, 9 mm below its first waypoint


def test_selected_views_become_a_path_the_swept_term_accepts(dev):
    """select_views -> plan_tour -> ModelTraj(clearance_mode='segments') on the bundled cloud: the swept clearance term of the planned
    path is exactly 0 at the first forward, whichever way the cloud is handed over."""
    from trajectory_optimization_amd import ops, tools
    from trajectory_optimization_amd.model import ModelTraj
    d = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
    pts_np, path = np.ascontiguousarray(d["pts"], dtype=f32), np.ascontiguousarray(d["poses"], dtype=f32)
    K, iw, ih = tools.load_intrinsics(device=dev)
    quats = torch.from_numpy(np.tile(f32([1.0, 0.0, 0.0, 0.0]), (len(path), 1)))
    model = ModelTraj(torch.from_numpy(pts_np), torch.from_numpy(path), quats, K, iw, ih, device=dev)
    cp, cq = synth.bundled_candidate_grid(pts_np, path)
    sel = tools.select_views(model, torch.from_numpy(cp), torch.from_numpy(cq), 8)
    poses = torch.cat([model.poses.data[:1], sel.poses])
    qs = torch.cat([model.quats.data[:1], sel.quats])
    r = BUNDLED_RADIUS
    t = tools.plan_tour(model, poses, qs, clearance_radius=r)
    assert t.blocked.any() and len(t.walk) >= len(t.order) >= 3 and t.length <= t.nn_length and t.converged
    assert torch.equal(t.poses, poses[torch.as_tensor(t.walk, device=dev)]) and torch.equal(t.quats, qs[torch.as_tensor(t.walk, device=dev)])
    planned = ModelTraj.sharing_cloud_of(model, t.poses, t.quats, clearance_radius=r, clearance_weight=5.0, clearance_mode="segments")
    planned(vis_wps_dist=0.0)
    assert float(planned.loss["clearance"].detach()) == 0.0
    # the selection order itself is not such a path: some of its legs come within the radius
    naive = ModelTraj.sharing_cloud_of(model, poses, qs, clearance_radius=r, clearance_weight=5.0, clearance_mode="segments")
    naive(vis_wps_dist=0.0)
    assert float(naive.loss["clearance"].detach()) > 0.0
    for first in (torch.from_numpy(pts_np).to(dev), ops.PackedCloud(torch.from_numpy(pts_np).to(dev), sort=False)):
        u = tools.plan_tour(first, poses, qs, clearance_radius=r)
        assert u.walk == t.walk and u.length_fixed == t.length_fixed and torch.equal(u.blocked, t.blocked)
        assert torch.equal(u.edge_distance, t.edge_distance) and torch.equal(u.D, t.D)


def test_the_example_runs(dev):
    import importlib.util
    spec = importlib.util.spec_from_file_location("view_tour_sample", os.path.join(REPO, "examples", "view_tour_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--opt-steps", "3"])
    assert out["planned_length"] <= out["nn_length"] and out["clearance_planned_start"] == 0.0 and out["n_walk"] >= 3
    assert all(np.isfinite(out[k]) for k in ("selection_length", "reward_before", "reward_after"))
