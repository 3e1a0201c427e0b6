"""The travel field without a GPU: the numpy restatements (synth.travel_*) against a plain heapq Dijkstra and scipy's, the hand cases
of the move rule, truncation, ops.check_travel's errors by name, the ABI entries and the pick's restatement."""
import numpy as np
import pytest

import abi_cases
import travel_cases as tc
from trajectory_optimization_amd import synth

ENTRIES = ["tohip_travel_bytes", "tohip_travel_workspace_bytes", "tohip_travel_build", "tohip_travel_positions", "tohip_travel_paths",
           "tohip_view_volume_pick_travel"]


def _random_T(dims, p, seed):
    return np.random.default_rng(seed).random(dims) < p


RANDOM = [((1, 1, 1), 1.0, 0), ((5, 6, 3), 0.8, 1), ((9, 4, 7), 0.6, 2), ((12, 11, 5), 0.7, 3), ((6, 6, 6), 1.0, 4), ((7, 8, 3), 0.0, 5)]


@pytest.mark.parametrize("dims,p,seed", RANDOM, ids=str)
def test_travel_ref_equals_a_heapq_dijkstra(dims, p, seed):
    T = _random_T(dims, p, seed)
    rng = np.random.default_rng(100 + seed)
    for n_seeds in (1, 3):
        seeds = rng.integers(0, np.asarray(dims), size=(n_seeds, 3))
        if T.any():
            seeds[0] = np.argwhere(T)[rng.integers(int(T.sum()))]
        want = tc.dijkstra(T, seeds)
        got = synth.travel_ref(T, seeds)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert ((got >= 0) <= T).all() and (T.any() == (got == 0).any())


@pytest.mark.parametrize("dims,p,seed", RANDOM[1:5], ids=str)
def test_travel_ref_equals_scipy_dijkstra(dims, p, seed):
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    T = _random_T(dims, p, seed)
    lin = np.arange(T.size).reshape(T.shape)
    rows, cols, vals = [], [], []
    for m, ok in synth.travel_allowed_ref(T).items():
        d = synth.TRAVEL_MOVES[m]
        v = np.argwhere(ok)
        rows.append(lin[tuple(v.T)])
        cols.append(lin[tuple((v + np.asarray(d)).T)])
        vals.append(np.full(len(v), synth.TRAVEL_WEIGHTS[sum(1 for k in d if k) - 1], dtype=np.float64))
    graph = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(T.size, T.size))
    seed_v = np.argwhere(T)[0]
    dist = csgraph.dijkstra(graph, directed=True, indices=int(lin[tuple(seed_v)]))
    want = np.where(np.isfinite(dist), dist, -1).astype(np.int64).reshape(T.shape)
    assert np.array_equal(synth.travel_ref(T, seed_v[None]), want)


@pytest.mark.parametrize("name", sorted(tc.hand_cases()))
def test_hand_cases_of_the_move_rule(name):
    T, src, want = tc.hand_cases()[name]
    got = synth.travel_ref(T, np.asarray([src]))
    for v, c in want.items():
        assert got[v] == c, (name, v, int(got[v]), c)
    assert np.array_equal(got, tc.dijkstra(T, [src]))


def test_the_serpentine_runs_every_lane():
    T, src, goal = tc.serpentine()
    cost = synth.travel_ref(T, np.asarray([src]))
    assert np.array_equal(cost, tc.dijkstra(T, [src]))
    assert ((cost >= 0) == T).all()
    path = synth.travel_paths_ref(tc.centre(goal)[None], tc.ORIGIN, tc.RES, cost, T)[0]
    assert len(path) > 640 and np.array_equal(path[0], tc.centre(goal)) and np.array_equal(path[-1], tc.centre(src))


def test_truncation_keeps_exact_values():
    T = _random_T((12, 11, 5), 0.8, 9)
    seed = np.argwhere(T)[:1]
    full = synth.travel_ref(T, seed)
    for limit in (0, 63, 64, 200, 640, 10_000):
        cut = synth.travel_ref(T, seed, limit)
        assert np.array_equal(cut, np.where((full >= 0) & (full <= limit), full, -1)), limit
        assert np.array_equal(cut, tc.dijkstra(T, seed, limit))
    assert synth.travel_limit(None, 0.125) == (1 << 31) - 1 and synth.travel_limit(1.25, 0.125) == 640
    assert synth.travel_limit(1e12, 0.125) == (1 << 31) - 1 and synth.travel_limit(0.0, 0.1) == 0
    # float64(max_dist) / float64(f32 resolution): 0.1f is a little above 0.1, so 1 m is a little less than 10 voxels
    assert synth.travel_limit(1.0, 0.1) == 639


def test_positions_paths_and_metres_restatements():
    T = np.ones((4, 3, 2), dtype=bool)
    T[2, :, :] = False
    T[2, 1, 0] = True
    cost = synth.travel_ref(T, [(0, 0, 0)])
    pos = np.concatenate([tc.centre([[0, 0, 0], [3, 2, 1], [2, 0, 0], [4, 0, 0], [-3, 0, 0]]), np.array([[np.nan, 0, 0], [1e9, 0, 0]], dtype=np.float32)])
    codes = synth.travel_positions_ref(pos, tc.ORIGIN, tc.RES, cost)
    assert codes.tolist() == [0, int(cost[3, 2, 1]), -1, -2, -2, -2, -2] and cost[3, 2, 1] > 0
    met = synth.travel_metres(codes, tc.RES)
    assert met[0] == 0 and met[1] == np.float32(np.float32(cost[3, 2, 1]) * np.float32(1 / 64)) * np.float32(tc.RES)
    assert np.isinf(met[2]) and np.isnan(met[3:]).all()
    paths = synth.travel_paths_ref(pos, tc.ORIGIN, tc.RES, cost, T)
    assert [len(p) for p in paths] == [1, len(paths[1]), 0, 0, 0, 0, 0]
    hops = np.abs(np.diff(((paths[1] - np.float32(tc.ORIGIN)) / np.float32(tc.RES)), axis=0)).max(axis=1)
    assert np.allclose(hops, 1.0) and np.array_equal(paths[1][-1], tc.centre((0, 0, 0)))
    # ties go to the lowest move number, on an open 3 x 3 x 1 square from the source (0,1,0):
    T = np.ones((3, 3, 1), dtype=bool)
    cost = synth.travel_ref(T, [(0, 1, 0)])
    p = synth.travel_paths_ref(tc.centre((2, 0, 0))[None], tc.ORIGIN, tc.RES, cost, T)[0]
    # cost 155 = 64 + 91 two ways: via (1,0,0) [move (-1,0,0), m = 12] or via (1,1,0) [move (-1,+1,0), m = 15]: the lower wins
    assert cost[2, 0, 0] == 155 and np.array_equal(p[1], tc.centre((1, 0, 0)))


def test_the_picks_restatement_covers_ties_and_unreachable_candidates():
    gains = np.array([10, 12, 12, 50, 3, 12])
    cost = np.array([64, 640, 640, -1, 0, -2])
    taken = np.zeros(6, dtype=np.int64)
    assert synth.view_pick_travel_ref(gains, taken, cost, 0) == 1                 # the unreachable 50 and the -2 never win; ties: lowest
    assert synth.view_pick_travel_ref(gains, taken, cost, 0, min_gain=13) == -1   # the stop rule is the gain's
    m = synth.travel_weight_fixed(8.0, 0.125)                                     # 8 voxels per metre: one voxel edge costs one voxel
    assert m == 1 << 14 and synth.view_pick_travel_ref(gains, taken, cost, m) == 0   # 10 - 1 beats 12 - 10
    taken[0] = 1
    assert synth.view_pick_travel_ref(gains, taken, cost, m) == 4                 # 3 - 0 beats 12 - 10
    assert synth.view_pick_travel_ref(gains, np.ones(6, dtype=np.int64), cost, m) == -1
    # equal scores: gain 11 at cost 0 and gain 12 at one voxel edge
    assert synth.view_pick_travel_ref([12, 11], [0, 0], [64, 0], m) == 0 and synth.view_pick_travel_ref([11, 12], [0, 0], [0, 64], m) == 0


def test_abi_entries():
    header, before = abi_cases.check_abi_entries(ENTRIES)
    assert "travel_kernels.hip" in header and "new symbols only" in before


def test_check_travel_errors_by_name():
    torch = pytest.importorskip("torch")
    from trajectory_optimization_amd import ops

    class Grid(ops.OccupancyGrid):
        def __init__(self, dims=(8, 8, 8), r=0.125):   # a grid's geometry without a device
            self.origin, self.resolution, self.dims, _ = ops.check_los((0.0, 0.0, 0.0), r, dims)
            self.device = torch.device("cuda", 0)

    class Field(ops.ClearanceField):
        def __init__(self, grid, D):
            self.occupied, self.free, self.D = grid, None, D
            self.origin, self.resolution, self.dims, self.device = grid.origin, grid.resolution, grid.dims, grid.device

    field = Field(Grid(), 3)
    src = torch.zeros(2, 3)
    assert ops.check_travel(field, 0.1, src) == (1, (1 << 31) - 1, 2)
    assert ops.check_travel(field, 0.1, torch.zeros(3), max_dist=1.25, rounds_per_check=1) == (1, 640, 1)
    assert ops.check_travel(field, 0.1, torch.full((1, 3), float("nan")))[2] == 1   # (a source that is not finite is ignored, not refused)
    bad = [
        (dict(field=object()), "field must be an ops.ClearanceField"),
        (dict(radius=0.0), "radius"),
        (dict(radius=float("nan")), "radius"),
        (dict(radius=1.0), "largest radius it can certify"),
        (dict(sources=[[0.0, 0.0, 0.0]]), "sources must be a floating-point tensor"),
        (dict(sources=torch.zeros(2, 3, dtype=torch.int64)), "sources must be a floating-point tensor"),
        (dict(sources=torch.zeros(0, 3)), "sources must have shape (S,3)"),
        (dict(sources=torch.zeros(2, 4)), "sources must have shape (S,3)"),
        (dict(space=object()), "space must be an ops.SpaceMap"),
        (dict(max_dist=-1.0), "max_dist must be None or a finite number"),
        (dict(max_dist=float("inf")), "max_dist must be None or a finite number"),
        (dict(max_dist="far"), "max_dist must be None or a finite number"),
        (dict(rounds_per_check=0), "rounds_per_check must be an integer"),
        (dict(rounds_per_check=1.5), "rounds_per_check must be an integer"),
        (dict(rounds_per_check=1 << 17), "rounds_per_check must be an integer"),
    ]
    for kw, text in bad:
        args = dict(field=field, radius=0.1, sources=src)
        args.update(kw)
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
            ops.check_travel(**args)
    other = ops.SpaceMap.__new__(ops.SpaceMap)
    other.occupied = other.free = Grid((8, 8, 9))
    with pytest.raises(ValueError, match="space: its dims differs"):
        ops.check_travel(field, 0.1, src, space=other)


def test_entries_refuse_bad_arguments_without_gpu():
    """Every argument check returns before anything is enqueued: bad calls come back with their code on a machine without a GPU."""
    import ctypes
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    EINVAL, ENOSPC = -1, -2
    p, q, r, t, u, v = (ctypes.c_void_p(a) for a in (64, 4096, 8192, 16384, 32768, 65536))   # pointers no call may reach
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))   # noqa: E731
    ok = geom()
    nb, fb, cb, wb = (fn(64, 64, 32) for fn in (L.tohip_occ_bytes, L.tohip_field_bytes, L.tohip_travel_bytes, L.tohip_travel_workspace_bytes))
    assert cb == 4 * 64 * 64 * 32 and L.tohip_travel_bytes(5, 6, 3) == 360 and L.tohip_travel_bytes(2047, 2045, 511) == 4 * 2047 * 2045 * 511
    assert wb == 256 + 2 * 256 + 4 * 256 and wb % 256 == 0            # 8 x 8 x 4 tiles: a header, two bitmaps, the list
    for bad in ((0, 4, 4), (4, 4, 2049), (2048, 2048, 2048)):
        assert L.tohip_travel_bytes(*bad) == 0 and L.tohip_travel_workspace_bytes(*bad) == 0, bad
    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 64, 32)), geom(d=(64, 2049, 32))]
    rounds = ctypes.c_int64(-7)
    calls = {
        "build": (L.tohip_travel_build, ("field", "fbytes", "occ", "free", "grid_bytes", "geom", "need2", "src", "S", "limit", "rpc", "cost", "bytes",
                                         "ws", "ws_bytes", "seeded", "rounds", "stream"),
                  (p, fb, None, None, nb, ok, 1, q, 2, 640, 16, r, cb, t, wb, None, ctypes.byref(rounds), None)),
        "positions": (L.tohip_travel_positions, ("cost", "bytes", "geom", "pos", "m", "out", "dist", "stream"), (r, cb, ok, q, 10, t, None, None)),
        "paths": (L.tohip_travel_paths, ("cost", "bytes", "field", "fbytes", "occ", "free", "grid_bytes", "geom", "need2", "goals", "G", "max_rows",
                                         "rows", "counts", "stream"), (r, cb, p, fb, None, None, nb, ok, 1, q, 4, 100, t, u, None)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name in calls:
        assert call(name, cost=None) == EINVAL, name
        assert call(name, geom=None) == EINVAL, name
        assert call(name, bytes=cb - 1) == ENOSPC, name
        for g in bad_geoms:
            assert call(name, geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    for name in ("build", "paths"):
        for kw in (dict(field=None), dict(need2=0), dict(need2=65536), dict(occ=u), dict(free=u), dict(occ=u, free=u)):
            assert call(name, **kw) == EINVAL, (name, kw)
        assert call(name, fbytes=fb - 1) == ENOSPC and call(name, occ=u, free=v, grid_bytes=nb - 1) == ENOSPC, name
    for kw in (dict(src=None), dict(S=0), dict(S=-1), dict(limit=-1), dict(limit=1 << 31), dict(rpc=0), dict(rpc=65537), dict(ws=None), dict(ws=r),
               dict(cost=p), dict(ws=p), dict(occ=r, free=u), dict(occ=u, free=t)):
        assert call("build", **kw) == EINVAL, kw
    assert call("build", ws_bytes=wb - 1) == ENOSPC and rounds.value == -7
    for kw in (dict(pos=None), dict(m=-1), dict(out=None, dist=None)):
        assert call("positions", **kw) == EINVAL, kw
    assert call("positions", m=0) == 0
    for kw in (dict(goals=None), dict(rows=None), dict(counts=None), dict(G=-1), dict(max_rows=0)):
        assert call("paths", **kw) == EINVAL, kw
    assert call("paths", G=0) == 0
    pick = lambda **kw: L.tohip_view_volume_pick_travel(*[kw.get(k, b) for k, b in zip(   # noqa: E731
        ("gains", "cost", "weight", "taken", "M", "min_gain", "round", "order", "picked", "stop", "stream"), (p, q, 5, r, 10, 1, 0, t, u, v, None))])
    for kw in (dict(gains=None), dict(cost=None), dict(taken=None), dict(order=None), dict(picked=None), dict(stop=None), dict(M=0), dict(M=1 << 31),
               dict(min_gain=0), dict(round=-1), dict(weight=-1), dict(weight=1 << 31)):
        assert pick(**kw) == EINVAL, kw
