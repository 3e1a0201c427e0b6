"""The weighted travel field without a GPU: synth.travel_weighted_ref against a heapq Dijkstra written independently of it, its
degeneration to synth.travel_ref at kappa = 16, the path rule, truncation, the weight gather, the host layer's refusals by name and
the C entries' refusals before any launch."""
import ctypes

import numpy as np
import pytest

import abi_cases
import travel_cases as tc
import travel_weighted_cases as wc
from trajectory_optimization_amd import synth

ENTRIES = ("tohip_travel_weights_bytes", "tohip_travel_weights_build", "tohip_travel_build_weighted", "tohip_travel_paths_weighted")
ORIGIN, RES = wc.ORIGIN, wc.RES


def _seeds(T, n=3):
    src = wc.sources_of(T, n)
    seeded, vox = synth.travel_seeds_ref(src, ORIGIN, RES, T)
    assert seeded[-3:].tolist() == [0, 0, 0] and seeded[:n].all()
    return vox[seeded == 1]


@pytest.fixture(scope="module")
def refs():
    """{(dims, fill): (T, kappa, seeds, travel_weighted_ref)}: computed once, never modified."""
    out = {}
    for dims in wc.GRIDS:
        T = wc.traversable_of(dims)
        seeds = _seeds(T)
        for fill in wc.FILLS:
            kappa = wc.kappa_of(dims, fill)
            out[dims, fill] = (T, kappa, seeds, synth.travel_weighted_ref(T, seeds, kappa))
    return out


def test_travel_step():
    for w in synth.TRAVEL_WEIGHTS:
        assert synth.travel_step(w, 16, 16) == w
        for ka, kb in ((16, 255), (255, 255), (17, 16), (100, 31)):
            s = synth.travel_step(w, ka, kb)
            assert s == synth.travel_step(w, kb, ka) == wc.step(w, ka, kb) == (w * (ka + kb) + 16) // 32 and s >= w
    assert synth.travel_step(111, 255, 255) == synth.TRAVEL_MAX_STEP == 1769
    assert 0xFFFFF000 + 1769 < 1 << 32 and 0xFFFFF000 > synth.TRAVEL_MAX_LIMIT   # the kernels' "no path" value in LDS
    k = np.arange(16, 256, dtype=np.int64)
    assert np.array_equal(synth.travel_step(91, k[:, None], k[None, :]), (91 * (k[:, None] + k[None, :]) + 16) >> 5)


@pytest.mark.parametrize("fill", wc.FILLS)
@pytest.mark.parametrize("dims", wc.GRIDS, ids=str)
def test_the_restatement_equals_dijkstra(refs, dims, fill):
    T, kappa, seeds, ref = refs[dims, fill]
    assert np.array_equal(ref, wc.dijkstra(T, seeds, kappa))
    assert (ref >= 0).sum() > 0.8 * T.sum()
    if fill != "neutral":
        assert (ref > synth.travel_ref(T, seeds)).any()


@pytest.mark.parametrize("dims", wc.GRIDS, ids=str)
def test_at_neutral_weights_it_is_the_travel_field(refs, dims):
    T, kappa, seeds, ref = refs[dims, "neutral"]
    assert np.array_equal(ref, synth.travel_ref(T, seeds))
    assert np.array_equal(synth.travel_weighted_ref(T, seeds, kappa, 640), synth.travel_ref(T, seeds, 640))
    goals = tc.centre(np.argwhere(ref > 0)[::97])
    a = synth.travel_weighted_paths_ref(goals, ORIGIN, RES, ref, T, kappa)
    b = synth.travel_paths_ref(goals, ORIGIN, RES, ref, T)
    assert len(a) == len(b) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fill", wc.FILLS)
@pytest.mark.parametrize("dims", wc.GRIDS, ids=str)
def test_paths_sum_to_the_cost_step_by_step(refs, dims, fill):
    T, kappa, seeds, ref = refs[dims, fill]
    reach = np.argwhere(ref >= 0)
    goals = reach[:: max(1, len(reach) // 40)]
    paths = synth.travel_weighted_paths_ref(tc.centre(goals), ORIGIN, RES, ref, T, kappa)
    for goal, rows in zip(goals, paths):
        vox = wc.voxels_of(rows)
        assert vox[0] == tuple(goal) and ref[vox[-1]] == 0
        total = 0
        for v, u in zip(vox[:-1], vox[1:]):
            axes = sum(1 for a in range(3) if v[a] != u[a])
            assert 1 <= axes and max(abs(v[a] - u[a]) for a in range(3)) == 1
            s = synth.travel_step(synth.TRAVEL_WEIGHTS[axes - 1], int(kappa[v]), int(kappa[u]))
            assert s >= synth.TRAVEL_WEIGHTS[axes - 1] and ref[v] - ref[u] == s
            total += s
        assert total == ref[tuple(goal)] >= 64 * (len(vox) - 1)      # so cost // 64 + 1 bounds the rows
    unreachable = synth.travel_weighted_paths_ref(tc.centre([np.asarray(dims) + 1]), ORIGIN, RES, ref, T, kappa)
    assert unreachable[0].shape == (0, 3)


@pytest.mark.parametrize("fill", wc.FILLS)
@pytest.mark.parametrize("dims", wc.GRIDS, ids=str)
def test_truncation_keeps_exact_values(refs, dims, fill):
    T, kappa, seeds, ref = refs[dims, fill]
    for limit in (640, 0, 63, 1000):
        cut = synth.travel_weighted_ref(T, seeds, kappa, limit)
        assert np.array_equal(cut, np.where((ref >= 0) & (ref <= limit), ref, -1)), limit
    assert np.array_equal(synth.travel_weighted_ref(T, seeds, kappa, 640), wc.dijkstra(T, seeds, kappa, 640))


def test_two_routes_by_hand():
    c = wc.two_routes()
    T, kappa = c["T"], c["kappa"]
    neutral = np.full(T.shape, 16, dtype=np.uint8)
    goal = tc.centre([c["goal"]])
    plain = synth.travel_weighted_ref(T, [c["source"]], neutral)
    weighted = synth.travel_weighted_ref(T, [c["source"]], kappa)
    assert plain[c["goal"]] == c["short_plain"] == 384 and weighted[c["goal"]] == c["long_weighted"] == 1260
    assert plain[c["far"]] * 2 == c["long_plain"] and weighted[c["near"]] + 542 + 542 + 64 == c["short_weighted"] == 2296
    assert c["short_plain"] < c["long_plain"] == c["long_weighted"] < c["short_weighted"]
    short = wc.voxels_of(synth.travel_weighted_paths_ref(goal, ORIGIN, RES, plain, T, neutral)[0])
    long_ = wc.voxels_of(synth.travel_weighted_paths_ref(goal, ORIGIN, RES, weighted, T, kappa)[0])
    assert c["near"] in short and c["far"] not in short and len(short) == 7
    assert c["far"] in long_ and c["near"] not in long_ and not any(kappa[v] > 16 for v in long_)
    assert np.array_equal(weighted, wc.dijkstra(T, [c["source"]], kappa))


def test_travel_weights_ref_by_hand():
    field = np.array([[[0, 1], [2, 4]], [[9, 65535], [3, 5]]])           # squared gaps, (2, 2, 2)
    lut = np.array([255, 200, 90, 40, 16], dtype=np.uint8)                # the last entry for everything beyond
    want = np.array([[[255, 200], [90, 16]], [[16, 16], [40, 16]]], dtype=np.uint8)
    got = synth.travel_weights_ref(field, lut)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    state = np.array([[[0, 0], [1, 2]], [[0, 1], [0, 0]]])                # 0 unknown, 1 free, 2 occupied
    want = np.array([[[255, 255], [90, 16]], [[116, 16], [140, 116]]], dtype=np.uint8)   # + 100 where unknown, saturating
    assert np.array_equal(synth.travel_weights_ref(field, lut, state, 100), want)
    assert np.array_equal(synth.travel_weights_ref(field, [16]), np.full((2, 2, 2), 16))


def test_travel_weights_lut():
    lut = synth.travel_weights_lut(0.1, 0.5, 0.125, 8, gain=4.0)
    assert lut.dtype == np.uint8 and lut.shape == (65,)
    g = np.sqrt(np.arange(65.0)) * float(np.float32(0.125))
    want = np.clip(np.rint(16 + 64 * np.maximum(0, (0.5 - g) / 0.4) ** 2), 16, 255)
    assert np.array_equal(lut, want.astype(np.uint8))
    assert (np.diff(lut.astype(int)) <= 0).all() and (lut[g >= 0.5] == 16).all() and lut[0] == 116 and lut[1] > 16
    assert synth.travel_weights_lut(0.1, 0.5, 0.125, 8, gain=100.0)[0] == 255      # clipped
    assert (synth.travel_weights_lut(0.1, 0.5, 0.125, 3, gain=0.0) == 16).all()


# ---------------------------------------------------------------------------------------------------------------- the host layer

def _fake_field(dims=(8, 8, 8), r=0.125, origin=(0.0, 0.0, 0.0)):
    torch = pytest.importorskip("torch")
    from trajectory_optimization_amd import ops

    class Grid(ops.OccupancyGrid):
        def __init__(self):   # a grid's geometry without a device
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, r, dims)
            self.device = torch.device("cuda", 0)

    class Field(ops.ClearanceField):
        def __init__(self, grid, D):
            self.occupied, self.free, self.D = grid, None, D
            self.origin, self.resolution, self.dims, self.device = grid.origin, grid.resolution, grid.dims, grid.device

    return Field(Grid(), 3)


def _fake_weights(field):
    from trajectory_optimization_amd import ops
    w = ops.TravelWeights.__new__(ops.TravelWeights)
    w.field, w.origin, w.resolution, w.dims, w.device = field, field.origin, field.resolution, field.dims, field.device
    return w


def test_the_host_layer_refuses_by_name():
    import torch
    from trajectory_optimization_amd import ops, tools
    field = _fake_field()
    good = torch.full((8, 8, 8), 16, dtype=torch.uint8)
    low = good.clone().to(torch.int64)
    low[3, 1, 2] = 15
    low[5, 5, 5] = 3
    high = good.clone().to(torch.int32)
    high[0, 7, 1] = 256
    for tensor, text in ((low, r"kappa\[3, 1, 2\] = 15 is outside \[16, 255\]"), (high, r"kappa\[0, 7, 1\] = 256 is outside \[16, 255\]"),
                         (good[:7], r"must have the field's dims \(8, 8, 8\), got \(7, 8, 8\)"), (good.float(), "must be an integer tensor"),
                         (good.bool(), "must be an integer tensor"), (good.numpy(), "must be an integer tensor"),
                         (good, "lives on device cpu, the field on cuda:0")):
        with pytest.raises(ValueError, match=text):
            ops.check_travel_dense(field, tensor)
        with pytest.raises(ValueError, match=text):
            ops.TravelWeights.from_dense(field, tensor)
    with pytest.raises(ValueError, match="field must be an ops.ClearanceField"):
        ops.TravelWeights.from_dense(object(), good)
    with pytest.raises(ValueError, match="field must be an ops.ClearanceField"):
        ops.TravelWeights(object())
    # weights= of the builders: the type, then the geometry, each difference by its name
    src = torch.zeros(3, 3)
    assert ops.check_travel(field, 0.1, src, weights=None) == ops.check_travel(field, 0.1, src, weights=_fake_weights(field))
    assert ops.check_travel_batch(field, 0.1, src, weights=_fake_weights(field))[3] == 3
    others = [(_fake_field(dims=(8, 8, 9)), "dims"), (_fake_field(r=0.25), "resolution"), (_fake_field(origin=(0.0, 1.0, 0.0)), "origin")]
    moved = _fake_field()
    moved.device = torch.device("cuda", 1)
    for other, what in others + [(moved, "device")]:
        for check in (ops.check_travel, ops.check_travel_batch):
            with pytest.raises(ValueError, match=f"weights: the layer's {what} differs from the field's"):
                check(field, 0.1, src, weights=_fake_weights(other))
    for bad in (good, 16, "neutral", field):
        with pytest.raises(ValueError, match="weights must be an ops.TravelWeights or None"):
            ops.check_travel(field, 0.1, src, weights=bad)
        with pytest.raises(ValueError, match="weights must be an ops.TravelWeights or None"):
            tools.travel_field(field, src, 0.1, weights=bad)
        with pytest.raises(ValueError, match="weights must be an ops.TravelWeights or None"):
            tools.travel_fields(field, src, 0.1, weights=bad)
        with pytest.raises(ValueError, match="weights must be an ops.TravelWeights or None"):
            tools.travel_matrix(field, src, 0.1, weights=bad)
    # the table and its settings
    for lut, text in (([16, 15, 16], r"lut\[1\] = 15 is outside \[16, 255\]"), ([16, 300], r"lut\[1\] = 300 is outside"),
                      ([], "1-D table"), (np.full((2, 2), 16), "1-D table"), ([16.0, 17.0], "1-D table"), (np.full(65537, 16), "1-D table")):
        with pytest.raises(ValueError, match=text):
            ops.check_travel_lut(lut)
        with pytest.raises(ValueError, match=text):
            tools.travel_weights(field, 0.1, 0.5, lut=lut)
    assert np.array_equal(ops.check_travel_lut(torch.tensor([16, 255])), np.array([16, 255], dtype=np.uint8))
    for kw, text in ((dict(soft_radius=0.1), "soft_radius must be a finite number of metres > radius"),
                     (dict(soft_radius=float("nan")), "soft_radius must be"), (dict(gain=-1.0), "gain must be a finite number >= 0"),
                     (dict(unknown_add=5), "unknown_add needs space="), (dict(unknown_add=256), r"unknown_add must be an integer in \[0, 255\]"),
                     (dict(unknown_add=1.5), "unknown_add must be an integer")):
        args = dict(radius=0.1, soft_radius=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            tools.travel_weights(field, **args)
    with pytest.raises(ValueError, match="field must be an ops.ClearanceField"):
        tools.travel_weights(object(), 0.1, 0.5)
    with pytest.raises(ValueError, match="weights= needs travel=True"):
        tools.plan_tour(field, torch.zeros(3, 3), clearance_radius=0.1, weights=_fake_weights(field))


# ---------------------------------------------------------------------------------------------------------------- the C entries

def test_abi_entries():
    header, before = abi_cases.check_abi_entries(ENTRIES)
    assert "new symbols only" in before.split("tohip_travel_paths_weighted")[1][:200] and "Weighted travel fields" in header


def test_entries_refuse_bad_arguments_without_gpu():
    """Every argument check returns before anything is enqueued: bad calls come back with their code on a machine without a GPU."""
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    EINVAL, ENOSPC = -1, -2
    nx, ny, nz = 64, 64, 32
    ok = _lib.OccGeom((ctypes.c_float * 3)(0.0, 0.0, 0.0), 0.1, (ctypes.c_int32 * 3)(nx, ny, nz))
    nb, fb = L.tohip_occ_bytes(nx, ny, nz), L.tohip_field_bytes(nx, ny, nz)
    kb = L.tohip_travel_weights_bytes(nx, ny, nz)
    assert kb == nx * ny * nz and L.tohip_travel_weights_bytes(2047, 2045, 511) == 2047 * 2045 * 511
    for bad in ((0, 4, 4), (4, 4, 2049), (4, -1, 4)):
        assert L.tohip_travel_weights_bytes(*bad) == 0, bad
    B = 3
    cb, wb = L.tohip_travel_batch_bytes(nx, ny, nz, B), L.tohip_travel_batch_workspace_bytes(nx, ny, nz, B)
    # pointers no call may reach, far enough apart that only the named overlaps overlap
    M = 1 << 24
    field, src, src_field, cost, ws, layer, occ, fre, lut, out = (ctypes.c_void_p(M * (i + 1)) for i in range(10))
    rounds = ctypes.c_int64(-7)
    names = ("field", "fbytes", "occ", "free", "grid_bytes", "geom", "need2", "src", "src_field", "S", "B", "limit", "rpc", "cost", "bytes", "ws",
             "ws_bytes", "seeded", "rounds", "weights", "wbytes", "stream", "flags")
    base = (field, fb, None, None, nb, ok, 1, src, src_field, 2, B, 640, 16, cost, cb, ws, wb, None, ctypes.byref(rounds), layer, kb, None, 0)

    def build(**kw):
        assert set(kw) <= set(names), kw
        return L.tohip_travel_build_weighted(*[kw.get(k, b) for k, b in zip(names, base)])

    inside = lambda p, off: ctypes.c_void_p(p.value + off)   # noqa: E731
    for kw in (dict(weights=None), dict(wbytes=kb - 1), dict(wbytes=0),
               dict(weights=cost), dict(weights=inside(cost, cb - 1)), dict(weights=inside(cost, 1 - kb)),         # a byte of cost
               dict(weights=ws), dict(weights=inside(ws, wb - 1)), dict(weights=inside(ws, 1 - kb)),                 # a byte of workspace
               dict(flags=1), dict(B=0), dict(B=257), dict(bytes=cb - 1), dict(ws_bytes=wb - 1), dict(src_field=None), dict(src=None),
               dict(S=0), dict(cost=None), dict(ws=None), dict(geom=None), dict(limit=-1), dict(limit=1 << 31), dict(rpc=0), dict(need2=0),
               dict(cost=field), dict(occ=occ)):
        assert build(**kw) == EINVAL, kw
    assert build(fbytes=fb - 1) == ENOSPC and rounds.value == -7
    # the paths
    names = ("cost", "bytes", "field", "fbytes", "occ", "free", "grid_bytes", "geom", "need2", "B", "goals", "goal_field", "G", "max_rows", "rows",
             "counts", "weights", "wbytes", "stream", "flags")
    base = (cost, cb, field, fb, None, None, nb, ok, 1, B, src, src_field, 4, 100, ws, out, layer, kb, None, 0)
    paths = lambda **kw: L.tohip_travel_paths_weighted(*[kw.get(k, b) for k, b in zip(names, base)])   # noqa: E731
    for kw in (dict(weights=None), dict(wbytes=kb - 1), dict(flags=2), dict(B=0), dict(B=257), dict(cost=None), dict(goal_field=None),
               dict(goals=None), dict(rows=None), dict(counts=None), dict(max_rows=0), dict(G=-1), dict(geom=None)):
        assert paths(**kw) == EINVAL, kw
    assert paths(bytes=cb - 1) == ENOSPC and paths(fbytes=fb - 1) == ENOSPC and paths(G=0) == 0
    # the gather
    names = ("field", "fbytes", "occ", "free", "grid_bytes", "geom", "lut", "n_lut", "add", "out", "out_bytes", "stream", "flags")
    base = (field, fb, None, None, nb, ok, lut, 10, 0, out, kb, None, 0)
    gather = lambda **kw: L.tohip_travel_weights_build(*[kw.get(k, b) for k, b in zip(names, base)])   # noqa: E731
    for kw in (dict(lut=None), dict(n_lut=0), dict(n_lut=-1), dict(n_lut=65537), dict(add=-1), dict(add=256), dict(out=None), dict(flags=1),
               dict(geom=None), dict(field=None), dict(occ=occ), dict(free=fre), dict(occ=occ, free=occ), dict(out=field),
               dict(out=inside(field, 2 * kb - 1)), dict(out=lut), dict(occ=occ, free=fre, out=inside(fre, nb - 1))):
        assert gather(**kw) == EINVAL, kw
    assert gather(out_bytes=kb - 1) == ENOSPC and gather(fbytes=fb - 1) == ENOSPC
