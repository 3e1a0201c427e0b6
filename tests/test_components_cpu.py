"""Connected components without a GPU: the numpy restatements (synth.components_*) against scipy.ndimage.label, np.bincount and plain
Python loops, the hand cases with their stated component counts, ops.check_components' errors by name, the ABI entries and their
argument checks, and the order of frontier_clusters' rows."""
import numpy as np
import pytest

import components_cases as cc
from trajectory_optimization_amd import synth


def _lin(shape):
    nx, ny, nz = shape
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return (z * ny + y) * nx + x


# ------------------------------------------------------------------------------------------------------------ 1. against scipy

@pytest.mark.parametrize("c", cc.CONNECTIVITIES)
@pytest.mark.parametrize("fill", sorted(cc.FILLS))
@pytest.mark.parametrize("dims", cc.GRIDS, ids=str)
def test_components_ref_equals_scipy_label(dims, fill, c):
    ndi = pytest.importorskip("scipy.ndimage")
    plane = cc.plane_of(dims, fill)
    lab, n = ndi.label(plane, structure=ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[c]))
    want_ids, want_roots = cc.canonical(lab - 1, plane)
    ids, roots = synth.components_ref(plane, c)
    assert ids.dtype == np.int64 and roots.dtype == np.int64 and len(roots) == n
    assert np.array_equal(ids, want_ids) and np.array_equal(roots, want_roots)
    assert np.isin(roots, _lin(dims)[plane]).all() and (np.diff(roots) > 0).all()        # every root is a set voxel, ascending
    if fill == "full":
        assert n == 1 and roots.tolist() == [0]
    if fill == "empty":
        assert n == 0 and (ids == -1).all()


def test_the_counts_the_gpu_matrix_relies_on():
    """At 30 % and 2 % fill of (64,64,32) the three connectivities give three different counts: none can pass for another."""
    counts = {fill: [len(synth.components_ref(cc.plane_of((64, 64, 32), fill), c)[1]) for c in cc.CONNECTIVITIES] for fill in ("30%", "2%")}
    for fill, (n6, n18, n26) in counts.items():
        assert n6 > n18 > n26 >= 1, (fill, n6, n18, n26)
    assert counts["30%"][0] > 50 * counts["30%"][1]


# ------------------------------------------------------------------------------------------------------------ 2. hand cases

@pytest.mark.parametrize("name", sorted(cc.hand_cases()))
def test_hand_cases_through_the_restatement(name):
    plane, counts = cc.hand_cases()[name]
    for c in cc.CONNECTIVITIES:
        ids, roots = synth.components_ref(plane, c)
        assert len(roots) == counts[c], (name, c, len(roots))
        assert (ids >= 0).sum() == plane.sum() and ((ids >= 0) == plane).all()
    if name == "full_plane":
        s = synth.components_stats_ref(ids, cc.ORIGIN, cc.RES)
        assert s["sizes"].tolist() == [plane.size] and s["bbox"].tolist() == [[[0, 0, 0], [d - 1 for d in plane.shape]]]


def test_checkerboard_and_serpentines_through_the_restatement():
    board = cc.checkerboard()
    ids, roots = synth.components_ref(board, 6)
    assert len(roots) == 65536 and np.array_equal(roots, np.sort(_lin(board.shape)[board]))
    assert np.array_equal(ids[board], np.searchsorted(roots, _lin(board.shape)[board]))   # the ids are the ranks of the indices
    assert len(synth.components_ref(board, 18)[1]) == 1 and len(synth.components_ref(board, 26)[1]) == 1
    for name, plane in cc.serpentines().items():
        for c in cc.CONNECTIVITIES:
            ids, roots = synth.components_ref(plane, c)
            assert len(roots) == 1 and roots[0] == _lin(plane.shape)[plane].min(), (name, c)
    fwd, rev = cc.serpentines()["forward"], cc.serpentines()["reversed"]
    assert fwd[0, 1, 0] and not fwd[1, 0, 0] and rev[65, 39, 0]   # the lowest index lies at opposite ends of the lane


# ------------------------------------------------------------------------------------------------------------ 3. stats and minima

def test_stats_ref_against_bincount():
    plane = cc.plane_of((37, 5, 20), "30%")
    ids, roots = synth.components_ref(plane, 6)
    s = synth.components_stats_ref(ids, cc.ORIGIN, cc.RES)
    C = len(roots)
    of, ijk = ids[plane], np.argwhere(plane)
    assert np.array_equal(s["sizes"], np.bincount(of, minlength=C))
    for a in range(3):
        assert np.array_equal(s["sums"][:, a], np.bincount(of, weights=ijk[:, a], minlength=C).astype(np.int64))
    for i in (0, C // 2, C - 1):
        rows = ijk[of == i]
        assert s["bbox"][i].tolist() == [rows.min(axis=0).tolist(), rows.max(axis=0).tolist()]
        want = np.asarray(cc.ORIGIN, dtype=np.float32).astype(np.float64) + (rows.mean(axis=0) + 0.5) * float(np.float32(cc.RES))
        assert s["centroids"].dtype == np.float32 and np.allclose(s["centroids"][i], want, rtol=0, atol=1e-6)
    assert s["sizes"].sum() == plane.sum()


def test_min_ref_against_a_loop():
    rng = np.random.default_rng(5)
    plane = cc.plane_of((37, 5, 20), "30%")
    ids, roots = synth.components_ref(plane, 18)
    values = rng.integers(0, 50, size=plane.shape).astype(np.int64)          # few distinct values: ties inside every large component
    values[rng.random(plane.shape) < 0.3] = 0xFFFFFFFF
    values[np.isin(ids, [0, 3, len(roots) - 1])] = 0xFFFFFFFF                # whole components without a value
    value, voxel = synth.components_min_ref(ids, values)
    lin = _lin(plane.shape)
    ties = 0
    for i in range(len(roots)):
        best, at = -1, -1
        for v, val in sorted(zip(lin[ids == i].tolist(), values[ids == i].tolist())):
            if val != 0xFFFFFFFF and (best < 0 or val < best):
                best, at = val, v
        ties += int(((values[ids == i] == best).sum() > 1))
        assert (int(value[i]), int(voxel[i])) == (best, at), i
    assert value[0] == -1 and voxel[3] == -1 and ties > 0


# ------------------------------------------------------------------------------------------------------------ 4. argument checks

def test_check_components_errors_by_name():
    torch = pytest.importorskip("torch")
    from trajectory_optimization_amd import ops

    class Grid(ops.OccupancyGrid):
        def __init__(self, dims=(8, 8, 8), r=0.125):   # a grid's geometry without a device
            self.origin, self.resolution, self.dims, _ = ops.check_los((0.0, 0.0, 0.0), r, dims)
            self.device = torch.device("cpu")

    class Travel(ops.TravelField):
        def __init__(self, grid):
            self.origin, self.resolution, self.dims, self.device = grid.origin, grid.resolution, grid.dims, grid.device

    grid = Grid()
    assert ops.check_components(grid) == (26, 16)
    assert ops.check_components(grid, 6, 1000, values=torch.zeros(512, dtype=torch.int32)) == (6, 1000)
    assert ops.check_components(grid, 18, 1, values=Travel(grid)) == (18, 1)
    bad = [
        (dict(grid=object()), "grid must be an ops.OccupancyGrid"),
        (dict(connectivity=8), "connectivity must be 6, 18 or 26"),
        (dict(connectivity=6.0), "connectivity must be 6, 18 or 26"),
        (dict(connectivity=None), "connectivity must be 6, 18 or 26"),
        (dict(rounds_per_check=0), "rounds_per_check must be an integer in [1, 1000]"),
        (dict(rounds_per_check=1001), "rounds_per_check must be an integer in [1, 1000]"),
        (dict(rounds_per_check=2.5), "rounds_per_check must be an integer in [1, 1000]"),
        (dict(values=torch.zeros(511, dtype=torch.int32)), "values must be an ops.TravelField or a contiguous int32 / uint8 tensor of 2048 bytes"),
        (dict(values=torch.zeros(512, dtype=torch.float32)), "values must be an ops.TravelField or a contiguous"),
        (dict(values=[1, 2]), "values must be an ops.TravelField or a contiguous"),
        (dict(values=Travel(Grid((8, 8, 9)))), "values: the travel field's dims differs"),
        (dict(values=Travel(Grid(r=0.25))), "values: the travel field's resolution differs"),
    ]
    for kw, text in bad:
        args = dict(grid=grid)
        args.update(kw)
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")):
            ops.check_components(**args)


# ------------------------------------------------------------------------------------------------------------ 5. the ABI

ENTRIES = ("tohip_components_bytes", "tohip_components_workspace_bytes", "tohip_components_build", "tohip_components_stats",
           "tohip_components_min", "tohip_components_positions")


def test_the_six_entries_are_bound_from_the_header():
    import ctypes
    from trajectory_optimization_amd import _lib
    assert _lib.ABI_VERSION == 15
    for name in ENTRIES:
        assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["tohip_components_build"]
    assert res is ctypes.c_int and len(args) == 14
    assert args[11] == ctypes.POINTER(ctypes.c_int64) and args[12] == ctypes.POINTER(ctypes.c_int64)   # n_components_host, rounds_host
    assert _lib.SIGNATURES["tohip_components_bytes"][0] is ctypes.c_size_t


def test_entries_refuse_bad_arguments_without_gpu():
    """Every argument check returns before anything is enqueued: bad calls come back with their code on a machine without a GPU."""
    import ctypes
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    EINVAL, ENOSPC = -1, -2
    p, q, r, t, u, v = (ctypes.c_void_p(a) for a in (4096, 8192, 16384, 32768, 65536, 131072))   # pointers no call may reach
    odd = ctypes.c_void_p(4098)
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))   # noqa: E731
    ok = geom()
    nb, lb, wb = (fn(64, 64, 32) for fn in (L.tohip_occ_bytes, L.tohip_components_bytes, L.tohip_components_workspace_bytes))
    assert lb == 4 * 64 * 64 * 32 and L.tohip_components_bytes(5, 6, 3) == 360 and L.tohip_components_bytes(2047, 2045, 511) == 4 * 2047 * 2045 * 511
    # the travel field's worklist (a header, two bitmaps, the list of 8 x 8 x 4 tiles), then 32 + 1 block counts padded to 256 bytes
    assert wb == L.tohip_travel_workspace_bytes(64, 64, 32) + 512 and wb % 256 == 0
    for bad in ((0, 4, 4), (4, 4, 2049), (2048, 2048, 2048)):
        assert L.tohip_components_bytes(*bad) == 0 and L.tohip_components_workspace_bytes(*bad) == 0, bad
    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 64, 32)), geom(d=(64, 2049, 32))]
    n, rounds = ctypes.c_int64(-7), ctypes.c_int64(-7)
    calls = {
        "build": (L.tohip_components_build, ("plane", "grid_bytes", "geom", "c", "labels", "bytes", "ws", "ws_bytes", "rpc", "roots", "capacity",
                                             "n", "rounds", "stream"),
                  (p, nb, ok, 26, q, lb, r, wb, 16, t, 100, ctypes.byref(n), ctypes.byref(rounds), None)),
        "stats": (L.tohip_components_stats, ("labels", "bytes", "geom", "C", "sizes", "sums", "bbox", "stream"), (q, lb, ok, 10, t, u, v, None)),
        "min": (L.tohip_components_min, ("labels", "bytes", "geom", "values", "vbytes", "C", "value", "voxel", "stream"),
                (q, lb, ok, r, lb, 10, t, u, None)),
        "positions": (L.tohip_components_positions, ("labels", "bytes", "geom", "pos", "m", "out", "stream"), (q, lb, ok, r, 10, t, None)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name in calls:
        assert call(name, labels=None) == EINVAL, name
        assert call(name, labels=odd) == EINVAL, name          # misaligned
        assert call(name, geom=None) == EINVAL, name
        assert call(name, bytes=lb - 1) == ENOSPC, name
        for g in bad_geoms:
            assert call(name, geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    for kw in (dict(plane=None), dict(c=0), dict(c=8), dict(c=27), dict(rpc=0), dict(rpc=1001), dict(ws=None), dict(ws=odd), dict(ws=q),
               dict(labels=p), dict(ws=p), dict(roots=None), dict(roots=odd), dict(roots=q), dict(capacity=-1), dict(n=None)):
        assert call("build", **kw) == EINVAL, kw
    assert call("build", ws_bytes=wb - 1) == ENOSPC and call("build", grid_bytes=nb - 1) == ENOSPC
    assert n.value == -7 and rounds.value == -7
    for name in ("stats", "min"):
        assert call(name, C=-1) == EINVAL and call(name, C=(1 << 31) + 1) == EINVAL and call(name, C=0) == 0, name
    for kw in (dict(sizes=None), dict(sums=None), dict(bbox=None), dict(sizes=odd), dict(sums=odd)):
        assert call("stats", **kw) == EINVAL, kw
    for kw in (dict(values=None), dict(values=q), dict(values=odd), dict(value=None), dict(voxel=None), dict(value=odd)):
        assert call("min", **kw) == EINVAL, kw
    assert call("min", vbytes=lb - 1) == ENOSPC
    for kw in (dict(pos=None), dict(m=-1), dict(out=None)):
        assert call("positions", **kw) == EINVAL, kw
    assert call("positions", m=0) == 0


# ------------------------------------------------------------------------------------------------------------ 6. the clusters' order

def test_frontier_clusters_ref_order_with_ties():
    sizes = [5, 1, 9, 9, 2, 5, 1]
    assert synth.frontier_clusters_ref(sizes).tolist() == [2, 3, 0, 5, 4, 1, 6]
    assert synth.frontier_clusters_ref(sizes, min_size=2).tolist() == [2, 3, 0, 5, 4]
    cost = [640, -1, 128, -1, 128, 640, 0]
    #        reachable by cost: 6 (0); 2, 4 (128: size 9 before 2); 0, 5 (640: equal sizes, the lower id); then the unreachable: 3 (9), 1
    assert synth.frontier_clusters_ref(sizes, cost).tolist() == [6, 2, 4, 0, 5, 3, 1]
    assert synth.frontier_clusters_ref(sizes, cost, min_size=2).tolist() == [2, 4, 0, 5, 3]
    assert synth.frontier_clusters_ref([], []).tolist() == [] and synth.frontier_clusters_ref([1, 1], [-1, -1], 2).tolist() == []
    # the same order by the two stable sorts the host layer runs on the device
    torch = pytest.importorskip("torch")
    s, c = torch.tensor(sizes), torch.tensor(cost)
    ids = torch.nonzero(s >= 1).reshape(-1)
    ids = ids[torch.sort(s[ids], stable=True, descending=True)[1]]
    key = torch.where(c < 0, torch.full_like(c, torch.iinfo(torch.int64).max), c)
    ids = ids[torch.sort(key[ids], stable=True)[1]]
    assert ids.tolist() == [6, 2, 4, 0, 5, 3, 1]
