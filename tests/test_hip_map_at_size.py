"""The map layer on the GPU beyond one grid-stride pass and at the largest grid (occupancy_kernels.hip, frontier_kernels.hip,
field_kernels.hip): N = 600 000 rows against the 524 288 lanes a launch gets, the field over 672 000 voxels with values up to
D^2 = 64 516, the listing over 265 blocks, the 2 139 104 765-voxel grid through a window in its far corner, and rays that span the
range on all three axes.  Every comparison is torch.equal against the numpy restatements of synth on the inputs of
tests/map_size_cases.py (checked without a GPU in tests/test_map_at_size_cpu.py); there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import map_size_cases as mc
from map_size_cases import DIMS, FIELD_DIMS, FIELD_ORIGIN, LIST_DIMS, N, ORIGIN, RES

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _grid_of(bits, dev, origin=ORIGIN):
    """An OccupancyGrid holding exactly the voxels of `bits` (their centres inserted)."""
    from trajectory_optimization_amd import ops
    g = ops.OccupancyGrid(origin, RES, bits.shape, device=dev)
    _, centres = synth.occ_export_ref(bits, origin, RES)
    if len(centres):
        assert g.insert(_t(centres, dev)) == 0
    return g


def _same(got, want):
    """torch.equal of a device tensor and a numpy array, dtype included."""
    want = torch.from_numpy(np.ascontiguousarray(want))
    return got.dtype == want.dtype and torch.equal(got.cpu(), want)


def _first_difference(got, want):
    """Where two flat arrays first differ, for the assertion message: the row tells the trip (row // 524 288) and the block."""
    bad = np.flatnonzero(got.cpu().numpy().ravel() != np.asarray(want).ravel())
    return f"{len(bad)} differ, the first at {bad[:5].tolist()} (trip {int(bad[0]) // mc.LANES})" if len(bad) else "equal"


# ------------------------------------------------------------------------------------------------------------ 1. past 524 288 lanes

def test_insert_and_lookup_past_one_pass(dev):
    from trajectory_optimization_amd import ops
    c = mc.insert_case()
    assert 0 < c["skipped"] < N and c["ref"].any() and not c["ref"].all()
    g = ops.OccupancyGrid(ORIGIN, RES, DIMS, device=dev)
    assert g.insert(_t(c["P"], dev)) == c["skipped"] == g.skipped
    assert _same(g.dense(), c["ref"])
    got = g.lookup(_t(c["ijk"], dev))
    assert _same(got, c["look"]), _first_difference(got, c["look"])
    assert c["look"][mc.LANES:].any() and not c["look"][mc.LANES:].all()


@pytest.mark.parametrize("skip", [(0, 0), (1, 1)])
def test_line_of_sight_past_one_pass(dev, skip):
    c = mc.los_case()
    want = c["want"][skip]
    assert (want == 0).sum() >= 0.05 * N and (want == 1).sum() >= 0.05 * N, np.bincount(want)
    assert np.array_equal(np.flatnonzero(want == 2), c["bad"]) and c["bad"].min() >= mc.LANES
    g = _grid_of(c["occ"], dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    got = g.line_of_sight(_t(c["A"], dev), _t(c["B"], dev), skip=skip, stats=stats)
    assert _same(got, want), _first_difference(got, want)
    assert int(stats[0]) == int((want != 2).sum()) == N - 4


@pytest.mark.parametrize("max_range", [None, 0.3])
def test_carve_past_one_pass(dev, max_range):
    from trajectory_optimization_amd import ops
    c = mc.carve_case(max_range)
    share = c["free"].mean()
    print(f"max_range {max_range}: flags {np.bincount(c['flags']).tolist()}, visits {c['visits']}, set share {share:.3f}")
    assert 0.1 <= share <= 0.9
    assert np.array_equal(np.flatnonzero(c["flags"] == 2), c["bad"]) and c["bad"].min() >= mc.LANES
    if max_range is not None:
        assert (c["flags"] == 0).sum() > 0.2 * N and (c["flags"] == 1).sum() > 0.2 * N
    free = ops.OccupancyGrid(ORIGIN, RES, LIST_DIMS, device=dev)
    stats = torch.zeros(3, dtype=torch.int64, device=dev)
    flags = torch.full((N,), 9, dtype=torch.uint8, device=dev)
    assert free.carve(_t(c["O"], dev), _t(c["P"], dev), max_range, stats=stats, flags=flags) == c["skipped"] == 4
    assert _same(flags, c["flags"]), _first_difference(flags, c["flags"])
    assert stats.tolist()[:2] == [N - c["skipped"], c["visits"]]
    assert _same(free.dense(), c["free"])
    assert free.count() == int(c["free"].sum())


def test_state_past_one_pass(dev):
    from trajectory_optimization_amd import ops
    m, c = mc.listing_case(), mc.state_case()
    want = c["want"]
    assert min(np.bincount(want, minlength=4)) > 1000 and want[c["rows"]].tolist() == [3, 3, 3, 3, int(want[c["rows"][4]]), 3]
    assert want[c["rows"][4]] != 3 and c["rows"].min() >= mc.LANES
    space = ops.SpaceMap(_grid_of(m["occ"], dev), _grid_of(m["free"], dev))
    got = space.state(_t(c["pos"], dev))
    assert _same(got, want), _first_difference(got, want)


@pytest.fixture(scope="module")
def corner_field(dev):
    """The field of one obstacle at [-1, 0, -1] of (300, 280, 8), D = 254: built once for the queries and the nodes."""
    from trajectory_optimization_amd import ops
    occ, _, D, _ = mc.field_fill("corner")
    return ops.ClearanceField(_grid_of(occ, dev, FIELD_ORIGIN), D=D)


def test_field_queries_past_one_pass(dev, corner_field):
    c, field = mc.field_query_case(), corner_field
    look, d2, vox = c["look"], c["d2"], c["vox"]
    # the reference holds every class in the second trip: large values, the sentinel, rows out of range
    tail = slice(mc.LANES, None)
    assert ((look[tail] > 8899) & (look[tail] < 65535)).any() and (look[tail] == 65535).any() and (look[tail] == -1).sum() == 4
    assert ((d2[tail] > 8899) & (d2[tail] < 65535)).any() and (d2[tail] == 65535).any() and np.array_equal(np.flatnonzero(d2 == -1), c["bad"])
    pos = _t(c["pos"], dev)
    got = field.lookup_positions(pos)
    assert _same(got, look), _first_difference(got, look)
    dist = field.distance(pos)
    assert dist.dtype == torch.float32 and _same(dist.view(torch.int32), synth.field_metres(look, RES).view(np.int32))
    a, b = _t(c["a"], dev), _t(c["b"], dev)
    got_d2, got_vox = field.segments(a, b)
    assert _same(got_d2, d2), _first_difference(got_d2, d2)
    assert _same(got_vox, vox), _first_difference(got_vox, vox)
    need2 = field.need2(mc.NODE_RADIUS)
    assert need2 == synth.field_need2(mc.NODE_RADIUS, RES) > 8899
    d_ref, idx_ref = synth.field_edges_ref(d2, vox, need2, RES)
    assert (idx_ref[tail] == -1).any() and (idx_ref[tail] >= 0).any()
    d, idx, s = field.edges(a, b, mc.NODE_RADIUS)
    assert _same(d.view(torch.int32), d_ref.view(np.int32)) and _same(idx, idx_ref), _first_difference(idx, idx_ref)
    assert s.shape == d.shape and not bool(s.any())


# ------------------------------------------------------------------------------------------------------------ 2. the field at size

def test_field_build_with_values_up_to_D2(dev, corner_field):
    ref = mc.field_case("corner")
    finite = ref[ref < 65535]
    assert len(finite) == 411_290 and finite.max() == 64_516 == 254 * 254
    assert int((finite > 8899).sum()) == 353_158 and int((ref == 65535).sum()) == 260_710
    got = corner_field.dense().cpu()
    assert got.dtype == torch.int32 and tuple(got.shape) == FIELD_DIMS
    assert torch.equal(got, torch.from_numpy(ref.astype(np.int32))), _first_difference(got.permute(2, 1, 0), ref.transpose(2, 1, 0))


@pytest.mark.parametrize("name", ["sparse", "strict"])
def test_field_build_over_random_fills(dev, name):
    from trajectory_optimization_amd import ops
    occ, free, D, unknown = mc.field_fill(name)
    ref = mc.field_case(name)
    assert 100 < occ.sum() < 1000 and ref.max() > 1
    grid = _grid_of(occ, dev, FIELD_ORIGIN)
    field = ops.ClearanceField(grid if free is None else ops.SpaceMap(grid, _grid_of(free, dev, FIELD_ORIGIN)), D=D, unknown=unknown)
    got = field.dense().cpu()
    assert torch.equal(got, torch.from_numpy(ref.astype(np.int32))), _first_difference(got.permute(2, 1, 0), ref.transpose(2, 1, 0))


@pytest.mark.parametrize("stride", [1, 3])
def test_free_nodes_depend_on_the_large_values(dev, corner_field, stride):
    from trajectory_optimization_amd import ops
    ref = mc.field_case("corner")
    need2 = synth.field_need2(mc.NODE_RADIUS, RES)
    want = synth.field_nodes_ref(ref, need2, stride)
    # (a plane that holds only the sentinel's voxels, or every voxel above 8 899, would be another one)
    assert need2 > 8899 and (want & (ref < 65535)).any() and (~want & (ref > 8899))[stride // 2::stride, stride // 2::stride, stride // 2::stride].any()
    nodes = corner_field.free_nodes(mc.NODE_RADIUS, stride)
    assert isinstance(nodes, ops.FreeNodes) and _same(nodes.grid.dense(), want)
    ijk, centres = synth.occ_export_ref(want, FIELD_ORIGIN, RES)
    assert nodes.n == len(ijk) > 1000 and _same(nodes.ijk, ijk) and _same(nodes.points, centres)


# ------------------------------------------------------------------------------------------------------------ 3. the listing at size

@pytest.fixture(scope="module")
def listed_map(dev):
    from trajectory_optimization_amd import ops
    m = mc.listing_case()
    return ops.SpaceMap(_grid_of(m["occ"], dev), _grid_of(m["free"], dev))


def _check_listing(grid, bits):
    ijk, centres = synth.occ_export_ref(bits, ORIGIN, RES)
    got_ijk, got_centres = grid.export()
    assert grid.count() == len(ijk) == int(bits.sum())
    assert _same(got_ijk, ijk), _first_difference(got_ijk, ijk)
    assert _same(got_centres, centres)


def test_listing_of_the_occupied_plane_over_265_blocks(dev, listed_map):
    from trajectory_optimization_amd import _lib
    assert _lib.lib().tohip_occ_export_workspace_bytes(*LIST_DIMS) == 8 * (265 + 1)
    occ = mc.listing_case()["occ"]
    assert _same(listed_map.occupied.dense(), occ)
    _check_listing(listed_map.occupied, occ)


@pytest.mark.parametrize("k", [1, 2, 6])
def test_frontier_and_its_listing_over_265_blocks(dev, listed_map, k):
    from trajectory_optimization_amd import ops
    want = mc.listing_case()["frontier"][k]
    print(f"frontier({k}): {int(want.sum())} voxels")
    assert want.sum() > (100_000 if k < 6 else 50)
    fr = listed_map.frontier(k)
    assert isinstance(fr, ops.Frontier) and _same(fr.grid.dense(), want)
    ijk, centres = synth.occ_export_ref(want, ORIGIN, RES)
    assert fr.n == len(ijk) and _same(fr.ijk, ijk) and _same(fr.points, centres)
    _check_listing(fr.grid, want)


def test_listing_of_an_empty_and_a_full_plane_over_265_blocks(dev):
    from trajectory_optimization_amd import ops
    empty = ops.OccupancyGrid(ORIGIN, RES, LIST_DIMS, device=dev)
    ijk, centres = empty.export()
    assert empty.count() == 0 and tuple(ijk.shape) == (0, 3) and tuple(centres.shape) == (0, 3)
    every = np.ones(LIST_DIMS, dtype=bool)
    _check_listing(_grid_of(every, dev), every)


# ------------------------------------------------------------------------------------------------------------ 4. the largest grid

def test_the_largest_grid_through_a_window_in_its_far_corner(dev):
    """(2047, 2045, 511): word indices up to 2^26, 262 144 blocks in the listing and 1 024 entries per lane in its scan, brick masks
    at far edges that are no brick multiple.  Three 256 MB planes at most are alive at once; dense() is never called."""
    from trajectory_optimization_amd import ops
    dims, win = mc.BIG_DIMS, mc.BIG_WINDOW
    assert dims[0] * dims[1] * dims[2] == 2_139_104_765 < 1 << 31 and all(d % b for d, b in zip(dims, (4, 4, 2)))
    c = mc.window_case(dims, win)
    off = c["off"]
    assert off.tolist() == [1983, 1981, 479]
    window, shift = _t(c["win_ijk"], dev), _t(off, dev).to(torch.int32)
    # insert, lookup, count, export
    g = ops.OccupancyGrid(ORIGIN, RES, dims, device=dev)
    assert g.count() == 0
    assert g.insert(_t(c["centres"], dev)) == 0
    assert _same(g.lookup(window), c["occ"].ravel().astype(np.uint8))
    assert g.lookup(_t(c["ijk"][-3:], dev)).tolist() == [1, 1, 1]
    assert g.lookup(_t(np.array([[2047, 2044, 510], [2046, 2045, 510], [2046, 2044, 511], [1, 0, 0], [2045, 0, 0]]), dev)).tolist() == [0] * 5
    assert g.count() == len(c["distinct"]) == int(c["occ"].sum()) + 2
    ijk, centres = synth.occ_export_sparse(c["distinct"], dims, ORIGIN, RES)
    got_ijk, got_centres = g.export()
    assert _same(got_ijk, ijk) and _same(got_centres, centres)
    # rays: line of sight, then the carve of a fresh plane read back through the window and by count()
    a, b = _t(c["a"], dev), _t(c["b"], dev)
    for skip, want in c["los"].items():
        assert (want == 0).sum() > 500 and (want == 1).sum() > 500
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        got = g.line_of_sight(a, b, skip=skip, stats=stats)
        assert _same(got, want), (skip, _first_difference(got, want))
        assert int(stats[0]) == len(want)
    assert len(c["leaves"]) > 1000 and (c["qb"][c["leaves"]] >= np.asarray(dims) * 256).any(axis=1).all()
    free = None
    for max_range in (mc.WINDOW_RANGE, None):   # (the plane of None stays for the state and the frontier)
        del free
        plane, flags_ref, visits = c["carve"][max_range]
        assert plane.any() and (max_range is None or 500 < (flags_ref == 1).sum() < len(flags_ref) - 500)
        free = g.empty_like()
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
        flags = torch.full((len(flags_ref),), 9, dtype=torch.uint8, device=dev)
        assert free.carve(a, b, max_range, stats=stats, flags=flags) == 0
        assert _same(flags, flags_ref) and stats.tolist()[:2] == [len(flags_ref), visits]
        assert _same(free.lookup(window), plane.ravel().astype(np.uint8))
        assert free.count() == int(plane.sum())   # (nothing was carved outside the window)
    # the three states at positions over the window and the far apron
    space = ops.SpaceMap(g, free)
    assert set(c["state"].tolist()) == {0, 1, 2, 3}
    assert _same(space.state(_t(c["pos"], dev)), c["state"])
    # the frontier, through export()
    assert len(c["frontier"]) > 1000
    ijk, centres = synth.occ_export_sparse(c["frontier"], dims, ORIGIN, RES)
    fr = space.frontier(1)
    assert fr.n == len(ijk) and _same(fr.ijk, ijk) and _same(fr.points, centres)
    assert bool((fr.ijk >= shift + 1).all())
    del fr, space, free, g
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ 5. the whole range

def test_rays_across_the_whole_range(dev):
    """256 rays from the apron through dims to the range limit on the other side, up to about 18 000 steps each; the truncated carve
    at R = 4000 * 256 takes carve_clip's products near 2^41."""
    from trajectory_optimization_amd import ops
    c = mc.long_case()
    n = len(c["a"])
    steps = np.abs((c["qb"] >> 8) - (c["qa"] >> 8)).sum(axis=1)
    print(f"steps: median {int(np.median(steps))}, max {int(steps.max())}; rays crossing dims {int(c['crosses'].sum())} of {n}")
    assert n == 256 and c["crosses"].sum() >= n // 2 and steps.max() > 12_000
    assert (c["los"] == 0).sum() >= 20 and (c["los"] == 1).sum() >= 20
    D = (c["qb"] - c["qa"]).astype(np.int64)
    assert int(np.abs(D).max()) * mc.LONG_R > 1 << 40
    a, b = _t(c["a"], dev), _t(c["b"], dev)
    g = _grid_of(c["occ"], dev)
    got = g.line_of_sight(a, b)
    assert _same(got, c["los"]), _first_difference(got, c["los"])
    for R, max_range in ((0, None), (mc.LONG_R, mc.LONG_RANGE)):
        want, skipped, flags_ref, visits = c["carve"][R]
        assert skipped == 0 and want.any() and (R == 0 or (flags_ref == 1).sum() > n // 2)
        assert synth.carve_range(max_range, RES) == R
        free = ops.OccupancyGrid(ORIGIN, RES, DIMS, device=dev)
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
        flags = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        assert free.carve(a, b, max_range, stats=stats, flags=flags) == 0
        assert _same(free.dense(), want) and _same(flags, flags_ref)
        assert stats.tolist()[:2] == [n, visits]
