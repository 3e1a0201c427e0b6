"""Connected components on the GPU (ops.Components, tools.label_components, tools.frontier_clusters, components_kernels.hip): every
comparison is torch.equal (or integer equality) against the numpy restatements (synth.components_*, themselves checked against
scipy.ndimage.label in tests/test_components_cpu.py)."""
import numpy as np
import pytest
import torch

import components_cases as cc
import travel_cases as tc
from map_size_cases import FIELD_DIMS, FIELD_ORIGIN
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
ORIGIN, RES = cc.ORIGIN, cc.RES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _grid_of(bits, dev, origin=ORIGIN, r=RES):
    """An OccupancyGrid holding exactly the voxels of `bits` (their centres inserted)."""
    from trajectory_optimization_amd import ops
    g = ops.OccupancyGrid(origin, r, bits.shape, device=dev)
    _, centres = synth.occ_export_ref(bits, origin, r)
    if len(centres):
        assert g.insert(_t(centres, dev)) == 0
    return g


def _labels_of(ids):
    """A dense id volume (nx,ny,nz), -1 clear -> the flat int32 label volume, x fastest."""
    return torch.from_numpy(np.ascontiguousarray(ids.transpose(2, 1, 0)).reshape(-1).astype(np.int32))


def _same(comp, plane, c, origin=ORIGIN, r=RES, what=None):
    """Every buffer of a Components against the restatement of `plane`."""
    ids, roots = synth.components_ref(plane, c)
    s = synth.components_stats_ref(ids, origin, r)
    C = len(roots)
    assert comp.n == C, (what, comp.n, C)
    assert comp.labels.dtype == torch.int32 and torch.equal(comp.labels.cpu(), _labels_of(ids)), what
    assert torch.equal(comp.dense().cpu(), torch.from_numpy(ids)), what
    assert comp.roots.dtype == torch.int32 and torch.equal(comp.roots.cpu(), torch.from_numpy(roots.astype(np.int32))), what
    assert comp.sizes.dtype == torch.int64 and torch.equal(comp.sizes.cpu(), torch.from_numpy(s["sizes"])), what
    assert comp.sums.dtype == torch.int64 and tuple(comp.sums.shape) == (C, 3) and torch.equal(comp.sums.cpu(), torch.from_numpy(s["sums"])), what
    assert comp.bbox.dtype == torch.int32 and tuple(comp.bbox.shape) == (C, 2, 3) and torch.equal(comp.bbox.cpu(), torch.from_numpy(s["bbox"])), what
    assert comp.centroids.dtype == torch.float32 and torch.equal(comp.centroids.cpu(), torch.from_numpy(s["centroids"])), what
    return ids, roots


# ------------------------------------------------------------------------------------------------------------ 1. the matrix

@pytest.mark.parametrize("fill", sorted(cc.FILLS))
@pytest.mark.parametrize("dims", cc.GRIDS, ids=str)
def test_build_equals_the_restatement(dev, dims, fill):
    from trajectory_optimization_amd import ops
    plane = cc.plane_of(dims, fill)
    grid = _grid_of(plane, dev)
    counts = []
    for c in cc.CONNECTIVITIES:
        comp = ops.Components(grid, c)
        _same(comp, plane, c, what=(dims, fill, c))
        assert (comp.rounds > 0) == bool(plane.any())
        counts.append(comp.n)
    if dims == (64, 64, 32) and fill in ("2%", "30%"):
        assert counts[0] > counts[1] > counts[2] >= 1, counts   # the three connectivities cannot be confused
    if fill == "full":
        assert counts == [1, 1, 1]
    if fill == "empty":
        assert counts == [0, 0, 0] and bool((comp.labels == -1).all())


# ------------------------------------------------------------------------------------------------------------ 2. the checkerboard

def test_checkerboard_singletons_and_one_component(dev):
    from trajectory_optimization_amd import ops
    board = cc.checkerboard()
    grid = _grid_of(board, dev)
    comp = ops.Components(grid, 6)
    assert comp.n == 65536 and bool((comp.sizes == 1).all())
    nx, ny, nz = board.shape
    lin = torch.arange(nx * ny * nz, device=dev)
    set_ = comp.labels >= 0
    assert torch.equal(comp.roots.long(), lin[set_])                                     # the roots are the set indices, ascending ...
    assert torch.equal(comp.labels[set_].long(), torch.arange(65536, device=dev))        # ... and the ids their ranks
    assert torch.equal(comp.bbox[:, 0], comp.bbox[:, 1]) and torch.equal(comp.sums.int(), comp.bbox[:, 0])
    _same(comp, board, 6)
    for c in (18, 26):
        comp = ops.Components(grid, c)
        assert comp.n == 1 and comp.roots.tolist() == [0] and comp.sizes.tolist() == [65536]
        assert torch.equal(comp.dense().cpu(), torch.from_numpy(np.where(board, 0, -1)))


# ------------------------------------------------------------------------------------------------------------ 3. hand cases

@pytest.mark.parametrize("name", sorted(cc.hand_cases()))
def test_hand_cases_on_the_device(dev, name):
    from trajectory_optimization_amd import tools
    plane, counts = cc.hand_cases()[name]
    grid = _grid_of(plane, dev)
    for c in cc.CONNECTIVITIES:
        comp = tools.label_components(grid, c)
        assert comp.n == counts[c], (name, c, comp.n)
        _same(comp, plane, c, what=(name, c))
    if name == "full_plane":
        assert comp.sizes.tolist() == [plane.size] and comp.bbox.tolist() == [[[0, 0, 0], [d - 1 for d in plane.shape]]]


# ------------------------------------------------------------------------------------------------------------ 4. the serpentine

@pytest.mark.parametrize("which", ["forward", "reversed"])
def test_the_serpentine_whatever_the_rounds_per_check(dev, which):
    from trajectory_optimization_amd import ops
    plane = cc.serpentines()[which]
    grid = _grid_of(plane, dev)
    for c in cc.CONNECTIVITIES:
        bufs = []
        for rpc in (1, 16, 1000):
            comp = ops.Components(grid, c, rounds_per_check=rpc)
            ids, roots = _same(comp, plane, c, what=(which, c, rpc))
            assert comp.n == 1 and comp.rounds > 5, (which, c, rpc, comp.rounds)
            bufs.append([b.clone() for b in (comp.labels, comp.roots, comp.sizes, comp.sums, comp.bbox, comp.centroids)])
        for other in bufs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(bufs[0], other))
    # the root: the x = 0 end of the first lane (y = 1), and in the flipped copy of what was the last (y = 37 -> 3)
    x, y, z = (0, 1, 0) if which == "forward" else (0, 3, 0)
    assert comp.roots.tolist() == [(z * plane.shape[1] + y) * plane.shape[0] + x] and comp.sizes.tolist() == [int(plane.sum())]


# ------------------------------------------------------------------------------------------------------------ 5. second trips

def test_second_trips_at_300_280_8(dev):
    from trajectory_optimization_amd import ops
    plane = np.random.default_rng(43).random(FIELD_DIMS) < 0.3
    grid = _grid_of(plane, dev, FIELD_ORIGIN)
    comp = ops.Components(grid, 6)
    _same(comp, plane, 6, FIELD_ORIGIN)
    assert comp.n > 40_000 and plane.size > 2048 * 256     # more voxels than one pass of a grid-stride kernel holds lanes


# ------------------------------------------------------------------------------------------------------------ 6. the largest grid

def test_the_largest_grid_through_a_window_in_its_far_corner(dev):
    """(2047, 2045, 511): an 8.5 GB label volume, byte offsets beyond 2^32, roots near 2^31.  The plane is empty but for a 30 % fill of
    a 64 x 64 x 32 window in the far corner: the labels inside the window are the window's restatement with the roots' ranks, the
    roots the window's with their indices mapped, and no word outside the window is anything but the sentinel."""
    from trajectory_optimization_amd import ops
    dims, win = (2047, 2045, 511), (64, 64, 32)
    nx, ny, nz = dims
    off = tuple(d - w for d, w in zip(dims, win))
    W = cc.plane_of(win, "30%")
    grid = ops.OccupancyGrid(ORIGIN, RES, dims, device=dev)
    ijk = np.argwhere(W) + np.asarray(off)
    assert grid.insert(_t(tc.centre(ijk), dev)) == 0 and grid.count() == int(W.sum())
    ids, roots = synth.components_ref(W, 6)
    wx, wy, wz = (np.asarray(a, dtype=np.int64) for a in np.unravel_index(roots, (win[2], win[1], win[0]))[::-1])
    big_roots = ((wz + off[2]) * ny + (wy + off[1])) * nx + (wx + off[0])
    assert (np.diff(big_roots) > 0).all() and (1 << 31) - (1 << 28) < big_roots.min() and big_roots.max() < 1 << 31
    comp = ops.Components(grid, 6)
    assert comp.n == len(roots) > 5000 and comp._buf.numel() == 4 * nx * ny * nz > 1 << 32
    assert torch.equal(comp.roots.cpu(), torch.from_numpy(big_roots.astype(np.int32)))
    vol = comp.labels.view(nz, ny, nx)
    got = vol[off[2]:, off[1]:, off[0]:].permute(2, 1, 0).to(torch.int64).cpu()
    assert torch.equal(got, torch.from_numpy(ids))
    s = synth.components_stats_ref(ids, ORIGIN, RES)
    assert torch.equal(comp.sizes.cpu(), torch.from_numpy(s["sizes"]))
    assert torch.equal(comp.sums.cpu(), torch.from_numpy(s["sums"] + s["sizes"][:, None] * np.asarray(off)))
    assert torch.equal(comp.bbox.cpu(), torch.from_numpy(s["bbox"] + np.asarray(off, dtype=np.int32)))
    # no word outside the window is anything but the sentinel: the set words are exactly the window's
    assert int((comp.labels != -1).sum()) == int(W.sum())
    # the lookups and the minimum at those offsets
    far = np.argwhere(W)[-1]
    clear = np.argwhere(~W)[-1]
    pos = np.stack([tc.centre(far + np.asarray(off)), tc.centre(clear + np.asarray(off)), tc.centre((0, 0, 0))])
    assert comp.at(_t(pos, dev)).tolist() == [int(ids[tuple(far)]), -1, -1]
    values = torch.full((nx * ny * nz,), -1, dtype=torch.int32, device=dev)
    values.view(nz, ny, nx)[off[2]:, off[1]:, off[0]:] = 7
    value, voxel = comp.min_over(values)
    assert bool((value == 7).all()) and torch.equal(voxel, comp.roots)   # a constant: the lowest index of each component is its root


# ------------------------------------------------------------------------------------------------------------ 7. min_over

def test_min_over_values_sentinels_and_ties(dev):
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(9)
    dims = (37, 5, 20)
    plane = cc.plane_of(dims, "30%")
    comp = ops.Components(_grid_of(plane, dev), 6)
    ids, roots = _same(comp, plane, 6)
    values = rng.integers(0, 6, size=dims).astype(np.int64)             # few distinct values: ties inside many components
    values[rng.random(dims) < 0.3] = 0xFFFFFFFF
    values[np.isin(ids, [0, 2, len(roots) - 1])] = 0xFFFFFFFF           # whole components at the sentinel
    values[0, 0, 0] = 0xFFFFFFFE                                        # the largest value there is
    flat = _t(values.transpose(2, 1, 0).reshape(-1).astype(np.uint32).view(np.int32), dev)
    want_value, want_voxel = synth.components_min_ref(ids, values)
    for vals in (flat, flat.view(torch.uint8)):
        value, voxel = comp.min_over(vals)
        assert value.dtype == torch.int64 and voxel.dtype == torch.int32
        assert torch.equal(value.cpu(), torch.from_numpy(want_value)) and torch.equal(voxel.cpu(), torch.from_numpy(want_voxel.astype(np.int32)))
    ties = sum(int((values[ids == i] == want_value[i]).sum() > 1) for i in range(len(roots)) if want_value[i] >= 0)
    assert value[0] == -1 and voxel[2] == -1 and int((want_value >= 0).sum()) > 100 and int((want_value < 0).sum()) > 10 and ties > 10
    with pytest.raises(ValueError, match="values must be"):
        comp.min_over(flat[:-1])


def test_min_over_a_real_travel_field(dev):
    from trajectory_optimization_amd import ops
    dims = (37, 5, 20)
    occ = tc.occ_of(dims, "2%")
    grid = _grid_of(occ, dev)
    field = ops.ClearanceField(grid, D=tc.D)
    T = synth.travel_traversable_ref(synth.field_ref(occ, None, tc.D), 1)
    src = np.argwhere(T)[len(np.argwhere(T)) // 2]
    tf = ops.TravelField(field, tc.RADIUS, _t(tc.centre(src)[None], dev), max_dist=20 * RES)
    cost = synth.travel_ref(T, [src], tf.limit)
    plane = cc.plane_of(dims, "30%", seed=3)
    comp = ops.Components(_grid_of(plane, dev), 6)
    ids, roots = synth.components_ref(plane, 6)
    want_value, want_voxel = synth.components_min_ref(ids, np.where(cost < 0, 0xFFFFFFFF, cost))
    value, voxel = comp.min_over(tf)
    assert torch.equal(value.cpu(), torch.from_numpy(want_value)) and torch.equal(voxel.cpu(), torch.from_numpy(want_voxel.astype(np.int32)))
    assert int((want_value >= 0).sum()) > 10 and int((want_value < 0).sum()) > 10
    other = ops.TravelField(ops.ClearanceField(_grid_of(np.zeros((5, 6, 3), bool), dev), D=tc.D), tc.RADIUS, _t(tc.centre((1, 1, 1))[None], dev))
    with pytest.raises(ValueError, match="the travel field's dims differs"):
        comp.min_over(other)


# ------------------------------------------------------------------------------------------------------------ 8. at()

def test_at_clear_nan_out_of_range_and_outside_dims(dev):
    from trajectory_optimization_amd import ops
    dims = (37, 5, 20)
    plane = cc.plane_of(dims, "30%")
    comp = ops.Components(_grid_of(plane, dev), 26)
    ids, _ = synth.components_ref(plane, 26)
    rng = np.random.default_rng(2)
    pos = (np.asarray(ORIGIN, dtype=f32) + rng.uniform(-2, [39, 7, 22], size=(4000, 3)).astype(f32) * f32(RES)).astype(f32)
    pos = np.concatenate([pos, tc.centre(np.argwhere(plane)[:50]), tc.centre(np.argwhere(~plane)[:50]),
                          np.array([[np.nan, 0, 0], [np.inf, 2, 1], [1e9, 2, 1], [-1e9, 2, 1]], dtype=f32), tc.centre([(37, 0, 0), (0, -1, 0), (0, 0, 20)])])
    want = synth.components_positions_ref(pos, ORIGIN, RES, ids)
    got = comp.at(_t(pos, dev))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(want))
    assert want[-7:].tolist() == [-2] * 7 and (want[4000:4050] >= 0).all() and (want[4050:4100] == -1).all()
    assert (want[:4000] == -2).sum() > 100 and (want[:4000] >= 0).sum() > 100
    assert comp.at(torch.empty((0, 3), device=dev)).numel() == 0


# ------------------------------------------------------------------------------------------------------------ 9. frontier clusters

@pytest.fixture(scope="module")
def slit(dev):
    from trajectory_optimization_amd import ops
    occ, free, robot = cc.slit_world()
    origin = (0.0, 0.0, 0.0)
    space = ops.SpaceMap(_grid_of(occ, dev, origin), _grid_of(free, dev, origin))
    field = ops.ClearanceField(space, D=tc.D)                       # unknown='free': a frontier voxel can be traversable
    tf = ops.TravelField(field, tc.RADIUS, _t(tc.centre(robot, origin)[None], dev), space=space)
    return dict(space=space, field=field, tf=tf, occ=occ, free=free, origin=origin)


def test_frontier_clusters_on_the_two_rooms_with_a_slit(dev, slit):
    from trajectory_optimization_amd import ops, tools
    space, tf, occ, free, origin = (slit[k] for k in ("space", "tf", "occ", "free", "origin"))
    front = synth.frontier_ref(occ, free, 1)
    ids, roots = synth.components_ref(front, 26)
    s = synth.components_stats_ref(ids, origin, RES)
    assert sorted(s["sizes"].tolist()) == [1, 1, 1, 96, 128]         # three strays, the shell of the blob, the sheet in the hall
    cost = tf.dense().cpu().numpy()
    want_value, want_voxel = synth.components_min_ref(ids, np.where(cost < 0, 0xFFFFFFFF, cost))
    for min_size, K in ((1, 5), (2, 2), (97, 1), (129, 0)):
        fc = tools.frontier_clusters(space, min_size=min_size, travel=tf)
        order = synth.frontier_clusters_ref(s["sizes"], want_value, min_size)
        assert fc.n == K == len(order) and torch.equal(fc.ids.cpu(), torch.from_numpy(order))
        assert torch.equal(fc.sizes.cpu(), torch.from_numpy(s["sizes"][order])) and torch.equal(fc.bbox.cpu(), torch.from_numpy(s["bbox"][order]))
        assert torch.equal(fc.centroids.cpu(), torch.from_numpy(s["centroids"][order]))
        assert torch.equal(fc.reachable.cpu(), torch.from_numpy(want_value[order] >= 0))
        want_cost = np.where(want_value[order] >= 0, want_value[order] / 64.0 * float(f32(RES)), np.inf)
        assert fc.cost.dtype == torch.float64 and torch.equal(fc.cost.cpu(), torch.from_numpy(want_cost))
        vox = want_voxel[order]
        nx, ny, _ = occ.shape
        want_app = np.where((vox >= 0)[:, None], tc.centre(np.stack([vox % nx, (vox // nx) % ny, vox // (nx * ny)], axis=1), origin), np.nan).astype(f32)
        assert fc.approach.dtype == torch.float32 and torch.equal(torch.nan_to_num(fc.approach.cpu(), nan=-7.0),
                                                                  torch.from_numpy(np.nan_to_num(want_app, nan=-7.0)))
    fc = tools.frontier_clusters(space, travel=tf)
    assert fc.sizes.tolist() == [96, 128, 1, 1, 1] and fc.reachable.tolist() == [True, False, False, False, False]
    assert tools.frontier_clusters(space, min_size=2, travel=tf).sizes.tolist() == [96, 128]      # exactly the strays fall
    assert int(fc.bbox[1, 0, 0]) == 30 and int(fc.bbox[1, 1, 0]) == 30                            # the hall's sheet: unreachable
    assert fc.frontier.n == 96 + 128 + 3 and fc.components.n == 5 and isinstance(fc.components, ops.Components)
    # the nearest reachable opening is a goal the travel layer takes as it is
    goal = fc.approach[fc.reachable][0]
    path = tools.travel_path(tf, goal)
    assert path.reachable and path.cost == int(want_value[int(fc.ids[0])]) and float(fc.cost[0]) == path.cost / 64.0 * float(f32(RES))
    assert torch.equal(path.poses[-1], goal) and int(fc.components.at(goal[None])[0]) == int(fc.ids[0])
    assert bool((space.state(fc.approach[fc.reachable]) == 1).all())
    # without a travel field: by size, then id; nothing is reachable
    plain = tools.frontier_clusters(space, connectivity=26)
    assert plain.sizes.tolist() == [128, 96, 1, 1, 1] and not bool(plain.reachable.any()) and bool(torch.isinf(plain.cost).all())
    assert torch.equal(plain.ids.cpu(), torch.from_numpy(synth.frontier_clusters_ref(s["sizes"])))
    # under c = 6 the blob's shell falls into its six faces
    six = tools.frontier_clusters(space, connectivity=6, travel=tf)
    assert sorted(six.sizes.tolist()) == [1, 1, 1, 16, 16, 16, 16, 16, 16, 128] and six.reachable.tolist() == [True] * 6 + [False] * 4
    # with unknown='obstacle' no frontier voxel is traversable: the documented limit
    strict = ops.TravelField(ops.ClearanceField(space, D=tc.D, unknown="obstacle"), tc.RADIUS, tf.sources, space=space)
    assert not bool(tools.frontier_clusters(space, travel=strict).reachable.any())
    for kw, text in ((dict(min_size=0), "min_size"), (dict(travel=object()), "travel must be"), (dict(connectivity=7), "connectivity")):
        with pytest.raises(ValueError, match=text):
            tools.frontier_clusters(space, **kw)


# ------------------------------------------------------------------------------------------------------------ 10. determinism, rebuild

def test_two_builds_are_identical_and_a_rebuild_merges_across_a_bridge(dev):
    from trajectory_optimization_amd import ops
    dims = (37, 5, 20)
    plane = cc.plane_of(dims, "30%")
    plane[10:13, 2, 7] = [True, False, True]
    plane[11, 1:4, 6:9] = False                      # (11, 2, 7) is clear and its other face neighbours too: it bridges exactly two
    plane[10, 2, 7] = plane[12, 2, 7] = True
    grid = _grid_of(plane, dev)
    a, b = ops.Components(grid, 6), ops.Components(grid, 6)
    for name in ("labels", "roots", "sizes", "sums", "bbox", "centroids"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    ids, _ = _same(a, plane, 6)
    assert ids[10, 2, 7] != ids[12, 2, 7]
    before, buf = a.n, a.labels.data_ptr()
    assert grid.insert(_t(tc.centre((11, 2, 7))[None], dev)) == 0
    plane[11, 2, 7] = True
    assert a.rebuild() is a and a.n == before - 1 and a.labels.data_ptr() == buf
    ids, _ = _same(a, plane, 6)
    assert ids[10, 2, 7] == ids[11, 2, 7] == ids[12, 2, 7]
    assert b.n == before                             # (the other object still holds the old labelling)
