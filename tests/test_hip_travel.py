"""The travel field on the GPU (ops.TravelField, travel_kernels.hip): every comparison is torch.equal (or integer equality) against
the numpy restatements (synth.travel_ref / travel_positions_ref / travel_paths_ref / view_pick_travel_ref, themselves checked against
a heapq Dijkstra in tests/test_travel_cpu.py) or, at size, against the Bellman certificate evaluated in torch ops."""
import numpy as np
import pytest
import torch

import travel_cases as tc
from map_size_cases import FIELD_DIMS, FIELD_ORIGIN
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
ORIGIN, RES, RADIUS = tc.ORIGIN, tc.RES, tc.RADIUS


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


def _field_of(T, dev, origin=ORIGIN, r=RES):
    """A ClearanceField (D = 3) whose buffer is written directly: 65535 in T, 0 elsewhere — with need2 = 1 its traversable set is T."""
    from trajectory_optimization_amd import ops
    field = ops.ClearanceField(ops.OccupancyGrid(origin, r, T.shape, device=dev), D=tc.D)
    _write(field, T)
    return field


def _write(field, T):
    nx, ny, nz = field.dims
    field.buf.view(torch.int16).view(nz, ny, nx).copy_(_t(np.where(T, -1, 0).astype(np.int16).transpose(2, 1, 0), field.device))


def _want(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))


def _travel(field, src, **kw):
    from trajectory_optimization_amd import ops
    return ops.TravelField(field, RADIUS, _t(np.asarray(src, dtype=f32).reshape(-1, 3), field.device), **kw)


# ------------------------------------------------------------------------------------------------------------ 1. the build

@pytest.mark.parametrize("fill", tc.FILLS)
@pytest.mark.parametrize("dims", tc.GRIDS, ids=str)
def test_build_equals_the_restatement(dev, dims, fill):
    from trajectory_optimization_amd import ops
    occ, free = tc.occ_of(dims, fill), tc.free_of(dims)
    grid = _grid_of(occ, dev)
    space = ops.SpaceMap(grid, _grid_of(free, dev))
    field = ops.ClearanceField(grid, D=tc.D)
    assert field.need2(RADIUS) == 1
    fref = synth.field_ref(occ, None, tc.D)
    state = np.where(occ, 2, np.where(free, 1, 0))
    for with_space in (False, True):
        T = synth.travel_traversable_ref(fref, 1, state if with_space else None)
        for n in (1, 3):
            src = tc.sources_of(T, n)
            seeded, vox = synth.travel_seeds_ref(src, ORIGIN, RES, T)
            assert seeded[-3:].tolist() == [0, 0, 0] and seeded[:n].all() == T.any()
            for max_dist in tc.MAX_DISTS:
                limit = synth.travel_limit(max_dist, RES)
                tf = ops.TravelField(field, RADIUS, _t(src, dev), space=space if with_space else None, max_dist=max_dist)
                ref = synth.travel_ref(T, vox[seeded == 1], limit)
                got = tf.dense().cpu()
                what = (with_space, n, max_dist)
                assert got.dtype == torch.int64 and tuple(got.shape) == dims and torch.equal(got, _want(ref)), what
                assert torch.equal(tf.seeded.cpu(), torch.from_numpy(seeded)) and tf.limit == limit, what
                assert (tf.rounds > 0) == bool(T.any()), what
                if max_dist is not None:
                    assert int(got.max()) <= 640
    if fill == "full":
        assert bool((got == -1).all())


# ------------------------------------------------------------------------------------------------------------ 2. the serpentine

def test_the_serpentine_whatever_the_rounds_per_check(dev):
    T, src, goal = tc.serpentine()
    field = _field_of(T, dev)
    ref = _want(synth.travel_ref(T, [src]))
    bufs = []
    for rpc in (1, 16, 1000):
        tf = _travel(field, tc.centre(src), rounds_per_check=rpc)
        assert torch.equal(tf.dense().cpu(), ref), rpc
        assert tf.rounds > 16, (rpc, tf.rounds)
        bufs.append(tf.buf.clone())
    assert torch.equal(bufs[0], bufs[1]) and torch.equal(bufs[0], bufs[2])
    assert int(ref[goal]) > 640 * 64 and int(ref.max()) - int(ref[goal]) <= 111   # (the far end of the last lane, z = 1 of three)


# ------------------------------------------------------------------------------------------------------------ 3. the move rule

@pytest.mark.parametrize("name", sorted(tc.hand_cases()))
def test_the_move_rule_on_the_device(dev, name):
    T, src, want = tc.hand_cases()[name]
    tf = _travel(_field_of(T, dev), tc.centre(src))
    got = tf.dense().cpu()
    for v, c in want.items():
        assert int(got[v]) == c, (name, v, int(got[v]), c)
    assert torch.equal(got, _want(synth.travel_ref(T, [src])))
    assert tf.seeded.tolist() == [1]


# ------------------------------------------------------------------------------------------------------------ 4. lookups and paths

@pytest.fixture(scope="module")
def maze(dev):
    """A random traversable set over (21, 13, 6), a field that holds it, its travel field from one source and the restatement."""
    dims = (21, 13, 6)
    T = np.random.default_rng(5).random(dims) < 0.8
    src = np.argwhere(T)[len(np.argwhere(T)) // 2]
    field = _field_of(T, dev)
    tf = _travel(field, tc.centre(src))
    ref = synth.travel_ref(T, [src])
    assert torch.equal(tf.dense().cpu(), _want(ref)) and (ref >= 0).sum() > 500
    return dict(T=T, src=src, field=field, tf=tf, ref=ref, dims=dims)


def _positions(dims, seed):
    """Positions over the box and a rim around it (the apron), then far out of range and non-finite rows."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(dims, dtype=np.float64) * RES
    pos = (rng.random((400, 3)) * ext * 1.5 - 0.25 * ext + np.asarray(ORIGIN)).astype(f32)
    bad = np.array([[1e9, 0, 0], [np.nan, 2.5, 1.0], [0, np.inf, 0], [0, 0, -np.inf], [-300.0, 2.5, 1.0], [600.0, 2.5, 1.0]], dtype=f32)
    return np.concatenate([pos, bad])


def test_cost_distance_and_reachable(dev, maze):
    tf, ref = maze["tf"], maze["ref"]
    pos = _positions(maze["dims"], 17)
    codes = synth.travel_positions_ref(pos, ORIGIN, RES, ref)
    assert (codes == -2).sum() >= 6 and (codes >= 0).sum() > 50 and (codes == -1).any()
    assert torch.equal(tf.cost(_t(pos, dev)).cpu(), torch.from_numpy(codes))
    assert torch.equal(tf.reachable(_t(pos, dev)).cpu(), torch.from_numpy(codes >= 0))
    got = tf.distance(_t(pos, dev)).cpu().numpy()
    want = synth.travel_metres(codes, RES)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32)[codes != -2], want.view(np.int32)[codes != -2])
    assert np.isnan(got[codes == -2]).all() and np.isinf(got[codes == -1]).all()
    assert tf.cost(torch.empty((0, 3), device=dev)).shape == (0,)


def test_paths_equal_the_restatement_and_every_leg_is_open(dev, maze):
    from trajectory_optimization_amd import tools
    tf, ref, T, field = maze["tf"], maze["ref"], maze["T"], maze["field"]
    pos = _positions(maze["dims"], 23)
    far = np.unravel_index(int(ref.argmax()), ref.shape)
    goals = np.concatenate([pos[:60], pos[-6:], tc.centre([far, tuple(maze["src"])])])
    want = synth.travel_paths_ref(goals, ORIGIN, RES, ref, T)
    got = tf.paths(_t(goals, dev))
    assert len(got) == len(want) and sum(len(w) > 1 for w in want) > 10 and sum(len(w) == 0 for w in want) > 6
    for e, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.float32 and torch.equal(g.cpu(), torch.from_numpy(w[::-1].copy())), e   # (source -> goal)
    legs_a = torch.cat([g[:-1] for g in got if len(g) > 1])
    legs_b = torch.cat([g[1:] for g in got if len(g) > 1])
    d, idx, _ = field.edges(legs_a, legs_b, RADIUS)
    assert bool(torch.isinf(d).all()) and bool((idx == -1).all()) and len(d) > 100
    # a path's hops add up to its cost
    hops = (got[-2][1:] - got[-2][:-1]).abs().div(RES).round().ne(0).sum(dim=1).cpu().numpy()
    assert int(sum(synth.TRAVEL_WEIGHTS[k - 1] for k in hops)) == int(ref[far])
    # the overflow report, and the sizes that fit
    L = len(want[-2])
    assert L > 8 and len(tf.paths(_t(goals[-2:], dev), max_rows=L)[0]) == L
    with pytest.raises(ValueError, match=f"goal 0 needs {L} rows, max_rows is {L - 1}"):
        tf.paths(_t(goals[-2:], dev), max_rows=L - 1)
    assert tf.paths(torch.empty((0, 3), device=dev)) == []
    # one path through the public wrapper, and refine_path takes its poses as they are
    path = tools.travel_path(tf, goals[-2])
    assert path.reachable and path.cost == int(ref[far]) and torch.equal(path.poses, got[-2])
    assert path.length == float(synth.travel_metres([path.cost], RES)[0])
    fine = tools.refine_path(field, path.poses, clearance_radius=RADIUS)
    assert not bool(fine.leg_blocked.any()) and fine.length <= fine.input_length and len(fine.poses) <= L
    assert torch.equal(fine.poses[0], path.poses[0]) and torch.equal(fine.poses[-1], path.poses[-1])
    lost = tools.travel_path(tf, goals[60])   # (out of range)
    assert not lost.reachable and lost.cost == -2 and lost.poses.shape == (0, 3) and np.isnan(lost.length)


# ------------------------------------------------------------------------------------------------------------ 5. at size

def _shift(a, d, fill):
    """out[v] = a[v + d] where v + d lies inside, else fill (torch, any device)."""
    out = torch.full_like(a, fill)
    src, dst = [], []
    for n, k in zip(a.shape, d):
        src.append(slice(max(k, 0), n + min(k, 0)))
        dst.append(slice(max(-k, 0), n + min(-k, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def _certificate(cost, T, seeds, limit):
    """The Bellman certificate in torch ops: cost == 0 exactly at the seeded voxels; elsewhere cost == min over the allowed moves of
    cost[u] + w where that is <= limit, and -1 exactly where it is not.  With positive weights it has one solution."""
    big = 1 << 40
    c = torch.where(cost < 0, torch.full_like(cost, big), cost)
    best = torch.full_like(cost, big)
    for m, d in enumerate(synth.TRAVEL_MOVES):
        if m == 13:
            continue
        ok = T.clone()
        for ex in {0, d[0]}:
            for ey in {0, d[1]}:
                for ez in {0, d[2]}:
                    ok &= _shift(T, (ex, ey, ez), False)
        cand = _shift(c, d, big) + synth.TRAVEL_WEIGHTS[sum(1 for k in d if k) - 1]
        best = torch.minimum(best, torch.where(ok, cand, torch.full_like(cand, big)))
    is_seed = torch.zeros_like(T)
    for x, y, z in seeds:
        is_seed[x, y, z] = True
    want = torch.where(best <= limit, best, torch.full_like(best, -1))
    want = torch.where(is_seed, torch.zeros_like(want), want)
    return torch.equal(cost, want) and bool(((cost == 0) == is_seed).all())


def test_the_bellman_certificate_at_300_280_8(dev):
    from trajectory_optimization_amd import ops
    occ = np.random.default_rng(41).random(FIELD_DIMS) < 0.03
    grid = _grid_of(occ, dev, FIELD_ORIGIN)
    field = ops.ClearanceField(grid, D=tc.D)
    T = field.dense() >= 1
    inT = torch.nonzero(T)
    seeds = inT[[len(inT) // 3, 2 * len(inT) // 3]].cpu().numpy()
    src = np.concatenate([tc.centre(seeds, FIELD_ORIGIN), tc.sources_of(np.ones(FIELD_DIMS, bool), 0)])
    for max_dist in (None, 12.0):
        tf = ops.TravelField(field, RADIUS, _t(src, dev), max_dist=max_dist)
        assert tf.seeded.tolist() == [1, 1, 0, 0, 0]
        cost = tf.dense()
        assert _certificate(cost, T, seeds.tolist(), tf.limit), max_dist
        assert int((cost >= 0).sum()) > 10_000 and bool((cost[~T] == -1).all())
    # the certificate is not vacuous: one word off by one fails it
    cost[tuple(seeds[0])] += 1
    assert not _certificate(cost, T, seeds.tolist(), tf.limit)


def test_the_largest_grid_through_a_window_in_its_far_corner(dev):
    """(2047, 2045, 511): an 8.5 GB cost array, byte offsets beyond 2^32 (word offsets up to 2^31 - 2^23).  Everything is traversable but
    a closed box of walls, with partitions inside, in a 64 x 64 x 32 window in the far corner; the source stands inside the box, so
    the reached region is the box's inside and the window equals the restatement over the window alone."""
    from trajectory_optimization_amd import ops
    dims, win = (2047, 2045, 511), (64, 64, 32)
    off = tuple(d - w for d, w in zip(dims, win))
    W = np.ones(win, dtype=bool)
    W[4:60, 4:60, [3, 28]] = False
    W[4:60, [4, 59], 3:29] = False
    W[[4, 59], 4:60, 3:29] = False          # the box's six walls
    W[20, 4:50, 3:29] = False               # two partitions that leave a gap at opposite ends
    W[40, 14:60, 3:29] = False
    src_w = (10, 10, 10)
    field = ops.ClearanceField(ops.OccupancyGrid(ORIGIN, RES, dims, device=dev), D=tc.D)
    field.buf.fill_(255)                    # 65535 everywhere
    nx, ny, nz = dims
    view = field.buf.view(torch.int16).view(nz, ny, nx)
    view[off[2]:, off[1]:, off[0]:] = _t(np.where(W, -1, 0).astype(np.int16).transpose(2, 1, 0), dev)
    src = tc.centre(np.asarray(src_w) + np.asarray(off))
    tf = ops.TravelField(field, RADIUS, _t(src[None], dev), max_dist=4.0)
    assert tf.seeded.tolist() == [1] and tf.limit == 2048 and tf.buf.numel() == 4 * nx * ny * nz > 1 << 32
    ref = synth.travel_ref(W, [src_w], tf.limit)
    assert (ref >= 0).sum() > 5000 and ref.max() > 1900 and (ref[5:59, 5:59, 4:28] >= 0).sum() == (ref >= 0).sum()
    cost = tf.buf.view(torch.int32).view(nz, ny, nx)
    got = cost[off[2]:, off[1]:, off[0]:].permute(2, 1, 0).to(torch.int64).cpu()   # (-1: the sentinel's bits as int32)
    assert torch.equal(got, _want(ref))
    # everything sampled outside the window is the sentinel: the slabs around it, the grid's first words and a random sample
    assert bool((cost[off[2] - 40:off[2]] == -1).all()) and bool((cost[:, off[1] - 40:off[1]] == -1).all())
    assert bool((cost[:, :, off[0] - 40:off[0]] == -1).all()) and bool((cost[:2] == -1).all())
    lin = torch.randint(0, nx * ny * nz, (2_000_000,), device=dev)
    inside = (lin % nx >= off[0]) & ((lin // nx) % ny >= off[1]) & (lin // (nx * ny) >= off[2])
    assert bool((tf.buf.view(torch.int32)[lin[~inside]] == -1).all())
    # the queries at those offsets
    far = np.unravel_index(int(ref.argmax()), ref.shape)
    goal = tc.centre(np.asarray(far) + np.asarray(off))
    assert tf.cost(_t(np.stack([goal, src, tc.centre((0, 0, 0))]), dev)).tolist() == [int(ref[far]), 0, -1]
    want = synth.travel_paths_ref(tc.centre(far, (0, 0, 0))[None], (0, 0, 0), RES, ref, W)[0]
    path = tf.paths(_t(goal[None], dev))[0]
    assert len(path) == len(want) and torch.equal(path[0].cpu(), torch.from_numpy(src)) and torch.equal(path[-1].cpu(), torch.from_numpy(goal))
    vox = ((path.cpu().numpy() - np.asarray(ORIGIN, dtype=f32)) / f32(RES)).astype(np.int64) - np.asarray(off)
    want_vox = ((want[::-1] - f32(0)) / f32(RES)).astype(np.int64)
    assert np.array_equal(vox, want_vox)


# ------------------------------------------------------------------------------------------------------------ 6. the selection

Q_PLUS_X = synth.Q_OPTICAL.astype(f32)                                                         # the camera looks along +x
Q_MINUS_X = synth.quat_mul(np.array([0.0, 0.0, 0.0, 1.0]), synth.Q_OPTICAL).astype(f32)        # ... along -x
CAMERA = dict(intrins=torch.from_numpy(synth.K_INTRINS), img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT, min_dist=0.2, max_dist=5.0)


@pytest.fixture(scope="module")
def two_rooms(dev):
    """(40, 16, 8) at r = 0.125: a wall at x = 24 with a slit one voxel wide at y = 8 — narrower than the robot.  Room A (x < 24) is
    known free but for an unknown 4 x 4 x 4 blob near x = 0; of room B only x = 25 .. 30 is known free (seen through the slit), the
    rest is unknown.  Candidates: [0] in room B looking at its unknown end; [1] far from the blob and [2] near it, both looking at it
    from room A and both seeing all of it.  The robot stands next to [2]."""
    from trajectory_optimization_amd import ops
    dims, origin = (40, 16, 8), (0.0, 0.0, 0.0)
    occ = np.zeros(dims, dtype=bool)
    occ[24, :, :] = True
    occ[24, 8, :] = False
    free = np.zeros(dims, dtype=bool)
    free[:24] = True
    free[2:6, 6:10, 2:6] = False
    free[24, 8, :] = True
    free[25:31] = True
    space = ops.SpaceMap(_grid_of(occ, dev, origin), _grid_of(free, dev, origin))
    field = ops.ClearanceField(space, D=tc.D)
    P = tc.centre([(28, 8, 4), (22, 8, 4), (12, 8, 4)], origin)
    Q = np.stack([Q_PLUS_X, Q_MINUS_X, Q_MINUS_X])
    robot = tc.centre((13, 8, 4), origin)
    tf = ops.TravelField(field, RADIUS, _t(robot[None], dev), space=space)
    return dict(space=space, field=field, tf=tf, P=_t(P, dev), Q=_t(Q, dev))


def test_selection_never_moves_behind_the_slit(dev, two_rooms):
    from trajectory_optimization_amd import tools
    space, tf, P, Q = (two_rooms[k] for k in ("space", "tf", "P", "Q"))
    gains = tools.view_volume(space, P, Q, **CAMERA).tolist()
    assert gains[0] > gains[1] == gains[2] == 64
    assert bool((space.state(P) == 1).all())                     # all three are "known free" ...
    assert tf.cost(P).tolist() == [-1, 9 * 64, 64]               # ... the first is not reachable
    plain = tools.select_views_volume(space, P, Q, 3, **CAMERA)
    assert plain.order.tolist() == [0, 1] and plain.travel is None
    same = tools.select_views_volume(space, P, Q, 3, travel=None, travel_weight=0.0, **CAMERA)
    assert torch.equal(same.order, plain.order) and torch.equal(same.gains, plain.gains) and torch.equal(same.revealed.buf, plain.revealed.buf)
    assert torch.equal(same.poses, plain.poses) and same.total == plain.total
    sel = tools.select_views_volume(space, P, Q, 3, travel=tf, **CAMERA)
    assert sel.order.tolist() == [1] and sel.gains.tolist() == [64]      # the best reachable one; [2] then adds nothing, [0] never wins
    assert torch.equal(sel.travel, tf.distance(P[1:2])) and sel.travel.tolist() == [9 * RES]
    near = tools.select_views_volume(space, P, Q, 3, travel=tf, travel_weight=100.0, **CAMERA)
    assert near.order.tolist() == [2] and near.gains.tolist() == [64] and near.travel.tolist() == [RES]
    with pytest.raises(ValueError, match="travel_weight .* too large"):
        tools.select_views_volume(space, P, Q, 3, travel=tf, travel_weight=1e12, **CAMERA)
    with pytest.raises(ValueError, match="travel_weight needs travel="):
        tools.select_views_volume(space, P, Q, 3, travel_weight=1.0, **CAMERA)


def test_the_pick_equals_its_restatement_on_random_rows_with_ties(dev):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd._lib import ptr
    rng = np.random.default_rng(77)
    for M, m in ((1, 0), (7, 5), (300, 1 << 14), (1000, (1 << 31) - 1), (2049, 3)):
        gains = rng.integers(0, 6, M)                         # few values: ties
        cost = rng.integers(-2, 4, M) * 64
        cost[cost < 0] //= 64
        taken = (rng.random(M) < 0.2).astype(np.int32)
        g, c, t = _t(gains.astype(np.int64), dev), _t(cost.astype(np.int64), dev), _t(taken, dev)
        order = torch.full((M + 1,), -1, dtype=torch.int32, device=dev)
        picked = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        stop = torch.zeros(1, dtype=torch.int32, device=dev)
        for j in range(min(M, 12) + 1):
            want = synth.view_pick_travel_ref(gains, taken, cost, m, min_gain=2)
            ops._map_call(dev, "tohip_view_volume_pick_travel", ptr(g), ptr(c), m, ptr(t), M, 2, j, ptr(order), ptr(picked), ptr(stop))
            if want < 0:
                assert stop.item() == 1 and order[j].item() == -1
                break
            taken[want] = 1
            assert (order[j].item(), picked[j].item(), stop.item()) == (want, int(gains[want]), 0), (M, m, j)
            assert torch.equal(t.cpu(), torch.from_numpy(taken))


# ------------------------------------------------------------------------------------------------------------ 7. repeatability

def test_two_builds_are_identical_and_a_rebuild_follows_a_new_wall(dev):
    from trajectory_optimization_amd import ops, tools
    dims = (37, 21, 6)
    occ = np.zeros(dims, dtype=bool)
    occ[18, 4:, :] = True                                  # a wall with a gap at y < 4
    grid = _grid_of(occ, dev)
    field = tools.clearance_field(grid, 3 * RES)
    src, probe = tc.centre((3, 15, 3)), tc.centre((33, 15, 3))
    a = tools.travel_field(field, _t(src, dev), RADIUS)
    b = tools.travel_field(field, _t(src, dev), RADIUS)
    T = synth.travel_traversable_ref(synth.field_ref(occ, None, 3), 1)
    assert torch.equal(a.buf, b.buf) and torch.equal(a.dense().cpu(), _want(synth.travel_ref(T, [(3, 15, 3)])))
    before = int(a.cost(_t(probe[None], dev)).item())
    assert before > 0
    ptr_, first = a.buf.data_ptr(), a.buf.clone()
    occ2 = occ.copy()
    occ2[18, :, :] = True                                  # the gap is shut
    grid.insert(_t(tc.centre(np.argwhere(occ2 & ~occ)), dev))
    assert torch.equal(a.rebuild().buf, first)             # (the travel field follows the clearance field, not the grid)
    field.rebuild()
    assert a.rebuild() is a and a.buf.data_ptr() == ptr_ and not torch.equal(a.buf, first)
    T2 = synth.travel_traversable_ref(synth.field_ref(occ2, None, 3), 1)
    assert torch.equal(a.dense().cpu(), _want(synth.travel_ref(T2, [(3, 15, 3)]))) and int(a.cost(_t(probe[None], dev)).item()) == -1
    # the robot has moved to the other side
    a.rebuild(_t(probe, dev))
    assert torch.equal(a.dense().cpu(), _want(synth.travel_ref(T2, [(33, 15, 3)]))) and a.seeded.tolist() == [1]
    assert int(a.cost(_t(src[None], dev)).item()) == -1 and int(a.cost(_t(probe[None], dev)).item()) == 0
