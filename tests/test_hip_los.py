"""The occupancy bit grid, the exact line-of-sight walk and occlusion='voxel' on the GPU: every comparison is torch.equal against the
numpy restatements (synth.occupancy_ref / los_ref, themselves checked in tests/test_los_cpu.py)."""
import numpy as np
import pytest
import torch

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
DIMS = (64, 64, 32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _grid_of(occ, origin, r, dev):
    """An OccupancyGrid holding exactly the voxels of occ (their centres inserted)."""
    from trajectory_optimization_amd import ops
    g = ops.OccupancyGrid(origin, r, occ.shape, device=dev)
    idx = np.argwhere(occ)
    if len(idx):
        centres = (np.asarray(origin, np.float64)[None, :] + (idx + 0.5) * float(np.float32(r))).astype(np.float32)
        assert g.insert(_t(centres, dev)) == 0
    return g


@pytest.fixture(scope="module")
def random_grid(dev):
    occ = np.random.default_rng(5).random(DIMS) < 0.02
    g = _grid_of(occ, (0.0, 0.0, 0.0), 0.125, dev)
    assert torch.equal(g.dense().cpu(), torch.from_numpy(occ))
    return g, occ


# ------------------------------------------------------------------------------------------------------------ insert and lookup

def _insert_rows(n, seed):
    rng = np.random.default_rng(seed)
    P = (rng.random((n, 3)) * np.array([10.0, 10.0, 6.0]) - 1.0).astype(np.float32)   # the 8 x 8 x 4 m box and a rim outside dims
    special = np.array([[0.125, 0.25, 0.375], [0.0, 0.0, 0.0], [8.0, 1.0, 1.0], [7.99999, 1.0, 1.0], [1.0, 1.0, 4.0], [-1e-7, 1.0, 1.0],
                        [-300.0, 1.0, 1.0], [600.0, 1.0, 1.0], [1.0, 1e9, 1.0], [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf],
                        [2.0, 3.0, 1.125]], dtype=np.float32)
    k = min(n, len(special))
    P[rng.choice(n, size=k, replace=False)] = special[:k]
    return P


@pytest.mark.parametrize("n", [1, 257, 20_000])
def test_insert_and_lookup(dev, n):
    from trajectory_optimization_amd import ops
    origin, r = (0.0, 0.0, 0.0), 0.125
    P = _insert_rows(n, seed=n)
    ref, skipped = synth.occupancy_ref(P, origin, r, DIMS)
    g = ops.OccupancyGrid(origin, r, DIMS, device=dev)
    assert not g.dense().any()
    assert g.insert(_t(P, dev)) == skipped == g.skipped
    dense = g.dense()
    assert dense.shape == DIMS and dense.dtype == torch.bool and torch.equal(dense.cpu(), torch.from_numpy(ref))
    if n > 1:
        assert 0 < skipped < n and ref.any()
    # lookup: any indices, outside dims reads 0
    rng = np.random.default_rng(n + 1)
    ijk = rng.integers(-3, 70, size=(1000, 3))
    inside = ((ijk >= 0) & (ijk < np.array(DIMS))).all(axis=1)
    want = np.zeros(1000, np.uint8)
    want[inside] = ref[ijk[inside, 0], ijk[inside, 1], ijk[inside, 2]]
    got = g.lookup(_t(ijk, dev))
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want))
    # two inserts = one insert of the concatenation; a permutation of the rows; inserting again changes nothing
    Q = _insert_rows(max(n // 2, 1), seed=n + 7)
    both, skipped_both = synth.occupancy_ref(np.concatenate([P, Q]), origin, r, DIMS)
    g.insert(_t(Q, dev))
    g2 = ops.OccupancyGrid(origin, r, DIMS, device=dev)
    perm = rng.permutation(len(P) + len(Q))
    assert g2.insert(_t(np.concatenate([P, Q])[perm], dev)) == skipped_both == g.skipped
    assert torch.equal(g.dense(), g2.dense()) and torch.equal(g2.dense().cpu(), torch.from_numpy(both))
    assert torch.equal(g.buf[256:], g2.buf[256:])
    g2.insert(_t(P, dev))
    assert torch.equal(g2.dense().cpu(), torch.from_numpy(both))


def test_from_points_holds_every_point(dev):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.tools import occupancy_grid
    pts = synth.make_cloud(5000, seed=2, extent=(12.0, 9.0, 3.0)) + np.float32([100.0, -50.0, 7.0])
    g = occupancy_grid(_t(pts, dev), resolution=0.1, margin=2)
    assert isinstance(g, ops.OccupancyGrid) and g.skipped == 0
    r = float(np.float32(0.1))
    assert np.array_equal(g.origin, (r * np.floor(pts.min(axis=0).astype(np.float64) / r) - 2 * r).astype(np.float32))
    ref, skipped = synth.occupancy_ref(pts, g.origin, g.resolution, g.dims)
    assert skipped == 0 and torch.equal(g.dense().cpu(), torch.from_numpy(ref))
    v = np.argwhere(ref)
    assert v.min() >= 2 and (v.max(axis=0) + 2 < np.array(g.dims)).all()   # the margin, on every side
    with pytest.raises(ValueError, match="exceeds 2048 per axis"):
        ops.OccupancyGrid.from_points(_t(pts, dev), resolution=0.005)
    with pytest.raises(ValueError, match="more than 2\\^31 voxels"):
        ops.OccupancyGrid.from_points(_t(synth.make_cloud(100, seed=2, extent=(10.0, 10.0, 4.0)), dev), resolution=0.005)   # 2004 x 2004 x 804
    nan = pts.copy()
    nan[3] = np.nan
    g3 = ops.OccupancyGrid.from_points(_t(nan, dev), resolution=0.1)   # (a row that is not finite is skipped, the box is the others')
    assert g3.skipped == 1 and g3.dims == g.dims


# ------------------------------------------------------------------------------------------------------------ segments

def _vox(*v):
    return [c * 0.125 for c in v]


HAND_A = np.array([_vox(2.5, 3.5, 1.5), _vox(1.5, 2.5, 3.5), _vox(5.25, 2.5, 3.5), _vox(3.0, 2.5, 2.5), _vox(3.0, 2.25, 2.5), _vox(0.5, 0.5, 0.5),
                   _vox(2.5, 2.5, 2.5), _vox(0.25, 0.5, 0.5), _vox(-1.5, 0.5, 0.5), _vox(0.5, 0.5, 0.5), _vox(63.5, 63.5, 31.5)], dtype=np.float32)
HAND_B = np.array([_vox(2.5, 3.5, 1.5), _vox(5.25, 2.5, 3.5), _vox(1.5, 2.5, 3.5), _vox(0.5, 2.5, 2.5), _vox(1.5, 3.75, 2.5), _vox(31.5, 31.5, 31.5),
                   _vox(0.5, 0.5, 0.5), _vox(1.25, 2.5, 2.5), _vox(1.5, 0.5, 0.5), _vox(60.5, 20.5, 0.5), _vox(0.5, 0.5, 0.5)], dtype=np.float32)


def _segments(n, seed):
    """n random segments over the 8 x 8 x 4 m box: a sixth with an end in the apron, a few out of range or not finite, the hand cases
    of tests/test_los_cpu.py in front (as many as fit)."""
    rng = np.random.default_rng(seed)
    box = np.array([8.0, 8.0, 4.0])
    A, B = rng.random((n, 3)) * box, rng.random((n, 3)) * box
    apron = rng.random(n) < 1 / 6
    A[apron] = (rng.random((n, 3)) * 3 * box - box)[apron]
    snap = rng.random(n) < 0.1   # ends exactly on faces and corners
    A[snap] = np.round(A[snap] * 8) / 8
    A, B = A.astype(np.float32), B.astype(np.float32)
    k = min(n, len(HAND_A))
    A[:k], B[:k] = HAND_A[:k], HAND_B[:k]
    if n >= 65:
        A[20], B[21], A[22], B[23], B[24] = [600.0, 1, 1], [1, -300.0, 1], [np.nan, 1, 1], [1, 1, np.inf], [1, 512.0, 1]
        A[25], B[25] = [-255.9, 1, 1], [511.9, 1, 1]   # the apron's ends: in range
    return A, B


@pytest.mark.parametrize("n", [1, 65, 5000])
@pytest.mark.parametrize("skip", [(0, 0), (1, 1), (2, 3)])
def test_segments_equal_the_restatement(dev, random_grid, n, skip):
    from trajectory_optimization_amd.tools import line_of_sight
    g, occ = random_grid
    A, B = _segments(n, seed=n + 10 * skip[1])
    want = synth.los_ref(A, B, g.origin, g.resolution, occ, skip)
    a, b = _t(A, dev), _t(B, dev)
    got = line_of_sight(g, a, b, skip=skip)
    assert got.dtype == torch.uint8 and got.shape == (n,) and torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(line_of_sight(g, a, b, skip=skip), got)   # the same call twice
    if n == 5000:
        assert (want == 0).sum() > 500 and (want == 1).sum() > 500
    if n >= 65:
        assert want[20:25].tolist() == [2] * 5 and want[25] != 2


def test_segments_through_an_empty_and_a_full_grid(dev):
    from trajectory_optimization_amd import ops
    A, B = _segments(5000, seed=3)
    a, b = _t(A, dev), _t(B, dev)
    empty = ops.OccupancyGrid((0, 0, 0), 0.125, DIMS, device=dev)
    in_range = synth.los_ref(A, B, (0, 0, 0), 0.125, np.zeros(DIMS, bool)) != 2
    got = empty.line_of_sight(a, b).cpu().numpy()
    assert (got[in_range] == 1).all() and (got[~in_range] == 2).all() and (~in_range).sum() == 5
    full = _grid_of(np.ones(DIMS, bool), (0, 0, 0), 0.125, dev)
    for skip in ((0, 0), (1, 1), (2, 3)):
        want = synth.los_ref(A, B, (0, 0, 0), 0.125, np.ones(DIMS, bool), skip)
        assert torch.equal(full.line_of_sight(a, b, skip=skip).cpu(), torch.from_numpy(want))
    assert (want == 1).any() and (want == 0).any()
    # the statistics: rays walked and voxels visited
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    empty.line_of_sight(a, b, stats=stats)
    assert int(stats[0]) == int(in_range.sum()) and int(stats[1]) > int(stats[0])


@pytest.mark.parametrize("E", [1, 65, 5000])
def test_line_of_sight_and_carve_count_one_walk(dev, E):
    """The rays of tests/walk_cases.py through an empty (37, 5, 20) grid, given to line_of_sight(skip=(0, 0)) and to carve
    on a fresh free plane: both run the one walk, so they walk the same rays, and carve — which counts v_0 ... v_T where line of sight
    stops before v_T — visits exactly one voxel per ray more.  Both counters equal what synth counts on the CPU; rays out of range
    count in neither."""
    from walk_cases import WALK_DIMS, WALK_R, walk_case
    from trajectory_optimization_amd import ops
    A, B, ok, traces, free_ref, carve_visits = walk_case(E)[:6]
    los_visits = sum(len(t) - 1 for t in traces)
    a, b = _t(A, dev), _t(B, dev)
    g = ops.OccupancyGrid((0, 0, 0), WALK_R, WALK_DIMS, device=dev)
    free = g.empty_like()
    los_stats, carve_stats = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    got = g.line_of_sight(a, b, skip=(0, 0), stats=los_stats)
    skipped = free.carve(a, b, max_range=None, stats=carve_stats)
    los_rays, los_seen = (int(v) for v in los_stats)
    carve_rays, carve_seen = int(carve_stats[0]), int(carve_stats[1])
    print(f"E {E}: rays {los_rays} / {carve_rays} (in range {int(ok.sum())}), visits los {los_seen} (synth {los_visits}) carve {carve_seen} (synth {carve_visits})")
    assert los_rays == carve_rays == int(ok.sum()) and skipped == int((~ok).sum())
    assert carve_seen == los_seen + los_rays
    assert los_seen == los_visits and carve_seen == carve_visits
    assert torch.equal(got.cpu(), torch.from_numpy(np.where(ok, 1, 2).astype(np.uint8)))
    assert torch.equal(free.dense().cpu(), torch.from_numpy(free_ref))


def test_a_wall_hides_what_lies_behind_it(dev):
    from trajectory_optimization_amd import ops
    occ = np.zeros(DIMS, bool)
    occ[30] = True
    g = _grid_of(occ, (0.0, 0.0, 0.0), 0.1, dev)
    assert torch.equal(g.dense().cpu(), torch.from_numpy(occ))
    pts = (np.random.default_rng(8).random((20_000, 3)) * np.array([6.4, 6.4, 3.2])).astype(np.float32)
    cam = np.broadcast_to(np.float32([1.03, 3.2, 1.6]), pts.shape).copy()
    got = g.line_of_sight(_t(cam, dev), _t(pts, dev)).cpu().numpy()
    assert np.array_equal(got, synth.los_ref(cam, pts, g.origin, g.resolution, occ))
    vx = synth.occ_fixed(pts, g.origin, g.resolution)[0][:, 0] >> 8
    assert (got[vx > 32] == 0).all() and (vx > 32).sum() > 5000     # behind the wall (and beyond the skipped neighbourhood of the end)
    assert (got[vx < 30] == 1).all() and (vx < 30).sum() > 5000     # in front of it


# ------------------------------------------------------------------------------------------------------------ occlusion rows

def _kept_masks(points, poses, quats, cam, dev):
    """(W, N) bool in the caller's order: what cull_waypoints keeps."""
    from trajectory_optimization_amd import ops
    kept_idx, _, counts, _ = ops.cull_waypoints(points, poses, quats, cam, 1.0, 15.0, normalize=True)
    out = torch.zeros((poses.shape[0], points.shape[0]), dtype=torch.bool, device=dev)
    for w, c in enumerate(counts):
        out[w, kept_idx[w, :c].long()] = True
    return out


def _rows_case(dev, n, W, sort, seed=4):
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(n, seed=seed) if n > 1 else np.float32([[-4.0, 0.3, 0.2]])
    poses, quats = synth.make_path(W, optical=True, jitter_seed=seed)
    points = _t(pts, dev)
    cloud = ops.PackedCloud(points, sort=sort)
    cam = ops.Camera(torch.from_numpy(K), IW, IH, 1.0, 5.0)
    return pts, poses, quats, points, cloud, cam, _t(poses, dev), _t(quats, dev)


def _expected_rows(pts, poses, kept, g, occ, skip=(1, 1)):
    want = kept.clone()
    for w in range(len(poses)):
        idx = np.flatnonzero(kept[w].cpu().numpy())
        a = np.broadcast_to(poses[w], (len(idx), 3))
        want[w, idx] = torch.from_numpy(synth.los_ref(a, pts[idx], g.origin, g.resolution, occ, skip) != 0).to(want.device)
    return want


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("n,W", [(1, 1), (257, 5), (20_000, 1), (20_000, 5)])
def test_rows_equal_kept_and_not_blocked(dev, n, W, sort):
    from trajectory_optimization_amd import ops
    pts, poses, quats, points, cloud, cam, p, q = _rows_case(dev, n, W, sort)
    kept = _kept_masks(points, p, q, cam, dev)
    if n == 1:
        assert kept.all()   # (the one point lies in front of the one camera)
    # an empty grid: exactly cull_waypoints' kept sets
    empty = ops.OccupancyGrid((-25.0, -25.0, -5.0), 0.25, (200, 200, 40), device=dev)
    rows = ops.occlusion_bits(cloud, points, p, q, cam, 1.0, 15.0, method="voxel", grid=empty)
    assert rows.shape == (W, cloud.npad // 32) and rows.dtype == torch.int32
    assert torch.equal(ops.unpack_occlusion_rows(cloud, rows), kept.float())
    # the grid of the cloud: kept and not blocked
    g = ops.OccupancyGrid.from_points(cloud, resolution=0.25)
    occ, _ = synth.occupancy_ref(pts, g.origin, g.resolution, g.dims)
    assert torch.equal(g.dense().cpu(), torch.from_numpy(occ))
    want = _expected_rows(pts, poses, kept, g, occ)
    rows = ops.occlusion_bits(cloud, points, p, q, cam, 1.0, 15.0, method="voxel", grid=g)
    assert torch.equal(ops.unpack_occlusion_rows(cloud, rows), want.float())
    if n == 20_000:
        assert 0 < int(want.sum()) < int(kept.sum())
    # prune on against off, the same call twice, other skips
    assert torch.equal(ops.los_rows(cloud, p, q, cam, 1.0, 15.0, g, prune=False), rows)
    assert torch.equal(ops.los_rows(cloud, p, q, cam, 1.0, 15.0, g), rows)
    rows23 = ops.los_rows(cloud, p, q, cam, 1.0, 15.0, g, skip=(2, 3))
    assert torch.equal(ops.unpack_occlusion_rows(cloud, rows23), _expected_rows(pts, poses, kept, g, occ, (2, 3)).float())
    assert torch.equal(ops.los_rows(cloud, p, q, cam, 1.0, 15.0, g, skip=(2, 3), prune=False), rows23)
    # pad bits are zero
    bits = ((rows[:, :, None] >> torch.arange(32, dtype=torch.int32, device=dev)) & 1).reshape(W, -1)
    assert not bits[:, n:].any() and int(bits.sum()) == int(want.sum())
    # other limits move the kept set, exactly as the cull's
    rows5 = ops.los_rows(cloud, p, q, cam, 2.0, 6.0, empty)
    kept_idx, _, counts, _ = ops.cull_waypoints(points, p, q, cam, 2.0, 6.0, normalize=True)
    assert int(ops.unpack_occlusion_rows(cloud, rows5).sum()) == sum(counts)


def test_rows_with_the_camera_out_of_range_are_the_kept_sets(dev):
    from trajectory_optimization_amd import ops
    pts, poses, quats, points, cloud, cam, p, q = _rows_case(dev, 20_000, 2, True)
    kept = _kept_masks(points, p, q, cam, dev)
    # 5 mm voxels: the range ends 10.24 m below the origin; both cameras lie 11 m below it, many of their points within range
    origin = (float(poses[:, 0].max()) + 11.0, -20.0, -2.0)
    g = _grid_of(np.ones((16, 16, 16), bool), origin, 0.005, dev)
    _, ok = synth.occ_fixed(poses, g.origin, g.resolution)
    assert not ok.any() and synth.occ_fixed(pts, g.origin, g.resolution)[1].sum() > 1000
    rows = ops.occlusion_bits(cloud, points, p, q, cam, 1.0, 15.0, method="voxel", grid=g)
    assert torch.equal(ops.unpack_occlusion_rows(cloud, rows), kept.float()) and kept.any()


def test_rows_of_a_rig_equal_its_virtual_waypoints_one_by_one(dev):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelTraj
    pts = synth.make_cloud(20_000, seed=23)
    poses, quats = synth.make_path(2, optical=True, jitter_seed=23)
    rq, rt = synth.camera_rig(3)
    rt = rt + np.array([[0.1, 0.0, 0.2], [0.0, 0.15, 0.2], [-0.1, 0.0, 0.25]], dtype=np.float32)
    m = ModelTraj(torch.from_numpy(pts), torch.from_numpy(poses), torch.from_numpy(quats), torch.from_numpy(K), IW, IH, device=dev,
                  rig=(rq, rt), occlusion="voxel", occlusion_voxel=0.25)
    g = m._occlusion_grid
    assert isinstance(g, ops.OccupancyGrid) and g.resolution == 0.25
    ps, qs = m.poses.detach().contiguous(), m.quats.detach().contiguous()
    rows = m._build_occlusion_rows(ps, qs)
    assert rows.shape == (6, m._cloud.npad // 32)
    # the six cameras' own poses, by the model's formulas in f32 on the device
    qn = qs / qs.norm(dim=1, keepdim=True).clamp_min(1e-12)
    aw, ax, ay, az = qn[:, None, :].unbind(-1)
    bw, bx, by, bz = m._rig.q[None, :, :].unbind(-1)
    vq = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                      aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1).reshape(-1, 4).contiguous()
    w, x, y, z = qn.unbind(-1)
    R = torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), w * w - x * x + y * y - z * z,
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1).reshape(-1, 3, 3)
    vt = (ps[:, None, :] + torch.einsum("wij,cj->wci", R, m._rig.t)).reshape(-1, 3).contiguous()
    for v in range(6):
        one = ops.occlusion_bits(m._cloud, m.points, vt[v:v + 1].contiguous(), vq[v:v + 1].contiguous(), m._cam, 1.0, 15.0, method="voxel", grid=g)
        assert torch.equal(one[0], rows[v]), v
    assert rows.any() and not torch.equal(rows[0], rows[3])


def test_rows_are_exactly_translation_invariant(dev):
    """Points and poses on the 2^-8 m lattice, voxels of 2^-3 m: shifting points, poses and origin by (8192, -8192, 4096) shifts
    every f32 involved exactly, so the rows must not change in a single bit."""
    from trajectory_optimization_amd import ops
    shift = np.float32([8192.0, -8192.0, 4096.0])
    snap = lambda a: (np.round(a.astype(np.float64) * 256) / 256).astype(np.float32)
    pts = snap(synth.make_cloud(20_000, seed=6))
    poses, quats = synth.make_path(5, optical=True, jitter_seed=6)
    poses = snap(poses)
    cam = ops.Camera(torch.from_numpy(K), IW, IH, 1.0, 5.0)
    out = []
    for s in (np.float32([0, 0, 0]), shift):
        P, T = pts + s, poses + s
        assert np.array_equal((P.astype(np.float64) - s), pts.astype(np.float64))
        points = _t(P, dev)
        cloud = ops.PackedCloud(points)
        g = ops.OccupancyGrid.from_points(cloud, resolution=0.125)
        rows = ops.occlusion_bits(cloud, points, _t(T, dev), _t(quats, dev), cam, 1.0, 15.0, method="voxel", grid=g)
        out.append((ops.unpack_occlusion_rows(cloud, rows), g))
    (a, ga), (b, gb) = out
    assert ga.dims == gb.dims and np.array_equal(gb.origin.astype(np.float64) - ga.origin.astype(np.float64), shift.astype(np.float64))
    assert torch.equal(ga.dense(), gb.dense()) and torch.equal(a, b)
    kept = _kept_masks(_t(pts, dev), _t(poses, dev), _t(quats, dev), cam, dev)
    assert 0 < int(a.sum()) < int(kept.sum())


# ------------------------------------------------------------------------------------------------------------ models

def _traj(dev, pts, poses, quats, **kw):
    from trajectory_optimization_amd.model import ModelTraj
    return ModelTraj(pts, torch.from_numpy(poses), torch.from_numpy(quats), torch.from_numpy(K), IW, IH, device=dev, **kw)


def _pose_model(dev, pts, t, q, **kw):
    from trajectory_optimization_amd.model import ModelPose
    return ModelPose(pts, torch.from_numpy(t), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev, **kw)


def test_unknown_occlusion_still_raises_the_old_message(dev):
    pts = torch.from_numpy(synth.make_cloud(1000, seed=1))
    poses, quats = synth.make_path(3, optical=True)
    for bad in ("bogus", "raycast"):
        with pytest.raises(ValueError, match="^occlusion must be None, 'hpr' or 'zbuffer', or 'voxel'"):
            _traj(dev, pts, poses, quats, occlusion=bad)
        with pytest.raises(ValueError, match="^occlusion must be None, 'hpr' or 'zbuffer', or 'voxel'"):
            _pose_model(dev, pts, poses[:1], quats[:1], occlusion=bad)
    with pytest.raises(ValueError, match="occlusion_grid needs occlusion='voxel'"):
        _traj(dev, pts, poses, quats, occlusion="hpr", occlusion_grid=object())
    with pytest.raises(ValueError, match="needs grid= an OccupancyGrid"):
        _traj(dev, pts, poses, quats, occlusion="voxel", occlusion_grid=object())


def test_model_traj_equals_the_step_given_the_voxel_rows(dev):
    """Three optimiser steps of ModelTraj(occlusion='voxel') against the same model handed, at every refresh, the rows of
    ops.occlusion_bits(method='voxel') over the same grid: loss, rewards and gradients to the bit; and the refresh counts of
    occlusion_refresh_every = 1 and 2."""
    from trajectory_optimization_amd import ops
    pts = torch.from_numpy(synth.make_cloud(60_000, seed=21))
    poses, quats = synth.make_path(5, optical=True, jitter_seed=21)
    m = _traj(dev, pts, poses, quats, occlusion="voxel", occlusion_voxel=0.25)
    g = m._occlusion_grid
    ref = _traj(dev, pts, poses, quats, occlusion="hpr")
    calls = []
    ref._build_occlusion_rows = lambda ps, qs: calls.append(ps.shape[0]) or ops.occlusion_bits(ref._cloud, ref.points, ps, qs, ref._cam, 1.0, 15.0,
                                                                                                method="voxel", grid=g)
    every2 = _traj(dev, pts, poses, quats, occlusion="voxel", occlusion_grid=g, occlusion_refresh_every=2)
    assert every2._occlusion_grid is g
    plain = _traj(dev, pts, poses, quats)
    opts = [torch.optim.Adam([{"params": [x.poses], "lr": 0.1}, {"params": [x.quats], "lr": 0.02}]) for x in (m, ref, every2)]
    for step in range(3):
        for x, opt in zip((m, ref, every2), opts):
            opt.zero_grad()
            x(vis_wps_dist=0.0).backward()
        assert torch.equal(m.loss["vis"], ref.loss["vis"]) and torch.equal(m.rewards, ref.rewards)
        assert torch.equal(m.poses.grad, ref.poses.grad) and torch.equal(m.quats.grad, ref.quats.grad)
        if step == 0:
            plain(vis_wps_dist=0.0)
            assert m.rewards.mean().item() < plain.rewards.mean().item()   # the rows hide something
            assert torch.equal(every2.rewards, m.rewards)
        for opt in opts:
            opt.step()
    assert calls == [5, 5, 5] and m.occlusion_rebuilds == [3, 0] and every2.occlusion_rebuilds == [2, 0]
    # the grid travels through sharing_cloud_of
    other = type(m).sharing_cloud_of(m, torch.from_numpy(poses), torch.from_numpy(quats), occlusion="voxel")
    assert other._occlusion_grid is g and other._cloud is m._cloud


def _starts(B, seed, t, q, spread=0.5):
    """B poses near (t, q): the position moved by up to `spread` metres, the quaternion by a few degrees."""
    rng = np.random.default_rng(seed)
    return [((t + rng.uniform(-spread, spread, (1, 3))).astype(np.float32), (q + 0.05 * rng.standard_normal((1, 4))).astype(np.float32))
            for _ in range(B)]


def test_model_pose_and_the_pose_loops(dev):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses
    pts = torch.from_numpy(synth.make_cloud(20_000, seed=9, extent=(30.0, 30.0, 4.0)))
    poses, quats = synth.make_path(5, optical=True, jitter_seed=9)
    t, q = np.ascontiguousarray(poses[2:3]), np.ascontiguousarray(quats[2:3])
    m = _pose_model(dev, pts, t, q, occlusion="voxel", occlusion_voxel=0.25)
    g = m._occlusion_grid
    ref = _pose_model(dev, pts, t, q, occlusion="hpr")
    ref._build_occlusion_rows = lambda tr, qu: ops.occlusion_bits(ref._cloud, ref.points, tr, qu, ref._cam, 1.0, 15.0, method="voxel", grid=g)
    plain = _pose_model(dev, pts, t, q)
    opts = [torch.optim.Adam([{"params": [x.trans], "lr": 0.05}, {"params": [x.quat], "lr": 0.02}]) for x in (m, ref)]
    for step in range(3):
        losses = []
        for x, opt in zip((m, ref), opts):
            opt.zero_grad()
            loss = x()
            loss.backward()
            losses.append(loss.detach())
        assert torch.equal(losses[0], losses[1]) and torch.equal(m.observations, ref.observations)
        assert torch.equal(m.trans.grad, ref.trans.grad) and torch.equal(m.quat.grad, ref.quat.grad)
        if step == 0:
            plain()
            assert 0 < float(m.observations.detach().sum()) < float(plain.observations.detach().sum())
        for opt in opts:
            opt.step()
    assert m.occlusion_rebuilds == 3
    # every pose of optimize_poses (B = 3) is bitwise its own optimize_pose run; the models share the grid object
    k, steps = 2, 3
    starts = [(t, q)] + _starts(2, seed=31, t=t, q=q)
    m0 = _pose_model(dev, pts, *starts[0], occlusion="voxel", occlusion_grid=g, occlusion_refresh_every=k)
    models = [m0] + [ModelPose.sharing_cloud_of(m0, torch.from_numpy(a), torch.from_numpy(b)) for a, b in starts[1:]]
    assert all(x._occlusion == "voxel" and x._occlusion_grid is g for x in models)
    res = optimize_poses(models, n_opt_steps=steps, lr_pose=0.05, lr_quat=0.02)
    for (a, b), x, r in zip(starts, models, res):
        s = _pose_model(dev, m0._cloud, a, b, occlusion="voxel", occlusion_grid=g, occlusion_refresh_every=k)
        rs = optimize_pose(s, n_opt_steps=steps, lr_pose=0.05, lr_quat=0.02)
        assert torch.equal(x.trans, s.trans) and torch.equal(x.quat, s.quat) and r.losses == rs.losses
        assert torch.equal(x.observations, s.observations) and x.occlusion_rebuilds == s.occlusion_rebuilds == 2
    own = ModelPose.sharing_cloud_of(m0, torch.from_numpy(starts[1][0]), torch.from_numpy(starts[1][1]),
                                     occlusion_grid=ops.OccupancyGrid.from_points(m0._cloud, resolution=0.25))
    with pytest.raises(ValueError, match="must share one occlusion_grid"):
        optimize_poses([m0, own], n_opt_steps=2)


def _wall(x, y0, y1, z0, z1, step=0.05):
    ys, zs = np.arange(y0, y1, step), np.arange(z0, z1, step)
    Y, Z = np.meshgrid(ys, zs, indexing="ij")
    return np.stack([np.full(Y.size, x), Y.ravel(), Z.ravel()], axis=1).astype(np.float32)


def test_a_wall_of_another_cloud_hides_the_models_points(dev):
    """The model's cloud is one wall at x = 4.05; a grid that also holds a narrower wall scanned earlier, at x = 2.05 and absent from
    the model's points, hides the middle of the wall behind it and lowers the mean reward of the three views that face through it
    (the flanks stay visible: a waypoint that sees nothing at all has no normalised reward, with any occlusion method)."""
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.tools import occupancy_grid
    seen, earlier = _wall(4.05, -3.0, 3.0, -1.5, 1.5), _wall(2.05, -0.8, 0.8, -1.5, 1.5)
    poses = np.float32([[0.0, -0.2, 0.0], [0.0, 0.0, 0.0], [0.0, 0.2, 0.0]])
    quats = np.repeat(synth.Q_OPTICAL[None, :].astype(np.float32), 3, axis=0)   # all three look along +x
    pts = torch.from_numpy(seen)
    own = _traj(dev, pts, poses, quats, occlusion="voxel")
    assert own._occlusion_grid.resolution == float(np.float32(0.1))
    both = occupancy_grid(origin=(-1.0, -4.0, -2.0), dims=(80, 80, 40), resolution=0.1, device=dev)
    assert both.insert(own) == 0 and both.insert(_t(earlier, dev)) == 0
    mapped = _traj(dev, pts, poses, quats, occlusion="voxel", occlusion_grid=both)
    empty = occupancy_grid(origin=(-1.0, -4.0, -2.0), dims=(80, 80, 40), resolution=0.1, device=dev)
    nothing = _traj(dev, pts, poses, quats, occlusion="voxel", occlusion_grid=empty)
    for x in (own, nothing, mapped):
        x(vis_wps_dist=0.0)
    # a thin wall does not hide itself (the end's neighbourhood is skipped): its own grid hides what an empty grid hides, nothing
    assert torch.equal(own.rewards, nothing.rewards)
    assert torch.equal(ops.unpack_occlusion_rows(own._cloud, own._occ_cache[0]), ops.unpack_occlusion_rows(own._cloud, nothing._occ_cache[0]))
    assert bool(torch.isfinite(mapped.rewards).all()) and mapped.rewards.mean().item() < own.rewards.mean().item()
    seen_own = ops.unpack_occlusion_rows(own._cloud, own._occ_cache[0])
    seen_mapped = ops.unpack_occlusion_rows(own._cloud, mapped._occ_cache[0])
    assert bool((seen_mapped <= seen_own).all()) and 0 < int(seen_mapped.sum()) < int(seen_own.sum())
    hidden = ((seen_own - seen_mapped).sum(dim=0) > 0).cpu().numpy()   # the points the earlier wall hides from some view: the middle
    assert hidden.any() and np.abs(seen[hidden, 1]).max() < 2.2 and hidden[np.abs(seen[:, 1]) < 1.0].all()


def test_select_views_never_gains_from_a_hidden_wall(dev):
    """Two walls, the far one hidden behind the near one for every candidate; three candidates stand 0.55 m before the near wall —
    inside min_dist, so all they could see is the far wall, through the near one.  With occlusion='voxel' none of them is chosen
    with a positive gain; through an empty grid the far wall is theirs alone and one of them is chosen."""
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.tools import select_views
    near, far, back = _wall(4.05, -3.0, 3.0, -1.5, 1.5), _wall(8.05, -3.0, 3.0, -1.5, 1.5), _wall(-4.05, -3.0, 3.0, -1.5, 1.5)
    pts = _t(np.concatenate([near, far, back]), dev)
    P, Q = synth.candidate_grid([0.0, 3.5], [-1.5, 0.0, 1.5], 0.0, 2)   # headings 0.1 (towards the walls) and pi + 0.1
    assert len(P) == 12
    hidden_only = {(1 * 3 + iy) * 2 + 0 for iy in range(3)}
    cam = dict(intrins=torch.from_numpy(K), img_width=IW, img_height=IH)
    sel = select_views(pts, _t(P, dev), _t(Q, dev), 3, occlusion="voxel", **cam)
    assert sel.n_selected >= 1 and float(sel.gains[0]) > 0
    chosen = {int(c) for c, gain in zip(sel.order.tolist(), sel.gains.tolist()) if gain > 0}
    assert chosen and not (chosen & hidden_only), (sel.order, sel.gains)
    # the rows behind it: through the grid of the cloud those three see nothing at all; through an empty grid they keep the far wall
    cloud, camera = ops.PackedCloud(pts), ops.Camera(torch.from_numpy(K), IW, IH, 1.0, 5.0)
    idx = sorted(hidden_only)
    p, q = _t(P[idx], dev), _t(Q[idx], dev)
    g = ops.OccupancyGrid.from_points(cloud, resolution=0.1)
    assert not ops.occlusion_bits(cloud, pts, p, q, camera, 1.0, 15.0, method="voxel", grid=g).any()
    empty = ops.OccupancyGrid(g.origin, 0.1, g.dims, device=dev)
    kept = ops.unpack_occlusion_rows(cloud, ops.occlusion_bits(cloud, pts, p, q, camera, 1.0, 15.0, method="voxel", grid=empty))
    n_near, n_far = len(near), len(far)
    assert (kept[:, n_near:n_near + n_far].sum(dim=1) > 1000).all() and not kept[:, :n_near].any()
    # a grid handed in is the one walked: with the empty one the three gain from the far wall and, every candidate with a gain being asked for, are chosen
    open_ = select_views(cloud, _t(P, dev), _t(Q, dev), 12, occlusion="voxel", occlusion_grid=empty, **cam)
    assert {int(c) for c, gain in zip(open_.order.tolist(), open_.gains.tolist()) if gain > 0} & hidden_only, (open_.order, open_.gains)
