"""The clearance term asked of the map (clearance_map_kernels.hip): the map query against the cloud query over the exported centres —
bit for bit — and against the numpy restatement (clearance_map_cases.py); unknown as obstacle; windows beyond one pass; every
ModelTraj path and optimiser loop with clearance_map=; TOHIP_TRAJ_CLEARANCE_PREFILLED at the C ABI; and a map that changes between
two steps of one model."""
import numpy as np
import pytest
import torch

import clearance_map_cases as cases
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
f32 = np.float32
W_TERM = 1.5   # the term's weight in the queries below


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    """A float tensor or array as integers: equality of these is equality to the bit, NaN included."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def make_grid(dev, vox, dims=cases.DIMS, res=cases.RES, origin=cases.ORIGIN):
    from trajectory_optimization_amd import ops
    g = ops.OccupancyGrid(origin, res, dims, device=dev)
    if len(vox):
        assert g.insert(torch.from_numpy(cases.centres(vox, origin, res)).to(dev)) == 0
    return g


def exported(grid):
    """The grid's set voxels in ascending linear index -> (lin (n,) int64 array, C (n,3) f32 device tensor)."""
    ijk, centres = grid.export()
    lin = cases.linear(ijk.cpu().numpy(), grid.dims)
    order = np.argsort(lin)
    return lin[order], centres[torch.from_numpy(order).to(centres.device)].contiguous()


def run_points(source, q, r, dev, w=W_TERM):
    from trajectory_optimization_amd import ops
    q = torch.as_tensor(np.asarray(q, f32), device=dev)
    grad = torch.full((q.shape[0], 3), 7.0, device=dev)
    terms = torch.full((max(q.shape[0], 32),), -1.0, dtype=torch.float64, device=dev)
    d, idx, value = ops.clearance(source, q, r, w, grad=grad, want_value=True, terms=terms)
    return dict(d=d.cpu().numpy(), idx=idx.cpu().numpy(), value=value.cpu().numpy(), grad=grad.cpu().numpy(), term=terms[:q.shape[0]].cpu().numpy())


def run_segments(source, poses, r, dev, n_traj, w=W_TERM):
    from trajectory_optimization_amd import ops
    q = torch.as_tensor(np.asarray(poses, f32), device=dev)
    grad = torch.full((q.shape[0], 3), 7.0, device=dev)
    terms = ops.clearance_terms(q.shape[0] // n_traj, n_traj, "segments", dev).fill_(-1.0)
    d, idx, s, value = ops.clearance_segments(source, q, r, w, n_traj=n_traj, grad=grad, want_value=True, terms=terms)
    return dict(d=d.cpu().numpy(), idx=idx.cpu().numpy(), s=s.cpu().numpy(), value=value.cpu().numpy(), grad=grad.cpu().numpy(),
                term=terms[:q.shape[0]].cpu().numpy())


def assert_same_query(got_map, got_cloud, ref, lin, what):
    """The map query, the cloud query over the centres in ascending linear index, and the restatement: d, s, terms, value and gradient
    rows to the bit; idx through lin."""
    for key in got_map:
        if key == "idx":
            ic = got_cloud["idx"]
            assert np.array_equal(got_map["idx"], np.where(ic >= 0, lin[np.maximum(ic, 0)], -1)), (what, key)
            assert np.array_equal(got_map["idx"], ref["idx"]), (what, key, got_map["idx"], ref["idx"])
        else:
            assert same(got_map[key], got_cloud[key]), (what, key, got_map[key], got_cloud[key])
            assert same(got_map[key], np.asarray(ref[key]).reshape(got_map[key].shape)), (what, key, got_map[key], ref[key])


# ---- 1. the map query equals the cloud query and the restatement -------------------------------------------------------------------

@pytest.fixture(scope="module")
def case1(dev):
    from trajectory_optimization_amd import ops
    vox = cases.case1_voxels()
    grid = make_grid(dev, vox)
    lin, C = exported(grid)
    lin_ref, C_ref = cases.obstacles(cases.dense(vox))
    assert np.array_equal(lin, lin_ref) and same(C, C_ref)   # the restatement's centres are export's, bit for bit
    return dict(grid=grid, lin=lin, C=C_ref, points=C, cloud=ops.PackedCloud(C), source=ops.MapObstacles(grid))


@pytest.mark.parametrize("r", cases.RADII)
def test_point_query_equals_the_cloud_query(dev, case1, r):
    names, q = cases.case1_points(r)
    lin, C = case1["lin"], case1["C"]
    got = run_points(case1["source"], q, r, dev)
    assert_same_query(got, run_points(case1["cloud"], q, r, dev), cases.query_points(lin, C, q, r, W_TERM), lin, r)
    at = {n: i for i, n in enumerate(names)}
    own = at["own centre"]
    assert got["d"][own] == 0.0 and got["idx"][own] == cases.linear([(6, 9, 2)])[0] and not got["grad"][own].any()
    assert got["term"][own] == float(f32(r)) ** 2
    for n in ("1e6", "1e30", "nan", "inf"):
        assert got["idx"][at[n]] == -1 and got["d"][at[n]] == np.inf and not got["grad"][at[n]].any() and got["term"][at[n]] == 0.0
    if r >= 0.25:
        assert got["idx"][at["outside dims"]] == cases.linear([cases.BOUNDARY])[0]   # 0.08 m beyond the far x face
        assert got["idx"][at["corner"]] == cases.linear([cases.BLOCK])[0] and got["idx"][at["face"]] == cases.linear([cases.BLOCK])[0]
    if r == 0.04:
        assert got["idx"][at["exactly r"]] == -1   # strict '<': the lone voxel's centre at exactly r is not a hit


@pytest.mark.parametrize("r", cases.RADII)
def test_segment_query_equals_the_cloud_query(dev, case1, r):
    lin, C = case1["lin"], case1["C"]
    for k, poses in enumerate(cases.case1_paths(r)):
        got = run_segments(case1["source"], poses, r, dev, 2)
        assert_same_query(got, run_segments(case1["cloud"], poses, r, dev, 2), cases.query_segments(lin, C, poses, r, W_TERM, 2), lin, (r, k))
        if k == 0:
            # the degenerate segment D -> D is the point query at D, bit for bit; D and E straddle the lone voxel and no segment joins them
            pt = run_points(case1["source"], poses[2:3], r, dev)
            assert same(got["d"][2:3], pt["d"]) and got["idx"][2] == pt["idx"][0] and same(got["term"][2:3], pt["term"])
            lone = cases.linear([cases.LONE])[0]
            assert got["idx"][2] != lone   # (D is farther than r from it, and so is E)
            joined = run_segments(case1["source"], np.stack([poses[3], poses[4]]), r, dev, 1)
            assert joined["d"][0] < 1e-6 and (joined["idx"][0] == lone or r > 0.25)   # (at r = 1 it also runs through the block's row)
        else:
            assert got["idx"][2] == -1 and got["d"][2] == np.inf and not got["grad"][3].any()   # the segment that ends in the NaN row


# ---- 2. unknown as obstacle ----------------------------------------------------------------------------------------------------------

def test_unknown_as_obstacle(dev):
    from trajectory_optimization_amd import ops
    vox = cases.case1_voxels()
    space = ops.SpaceMap(make_grid(dev, vox))
    pocket = np.array([(x, y, z) for x in range(5, 10) for y in range(4, 9) for z in range(1, 5)])
    free = make_grid(dev, pocket)   # a carved pocket, as a plane
    space.free.buf.copy_(free.buf)
    occ, fre = cases.dense(vox), cases.dense(pocket)
    lin, C = cases.obstacles(occ, fre)
    assert len(lin) == 13 * 10 * 7 - int((fre & ~occ).sum())   # states 0 and 2
    cloud = ops.PackedCloud(torch.from_numpy(C).to(dev))
    source = ops.MapObstacles(space, "obstacle")
    q = np.array([(0.95, 0.2, 0.33), (0.98, 0.25, 0.31), (0.76, 0.04, 0.2), (1.55, 0.6, 0.78), (0.22, -0.42, 0.06)], f32)
    for r in (0.15, 0.3):
        got = run_points(source, q, r, dev)
        assert_same_query(got, run_points(cloud, q, r, dev), cases.query_points(lin, C, q, r, W_TERM), lin, r)
        assert (got["idx"][2:] >= 0).all()
    poses = np.concatenate([q[:4], q[1:5]])
    got = run_segments(source, poses, 0.2, dev, 2)
    assert_same_query(got, run_segments(cloud, poses, 0.2, dev, 2), cases.query_segments(lin, C, poses, 0.2, W_TERM, 2), lin, "segments")
    # unknown='free' over the same space: only the occupied voxels
    got = run_points(ops.MapObstacles(space), q, 0.3, dev)
    assert_same_query(got, run_points(ops.PackedCloud(torch.from_numpy(cases.obstacles(occ)[1]).to(dev)), q, 0.3, dev),
                      cases.query_points(*cases.obstacles(occ), q, 0.3, W_TERM), cases.obstacles(occ)[0], "free")
    # every voxel inside dims free: queries hugging the three far faces find nothing — the complement bits of the partial bricks
    # beyond dims do not count; over an all-unknown space the same queries hit
    o, far = np.asarray(cases.ORIGIN, f32), np.asarray(cases.ORIGIN, f32) + f32(cases.RES) * np.asarray(cases.DIMS, f32)
    hug = np.array([(far[0] + 0.03, 0.1, 0.3), (0.8, far[1] + 0.03, 0.3), (0.8, 0.1, far[2] + 0.03), far + f32(0.02), (far[0] - 0.01, far[1] - 0.01, far[2] + 0.04)], f32)
    empty = ops.SpaceMap(make_grid(dev, []))
    everything = np.argwhere(np.ones(cases.DIMS, bool))
    empty.free.buf.copy_(make_grid(dev, everything).buf)
    all_free = run_points(ops.MapObstacles(empty, "obstacle"), hug, 0.25, dev)
    assert (all_free["idx"] == -1).all() and np.isinf(all_free["d"]).all() and not all_free["grad"].any()
    seg_free = run_segments(ops.MapObstacles(empty, "obstacle"), hug[:4], 0.25, dev, 1)
    assert (seg_free["idx"] == -1).all()
    unknown = ops.MapObstacles(ops.SpaceMap(make_grid(dev, [])), "obstacle")
    lin_all, C_all = cases.obstacles(np.zeros(cases.DIMS, bool), np.zeros(cases.DIMS, bool))
    got = run_points(unknown, hug, 0.25, dev)
    assert (got["idx"] >= 0).all()
    assert_same_query(got, run_points(ops.PackedCloud(torch.from_numpy(C_all).to(dev)), hug, 0.25, dev),
                      cases.query_points(lin_all, C_all, hug, 0.25, W_TERM), lin_all, "all unknown")
    with pytest.raises(ValueError, match="unknown='obstacle' needs"):
        ops.MapObstacles(space.occupied, "obstacle")


# ---- 3. windows beyond one pass -------------------------------------------------------------------------------------------------------

def test_windows_beyond_one_pass(dev):
    """80 x 40 x 30 voxels, r = 1 m.  A 4 m leg along x: its window is more than 16 x 64 words, so every wave of the block loops and
    the radius shrinks between passes; a point query whose window is more than 64 words, so the lanes stride.  One obstacle in the
    first word of each window and one in the last, obstacles at several distances in between."""
    from trajectory_optimization_amd import ops
    dims, res, origin, r = (80, 40, 30), 0.1, (-0.37, 0.12, -0.05), 1.0
    a, b = np.array([1.6, 2.1, 1.45], f32), np.array([5.6, 2.1, 1.45], f32)
    t = np.array([3.1, 1.9, 1.5], f32)
    vox = set()
    for lo, hi in ((np.minimum(a, b), np.maximum(a, b)), (t, t)):
        win = cases.window(lo, hi, r, origin, res, dims)
        words = win[0][1] * win[1][1] * win[2][1]
        assert words > (16 * 64 if lo is not t else 64), win
        first = (4 * win[0][0], 4 * win[1][0], 2 * win[2][0])
        last = tuple(min(p * (w0 + n) - 1, d - 1) for p, (w0, n), d in zip((4, 4, 2), win, dims))
        vox |= {first, last}
    # along the leg, nearer and nearer as z (the slowest axis of the window) grows: the best distance improves pass after pass
    for k, (x, z) in enumerate(((20, 6), (34, 9), (48, 12), (27, 14), (55, 16), (41, 19), (30, 22))):
        vox.add((x, 20 - (6 - k), z))
    vox |= {(x, y, 15) for x in (10, 70) for y in (5, 35)}
    vox = np.array(sorted(vox))
    grid = make_grid(dev, vox, dims, res, origin)
    lin, pts = exported(grid)
    lin_ref, C = cases.obstacles(cases.dense(vox, dims), origin=origin, res=res)
    assert np.array_equal(lin, lin_ref) and same(pts, C)
    cloud, source = ops.PackedCloud(pts), ops.MapObstacles(grid)
    poses = np.stack([a, b, t, t + f32(0.3), b, a, a + f32(0.2), t])
    got = run_segments(source, poses, r, dev, 2)
    assert_same_query(got, run_segments(cloud, poses, r, dev, 2), cases.query_segments(lin, C, poses, r, W_TERM, 2), lin, "leg")
    assert got["idx"][0] >= 0 and got["idx"][0] == got["idx"][3]   # a -> b and b -> a
    q = np.stack([t, a, b, (a + b) * f32(0.5)])
    got = run_points(source, q, r, dev)
    assert_same_query(got, run_points(cloud, q, r, dev), cases.query_points(lin, C, q, r, W_TERM), lin, "point")
    assert got["idx"][0] >= 0


# ---- 4. every model path, bit for bit -------------------------------------------------------------------------------------------------

CLR = dict(clearance_radius=0.25, clearance_weight=2.0)
TERMS = ("vis", "l2", "length", "smooth", "clearance")
RUN = (5, 0.02, 0.01, 1e9, 1e9, 0.0)


def _path(j=0):
    """Eight waypoints through case 1's grid."""
    s = np.linspace(0.0, 1.0, 8, dtype=f32)[:, None]
    p = (np.array([0.3, -0.3, 0.3], f32) + s * np.array([1.1, 0.8, 0.2], f32) + f32(0.04 * j) * np.array([0.0, 1.0, 0.5], f32)).astype(f32)
    p[:, 2] += (0.05 * np.sin(7.0 * s[:, 0])).astype(f32)
    return torch.from_numpy(p), torch.from_numpy(synth.make_path(8, optical=True, jitter_seed=3)[1])


def _model(dev, points, j=0, cls=None, **kw):
    from trajectory_optimization_amd.model import ModelTraj
    p, q = _path(j)
    return (cls or ModelTraj)(points, p, q, torch.from_numpy(K), IW, IH, min_dist=0.2, device=dev, **kw)


@pytest.mark.parametrize("mode", ["waypoints", "segments"])
def test_every_model_path_equals_the_cloud_term(dev, case1, mode):
    """The cloud is C, the centres of the grid's voxels: the cloud term and the map term have the same obstacles, so every path gives
    the same bits."""
    from trajectory_optimization_amd import optimizer as O
    from trajectory_optimization_amd.model import ModelTraj

    class OpByOp(ModelTraj):
        def criterion(self, rewards):
            return super().criterion(rewards)

    pts, grid = case1["points"], case1["grid"]
    kw = dict(CLR, clearance_mode=mode)
    pair = lambda **k: (_model(dev, pts, **dict(kw, **k)), _model(dev, pts, clearance_map=grid, **dict(kw, **k)))   # noqa: E731
    # model() and backward(); the op-by-op criterion
    for cls in (None, OpByOp):
        a, b = pair(cls=cls)
        la, lb = a(vis_wps_dist=0.0), b(vis_wps_dist=0.0)
        assert same(la, lb) and all(same(a.loss[k], b.loss[k]) for k in TERMS) and float(b.loss["clearance"].detach()) > 0.0
        la.backward(), lb.backward()
        assert same(a.poses.grad, b.poses.grad) and same(a.quats.grad, b.quats.grad) and a.poses.grad.abs().sum() > 0
    a, b = pair()
    a(vis_wps_dist=0.0), b(vis_wps_dist=0.0)
    a.loss["clearance"].backward(), b.loss["clearance"].backward()
    assert same(a.poses.grad, b.poses.grad) and a.poses.grad.abs().sum() > 0
    # optimize_trajectory
    a, b = pair()
    ra, rb = O.optimize_trajectory(a, *RUN), O.optimize_trajectory(b, *RUN)
    assert ra.steps_taken == rb.steps_taken == 5 and same(np.array(ra.losses), np.array(rb.losses))
    assert same(a.poses.data, b.poses.data) and same(a.quats.data, b.quats.data) and same(a.rewards, b.rewards)
    assert all(same(a.loss[k], b.loss[k]) for k in TERMS) and float(b.loss["clearance"]) > 0.0
    # optimize_trajectories, B = 2, and optimize_team of 2
    for fn in (O.optimize_trajectories, O.optimize_team):
        A = [_model(dev, pts, j=j, **kw) for j in range(2)]
        first = _model(dev, pts, j=0, clearance_map=grid, **kw)
        p1, q1 = _path(1)
        Bm = [first, ModelTraj.sharing_cloud_of(first, p1, q1, min_dist=0.2, **kw)]
        assert Bm[1].clearance_map is grid
        ra, rb = fn(A, *RUN), fn(Bm, *RUN)
        for ma, mb in zip(A, Bm):
            assert same(ma.poses.data, mb.poses.data) and same(ma.quats.data, mb.quats.data)
            assert all(same(ma.loss[k], mb.loss[k]) for k in TERMS) and float(mb.loss["clearance"]) > 0.0
        if fn is O.optimize_team:
            assert same(ra.loss_log, rb.loss_log) and same(ra.poses_grad, rb.poses_grad) and same(np.array(ra.losses), np.array(rb.losses))
        else:
            assert all(same(np.array(x.losses), np.array(y.losses)) for x, y in zip(ra, rb))
    with pytest.raises(ValueError, match="clearance_map"):   # members must share the map objects
        O.optimize_team([_model(dev, pts, clearance_map=grid, **kw), _model(dev, pts, clearance_map=make_grid(dev, cases.case1_voxels()), **kw)], 1)
    with pytest.raises(ValueError, match="clearance_map"):
        O.optimize_trajectories([_model(dev, pts, clearance_map=grid, **kw), _model(dev, pts, **kw)], 1)


@pytest.mark.parametrize("mode", ["waypoints", "segments"])
def test_the_map_repels_where_the_cloud_is_elsewhere(dev, case1, mode):
    """The visibility cloud is a wall two metres away; the map holds a pillar beside the path."""
    from trajectory_optimization_amd import tools
    rng = np.random.default_rng(5)
    wall = torch.from_numpy((np.array([3.0, -1.0, 0.0]) + rng.random((500, 3)) * np.array([0.05, 2.0, 1.0])).astype(f32)).to(dev)
    pillar = make_grid(dev, [(6, 4, z) for z in range(7)])
    kw = dict(CLR, clearance_mode=mode)
    m = _model(dev, wall, clearance_map=pillar, **kw)
    m(vis_wps_dist=0.0)
    out = tools.trajectory_clearance(pillar, m.poses.data, CLR["clearance_radius"], segments=mode == "segments")
    d, idx = out[0], out[1]
    assert (idx >= 0).any()
    value = CLR["clearance_weight"] * float(((float(f32(CLR["clearance_radius"])) - d[idx >= 0].double()) ** 2).sum())
    # (d is the f64 distance rounded to f32, 6e-8 relative: 1e-5 of the value is two orders above what that can move the sum by)
    got = float(m.loss["clearance"].detach())
    assert got > 0.0 and abs(got - value) <= 1e-5 * value
    plain = _model(dev, wall, **kw)
    plain(vis_wps_dist=0.0)
    assert float(plain.loss["clearance"].detach()) == 0.0
    m.set_clearance_map(None)
    m(vis_wps_dist=0.0)
    assert float(m.loss["clearance"].detach()) == 0.0 and m.clearance_map is None


# ---- 5. TOHIP_TRAJ_CLEARANCE_PREFILLED at the C ABI -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["waypoints", "segments"])
def test_prefilled_step_equals_the_step_that_asks_itself(dev, case1, mode):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd import optimizer as O
    pts = case1["points"]

    def step(prefill, **kw):
        models = [_model(dev, pts, j=j, clearance_mode=mode, **kw) for j in range(2)]
        run = O._OptRun(models, 1, 0.02, 0.01, 1e9, 1e9, 0.0, (0.9, 0.999), 1e-8)
        if prefill:
            run.c.flags |= ops.CLEARANCE_PREFILLED
            if run.clearance:   # tohip_clearance / tohip_clearance_segments into the plan's scratch, on the step's stream
                m0 = models[0]
                ops.clearance_rows(m0._cloud, run.poses, m0.clearance_radius, m0.clearance_weight, mode, 2,
                                   *ops.clearance_scratch_views(run.clr_scratch, run.poses.shape[0]))
        run.run(1)
        torch.cuda.synchronize()
        return [run.poses, run.quats, run.pg, run.qg, run.lo_sum, run.minmax, run.rewards, run.scalars, run.loss_log, run.state_log, *run.moments]
    for kw in (CLR, {}):   # with the term; and with weight 0, where the bit is accepted and does nothing
        asks, prefilled = step(False, **kw), step(True, **kw)
        assert all(same(x, y) for x, y in zip(asks, prefilled))
        assert bool((asks[8][:, 0, 5] > 0).all()) == bool(kw)


# ---- 6. the map is read live ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["waypoints", "segments"])
def test_the_model_sees_the_map_change_between_two_steps(dev, mode):
    from trajectory_optimization_amd import optimizer as O
    from trajectory_optimization_amd.tools import evidence_map, occupancy_grid
    S = synth.EVID_SCENE
    scanner = torch.tensor(S["scanner"], device=dev)
    room = synth.box_room(step=S["step"])
    with_pillar = torch.from_numpy(synth.pillar_scan(room, S["scanner"], *S["pillar"])).to(dev)
    room = torch.from_numpy(room).to(dev)
    m = evidence_map(occupancy_grid(origin=S["origin"], dims=S["dims"], resolution=S["resolution"], device=dev))
    for _ in range(2):
        m.integrate(scanner, with_pillar)
    # eight waypoints 0.2 m in front of the pillar's face (x = 1.0), half a metre from the floor, the ceiling and every wall
    p = torch.tensor([[0.8, 0.65 + 0.1 * k, 0.5] for k in range(8)])
    q = torch.from_numpy(synth.make_path(8, optical=True)[1])
    from trajectory_optimization_amd.model import ModelTraj
    model = ModelTraj(room, p, q, torch.from_numpy(K), IW, IH, device=dev, clearance_radius=0.3, clearance_weight=2.0,
                      clearance_mode=mode, clearance_map=m)
    model(vis_wps_dist=0.0)
    assert float(model.loss["clearance"].detach()) > 0.0
    face = torch.tensor([[x, y, 0.45] for x in (0.95, 1.05) for y in (0.85, 1.0, 1.15)], device=dev)   # either side of x = 1.0
    assert bool((m.log_odds(face)[1] == 2).any())
    dropped = None
    for k in range(8):   # the sample's eight scans of the empty room: hit 17 twice, miss 8 — the pillar's voxels go after five
        m.integrate(scanner, room)
        if dropped is None and not bool((m.log_odds(face)[1] == 2).any()):
            dropped = k + 1
    assert dropped is not None and 1 <= dropped <= 8
    loss = model(vis_wps_dist=0.0)   # the same model object: no set_clearance_map, no re-pack
    assert float(model.loss["clearance"].detach()) == 0.0
    loss.backward()
    O.optimize_trajectory(model, 1, 0.01, 0.0, 1e9, 1e9, 0.0)
    assert float(model.loss["clearance"].detach()) == 0.0
    m.occupied.insert(torch.tensor([[0.85, 1.0, 0.5]], device=dev))
    model(vis_wps_dist=0.0)
    assert float(model.loss["clearance"].detach()) > 0.0
    O.optimize_trajectory(model, 1, 0.01, 0.0, 1e9, 1e9, 0.0)
    assert float(model.loss["clearance"].detach()) > 0.0
