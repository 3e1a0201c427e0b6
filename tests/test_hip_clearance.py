"""The clearance term (clearance_kernels.hip): the nearest-point query against a numpy brute force, the term's value and gradient,
every ModelTraj path and optimiser loop that carries it, weight 0 = the model without it, and a wall it keeps a path off."""
import numpy as np
import pytest
import torch

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def brute(pts, q, r):
    """numpy restatement of the query: f32, (dx*dx + dy*dy) + dz*dz, finite rows only, d2 < fl(r*r), ties to the lowest row."""
    pts, q = np.asarray(pts, f32), np.asarray(q, f32)
    r2 = f32(r) * f32(r)
    fin = np.isfinite(pts).all(axis=1)
    d_out = np.full(len(q), np.inf, f32)
    i_out = np.full(len(q), -1, np.int32)
    for w, t in enumerate(q):
        if not np.isfinite(t).all():
            continue
        dx, dy, dz = (t[0] - pts[:, 0]).astype(f32), (t[1] - pts[:, 1]).astype(f32), (t[2] - pts[:, 2]).astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((dx * dx + dy * dy) + dz * dz).astype(f32)
        d2 = np.where(fin, d2, np.inf).astype(f32)
        i = int(np.argmin(d2))
        if d2[i] < r2:
            i_out[w], d_out[w] = i, f32(np.sqrt(np.float64(d2[i])))
    return d_out, i_out


def query(pts_or_cloud, q, r, dev):
    from trajectory_optimization_amd import tools
    d, idx = tools.trajectory_clearance(pts_or_cloud, torch.as_tensor(np.asarray(q, f32), device=dev), r)
    return d.cpu().numpy(), idx.cpu().numpy()


def _queries(pts, rng, n_in, n_far):
    """inside the cloud (random), on its surface (at a point), far away."""
    lo, hi = pts.min(0), pts.max(0)
    inside = rng.uniform(lo, hi, (n_in, 3)).astype(f32)
    surface = pts[rng.integers(0, len(pts), 4)] + f32(1e-3)
    far = (hi + 50.0 + rng.uniform(0, 5, (n_far, 3))).astype(f32)
    return np.concatenate([inside, surface, far]).astype(f32)


@pytest.mark.parametrize("n", [1000, 100_000, 1_000_000])
def test_query_equals_brute_force(dev, n):
    rng = np.random.default_rng(n)
    pts = synth.make_cloud(n, seed=5)
    q = _queries(pts, rng, 40 if n < 1_000_000 else 24, 4)
    r = {1000: 2.5, 100_000: 0.8}.get(n, 0.5)   # a few points within r of most queries inside the slab
    d, idx = query(torch.from_numpy(pts).to(dev), q, r, dev)
    d_ref, i_ref = brute(pts, q, r)
    assert np.array_equal(idx, i_ref)
    assert np.array_equal(d.view(np.uint32), d_ref.view(np.uint32))
    assert (idx >= 0).sum() > len(q) // 3 and (idx[-4:] == -1).all()


def test_query_edge_cases(dev):
    """d2 == fl(r*r) is excluded; exact duplicates resolve to the lowest row; a NaN row and an inf row in the tile of the true
    nearest point do not hide it; the same on a sorted and an unsorted pack."""
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(7)
    pts = synth.make_cloud(4096, seed=9)
    r = 0.5
    # 1) a lone point at exactly d2 == r*r (0.25) from a far query
    pts[100] = (100.5, 100.0, 100.0)
    # 2) duplicates: rows 3000 and 200 (and 201) hold the same point, near the query at (60, 60, 60)
    pts[200] = pts[201] = pts[3000] = (60.0, 60.0, 60.0)
    # 3) unsorted pack: tile of 256 rows [512, 768) holds the nearest point of query (70, 70, 70) plus a NaN row and an inf row
    pts[520] = (70.1, 70.0, 70.0)
    pts[530] = (np.nan, 70.0, 70.0)
    pts[540] = (np.inf, 70.0, 70.0)
    pts[541] = (70.0, -np.inf, 70.0)
    # a NaN row in another tile of the sorted pack's nearest point, too
    pts[3500] = (80.0, 80.0, 80.2)
    pts[3501] = (80.0, np.nan, 80.0)
    q = np.array([[100.0, 100.0, 100.0], [60.0, 60.0, 60.1], [70.0, 70.0, 70.0], [80.0, 80.0, 80.0], [np.nan, 0, 0], [0, np.inf, 0]], f32)
    q = np.concatenate([q, _queries(pts[np.isfinite(pts).all(1)], rng, 20, 1)]).astype(f32)
    d_ref, i_ref = brute(pts, q, r)
    assert i_ref[0] == -1 and i_ref[1] == 200 and i_ref[2] == 520 and i_ref[3] == 3500 and i_ref[4] == -1 and i_ref[5] == -1
    t = torch.from_numpy(pts).to(dev)
    for sort in (True, False):
        cloud = ops.PackedCloud(t, sort=sort)
        d, idx = query(cloud, q, r, dev)
        assert np.array_equal(idx, i_ref), sort
        assert np.array_equal(d.view(np.uint32), d_ref.view(np.uint32)), sort
    assert np.isinf(d[[0, 4, 5]]).all()


def test_value_and_gradient(dev):
    """Value and gradient against an f64 restatement given the kernel's idx, and against central differences."""
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(11)
    pts = (rng.uniform(-4, 4, (3000, 3))).astype(f32)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    q = rng.uniform(-4, 4, (64, 3)).astype(f32)
    r, w = 0.7, 1.7
    qt = torch.from_numpy(q).to(dev)
    g = torch.empty((64, 3), dtype=torch.float32, device=dev)
    d, idx, val = ops.clearance(cloud, qt, r, w, grad=g, want_value=True)
    idx = idx.cpu().numpy()
    on = idx >= 0
    assert on.sum() > 10
    t64, x64 = q.astype(np.float64), pts[np.maximum(idx, 0)].astype(np.float64)
    dd = np.linalg.norm(t64 - x64, axis=1)
    v_ref = w * np.sum(np.where(on, (r - dd) ** 2, 0.0))
    g_ref = np.where(on[:, None], -2.0 * w * (r - dd)[:, None] * (t64 - x64) / dd[:, None], 0.0)
    assert abs(float(val) - v_ref) <= 1e-6 * abs(v_ref)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref, rtol=1e-6, atol=1e-6 * np.abs(g_ref).max())
    # accumulate adds to what the rows held
    g2 = torch.ones((64, 3), dtype=torch.float32, device=dev)
    ops.clearance(cloud, qt, r, w, grad=g2, accumulate=True)
    assert torch.equal(g2, torch.ones_like(g2) + g)
    # central differences on the waypoints whose d stays clear of r and whose nearest point stays the same
    h = 1e-3
    gd = g.cpu().numpy().astype(np.float64)
    checked = 0
    for i in np.nonzero(on & (dd < r - 0.05) & (dd > 0.05))[0][:12]:
        for k in range(3):
            vals, ids = [], []
            for s in (1, -1):
                qq = q.copy()
                qq[i, k] += s * h
                _, ii, vv = ops.clearance(cloud, torch.from_numpy(qq).to(dev), r, w, want_value=True)
                vals.append(float(vv))
                ids.append(int(ii[i]))
            if ids[0] != idx[i] or ids[1] != idx[i]:
                continue
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - gd[i, k]) <= 2e-3 * max(1.0, abs(gd[i, k])), (i, k, fd, gd[i, k])
            checked += 1
    assert checked >= 12


def _model(dev, n=90_000, W=23, seed=31, **kw):
    from trajectory_optimization_amd.model import ModelTraj
    pts = torch.from_numpy(synth.make_cloud(n, seed=seed))
    p, q = synth.make_path(W, optical=True, jitter_seed=seed)
    return ModelTraj(pts, torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev, **kw)


CLR = dict(clearance_radius=0.6, clearance_weight=2.0)


def test_model_paths_agree(dev):
    """The fused plan, _TrajLoss (occlusion 'zbuffer') and the op-by-op criterion give the same loss['clearance'] and the same
    gradient of it; the total includes it."""
    from trajectory_optimization_amd.model import ModelTraj

    class OpByOp(ModelTraj):
        def criterion(self, rewards):
            return super().criterion(rewards)

    out = []
    for kind in ("plan", "zbuffer", "ops"):
        kw = dict(CLR, occlusion="zbuffer") if kind == "zbuffer" else dict(CLR)
        m = _model(dev, **kw) if kind != "ops" else None
        if kind == "ops":
            pts = torch.from_numpy(synth.make_cloud(90_000, seed=31))
            p, q = synth.make_path(23, optical=True, jitter_seed=31)
            m = OpByOp(pts, torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev, **CLR)
        loss = m(vis_wps_dist=0.0)
        assert "clearance" in m.loss
        parts = sum(float(m.loss[k]) for k in ("vis", "l2", "length", "smooth", "clearance"))
        assert abs(float(loss) - parts) <= 1e-5 * abs(parts)
        m.loss["clearance"].backward()
        out.append((float(m.loss["clearance"]), m.poses.grad.clone()))
    assert out[0][0] > 0.0
    for v, g in out[1:]:
        assert v == out[0][0]
        assert torch.equal(g, out[0][1])
    assert out[0][1].abs().sum() > 0


def test_backward_equals_the_one_call_step_gradient(dev):
    """loss.backward() after model() gives the one-call step's poses_grad: first without the term (the tolerance that holds there
    is the one asked of the term), then with it."""
    from trajectory_optimization_amd import optimizer as O
    exact = None
    for kw in ({}, CLR):
        a, b = _model(dev, **kw), _model(dev, **kw)
        a(vis_wps_dist=0.0).backward()
        run = O._OptRun([b], 1, 0.05, 0.01, 1e9, 1e9, 0.0, (0.9, 0.999), 1e-8)
        run.run(1)
        torch.cuda.synchronize()
        ga, gb = a.poses.grad, run.pg
        if exact is None:
            exact = torch.equal(ga, gb)
            if not exact:
                np.testing.assert_allclose(ga.cpu().numpy(), gb.cpu().numpy(), rtol=1e-6, atol=1e-7)
        elif exact:
            assert torch.equal(ga, gb)
        else:
            np.testing.assert_allclose(ga.cpu().numpy(), gb.cpu().numpy(), rtol=1e-6, atol=1e-7)
    assert exact, "without the term the fused backward and the one-call step agree to the bit on these inputs"


@pytest.mark.parametrize("vwd,rig", [(0.0, False), (1.1, False), (0.0, True)])
def test_one_call_step_equals_the_split_step(dev, vwd, rig):
    from trajectory_optimization_amd import optimizer as O
    kw = dict(CLR, rig=synth.camera_rig(3)) if rig else dict(CLR)
    runs = []
    for split in (False, True):
        m = _model(dev, **kw)
        args = (m, 7, 0.05, 0.01, 1.003, 0.5, vwd, (0.9, 0.999), 1e-8)
        res = O._optimize_trajectory_split(*args) if split else O.optimize_trajectory(m, *args[1:7])
        runs.append((m, res))
    (ma, ra), (mb, rb) = runs
    assert (ma._wps_step(vwd) > 1) == (vwd > 0.0)
    assert torch.equal(ma.poses.data, mb.poses.data) and torch.equal(ma.quats.data, mb.quats.data)
    assert torch.equal(ma.rewards, mb.rewards)
    assert (ra.steps_taken, ra.stopped, ra.losses) == (rb.steps_taken, rb.stopped, rb.losses)
    for k in ("vis", "l2", "length", "smooth", "clearance"):
        assert float(ma.loss[k]) == float(mb.loss[k])
    assert float(ma.loss["clearance"]) > 0.0


def test_optimize_trajectories_equals_independent_runs(dev):
    from trajectory_optimization_amd import optimizer as O
    from trajectory_optimization_amd.model import ModelTraj
    base = _model(dev, **CLR)
    p0 = base.poses0.cpu().numpy()
    q0 = base.quats0.cpu()

    def make(j):
        p = torch.from_numpy(p0 + np.float32(0.3 * j) * np.array([0.0, 1.0, 0.1], f32))
        return ModelTraj.sharing_cloud_of(base, p, q0, **CLR)
    together = [make(j) for j in range(3)]
    res = O.optimize_trajectories(together, 9, 0.05, 0.01, 1e9, 1e9, 0.0)
    for j in range(3):
        m = make(j)
        r1 = O.optimize_trajectory(m, 9, 0.05, 0.01, 1e9, 1e9, 0.0)
        assert torch.equal(m.poses.data, together[j].poses.data)
        assert r1.losses == res[j].losses
        assert float(m.loss["clearance"]) == float(together[j].loss["clearance"])
    other = make(0)
    other.clearance_weight = 3.0
    with pytest.raises(ValueError):
        O.optimize_trajectories([together[0], other], 1)


def test_weight_zero_is_the_model_without_the_term(dev):
    from trajectory_optimization_amd import optimizer as O
    a, b = _model(dev), _model(dev, clearance_weight=0.0, clearance_radius=0.6)
    la, lb = a(vis_wps_dist=0.0), b(vis_wps_dist=0.0)
    assert "clearance" not in b.loss and "clearance" not in a.loss
    assert float(la) == float(lb) and torch.equal(a.rewards, b.rewards)
    for k in ("vis", "l2", "length", "smooth"):
        assert float(a.loss[k]) == float(b.loss[k])
    la.backward()
    lb.backward()
    assert torch.equal(a.poses.grad, b.poses.grad) and torch.equal(a.quats.grad, b.quats.grad)
    ra = O.optimize_trajectory(a, 5, 0.05, 0.01, 1e9, 1e9, 0.0)
    rb = O.optimize_trajectory(b, 5, 0.05, 0.01, 1e9, 1e9, 0.0)
    assert ra.losses == rb.losses and torch.equal(a.poses.data, b.poses.data)
    assert "clearance" not in b.loss


def _wall_case(dev, weight):
    """A wall of points (the plane y = 0) with a denser block behind it that the cameras face: the path starts 0.1 m in front of
    the wall, where the visibility reward holds it."""
    from trajectory_optimization_amd.model import ModelTraj
    xs, zs = np.arange(-4.0, 14.0, 0.1), np.arange(-2.0, 2.0, 0.1)
    X, Z = np.meshgrid(xs, zs)
    wall = np.stack([X.ravel(), np.zeros(X.size), Z.ravel()], 1)
    rng = np.random.default_rng(3)
    block = rng.uniform((-2.0, 1.5, -1.5), (12.0, 4.0, 1.5), (60_000, 3))
    pts = torch.from_numpy(np.concatenate([wall, block]).astype(f32))
    W = 21
    p = np.stack([np.linspace(0.0, 10.0, W), np.full(W, -0.1), np.zeros(W)], 1).astype(f32)
    q = np.tile(np.array([np.sqrt(0.5), -np.sqrt(0.5), 0.0, 0.0], f32), (W, 1))   # camera z (optical axis) along world +y
    m = ModelTraj(pts, torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev,
                  clearance_radius=1.0, clearance_weight=weight)
    return m


def test_the_term_keeps_the_path_off_a_wall(dev):
    from trajectory_optimization_amd import optimizer as O, tools
    r = 1.0
    ends = []
    for weight in (0.0, 50.0):
        m = _wall_case(dev, weight)
        O.optimize_trajectory(m, 150, 0.02, 0.0, 1e9, 1e9, 0.0)
        d, _ = tools.trajectory_clearance(m, m.poses.data, 10.0)
        ends.append(float(d.min()))
    assert ends[0] < 0.5 * r, ends
    assert ends[1] >= 0.9 * r, ends


@pytest.mark.parametrize("occlusion", [None, "zbuffer"])
def test_single_terms_with_the_term_on(dev, occlusion):
    """Each entry of model.loss alone (vis, l2, length, smooth, clearance) back-propagates through the fused node (_TrajLossPlan,
    or _TrajLoss with occlusion) and gives the gradient the op-by-op criterion gives for it, the term on."""
    from trajectory_optimization_amd.model import ModelTraj
    pts = synth.make_cloud(40_000, seed=6, extent=(20.0, 20.0, 4.0))
    poses, quats = synth.make_path(9, optical=True, jitter_seed=4)
    for term in ("vis", "l2", "length", "smooth", "clearance"):
        grads = []
        for fused in (True, False):
            m = ModelTraj(torch.from_numpy(pts), torch.from_numpy(poses), torch.from_numpy(quats), torch.from_numpy(K), IW, IH, device=dev,
                          occlusion=occlusion, clearance_radius=0.8, clearance_weight=2.0)
            m.fused_loss = fused
            with torch.no_grad():
                m.poses += 0.05 * torch.randn(m.poses.shape, generator=torch.Generator().manual_seed(1)).to(dev)  # l2 > 0
            m(vis_wps_dist=0.0)
            (3.0 * m.loss[term]).backward()
            grads.append((m.poses.grad.clone(), None if m.quats.grad is None else m.quats.grad.clone()))
        (pa, qa), (pb, qb) = grads
        assert float(pa.abs().max()) > 0.0, term
        # as tests/test_hip_models.py::test_fused_loss_terms_are_differentiable: the op-by-op side differentiates arccos in f32
        tol = {"smooth": 5e-4, "clearance": 0.0}.get(term, 1e-4)
        err = float((pa - pb).abs().max() / pb.abs().max())
        assert err <= tol, (term, err)
        if term == "vis":
            assert float((qa - qb).abs().max() / qb.abs().max()) < 1e-5
        else:
            assert qa is None or float(qa.abs().max()) == 0.0


def test_separate_calls_round_the_total_once(dev):
    """_TrajLoss (the node of occlusion-aware and sharded models: separate visibility calls, then the regularisers' kernel) gives
    the fused plan's loss terms and total to the bit: the five-term sum is rounded once on both."""
    from trajectory_optimization_amd.model import _TrajLoss
    a, b = _model(dev, **CLR), _model(dev, **CLR)
    la = a(vis_wps_dist=0.0)
    lb, _, *terms_b = _TrajLoss.apply(b.poses, b.quats, b, 1)
    terms_a = [a.loss[k] for k in ("vis", "l2", "length", "smooth", "clearance")]
    assert [float(t) for t in terms_a] == [float(t) for t in terms_b]
    assert float(la) == float(lb)


def test_settings_follow_the_attributes(dev):
    """clearance_weight / clearance_radius are the live settings: weight 0 after construction is the model without the term, a
    weight set on a model built without it is the model built with it; bad values raise."""
    a, b = _model(dev, **CLR), _model(dev)
    a(vis_wps_dist=0.0)
    a.clearance_weight = 0.0
    b0 = _model(dev)
    la, lb0 = a(vis_wps_dist=0.0), b0(vis_wps_dist=0.0)
    assert "clearance" not in a.loss and float(la) == float(lb0)
    b.set_clearance(CLR["clearance_radius"], CLR["clearance_weight"])
    c = _model(dev, **CLR)
    lb, lc = b(vis_wps_dist=0.0), c(vis_wps_dist=0.0)
    assert float(b.loss["clearance"]) == float(c.loss["clearance"]) > 0.0 and float(lb) == float(lc)
    with pytest.raises(ValueError):
        b.clearance_weight = -1.0
    with pytest.raises(ValueError):
        b0.set_clearance(None, 1.0)
    assert b.clearance_weight == CLR["clearance_weight"] and b0.clearance_weight == 0.0
