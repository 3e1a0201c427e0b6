"""ModelPose(occlusion='hpr'|'zbuffer'): each pose hides the points its own camera does not see (the per-camera pipeline of
/root/reference/src/pc_processor.py:158-187, as ModelTraj's rows), read by the pose kernels as one bit row per pose."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_inf
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bundled():
    return load_golden("bundled")["pts"]


def _pose(seed, i=2):
    poses, quats = synth.make_path(5, optical=True, jitter_seed=seed)
    return np.ascontiguousarray(poses[i:i + 1]), np.ascontiguousarray(quats[i:i + 1])


def _model(points, t0, q0, dev, **kw):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelPose
    return ModelPose(points if isinstance(points, ops.PackedCloud) else torch.as_tensor(points),
                     torch.from_numpy(np.ascontiguousarray(t0, np.float32)), torch.from_numpy(np.ascontiguousarray(q0, np.float32)),
                     torch.from_numpy(K), IW, IH, device=dev, **kw)


def _quat(rng):
    q = rng.standard_normal(4).astype(np.float32)
    q /= np.linalg.norm(q)
    return q[None, :] * (1.0 if q[0] >= 0 else -1.0)


def _starts(B, seed, centre=(6.0, 2.0, 0.0), spread=1.0):
    rng = np.random.default_rng(seed)
    return [((np.float32(centre) + rng.uniform(-spread, spread, 3).astype(np.float32))[None, :], _quat(rng)) for _ in range(B)]


def _used_row(m):
    """The (N,) float mask of the row the model's last forward used, in the caller's order."""
    from trajectory_optimization_amd import ops
    return ops.unpack_occlusion_rows(m._cloud, m._occ_cache[0])[0]


# ---------------------------------------------------------------------------------------------------------- 1, 2: the oracle

@pytest.mark.parametrize("seed", [3, 17])
def test_rows_equal_the_oracle(dev, seed):
    from oracle import oracle
    pts = synth.make_cloud(60_000, seed)
    t, q = _pose(seed)
    m = _model(pts, t, q, dev, occlusion="hpr")
    m()
    row = _used_row(m).cpu().numpy()
    ref = oracle.occlusion_masks(pts, t, q, K, IW, IH, 1.0, 15.0)[0]
    assert np.array_equal(row, ref)
    hidden = int((ref == 0).sum())
    assert 0 < hidden < len(ref)
    # not every kept point is hidden: the pose sees some of the cloud
    cam = oracle.to_camera_frame(pts, q[0], t[0], normalize=True)
    d, f = oracle.frustum_masks(np.ascontiguousarray(cam.T), K, IW, IH, 1.0, 15.0)
    assert hidden < int((d & f).sum())


@pytest.mark.parametrize("method", ["hpr", "zbuffer"])
def test_values_against_the_oracle(dev, method):
    from oracle import oracle
    pts = synth.make_cloud(60_000, 5)
    t, q = _pose(5, 1)
    m = _model(pts, t, q, dev, occlusion=method)
    loss = m()
    loss.backward()
    row = _used_row(m).cpu().numpy()
    assert (row == 0).any()
    obs, ref_loss = oracle.pose_forward(pts, t, q, K, IW, IH, mask=row, prec="f64")
    tg, qg = oracle.pose_backward(pts, t, q, K, IW, IH, ref_loss, mask=row, prec="f64")
    assert abs(loss.item() - ref_loss) <= 1e-5 * ref_loss
    np.testing.assert_allclose(m.observations.detach().cpu().numpy(), obs, rtol=5e-5, atol=1e-9)
    assert rel_inf(m.trans.grad.cpu().numpy(), tg) < 1e-5 and rel_inf(m.quat.grad.cpu().numpy(), qg) < 1e-5
    # occlusion only removes observations
    m0 = _model(pts, t, q, dev)
    assert m0().item() <= loss.item()


# ---------------------------------------------------------------------------------------------------------- 3: bits == float mask

@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 100_003])
def test_bit_rows_equal_the_float_mask_bitwise(dev, n):
    """Every bit-row call equals the float-mask call given the unpacked row, to the bit (random rows with random pad bits: pads carry
    no weight either way); the multi call with B distinct rows equals B single float-mask calls."""
    from trajectory_optimization_amd import ops
    pts = torch.from_numpy(synth.make_cloud(n, seed=n % 97) * np.float32(0.25)).to(dev)   # a 10 x 10 x 1 m slab: most points in view
    cloud = ops.PackedCloud(pts, sort=False)
    cam = ops.Camera(torch.from_numpy(K), IW, IH, 1.0, 5.0)
    g = torch.Generator().manual_seed(n)
    B = 5
    rows = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, cloud.npad // 32), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
    masks = ops.unpack_occlusion_rows(cloud, rows)
    starts = _starts(B, seed=n, centre=(0.0, 0.0, 0.0), spread=0.5)
    trans = torch.from_numpy(np.concatenate([s[0] for s in starts])).to(dev).contiguous()
    quat = torch.from_numpy(np.concatenate([s[1] for s in starts])).to(dev).contiguous()
    ws = ops.PoseWorkspace(cloud)
    grad_obs = torch.rand(n, generator=g).to(dev)
    gout = torch.full((1,), 0.75, device=dev)
    single = []
    for b in range(B):
        t, q, row, mask = trans[b:b + 1], quat[b:b + 1], rows[b:b + 1], masks[b].contiguous()
        o1, s1 = ops.pose_forward(cloud, t, q, cam, ws, occ=row)
        o2, s2 = ops.pose_forward(cloud, t, q, cam, ws, mask=mask)
        assert torch.equal(o1, o2) and torch.equal(s1, s2)
        a = ops.pose_forward_backward(cloud, t, q, cam, ws, occ=row, gout=gout)
        c = ops.pose_forward_backward(cloud, t, q, cam, ws, mask=mask, gout=gout)
        assert all(torch.equal(x, y) for x, y in zip(a, c))
        assert torch.equal(a[0], o2)
        for kw in (dict(grad_obs=grad_obs), dict(scalars=s2, gout=gout)):
            x = ops.pose_backward(cloud, t, q, cam, ws, occ=row, **kw)
            y = ops.pose_backward(cloud, t, q, cam, ws, mask=mask, **kw)
            assert all(torch.equal(u, v) for u, v in zip(x, y))
        single.append(ops.pose_forward_backward(cloud, t, q, cam, ws, mask=mask))
    wsm = ops.PoseWorkspace(cloud, B)
    obs, sc, tg, qg = ops.pose_forward_backward_multi(cloud, trans, quat, cam, wsm, observations=True, occ=rows)
    for b, (o, s, t_, q_) in enumerate(single):
        assert torch.equal(obs[b], o) and torch.equal(sc[b], s) and torch.equal(tg[b], t_[0]) and torch.equal(qg[b], q_[0])
    obs_f, sc_f, _, _ = ops.pose_forward_backward_multi(cloud, trans, quat, cam, wsm, observations=True, grad=False, occ=rows)
    assert torch.equal(obs_f, obs) and torch.equal(sc_f, sc)
    if n > 1:   # the weights really come from the rows
        assert not torch.equal(obs[0], ops.pose_forward(cloud, trans[:1], quat[:1], cam, ws)[0])


# ---------------------------------------------------------------------------------------------------------- 4: autograd paths

@pytest.mark.parametrize("method", ["hpr", "zbuffer"])
def test_autograd_paths_agree(dev, bundled, method):
    """With occlusion on: the fused node's calling-thread backward == its backward through the engine, bit for bit; the
    observations node + torch criterion (fused_loss=False) reads the same row (observations bitwise) and gives the same loss and
    gradient within the bars of the no-occlusion case; a loss built on the observations honours the row too."""
    from trajectory_optimization_amd import ops
    t, q = _starts(1, seed=103)[0]   # a view of the bundled cloud with 15 k points in the frustum, most of them hidden
    out = []
    for fused, fast in ((True, True), (True, False), (False, False)):
        m = _model(bundled, t, q, dev, occlusion=method)
        m.fused_loss, m.fast_backward = fused, fast
        loss = m()
        assert loss.grad_fn.__class__.__name__.startswith("_PoseLoss") == fused
        loss.backward()
        out.append((loss.detach().clone(), m.trans.grad.clone(), m.quat.grad.clone(), m.observations.detach().clone(), _used_row(m)))
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[1]))
    assert torch.equal(out[2][3], out[0][3]) and torch.equal(out[2][4], out[0][4])
    assert (out[0][4] == 0).any()
    assert abs(out[2][0].item() - out[0][0].item()) <= 2e-6 * abs(out[0][0].item())
    assert rel_inf(out[2][1].cpu().numpy(), out[0][1].cpu().numpy()) < 1e-5 and rel_inf(out[2][2].cpu().numpy(), out[0][2].cpu().numpy()) < 1e-5
    # a custom loss on the observations: the general dL/d observations pass, with the row, == the float-mask call
    m = _model(bundled, t, q, dev, occlusion=method)
    loss = m()
    w = torch.linspace(0.0, 2.0, m.observations.numel(), device=dev)
    (5.0 * loss + 1e-4 * (w * m.observations).sum()).backward()
    g = (1e-4 * w - 5.0 * loss.detach() * loss.detach()).contiguous()
    tg, qg = ops.pose_backward(m._cloud, m.trans.detach(), m.quat.detach(), m._cam, m._ws, mask=_used_row(m).contiguous(), grad_obs=g)
    assert torch.equal(m.trans.grad, tg) and torch.equal(m.quat.grad, qg)


# ---------------------------------------------------------------------------------------------------------- 5: refresh policy

def test_refresh_policy(dev, bundled):
    t, q = _starts(1, seed=103)[0]   # a view of the bundled cloud with 15 k points in the frustum, most of them hidden
    m = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=3)
    opt = torch.optim.Adam([{"params": [m.trans], "lr": 0.2}, {"params": [m.quat], "lr": 0.05}])
    seen = []
    for _ in range(7):
        opt.zero_grad()
        m().backward()
        opt.step()
        seen.append(m._occ_cache[0])
    same = [seen[i] is seen[i + 1] for i in range(6)]
    assert same == [True, True, False, True, True, False]
    assert m.occlusion_rebuilds == 3
    m.refresh_occlusion()
    m()
    assert m.occlusion_rebuilds == 4 and m._occ_cache[0] is not seen[6]
    m()
    assert m.occlusion_rebuilds == 4
    # k = 1 at the first forward is a fresh model's forward, to the bit
    a = _model(bundled, t, q, dev, occlusion="hpr")
    b = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=1)
    la, lb = a(), b()
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.observations, b.observations) and torch.equal(a.trans.grad, b.trans.grad)
    assert a.occlusion_rebuilds == b.occlusion_rebuilds == 1
    # occlusion=None changes nothing
    c, d = _model(bundled, t, q, dev), _model(bundled, t, q, dev, occlusion=None)
    assert torch.equal(c(), d()) and torch.equal(c.observations, d.observations) and c.occlusion_rebuilds == 0


# ---------------------------------------------------------------------------------------------------------- 6, 7: the loops

@pytest.mark.parametrize("k", [1, 3])
def test_optimize_pose_follows_the_dropin_loop(dev, bundled, k):
    """The launch-only loop against `loss = m(); loss.backward(); torch.optim.Adam.step()`.  The Adam step is the library's update
    (accelerate_torch_adam on this optimiser: the same arithmetic as optimize_pose's), so both loops hold the same pose at every
    refresh: torch's own Adam differs from it by an ulp or so, and an ulp in the pose can move a point across the hull's boundary —
    a row rebuilt from it then differs in a few bits (measured: 6e-4 of the loss after six steps at k = 1)."""
    from trajectory_optimization_amd.optimizer import accelerate_torch_adam, optimize_pose
    t, q = _starts(1, seed=103)[0]   # a view of the bundled cloud with 15 k points in the frustum, most of them hidden
    m1 = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=k)
    m2 = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=k)
    res = optimize_pose(m1, n_opt_steps=7, lr_pose=0.05, lr_quat=0.02)
    opt = accelerate_torch_adam(torch.optim.Adam([{"params": [m2.trans], "lr": 0.05}, {"params": [m2.quat], "lr": 0.02}]))
    ref = []
    for _ in range(7):
        opt.zero_grad()
        loss = m2()
        loss.backward()
        opt.step()
        ref.append(loss.item())
    assert m2.occlusion_rebuilds == (7 + k - 1) // k
    np.testing.assert_allclose(res.losses, ref, rtol=1e-5)
    np.testing.assert_allclose(m1.trans.detach().cpu().numpy(), m2.trans.detach().cpu().numpy(), atol=1e-5)
    np.testing.assert_allclose(m1.quat.detach().cpu().numpy(), m2.quat.detach().cpu().numpy(), atol=1e-5)
    # the loop leaves the model's row cache as its seven forwards would: same rebuild count, and the next forward (a rebuild at
    # k = 1, the last row reused at k = 3) gives what the drop-in model's gives
    assert m1.occlusion_rebuilds == m2.occlusion_rebuilds
    l1, l2 = m1(), m2()
    assert m1.occlusion_rebuilds == m2.occlusion_rebuilds
    np.testing.assert_allclose(l1.item(), l2.item(), rtol=1e-5)
    # the rows matter: the same run without occlusion goes elsewhere
    m3 = _model(bundled, t, q, dev)
    assert optimize_pose(m3, n_opt_steps=7, lr_pose=0.05, lr_quat=0.02).losses != res.losses


@pytest.mark.parametrize("k,steps", [(3, 3), (10, 7)])
def test_optimize_pose_follows_torch_adam_while_the_row_stays(dev, bundled, k, steps):
    """The issue's comparison with torch.optim.Adam itself, where the row is built once, at the start pose both loops share (the
    refreshes after it are compared above with the library's Adam update)."""
    from trajectory_optimization_amd.optimizer import optimize_pose
    t, q = _starts(1, seed=103)[0]
    m1 = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=k)
    m2 = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=k)
    res = optimize_pose(m1, n_opt_steps=steps, lr_pose=0.05, lr_quat=0.02)
    opt = torch.optim.Adam([{"params": [m2.trans], "lr": 0.05}, {"params": [m2.quat], "lr": 0.02}])
    ref = []
    for _ in range(steps):
        opt.zero_grad()
        loss = m2()
        loss.backward()
        opt.step()
        ref.append(loss.item())
    assert m1.occlusion_rebuilds == m2.occlusion_rebuilds == 1
    np.testing.assert_allclose(res.losses, ref, rtol=1e-5)
    np.testing.assert_allclose(m1.trans.detach().cpu().numpy(), m2.trans.detach().cpu().numpy(), atol=1e-5)
    np.testing.assert_allclose(m1.quat.detach().cpu().numpy(), m2.quat.detach().cpu().numpy(), atol=1e-5)


def test_loops_leave_the_row_cache_coherent(dev, bundled):
    """m(); optimize_pose(m) with k = 10 over 10 steps; m() is a fresh model's forward at the final pose (the row the cache held
    from before the loop is not reused).  Over 7 steps the next forward reuses the loop's last row, as a model's 8th forward would."""
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses
    t, q = _starts(1, seed=103)[0]

    def fresh_at(m):
        f = _model(bundled, m.trans.detach().cpu().numpy(), m.quat.detach().cpu().numpy(), dev, occlusion="hpr", occlusion_refresh_every=10)
        return f(), f

    m = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=10)
    m()
    optimize_pose(m, n_opt_steps=10, lr_pose=0.05, lr_quat=0.02)
    assert m.occlusion_rebuilds == 2
    loss = m()
    assert m.occlusion_rebuilds == 3
    fl, f = fresh_at(m)
    assert torch.equal(loss, fl) and torch.equal(m.observations, f.observations) and torch.equal(_used_row(m), _used_row(f))
    m = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=10)
    m()
    optimize_pose(m, n_opt_steps=7, lr_pose=0.05, lr_quat=0.02)
    kept = m._occ_cache[0]
    m()
    assert m.occlusion_rebuilds == 2 and m._occ_cache[0] is kept and m._occ_cache[1] == 8
    # optimize_poses: each model's own last row and age
    starts = _starts(3, seed=7)
    m0 = _model(bundled, *starts[0], dev, occlusion="hpr", occlusion_refresh_every=10)
    models = [m0] + [ModelPose.sharing_cloud_of(m0, torch.from_numpy(a), torch.from_numpy(b)) for a, b in starts[1:]]
    for x in models:
        x()
    optimize_poses(models, n_opt_steps=10, lr_pose=0.05, lr_quat=0.02)
    for x in models:
        assert x.occlusion_rebuilds == 2
        loss = x()
        fl, f = fresh_at(x)
        assert torch.equal(loss, fl) and torch.equal(x.observations, f.observations) and torch.equal(_used_row(x), _used_row(f))


@pytest.mark.parametrize("B", [3, 64])
def test_optimize_poses_is_bitwise_the_single_runs(dev, bundled, B, monkeypatch):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses
    k, steps = 3, 7
    starts = _starts(B, seed=100 + B)
    m0 = _model(bundled, *starts[0], dev, occlusion="hpr", occlusion_refresh_every=k)
    models = [m0] + [ModelPose.sharing_cloud_of(m0, torch.from_numpy(t), torch.from_numpy(q)) for t, q in starts[1:]]
    assert all(m._occlusion == "hpr" and m.occlusion_refresh_every == k for m in models)
    widths = []
    real = ops.occlusion_bits
    monkeypatch.setattr(ops, "occlusion_bits", lambda cloud, points, poses, *a, **kw: widths.append(poses.shape[0]) or real(cloud, points, poses, *a, **kw))
    res = optimize_poses(models, n_opt_steps=steps, lr_pose=0.05, lr_quat=0.02)
    assert widths == [B] * ((steps + k - 1) // k)   # one batched hull pass per refresh step
    monkeypatch.setattr(ops, "occlusion_bits", real)
    for (t, q), m, r in zip(starts, models, res):
        s = _model(bundled, t, q, dev, occlusion="hpr", occlusion_refresh_every=k)
        rs = optimize_pose(s, n_opt_steps=steps, lr_pose=0.05, lr_quat=0.02)
        assert torch.equal(m.trans, s.trans) and torch.equal(m.quat, s.quat)
        assert r.losses == rs.losses
        assert torch.equal(m.observations, s.observations)


# ---------------------------------------------------------------------------------------------------------- 8: errors

def test_errors(dev, bundled):
    from trajectory_optimization_amd import _lib, ops
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses
    t, q = _starts(1, seed=103)[0]   # a view of the bundled cloud with 15 k points in the frustum, most of them hidden
    with pytest.raises(ValueError):
        _model(bundled, t, q, dev, occlusion="raytrace")
    m = _model(bundled, t, q, dev, occlusion="hpr")
    with pytest.raises(ValueError):
        m(hpr=True)
    with pytest.raises(ValueError):
        optimize_pose(m, n_opt_steps=2, hpr=True)
    other = ModelPose.sharing_cloud_of(m, torch.from_numpy(t + 0.5), torch.from_numpy(q))
    with pytest.raises(ValueError):
        optimize_poses([m, other], n_opt_steps=2, hpr=True)
    for kw in (dict(occlusion=None), dict(occlusion="zbuffer"), dict(occlusion_limits=(1.0, 10.0)), dict(occlusion_refresh_every=2)):
        bad = ModelPose.sharing_cloud_of(m, torch.from_numpy(t + 0.5), torch.from_numpy(q), **kw)
        with pytest.raises(ValueError):
            optimize_poses([m, bad], n_opt_steps=2)
    assert m.occlusion_rebuilds == 0   # nothing ran
    # a float mask and bit rows together at the C ABI: the invalid-argument code, before any launch
    L = _lib.lib()
    cloud, B = m._cloud, 2
    f32 = dict(dtype=torch.float32, device=dev)
    trans, quat = torch.zeros((B, 3), **f32), torch.tensor([[1.0, 0, 0, 0]] * B, **f32)
    bufs = [torch.zeros((B, 4), **f32) for _ in range(6)]
    losses = torch.zeros((B, 2), **f32)
    mask = torch.ones(cloud.n, **f32)
    rows = torch.zeros((B, cloud.npad // 32), dtype=torch.int32, device=dev)
    ws = ops.PoseWorkspace(cloud, B)
    c = _lib.PoseOpt()
    c.packed, c.n_points, c.n_poses, c.n_steps, c.cam = cloud.blob.data_ptr(), cloud.n, B, 2, m._cam.c
    c.trans, c.quat = trans.data_ptr(), quat.data_ptr()
    c.exp_avg_t, c.exp_avg_sq_t, c.exp_avg_q, c.exp_avg_sq_q, c.scalars, c.trans_grad = (b.data_ptr() for b in bufs)
    c.quat_grad, c.loss_log = None, losses.data_ptr()
    c.workspace, c.workspace_bytes = ws.buf.data_ptr(), ws.bytes
    c.occlusion_mask, c.occlusion_bits = mask.data_ptr(), rows.data_ptr()
    assert L.tohip_pose_opt_step_multi(ctypes.byref(c), 1, None, None) == -1
    torch.cuda.synchronize(dev)
    assert torch.equal(trans, torch.zeros_like(trans))   # untouched
    with pytest.raises(ValueError):
        ops.pose_forward_backward_multi(cloud, trans, quat, m._cam, ws, mask=mask, occ=rows)
    # the single-pose wrappers refuse the same
    row, t1, q1 = rows[:1], trans[:1].contiguous(), quat[:1].contiguous()
    ws1 = ops.PoseWorkspace(cloud)
    for call in (lambda: ops.pose_forward(cloud, t1, q1, m._cam, ws1, mask=mask, occ=row),
                 lambda: ops.pose_forward_backward(cloud, t1, q1, m._cam, ws1, mask=mask, occ=row),
                 lambda: ops.pose_backward(cloud, t1, q1, m._cam, ws1, mask=mask, occ=row, grad_obs=mask)):
        with pytest.raises(ValueError):
            call()
    # the bit-row twins refuse a missing row (NULL is not "nothing occluded" there: that is the float calls' job)
    obs1, sc1, g1 = torch.empty(cloud.n, **f32), torch.empty(4, **f32), torch.empty(8, **f32)
    assert L.tohip_pose_forward_backward_bits(cloud.blob.data_ptr(), cloud.n, t1.data_ptr(), q1.data_ptr(), m._cam.ref(), None, obs1.data_ptr(),
                                              sc1.data_ptr(), None, g1.data_ptr(), g1.data_ptr() + 16, ws1.buf.data_ptr(), ws1.bytes,
                                              None) == -1
    scB = torch.empty((B, 4), **f32)
    assert L.tohip_pose_forward_backward_multi_bits(cloud.blob.data_ptr(), cloud.n, trans.data_ptr(), quat.data_ptr(), B, m._cam.ref(), None,
                                                    None, scB.data_ptr(), None, bufs[0].data_ptr(), bufs[1].data_ptr(), ws.buf.data_ptr(),
                                                    ws.bytes, None) == -1
