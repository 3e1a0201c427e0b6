"""Many poses of one camera over one cloud at once (optimizer.optimize_poses, ops.pose_forward_backward_multi): every pose of a
batch must end bit for bit where its own single-pose run ends."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_inf
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


def _quat(rng):
    q = rng.standard_normal(4).astype(np.float32)
    q /= np.linalg.norm(q)
    return q[None, :] * (1.0 if q[0] >= 0 else -1.0)


def _starts(B, seed, centre=(6.0, 2.0, 0.0), spread=1.0):
    rng = np.random.default_rng(seed)
    return [((np.float32(centre) + rng.uniform(-spread, spread, 3).astype(np.float32))[None, :], _quat(rng)) for _ in range(B)]


def _model(points, t0, q0, dev, **kw):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelPose
    return ModelPose(points=points if isinstance(points, ops.PackedCloud) else torch.as_tensor(points), trans0=torch.from_numpy(np.ascontiguousarray(t0, np.float32)),
                     q0=torch.from_numpy(np.ascontiguousarray(q0, np.float32)), intrins=torch.from_numpy(K), img_width=IW,
                     img_height=IH, device=dev, **kw)


def _batch_vs_single(points, starts, dev, steps, **kw):
    """optimize_poses over models sharing one cloud vs a fresh optimize_pose run per start: everything bitwise."""
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses
    m0 = _model(points, *starts[0], dev)
    models = [m0] + [ModelPose.sharing_cloud_of(m0, torch.from_numpy(t), torch.from_numpy(q)) for t, q in starts[1:]]
    res = optimize_poses(models, n_opt_steps=steps, **kw)
    assert len(res) == len(models)
    for (t, q), m, r in zip(starts, models, res):
        s = _model(points, t, q, dev)
        rs = optimize_pose(s, n_opt_steps=steps, **kw)
        assert torch.equal(m.trans, s.trans) and torch.equal(m.quat, s.quat)
        assert r.losses == rs.losses
        assert torch.equal(m.observations, s.observations)
    return models, res


@pytest.mark.parametrize("B", [1, 3, 64, 257])
def test_batch_is_bitwise_the_single_runs(dev, bundled, B):
    _batch_vs_single(bundled, _starts(B, seed=B), dev, 10)


def test_batch_with_hpr_builds_the_mask_once(dev, bundled, monkeypatch):
    from trajectory_optimization_amd import model as model_mod
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses
    starts = _starts(8, seed=8)
    m0 = _model(bundled, *starts[0], dev)
    models = [m0] + [ModelPose.sharing_cloud_of(m0, torch.from_numpy(t), torch.from_numpy(q)) for t, q in starts[1:]]
    calls = []
    real = model_mod.hidden_pts_removal
    monkeypatch.setattr(model_mod, "hidden_pts_removal", lambda *a, **k: calls.append(1) or real(*a, **k))
    res = optimize_poses(models, n_opt_steps=10, lr_pose=0.05, lr_quat=0.02, hpr=True)
    assert len(calls) == 1
    monkeypatch.setattr(model_mod, "hidden_pts_removal", real)
    for (t, q), m, r in zip(starts, models, res):
        s = _model(bundled, t, q, dev)
        rs = optimize_pose(s, n_opt_steps=10, lr_pose=0.05, lr_quat=0.02, hpr=True)
        assert torch.equal(m.trans, s.trans) and torch.equal(m.quat, s.quat)
        assert r.losses == rs.losses and torch.equal(m.observations, s.observations)


def test_striding_blocks(dev):
    """1.5 M points: 733 chunks of 2048 points exceed the resident grid (2 blocks x 256 CUs), so blocks stride over chunks."""
    pts = synth.make_cloud(1_500_000, seed=5)
    _batch_vs_single(pts, _starts(8, seed=15, centre=(0.0, 0.0, 0.0), spread=5.0), dev, 3)


@pytest.mark.parametrize("n", [1, 7, 2047, 2049, 40_960])
def test_cloud_sizes_at_tile_edges(dev, n):
    pts = synth.make_cloud(n, seed=n, extent=(6.0, 6.0, 6.0))
    _batch_vs_single(pts, _starts(5, seed=n, centre=(0.0, 0.0, -3.0), spread=0.5), dev, 10)


def test_reference_fixtures_inside_a_batch(dev, bundled):
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses
    d = load_golden("pose_adam_bundled")
    lr = dict(lr_pose=float(d["lr_pose"]), lr_quat=float(d["lr_quat"]))
    starts = _starts(15, seed=77)
    starts.insert(6, (d["trans0"], d["q0"]))
    for steps in (1, 5, 10):
        m0 = _model(bundled, *starts[0], dev)
        models = [m0] + [ModelPose.sharing_cloud_of(m0, torch.from_numpy(t), torch.from_numpy(q)) for t, q in starts[1:]]
        res = optimize_poses(models, n_opt_steps=steps, **lr)
        m = models[6]
        np.testing.assert_allclose(m.trans.detach().cpu().numpy(), d[f"trans_step{steps}"], rtol=0, atol=1e-3)
        np.testing.assert_allclose(m.quat.detach().cpu().numpy(), d[f"quat_step{steps}"], rtol=0, atol=1e-3)
        np.testing.assert_allclose(res[6].losses, d["losses"][:steps], rtol=1e-3)

    z = load_golden("pose_sees_nothing")
    starts = [(z["trans0"], z["q0"])] + [(np.float32([[30.7 + dx, 3.0 + dy, 0.0]]), np.float32([[1.0, 0.0, 0.0, 0.0]]) + np.float32([[0, dq, -dq, 0]]))
                                          for dx, dy, dq in ((0.0, 0.0, 0.0), (0.3, -0.2, 0.05), (-0.4, 0.3, -0.08))]
    models, res = _batch_vs_single(z["points"], starts, dev, 10)
    loss0 = float(z["loss"])
    assert all(abs(x - loss0) <= 1e-6 * loss0 for x in res[0].losses)
    assert all(r.losses[0] < 1e-2 * loss0 for r in res[1:])   # the neighbours see the cloud


def _pose_set(B, seed):
    rng = np.random.default_rng(seed)
    t = np.stack([np.float32([rng.uniform(-12, 12), rng.uniform(-12, 12), rng.uniform(-1.5, 1.5)]) for _ in range(B)])
    q = np.concatenate([_quat(rng) for _ in range(B)])
    return t, q


@pytest.mark.parametrize("masked", [False, True])
def test_ops_multi_matches_single_and_oracle(dev, masked):
    from oracle import oracle
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(100_000, seed=21)
    t_np, q_np = _pose_set(16, seed=22)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=False)
    cam = ops.Camera(torch.from_numpy(K), IW, IH, 1.0, 5.0, 1e-6)
    mask_np = (np.random.default_rng(23).random(len(pts)) < 0.7).astype(np.float32) if masked else None
    mask = torch.from_numpy(mask_np).to(dev) if masked else None
    t, q = torch.from_numpy(t_np).to(dev), torch.from_numpy(q_np).to(dev)
    ws = ops.PoseWorkspace(cloud, 16)
    obs, sc, tg, qg = ops.pose_forward_backward_multi(cloud, t, q, cam, ws, mask=mask, observations=True)
    obs_f, sc_f, tg_f, qg_f = ops.pose_forward_backward_multi(cloud, t, q, cam, ws, mask=mask, observations=True, grad=False)
    assert tg_f is None and qg_f is None
    assert torch.equal(sc_f, sc) and torch.equal(obs_f, obs)
    ws1 = ops.PoseWorkspace(cloud)
    for b in range(16):
        o1, s1, tg1, qg1 = ops.pose_forward_backward(cloud, t[b:b + 1].contiguous(), q[b:b + 1].contiguous(), cam, ws1, mask=mask)
        assert torch.equal(obs[b], o1) and torch.equal(sc[b], s1)
        assert torch.equal(tg[b:b + 1], tg1) and torch.equal(qg[b:b + 1], qg1)
        of, lf = oracle.pose_forward(pts, t_np[b], q_np[b], K, IW, IH, mask=mask_np, prec="f64")
        assert rel_inf(obs[b].cpu().numpy(), of) < 1e-5
        assert abs(float(sc[b, 1]) - lf) <= 1e-5 * lf
        tr, qr = oracle.pose_backward(pts, t_np[b], q_np[b], K, IW, IH, lf, mask=mask_np, prec="f64")
        for g, r in ((tg[b:b + 1], tr), (qg[b:b + 1], qr)):
            g = g.cpu().numpy()
            if np.abs(r).max() > 1e-20:
                assert rel_inf(g, r) < 1e-5, (b, g, r)
            else:
                assert np.abs(g).max() <= 1e-20


@pytest.mark.parametrize("n", [7, 2049])
@pytest.mark.parametrize("case", ["sorted", "bits"])
def test_ops_multi_sorted_cloud_and_bit_rows(dev, n, case):
    """What the cases above leave to other files: a cloud packed with sort=True (observations and the float mask go through the
    permutation) and each pose's own occlusion bit row, at B = 3 (a full tile and a short one).  n = 7 is less than one lane's
    eight points; n = 2049 is one chunk and one point, so the second chunk is nearly all pads."""
    from oracle import oracle
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(n, seed=n % 97) * np.float32(0.25)   # a 10 x 10 x 1 m slab: most points in view
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=case == "sorted")
    cam = ops.Camera(torch.from_numpy(K), IW, IH, 1.0, 5.0, 1e-6)
    B = 3
    g = torch.Generator().manual_seed(n)
    if case == "sorted":
        masks = (torch.rand(n, generator=g) < 0.7).to(torch.float32).to(dev).expand(B, n)
        kw = [dict(mask=masks[0].contiguous())] * B
        kw_multi = kw[0]
    else:   # random rows with random pad bits
        rows = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, cloud.npad // 32), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
        masks = ops.unpack_occlusion_rows(cloud, rows)
        kw = [dict(occ=rows[b:b + 1]) for b in range(B)]
        kw_multi = dict(occ=rows)
    starts = _starts(B, seed=n, centre=(0.0, 0.0, 0.0), spread=0.5)
    t_np, q_np = np.concatenate([s[0] for s in starts]), np.concatenate([s[1] for s in starts])
    t, q = torch.from_numpy(t_np).to(dev), torch.from_numpy(q_np).to(dev)
    obs, sc, tg, qg = ops.pose_forward_backward_multi(cloud, t, q, cam, ops.PoseWorkspace(cloud, B), observations=True, **kw_multi)
    ws1 = ops.PoseWorkspace(cloud)
    for b in range(B):
        o1, s1, tg1, qg1 = ops.pose_forward_backward(cloud, t[b:b + 1].contiguous(), q[b:b + 1].contiguous(), cam, ws1, **kw[b])
        assert torch.equal(obs[b], o1) and torch.equal(sc[b], s1)
        assert torch.equal(tg[b:b + 1], tg1) and torch.equal(qg[b:b + 1], qg1)
        mask_np = masks[b].cpu().numpy()
        of, lf = oracle.pose_forward(pts, t_np[b], q_np[b], K, IW, IH, mask=mask_np, prec="f64")
        assert rel_inf(obs[b].cpu().numpy(), of) < 1e-5
        assert abs(float(sc[b, 1]) - lf) <= 1e-5 * lf
        tr, qr = oracle.pose_backward(pts, t_np[b], q_np[b], K, IW, IH, lf, mask=mask_np, prec="f64")
        for gr, r in ((tg[b:b + 1], tr), (qg[b:b + 1], qr)):
            gr = gr.cpu().numpy()
            if np.abs(r).max() > 1e-20:
                assert rel_inf(gr, r) < 1e-5, (b, gr, r)
            else:
                assert np.abs(gr).max() <= 1e-20


def test_opt_step_writes_observations_only_when_asked(dev):
    import ctypes
    from trajectory_optimization_amd import _lib, ops
    pts = synth.make_cloud(5000, seed=31, extent=(6.0, 6.0, 6.0))
    B, steps = 6, 3
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=False)
    cam = ops.Camera(torch.from_numpy(K), IW, IH, 1.0, 5.0, 1e-6)
    t_np, q_np = _pose_set(B, seed=32)
    f32 = dict(dtype=torch.float32, device=dev)
    trans, quat = torch.from_numpy(t_np).to(dev), torch.from_numpy(q_np).to(dev)
    moments = [torch.zeros((B, 3), **f32), torch.zeros((B, 3), **f32), torch.zeros((B, 4), **f32), torch.zeros((B, 4), **f32)]
    scalars, losses = torch.zeros((B, 4), **f32), torch.zeros((B, steps), **f32)
    ws = ops.PoseWorkspace(cloud, B)
    c = _lib.PoseOpt()
    c.packed, c.n_points, c.n_poses, c.n_steps, c.cam = cloud.blob.data_ptr(), cloud.n, B, steps, cam.c
    c.trans, c.quat = trans.data_ptr(), quat.data_ptr()
    c.lr_pose, c.lr_quat, c.beta1, c.beta2, c.adam_eps = 0.1, 0.1, 0.9, 0.999, 1e-8
    c.exp_avg_t, c.exp_avg_sq_t, c.exp_avg_q, c.exp_avg_sq_q = (m.data_ptr() for m in moments)
    c.scalars, c.loss_log = scalars.data_ptr(), losses.data_ptr()
    c.workspace, c.workspace_bytes = ws.buf.data_ptr(), ws.bytes
    sentinel = -12345.0
    obs = torch.full((B, cloud.n), sentinel, **f32)
    L = _lib.lib()
    with torch.cuda.device(dev):
        for s in (1, 2):
            _lib.check(L.tohip_pose_opt_step_multi(ctypes.byref(c), s, None, _lib.stream_ptr()), "step")
        torch.cuda.synchronize()
        assert bool((obs == sentinel).all())
        _lib.check(L.tohip_pose_opt_step_multi(ctypes.byref(c), 3, ctypes.c_void_p(obs.data_ptr()), _lib.stream_ptr()), "step")
        torch.cuda.synchronize()
    assert not bool((obs == sentinel).any())
    assert bool(((obs >= 0) & (obs <= 1)).all())


def test_model_pose_sharing_a_cloud(dev, bundled):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelPose
    (t0, q0), (t1, q1) = _starts(2, seed=41)
    own = _model(bundled, t1, q1, dev)
    base = _model(bundled, t0, q0, dev)
    shared = ModelPose.sharing_cloud_of(base, torch.from_numpy(t1), torch.from_numpy(q1))
    named = _model(bundled, t1, q1, dev, cloud=base)
    packed = _model(base._cloud, t1, q1, dev)
    for m in (shared, named, packed):
        assert m._cloud is base._cloud and m.points.data_ptr() == base.points.data_ptr()
    for m in (own, shared, named, packed):
        loss = m()
        loss.backward()
    for m in (shared, named, packed):
        assert torch.equal(m.observations, own.observations)
        assert torch.equal(m.trans.grad, own.trans.grad) and torch.equal(m.quat.grad, own.quat.grad)
    with pytest.raises(ValueError):
        _model(bundled, t1, q1, dev, cloud=ops.PackedCloud(torch.from_numpy(bundled).to(dev), sort=True))
    other = bundled.copy()
    other[5, 1] += 1.0
    with pytest.raises(ValueError):
        _model(other, t1, q1, dev, cloud=base)


def test_optimize_poses_refuses_mismatched_models(dev, bundled):
    from trajectory_optimization_amd.optimizer import optimize_poses
    (t0, q0), (t1, q1) = _starts(2, seed=51)
    a = _model(bundled, t0, q0, dev)
    other = bundled.copy()
    other[0, 0] += 0.5
    K2 = K.copy()
    K2[0, 0] *= 1.01
    from trajectory_optimization_amd.model import ModelPose
    bad = [_model(other, t1, q1, dev),
           ModelPose(torch.from_numpy(bundled), torch.from_numpy(t1), torch.from_numpy(q1), torch.from_numpy(K2), IW, IH, device=dev),
           ModelPose(torch.from_numpy(bundled), torch.from_numpy(t1), torch.from_numpy(q1), torch.from_numpy(K), IW + 2, IH, device=dev),
           _model(bundled, t1, q1, dev, min_dist=0.5),
           _model(bundled, t1, q1, dev, max_dist=6.0)]
    eps = _model(bundled, t1, q1, dev)
    eps.eps = 1e-5
    bad.append(eps)
    for b in bad:
        with pytest.raises(ValueError):
            optimize_poses([a, b], n_opt_steps=2)
    with pytest.raises(ValueError):
        optimize_poses([], n_opt_steps=2)
    ms = [_model(bundled, t, q, dev) for t, q in _starts(3, seed=52)]
    before = [(m.trans.detach().clone(), m.quat.detach().clone()) for m in ms]
    assert optimize_poses(ms, n_opt_steps=0) == []
    for m, (t, q) in zip(ms, before):
        assert torch.equal(m.trans, t) and torch.equal(m.quat, q) and m.observations is None


def test_multistart_example(dev, bundled, tmp_path):
    from trajectory_optimization_amd.optimizer import optimize_pose
    sys.path.insert(0, os.path.join(REPO, "examples"))
    from pose_optimization_sample import random_quaternion
    out = tmp_path / "multi.npz"
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "pose_multistart_sample.py"), "--starts", "8", "--opt-steps", "30",
                        "--out", str(out)], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    d = np.load(out)
    assert d["final_losses"].shape == (8,)
    s = _model(bundled, np.float32([[6.0, 2.0, 0.0]]), random_quaternion(0).numpy(), dev)
    res = optimize_pose(s, n_opt_steps=30, lr_pose=0.1, lr_quat=0.1)
    assert float(d["final_losses"][0]) == res.losses[-1]
    best = int(np.argmin(d["final_losses"]))
    assert int(d["best_start"]) == best
    np.testing.assert_array_equal(d["trans"], d["all_trans"][best:best + 1])
    assert d["losses"].shape == (30,) and float(d["losses"][-1]) == float(d["final_losses"][best])


def test_multi_workspace_and_argument_checks(dev, bundled):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_poses
    pts = synth.make_cloud(3000, seed=61, extent=(6.0, 6.0, 6.0))
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=False)
    cam = ops.Camera(torch.from_numpy(K), IW, IH, 1.0, 5.0, 1e-6)
    t_np, q_np = _pose_set(3, seed=62)
    t, q = torch.from_numpy(t_np).to(dev), torch.from_numpy(q_np).to(dev)
    # B = 1 through the multi call with a workspace sized for it, bitwise the single call
    _, sc, tg, qg = ops.pose_forward_backward_multi(cloud, t[:1].contiguous(), q[:1].contiguous(), cam, ops.PoseWorkspace(cloud, 1, multi=True))
    _, s1, tg1, qg1 = ops.pose_forward_backward(cloud, t[:1].contiguous(), q[:1].contiguous(), cam, ops.PoseWorkspace(cloud))
    assert torch.equal(sc[0], s1) and torch.equal(tg, tg1) and torch.equal(qg, qg1)
    ws = ops.PoseWorkspace(cloud, 3)
    for bad in (dict(ws=ops.PoseWorkspace(cloud)), dict(ws=ops.PoseWorkspace(cloud, 2)), dict(trans=t.t().contiguous().t()),
                dict(quat=q.double()), dict(trans=t.cpu()), dict(mask=torch.ones(10, device=dev))):
        kw = dict(trans=t, quat=q, ws=ws, mask=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.pose_forward_backward_multi(cloud, kw["trans"], kw["quat"], cam, kw["ws"], mask=kw["mask"])
    # a model on a slice of the same tensor shares its data pointer, not its points
    full = torch.from_numpy(bundled).to(dev)
    (t0, q0), (t1, q1) = _starts(2, seed=63)
    a = ModelPose(full, torch.from_numpy(t0), torch.from_numpy(q0), torch.from_numpy(K), IW, IH, device=dev)
    b = ModelPose(full[:1000], torch.from_numpy(t1), torch.from_numpy(q1), torch.from_numpy(K), IW, IH, device=dev)
    assert b.points.data_ptr() == a.points.data_ptr()
    with pytest.raises(ValueError):
        optimize_poses([a, b], n_opt_steps=2)
