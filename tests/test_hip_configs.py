"""The five BASELINE.json configurations, by name, at their full sizes (seeded synthetic inputs of BASELINE.md)."""
import numpy as np
import pytest
import torch

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _setup(dev, n, w, rig=None):
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(n, seed=0)
    poses, quats = synth.make_path(w, optical=True)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    cam = ops.Camera(K, IW, IH)
    rg = ops.CameraRig(rig[0], rig[1], dev) if rig is not None else None
    return ops, pts, poses, quats, cloud, cam, rg


def test_config1_100k_x32_forward_only(dev):
    """configs[1]: 100k-point cloud, 32 waypoints, fwd-only visibility + reward."""
    from oracle import oracle
    ops, pts, poses, quats, cloud, cam, _ = _setup(dev, 100_000, 32)
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    ws = ops.TrajWorkspace(cloud, 32)
    with torch.no_grad():
        lo, mm = ops.traj_forward(cloud, p, q, cam, ws)
        r, sc = ops.traj_reward(cloud, lo, cam, ws)
    f = oracle.traj_forward(pts, poses, quats, K, IW, IH, prec="f64")
    np.testing.assert_allclose(r.cpu().numpy(), f["rewards"], rtol=1e-5, atol=0)
    assert abs(sc[1].item() - f["loss_vis"]) <= 3e-6 * f["loss_vis"]


def test_config3_1m_x1024_sharded_over_8(dev):
    """configs[3]: 1M points x 1024 waypoints as 8 shards of 128 (what 8 ranks compute before the all-reduce):
    the shards' log-odds add up to the single-device result; rewards match the oracle on a waypoint subsample, and all 1 M of
    them — from the summed shard log-odds — match the f64 oracle over all 1024 waypoints.  A rank's real work, the backward of
    its 128 waypoints behind the summed log-odds, is checked for two shards against the f64 oracle under the conditional 1e-5
    bar (a waypoint with a point within MARGIN of a threshold is excused only within what the band is worth; the excused set is
    asserted exactly)."""
    import warnings
    from oracle import oracle
    from test_hip_conditioning import BASELINE_EXCLUDED_WAYPOINTS, MARGIN, _margins
    ops, pts, poses, quats, cloud, cam, _ = _setup(dev, 1_000_000, 1024)
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    ws1 = ops.TrajWorkspace(cloud, 1024)
    lo_all, mm_all = ops.traj_forward(cloud, p, q, cam, ws1)
    ws = ops.TrajWorkspace(cloud, 128)
    total = torch.zeros_like(lo_all)
    mms = []
    for r in range(8):
        lo, mm = ops.traj_forward(cloud, p[128 * r:128 * (r + 1)].contiguous(), q[128 * r:128 * (r + 1)].contiguous(), cam, ws)
        total += lo
        mms.append(mm.clone())
    assert torch.equal(torch.cat(mms), mm_all)                       # per-waypoint min/max are shard-local
    np.testing.assert_allclose(total.cpu().numpy(), lo_all.cpu().numpy(), rtol=2e-6, atol=1e-4)
    rew, sc = ops.traj_reward(cloud, total, cam, ws)
    assert 0.5 <= sc[0].item() <= 1.0 and np.isfinite(sc[1].item())
    sel = np.arange(0, 1024, 64)
    lo_s, _ = ops.traj_forward(cloud, p[sel].contiguous(), q[sel].contiguous(), cam, ops.TrajWorkspace(cloud, len(sel)))
    r_s, _ = ops.traj_reward(cloud, lo_s, cam, ws)
    f = oracle.traj_forward(pts, poses[sel], quats[sel], K, IW, IH, prec="f64")
    np.testing.assert_allclose(r_s.cpu().numpy(), f["rewards"], rtol=1e-5, atol=0)
    # every reward of the 1024-waypoint trajectory (the summed shards' log-odds) against the f64 oracle, computed once
    rew_all = rew.cpu().numpy()
    f_all = oracle.traj_forward(pts, poses, quats, K, IW, IH, prec="f64")
    np.testing.assert_allclose(rew_all, f_all["rewards"], rtol=1e-5, atol=0)
    assert abs(sc[1].item() - f_all["loss_vis"]) <= 5e-6 * f_all["loss_vis"]
    # a rank's backward: its shard's forward again (the workspace then holds that step), the reward of the summed log-odds, and the
    # backward of its 128 waypoints behind it
    gout = torch.ones(1, device=dev)
    for s in (0, 5):
        rows = slice(128 * s, 128 * (s + 1))
        ops.traj_forward(cloud, p[rows].contiguous(), q[rows].contiguous(), cam, ws)
        rew_s, sc_s = ops.traj_reward(cloud, total, cam, ws)
        assert torch.equal(rew_s, rew) and torch.equal(sc_s, sc)
        pg, qg = ops.traj_backward(cloud, 128, cam, ws, total, scalars=sc_s, gout=gout)
        pg, qg = pg.cpu().numpy().astype(np.float64), qg.cpu().numpy().astype(np.float64)
        kw = dict(min_dist=1.0, max_dist=5.0, prec="f64")
        ref = oracle.traj_backward(pts, poses[rows], quats[rows], K, IW, IH, f_all, **kw)
        keep = _margins(pts, poses[rows], quats[rows], (1.0, 5.0)) > MARGIN
        assert np.flatnonzero(~keep).tolist() == BASELINE_EXCLUDED_WAYPOINTS[f"config3_shard{s}"]
        band = None
        if not keep.all():   # what the points inside the band are worth: the activity threshold moved by -/+ 2 MARGIN
            lo_b = oracle.traj_backward(pts, poses[rows], quats[rows], K, IW, IH, f_all, act_shift=-2 * MARGIN, **kw)
            hi_b = oracle.traj_backward(pts, poses[rows], quats[rows], K, IW, IH, f_all, act_shift=2 * MARGIN, **kw)
            band = [np.abs(a - b).max(axis=1) for a, b in zip(lo_b, hi_b)]
        worst = worst_ex = 0.0
        for k, (g, r) in enumerate(((pg, ref[0]), (qg, ref[1]))):
            den = np.abs(r).max()
            err = np.abs(g - r).max(axis=1)
            assert (err[keep] < 1e-5 * den).all(), (s, k, (err[keep] / den).max())
            worst = max(worst, float((err[keep] / den).max()))
            for v in np.flatnonzero(~keep):
                assert band[k][v] > 0 and err[v] <= 1.05 * band[k][v] + 1e-5 * den, (s, k, v, err[v] / den, band[k][v] / den)
                worst_ex = max(worst_ex, float(err[v] / den))
        warnings.warn(f"config 3 shard {s} backward vs the f64 oracle over 1024 waypoints: {int(keep.sum())} waypoints within 1e-5 (worst "
                      f"{worst:.1e} of the largest row), {int((~keep).sum())} excused within the band (worst {worst_ex:.1e})")


def test_config4_five_cameras_1m_x256(dev):
    """configs[4]: 5-camera rig x 1M points x 256 waypoints (1280 virtual waypoints): the rig path equals the same
    cameras written out as independent waypoints, exact culling equals dense evaluation, and the body-pose gradient
    is the sum over the rig's cameras (checked by the quaternion-tangency and shard-additivity properties)."""
    rq, rt = synth.camera_rig(5)
    ops, pts, poses, quats, cloud, cam, rg = _setup(dev, 1_000_000, 256, rig=(rq, rt))
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    ws = ops.TrajWorkspace(cloud, 256 * 5)
    gout = torch.ones(1, device=dev)
    out = {}
    for flags in (0, ops.DENSE):
        lo, mm = ops.traj_forward(cloud, p, q, cam, ws, rg, flags=flags)
        r, sc = ops.traj_reward(cloud, lo, cam, ws)
        pg, qg = ops.traj_backward(cloud, p.shape[0], cam, ws, lo, scalars=sc, gout=gout, rig=rg, flags=flags)
        out[flags] = (lo.clone(), r.clone(), pg.clone(), qg.clone(), mm.clone())
    for a, b in zip(out[0], out[ops.DENSE]):
        assert torch.equal(a, b)
    lo, r, pg, qg, mm = out[0]
    # explicit virtual waypoints (body pose composed with each camera on the host, f64)
    qn = quats.astype(np.float64) / np.linalg.norm(quats.astype(np.float64), axis=1, keepdims=True)
    vq = synth.quat_mul(qn[:, None, :], rq[None].astype(np.float64)).reshape(-1, 4).astype(np.float32)
    vt = np.repeat(poses, 5, axis=0)  # zero lever arms
    lo_v, mm_v = ops.traj_forward(cloud, torch.from_numpy(vt).to(dev), torch.from_numpy(vq).to(dev), cam, ws)
    np.testing.assert_allclose(mm.cpu().numpy(), mm_v.cpu().numpy(), rtol=2e-5, atol=1e-30)
    r_v, _ = ops.traj_reward(cloud, lo_v, cam, ws)
    np.testing.assert_allclose(r.cpu().numpy(), r_v.cpu().numpy(), rtol=2e-5, atol=2e-5)
    assert np.isfinite(pg.cpu().numpy()).all() and np.abs(pg.cpu().numpy()).max() > 0
    dots = (quats.astype(np.float64) * qg.cpu().numpy()).sum(1)
    assert np.abs(dots).max() <= 1e-5 * np.abs(qg.cpu().numpy()).max()
    # the f64 oracle on the explicit 1280 virtual waypoints at the full size: rewards, loss, and the body-pose gradients through
    # the chain rule of the rig composition (autograd in f64 over q_v = q_w/|q_w| (x) q_c, t_v = t_w + R(q_w) l_c)
    from oracle import oracle
    f = oracle.traj_forward(pts, vt, vq, K, IW, IH, prec="f64")
    rew_err = float(np.abs(r.cpu().numpy() - f["rewards"]).max() / 0.5)
    print(f"config 4 vs f64 oracle: rewards max rel err {rew_err:.2e}")
    np.testing.assert_allclose(r.cpu().numpy(), f["rewards"], rtol=1e-5, atol=0)
    g_vt, g_vq = oracle.traj_backward(pts, vt, vq, K, IW, IH, f, prec="f64")
    P = torch.tensor(poses, dtype=torch.float64, requires_grad=True)
    Q = torch.tensor(quats, dtype=torch.float64, requires_grad=True)
    Qn = Q / Q.norm(dim=1, keepdim=True)
    rqt = torch.tensor(rq, dtype=torch.float64)

    def qmul(a, b):
        aw, ax, ay, az = a.unbind(-1)
        bw, bx, by, bz = b.unbind(-1)
        return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)
    VQ = qmul(Qn[:, None, :], rqt[None]).reshape(-1, 4)
    VT = P[:, None, :].expand(-1, 5, -1).reshape(-1, 3)   # zero lever arms
    ((VT * torch.tensor(g_vt)).sum() + (VQ * torch.tensor(g_vq)).sum()).backward()
    from conftest import rel_inf
    print(f"config 4 body gradients vs oracle chain rule: poses {rel_inf(pg.cpu().numpy(), P.grad.numpy()):.2e}, "
          f"quats {rel_inf(qg.cpu().numpy(), Q.grad.numpy()):.2e}")
    assert rel_inf(pg.cpu().numpy(), P.grad.numpy()) < 1e-5 and rel_inf(qg.cpu().numpy(), Q.grad.numpy()) < 1e-5
