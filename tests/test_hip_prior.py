"""The per-point log-odds prior (ModelTraj(prior_log_odds=...), prior_kernels.hip): rewards = sigmoid(lo_sum + prior).

A zero prior changes no bit on any path; rewards, mean and gradients meet the f64 oracle given the prior; a path cut in two and
fused through coverage_log_odds is the whole path; two waypoint-sharded ranks give the single process's result; what is not
supported says so; the receding-horizon example runs."""
import importlib.util
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import load_golden, rel_inf
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _model(dev, pts, poses, quats, cls=None, **kw):
    from trajectory_optimization_amd.model import ModelTraj
    return (cls or ModelTraj)(torch.from_numpy(pts), torch.from_numpy(poses), torch.from_numpy(quats), torch.from_numpy(K), IW, IH,
                              device=dev, **kw)


def _case(n=90_000, W=17, seed=41):
    pts = synth.make_cloud(n, seed=seed)
    poses, quats = synth.make_path(W, optical=True, jitter_seed=seed)
    return pts, poses, quats


def _same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


# ---- 1. a zero prior is invisible, bitwise --------------------------------------------------------------------------------------

KINDS = {"culled": {}, "dense": dict(dense=True), "rig": dict(rig=synth.camera_rig(3)), "zbuffer": dict(occlusion="zbuffer")}


@pytest.mark.parametrize("kind", list(KINDS))
def test_zero_prior_is_invisible(dev, kind):
    from trajectory_optimization_amd.model import ModelTraj
    pts, poses, quats = _case()
    kw = KINDS[kind]
    zeros = torch.zeros(len(pts), dtype=torch.float32, device=dev)
    a, b = _model(dev, pts, poses, quats, **kw), _model(dev, pts, poses, quats, prior_log_odds=zeros, **kw)
    for _ in range(2):   # (the second round: a forward after a backward, over the same workspaces)
        la, lb = a(vis_wps_dist=0.0), b(vis_wps_dist=0.0)
        assert type(lb.grad_fn).__name__ == "_TrajLossBackward"   # the prior model takes the separate calls
        la.backward()
        lb.backward()
        assert _same(la.detach(), lb.detach()) and _same(a.rewards, b.rewards)
        for k in ("vis", "l2", "length", "smooth"):
            assert float(a.loss[k]) == float(b.loss[k]), k
        assert _same(a.poses.grad, b.poses.grad) and _same(a.quats.grad, b.quats.grad)
    # a loss built on model.rewards: the general dL/d rewards path
    for m in (a, b):
        m.poses.grad = m.quats.grad = None
        m(vis_wps_dist=0.0)
        (m.rewards.square().mean() + m.loss["vis"]).backward()
    assert _same(a.poses.grad, b.poses.grad) and _same(a.quats.grad, b.quats.grad)

    if kind == "culled":
        # the op-by-op criterion (a subclass criterion) with and without a zero prior
        class OpByOp(ModelTraj):
            def criterion(self, rewards):
                return super().criterion(rewards)
        c, d = _model(dev, pts, poses, quats, cls=OpByOp), _model(dev, pts, poses, quats, cls=OpByOp, prior_log_odds=zeros)
        lc, ld = c(vis_wps_dist=0.0), d(vis_wps_dist=0.0)
        lc.backward()
        ld.backward()
        assert _same(lc.detach(), ld.detach()) and _same(c.rewards, d.rewards)
        assert _same(c.poses.grad, d.poses.grad) and _same(c.quats.grad, d.quats.grad)


@pytest.mark.parametrize("kind", ["culled", "rig", "zbuffer"])
def test_zero_prior_optimize_trajectory_is_invisible(dev, kind):
    from trajectory_optimization_amd.optimizer import optimize_trajectory
    pts, poses, quats = _case(60_000, 13, 43)
    kw = KINDS[kind]
    a = _model(dev, pts, poses, quats, **kw)
    b = _model(dev, pts, poses, quats, prior_log_odds=torch.zeros(len(pts), device=dev), **kw)
    ra = optimize_trajectory(a, n_opt_steps=30, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
    rb = optimize_trajectory(b, n_opt_steps=30, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
    assert ra.steps_taken == rb.steps_taken == 30 and ra.losses == rb.losses
    assert _same(a.poses.data, b.poses.data) and _same(a.quats.data, b.quats.data) and _same(a.rewards, b.rewards)


def test_prior_back_to_none_is_the_fused_path(dev):
    pts, poses, quats = _case(50_000, 11, 44)
    a = _model(dev, pts, poses, quats)
    b = _model(dev, pts, poses, quats, prior_log_odds=torch.rand(len(pts), device=dev) * 2)
    lb = b(vis_wps_dist=0.0)
    assert type(lb.grad_fn).__name__ == "_TrajLossBackward" and b.prior_log_odds is not None
    b.prior_log_odds = None
    assert b.prior_log_odds is None
    la, lb = a(vis_wps_dist=0.0), b(vis_wps_dist=0.0)
    assert type(lb.grad_fn).__name__ == "_TrajLossPlanBackward"   # the one-call plan again
    la.backward()
    lb.backward()
    assert _same(la.detach(), lb.detach()) and _same(a.rewards, b.rewards)
    assert _same(a.poses.grad, b.poses.grad) and _same(a.quats.grad, b.quats.grad)


# ---- 2. against the unchanged f64 oracle ----------------------------------------------------------------------------------------

def _oracle_case(name):
    if name == "traj_synth_20000x32":
        d = load_golden(name)
        clip = (float(d["min_dist"]), float(d["max_dist"])) if "min_dist" in d else (1.0, 5.0)
        return d["points"], d["poses"], d["quats"], clip
    pts, poses, quats = _case(100_000, 32, 61)
    return pts, poses, quats, (1.0, 5.0)


# waypoints on the knife edge (test_hip_conditioning._margins: p_hat within 3e-7 of a clipping threshold) are excluded from the
# gradient bar; on these two cases there are none
EXCLUDED = {"traj_synth_20000x32": [], "synth_100000x32": []}


@pytest.mark.parametrize("name", ["traj_synth_20000x32", "synth_100000x32"])
@pytest.mark.parametrize("which", ["random", "committed"])
def test_prior_against_the_f64_oracle(dev, name, which):
    from oracle import oracle
    from test_hip_conditioning import MARGIN, _margins
    pts, poses, quats, clip = _oracle_case(name)
    excluded = np.nonzero(_margins(pts, poses, quats, clip) < MARGIN)[0].tolist()
    assert excluded == EXCLUDED[name]
    keep = np.setdiff1d(np.arange(len(poses)), excluded)
    if which == "random":
        prior = np.random.default_rng(7).uniform(0.0, 3.0, len(pts)).astype(np.float32)
    else:   # what another path (the same one shifted by 1.5 m sideways) committed
        other = _model(dev, pts, (poses + np.float32([0.0, 1.5, 0.0])).astype(np.float32), quats, min_dist=clip[0], max_dist=clip[1])
        prior = other.coverage_log_odds(vis_wps_dist=0.0).cpu().numpy()
        assert (prior > 0).any()
    f = oracle.traj_forward(pts, poses, quats, K, IW, IH, clip[0], clip[1], prec="f64")
    r_ref = 1.0 / (1.0 + np.exp(-(prior.astype(np.float64) + f["lo_sum"])))
    mean_ref = float(r_ref.mean())
    pg_ref, qg_ref = oracle.traj_backward(pts, poses, quats, K, IW, IH, dict(f, rewards=r_ref, mean_reward=mean_ref), min_dist=clip[0],
                                          max_dist=clip[1], prec="f64")
    # the fused visibility loss (unit sums) and a loss built on the rewards (the general dL/d rewards path)
    for path in ("vis", "rewards"):
        m = _model(dev, pts, poses, quats, min_dist=clip[0], max_dist=clip[1], prior_log_odds=torch.from_numpy(prior).to(dev))
        m(vis_wps_dist=0.0)
        if path == "vis":
            m.loss["vis"].backward()
        else:
            (1.0 / (torch.mean(m.rewards) + m.eps)).backward()
        np.testing.assert_allclose(m.rewards.detach().cpu().numpy(), r_ref, rtol=1e-5, atol=0.0)
        assert abs(float(m.mean_reward) - mean_ref) <= 1e-5 * mean_ref
        assert rel_inf(m.poses.grad.cpu().numpy()[keep], pg_ref[keep]) < 1e-5, path
        assert rel_inf(m.quats.grad.cpu().numpy()[keep], qg_ref[keep]) < 1e-5, path


# ---- 3. splitting a path is fusing maps -----------------------------------------------------------------------------------------

def test_split_path_equals_whole_path(dev):
    from oracle import oracle
    pts, poses, quats = _case(80_000, 14, 47)
    k = 6
    whole = _model(dev, pts, poses, quats)
    A = _model(dev, pts, poses[:k].copy(), quats[:k].copy())
    cov_a = A.coverage_log_odds(vis_wps_dist=0.0)
    B = _model(dev, pts, poses[k:].copy(), quats[k:].copy(), prior_log_odds=cov_a)
    whole(vis_wps_dist=0.0)
    whole.loss["vis"].backward()
    B(vis_wps_dist=0.0)
    B.loss["vis"].backward()
    assert (B.rewards - whole.rewards).abs().max().item() <= 2e-6
    assert rel_inf(B.poses.grad.cpu().numpy(), whole.poses.grad.cpu().numpy()[k:]) < 1e-5
    assert rel_inf(B.quats.grad.cpu().numpy(), whole.quats.grad.cpu().numpy()[k:]) < 1e-5
    # the first k waypoints of the whole path: A's map, to the bit
    assert _same(whole.coverage_log_odds(upto=k, vis_wps_dist=0.0), cov_a)
    # prior + lo_sum: B's map is the whole path's within rounding, and upto=0 is the prior itself
    full = whole.coverage_log_odds(vis_wps_dist=0.0)
    np.testing.assert_allclose(B.coverage_log_odds(vis_wps_dist=0.0).cpu().numpy(), full.cpu().numpy(), rtol=2e-6, atol=1e-5)
    assert _same(B.coverage_log_odds(upto=0), cov_a)
    # clamp_max clamps
    c = float(full.max()) / 2
    assert c > 0 and _same(whole.coverage_log_odds(clamp_max=c, vis_wps_dist=0.0), torch.clamp(full, max=c))
    # the caller's order on a sorted-packed cloud: sigmoid of the map is the oracle's rewards, point by point (its log-odds near
    # p_hat = 1 - 1e-6 are as undecided in f32 as the reference's own; the rewards are not)
    assert whole._cloud.sorted and not torch.equal(whole._cloud.perm[:whole._cloud.n].cpu(), torch.arange(len(pts), dtype=torch.int32))
    f = oracle.traj_forward(pts, poses, quats, K, IW, IH, prec="f64")
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-full.cpu().numpy().astype(np.float64))), f["rewards"], rtol=1e-5, atol=0.0)
    assert (torch.sigmoid(full) - whole.rewards).abs().max().item() <= 1e-6


# ---- 4. WaypointShard --------------------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _prior(n, dev):
    return torch.from_numpy(np.random.default_rng(5).uniform(0.0, 2.5, n).astype(np.float32)).to(dev)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from trajectory_optimization_amd.distributed import PointShard, WaypointShard, init_from_env
    from trajectory_optimization_amd.optimizer import optimize_trajectory
    _, _, device = init_from_env(backend="gloo")
    pts, poses, quats = _case(60_000, 9, 49)
    m = _model(device, pts, poses, quats, shard=WaypointShard(), prior_log_odds=_prior(len(pts), device))
    loss = m(vis_wps_dist=0.0)
    loss.backward()
    m2 = _model(device, pts, poses, quats, shard=WaypointShard(), prior_log_odds=_prior(len(pts), device))
    res = optimize_trajectory(m2, n_opt_steps=4, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
    try:   # a prior with point sharding: refused with a message that says so
        _model(device, pts, poses, quats, shard=PointShard(), prior_log_odds=_prior(len(pts), device))
        refused = ""
    except ValueError as e:
        refused = str(e)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), loss=loss.item(), rewards=m.rewards.detach().cpu().numpy(),
             pg=m.poses.grad.cpu().numpy(), qg=m.quats.grad.cpu().numpy(), opt_poses=m2.poses.detach().cpu().numpy(),
             opt_quats=m2.quats.detach().cpu().numpy(), opt_losses=np.asarray(res.losses), refused=refused)
    dist.barrier()
    dist.destroy_process_group()


def test_waypoint_shard_with_prior_equals_single_process(dev, tmp_path):
    from trajectory_optimization_amd.optimizer import optimize_trajectory
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / f"rank{r}.npz") for r in range(world))
    for k in ("loss", "rewards", "pg", "qg", "opt_poses", "opt_quats", "opt_losses"):
        assert np.array_equal(r0[k], r1[k]), k
    assert "PointShard" in str(r0["refused"])
    pts, poses, quats = _case(60_000, 9, 49)
    m = _model(dev, pts, poses, quats, prior_log_odds=_prior(len(pts), dev))
    loss = m(vis_wps_dist=0.0)
    loss.backward()
    assert abs(loss.item() - float(r0["loss"])) <= 2e-6 * abs(loss.item())
    np.testing.assert_allclose(r0["rewards"], m.rewards.detach().cpu().numpy(), rtol=2e-6, atol=2e-7)
    pg, qg = m.poses.grad.cpu().numpy(), m.quats.grad.cpu().numpy()
    assert np.abs(r0["pg"] - pg).max() <= 2e-5 * np.abs(pg).max()
    assert np.abs(r0["qg"] - qg).max() <= 2e-5 * np.abs(qg).max()
    m2 = _model(dev, pts, poses, quats, prior_log_odds=_prior(len(pts), dev))
    res = optimize_trajectory(m2, n_opt_steps=4, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
    np.testing.assert_allclose(r0["opt_losses"], res.losses, rtol=2e-5)
    np.testing.assert_allclose(r0["opt_poses"], m2.poses.detach().cpu().numpy(), atol=2e-4)
    np.testing.assert_allclose(r0["opt_quats"], m2.quats.detach().cpu().numpy(), atol=2e-4)


# ---- 5. errors and the example --------------------------------------------------------------------------------------------------

def test_rejected_inputs(dev):
    from trajectory_optimization_amd.optimizer import optimize_trajectories
    pts, poses, quats = _case(20_000, 7, 51)
    n = len(pts)
    good = torch.rand(n, device=dev)
    bad = {"wrong length": torch.zeros(n + 1, device=dev), "NaN": good.clone().index_fill_(0, torch.tensor([3], device=dev), float("nan")),
           "inf": good.clone().index_fill_(0, torch.tensor([3], device=dev), float("inf")),
           "negative": good.clone().index_fill_(0, torch.tensor([3], device=dev), -0.5), "wrong device": good.cpu()}
    for what, p in bad.items():
        with pytest.raises(ValueError):
            _model(dev, pts, poses, quats, prior_log_odds=p)
    m = _model(dev, pts, poses, quats, prior_log_odds=good)
    for what, p in bad.items():
        with pytest.raises(ValueError):
            m.prior_log_odds = p
    assert torch.equal(m.prior_log_odds, good)   # a refused value leaves the prior as it was
    other = _model(dev, pts, poses, quats)
    with pytest.raises(ValueError, match="prior"):
        optimize_trajectories([other, m], n_opt_steps=2)
    with pytest.raises(ValueError):
        m.coverage_log_odds(clamp_max=-1.0)
    with pytest.raises(ValueError):
        m.coverage_log_odds(upto=len(poses) + 1)


def test_receding_horizon_example(dev):
    spec = importlib.util.spec_from_file_location("receding", os.path.join(REPO, "examples", "receding_horizon_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--plans", "3", "--opt-steps", "20"])
    committed = out["committed_mean_reward"]
    assert len(committed) == 3 and len(out["plan_mean_reward"]) == 3
    assert all(b >= a for a, b in zip(committed, committed[1:])), committed
    assert committed[-1] > committed[0]
