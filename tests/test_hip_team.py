"""Team coverage (optimizer.optimize_team, model.TeamTraj, team_kernels.hip): B robots over one cloud behind ONE reward.

The team's visibility term is, bit for bit, a plain ModelTraj's on the members' evaluated waypoints laid end to end; a team of one is
optimize_trajectory; rewards, gradients, terms and the total meet the f64 oracle, the reference's own numbers (a fixture) and finite
differences; the early stop is the team's; member_gains attributes the coverage; the example runs."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_inf
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
SIDE = np.float32([0.0, 1.5, 0.0])   # member b starts b x 1.5 m sideways of the path


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _members(dev, pts, paths, quats, clip=(1.0, 5.0), prior=None, cls=None, **kw):
    """One ModelTraj per path over one packed cloud; the prior, if any, is the first model's (the team's)."""
    from trajectory_optimization_amd.model import ModelTraj
    cls = cls or ModelTraj
    first = cls(torch.from_numpy(pts), torch.from_numpy(paths[0]), torch.from_numpy(quats), torch.from_numpy(K), IW, IH, device=dev,
                min_dist=clip[0], max_dist=clip[1], prior_log_odds=prior, **kw)
    return [first] + [cls.sharing_cloud_of(first, torch.from_numpy(p), torch.from_numpy(quats), **kw) for p in paths[1:]]


def _paths(poses, B, side=SIDE):
    return [(poses + b * side).astype(np.float32) for b in range(B)]


def _cloud_case(name):
    if name == "traj_synth_20000x32":
        d = load_golden(name)
        clip = (float(d["min_dist"]), float(d["max_dist"])) if "min_dist" in d else (1.0, 5.0)
        return d["points"], d["poses"], d["quats"], clip
    poses, quats = synth.make_path(32, optical=True, jitter_seed=61)
    return synth.make_cloud(100_000, seed=61), poses, quats, (1.0, 5.0)


CLOUDS = ["traj_synth_20000x32", "synth_100000"]


def _reg_f64(p, p0, sw=14.0, lw=0.02, eps=1e-6):
    """criterion's l2, length, smooth (the reference's model.py:244-260) in f64 numpy."""
    p, p0 = np.asarray(p, np.float64), np.asarray(p0, np.float64)
    length = lambda t: np.linalg.norm(t[1:] - t[:-1], axis=1).sum()
    ab, ac = p[:-2] - p[1:-1], p[2:] - p[1:-1]
    c = (ab * ac).sum(1) / (np.linalg.norm(ab, axis=1) * np.linalg.norm(ac, axis=1) + eps)
    mean_angle = np.arccos(np.clip(c, -1.0, 1.0)).mean()
    return np.linalg.norm(p[0] - p0[0]), lw * abs(length(p) - length(p0)), sw / (mean_angle + eps)


# ---- 1. the invariant: the team's visibility term IS a plain ModelTraj's on E, bit for bit ---------------------------------------------

def _invariant(dev, pts, poses, quats, clip, B, vis_wps_dist, prior, kw):
    from trajectory_optimization_amd.model import ModelTraj, TeamTraj
    paths = _paths(poses, B)
    team = TeamTraj(_members(dev, pts, paths, quats, clip, prior=prior, **kw))
    step = team.models[0]._wps_step(vis_wps_dist)
    E = np.concatenate([p[::step] for p in paths])
    Eq = np.concatenate([quats[::step]] * B)
    ref = ModelTraj(team.models[0]._cloud, torch.from_numpy(E), torch.from_numpy(Eq), torch.from_numpy(K), IW, IH, device=dev,
                    min_dist=clip[0], max_dist=clip[1], prior_log_odds=prior, **kw)
    n_eval = len(E) // B
    rows = lambda grads: torch.cat([g[::step] for g in grads])
    total, lref = team(vis_wps_dist=vis_wps_dist), ref(vis_wps_dist=0.0)
    assert len(ref.poses) == B * n_eval and ref._wps_step(0.0) == 1
    assert torch.equal(team.rewards, ref.rewards) and torch.equal(team.mean_reward(), ref.mean_reward)
    assert torch.equal(team.loss["vis"].detach(), ref.loss["vis"].detach())
    # loss.backward(): the quaternion rows are the visibility term's alone (the regularisers do not see the orientations)
    total.backward()
    lref.backward()
    assert torch.equal(rows([m.quats.grad for m in team.models]), ref.quats.grad)
    for m in team.models:   # the waypoints in between carry no visibility gradient
        keep = torch.ones(len(m.quats), dtype=torch.bool)
        keep[::step] = False
        assert not m.quats.grad[keep].any()
    # loss['vis'].backward(): the visibility rows of positions and orientations
    for m in list(team.models) + [ref]:
        m.poses.grad = m.quats.grad = None
    team(vis_wps_dist=vis_wps_dist)
    ref(vis_wps_dist=0.0)
    team.loss["vis"].backward()
    ref.loss["vis"].backward()
    assert torch.equal(rows([m.poses.grad for m in team.models]), ref.poses.grad)
    assert torch.equal(rows([m.quats.grad for m in team.models]), ref.quats.grad)
    assert float(ref.poses.grad.abs().max()) > 0


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("kind", ["culled", "dense", "prior", "prior_dense", "rig"])
@pytest.mark.parametrize("name", CLOUDS)
def test_team_is_one_trajectory_on_E(dev, name, kind, B):
    pts, poses, quats, clip = _cloud_case(name)
    prior = None
    if kind.startswith("prior"):
        prior = torch.from_numpy(np.random.default_rng(7).uniform(0.0, 3.0, len(pts)).astype(np.float32)).to(dev)
    kw = dict(dense=True) if kind.endswith("dense") else (dict(rig=synth.camera_rig(3)) if kind == "rig" else {})
    _invariant(dev, pts, poses, quats, clip, B, 0.0, prior, kw)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("name", CLOUDS)
def test_team_is_one_trajectory_on_E_with_a_step_that_does_not_divide_W(dev, name, B):
    """W = 33 and step 2: every 2nd row of the concatenation would land on the members' odd rows from the second member on."""
    pts, _, _, clip = _cloud_case(name)
    poses, quats = synth.make_path(33, optical=True, jitter_seed=62)
    mean_dist = float(np.linalg.norm(poses[1:] - poses[:-1], axis=1).mean())
    _invariant(dev, pts, poses, quats, clip, B, 1.5 * mean_dist, None, {})


# ---- 2. a team of one is optimize_trajectory on the separate-calls path, bit for bit ---------------------------------------------------

@pytest.mark.parametrize("kind", ["plain", "stops", "clearance", "step3"])
def test_team_of_one_is_optimize_trajectory(dev, kind):
    from trajectory_optimization_amd.optimizer import optimize_team, optimize_trajectory
    pts = synth.make_cloud(60_000, seed=43, extent=(20.0, 20.0, 4.0))
    poses, quats = synth.make_path(13, optical=True, jitter_seed=43)
    kw = dict(clearance_radius=1.5, clearance_weight=2.0) if kind == "clearance" else {}
    zeros = torch.zeros(len(pts), device=dev)   # a zero prior: optimize_trajectory takes the separate calls as well
    a, = _members(dev, pts, [poses], quats, prior=zeros, **kw)
    b, = _members(dev, pts, [poses], quats, prior=zeros, **kw)
    vis_wps_dist = 2.5 * float(np.linalg.norm(poses[1:] - poses[:-1], axis=1).mean()) if kind == "step3" else 0.0   # step 3
    run = dict(n_opt_steps=30, lr_pose=0.05, lr_quat=0.01, rewards_th=1.0005 if kind == "stops" else 1e9, smoothness_th=0.5,
               vis_wps_dist=vis_wps_dist)
    ra, rb = optimize_trajectory(a, **run), optimize_team([b], **run)
    print(kind, "steps", ra.steps_taken, rb.steps_taken, "stopped", ra.stopped, rb.stopped)
    assert (ra.steps_taken, ra.stopped) == (rb.steps_taken, rb.stopped) and ra.losses == rb.losses
    if kind == "stops":
        assert ra.stopped and 1 < ra.steps_taken < 30
    if kind == "step3":
        assert a._wps_step(vis_wps_dist) == 3 and len(poses) % 3 != 0
    assert ra.visibility_gain == rb.visibility_gain and ra.smoothness_gain == rb.smoothness_gains[0]
    assert torch.equal(a.poses.data, b.poses.data) and torch.equal(a.quats.data, b.quats.data) and torch.equal(a.rewards, b.rewards)
    assert set(a.loss) == set(b.loss)
    for k in a.loss:
        assert float(a.loss[k]) == float(b.loss[k]), k


def test_next_terms_in_the_state_are_the_logged_terms(dev):
    """The terms a step's blocks read of the other members are what those members' own blocks log for that step, to the bit (the
    state's f64 terms rounded to f32 against the loss log), and the stop decision is the same in every member's state row."""
    from trajectory_optimization_amd import _lib
    from trajectory_optimization_amd._lib import ptr, stream_ptr
    L = _lib.lib()
    B, W, n = 3, 9, 4
    g = torch.Generator().manual_seed(3)
    p0 = torch.from_numpy(np.concatenate(_paths(synth.make_path(W, optical=True, jitter_seed=5)[0], B))).to(dev)
    poses = (p0 + 0.05 * torch.randn(p0.shape, generator=g).to(dev)).contiguous()
    quats = torch.randn(B * W, 4, generator=g).to(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    sb = L.tohip_team_state_bytes(B, n)
    state_buf = torch.zeros(sb, dtype=torch.uint8, device=dev)
    state = state_buf[:sb // 2].view(torch.float32).view(n + 1, B, 8)
    terms64 = state_buf[sb // 2:].view(torch.float64).view(n + 1, B, 4)
    log, member_terms = torch.zeros((B, n, 8), **f32), torch.empty((B, 8), **f32)
    pge, qge = 0.01 * torch.randn(B * W, 3, generator=g).to(dev), 0.01 * torch.randn(B * W, 4, generator=g).to(dev)
    pg, qg = torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 4), **f32)
    mom = [torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 4), **f32), torch.zeros((B * W, 4), **f32)]
    scalars = torch.tensor([0.6, 1.0 / 0.6, 0.0, 0.0], **f32)
    assert L.tohip_team_loss(ptr(poses), ptr(p0), W, B, 14.0, 0.02, 1e-6, None, 0.0, None, ptr(member_terms), ptr(terms64), None, None, None,
                             stream_ptr()) == 0
    for i in range(n):
        assert L.tohip_team_step_tail(ptr(poses), ptr(quats), ptr(p0), W, B, ptr(pge), ptr(qge), W, 1, ptr(pg), ptr(qg), *(ptr(t) for t in mom),
                                      14.0, 0.02, 1e-6, 0.05, 0.01, 0.9, 0.999, 1e-8, 1e9, 1e9, ptr(scalars), ptr(log), n * 8, ptr(state_buf),
                                      sb, n, i, 0.0, None, None, stream_ptr()) == 0
    t32 = terms64[:n, :, :3].to(torch.float32).permute(1, 0, 2)   # (B, n, 3): what step i read
    assert torch.equal(t32, log[:, :, 1:4])
    assert torch.equal(member_terms[:, 1:4], log[:, 0, 1:4])
    st = state[n].cpu()
    assert (st[:, 3] == n).all() and (st[:, 2] == 0).all() and (st[:, 0] == st[0, 0]).all()
    assert torch.equal(log[:, :, 4], log[0:1, :, 4].expand(B, n))   # one team total, in every member's row


# ---- 3. against the f64 oracle --------------------------------------------------------------------------------------------------

# waypoints of E on the knife edge (test_hip_conditioning._margins: p_hat within 3e-7 of a clipping threshold) are excluded from the
# gradient bar; on these cases there are none
EXCLUDED = {"traj_synth_20000x32": [], "synth_100000": []}


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("name", CLOUDS)
def test_team_against_the_f64_oracle(dev, name, with_prior):
    from oracle import oracle
    from test_hip_conditioning import MARGIN, _margins
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelTraj, TeamTraj
    pts, poses, quats, clip = _cloud_case(name)
    B = 2
    paths = _paths(poses, B)
    E, Eq = np.concatenate(paths), np.concatenate([quats] * B)
    excluded = np.nonzero(_margins(pts, E, Eq, clip) < MARGIN)[0].tolist()
    assert excluded == EXCLUDED[name]
    keep = np.setdiff1d(np.arange(len(E)), excluded)
    prior = np.random.default_rng(7).uniform(0.0, 3.0, len(pts)).astype(np.float32) if with_prior else np.zeros(len(pts), np.float32)
    f = oracle.traj_forward(pts, E, Eq, K, IW, IH, clip[0], clip[1], prec="f64")
    r_ref = 1.0 / (1.0 + np.exp(-(prior.astype(np.float64) + f["lo_sum"])))
    mean_ref = float(r_ref.mean())
    pg_ref, qg_ref = oracle.traj_backward(pts, E, Eq, K, IW, IH, dict(f, rewards=r_ref, mean_reward=mean_ref), min_dist=clip[0],
                                          max_dist=clip[1], prec="f64")
    members = _members(dev, pts, paths, quats, clip, prior=torch.from_numpy(prior).to(dev) if with_prior else None)
    team = TeamTraj(members)
    team(vis_wps_dist=0.0)
    team.loss["vis"].backward()
    np.testing.assert_allclose(team.rewards.detach().cpu().numpy(), r_ref, rtol=1e-5, atol=0.0)
    assert abs(float(team.mean_reward()) - mean_ref) <= 1e-5 * mean_ref
    pg = torch.cat([m.poses.grad for m in members]).cpu().numpy()
    qg = torch.cat([m.quats.grad for m in members]).cpu().numpy()
    assert rel_inf(pg[keep], pg_ref[keep]) < 1e-5 and rel_inf(qg[keep], qg_ref[keep]) < 1e-5

    # off the start, so that l2 and length are not zero: every member's regularisers against the op-by-op criterion of that member alone, and the total against the defined f64 sum
    class OpByOp(ModelTraj):
        def criterion(self, rewards):
            return super().criterion(rewards)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in members:
            m.poses += 0.05 * torch.randn(m.poses.shape, generator=gen).to(dev)
    total = team(vis_wps_dist=0.0)
    p_all = torch.cat([m.poses.detach() for m in members]).contiguous()
    _, total2, reg = ops.team_loss(p_all, team._poses0, B, 14.0, 0.02, 1e-6, torch.stack([team.mean_reward(), team.loss["vis"].detach(),
                                                                                           team.mean_reward(), team.mean_reward()]))
    assert torch.equal(total2.reshape(()), total.detach())
    Enow = np.concatenate([m.poses.detach().cpu().numpy() for m in members])
    f2 = oracle.traj_forward(pts, Enow, Eq, K, IW, IH, clip[0], clip[1], prec="f64")
    mean2 = float((1.0 / (1.0 + np.exp(-(prior.astype(np.float64) + f2["lo_sum"])))).mean())
    want = 1.0 / (mean2 + 1e-6)
    for b, m in enumerate(members):
        solo, = _members(dev, pts, [paths[b]], quats, clip, cls=OpByOp)
        with torch.no_grad():
            solo.poses.copy_(m.poses)
        solo(vis_wps_dist=0.0)
        (solo.loss["l2"] + solo.loss["length"] + solo.loss["smooth"]).backward()
        l2, length, smooth = _reg_f64(m.poses.detach().cpu().numpy(), paths[b])
        want += l2 + length + smooth
        # the op-by-op terms are f32 torch expressions: 1e-5 relative, plus 1e-5 absolute for `length`, a difference of two f32 sums
        # of about ten metres each (a few 1e-6 of rounding) times its weight
        for k, ref64 in (("l2", l2), ("length", length), ("smooth", smooth)):
            got = float(team.loss[k][b])
            assert abs(got - ref64) <= 1e-6 * abs(ref64) + 1e-9, (k, got, ref64)   # the kernel's own terms are f64 rounded once
            assert abs(got - float(solo.loss[k].detach())) <= 1e-5 * abs(got) + (1e-5 if k == "length" else 0.0), (k, got, float(solo.loss[k].detach()))
        # the op-by-op side differentiates arccos in f32 (test_hip_models: 5e-4 on the smoothness term's rows, which these include)
        assert rel_inf(reg[b * len(poses):(b + 1) * len(poses)].cpu().numpy(), solo.poses.grad.cpu().numpy()) < 5e-4
    assert abs(float(total.detach()) - want) <= 1e-5 * want


# ---- 4. against the reference itself ------------------------------------------------------------------------------------------------

def test_team_against_the_reference_fixture(dev):
    from trajectory_optimization_amd.model import TeamTraj
    d = load_golden("team_bundled_2")
    pts = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))["pts"].astype(np.float32)
    starts, now, quats = d["poses0"], d["poses"], d["quats"][0]
    members = _members(dev, pts, [starts[0], starts[1]], quats)
    with torch.no_grad():
        for m, p in zip(members, now):
            m.poses.copy_(torch.from_numpy(p).to(dev))
    team = TeamTraj(members)
    team(vis_wps_dist=0.0)
    team.loss["vis"].backward()
    assert abs(float(team.loss["vis"]) - float(d["loss_vis"])) <= 1e-5 * float(d["loss_vis"])
    np.testing.assert_allclose(team.rewards.detach().cpu().numpy(), d["rewards"], rtol=1e-5, atol=0.0)
    pg = torch.cat([m.poses.grad for m in members]).cpu().numpy()
    qg = torch.cat([m.quats.grad for m in members]).cpu().numpy()
    print("rel_inf vs the reference: poses", rel_inf(pg, d["vis_poses_grad"]), "quats", rel_inf(qg, d["vis_quats_grad"]))
    assert rel_inf(pg, d["vis_poses_grad"]) < 1e-5 and rel_inf(qg, d["vis_quats_grad"]) < 1e-5
    for b in range(2):
        l2, length, smooth = d["member_terms"][b]
        assert abs(float(team.loss["l2"][b]) - l2) <= 1e-5 * l2
        assert abs(float(team.loss["smooth"][b]) - smooth) <= 1e-5 * smooth
        # the reference's length term is weight x |difference of two f32 sums of nine segment lengths|: each sum carries a few ulp of
        # its own size, which the 1e-5 relative bar of the (much smaller) difference cannot absorb
        seg = lambda p: float(np.linalg.norm(p[1:] - p[:-1], axis=1).sum())
        atol = 0.02 * 8 * 2.0 ** -23 * (seg(now[b]) + seg(starts[b]))
        assert abs(float(team.loss["length"][b]) - length) <= 1e-5 * length + atol, (float(team.loss["length"][b]), length, atol)


# ---- 5. finite differences of the team total -----------------------------------------------------------------------------------

def test_team_total_gradient_matches_finite_differences(dev):
    from oracle import oracle
    from trajectory_optimization_amd.model import TeamTraj
    pts = synth.make_cloud(40_000, seed=33)
    poses, quats = synth.make_path(5, optical=True, jitter_seed=33)
    B = 2
    starts = _paths(poses, B)
    rng = np.random.default_rng(3)
    now = [(p + 0.05 * rng.standard_normal(p.shape)).astype(np.float32) for p in starts]
    members = _members(dev, pts, starts, quats)
    with torch.no_grad():
        for m, p in zip(members, now):
            m.poses.copy_(torch.from_numpy(p).to(dev))
    team = TeamTraj(members)
    team(vis_wps_dist=0.0).backward()
    Eq = np.concatenate([quats] * B)

    def total(P):
        t = oracle.traj_forward(pts, np.concatenate(P).astype(np.float32), Eq, K, IW, IH, prec="f64")["loss_vis"]
        return t + sum(sum(_reg_f64(P[b], starts[b])) for b in range(B))
    h = 2e-3   # test_hip_models.test_xy_yaw_gradient_matches_finite_differences: central differences of the f64 oracle, 3 % of the largest
    for b in range(B):
        g = members[b].poses.grad.cpu().numpy()
        for wi, ci in ((0, 0), (2, 1), (4, 0)):
            Pp, Pm = [p.astype(np.float64).copy() for p in now], [p.astype(np.float64).copy() for p in now]
            Pp[b][wi, ci] += h
            Pm[b][wi, ci] -= h
            fd = (total(Pp) - total(Pm)) / (2 * h)
            assert abs(g[wi, ci] - fd) <= 0.03 * np.abs(g).max() + 1e-7, (b, wi, ci, g[wi, ci], fd)


# ---- 6. the early stop is the team's ------------------------------------------------------------------------------------------------

def test_team_early_stop(dev):
    from trajectory_optimization_amd.optimizer import optimize_team
    pts = synth.make_cloud(30_000, seed=51, extent=(20.0, 20.0, 4.0))
    poses, quats = synth.make_path(12, optical=True, jitter_seed=None)
    zig = np.zeros_like(poses)
    zig[1::2, 1] = 1.0
    starts = [(poses + 0.6 * zig).astype(np.float32), (poses + SIDE + 0.15 * zig).astype(np.float32)]   # a rough path and a nearly smooth one
    n = 25
    run = dict(n_opt_steps=n, lr_pose=0.03, lr_quat=0.0, rewards_th=0.0, vis_wps_dist=0.0)   # (every visibility gain passes 0)

    def gains(log):   # (B, steps, 8) -> (steps, B): smooth0_b / smooth_b in f32, as the rule takes them
        s = log[:, :, 3]
        return (s[:, :1] / s).T.astype(np.float32)

    free = optimize_team(_members(dev, pts, starts, quats), smoothness_th=1e9, **run)
    assert free.steps_taken == n and not free.stopped and free.loss_log.shape == (2, n, 8)
    G = gains(free.loss_log)
    assert (G[0] == 1.0).all()
    # one member passes, the other never does: the team does not stop
    th = np.float32(float(G[:, 1].max()) * 1.001)
    assert (G[:, 0] > th).any() and not (G[:, 1] > th).any(), (G[:, 0].max(), G[:, 1].max())
    held = _members(dev, pts, starts, quats)
    res = optimize_team(held, smoothness_th=float(th), **run)
    assert res.steps_taken == n and not res.stopped
    assert np.array_equal(res.loss_log, free.loss_log)
    # both pass: the team stops at the step the logged terms name
    M = G.min(axis=1)
    k = next(i for i in range(2, n - 1) if M[i] > M[:i].max())
    th2 = np.float32((float(M[:k].max()) + float(M[k])) / 2)
    assert M[:k].max() < th2 < M[k]
    team = _members(dev, pts, starts, quats)
    res = optimize_team(team, smoothness_th=float(th2), **run)
    own = gains(res.loss_log).min(axis=1)   # the replay of the run's own log
    expected = next(i for i in range(len(own)) if own[i] > th2)
    assert res.stopped and res.steps_taken == expected + 1 == k + 1, (res.steps_taken, expected, k)
    assert min(res.smoothness_gains) > th2 and np.float32(min(res.smoothness_gains)) == own[expected]
    assert res.losses == free.losses[:k + 1]
    # a stopped team stays put: where k + 1 steps without a stop leave it
    cut = _members(dev, pts, starts, quats)
    optimize_team(cut, smoothness_th=1e9, **dict(run, n_opt_steps=k + 1))
    for a, b in zip(team, cut):
        assert torch.equal(a.poses.data, b.poses.data) and torch.equal(a.quats.data, b.quats.data)


# ---- 7. who adds what ------------------------------------------------------------------------------------------------------------------

def _member_rows(dev, m0, paths, quats, step=1):
    """The per-member log-odds rows (B, npad) of the forward that keeps the members apart, built here from the paths."""
    from trajectory_optimization_amd import ops
    n, C = len(paths), (m0._rig.n_cams if m0._rig is not None else 1)
    E = torch.from_numpy(np.concatenate([p[::step] for p in paths])).to(dev)
    Eq = torch.from_numpy(np.concatenate([quats[::step]] * n)).to(dev)
    n_eval = len(E) // n
    toff = (torch.arange(n + 1, dtype=torch.int32) * n_eval).to(dev)
    return ops.traj_forward(m0._cloud, E, Eq, m0._cam, ops.TrajWorkspace(m0._cloud, n * n_eval * C, n), m0._rig, flags=m0._flags,
                            traj_offsets=toff)[0]


@pytest.mark.parametrize("B", [2, 3, 5, 9])   # the pass's four instantiations hold 2, 4, 8 and 16 members
@pytest.mark.parametrize("with_prior", [False, True])
def test_member_gains(dev, with_prior, B):
    from oracle import oracle
    from trajectory_optimization_amd.model import TeamTraj
    pts, poses, quats, clip = _cloud_case("synth_100000")
    W = 8 if B == 3 else 4
    poses, quats = poses[:W], quats[:W]
    paths = _paths(poses, B, side=np.float32([0.0, 0.7, 0.0]))
    prior = np.random.default_rng(9).uniform(0.0, 2.0, len(pts)).astype(np.float32) if with_prior else np.zeros(len(pts), np.float32)
    tprior = torch.from_numpy(prior).to(dev) if with_prior else None
    members = _members(dev, pts, paths, quats, clip, prior=tprior)
    team = TeamTraj(members)
    gain, count = team.member_gains(vis_wps_dist=0.0)
    gain2, count2 = team.member_gains(vis_wps_dist=0.0)
    assert torch.equal(gain, gain2) and torch.equal(count, count2)
    assert gain.dtype == torch.float64 and count.dtype == torch.int64 and gain.shape == count.shape == (B,)
    # the counts: exact against the per-member rows of the forward that keeps them apart
    m0 = members[0]
    assert torch.equal(count, (_member_rows(dev, m0, paths, quats)[:, :len(pts)] > 0).sum(dim=1).cpu())
    assert (count > 0).all() and (gain > 0).all()

    # the gains: two means from the f64 oracle, each under the 1e-5 relative bar
    def mean_of(which):
        P, Q = np.concatenate([paths[b] for b in which]), np.concatenate([quats] * len(which))
        f = oracle.traj_forward(pts, P, Q, K, IW, IH, clip[0], clip[1], prec="f64")
        return float((1.0 / (1.0 + np.exp(-(prior.astype(np.float64) + f["lo_sum"])))).mean())
    full = mean_of(range(B))
    for b in range(B):
        want = full - mean_of([c for c in range(B) if c != b])
        print("B", B, "member", b, "gain", float(gain[b]), "oracle", want, "bar", 2e-5 * full)
        assert abs(float(gain[b]) - want) <= 2e-5 * full
    if B != 3:
        return
    # a member far from the cloud sees nothing at all — every p of its waypoints is 0, which makes the reference's rewards (and the f64
    # oracle's) NaN for the whole team: member_gains counts it as absent — gain 0 and count 0 exactly, the others' as without it
    far = (poses + np.float32([1000.0, 0.0, 0.0])).astype(np.float32)
    with_far = paths[:2] + [far] + paths[2:]
    assert torch.isnan(_member_rows(dev, m0, with_far, quats)[2, :len(pts)]).all()
    g4, c4 = TeamTraj(_members(dev, pts, with_far, quats, clip, prior=tprior)).member_gains(vis_wps_dist=0.0)
    assert c4[2] == 0 and g4[2] == 0.0
    keep = [0, 1, 3]
    assert torch.equal(g4[keep], gain) and torch.equal(c4[keep], count)


def test_member_gains_with_a_rig_and_a_step_and_too_many_members(dev):
    """member_gains builds its own workspace and offsets: with a 3-camera rig and every 2nd waypoint, counts exact and gains against
    the means of sigmoid over the forward's own per-member rows (the f64 oracle has no rig); more than 16 members are refused by name."""
    from trajectory_optimization_amd.model import TeamTraj
    pts, poses, quats, clip = _cloud_case("synth_100000")
    poses, quats = poses[:9], quats[:9]
    B = 3
    paths = _paths(poses, B)
    vis_wps_dist = 1.5 * float(np.linalg.norm(poses[1:] - poses[:-1], axis=1).mean())
    members = _members(dev, pts, paths, quats, clip, rig=synth.camera_rig(3))
    team = TeamTraj(members)
    assert members[0]._wps_step(vis_wps_dist) == 2
    gain, count = team.member_gains(vis_wps_dist=vis_wps_dist)
    lo = _member_rows(dev, members[0], paths, quats, step=2)[:, :len(pts)].double()
    assert torch.equal(count, (lo > 0).sum(dim=1).cpu()) and (count > 0).all()
    S = lo.sum(dim=0)
    full = float(torch.sigmoid(S).mean())
    for b in range(B):
        want = full - float(torch.sigmoid(S - lo[b]).mean())
        assert abs(float(gain[b]) - want) <= 2e-5 * full, (b, float(gain[b]), want)
    # and the team's own map agrees with those rows: one sum over all members' evaluated waypoints
    cov = team.coverage_log_odds(vis_wps_dist=vis_wps_dist)
    perm = members[0]._cloud.perm[:len(pts)].long()
    np.testing.assert_allclose(cov[perm].cpu().numpy(), S.float().cpu().numpy(), rtol=2e-6, atol=1e-5)
    many = _members(dev, pts, _paths(poses[:3], 17, side=np.float32([0.0, 0.1, 0.0])), quats[:3], clip)
    with pytest.raises(ValueError, match="at most 16"):
        TeamTraj(many).member_gains()


# ---- 8. autograd and the launch-only loop walk the same path; the example ---------------------------------------------------------

def test_team_autograd_loop_follows_optimize_team(dev):
    from trajectory_optimization_amd.model import TeamTraj
    from trajectory_optimization_amd.optimizer import optimize_team
    pts = synth.make_cloud(60_000, seed=49)
    poses, quats = synth.make_path(9, optical=True, jitter_seed=49)
    paths = _paths(poses, 2)
    a, b = _members(dev, pts, paths, quats), _members(dev, pts, paths, quats)
    team = TeamTraj(a)
    assert len(list(team.parameters())) == 4
    opt = torch.optim.Adam([{"params": [m.poses for m in a], "lr": 0.05}, {"params": [m.quats for m in a], "lr": 0.01}])
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = team(vis_wps_dist=0.0)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    res = optimize_team(b, n_opt_steps=4, lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=0.0)
    print("bitwise:", all(torch.equal(x.poses.data, y.poses.data) and torch.equal(x.quats.data, y.quats.data) for x, y in zip(a, b)),
          losses == res.losses)
    # the bars test_hip_prior holds the prior model's autograd and launch-only paths to
    np.testing.assert_allclose(losses, res.losses, rtol=2e-5)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x.poses.detach().cpu().numpy(), y.poses.detach().cpu().numpy(), atol=2e-4)
        np.testing.assert_allclose(x.quats.detach().cpu().numpy(), y.quats.detach().cpu().numpy(), atol=2e-4)
    # the team's map is the next plan's prior: the rewards are its sigmoid
    team(vis_wps_dist=0.0)
    cov = team.coverage_log_odds(vis_wps_dist=0.0)
    assert cov.shape == (len(pts),) and (torch.sigmoid(cov) - team.rewards.detach()).abs().max().item() <= 1e-6
    assert torch.equal(team.coverage_log_odds(clamp_max=1.0, vis_wps_dist=0.0), torch.clamp(cov, max=1.0))


def _brute_clearance(pts, p, r, w):
    """weight x sum (r - d)^2 over the waypoints whose nearest cloud point lies within r, f64 brute force."""
    d = np.sqrt(((p.astype(np.float64)[:, None, :] - pts.astype(np.float64)[None, :, :]) ** 2).sum(-1)).min(axis=1)
    return w * float(((r - d[d < r]) ** 2).sum())


@pytest.mark.parametrize("clearance", [False, True])
@pytest.mark.parametrize("W", [33, 32])   # at step 2: a gather of each member's rows, and a stride over the concatenation
@pytest.mark.parametrize("B", [2, 3])
def test_optimize_team_with_a_waypoint_step(dev, B, W, clearance):
    """optimize_team with B > 1 and step 2: the evaluated rows are every member's own (gathered when W is not a multiple of the step,
    a stride of the concatenated rows when it is), the tail scatters member b's rows back to ITS rows r * step, and the rows in
    between move by the regularisers (and clearance) only.  The first step's gradients and loss rows are TeamTraj's, bit for bit
    (both take the unit-sum arithmetic); a few steps follow the TeamTraj + Adam loop within test_hip_prior's bars.  With clearance
    on, every member's term and the total against an f64 brute force."""
    from oracle import oracle
    from test_hip_conditioning import MARGIN, _margins
    from trajectory_optimization_amd import _lib, ops
    from trajectory_optimization_amd.model import TeamTraj
    from trajectory_optimization_amd.optimizer import optimize_team
    pts = synth.make_cloud(60_000, seed=49, extent=(20.0, 20.0, 4.0))
    poses, quats = synth.make_path(W, optical=True, jitter_seed=62)
    vis_wps_dist = 1.5 * float(np.linalg.norm(poses[1:] - poses[:-1], axis=1).mean())
    starts = _paths(poses, B)
    rng = np.random.default_rng(7)
    now = [(p + 0.03 * rng.standard_normal(p.shape)).astype(np.float32) for p in starts]   # off the start: l2, length > 0
    CLR = dict(clearance_radius=1.5, clearance_weight=2.0) if clearance else {}

    def members():
        ms = _members(dev, pts, starts, quats, **CLR)
        with torch.no_grad():
            for m, p in zip(ms, now):
                m.poses.copy_(torch.from_numpy(p).to(dev))
        return ms
    run = dict(lr_pose=0.05, lr_quat=0.01, rewards_th=1e9, vis_wps_dist=vis_wps_dist)
    a, b = members(), members()
    assert a[0]._wps_step(vis_wps_dist) == 2 and (W % 2 != 0) == (W == 33)
    n_eval = (W + 1) // 2
    team = TeamTraj(a)
    total = team(vis_wps_dist=vis_wps_dist)
    total.backward()
    res = optimize_team(b, n_opt_steps=1, **run)
    # the first step: gradients and loss rows, bit for bit
    for k, m in enumerate(a):
        assert torch.equal(res.poses_grad[k], m.poses.grad) and torch.equal(res.quats_grad[k], m.quats.grad), k
        row = res.loss_log[k, 0]
        assert row[0] == float(team.loss["vis"]) and row[4] == float(total)
        for i, name in ((1, "l2"), (2, "length"), (3, "smooth")) + (((5, "clearance"),) if clearance else ()):
            assert row[i] == float(team.loss[name][k]), (k, name)
    # the rows in between carry the regularisers' (and clearance) rows only, and their orientations do not move
    between = torch.ones(W, dtype=torch.bool, device=dev)
    between[::2] = False
    p_all = torch.cat([torch.from_numpy(p) for p in now]).to(dev).contiguous()
    clr_terms = clr_rows = None
    if clearance:
        clr_rows = torch.empty((B * W, 3), dtype=torch.float32, device=dev)
        clr_terms = torch.empty(_lib.lib().tohip_clearance_workspace_bytes(B * W) // 8, dtype=torch.float64, device=dev)
        ops.clearance(a[0]._cloud, p_all, 1.5, 2.0, grad=clr_rows, terms=clr_terms)
    scalars = torch.stack([team.mean_reward(), team.loss["vis"].detach(), team.mean_reward(), team.mean_reward()])
    _, _, reg = ops.team_loss(p_all, team._poses0, B, 14.0, 0.02, 1e-6, scalars, 2.0 if clearance else 0.0, clr_terms)
    other = reg + clr_rows if clearance else reg
    q0 = torch.from_numpy(quats).to(dev)
    for k, m in enumerate(b):
        assert torch.equal(res.poses_grad[k][between], other[k * W:(k + 1) * W][between])
        assert not res.quats_grad[k][between].any() and torch.equal(m.quats.data[between], q0[between])
        assert res.quats_grad[k][::2].abs().sum() > 0 and not torch.equal(m.quats.data[::2], q0[::2])
    # the orientations' rows (the visibility term's alone) are the f64 oracle's on E, member by member (1e-5): each member's rows
    # came from ITS waypoints (the positions' rows carry the regularisers too; they are TeamTraj's bits, checked above)
    E, Eq = np.concatenate([p[::2] for p in now]), np.concatenate([quats[::2]] * B)
    assert not (_margins(pts, E, Eq, (1.0, 5.0)) < MARGIN).any()   # no waypoint of E on the knife edge: none is excluded from the bar
    f = oracle.traj_forward(pts, E, Eq, K, IW, IH, prec="f64")
    _, qg_ref = oracle.traj_backward(pts, E, Eq, K, IW, IH, f, prec="f64")
    for k in range(B):
        assert rel_inf(res.quats_grad[k][::2].cpu().numpy(), qg_ref[k * n_eval:(k + 1) * n_eval]) < 1e-5, k
    # the total against the defined f64 sum
    want = f["loss_vis"]
    for k in range(B):
        want += sum(_reg_f64(now[k], starts[k]))
        if clearance:
            c = _brute_clearance(pts, now[k], 1.5, 2.0)
            want += c
            assert abs(float(team.loss["clearance"][k]) - c) <= 1e-5 * c + 1e-12, (k, float(team.loss["clearance"][k]), c)
    assert abs(float(total) - want) <= 1e-5 * want
    if clearance:
        assert sum(float(x) for x in team.loss["clearance"]) > 0
    # a few steps: the launch-only loop follows TeamTraj + Adam
    a, b = members(), members()
    team = TeamTraj(a)
    opt = torch.optim.Adam([{"params": [m.poses for m in a], "lr": 0.05}, {"params": [m.quats for m in a], "lr": 0.01}])
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = team(vis_wps_dist=vis_wps_dist)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    res = optimize_team(b, n_opt_steps=4, **run)
    np.testing.assert_allclose(losses, res.losses, rtol=2e-5)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x.poses.detach().cpu().numpy(), y.poses.detach().cpu().numpy(), atol=2e-4)
        np.testing.assert_allclose(x.quats.detach().cpu().numpy(), y.quats.detach().cpu().numpy(), atol=2e-4)


def test_team_coverage_example(dev):
    spec = importlib.util.spec_from_file_location("team_sample", os.path.join(REPO, "examples", "team_coverage_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--opt-steps", "10"])
    vals = [out["start"], out["alone_fused"], out["team"]] + out["member_gain"]
    assert all(np.isfinite(v) for v in vals) and len(out["member_gain"]) == 2 and len(out["member_count"]) == 2
    assert 0.5 <= out["start"] < 1.0 and 0.5 <= out["team"] < 1.0
