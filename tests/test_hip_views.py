"""Greedy view selection on the device (views_kernels.hip): the sparse rows are the forward's rows, the rounds follow the
greedy rule to the integer, the stops and ties are the documented ones, and the result is what the models and the reference reward.

The brute force every selection is compared with uses the EXISTING calls only: per round S + lo_c in torch f32 for every candidate,
tohip_traj_reward(_prior) on it, F recomputed exactly from the f32 rewards it returns (N <= 2^23: reward_fixed is exact on them),
argmax with the lowest-index tie rule.

Rows are compared with the forward's over the N points; the forward's pad positions [N, npad) repeat the last sorted point, a view
set stores no pad entry, so ViewSet.row has zeros there (checked)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mods():
    from trajectory_optimization_amd import ops, synth, tools
    return ops, synth, tools


def _cam(ops, synth):
    return ops.Camera(synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT, 1.0, 5.0)


def _synth_grid(synth, g, h):
    return synth.candidate_grid(np.linspace(-15, 15, g), np.linspace(-15, 15, g), 0.0, h)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_CLOUDS = {}


def _cloud(name, dev):
    """'golden20k': traj_synth_20000x32's cloud; an int: synth.make_cloud(n, 0).  Packed once per module."""
    ops, synth, _ = _mods()
    if name not in _CLOUDS:
        pts = load_golden("traj_synth_20000x32")["points"] if name == "golden20k" else synth.make_cloud(int(name), 0)
        _CLOUDS[name] = ops.PackedCloud(_t(pts.astype(np.float32), dev))
    return _CLOUDS[name]


def _fixed_sum(rewards, n):
    """F: the integer the reward kernel sums, recomputed exactly from f32 rewards in [1/2, 1] (..., N) -> int64 (...)."""
    shift = 47 - (n - 1).bit_length()
    assert n <= 2 ** 23 and shift >= 24
    return (rewards.double() * float(2 ** shift)).round().long().sum(-1)


def _F(ops, cloud, cam, X, prior, ws):
    """F of every row of X (B, npad) through the existing reward call."""
    if prior is None:
        return _fixed_sum(ops.traj_reward(cloud, X, cam, ws)[0], cloud.n)
    return torch.stack([_fixed_sum(ops.traj_reward(cloud, X[b], cam, ws, prior=prior)[0], cloud.n) for b in range(X.shape[0])])


def brute_force(ops, cloud, cam, rows, k, prior=None, min_gain=0.0):
    """The greedy rule with the existing calls.  rows (M, npad) f32 (a NaN row: absent) -> (order, gain_fixed, S, per-round gains)."""
    M, n = rows.shape[0], cloud.n
    ws = ops.TrajWorkspace(cloud, M, M)
    absent = torch.isnan(rows[:, :n]).any(dim=1)
    rows = torch.where(absent[:, None], torch.zeros_like(rows), rows)
    S = torch.zeros(cloud.npad, dtype=torch.float32, device=rows.device)
    shift = 47 - (n - 1).bit_length()
    taken = absent.clone()
    order, gains, every = [], [], []
    for _ in range(k):
        if bool(taken.all()):
            break
        G = _F(ops, cloud, cam, S[None, :] + rows, prior, ws) - _F(ops, cloud, cam, S[None, :], prior, ws)[0]
        G = torch.where(taken, torch.full_like(G, torch.iinfo(torch.int64).min), G)
        g = int(G.max())
        c = int(torch.nonzero(G == g)[0])   # the lowest index among the best
        every.append(G.cpu())
        if g <= 0 or g / 2 ** shift / n < min_gain:
            break
        order.append(c); gains.append(g)
        S = S + rows[c]
        taken[c] = True
    return order, gains, S, every


def _dense_rows(ops, vs):
    return torch.stack([vs.row(c) for c in range(vs.n_candidates)])


def _select(ops, vs, k, prior=None, min_gain=0.0):
    order, gain, n_sel, S = ops.views_select(vs, k, prior, min_gain)
    n = int(n_sel.item())
    return order[:n].tolist(), gain[:n].tolist(), S


# ---- 1. rows ---------------------------------------------------------------------------------------------------------------------

ROW_CASES = [("golden20k", "culled"), ("golden20k", "dense"), ("golden20k", "rig3"), ("golden20k", "hpr"), ("100000", "culled"),
             ("100000", "dense")]


@pytest.mark.parametrize("cloud_name,mode", ROW_CASES)
def test_rows_are_the_forwards_rows_whatever_the_chunk(dev, cloud_name, mode):
    ops, synth, _ = _mods()
    cloud, cam, M = _cloud(cloud_name, dev), _cam(ops, synth), 40
    p, q = synth.make_path(M, optical=True, jitter_seed=5)
    p, q = _t(p, dev), _t(q, dev)
    rig = ops.CameraRig(*synth.camera_rig(3), dev) if mode == "rig3" else None
    flags = ops.DENSE if mode == "dense" else 0
    occ = ops.occlusion_bits(cloud, cloud.points, p, q, cam, 1.0, 15.0, "hpr") if mode == "hpr" else None
    C = 3 if rig is not None else 1
    ref, _ = ops.traj_forward(cloud, p, q, cam, ops.TrajWorkspace(cloud, M * C, M), rig, flags=flags, occ=occ,
                              traj_offsets=torch.arange(M + 1, dtype=torch.int32, device=dev))
    ref = ref[:, :cloud.n]
    assert not bool(torch.isnan(ref).any()) and bool((ref > 0).any(dim=1).all())
    for chunk in (1, 7, M):
        vs = ops.ViewSet(cloud, cam, M, rig=rig, flags=flags, chunk=chunk, nnz_capacity=int((ref > 0).sum()))   # exactly what it needs
        vs.append(p, q, occ)
        stored, needed, fits = vs.status()
        assert fits and stored == needed == int((ref > 0).sum()) == vs.nnz
        idx, val = vs.entries()
        off = vs.offsets.cpu().tolist()
        assert off[0] == 0 and off[-1] == stored and not bool(vs.absent.any())
        assert bool((val > 0).all()) and bool((idx >= 0).all()) and bool((idx < cloud.n).all())   # no zero, no pad entry
        for c in range(M):
            row = vs.row(c)
            assert torch.equal(row[:cloud.n], ref[c]), (chunk, c)
            assert not bool(row[cloud.n:].any())
            seg = idx[off[c]:off[c + 1]]
            assert off[c + 1] - off[c] == int((ref[c] > 0).sum()) and bool((seg[1:] > seg[:-1]).all()), (chunk, c)


def test_capacity_too_small_reports_the_needed_count_and_stores_nothing(dev):
    ops, synth, _ = _mods()
    cloud, cam = _cloud("golden20k", dev), _cam(ops, synth)
    p, q = [_t(a, dev) for a in _synth_grid(synth, 6, 4)]
    full = ops.ViewSet(cloud, cam, 144)
    full.append(p, q)
    need = full.nnz
    small = ops.ViewSet(cloud, cam, 144, nnz_capacity=need // 3, chunk=16)
    small.append(p, q)
    stored, needed, fits = small.status()
    assert not fits and needed == need and stored <= need // 3
    order, gain, n_sel, S = ops.views_select(small, 4)      # a set that did not fit selects nothing
    assert int(n_sel.item()) == 0 and not bool(S.any())
    exact = ops.ViewSet(cloud, cam, 144, nnz_capacity=need, chunk=16)
    exact.append(p, q)
    assert exact.status() == (need, need, True)
    assert _select(ops, exact, 4)[:2] == _select(ops, full, 4)[:2]


# ---- 2. the greedy rule ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,g,h,k", [(20_000, 6, 4, 12), (100_000, 8, 8, 16)])
@pytest.mark.parametrize("with_prior", [False, True])
def test_selection_is_the_greedy_rule_to_the_integer(dev, n, g, h, k, with_prior):
    ops, synth, _ = _mods()
    cloud, cam = _cloud(str(n), dev), _cam(ops, synth)
    p, q = [_t(a, dev) for a in _synth_grid(synth, g, h)]
    prior = None
    if with_prior:
        prior = ops.LogOddsPrior(cloud, 3.0 * torch.rand(n, generator=torch.Generator().manual_seed(11)).to(dev))
    vs = ops.ViewSet(cloud, cam, p.shape[0])
    vs.append(p, q)
    rows = _dense_rows(ops, vs)
    want_order, want_gain, want_S, _ = brute_force(ops, cloud, cam, rows, k, prior)
    assert len(want_order) == k
    for _ in range(2):   # the same twice in a row
        order, gain, S = _select(ops, vs, k, prior)
        assert order == want_order and gain == want_gain
        assert torch.equal(S, want_S)


# ---- 3. ties and stops -----------------------------------------------------------------------------------------------------------

def test_ties_absent_candidates_and_stops(dev):
    ops, synth, _ = _mods()
    cloud, cam = _cloud("20000", dev), _cam(ops, synth)
    gp, gq = _synth_grid(synth, 6, 4)
    base = ops.ViewSet(cloud, cam, 144)
    base.append(_t(gp, dev), _t(gq, dev))
    order8, gain8, _ = _select(ops, base, 8)
    assert len(order8) == 8 and gain8[3] > gain8[4]
    best = order8[0]

    # an exact duplicate of the best view at a higher index, and a view that looks away from everything
    away_p, away_q = np.float32([[1e4, 1e4, 0.0]]), gq[:1]
    p = _t(np.concatenate([gp, gp[best:best + 1], away_p]), dev)
    q = _t(np.concatenate([gq, gq[best:best + 1], away_q]), dev)
    vs = ops.ViewSet(cloud, cam, 146, chunk=32)
    vs.append(p, q)
    assert vs.absent.cpu().tolist() == [False] * 145 + [True]
    assert bool(torch.isnan(vs.row(145)[:cloud.n]).all()) and torch.equal(vs.row(144), vs.row(best))
    rows = _dense_rows(ops, vs)
    want_order, want_gain, _, every = brute_force(ops, cloud, cam, rows, 146)
    order, gain, S = _select(ops, vs, 146)
    assert order == want_order and gain == want_gain
    assert order[0] == best and 145 not in order                      # the lower index wins the tie; the absent one is never chosen
    assert int(every[0][144]) == int(every[0][best]) == gain[0]        # ... it was a tie
    assert 0 <= int(every[1][144]) < gain[0]                           # the duplicate is still offered, and then adds less
    assert len(order) <= 145                                           # k beyond the candidates that can be chosen: ends early

    # k = 1 is the argmax of the single-view gains
    o1, g1, _ = _select(ops, vs, 1)
    assert o1 == [best] and g1 == [int(every[0].max())]

    # three candidates, one of them absent, k = 3: two are chosen
    tiny = ops.ViewSet(cloud, cam, 3)
    tiny.append(_t(np.concatenate([gp[order8[0]:order8[0] + 1], away_p, gp[order8[1]:order8[1] + 1]]), dev),
                _t(np.concatenate([gq[order8[0]:order8[0] + 1], away_q, gq[order8[1]:order8[1] + 1]]), dev))
    o3, g3, _ = _select(ops, tiny, 3)
    assert o3 == [0, 2] and g3 == gain8[:2]

    # a prior that leaves nothing to gain (sigmoid(40) is 1 in f32): the first round's best adds 0 and nothing is chosen
    full = ops.LogOddsPrior(cloud, torch.full((cloud.n,), 40.0, device=dev))
    assert _select(ops, base, 8, prior=full)[:2] == ([], [])

    # min_gain between two consecutive gains of the earlier run stops exactly there
    shift = 47 - (cloud.n - 1).bit_length()
    mid = 0.5 * (gain8[3] + gain8[4]) / 2 ** shift / cloud.n
    o4, g4, _ = _select(ops, base, 8, min_gain=mid)
    assert o4 == order8[:4] and g4 == gain8[:4]


# ---- 4. S and the map; 5. against the models -------------------------------------------------------------------------------------

def test_outputs_and_models(dev):
    ops, synth, tools = _mods()
    from trajectory_optimization_amd.model import ModelTraj
    n = 20_000
    pts = _t(synth.make_cloud(n, 0), dev)
    gp, gq = [_t(a, dev) for a in _synth_grid(synth, 6, 4)]
    prior = 2.0 * torch.rand(n, generator=torch.Generator().manual_seed(3)).to(dev)
    K = torch.from_numpy(synth.K_INTRINS)
    kw = dict(intrins=K, img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT)
    sel = tools.select_views(pts, gp, gq, 8, prior_log_odds=prior, clamp_max=2.5, **kw)
    assert sel.n_selected == 8 and sel.order.dtype == torch.int64 and sel.gains.dtype == torch.float64
    assert torch.equal(sel.poses, gp[sel.order.to(dev)]) and torch.equal(sel.quats, gq[sel.order.to(dev)])
    assert not bool(sel.absent.any()) and sel.absent.shape == (144,)

    cloud, cam = ops.PackedCloud(pts), _cam(ops, synth)
    lp = ops.LogOddsPrior(cloud, prior)
    vs = ops.ViewSet(cloud, cam, 144, chunk=50)
    vs.append(gp, gq)
    assert sel.nnz == vs.nnz
    S = torch.zeros(cloud.npad, dtype=torch.float32, device=dev)
    for c in sel.order.tolist():
        S = S + vs.row(c)                                  # the chosen rows, in selection order
    assert torch.equal(sel.log_odds, S)
    assert torch.equal(sel.coverage_log_odds, ops.traj_coverage(cloud, S, lp, 2.5))
    rewards, scalars = ops.traj_reward(cloud, S, cam, ops.TrajWorkspace(cloud, 1), prior=lp)
    assert torch.equal(sel.rewards, rewards) and sel.mean_reward == float(scalars[0])
    shift = 47 - (n - 1).bit_length()
    assert torch.equal(sel.gains, sel.gain_fixed.double() / 2 ** shift / n)
    # the gains add up to what the chosen views add to the prior's mean reward, exactly (integers)
    r0, _ = ops.traj_reward(cloud, torch.zeros_like(S), cam, ops.TrajWorkspace(cloud, 1), prior=lp)
    assert int(sel.gain_fixed.sum()) == int(_fixed_sum(rewards, n) - _fixed_sum(r0, n))

    # a ModelTraj on the chosen views rewards them as the selection does (another summation order: the parity bar, not bits)
    m = ModelTraj(pts, sel.poses, sel.quats, K, synth.IMG_WIDTH, synth.IMG_HEIGHT, device=dev, prior_log_odds=prior)
    m(vis_wps_dist=0.0)
    a, b = m.rewards.detach().double(), sel.rewards.double()
    assert float(((a - b).abs() / b).max()) < 1e-5

    # select_views(model) scores as select_views(points, same settings)
    for extra, mk in ((dict(), dict()), (dict(dense=True, rig=synth.camera_rig(3)), dict(dense=True, rig=synth.camera_rig(3)))):
        model = ModelTraj(pts, gp[:8], gq[:8], K, synth.IMG_WIDTH, synth.IMG_HEIGHT, device=dev, prior_log_odds=prior, **mk)
        s1 = tools.select_views(model, gp, gq, 6)
        s2 = tools.select_views(pts, gp, gq, 6, prior_log_odds=prior, **kw, **extra)
        assert torch.equal(s1.order, s2.order) and torch.equal(s1.gain_fixed, s2.gain_fixed) and s1.n_selected == 6
        assert torch.equal(s1.rewards, s2.rewards) and torch.equal(s1.coverage_log_odds, s2.coverage_log_odds)


def test_occlusion_and_capacity_retry_through_the_public_call(dev):
    ops, synth, tools = _mods()
    n = 20_000
    pts = _t(synth.make_cloud(n, 0), dev)
    gp, gq = [_t(a, dev) for a in _synth_grid(synth, 6, 4)]
    kw = dict(intrins=torch.from_numpy(synth.K_INTRINS), img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT)
    plain = tools.select_views(pts, gp, gq, 5, chunk=48, **kw)
    occ = tools.select_views(pts, gp, gq, 5, occlusion="hpr", chunk=48, **kw)
    assert occ.n_selected == 5 and occ.nnz < plain.nnz            # hidden points store nothing
    cloud, cam = ops.PackedCloud(pts), _cam(ops, synth)
    rows = ops.occlusion_bits(cloud, cloud.points, gp, gq, cam, 1.0, 15.0, "hpr")
    vs = ops.ViewSet(cloud, cam, 144)
    vs.append(gp, gq, rows)
    o, g, _ = _select(ops, vs, 5)
    assert occ.order.tolist() == o and occ.gain_fixed.tolist() == g
    # the first capacity guess (1 % of M N) is too small for a cloud this dense around the candidates: the call sizes it again
    near = _t((synth.make_cloud(n, 0) * np.float32([0.2, 0.2, 1.0])).astype(np.float32), dev)
    few_p, few_q = [_t(a, dev) for a in synth.candidate_grid(np.linspace(-3, 3, 2), np.linspace(-3, 3, 2), 0.0, 4)]
    sel = tools.select_views(near, few_p, few_q, 4, **kw)
    assert sel.nnz > max(4096, 16 * n // 100) and sel.n_selected == 4


# ---- 6. against the reference; 7. the example -------------------------------------------------------------------------------------

def test_reference_order_and_rewards_on_the_bundled_grid(dev):
    """Conditional on the fixture's margins (tests/golden/make_golden_views.py refuses to write it below 100 x the rounding bound)."""
    ops, synth, tools = _mods()
    d = np.load(os.path.join(GOLDEN, "views_bundled_144.npz"))
    b = np.load(os.path.join(GOLDEN, "bundled.npz"))
    assert float(d["margins"].min()) >= 100.0 * float(d["bound"])
    gp, gq = synth.bundled_candidate_grid(b["pts"], b["poses"])
    assert np.array_equal(gp, d["cand_poses"]) and np.array_equal(gq, d["cand_quats"])
    sel = tools.select_views(_t(b["pts"].astype(np.float32), dev), _t(gp, dev), _t(gq, dev), 8, intrins=torch.from_numpy(synth.K_INTRINS),
                             img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT)
    assert sel.order.tolist() == d["order"].tolist()
    ref = torch.from_numpy(d["rewards"]).double()
    assert float(((sel.rewards.cpu().double() - ref).abs() / ref).max()) < 1e-5
    assert abs(sel.mean_reward - float(d["mean_reward"])) < 1e-5 * float(d["mean_reward"])
    np.testing.assert_allclose(sel.gains.numpy(), d["gains"], rtol=1e-3)


def test_example_selects_better_views_than_the_bundled_path(dev):
    import importlib.util
    spec = importlib.util.spec_from_file_location("view_selection_sample", os.path.join(REPO, "examples", "view_selection_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--opt-steps", "5"])
    assert out["selected"] > out["path"]
    assert out["n_views"] == out["n_selected"]
