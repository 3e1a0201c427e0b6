"""The conditional part of the gradient parity claim, pinned on the REFERENCE (not on the oracle): fixtures written by
tests/golden/make_golden.py `dense` hold the reference's own f32 rewards and visibility gradients for a dense room (200 k points in
6 x 6 x 3 m) and for the two configurations of tests/test_hip_conditioning.py's generator that have a waypoint with a point within
f32 rounding of p_hat = 1/2 (/root/reference/src/model.py:226-231).

  kept waypoints      |hip - reference| / max|reference| < 1e-5, and the same against each waypoint's OWN row norm is reported;
  excluded waypoints  |hip - reference| and |reference - oracle f64| are both at most what the points inside the band are worth
                      (oracle f64 with the activity threshold moved by -/+ 2 x 3e-7): the reference's own f32 result is as
                      undecided there as this implementation's.
"""
import warnings

import numpy as np
import pytest
import torch

from conftest import EXCLUDED_WAYPOINTS, conditional_gradient_report, load_reference_case, rel_inf
from test_hip_conditioning import MARGIN
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", ["traj_dense_room_200k", "traj_conditioning_32", "traj_conditioning_34"])
def test_hip_against_the_references_own_f32_gradients(name, dense):
    from trajectory_optimization_amd.model import ModelTraj
    d = load_reference_case(name)
    dev = torch.device("cuda:0")
    m = ModelTraj(torch.from_numpy(d["points"]), torch.from_numpy(d["poses"]), torch.from_numpy(d["quats"]), torch.from_numpy(K), IW, IH,
                  min_dist=d["clip"][0], max_dist=d["clip"][1], device=dev, dense=dense)
    m(vis_wps_dist=0.0)
    m.loss["vis"].backward()
    torch.cuda.synchronize()
    # rewards and the loss are continuous in p_hat at the thresholds: no condition on them (north star: 1e-5 relative)
    assert abs(m.loss["vis"].item() - float(d["loss_vis"])) <= 5e-6 * float(d["loss_vis"])
    np.testing.assert_allclose(m.rewards.detach().cpu().numpy(), d["rewards"], rtol=1e-5, atol=0)
    gp, gq = m.poses.grad.cpu().numpy(), m.quats.grad.cpu().numpy()
    rep = conditional_gradient_report(d, gp, gq, MARGIN)
    # exactly the waypoints the fixture was built around are outside the plain bar — nobody else is excused
    assert rep["excluded_waypoints"] == EXCLUDED_WAYPOINTS[name] and rep["kept"] == len(d["poses"]) - len(EXCLUDED_WAYPOINTS[name])
    warnings.warn(f"{name} ({'dense' if dense else 'culled'}) against the reference's f32 gradients: {rep['kept']} waypoints within 1e-5 (worst "
                  f"{rep['worst_kept']:.1e} of the largest row, {rep['worst_kept_own_row']:.1e} of their own row), {rep['excluded']} with a point "
                  f"within {MARGIN:g} of p_hat = 1/2 (worst {rep['worst_excluded']:.1e}, inside what those points are worth; the reference "
                  f"differs from the f64 restatement by as much); global rel_inf poses {rel_inf(gp, d['vis_poses_grad']):.1e} quats "
                  f"{rel_inf(gq, d['vis_quats_grad']):.1e}")


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", ["traj_stress_23_4", "traj_stress_31_83", "traj_stress_31_101", "traj_stress_23_134"])
def test_hip_on_what_the_stress_runs_found(name, dense):
    """tools/stress_models.py's finds, pinned on the reference's own f32 results (make_golden.py stress; the oracle's twin of this
    test is tests/test_oracle_golden.py::test_stress_findings_against_the_reference): a waypoint whose p all underflow to 0 in f32
    (NaN everywhere, as the reference), one point just below the upper threshold carrying a waypoint's gradient (determined to
    what an f32 uncertainty of p_hat is worth, and the reference no better), a gradient of 7e-9 out of r (1 - r) at r = 0.999999."""
    from conftest import phat_uncertainty_report
    from trajectory_optimization_amd.model import ModelTraj
    d = load_reference_case(name)
    dev = torch.device("cuda:0")
    m = ModelTraj(torch.from_numpy(d["points"]), torch.from_numpy(d["poses"]), torch.from_numpy(d["quats"]), torch.from_numpy(K), IW, IH,
                  min_dist=d["clip"][0], max_dist=d["clip"][1], device=dev, dense=dense)
    m(vis_wps_dist=0.0)
    m.loss["vis"].backward()
    torch.cuda.synchronize()
    gp, gq, rew = m.poses.grad.cpu().numpy(), m.quats.grad.cpu().numpy(), m.rewards.detach().cpu().numpy()
    if name == "traj_stress_23_134":
        assert np.isnan(rew).all() and np.isnan(m.loss["vis"].item()) and np.isnan(gp).all() and np.isnan(gq).all()
        return
    assert abs(m.loss["vis"].item() - float(d["loss_vis"])) <= 5e-6 * float(d["loss_vis"])
    np.testing.assert_allclose(rew, d["rewards"], rtol=1e-5, atol=0)
    if name == "traj_stress_31_101":
        ref = d["vis_poses_grad"].astype(np.float64)
        assert np.array_equal(np.abs(gp).max(axis=1) > 0, np.abs(ref).max(axis=1) > 0)   # the same single waypoint carries gradient
        # the bound, derived on the f64 restatement: the gradient is (dL/dr) r (1 - r) of points with r -> 1, and an f32 r carries
        # half an ulp of 1 (2^-25) of its own rounding — what is the gradient worth when every reward moves by that much either way?
        from oracle import oracle
        f64 = oracle.traj_forward(d["points"], d["poses"], d["quats"], K, IW, IH, d["clip"][0], d["clip"][1], prec="f64")
        kw = dict(min_dist=d["clip"][0], max_dist=d["clip"][1], prec="f64")
        pg64, qg64 = oracle.traj_backward(d["points"], d["poses"], d["quats"], K, IW, IH, f64, **kw)
        spread = []
        for sgn in (-1.0, 1.0):
            f = dict(f64)
            f["rewards"] = np.clip(f64["rewards"] + sgn * 2.0 ** -25, 0.0, 1.0)
            spread.append(oracle.traj_backward(d["points"], d["poses"], d["quats"], K, IW, IH, f, **kw))
        worth_p = np.abs(spread[1][0] - spread[0][0]).max()
        worth_q = np.abs(spread[1][1] - spread[0][1]).max()
        assert 0.01 * np.abs(pg64).max() < worth_p < np.abs(pg64).max(), (worth_p, np.abs(pg64).max())
        for got in (gp, ref):   # this implementation and the reference itself, both against the f64 restatement
            assert np.abs(got - pg64).max() <= 1.05 * worth_p
        assert np.abs(gq - qg64).max() <= 1.05 * worth_q and np.abs(d["vis_quats_grad"] - qg64).max() <= 1.05 * worth_q
        # ... and since r05 this implementation takes 1 - r from the exponential (r e, no cancellation): it holds the plain bar here too
        assert np.abs(gp - ref).max() <= 1e-5 * np.abs(ref).max() and np.abs(gq - d["vis_quats_grad"]).max() <= 1e-5 * np.abs(d["vis_quats_grad"]).max()
        assert np.abs(gp - pg64).max() <= 1e-5 * np.abs(pg64).max()
        warnings.warn(f"{name}: one gradient row of {np.abs(ref).max():.1e}; half an ulp of 1 in the rewards, either way, is worth {worth_p / np.abs(pg64).max():.2f} of it; "
                      f"HIP vs reference {np.abs(gp - ref).max() / np.abs(ref).max():.2e}, HIP vs f64 {np.abs(gp - pg64).max() / np.abs(pg64).max():.2e}, "
                      f"reference vs f64 {np.abs(ref - pg64).max() / np.abs(pg64).max():.2e}")
        return
    rep = phat_uncertainty_report(d, gp, gq, MARGIN)
    # ONE waypoint per fixture is worth more than the bar under +-6e-7 of p_hat; its two rows (position, quaternion) are the only
    # ones that may miss the plain bar (the report asserts that every other row holds it)
    assert rep["uncertain_waypoints"] == EXCLUDED_WAYPOINTS[name] and rep["inside_bar"] >= 2 * (len(d["poses"]) - 1), rep
    warnings.warn(f"{name} ({'dense' if dense else 'culled'}): {rep['inside_bar']} gradient rows within 1e-5 of the reference, {rep['excused']} within "
                  f"what +-{2 * MARGIN:g} in p_hat is worth to their waypoint (worst {rep['worst']:.1e} of the largest row, worth {rep['worst_worth']:.1e})")


@pytest.mark.parametrize("dense", [False, True])
def test_hip_full_size_against_the_reference(dense):
    """1 M points x 16 waypoints against the reference's own f32 results at that size (make_golden.py full; the oracle's twin:
    tests/test_oracle_golden.py::test_full_size_against_the_reference)."""
    from trajectory_optimization_amd.model import ModelTraj
    d = load_reference_case("traj_full_1m_16")
    dev = torch.device("cuda:0")
    m = ModelTraj(torch.from_numpy(d["points"]), torch.from_numpy(d["poses"]), torch.from_numpy(d["quats"]), torch.from_numpy(K), IW, IH,
                  min_dist=d["clip"][0], max_dist=d["clip"][1], device=dev, dense=dense)
    m(vis_wps_dist=0.0)
    m.loss["vis"].backward()
    torch.cuda.synchronize()
    rew = m.rewards.detach().cpu().numpy()
    assert abs(m.loss["vis"].item() - float(d["loss_vis"])) <= 5e-6 * float(d["loss_vis"])
    np.testing.assert_allclose(rew[::997], d["rewards_every_997th"], rtol=1e-5, atol=0)
    assert abs(float(rew.astype(np.float64).sum()) - float(d["rewards_sum"])) <= 1e-6 * float(d["rewards_sum"])
    assert abs(int((rew > 0.5).sum()) - int(d["rewards_above_half"])) <= 2
    gp, gq = m.poses.grad.cpu().numpy(), m.quats.grad.cpu().numpy()
    rep = conditional_gradient_report(d, gp, gq, MARGIN)
    assert rep["excluded_waypoints"] == EXCLUDED_WAYPOINTS["traj_full_1m_16"] == [] and rep["kept"] == 16   # all 16 hold the plain bar
    warnings.warn(f"1 M x 16 ({'dense' if dense else 'culled'}) against the reference's f32 results: {rep['kept']} waypoints within 1e-5 (worst "
                  f"{rep['worst_kept']:.1e} of the largest row, {rep['worst_kept_own_row']:.1e} of their own row), {rep['excluded']} excluded; "
                  f"global rel_inf poses {rel_inf(gp, d['vis_poses_grad']):.1e} quats {rel_inf(gq, d['vis_quats_grad']):.1e}")


def _reward_samples(rew, d, every):
    """A `baseline` fixture's reward samples (make_golden.py baseline) against all N rewards in the caller's order."""
    np.testing.assert_allclose(rew[::every], d[f"rewards_every_{every}th"], rtol=1e-5, atol=0)
    assert abs(float(rew.astype(np.float64).sum()) - float(d["rewards_sum"])) <= 1e-6 * float(d["rewards_sum"])
    assert abs(int((rew > 0.5).sum()) - int(d["rewards_above_half"])) <= 2


def _config2_checks(d, what, loss_vis, rew, gp, gq):
    """Config 2 (1 M x 128, bench.py's step) against the reference's own f32 results: the 1 M x 16 test's bars, the excluded set
    exact (test_hip_conditioning.BASELINE_EXCLUDED_WAYPOINTS)."""
    from test_hip_conditioning import BASELINE_EXCLUDED_WAYPOINTS
    assert rew.shape == (1_000_000,) and gp.shape == (128, 3) and gq.shape == (128, 4)
    assert abs(loss_vis - float(d["loss_vis"])) <= 5e-6 * float(d["loss_vis"])
    _reward_samples(rew, d, 997)
    rep = conditional_gradient_report(d, gp, gq, MARGIN)
    excluded = BASELINE_EXCLUDED_WAYPOINTS["traj_full_1m_128"]
    assert rep["excluded_waypoints"] == excluded and rep["kept"] == 128 - len(excluded)
    warnings.warn(f"1 M x 128 ({what}) against the reference's f32 results: {rep['kept']} waypoints within 1e-5 (worst {rep['worst_kept']:.1e} "
                  f"of the largest row, {rep['worst_kept_own_row']:.1e} of their own row), {rep['excluded']} excluded; global rel_inf poses "
                  f"{rel_inf(gp, d['vis_poses_grad']):.1e} quats {rel_inf(gq, d['vis_quats_grad']):.1e}")


@pytest.mark.parametrize("dense", [False, True])
def test_hip_config2_against_the_reference(dense):
    """BASELINE config 2 — the size bench.py times, 1 M points x 128 waypoints, fwd + bwd — against the reference ITSELF at that size
    (make_golden.py baseline; the oracle's twin: tests/test_oracle_golden.py::test_benchmark_workloads_against_the_reference)."""
    from trajectory_optimization_amd.model import ModelTraj
    d = load_reference_case("traj_full_1m_128")
    m = ModelTraj(torch.from_numpy(d["points"]), torch.from_numpy(d["poses"]), torch.from_numpy(d["quats"]), torch.from_numpy(K), IW, IH,
                  min_dist=d["clip"][0], max_dist=d["clip"][1], device=torch.device("cuda:0"), dense=dense)
    m(vis_wps_dist=0.0)
    m.loss["vis"].backward()
    torch.cuda.synchronize()
    _config2_checks(d, "dense" if dense else "culled", m.loss["vis"].item(), m.rewards.detach().cpu().numpy(), m.poses.grad.cpu().numpy(),
                    m.quats.grad.cpu().numpy())


def test_hip_dropin_loop_at_size_against_the_reference():
    """The reference's own loop body at 1 M x 128: `loss = m()` (vis_wps_dist = 0.5: every 3rd waypoint) and `loss.backward()`, against
    the reference's f32 results (make_golden.py baseline).  The total loss and each term to 1e-5; the reward samples; the visibility
    gradient (a second pass, loss['vis'].backward()) under the conditional 1e-5 bar; the total's quaternion gradient (no regulariser
    reaches it) to 1e-5.  The total's position gradient holds 1e-5 against the f64 restatement (oracle f64 visibility + the f64
    regularisers: this implementation takes the regularisers in f64), and is no farther from the reference than that restatement
    is: the reference's own f32 smoothness gradient is rounding noise on the path's nearly straight segments (1 + cos down to 1.5e-7)."""
    from oracle import oracle
    from test_hip_conditioning import BASELINE_EXCLUDED_WAYPOINTS, dropin_visibility_case, regularisers_f64
    from trajectory_optimization_amd.model import ModelTraj
    d = load_reference_case("traj_full_1m_128_dropin")
    v, idx = dropin_visibility_case(d)
    m = ModelTraj(torch.from_numpy(d["points"]), torch.from_numpy(d["poses"]), torch.from_numpy(d["quats"]), torch.from_numpy(K), IW, IH,
                  min_dist=d["clip"][0], max_dist=d["clip"][1], device=torch.device("cuda:0"))
    loss = m()
    loss.backward()
    torch.cuda.synchronize()
    assert m._wps_step(0.5) == int(d["wps_step"]) == 3
    assert abs(loss.item() - float(d["loss"])) <= 1e-5 * float(d["loss"])
    for term in ("vis", "l2", "length", "smooth"):
        ref = float(d["loss_" + term])
        assert abs(m.loss[term].item() - ref) <= 1e-5 * max(1.0, abs(ref)), term
    _reward_samples(m.rewards.detach().cpu().numpy(), d, 997)
    gp, gq = m.poses.grad.cpu().numpy().astype(np.float64), m.quats.grad.cpu().numpy()
    off = np.setdiff1d(np.arange(len(d["poses"])), idx)
    assert np.all(gq[off] == 0) and rel_inf(gq, d["quats_grad"]) < 1e-5
    f = oracle.traj_forward(v["points"], v["poses"], v["quats"], K, IW, IH, d["clip"][0], d["clip"][1], prec="f64")
    pg64, _ = oracle.traj_backward(v["points"], v["poses"], v["quats"], K, IW, IH, f, min_dist=d["clip"][0], max_dist=d["clip"][1], prec="f64")
    total64 = regularisers_f64(d["poses"])[3]
    total64[idx] += pg64
    ref = d["poses_grad"].astype(np.float64)
    assert rel_inf(gp, total64) < 1e-5
    assert (np.abs(gp - ref).max(axis=1) <= np.abs(total64 - ref).max(axis=1) + 1e-5 * np.abs(ref).max()).all()
    # the visibility term alone
    m.zero_grad()
    m()
    m.loss["vis"].backward()
    torch.cuda.synchronize()
    gvp, gvq = m.poses.grad.cpu().numpy(), m.quats.grad.cpu().numpy()
    assert np.all(gvp[off] == 0) and np.all(gvq[off] == 0)
    rep = conditional_gradient_report(v, gvp[idx], gvq[idx], MARGIN)
    excluded = BASELINE_EXCLUDED_WAYPOINTS["traj_full_1m_128_dropin"]
    assert rep["excluded_waypoints"] == excluded and rep["kept"] == len(idx) - len(excluded)
    warnings.warn(f"drop-in loop 1 M x 128 (every 3rd waypoint) against the reference: loss {abs(loss.item() / float(d['loss']) - 1):.1e} relative; "
                  f"visibility gradient: {rep['kept']} waypoints within 1e-5 (worst {rep['worst_kept']:.1e} of the largest row), {rep['excluded']} "
                  f"excluded; total positions vs the f64 restatement {rel_inf(gp, total64):.1e}, vs the reference {rel_inf(gp, ref):.1e} (the "
                  f"reference vs the f64 restatement {rel_inf(ref, total64):.1e}); total quaternions {rel_inf(gq, d['quats_grad']):.1e}")


def test_hip_config1_against_the_reference():
    """BASELINE config 1 (100 k x 32, forward only) through ops.traj_forward + ops.traj_reward, with exact culling and with ops.DENSE,
    against the reference itself (make_golden.py baseline): the two paths bitwise equal, the loss and the reward samples."""
    from trajectory_optimization_amd import ops
    d = load_reference_case("traj_config1_100k_32")
    dev = torch.device("cuda:0")
    cloud = ops.PackedCloud(torch.from_numpy(d["points"]).to(dev))
    cam = ops.Camera(K, IW, IH, d["clip"][0], d["clip"][1])
    p, q = torch.from_numpy(d["poses"]).to(dev), torch.from_numpy(d["quats"]).to(dev)
    ws = ops.TrajWorkspace(cloud, 32)
    out = {}
    for flags in (0, ops.DENSE):
        with torch.no_grad():
            lo, _ = ops.traj_forward(cloud, p, q, cam, ws, flags=flags)
            r, sc = ops.traj_reward(cloud, lo, cam, ws)
        out[flags] = (r.cpu().numpy(), sc.cpu().numpy())
    assert np.array_equal(out[0][0], out[ops.DENSE][0]) and np.array_equal(out[0][1], out[ops.DENSE][1])
    r, sc = out[0]
    assert abs(float(sc[1]) - float(d["loss_vis"])) <= 5e-6 * float(d["loss_vis"])
    _reward_samples(r, d, 97)
    warnings.warn(f"config 1 against the reference: loss {abs(float(sc[1]) / float(d['loss_vis']) - 1):.1e} relative, every 97th reward "
                  f"{np.abs(r[::97] / d['rewards_every_97th'] - 1).max():.1e}")


def test_bench_timed_step_against_the_reference(tmp_path):
    """What bench.py times and prints is the reference's answer: bench.py at its default size (1 M x 128) as a child process, its
    last timed step's outputs (--dump-outputs: written whole at this size; rewards in the caller's order, as the step's
    traj_forward_backward writes them) against traj_full_1m_128, for the dense headline and the culled path (the same scalars and rewards, bit for bit)."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = load_reference_case("traj_full_1m_128")
    out = tmp_path / "outputs"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--cpu-wps", "0", "--mode", "both",
           "--dump-outputs", str(out), "--details-file", str(tmp_path / "details.json")]
    r = subprocess.run(cmd, cwd=repo, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n---\n" + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["n_gpus"] == 1
    names = ("scalars", "poses_grad", "quats_grad", "rewards")
    assert sorted(os.listdir(out)) == sorted(f"{c}{k}.npy" for c in ("", "culled_") for k in names)   # no row samples: whole
    got = {c: [np.load(out / f"{c}{k}.npy") for k in names] for c in ("", "culled_")}
    assert np.array_equal(got[""][0], got["culled_"][0]) and np.array_equal(got[""][3], got["culled_"][3])   # scalars, rewards
    for c, what in (("", "bench.py dense headline"), ("culled_", "bench.py culled")):
        sc, pg, qg, rew = got[c]
        _config2_checks(d, what, float(sc[1]), rew, pg, qg)
