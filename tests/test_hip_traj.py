"""Parity of the HIP ModelTraj path (through the C ABI) with the golden vectors and the CPU oracle."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_inf
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu

K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
GRAD_TOL = 1e-5     # north star: gradients within 1e-5 relative (||g-g_ref||_inf / ||g_ref||_inf)
REW_RTOL, REW_ATOL = 1e-5, 0.0   # north star: rewards within 1e-5 relative (rewards live in [0.5, 1]: no absolute slack needed)
# measured (MI355X, r02): rewards 4e-7 .. 7e-7 max relative error, gradients 2e-7 .. 8e-7 against the f64 oracle


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _ops():
    from trajectory_optimization_amd import ops
    return ops


def _run_ops(dev, points, poses, quats, rig=None, flags=0, sort=True, clip=(1.0, 5.0)):
    ops = _ops()
    cloud = ops.PackedCloud(torch.from_numpy(np.ascontiguousarray(points)).to(dev), sort=sort)
    cam = ops.Camera(K, IW, IH, clip[0], clip[1])
    p = torch.from_numpy(np.ascontiguousarray(poses)).to(dev)
    q = torch.from_numpy(np.ascontiguousarray(quats)).to(dev)
    rg = ops.CameraRig(rig[0], rig[1], dev) if rig is not None else None
    ws = ops.TrajWorkspace(cloud, p.shape[0] * (rg.n_cams if rg else 1))
    lo_sum, minmax = ops.traj_forward(cloud, p, q, cam, ws, rg, flags=flags)
    rewards, scalars = ops.traj_reward(cloud, lo_sum, cam, ws)
    gout = torch.ones(1, device=dev)
    pg, qg = ops.traj_backward(cloud, p.shape[0], cam, ws, lo_sum, scalars=scalars, gout=gout, rig=rg, flags=flags)
    torch.cuda.synchronize()
    return dict(lo_sum=lo_sum[:cloud.n].cpu().numpy(), rewards=rewards.cpu().numpy(), minmax=minmax.cpu().numpy(),
                scalars=scalars.cpu().numpy(), pg=pg.cpu().numpy(), qg=qg.cpu().numpy())


def test_wave_reduce_selftest(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(0)
    m = torch.randn(64, 37, generator=g).to(dev)
    s, mn, mx = ops.selftest_wave_reduce(m)
    torch.cuda.synchronize()
    np.testing.assert_allclose(s.cpu().numpy(), m.double().sum(0).cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(mn, m.min(0).values) and torch.equal(mx, m.max(0).values)


def test_packed_cloud_is_a_permutation(dev):
    ops = _ops()
    pts = synth.make_cloud(70_001, seed=2)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    perm = cloud.perm.cpu().numpy()
    n, npad = cloud.n, cloud.npad
    assert np.array_equal(np.sort(perm[:n]), np.arange(n)) and np.all(perm[n:] == -1)
    soa = cloud.soa.cpu().numpy().reshape(3, npad)
    assert np.array_equal(soa[:, :n].T, pts[perm[:n]])
    assert np.array_equal(soa[:, n:], np.repeat(soa[:, n - 1:n], npad - n, axis=1))
    unsorted = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=False)
    assert np.array_equal(unsorted.perm.cpu().numpy()[:n], np.arange(n))


GOLD = ["traj_bundled_tilted_all", "traj_synth_1000x3", "traj_synth_10000x8", "traj_synth_20000x32",
        "traj_synth_ties", "traj_synth_ties3", "traj_synth_dense", "traj_synth_clip"]


@pytest.mark.parametrize("name", GOLD)
def test_c_abi_vs_golden(dev, name):
    d = load_golden(name)
    clip = (float(d["min_dist"]), float(d["max_dist"])) if "min_dist" in d else (1.0, 5.0)  # pc_clip_limits of the fixture
    r = _run_ops(dev, d["points"], d["poses"], d["quats"], clip=clip)
    for flags in (0, _ops().DENSE):
        assert np.array_equal(_run_ops(dev, d["points"], d["poses"], d["quats"], clip=clip, flags=flags)["pg"], r["pg"])
    assert abs(r["scalars"][1] - float(d["loss_vis"])) <= 3e-6 * float(d["loss_vis"])
    np.testing.assert_allclose(r["rewards"], d["rewards"], rtol=REW_RTOL, atol=REW_ATOL)
    assert rel_inf(r["pg"], d["vis_poses_grad"]) < GRAD_TOL
    assert rel_inf(r["qg"], d["vis_quats_grad"]) < GRAD_TOL


@pytest.mark.parametrize("name", ["traj_synth_ties", "traj_synth_ties3", "traj_synth_dense", "traj_synth_20000x32", "traj_bundled_tilted_all"])
def test_culling_is_bitwise_exact(dev, name):
    """The default path skips pairs that provably contribute nothing; TOHIP_TRAJ_DENSE evaluates every pair.
    Same bits out (fixtures incl. ties at the max and a dense cloud with min p > 0)."""
    ops = _ops()
    d = load_golden(name)
    a = _run_ops(dev, d["points"], d["poses"], d["quats"])
    b = _run_ops(dev, d["points"], d["poses"], d["quats"], flags=ops.DENSE)
    for k in ("lo_sum", "rewards", "minmax", "scalars", "pg", "qg"):
        assert np.array_equal(a[k], b[k]), k
    # caller's order is independent of the internal Morton order (sums differ only by association)
    c = _run_ops(dev, d["points"], d["poses"], d["quats"], sort=False)
    np.testing.assert_allclose(c["rewards"], a["rewards"], rtol=1e-6, atol=1e-7)
    assert rel_inf(c["pg"], a["pg"]) < 2e-6 and rel_inf(c["qg"], a["qg"]) < 2e-6


def test_culling_is_bitwise_exact_rig_and_large(dev):
    ops = _ops()
    pts = synth.make_cloud(300_000, seed=51)
    poses, quats = synth.make_path(12, optical=True, jitter_seed=51)
    rq, rt = synth.camera_rig(5)
    for rig in (None, (rq, rt)):
        a = _run_ops(dev, pts, poses, quats, rig=rig)
        b = _run_ops(dev, pts, poses, quats, rig=rig, flags=ops.DENSE)
        for k in ("lo_sum", "rewards", "minmax", "scalars", "pg", "qg"):
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("n,w,seed", [(50_000, 16, 31), (200_000, 8, 32), (600_000, 4, 33), (1_000_003, 3, 34)])
def test_c_abi_vs_oracle(dev, n, w, seed):
    """Sizes that exercise every points-per-lane variant (1, 2, 4) and a ragged last tile."""
    from oracle import oracle
    pts = synth.make_cloud(n, seed=seed)
    poses, quats = synth.make_path(w, optical=True, jitter_seed=seed)
    r = _run_ops(dev, pts, poses, quats)
    f = oracle.traj_forward(pts, poses, quats, K, IW, IH, prec="f64")
    pg, qg = oracle.traj_backward(pts, poses, quats, K, IW, IH, f, prec="f64")
    assert abs(r["scalars"][1] - f["loss_vis"]) <= 3e-6 * f["loss_vis"]
    np.testing.assert_allclose(r["rewards"], f["rewards"], rtol=REW_RTOL, atol=REW_ATOL)
    np.testing.assert_allclose(r["minmax"][:, 0], f["pmin"], rtol=1e-5, atol=1e-30)
    np.testing.assert_allclose(r["minmax"][:, 1], f["pmax"], rtol=1e-5)
    assert rel_inf(r["pg"], pg) < GRAD_TOL
    assert rel_inf(r["qg"], qg) < GRAD_TOL


def test_rig_equals_explicit_virtual_waypoints(dev):
    """A C-camera rig == the same cameras written out as W*C independent waypoints (rewards), and the body
    gradient == the chain rule through the composition (checked against finite differences of the oracle)."""
    from oracle import oracle
    pts = synth.make_cloud(30_000, seed=41)
    poses, quats = synth.make_path(4, optical=True, jitter_seed=41)
    rq, rt = synth.camera_rig(3)
    rt = rt + np.array([[0.1, 0.0, 0.2], [0.0, 0.15, 0.2], [-0.1, 0.0, 0.25]], dtype=np.float32)
    r = _run_ops(dev, pts, poses, quats, rig=(rq, rt))

    def virtual(poses, quats):
        qn = quats.astype(np.float64) / np.linalg.norm(quats.astype(np.float64), axis=1, keepdims=True)
        vq = synth.quat_mul(qn[:, None, :], rq[None].astype(np.float64)).reshape(-1, 4)
        R = np.stack([_rot(q) for q in qn])
        vt = (poses.astype(np.float64)[:, None, :] + np.einsum("wij,cj->wci", R, rt.astype(np.float64))).reshape(-1, 3)
        return vt.astype(np.float32), vq.astype(np.float32)

    vt, vq = virtual(poses, quats)
    f = oracle.traj_forward(pts, vt, vq, K, IW, IH, prec="f64")
    np.testing.assert_allclose(r["rewards"], f["rewards"], rtol=5e-5, atol=5e-6)
    assert abs(r["scalars"][1] - f["loss_vis"]) <= 1e-5 * f["loss_vis"]
    # body-pose gradient by central differences of the oracle's loss (coarse: 2e-2 relative)
    h = 1e-3
    for (wi, ci) in [(0, 0), (2, 1), (3, 2)]:
        pp, pm = poses.copy(), poses.copy()
        pp[wi, ci] += h
        pm[wi, ci] -= h
        lp = oracle.traj_forward(pts, *virtual(pp, quats), K, IW, IH, prec="f64")["loss_vis"]
        lm = oracle.traj_forward(pts, *virtual(pm, quats), K, IW, IH, prec="f64")["loss_vis"]
        fd = (lp - lm) / (2 * h)
        assert abs(r["pg"][wi, ci] - fd) <= 0.05 * np.abs(r["pg"]).max() + 1e-7


def _rot(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def test_full_size_properties(dev):
    """BASELINE.json config 3 (1 M x 128): size-independent properties."""
    ops = _ops()
    n, w = 1_000_000, 128
    pts = synth.make_cloud(n, seed=0)
    poses, quats = synth.make_path(w, optical=True)
    r1 = _run_ops(dev, pts, poses, quats)
    r2 = _run_ops(dev, pts, poses, quats)
    r3 = _run_ops(dev, pts, poses, quats, flags=ops.DENSE)
    # deterministic: fixed-order reductions, bitwise reproducible; exact culling == dense evaluation
    for k in ("rewards", "pg", "qg", "scalars", "minmax"):
        assert np.array_equal(r1[k], r2[k]), k
        assert np.array_equal(r1[k], r3[k]), k
    # every log-odds term is >= 0, so rewards live in [0.5, 1] (f32 sigmoid saturates to exactly 1)
    assert r1["rewards"].min() >= 0.5 and r1["rewards"].max() <= 1.0
    assert 0.5 < r1["rewards"].mean() < 0.9
    assert np.isfinite(r1["pg"]).all() and np.isfinite(r1["qg"]).all() and np.abs(r1["pg"]).max() > 0
    # additivity of the log-odds over waypoint shards (what the multi-GPU all-reduce relies on)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    cam = ops.Camera(K, IW, IH)
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    ws = ops.TrajWorkspace(cloud, 64)
    a, _ = ops.traj_forward(cloud, p[:64].contiguous(), q[:64].contiguous(), cam, ws)
    a = a.clone()
    b, _ = ops.traj_forward(cloud, p[64:].contiguous(), q[64:].contiguous(), cam, ws)
    np.testing.assert_allclose((a + b)[:n].cpu().numpy(), r1["lo_sum"], rtol=1e-5, atol=1e-5)
    # quaternion gradient is tangent to the unit sphere: <q, dL/dq> = 0 (F.normalize)
    dots = (quats.astype(np.float64) * r1["qg"]).sum(1)
    assert np.abs(dots).max() <= 1e-5 * np.abs(r1["qg"]).max()
    # parity against the f64 oracle at the full size: all 128 waypoints, rewards and gradients
    from oracle import oracle
    f = oracle.traj_forward(pts, poses, quats, K, IW, IH, prec="f64")
    pg, qg = oracle.traj_backward(pts, poses, quats, K, IW, IH, f, prec="f64")
    rew_err = float(np.abs(r1["rewards"] - f["rewards"]).max() / 0.5)
    print(f"1M x 128 vs f64 oracle: rewards max rel err {rew_err:.2e}, poses grad {rel_inf(r1['pg'], pg):.2e}, "
          f"quats grad {rel_inf(r1['qg'], qg):.2e}, loss_vis {abs(r1['scalars'][1] - f['loss_vis']) / f['loss_vis']:.2e}")
    np.testing.assert_allclose(r1["rewards"], f["rewards"], rtol=REW_RTOL, atol=REW_ATOL)
    assert abs(r1["scalars"][1] - f["loss_vis"]) <= 1e-6 * f["loss_vis"]
    assert rel_inf(r1["pg"], pg) < GRAD_TOL and rel_inf(r1["qg"], qg) < GRAD_TOL


@pytest.mark.parametrize("seed", list(range(12)))
def test_culling_randomized_bitwise(dev, seed):
    """Random clouds (uniform slabs, clustered blobs, thin walls), random paths and cameras: exact culling must
    reproduce the dense evaluation bit for bit (the tile bounds and distance bounds are conservative)."""
    ops = _ops()
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([300, 5_000, 40_000, 150_000, 600_000]))
    kind = seed % 3
    if kind == 0:
        pts = (rng.random((n, 3)) * rng.uniform(5, 60, 3) - rng.uniform(2, 30, 3)).astype(np.float32)
    elif kind == 1:
        centres = rng.uniform(-15, 15, (6, 3))
        pts = (centres[rng.integers(0, 6, n)] + rng.standard_normal((n, 3)) * rng.uniform(0.05, 2.0)).astype(np.float32)
    else:
        pts = np.stack([rng.uniform(-20, 20, n), rng.uniform(-0.02, 0.02, n) + 4.0, rng.uniform(-3, 3, n)], 1).astype(np.float32)
    w = int(rng.integers(3, 40))
    poses = rng.uniform(-8, 8, (w, 3)).astype(np.float32)
    quats = rng.standard_normal((w, 4)).astype(np.float32)
    a = _run_ops(dev, pts, poses, quats)
    b = _run_ops(dev, pts, poses, quats, flags=ops.DENSE)
    for k in ("lo_sum", "rewards", "minmax", "scalars", "pg", "qg"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, n, w)


def _setup(dev, n, w, cams=1, occ=False, seed=5, dense=False):
    ops = _ops()
    pts = synth.make_cloud(n, seed=seed)
    poses, quats = synth.make_path(w, optical=True, jitter_seed=seed - 1)
    P = torch.from_numpy(pts).to(dev)
    cloud = ops.PackedCloud(P)
    cam = ops.Camera(K, IW, IH)
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    rg = ops.CameraRig(*synth.camera_rig(cams), dev) if cams > 1 else None
    ws = ops.TrajWorkspace(cloud, w * cams)
    bits = ops.occlusion_bits(cloud, P, p, q, cam, 1.0, 15.0, "zbuffer") if occ else None
    return dict(pts=pts, poses=poses, quats=quats, cloud=cloud, cam=cam, p=p, q=q, rig=rg, ws=ws, occ=bits,
                flags=ops.DENSE if dense else 0)


@pytest.mark.parametrize("n,w,cams,occ", [(1_000_000, 24, 1, False), (200_000, 70, 1, True), (60_000, 9, 3, False), (3000, 5, 1, False),
                                         (300_000, 130, 1, False)])
def test_backward_paths_and_modes_agree_bitwise(dev, n, w, cams, occ):
    """Culled == dense, bit for bit, for the fused visibility loss and for a general dL/d rewards vector: rig, occlusion bits,
    more than 64 and more than 128 waypoints (flag words), ragged sizes; and the backward is a pure function of the forward's
    state (called twice: same bits)."""
    ops = _ops()
    out = []
    for dense in (False, True):
        c = _setup(dev, n, w, cams, occ, dense=dense)
        lo_sum, minmax = ops.traj_forward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], c["rig"], flags=c["flags"], occ=c["occ"])
        rewards, scalars = ops.traj_reward(c["cloud"], lo_sum, c["cam"], c["ws"])
        gout = torch.ones(1, device=dev)
        g = torch.rand(n, generator=torch.Generator().manual_seed(2)).to(dev) - 0.3
        res = [lo_sum, minmax, rewards, scalars]
        for kw in (dict(scalars=scalars, gout=gout), dict(grad_rewards=g)):
            a = ops.traj_backward(c["cloud"], w, c["cam"], c["ws"], lo_sum, rig=c["rig"], flags=c["flags"], occ=c["occ"], **kw)
            b = ops.traj_backward(c["cloud"], w, c["cam"], c["ws"], lo_sum, rig=c["rig"], flags=c["flags"], occ=c["occ"], **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert bool(torch.isfinite(a[0]).all()) and float(a[0].abs().max()) > 0
            res += [a[0], a[1]]
        out.append(res)
    for x, y in zip(out[0], out[1]):
        assert torch.equal(x, y)


def test_general_grad_rewards_matches_the_fused_loss(dev):
    """dL/d rewards = d loss_vis / d rewards handed over as a vector == the fused path (same arithmetic, same bits apart
    from the host-side product), and a scaled upstream gradient scales the result."""
    ops = _ops()
    c = _setup(dev, 120_000, 20)
    lo_sum, _ = ops.traj_forward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"])
    rewards, scalars = ops.traj_reward(c["cloud"], lo_sum, c["cam"], c["ws"])
    fused = ops.traj_backward(c["cloud"], 20, c["cam"], c["ws"], lo_sum, scalars=scalars, gout=torch.ones(1, device=dev))
    g = torch.full((120_000,), float(scalars[2]), device=dev)
    general = ops.traj_backward(c["cloud"], 20, c["cam"], c["ws"], lo_sum, grad_rewards=g)
    assert rel_inf(general[0].cpu().numpy(), fused[0].cpu().numpy()) < 1e-6
    assert rel_inf(general[1].cpu().numpy(), fused[1].cpu().numpy()) < 1e-6
    twice = ops.traj_backward(c["cloud"], 20, c["cam"], c["ws"], lo_sum, scalars=scalars, gout=torch.full((1,), 2.0, device=dev))
    assert rel_inf(twice[0].cpu().numpy(), 2 * fused[0].cpu().numpy()) < 1e-6


@pytest.mark.parametrize("copies", [3, 5, 40])
def test_tie_sets_are_deterministic_and_split_evenly(dev, copies):
    """torch splits the gradient of min()/max() evenly among tied elements (model.py:226-227).  A cloud whose argmax (and,
    for a compact cloud with min p > 0, argmin) points exist in `copies` exact copies: the gradients are the oracle's
    (which implements that rule), identical from run to run and between the two modes — there are no float atomics on the
    path — including more tied rows than the select kernel records (40 copies spread by the Morton sort)."""
    from oracle import oracle
    ops = _ops()
    base = (synth.make_cloud(6000, seed=77) * np.float32(0.3)).astype(np.float32)   # compact: min p > 0 at some waypoints
    poses, quats = synth.make_path(5, optical=True, jitter_seed=77)
    f0 = oracle.traj_forward(base, poses, quats, K, IW, IH, prec="f64")
    # replicate, for every waypoint, its argmax and argmin points
    extra = []
    for v in range(5):
        pv = oracle.pose_forward(base, poses[v], quats[v], K, IW, IH, prec="f64")[0]   # p of every point for waypoint v
        extra += [base[int(np.argmax(pv))]] * (copies - 1) + [base[int(np.argmin(pv))]] * (copies - 1)
    pts = np.concatenate([base, np.asarray(extra, np.float32)])
    rng = np.random.default_rng(0)
    pts = pts[rng.permutation(len(pts))]
    f = oracle.traj_forward(pts, poses, quats, K, IW, IH, prec="f64")
    pg, qg = oracle.traj_backward(pts, poses, quats, K, IW, IH, f, prec="f64")
    assert (f0["pmin"] > 0).any()
    runs = [_run_ops(dev, pts, poses, quats, flags=fl) for fl in (0, 0, ops.DENSE)]
    for k in ("pg", "qg", "rewards"):
        assert np.array_equal(runs[0][k], runs[1][k]) and np.array_equal(runs[0][k], runs[2][k]), k
    assert rel_inf(runs[0]["pg"], pg) < GRAD_TOL and rel_inf(runs[0]["qg"], qg) < GRAD_TOL


def test_more_tie_slots_than_recorded_on_a_used_workspace(dev):
    """The extremum in more slots than a waypoint's tie record holds (2 500 exact copies of its argmax point: ten slots) sends the
    finish kernel through every slot's (min, max) of that waypoint.  In the culled mode the pairs pass 1 did not evaluate are not
    written at all — whatever an earlier step at other poses left there must not be looked at: a workspace that has seen other
    poses gives the bits of a fresh one, and those of the dense mode."""
    from oracle import oracle
    ops = _ops()
    base = synth.make_cloud(60_000, seed=21)
    poses, quats = synth.make_path(6, optical=True, jitter_seed=21)
    pv = oracle.pose_forward(base, poses[2], quats[2], K, IW, IH, prec="f64")[0]
    pts = np.concatenate([base, np.repeat(base[int(np.argmax(pv))][None], 2500, 0)]).astype(np.float32)
    pts = pts[np.random.default_rng(1).permutation(len(pts))]
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    cam = ops.Camera(K, IW, IH)
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    gout = torch.ones(1, device=dev)
    fresh = ops.traj_forward_backward(cloud, p, q, cam, ops.TrajWorkspace(cloud, 6), gout, flags=0)
    dense = ops.traj_forward_backward(cloud, p, q, cam, ops.TrajWorkspace(cloud, 6), gout, flags=ops.DENSE)
    used = ops.TrajWorkspace(cloud, 6)
    for shift in (3.0, -4.0, 1.5):   # other poses first: every slot near them gets written
        ops.traj_forward_backward(cloud, p + torch.tensor([shift, -shift, 0.0], device=dev), q, cam, used, gout, flags=0)
    again = ops.traj_forward_backward(cloud, p, q, cam, used, gout, flags=0)
    for a, b, c in zip(fresh[:5], dense[:5], again[:5]):
        assert torch.equal(a, b) and torch.equal(a, c)
    f = oracle.traj_forward(pts, poses, quats, K, IW, IH, prec="f64")
    pg, qg = oracle.traj_backward(pts, poses, quats, K, IW, IH, f, prec="f64")
    assert rel_inf(fresh[2].cpu().numpy(), pg) < GRAD_TOL and rel_inf(fresh[3].cpu().numpy(), qg) < GRAD_TOL


def test_workspace_state_contract(dev):
    """The backward reads the state its forward left in the workspace, not the Parameters: an optimizer step (an in-place edit)
    between model() and backward() changes nothing.  ModelTraj notices when another forward has used the workspace in between
    and rebuilds the state from the (unchanged) inputs: gradients of the first loss are the same either way.  Both at once —
    another forward AND edited inputs — cannot be served and raises."""
    from trajectory_optimization_amd.model import ModelTraj
    pts = synth.make_cloud(30_000, seed=9)
    poses, quats = synth.make_path(6, optical=True, jitter_seed=9)
    def grads(second_forward, edit, fast=True):
        m = ModelTraj(torch.from_numpy(pts), torch.from_numpy(poses), torch.from_numpy(quats), torch.from_numpy(K), IW, IH, device=dev)
        m.fast_backward = fast
        loss = m(vis_wps_dist=0.0)
        if second_forward:
            m(vis_wps_dist=0.0)
        if edit:
            with torch.no_grad():
                m.poses.add_(0.05)
                m.quats.mul_(1.5)
        loss.backward()
        return m.poses.grad.clone(), m.quats.grad.clone()
    a = grads(False, False)
    for fast in (True, False):
        for b in (grads(True, False, fast), grads(False, True, fast)):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        with pytest.raises(RuntimeError, match="inplace"):
            grads(True, True, fast)


@pytest.mark.parametrize("seed", range(10))
def test_modes_agree_on_random_configs(dev, seed):
    """Random clouds (compact ones with min p > 0 included), paths, rigs, clip limits, unsorted packing, duplicated points:
    culled == dense, bit for bit.  (tools/stress_bitwise.py runs more of the same.)"""
    ops = _ops()
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([700, 5000, 40_000, 140_000, 300_000]))
    cams = int(rng.choice([1, 1, 2, 5]))
    w = max(1, int(rng.integers(1, 90)) // cams)
    scale = float(rng.choice([0.3, 0.3, 1.0, 2.5]))  # 0.3: everything in front of the cameras -> min p > 0 at some waypoints
    pts = (synth.make_cloud(n, seed=int(rng.integers(1 << 30))) * np.float32(scale)).astype(np.float32)
    if rng.random() < 0.4:
        pts = np.concatenate([pts, pts[: n // 5]])
    poses, quats = synth.make_path(w, optical=True, jitter_seed=int(rng.integers(1 << 30)))
    quats = (quats * np.float32(rng.uniform(0.5, 2.0))).astype(np.float32)
    P = torch.from_numpy(pts).to(dev)
    cloud = ops.PackedCloud(P, sort=bool(rng.random() < 0.8))
    cam = ops.Camera(K, IW, IH, float(rng.uniform(0.2, 2.0)), float(rng.uniform(3.0, 12.0)))
    p, q = torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev)
    rg = ops.CameraRig(*synth.camera_rig(cams), dev) if cams > 1 else None
    ws = ops.TrajWorkspace(cloud, w * cams)
    gout = torch.ones(1, device=dev)

    def same(x, y):
        return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))

    grads = []
    for flags in (0, ops.DENSE):
        lo, mm = ops.traj_forward(cloud, p, q, cam, ws, rg, flags=flags)
        rew, sc = ops.traj_reward(cloud, lo, cam, ws)
        pg, qg = ops.traj_backward(cloud, w, cam, ws, lo, rig=rg, flags=flags, scalars=sc, gout=gout)
        grads.append((lo.clone(), mm.clone(), rew, pg, qg))
    for a, b in zip(grads[0], grads[1]):
        assert same(a, b)  # culled == dense


@pytest.mark.parametrize("n,w", [(1_000_003, 9), (70_001, 33), (300, 2)])
def test_prefilled_rewards_equal_the_scattered_ones(dev, n, w):
    """tohip_traj_forward can fill the rewards vector with sigmoid(0) = 0.5 on its way, after which tohip_traj_reward only
    stores the points with a non-zero log-odds: same rewards and the same mean / loss, bit for bit, as the plain call."""
    ops = _ops()
    c = _setup(dev, n, w)
    lo_a, _ = ops.traj_forward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"])
    rew_a, sc_a = ops.traj_reward(c["cloud"], lo_a, c["cam"], c["ws"])
    half = torch.full((n,), -7.0, device=dev)
    lo_b, _ = ops.traj_forward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], rewards_half=half)
    assert bool((half == 0.5).all())
    rew_b, sc_b = ops.traj_reward(c["cloud"], lo_b, c["cam"], c["ws"], rewards=half, prefilled=True)
    assert torch.equal(lo_a, lo_b) and torch.equal(rew_a, rew_b) and torch.equal(sc_a, sc_b)
    assert float(rew_a.min()) >= 0.5 and float(rew_a.max()) > 0.5
    # the mean is the f64 mean of the rewards
    assert abs(float(sc_a[0]) - float(rew_a.double().mean())) <= 1e-7


@pytest.mark.parametrize("name", ["traj_synth_20000x32", "traj_synth_ties3", "traj_bundled_tilted_all"])
def test_fused_reward_backward_equals_the_two_calls(dev, name):
    """tohip_traj_reward_backward: rewards + scalars in the backward's first launch.  rewards / scalars bitwise those of
    tohip_traj_reward; the gradients those of tohip_traj_backward to rounding (dL/d reward applied per waypoint in f64 instead
    of per point in f32)."""
    ops = _ops()
    d = load_golden(name)
    cloud = ops.PackedCloud(torch.from_numpy(d["points"]).to(dev))
    cam = ops.Camera(K, IW, IH)
    p = torch.from_numpy(d["poses"]).to(dev)   # (these fixtures evaluate every waypoint)
    q = torch.from_numpy(d["quats"]).to(dev)
    ws = ops.TrajWorkspace(cloud, p.shape[0])
    gout = torch.tensor([0.7], device=dev)
    for flags in (0, ops.DENSE):
        half = torch.empty(cloud.n, device=dev)
        lo, _ = ops.traj_forward(cloud, p, q, cam, ws, flags=flags, rewards_half=half)
        rew, sc = ops.traj_reward(cloud, lo, cam, ws, rewards=half.clone(), prefilled=True)
        pg, qg = ops.traj_backward(cloud, p.shape[0], cam, ws, lo, scalars=sc, gout=gout, flags=flags)
        rew2, sc2, pg2, qg2 = ops.traj_reward_backward(cloud, p.shape[0], cam, ws, lo, gout, rewards=half, prefilled=True, flags=flags)
        assert torch.equal(rew, rew2) and torch.equal(sc, sc2)
        assert rel_inf(pg2.cpu().numpy(), pg.cpu().numpy()) < 1e-6 and rel_inf(qg2.cpu().numpy(), qg.cpu().numpy()) < 1e-6
    # dense and culled agree bitwise through the fused entry point too
    outs = []
    for flags in (0, ops.DENSE):
        lo, _ = ops.traj_forward(cloud, p, q, cam, ws, flags=flags)
        outs.append(ops.traj_reward_backward(cloud, p.shape[0], cam, ws, lo, gout, flags=flags))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("n,w,cams,occ", [(200_000, 70, 1, True), (60_000, 9, 3, False), (300_000, 130, 1, False)])
def test_fused_reward_backward_with_rig_and_occlusion(dev, n, w, cams, occ):
    """tohip_traj_reward_backward on the cases the fixtures do not have: occlusion rows, a camera rig (k_traj_bwd_finish2),
    more than 128 waypoints; against the two separate calls and the f64 oracle."""
    from oracle import oracle
    ops = _ops()
    c = _setup(dev, n, w, cams, occ)
    gout = torch.tensor([1.0], device=dev)
    lo, _ = ops.traj_forward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], c["rig"], occ=c["occ"])
    rew, sc = ops.traj_reward(c["cloud"], lo, c["cam"], c["ws"])
    pg, qg = ops.traj_backward(c["cloud"], w, c["cam"], c["ws"], lo, scalars=sc, gout=gout, rig=c["rig"], occ=c["occ"])
    rew2, sc2, pg2, qg2 = ops.traj_reward_backward(c["cloud"], w, c["cam"], c["ws"], lo, gout, rig=c["rig"], occ=c["occ"])
    assert torch.equal(rew, rew2) and torch.equal(sc, sc2)
    assert rel_inf(pg2.cpu().numpy(), pg.cpu().numpy()) < 1e-6 and rel_inf(qg2.cpu().numpy(), qg.cpu().numpy()) < 1e-6
    if cams == 1 and not occ:
        f = oracle.traj_forward(c["pts"], c["poses"], c["quats"], K, IW, IH, prec="f64")
        pgo, qgo = oracle.traj_backward(c["pts"], c["poses"], c["quats"], K, IW, IH, f, prec="f64")
        assert rel_inf(pg2.cpu().numpy(), pgo) < GRAD_TOL and rel_inf(qg2.cpu().numpy(), qgo) < GRAD_TOL


@pytest.mark.parametrize("n,w,cams,occ", [(200_000, 70, 1, True), (60_000, 9, 3, False), (300_000, 130, 1, False), (3000, 5, 1, False),
                                          (1_000_003, 17, 1, False)])
def test_fused_step_equals_the_split_calls(dev, n, w, cams, occ):
    """tohip_traj_forward_backward (four launches, no collective between forward and backward): log-odds, minmax, rewards and
    scalars are bitwise those of tohip_traj_forward + tohip_traj_reward (the reward sum is an integer sum: no order to depend
    on); the gradients those of tohip_traj_backward to rounding (the dL/d reward factor is applied per waypoint in f64 instead
    of per point in f32).  Dense and culled agree bitwise through it; two runs agree bitwise."""
    ops = _ops()
    c = _setup(dev, n, w, cams, occ)
    gout = torch.tensor([0.7], device=dev)
    outs = []
    for flags in (0, ops.DENSE):
        half = torch.empty(c["cloud"].n, device=dev)
        lo, mm = ops.traj_forward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], c["rig"], flags=flags, occ=c["occ"], rewards_half=half)
        rew, sc = ops.traj_reward(c["cloud"], lo, c["cam"], c["ws"], rewards=half, prefilled=True)
        pg, qg = ops.traj_backward(c["cloud"], w, c["cam"], c["ws"], lo, scalars=sc, gout=gout, rig=c["rig"], flags=flags, occ=c["occ"])
        lo, mm = lo.clone(), mm.clone()
        f = ops.traj_forward_backward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], gout, rig=c["rig"], flags=flags, occ=c["occ"])
        assert torch.equal(f[0], rew) and torch.equal(f[1], sc) and torch.equal(f[4][:c["cloud"].n], lo[:c["cloud"].n]) and torch.equal(f[5], mm)
        assert rel_inf(f[2].cpu().numpy(), pg.cpu().numpy()) < 1e-6 and rel_inf(f[3].cpu().numpy(), qg.cpu().numpy()) < 1e-6
        g = ops.traj_forward_backward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], gout, rig=c["rig"], flags=flags, occ=c["occ"])
        assert all(torch.equal(a, b) for a, b in zip(f[:4], g[:4]))
        outs.append(f)
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:4], outs[1][:4]))


def test_fused_step_of_several_trajectories_equals_single_calls(dev):
    """tohip_traj_forward_backward_multi: each trajectory's rewards, scalars and gradient rows are, bit for bit, those of a call
    with that trajectory alone."""
    ops = _ops()
    pts = synth.make_cloud(120_000, seed=21)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    cam = ops.Camera(K, IW, IH)
    lens = [7, 19, 3]
    ps, qs = [], []
    for i, n in enumerate(lens):
        p, q = synth.make_path(n, optical=True, jitter_seed=40 + i)
        p[:, 1] += 0.7 * i
        ps.append(p); qs.append(q)
    P, Q = torch.from_numpy(np.concatenate(ps)).to(dev), torch.from_numpy(np.concatenate(qs)).to(dev)
    toff = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
    gout = torch.tensor([1.0, 0.5, 2.0], device=dev)
    ws = ops.TrajWorkspace(cloud, sum(lens), len(lens))
    rew, sc, pg, qg, lo, mm = ops.traj_forward_backward(cloud, P, Q, cam, ws, gout, traj_offsets=toff)
    o = 0
    for b, n in enumerate(lens):
        ws1 = ops.TrajWorkspace(cloud, n)
        r1, s1, pg1, qg1, lo1, mm1 = ops.traj_forward_backward(cloud, P[o:o + n].contiguous(), Q[o:o + n].contiguous(), cam, ws1, gout[b:b + 1])
        assert torch.equal(rew[b], r1) and torch.equal(sc[b], s1) and torch.equal(lo[b, :cloud.n], lo1[:cloud.n]) and torch.equal(mm[o:o + n], mm1)
        assert torch.equal(pg[o:o + n], pg1) and torch.equal(qg[o:o + n], qg1)
        o += n
