"""The wide dense pass 1 (csrc/traj_kernels.hip: k_traj_pass1_dense16): a lane owns sixteen points, a row of 16 lanes one slot,
a block 4096 points while the padded cloud is a multiple of 2048 — the last point block may be half present.  The host routes a
DENSE launch without occlusion bits to it when the (point block, waypoint) range is long enough for its resident grid; the
kernel's clock stamps carry bit 8 in their XCC word, which is how each case here proves which kernel it ran.  The culled step is
unchanged and is the twin: every output of DENSE equals it bit for bit."""
import numpy as np
import pytest
import torch

from conftest import rel_inf
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu

K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
WIDE_V = (517, 1029, 2053)   # waypoint counts tried in turn: the first one the host routes wide is used
KEYS = ("rewards", "scalars", "pg", "qg", "lo_sum", "minmax")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _problem(dev, pts, poses, quats, n_traj=1):
    from trajectory_optimization_amd import ops
    pts = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    cloud = ops.PackedCloud(pts)
    return dict(cloud=cloud, cam=ops.Camera(K, IW, IH), p=torch.from_numpy(poses).to(dev), q=torch.from_numpy(quats).to(dev),
                ws=ops.TrajWorkspace(cloud, poses.shape[0], n_traj))


def _step(c, flags, gout=None, traj_offsets=None):
    from trajectory_optimization_amd import ops
    gout = torch.ones(1, device=c["p"].device) if gout is None else gout
    o = ops.traj_forward_backward(c["cloud"], c["p"], c["q"], c["cam"], c["ws"], gout, flags=flags, traj_offsets=traj_offsets)
    torch.cuda.synchronize()
    out = dict(zip(KEYS, (t.cpu().numpy() for t in o)))
    out["lo_sum"] = out["lo_sum"][..., :c["cloud"].n]
    return out


def _stamped_xcc_words(dev, c, **kw):
    """The XCC words of one DENSE step's clock stamps, the grid the host says it launches, and the step's outputs."""
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    nb = int(L.tohip_profile_clock_blocks(c["cloud"].n, c["p"].shape[0], ops.DENSE, 0))
    assert nb > 0
    cap = max(2 * nb, 8 * torch.cuda.get_device_properties(dev).multi_processor_count + 1)   # (as tests/test_hip_dense_residency.py)
    buf = torch.zeros(6 * cap, dtype=torch.int64, device=dev)
    L.tohip_profile_clock(buf.data_ptr())
    try:
        out = _step(c, ops.DENSE, **kw)
    finally:
        L.tohip_profile_clock(None)
    raw = buf.cpu().numpy()
    assert not raw[6 * nb:].any(), "the launch stamped more blocks than tohip_profile_clock_blocks answers"
    ext = raw[2 * nb:6 * nb].reshape(nb, 4)
    assert (ext[:, 1] != 0).all(), "fewer blocks stamped than tohip_profile_clock_blocks answers"
    return ext[:, 3], nb, out


def _wide_case(dev, pts, path=None, **kw):
    """The first waypoint count of WIDE_V for which the host routes this cloud's DENSE step to the wide kernel (bit 8 of every
    block's XCC word set): -> (problem, grid, DENSE outputs of that stamped step, path)."""
    for V in WIDE_V:
        poses, quats = path(V) if path is not None else synth.make_path(V, optical=True, jitter_seed=7)
        c = _problem(dev, pts, poses, quats)
        xcc, nb, out = _stamped_xcc_words(dev, c, **kw)
        if (xcc & 0x100).all():
            return c, nb, out, (poses, quats)
        assert not (xcc & 0x100).any(), "one launch, two kernels?"
    pytest.fail(f"the host routes none of V = {WIDE_V} to the wide kernel for {len(pts)} points")


def _assert_dense_equals_culled(c, dense, **kw):
    culled = _step(c, 0, **kw)
    assert np.isfinite(dense["pg"]).all() and np.abs(dense["pg"]).max() > 0
    for key in KEYS:
        assert np.array_equal(dense[key].view(np.uint32), culled[key].view(np.uint32)), key


# 6 139: three 2 048-point blocks, the second wide block half present; 300: one partial block, rows beyond the last slot;
# 4 096 / 4 097: exactly one wide block, and one point past it; 10 000: three wide blocks (the last half present) whose
# (point block, waypoint) range the grid does not divide — pieces start inside one point block and end in the next
@pytest.mark.parametrize("n", [6_139, 300, 4_096, 4_097, 10_000])
def test_wide_dense_equals_culled_bitwise(dev, n):
    c, nb, dense, _ = _wide_case(dev, synth.make_cloud(n, seed=11))
    if n == 10_000:
        units = -(-c["cloud"].npad // 4096) * c["p"].shape[0]
        assert units % nb != 0 and units > nb, (units, nb)
    _assert_dense_equals_culled(c, dense)


def _near_path(V):
    return synth.make_path(V, optical=True, jitter_seed=9, scale=0.02)   # 0.4 m from end to end


def test_wide_dense_minimum_path_and_oracle(dev):
    """500 points within half a metre of a short path, in a ball of 12 cm just ahead of its end where every camera sees them (a
    point beside or behind a camera underflows): no p underflows (f32 oracle: min p of a waypoint is 0.012 .. 0.040), the probe
    exhibits no zero and every waypoint takes the minimum path (row_min16_nn behind U != 0).  Also against the f64 oracle at the
    bars of tests/test_hip_traj.py."""
    from oracle import oracle
    rng = np.random.default_rng(13)
    d = rng.standard_normal((500, 3))
    d *= (0.12 * rng.random((500, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)   # uniform in a ball of radius 0.12 m
    end = synth.make_path(2, optical=True, scale=0.02)[0][-1].astype(np.float64)
    pts = (end + np.array([0.35, 0.0, 0.0]) + d).astype(np.float32)
    c, _, dense, (poses, quats) = _wide_case(dev, pts, path=_near_path)
    gap = np.linalg.norm(pts[:, None, :].astype(np.float64) - poses[None].astype(np.float64), axis=2).min(1)
    assert gap.max() < 0.5
    assert (dense["minmax"][:, 0] > 0).all()
    _assert_dense_equals_culled(c, dense)
    f = oracle.traj_forward(pts, poses, quats, K, IW, IH, prec="f64")
    pg, qg = oracle.traj_backward(pts, poses, quats, K, IW, IH, f, prec="f64")
    assert abs(dense["scalars"][1] - f["loss_vis"]) <= 3e-6 * f["loss_vis"]
    np.testing.assert_allclose(dense["rewards"], f["rewards"], rtol=1e-5, atol=0.0)
    np.testing.assert_allclose(dense["minmax"][:, 0], f["pmin"], rtol=1e-5, atol=1e-30)
    np.testing.assert_allclose(dense["minmax"][:, 1], f["pmax"], rtol=1e-5)   # (the oracle's pmax is the normaliser M = max p - min p)
    assert rel_inf(dense["pg"], pg) < 1e-5 and rel_inf(dense["qg"], qg) < 1e-5


def test_wide_dense_two_trajectories_equal_their_runs_alone(dev):
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(6_139, seed=17)
    c, _, _, (poses, quats) = _wide_case(dev, pts)
    V = poses.shape[0]
    lens = [V - 200, 200]
    poses = poses.copy()
    poses[lens[0]:, 1] += 0.7
    both = _problem(dev, pts, poses, quats, n_traj=2)
    toff = torch.tensor([0, lens[0], V], dtype=torch.int32, device=dev)
    gout = torch.tensor([1.0, 0.5], device=dev)
    xcc, _, dense = _stamped_xcc_words(dev, both, gout=gout, traj_offsets=toff)
    assert (xcc & 0x100).all()
    _assert_dense_equals_culled(both, dense, gout=gout, traj_offsets=toff)
    o = 0
    for b, w in enumerate(lens):
        one = _problem(dev, pts, poses[o:o + w].copy(), quats[o:o + w].copy())
        alone = _step(one, ops.DENSE, gout=gout[b:b + 1])
        for key, a in (("rewards", dense["rewards"][b]), ("scalars", dense["scalars"][b]), ("lo_sum", dense["lo_sum"][b]),
                       ("minmax", dense["minmax"][o:o + w]), ("pg", dense["pg"][o:o + w]), ("qg", dense["qg"][o:o + w])):
            assert np.array_equal(a.view(np.uint32), alone[key].view(np.uint32)), (b, key)
        o += w


def test_a_short_range_keeps_the_narrow_kernel(dev):
    """50 000 x 37: about one of the wide kernel's (point block, waypoint) pairs per resident block — latency-bound, routed narrow."""
    poses, quats = synth.make_path(37, optical=True, jitter_seed=7)
    c = _problem(dev, synth.make_cloud(50_000, seed=11), poses, quats)
    xcc, _, dense = _stamped_xcc_words(dev, c)
    assert not (xcc & 0x100).any()
    _assert_dense_equals_culled(c, dense)
