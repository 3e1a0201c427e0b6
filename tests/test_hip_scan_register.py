"""Scan registration on the GPU (scanreg_kernels.hip, DESIGN.md 10 "Scan registration"): every comparison is bit for bit against the
restatements of synth.py — the integer records of the normal kernel over grids of partial bricks and of one voxel, scans of one
point to more than a tile and, once, 2^22 points at the sums' bound; the f64 step on crafted records; whole registrations after 1,
2, 5 and 30 iterations — and a batch against its single runs."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import contract_cases as cc
import scan_match_cases as sc
import scan_register_cases as rc
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOM = (sc.ROOM["origin"], sc.ROOM["resolution"])
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _map(dev, L, origin=sc.ORIGIN, res=sc.RES):
    from trajectory_optimization_amd import ops
    m = ops.EvidenceMap(origin, res, L.shape, device=dev, **sc.PARAMS)
    return m.load(torch.from_numpy(np.array(L)))   # (a copy: the shared room is read-only)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)   # (a copy: the shared cases are read-only)


@pytest.fixture(scope="module")
def room(dev):
    """-> (matcher of the room, its scan on the device, L, the scan on the host)."""
    from trajectory_optimization_amd import ops
    L, P = rc.room()
    return ops.ScanMatcher(_map(dev, L, *ROOM)), _t(P, dev), L, P


# ---- the normal kernel ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [cc.GRID_A, cc.GRID_B, cc.GRID_1])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049])
@pytest.mark.parametrize("B", [1, 3])
def test_normal_is_the_restatement(dev, dims, n, B):
    """All byte values, points of every kind, rotations about all three axes; with B = 3 the last pose's translation is out of range."""
    from trajectory_optimization_amd import ops
    L, P, poses12 = rc.random_case(dims, n, seed=n + B, B=B, bad_t=B > 1)
    matcher = ops.ScanMatcher(_map(dev, L), floor=-20, unknown_value=-3)
    got = matcher.normal(_t(P, dev), poses12=_t(poses12, dev))
    want = synth.scan_normal_ref(L, sc.ORIGIN, sc.RES, P, poses12, -20, -3)
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, 32)
    assert np.array_equal(got.cpu().numpy(), want), (dims, n, B)
    assert B == 1 or not want[-1].any()
    if n >= 255:
        assert (want[:max(1, B - 1), 28] > 0).all() and (want[:, 28] < n).all()


def test_normal_takes_host_poses(dev, room):
    matcher, pts, L, P = room
    poses, quats = rc.starts(3)
    got = matcher.normal(pts, poses, quats)
    p12 = matcher.poses(poses, quats)
    assert torch.equal(got, matcher.normal(pts, poses12=p12))
    assert np.array_equal(got.cpu().numpy(), synth.scan_normal_ref(L, *ROOM, P, p12.cpu().numpy()))


def test_normal_beyond_one_pass_and_at_the_bound(dev):
    """2^22 points, eight times the tiles one launch's blocks hold.  FLAT: every residual the largest there is, the sum of e^2 within
    2 percent of 2^62.  STEEP: the largest gradient at a lever arm of 4094 voxels.  Both equal the Python-int sums."""
    from trajectory_optimization_amd import ops
    c = rc.bound_case()
    N = synth.SCAN_MAX_POINTS
    pts = _t(np.tile(c["points"], (N // 64, 1)), dev)
    pose = _t(c["pose"], dev)
    rows = {k: [rc.slow_record(c[k], c["origin"], c["resolution"], c["points"][i:i + 1], c["pose"][0]) for i in range(64)] for k in ("flat", "steep")}
    for k in ("flat", "steep"):
        matcher = ops.ScanMatcher(_map(dev, c[k], c["origin"], c["resolution"]))
        got = [int(v) for v in matcher.normal(pts, poses12=pose)[0].cpu().numpy()]
        want = [sum(rec[w] for rec in rows[k]) * (N // 64) for w in range(32)]
        assert got == want, k
        assert max(abs(v) for v in want) < 2 ** 62 and want[28] == want[29] == N
    flat = [sum(rec[w] for rec in rows["flat"]) * (N // 64) for w in range(32)]
    assert flat[27] == N * (254 * 4096) ** 2 > 0.98 * 2 ** 62
    with pytest.raises(ValueError, match="2\\^22"):
        matcher.normal(torch.zeros((N + 1, 3), device=dev), poses12=pose)


# ---- the step kernel ------------------------------------------------------------------------------------------------------------------

def test_step_is_the_restatement_on_crafted_records(dev, room):
    matcher = room[0]
    records, state = rc.crafted_steps()
    want, want12 = synth.scan_step_ref(records, state, ROOM[1])
    rc.check_crafted_steps(state, want, want12)
    st, p12 = _t(state, dev), torch.full((len(state), 12), 7.0, dtype=torch.float32, device=dev)
    out = matcher.step(_t(records, dev), st, p12)
    assert out is st
    got, got12 = st.cpu().numpy(), p12.cpu().numpy()
    assert np.array_equal(got, want)
    for b, row in enumerate(want12):
        assert got12[b].tobytes() == (np.full(12, 7.0, f32) if row is None else row).tobytes(), b
    # locked degrees of freedom and other tolerances, bit for bit as well
    want, want12 = synth.scan_step_ref(records, state, ROOM[1], dof="xyw", tol_t=0.5, tol_r=0.5)
    st = _t(state, dev)
    matcher.step(_t(records, dev), st, p12, dof="xyw", tol_t=0.5, tol_r=0.5)
    assert np.array_equal(st.cpu().numpy(), want) and [int(v) for v in want[:, synth.SR_STATUS]] == [0, 1, 0, 1, 1, 2, 4, 0, 1]
    got12 = p12.cpu().numpy()
    assert all(row is None or got12[b].tobytes() == row.tobytes() for b, row in enumerate(want12))


# ---- whole registrations --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [1, 2, 5, 30])
def test_register_is_the_restatement(dev, room, iterations):
    matcher, pts, L, P = room
    poses, quats = rc.starts()
    state = matcher.register(pts, poses, quats, iterations=iterations)
    want = synth.scan_register_ref(L, *ROOM, P, poses, quats, iterations)
    got = state.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (6, 64)
    assert np.array_equal(got, want), [int(b) for b in np.flatnonzero((got != want).any(axis=1))]
    if iterations == 30:
        assert (want[:, synth.SR_STATUS] == 1).sum() >= 3 and (want[:, synth.SR_ACCEPTED] >= 3).all()


def test_register_with_locked_dof_and_a_floor(dev):
    from trajectory_optimization_amd import ops
    L, P = rc.room()
    matcher = ops.ScanMatcher(_map(dev, L, *ROOM), floor=-20, unknown_value=-8)
    poses, quats = rc.starts(2, max_t=0.3, max_deg=0.0)
    poses[:, 2] = sc.true_pose()[0][2]
    state = matcher.register(_t(P, dev), poses, quats, iterations=12, dof="xyw", tol_t=0.001, tol_r=1e-5)
    want = synth.scan_register_ref(L, *ROOM, P, poses, quats, 12, "xyw", 0.001, 1e-5, -20, -8)
    assert np.array_equal(state.cpu().numpy(), want)


def test_a_batch_is_its_single_runs_and_frozen_poses_stay(dev, room):
    matcher, pts, L, P = room
    poses, quats = rc.starts(5)
    batch = matcher.register(pts, poses, quats, iterations=30).cpu().numpy()
    for b in range(5):
        single = matcher.register(pts, poses[b:b + 1], quats[b:b + 1], iterations=30).cpu().numpy()
        assert np.array_equal(single[0], batch[b]), b
    frozen = np.flatnonzero(batch[:, synth.SR_STATUS] != 0)
    assert len(frozen) > 0
    longer = matcher.register(pts, poses, quats, iterations=40).cpu().numpy()
    assert np.array_equal(longer[frozen], batch[frozen])
    # the records of frozen poses are not evaluated
    st, p12 = _t(batch, dev), matcher.poses(poses, quats)
    rec = matcher.normal(pts, poses12=p12, state=st).cpu().numpy()
    assert not rec[frozen].any() and rec[np.setdiff1d(np.arange(5), frozen)].any(axis=1).all()


def test_two_runs_agree(dev, room):
    matcher, pts, L, P = room
    poses, quats = rc.starts()
    a = matcher.register(pts, poses, quats, iterations=30)
    b = matcher.register(pts, poses, quats, iterations=30)
    assert torch.equal(a, b)
    assert torch.equal(matcher.normal(pts, poses, quats), matcher.normal(pts, poses, quats))


def test_register_scan_returns_the_restatements_result(dev, room):
    from trajectory_optimization_amd import tools
    matcher, pts, L, P = room
    poses, quats = rc.starts(2)
    got = tools.register_scan(matcher, pts, poses, quats)
    want = tools.scan_registrations(synth.scan_register_ref(L, *ROOM, P, poses, quats, 30), ROOM[1])
    assert isinstance(got, list) and len(got) == 2
    for g, w in zip(got, want):
        for k in tools.ScanRegistration.__slots__:
            assert np.array_equal(getattr(g, k), getattr(w, k)), k
        err = rc.pose_error(g.pose, g.quat)
        assert err[0] < 0.05 and err[1] < 0.05 and g.status in ops_status() and g.used == len(P) and 0 < g.inside <= g.used
        assert (np.linalg.eigvalsh(g.covariance) > 0).all() and np.allclose(g.covariance @ g.information, np.eye(6) * g.cost / (g.used - 6), rtol=1e-6, atol=1e-6 * g.cost / g.used)
    one = tools.register_scan(matcher, pts, poses[0], quats[0])
    assert isinstance(one, tools.ScanRegistration) and np.array_equal(one.pose, got[0].pose)
    world = one.world(pts).cpu().numpy()
    o, r = np.asarray(ROOM[0]), ROOM[1]
    centres = (np.floor((world - o) / r) + 0.5) * r + o
    assert np.abs(world - centres).max() < 0.1 * r      # every point back within a tenth of a voxel of a voxel centre
    planar = tools.register_scan(matcher.map, pts, poses[0], quats[0], dof="xyw", iterations=3)
    assert planar.pose[2] == poses[0, 2] and not planar.covariance[2].any()
    with pytest.raises(ValueError, match="belong to the ScanMatcher"):
        tools.register_scan(matcher, pts, poses[0], quats[0], floor=-10)


def ops_status():
    from trajectory_optimization_amd import ops
    return ops.SCAN_REGISTER_STATUS


# ---- the example ----------------------------------------------------------------------------------------------------------------------

def test_the_example_registers_below_the_match(dev):
    spec = importlib.util.spec_from_file_location("scan_registration_sample", os.path.join(REPO, "examples", "scan_registration_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    result = mod.run(steps=5, device=str(dev), verbose=False)
    e = np.asarray(result["errors"])
    assert e.shape == (4, 3, 2) and e[:, 2, 0].mean() < 0.5 * e[:, 1, 0].mean(), e
    assert all(s in ("CONVERGED", "STALLED", "RUNNING") for s in result["statuses"])


# ---- argument errors ------------------------------------------------------------------------------------------------------------------

def test_argument_errors_come_before_a_launch(dev, room):
    """Through ops: ValueError with nothing enqueued.  Through the C entries: TOHIP_EINVAL or TOHIP_ENOSPC, and the output buffers,
    filled with a pattern beforehand, keep it — not even the clear of the records was enqueued."""
    from trajectory_optimization_amd import _lib, ops
    from trajectory_optimization_amd._lib import ptr, stream_ptr
    matcher, pts, L, P = room
    poses, quats = rc.starts(2)
    p12 = matcher.poses(poses, quats)
    st, _ = ops.scan_register_start(poses, quats)
    st = _t(st, dev)
    for call in (lambda: matcher.register(pts, poses, quats, iterations=0), lambda: matcher.register(pts, poses, quats, iterations=257),
                 lambda: matcher.register(pts, poses, quats, dof="xq"), lambda: matcher.register(pts, poses, quats, tol_t=-1.0),
                 lambda: matcher.register(pts, poses, quats[:1].repeat(3, axis=0)), lambda: matcher.register(pts[:0], poses, quats),
                 lambda: matcher.register(pts, np.zeros((257, 3)), np.tile(quats[:1], (257, 1))),
                 lambda: matcher.register(pts, state=st.to(torch.float64), poses12=p12), lambda: matcher.register(pts, state=st, poses12=p12[:1]),
                 lambda: matcher.register(pts, state=st[:, :32].contiguous(), poses12=p12), lambda: matcher.normal(pts, poses12=p12.double()),
                 lambda: matcher.normal(pts, poses12=p12, state=st[:1]), lambda: matcher.normal(pts.cpu(), poses12=p12),
                 lambda: matcher.step(torch.zeros((2, 31), dtype=torch.int64, device=dev), st, p12),
                 lambda: matcher.step(torch.zeros((2, 32), dtype=torch.int64, device=dev), st, p12, dof=64)):
        with pytest.raises((ValueError, RuntimeError)):
            call()
    lib = _lib.lib()
    EINVAL, ENOSPC = _lib.CONSTANTS["TOHIP_EINVAL"], _lib.CONSTANTS["TOHIP_ENOSPC"]
    rec = torch.full((2, 32), 0x5555, dtype=torch.int64, device=dev)
    big = torch.full((2 * 32 + 1,), 0x5555, dtype=torch.int64, device=dev)
    odd = ctypes.c_void_p(big.data_ptr() + 4)
    geom, table, nb = ctypes.byref(matcher.geom), ptr(matcher.table), matcher.table.numel()
    n = pts.shape[0]
    null = ctypes.c_void_p(0)

    def normal(table=table, nb=nb, unknown=0, points=ptr(pts), n=n, poses=ptr(p12), b=2, state=ptr(st), records=ptr(rec), flags=0):
        return lib.tohip_scanreg_normal(table, nb, geom, unknown, points, n, poses, b, state, records, stream_ptr(), flags)
    bad = [normal(flags=1), normal(n=0), normal(n=(1 << 22) + 1), normal(b=0), normal(b=257), normal(unknown=1), normal(unknown=-128),
           normal(points=null), normal(poses=null), normal(records=null), normal(table=null), normal(records=odd),
           normal(state=ctypes.c_void_p(st.data_ptr() + 4)), normal(records=ptr(st), state=ptr(st)), normal(records=ptr(p12)),
           normal(points=ctypes.c_void_p(pts.data_ptr() + 2))]
    assert bad == [EINVAL] * len(bad), bad
    assert normal(nb=nb - 1) == ENOSPC
    before = st.clone()
    out12 = torch.full((2, 12), 7.0, dtype=torch.float32, device=dev)

    def step(records=ptr(rec), state=ptr(st), b=2, r=0.1, mask=63, tol_t=0.004, tol_r=1e-4, poses=ptr(out12), flags=0):
        return lib.tohip_scanreg_step(records, state, b, r, mask, tol_t, tol_r, poses, stream_ptr(), flags)
    bad = [step(flags=2), step(b=0), step(b=257), step(r=0.0), step(r=float("inf")), step(r=float("nan")), step(mask=0), step(mask=64),
           step(tol_t=-1.0), step(tol_r=float("nan")), step(tol_t=float("inf")), step(records=null), step(state=null), step(poses=null),
           step(records=odd), step(state=odd), step(records=ptr(st)), step(poses=ptr(st))]
    assert bad == [EINVAL] * len(bad), bad
    torch.cuda.synchronize()
    assert (rec == 0x5555).all() and (big == 0x5555).all() and torch.equal(st, before) and (out12 == 7.0).all()
    assert normal() == 0 and step() == 0     # the same calls with nothing wrong go through
    torch.cuda.synchronize()
    assert (rec != 0x5555).all() and not torch.equal(st, before)
