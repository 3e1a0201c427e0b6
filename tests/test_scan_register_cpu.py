"""Scan registration without a GPU ("Scan registration"): the numpy restatements the kernels are held to —
synth.scan_normal_ref against a per-point reference in Python ints and against hand cases, the record's bound, and
synth.scan_register_ref's behaviour: convergence on the room, the corridor's unconstrained axis, locked degrees of freedom and the
status paths — and the host layer's checks."""
import numpy as np
import pytest

import abi_cases
import contract_cases as cc
import scan_match_cases as sc
import scan_register_cases as rc
from trajectory_optimization_amd import synth

f32 = np.float32
ENTRIES = ("tohip_scanreg_normal", "tohip_scanreg_step")
ROOM = (sc.ROOM["origin"], sc.ROOM["resolution"])


def identity12(t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.eye(3).reshape(9), np.asarray(t)]).astype(f32)[None, :]


def test_entry_points_are_declared_bound_and_exported():
    from trajectory_optimization_amd import _lib, ops
    header, before = abi_cases.check_abi_entries(ENTRIES)
    assert [len(_lib.SIGNATURES[s][1]) for s in ENTRIES] == [12, 10]
    assert "still 15" in before.split("tohip_scanreg_normal")[0][-40:]
    assert (ops.SCAN_REGISTER_RECORD, ops.SCAN_REGISTER_STATE) == (synth.SCANREG_RECORD, synth.SCANREG_STATE) == (32, 64)
    assert ops.SCAN_REGISTER_STATUS == synth.SCANREG_STATUS and ops.SCAN_REGISTER_DOF == synth.SCANREG_DOF
    F = ops.SCAN_REGISTER_FIELDS
    assert [F[k] for k in ("t", "q", "lam", "delta", "status", "iterations", "accepted", "trial_t", "trial_q", "record")] == [
        synth.SR_T, synth.SR_Q, synth.SR_LAMBDA, synth.SR_DELTA, synth.SR_STATUS, synth.SR_ITER, synth.SR_ACCEPTED, synth.SR_TRIAL_T,
        synth.SR_TRIAL_Q, synth.SR_RECORD]
    assert (ops.SCAN_REGISTER_LAMBDA0, ops.SCAN_REGISTER_TOL_T, ops.SCAN_REGISTER_TOL_R, ops.SCAN_REGISTER_MAX_ITERATIONS) == (
        synth.SCANREG_LAMBDA0, synth.SCANREG_TOL_T, synth.SCANREG_TOL_R, synth.SCANREG_MAX_ITERATIONS)


@pytest.mark.parametrize("dims, n", [(cc.GRID_A, 200), (cc.GRID_B, 150), (cc.GRID_1, 40)])
def test_normal_ref_is_the_slow_reference(dims, n):
    """Every kind of point, all byte values, rotations about all three axes, one translation out of range; a floor and an
    unknown_value of their own."""
    L, P, poses12 = rc.random_case(dims, n, seed=3, B=3, bad_t=True)
    got = synth.scan_normal_ref(L, sc.ORIGIN, sc.RES, P, poses12, -20, -3)
    assert got.dtype == np.int64 and got.shape == (3, 32)
    for b in range(3):
        assert [int(v) for v in got[b]] == rc.slow_record(L, sc.ORIGIN, sc.RES, P, poses12[b], -20, -3), b
    assert not got[2].any() and (got[:2, 28] > 0).all() and (got[:2, 28] < n).all()
    if dims != cc.GRID_1:
        assert (got[:2, 29] > 0).all() and (got[:2, 29] < got[:2, 28]).all() and (got[:2, :27] != 0).all()


def _one(L, world_voxel, unknown_value=0):
    """The record of one point at `world_voxel` (voxel units, any fractions that are multiples of 1/256) under the identity pose."""
    p = (np.asarray(sc.ORIGIN) + sc.RES * np.asarray(world_voxel, dtype=np.float64)).astype(f32)[None, :]
    return [int(v) for v in synth.scan_normal_ref(L, sc.ORIGIN, sc.RES, p, identity12(), None, unknown_value)[0]]


def test_hand_cases():
    L = sc.random_log_odds((6, 5, 4), seed=1)
    L[L == synth.EVID_UNKNOWN] = -7
    T = L + 128
    # exactly on a voxel centre: M is that voxel's byte, the gradient the forward difference
    v = (2, 1, 1)
    rec = _one(L, (2.5, 1.5, 1.5))
    e = (255 - int(T[v])) * 4096
    g = [256 * int(T[3, 1, 1] - T[v]), 256 * int(T[2, 2, 1] - T[v]), 256 * int(T[2, 1, 2] - T[v])]
    a = [(int(256 * c) + 32) >> 6 for c in (2.5 - 4.0, 1.5 + 2.0, 1.5 - 1.0)]   # q - q_t: t = 0 lies at voxel (4, -2, 1) of the box
    assert a == [-6, 14, 2]
    j = [(a[1] * g[2] - a[2] * g[1] + 2048) >> 12, (a[2] * g[0] - a[0] * g[2] + 2048) >> 12, (a[0] * g[1] - a[1] * g[0] + 2048) >> 12]
    J = g + j
    assert rec[27] == e * e and rec[21:27] == [c * e for c in J] and rec[:6] == [g[0] * c for c in J] and rec[28:] == [1, 1, 0, 0]
    # f = 128 on each axis: the mean of the eight corners
    rec = _one(L, (3.0, 2.0, 2.0))
    total = int(T[2:4, 1:3, 1:3].sum())
    assert rec[27] == ((255 * 2 ** 24 - total * 2 ** 21 + 2 ** 11) >> 12) ** 2
    gx = (128 * 128 * int(T[3, 1:3, 1:3].sum() - T[2, 1:3, 1:3].sum()) + 128) >> 8
    assert rec[0] == gx * gx
    # a corner outside dims is 128 + unknown_value: beyond the last voxel along x, with another unknown_value
    rec = _one(L, (5.75, 1.5, 1.5), unknown_value=-5)
    m = 192 * int(T[5, 1, 1]) + 64 * 123
    assert rec[27] == ((255 * 2 ** 24 - m * 2 ** 16 + 2 ** 11) >> 12) ** 2 and rec[0] == (256 * (123 - int(T[5, 1, 1]))) ** 2 and rec[28:30] == [1, 0]
    # far outside dims, in range: the residual of the unknown byte, no gradient
    rec = _one(L, (100.5, 1.5, 1.5))
    assert rec[27] == (127 * 4096) ** 2 and not any(rec[:27]) and rec[28:30] == [1, 0]
    # t out of range: a zero record, whatever the points
    P = sc.random_scan((6, 5, 4), 50, 0)
    assert not synth.scan_normal_ref(L, sc.ORIGIN, sc.RES, P, identity12((1.0e7, 0.0, 0.0))).any()
    assert not synth.scan_normal_ref(L, sc.ORIGIN, sc.RES, P, identity12((np.nan, 0.0, 0.0))).any()


def test_the_bound_is_reached_and_holds():
    c = rc.bound_case()
    N = synth.SCAN_MAX_POINTS
    # FLAT: each of N points adds e^2 = (254 x 4096)^2, and N of them stay below 2^62
    flat = [rc.slow_record(c["flat"], c["origin"], c["resolution"], c["points"][i:i + 1], c["pose"][0]) for i in range(4)]
    assert all(rec[27] == (254 * 4096) ** 2 and rec[28] == 1 for rec in flat)
    assert 2 ** 61 < N * (254 * 4096) ** 2 < 2 ** 62
    # STEEP: the largest gradient and a lever arm of 4095 voxels: Python-int sums of N points stay below 2^62, and numpy's int64 sums
    # of 2^12 copies are the Python ints
    rows = [rc.slow_record(c["steep"], c["origin"], c["resolution"], c["points"][i:i + 1], c["pose"][0]) for i in range(64)]
    assert all(abs(rec[6]) == (254 * 256) ** 2 for rec in rows)                       # H_yy: g_y^2
    assert max(rec[20] for rec in rows) > (2 ** 17) ** 2                              # H_ww: j_z^2, the lever arm 4094 voxels
    sums = [sum(rec[k] for rec in rows) * (N // 64) for k in range(32)]
    assert max(abs(s) for s in sums) < 2 ** 62 and sums[20] > 2 ** 57
    tiled = np.tile(c["points"], (64, 1))
    got = synth.scan_normal_ref(c["steep"], c["origin"], c["resolution"], tiled, c["pose"], chunk=1000)
    assert [int(v) for v in got[0]] == [sum(rec[k] for rec in rows) * 64 for k in range(32)]
    with pytest.raises(ValueError, match="2\\^22"):
        synth.scan_normal_ref(c["flat"], c["origin"], c["resolution"], np.zeros((N + 1, 3), f32), c["pose"])


def _results(state, resolution, dof="xyzrpw"):
    from trajectory_optimization_amd import tools
    return tools.scan_registrations(state, resolution, dof)


def test_the_restatement_converges_on_the_room():
    """Six seeded starts within 0.45 voxel and 0.7 degrees per axis end within 0.05 voxel and 0.05 degrees of the truth in 30
    iterations (reached: 0.0066 voxel and 0.025 degrees at worst)."""
    L, P = rc.room()
    assert len(P) == 4202
    poses, quats = rc.starts()
    state = synth.scan_register_ref(L, *ROOM, P, poses, quats, 30)
    worst = [0.0, 0.0]
    for b, res in enumerate(_results(state, ROOM[1])):
        before, after = rc.pose_error(poses[b], quats[b]), rc.pose_error(res.pose, res.quat)
        print(f"start {b}: {before[0]:.3f} voxel {before[1]:.3f} deg -> {after[0]:.4f} voxel {after[1]:.4f} deg, {res.status} after {res.iterations}"
              f" iterations, {res.accepted} accepted, rms {res.rms:.2f} byte")
        assert before[0] <= 0.45 and before[1] <= 0.7 * np.sqrt(3.0) and before[0] > 0.1
        assert res.status in ("CONVERGED", "RUNNING", "STALLED") and res.used == 4202 and res.accepted >= 3
        assert abs(float(np.sqrt((res.quat ** 2).sum())) - 1.0) < 1e-15
        worst = [max(worst[0], after[0]), max(worst[1], after[1])]
    assert worst[0] <= 0.05 and worst[1] <= 0.05, worst


def test_a_batch_is_its_single_runs_and_frozen_poses_stay():
    L, P = rc.room()
    poses, quats = rc.starts(3)
    batch = synth.scan_register_ref(L, *ROOM, P, poses, quats, 30)
    for b in range(3):
        assert np.array_equal(synth.scan_register_ref(L, *ROOM, P, poses[b:b + 1], quats[b:b + 1], 30)[0], batch[b])
    frozen = np.flatnonzero(batch[:, synth.SR_STATUS] != 0)
    assert len(frozen) > 0
    longer = synth.scan_register_ref(L, *ROOM, P, poses, quats, 40)
    assert np.array_equal(longer[frozen], batch[frozen])


def test_the_corridor():
    L, P = rc.corridor()
    truth = rc.corridor_pose()
    r = rc.CORRIDOR["resolution"]
    poses, quats = rc.starts(2, seed=1, max_t=0.3, max_deg=0.3, truth=truth, resolution=r)
    # all six: x is not constrained — its column of J is zero, the first pivot 0
    state = synth.scan_register_ref(L, rc.CORRIDOR["origin"], r, P, poses, quats, 30)
    for res in _results(state, r):
        assert res.status == "DEGENERATE" and res.iterations == 1 and res.information[0, 0] == 0.0 and not res.covariance.any()
    # x locked: it registers, and the covariance has no x
    state = synth.scan_register_ref(L, rc.CORRIDOR["origin"], r, P, poses, quats, 30, dof="yzrpw")
    for b, res in enumerate(_results(state, r, "yzrpw")):
        err = np.abs(res.pose - truth[0]) / r
        assert res.status in ("CONVERGED", "STALLED") and err[1] < 0.05 and err[2] < 0.05 and rc.pose_error(res.pose, res.quat, truth, r)[1] < 0.05
        assert res.pose[0] == poses[b, 0]
        assert not res.covariance[0].any() and not res.covariance[:, 0].any() and (np.diag(res.covariance)[1:] > 0).all()
        w, v = np.linalg.eigh(res.covariance[:3, :3])
        assert v[0, np.argmax(w)] == 0.0
    # end walls far apart: x is constrained by few points, y by many
    L, P = rc.corridor(end_walls=True)
    state = synth.scan_register_ref(L, rc.CORRIDOR["origin"], r, P, poses, quats, 30)
    for res in _results(state, r):
        assert res.status in ("CONVERGED", "STALLED", "RUNNING") and rc.pose_error(res.pose, res.quat, truth, r)[0] < 0.05
        assert res.covariance[0, 0] > 3.0 * res.covariance[1, 1] > 0.0
        assert np.allclose(res.covariance, res.covariance.T) and (np.linalg.eigvalsh(res.covariance) > 0).all()


def test_a_planar_robot_keeps_z_roll_and_pitch():
    L, P = rc.room()
    t, q = sc.true_pose()
    start_t = t + np.asarray([0.03, -0.02, 0.0])
    start_q = synth.quat_mul(sc.yaw_quat(np.deg2rad(0.4)), q)
    state = synth.scan_register_ref(L, *ROOM, P, start_t[None], start_q[None], 30, dof="xyw")
    F = state.view(np.float64)[0]
    assert F[synth.SR_T + 2].tobytes() == np.float64(start_t[2]).tobytes()                       # z: the input's bits
    assert F[synth.SR_Q + 1:synth.SR_Q + 3].tobytes() == np.zeros(2).tobytes()                   # roll and pitch: +0, as given
    assert F[synth.SR_DELTA + 2:synth.SR_DELTA + 5].tobytes() == np.zeros(3).tobytes()
    res = _results(state, ROOM[1], "xyw")[0]
    err = rc.pose_error(res.pose, res.quat)
    assert np.abs(res.pose[:2] - t[:2]).max() / ROOM[1] < 0.05 and err[1] < 0.05 and res.accepted >= 2
    free = [0, 1, 5]
    assert (np.diag(res.covariance)[free] > 0).all() and not np.delete(res.covariance, free, axis=0).any()
    assert synth.scan_dof_mask("xyw") == 0b100011 and synth.scan_dof_mask(63) == synth.scan_dof_mask("xyzrpw") == 63
    for bad in ("", "xx", "xyq", 0, 64, None, True):
        with pytest.raises(ValueError):
            synth.scan_dof_mask(bad)


def test_status_paths():
    L, P = rc.room()
    t, q = sc.true_pose()
    # EMPTY: every point out of range under the pose (the translation is in range, the points are not)
    far = np.full((5, 3), 1.0e6, dtype=f32)
    state = synth.scan_register_ref(L, *ROOM, far, t[None], q[None], 5)
    assert state[0, synth.SR_STATUS] == 4 and state[0, synth.SR_ITER] == 1 and not state[0, synth.SR_RECORD:].any()
    # ... and a translation out of range
    state = synth.scan_register_ref(L, *ROOM, P, np.asarray([[1.0e7, 0.0, 0.0]]), q[None], 5)
    assert state[0, synth.SR_STATUS] == 4
    # STALLED: with tolerances of zero nothing counts as converged; at the kinked maximum every step is rejected in the end and
    # lambda climbs past 2^30
    state = synth.scan_register_ref(L, *ROOM, P, t[None], q[None], 256, tol_t=0.0, tol_r=0.0)
    F = state.view(np.float64)[0]
    assert state[0, synth.SR_STATUS] == 2 and F[synth.SR_LAMBDA] > 2.0 ** 30 and state[0, synth.SR_ITER] < 256
    res = _results(state, ROOM[1])[0]
    assert res.status == "STALLED" and rc.pose_error(res.pose, res.quat)[0] < 0.05
    with pytest.raises(ValueError, match="iterations"):
        synth.scan_register_ref(L, *ROOM, P, t[None], q[None], 257)


def test_the_step_ref_on_crafted_records():
    """A zero pivot freezes as DEGENERATE, a rejected step multiplies lambda by 8 and keeps the pose, a frozen pose is not touched."""
    records, state = rc.crafted_steps()
    new, poses12 = synth.scan_step_ref(records, state, ROOM[1])
    rc.check_crafted_steps(state, new, poses12)


def test_the_host_layer_checks_and_start():
    from trajectory_optimization_amd import ops, tools
    poses, quats = rc.starts(3)
    quats = quats * np.asarray([[1.0], [2.5], [0.3]])   # unnormalised quaternions are taken as they are
    st, p12 = ops.scan_register_start(poses, quats)
    want_st, want_p12 = synth.scan_register_init_ref(poses, quats)
    assert st.dtype == np.int64 and np.array_equal(st, want_st) and p12.dtype == f32 and p12.tobytes() == want_p12.tobytes()
    assert np.abs(p12[1, :9].astype(np.float64) - synth.scan_rotation(quats[1]).reshape(9)).max() < 2e-7

    class NotAMap:
        pass
    with pytest.raises(ValueError, match="EvidenceMap"):
        ops.check_scan_register(NotAMap())
    em = ops.EvidenceMap.__new__(ops.EvidenceMap)   # (the checks look at its type only)
    assert ops.check_scan_register(em, 30, "xyw", None, 0.5, 256) == (30, 0b100011, 1.0 / 256.0, 0.5)
    for kw in (dict(iterations=0), dict(iterations=257), dict(iterations=1.5), dict(dof="xyq"), dict(dof=0), dict(tol_t=-1.0), dict(tol_r=np.nan),
               dict(tol_t="a"), dict(n_poses=0), dict(n_poses=257)):
        with pytest.raises(ValueError, match=next(iter(kw)).split("_")[0]):
            ops.check_scan_register(em, **kw)
    assert "THE COVARIANCE" in tools.register_scan.__doc__ and "not a calibrated uncertainty" in tools.register_scan.__doc__
