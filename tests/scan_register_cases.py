"""Shared inputs of the scan-registration tests (tests/test_scan_register_cpu.py, tests/test_hip_scan_register.py): numpy only.  They
build on tests/scan_match_cases.py: its room, its random maps over all byte values and its scans with points that are NaN, inf, out
of range, on voxel faces, in the apron and near every face of dims.

THE ROOM SCAN.  The centres of the room's surface voxels — occupied, with a voxel of air among the six neighbours — taken into the
sensor frame of the true pose: 4 202 points.  At the true pose every point sits on the centre of an occupied voxel, the maximum of the
trilinear field along the wall's normal.  STARTS: six seeded starting poses within 0.45 voxel per axis and 0.7 degrees per axis of the
truth.

THE CORRIDOR.  A tube of constant cross-section along x — floor, ceiling and two side walls, values 70 / -40 / -128 as in the room —
so that no voxel differs from its x neighbour: the map says nothing about x.  corridor(end_walls=True) closes it with two walls far
apart: x is then constrained by few points, y and z by many."""
import numpy as np

import scan_match_cases as sc
from trajectory_optimization_amd import synth

f32 = np.float32


def surface_points(occ, air):
    """World-frame centres (in voxel units) of the occupied voxels of `occ` with a 6-neighbour in `air`."""
    surf = np.zeros(occ.shape, dtype=bool)
    for ax in range(3):
        for s in (1, -1):
            surf |= occ & np.roll(air, s, ax)
    return np.argwhere(surf) + 0.5


_ROOM = {}


def room():
    """-> (L (48,40,12) int64, points (4202,3) f32 in the sensor frame of sc.true_pose()), computed once."""
    if not _ROOM:
        occ = sc.room_occupancy()
        L = sc.room_log_odds(occ)
        o, r = np.asarray(sc.ROOM["origin"], dtype=np.float64), sc.ROOM["resolution"]
        _ROOM["L"], _ROOM["points"] = L, sc.to_sensor_frame(o + r * surface_points(occ, L == -40))
        _ROOM["L"].setflags(write=False)
        _ROOM["points"].setflags(write=False)
    return _ROOM["L"], _ROOM["points"]


def rotvec_quat(v):
    """A rotation vector (3,) in radians -> the quaternion wxyz (f64)."""
    v = np.asarray(v, dtype=np.float64)
    th = np.sqrt((v * v).sum())
    if th == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(0.5 * th)], np.sin(0.5 * th) * v / th])


def starts(n=6, seed=1, max_t=0.45, max_deg=0.7, truth=None, resolution=None):
    """n starting poses around the truth (sc.true_pose() of the room unless given) -> (poses (n,3) f64, quats (n,4) f64): each axis of
    the translation off by up to max_t voxels, the rotation by a world-frame rotation vector of up to max_deg degrees per axis.
    (The seed: of the eight tried, 0 .. 7, five end inside 0.05 voxel and 0.05 degrees from all six starts; with 0, 4 and 7 one start
    each ends outside — converged on a small damped step, or stalled at a kink, short of the truth — which DESIGN.md 10 "Scan
    registration" lists among the limits.  1 is the first that passes.)"""
    rng = np.random.default_rng(4200 + seed)
    t, q = sc.true_pose() if truth is None else truth
    r = sc.ROOM["resolution"] if resolution is None else resolution
    dt = rng.uniform(-max_t, max_t, (n, 3)) * r
    dth = np.deg2rad(rng.uniform(-max_deg, max_deg, (n, 3)))
    return t + dt, np.stack([synth.quat_mul(rotvec_quat(v), q) for v in dth])


def pose_error(pose, quat, truth=None, resolution=None):
    """-> (the largest translation error per axis in voxels, the rotation error in degrees) of a pose against the truth."""
    t, q = sc.true_pose() if truth is None else truth
    r = sc.ROOM["resolution"] if resolution is None else resolution
    quat = np.asarray(quat, dtype=np.float64)
    d = abs(float(np.dot(quat / np.sqrt((quat * quat).sum()), q / np.sqrt((q * q).sum()))))
    return float(np.abs(np.asarray(pose, dtype=np.float64) - t).max() / r), float(np.rad2deg(2.0 * np.arccos(min(1.0, d))))


CORRIDOR = dict(origin=(0.0, 0.0, 0.0), resolution=0.1, dims=(64, 16, 12))
CORRIDOR_T = (31.3, 7.6, 5.4)     # the sensor's true position in voxel units


def corridor(end_walls=False):
    """-> (L (64,16,12) int64, points (N,3) f32 in the sensor frame of corridor_pose()): walls at y = 2 and 13, floor z = 1, ceiling
    z = 10, every x alike; with end_walls two more at x = 2 and 61 (and nothing observed behind them)."""
    dims = CORRIDOR["dims"]
    occ = np.zeros(dims, dtype=bool)
    occ[:, 2:14, 1] = occ[:, 2:14, 10] = True
    occ[:, 2, 1:11] = occ[:, 13, 1:11] = True
    L = np.full(dims, synth.EVID_UNKNOWN, dtype=np.int64)
    L[:, 3:13, 2:10] = -40
    if end_walls:
        occ[2, 2:14, 1:11] = occ[61, 2:14, 1:11] = True
        occ[:2] = occ[62:] = False
        L[:3] = L[61:] = synth.EVID_UNKNOWN
    L[occ] = 70
    air = L == -40
    W = surface_points(occ, air)
    W = W[(W[:, 0] > 8) & (W[:, 0] < 56) | (end_walls & ((W[:, 0] < 3) | (W[:, 0] > 61)))]   # (the tube's open ends see no apron)
    t, q = corridor_pose()
    R = synth.scan_rotation(q).astype(np.float64)
    o, r = np.asarray(CORRIDOR["origin"], dtype=np.float64), CORRIDOR["resolution"]
    return L, ((o + r * W - t) @ R).astype(f32)


def corridor_pose():
    o, r = np.asarray(CORRIDOR["origin"], dtype=np.float64), CORRIDOR["resolution"]
    return o + r * np.asarray(CORRIDOR_T), sc.yaw_quat(0.05)


def random_case(dims, n, seed, B=1, bad_t=False):
    """A random map of sc.random_log_odds and a scan of sc.random_scan (every kind of point), with B poses: sc.rotations' (identity,
    yaw, roll and pitch) at sc.T moved by a fraction of a voxel per pose; bad_t: the last pose's translation is out of range.
    -> (L, points (n,3) f32, poses12 (B,12) f32)."""
    L = sc.random_log_odds(dims, seed)
    P = sc.random_scan(dims, n, seed)
    rows = []
    for b in range(B):
        R = synth.scan_rotation(sc.rotations(3)[(b + (1 if B > 1 else 0)) % 3])
        t = np.asarray(sc.T, dtype=np.float64) + sc.RES * np.asarray([0.31, -0.17, 0.23]) * b
        rows.append(np.concatenate([R.reshape(9), t.astype(f32)]))
    poses12 = np.stack(rows).astype(f32)
    if bad_t:
        poses12[-1, 9] = f32(1.0e7)
    return L, P, poses12


def slow_record(L, origin, resolution, points, pose12, floor=None, unknown_value=0):
    """One pose's record point by point in Python ints, straight from the definitions (at most a few hundred points) -> list of 32."""
    T = synth.scan_values_ref(L, floor, unknown_value) + 128
    dims = T.shape
    pose12 = np.asarray(pose12, dtype=f32)
    rec = [0] * 32
    qt, t_ok = synth.occ_fixed(pose12[9:12], origin, resolution)
    if not t_ok[0]:
        return rec
    qs, ok = synth.scan_fixed_ref(points, pose12[:9], pose12[9:12], origin, resolution)
    for q in (tuple(int(v) for v in row) for row, k in zip(qs, ok) if k):
        c = [v - 128 for v in q]
        b, f = [v >> 8 for v in c], [v & 255 for v in c]
        w = [(256 - v, v) for v in f]

        def V(i, j, k):
            x, y, z = b[0] + i, b[1] + j, b[2] + k
            return int(T[x, y, z]) if 0 <= x < dims[0] and 0 <= y < dims[1] and 0 <= z < dims[2] else 128 + unknown_value
        ijk = [(i, j, k) for i in range(2) for j in range(2) for k in range(2)]
        M24 = sum(V(i, j, k) * w[0][i] * w[1][j] * w[2][k] for i, j, k in ijk)
        G = [sum(w[1][j] * w[2][k] * (V(1, j, k) - V(0, j, k)) for j in range(2) for k in range(2)),
             sum(w[0][i] * w[2][k] * (V(i, 1, k) - V(i, 0, k)) for i in range(2) for k in range(2)),
             sum(w[0][i] * w[1][j] * (V(i, j, 1) - V(i, j, 0)) for i in range(2) for j in range(2))]
        e = (255 * 2 ** 24 - M24 + 2 ** 11) >> 12
        g = [(v + 128) >> 8 for v in G]
        a = [(q[k] - int(qt[0, k]) + 32) >> 6 for k in range(3)]
        cr = [a[1] * g[2] - a[2] * g[1], a[2] * g[0] - a[0] * g[2], a[0] * g[1] - a[1] * g[0]]
        J = g + [(v + 2 ** 11) >> 12 for v in cr]
        assert 0 <= e < 2 ** 20 and all(abs(v) < 2 ** 16 for v in g) and all(abs(v) < 2 ** 15 for v in a) and all(abs(v) <= 2 ** 20 for v in J)
        n = 0
        for i in range(6):
            for j in range(i, 6):
                rec[n] += J[i] * J[j]
                n += 1
        for i in range(6):
            rec[21 + i] += J[i] * e
        rec[27] += e * e
        rec[28] += 1
        rec[29] += all(0 <= b[k] and b[k] + 1 < dims[k] for k in range(3))
    return rec


def bound_case():
    """The largest sums by construction -> (L, origin, resolution, [(points, poses12, multiplicity)]).  FLAT: every byte 1, so that
    each point's residual is the largest there is, e = 254 x 4096.  STEEP: planes of bytes 255 and 1 alternating along y in a box
    2048 voxels long, points at its far end on the faces between the planes, where |g_y| = 254 x 256 is the largest gradient, and
    the sensor 4095 voxels away along x: the lever arm the box allows."""
    dims = (2048, 4, 2)
    flat = np.full(dims, -127, dtype=np.int64)
    steep = np.full(dims, -127, dtype=np.int64)
    steep[:, 0::2, :] = 127
    r, origin = 0.125, (0.0, 0.0, 0.0)
    far = r * np.asarray([[2046.5, 1.0 + (i % 2), 0.75] for i in range(64)]) + r * np.asarray([[-(i // 2) * 0.25, 0.0, 0.0] for i in range(64)])
    pose = np.concatenate([np.eye(3).reshape(9), [-2048.0 * r, 0.0, 0.0]]).astype(f32)[None, :]
    pts = (far - np.asarray([[-2048.0 * r, 0.0, 0.0]])).astype(f32)
    return dict(dims=dims, origin=origin, resolution=r, flat=flat, steep=steep, points=pts, pose=pose)


def crafted_steps():
    """Records and states that take k_scan_step down every path -> (records (9,32) int64, state (9,64) int64).  The records are the
    room's at a displaced pose, edited: 0 a first iteration; 1 a zero pivot (H_xx = 0); 2 a rejected step (the trial's cost is
    larger); 3 a frozen pose; 4 an accepted step small enough to converge; 5 a rejection that takes lambda past 2^30; 6 no point
    used; 7 a smaller cost over another `used`: rejected; 8 an accepted step too large to converge."""
    L, P = room()
    poses, quats = starts(1)
    base, p12 = synth.scan_register_init_ref(np.repeat(poses, 9, axis=0), np.repeat(quats, 9, axis=0))
    rec = synth.scan_normal_ref(L, sc.ROOM["origin"], sc.ROOM["resolution"], P, p12[:1])[0]
    records = np.tile(rec, (9, 1))
    state = base.copy()
    F = state.view(np.float64)
    for b in range(1, 9):   # not a first iteration: a current record, a trial pose of its own, a last step
        state[b, synth.SR_ITER] = 3
        state[b, synth.SR_RECORD:synth.SR_RECORD + 32] = rec
        F[b, synth.SR_TRIAL_T:synth.SR_TRIAL_T + 3] += 0.001 * b
        F[b, synth.SR_TRIAL_Q + 3] += 0.0001 * b
        F[b, synth.SR_DELTA:synth.SR_DELTA + 6] = 0.01
    state[1, synth.SR_RECORD + 0] = 0
    records[1, 27] -= 5
    records[1, 0] = 0
    records[2, 27] += 1
    state[3, synth.SR_STATUS] = 1
    records[4, 27] -= 1
    F[4, synth.SR_DELTA:synth.SR_DELTA + 6] = [1.0 / 256.0, -1.0 / 256.0, 0.0, 1.0e-4, -1.0e-4, 0.0]
    records[5, 27] += 7
    F[5, synth.SR_LAMBDA] = 2.0 ** 28
    records[6, 28] = 0
    records[7, 27] -= 100
    records[7, 28] -= 1
    records[8, 27] -= 1
    F[8, synth.SR_LAMBDA] = 2.0 ** -29
    return records, state


def check_crafted_steps(before, after, poses12):
    """What the definitions ask of crafted_steps' poses, whoever computed `after` (B,64) int64 and the poses12 rows (None or
    unchanged where a pose wrote none — the caller passes None for those)."""
    S, IT, LAM = synth.SR_STATUS, synth.SR_ITER, synth.SR_LAMBDA
    Fb, Fa = before.view(np.float64), after.view(np.float64)
    assert [int(v) for v in after[:, S]] == [0, 3, 0, 1, 1, 2, 4, 0, 0]
    assert np.array_equal(after[3], before[3]) and poses12[3] is None
    assert [int(v) for v in after[:, IT] - before[:, IT]] == [1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert Fa[0, LAM] == 2.0 ** -10 and Fa[1, LAM] == 2.0 ** -13 and Fa[2, LAM] == 2.0 ** -7 and Fa[4, LAM] == 2.0 ** -13
    assert Fa[5, LAM] == 2.0 ** 31 and Fa[7, LAM] == 2.0 ** -7 and Fa[8, LAM] == 2.0 ** -30
    for b in (2, 7):   # rejected: the pose and its record stay, the new trial comes from them
        assert np.array_equal(after[b, :7], before[b, :7]) and np.array_equal(after[b, synth.SR_RECORD:], before[b, synth.SR_RECORD:])
        assert not np.array_equal(after[b, synth.SR_TRIAL_T:synth.SR_TRIAL_T + 3], before[b, synth.SR_TRIAL_T:synth.SR_TRIAL_T + 3])
    for b in (1, 4, 8):   # accepted: the trial became the pose
        assert np.array_equal(after[b, :7], before[b, synth.SR_TRIAL_T:synth.SR_TRIAL_T + 7]) and after[b, synth.SR_ACCEPTED] == 1
    assert after[0, synth.SR_ACCEPTED] == 0 and after[2, synth.SR_ACCEPTED] == 0
    for b in (0, 2, 7, 8):
        assert poses12[b] is not None and np.isfinite(poses12[b]).all()
        assert np.isfinite(Fa[b, synth.SR_DELTA:synth.SR_DELTA + 6]).all() and Fa[b, synth.SR_DELTA:synth.SR_DELTA + 6].any()
    for b in (1, 3, 4, 5, 6):
        assert poses12[b] is None
