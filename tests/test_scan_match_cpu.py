"""CPU checks of scan matching (no GPU): the four entry points are declared in the header and in _lib's table at ABI 15 and refuse
bad arguments — a non-zero `flags` among them — before any launch; yaw_candidates and the parabola of match_scan's refinement do what
their definitions say; the two numpy restatements the kernels are compared against, one point by point and one by windows of a padded
volume, agree with each other on random maps; and on the end-to-end scene of tests/scan_match_cases.py the restatement alone recovers
the planted offset uniquely, so that the GPU test's claim is one about the kernel and not about the scene."""
import ctypes

import numpy as np
import pytest

import scan_match_cases as sc
from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

EINVAL, ENOSPC = -1, -2
ENTRIES = ["tohip_scan_prepare", "tohip_scan_score", "tohip_scan_correlate", "tohip_scan_best"]


def test_header_and_table_declare_the_new_entries_at_abi_15():
    from trajectory_optimization_amd import _lib
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_scan_prepare / tohip_scan_score / tohip_scan_correlate / tohip_scan_best" in before
    for sym in ENTRIES:   # `..., void *stream, uint32_t flags)`: the reserved word comes last
        assert " ".join(header.split("int " + sym + "(")[1].split(";")[0].split()).endswith("void *stream, uint32_t flags)")
    assert [len(_lib.SIGNATURES[s][1]) for s in ENTRIES] == [9, 16, 16, 8]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("tohip_scan_")) == sorted(ENTRIES)


def test_entries_refuse_bad_arguments_and_flags_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    evid, table, pts, poses, shifts, a, b, c, d = (ctypes.c_void_p(v) for v in (4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288, 1048576))
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, dims=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*dims))
    ok, nb = geom(), L.tohip_evid_bytes(64, 64, 32)
    calls = {
        "prepare": (L.tohip_scan_prepare, ("evid", "evid_bytes", "geom", "floor", "unknown", "table", "table_bytes", "stream", "flags"),
                    (evid, nb, ok, -127, 0, table, nb, None, 0)),
        "score": (L.tohip_scan_score, ("evid", "evid_bytes", "geom", "floor", "unknown", "points", "n", "poses", "shifts", "b", "score", "used",
                                       "inside", "known", "stream", "flags"),
                  (evid, nb, ok, -127, 0, pts, 100, poses, shifts, 5, a, b, c, d, None, 0)),
        "correlate": (L.tohip_scan_correlate, ("table", "table_bytes", "geom", "unknown", "points", "n", "poses", "k", "wx", "wy", "wz", "scores",
                                               "scores_bytes", "used", "stream", "flags"),
                      (table, nb, ok, 0, pts, 100, poses, 3, 2, 1, 1, a, 4 * 3 * 45, b, None, 0)),
        "best": (L.tohip_scan_best, ("scores", "k", "wx", "wy", "wz", "best", "stream", "flags"), (a, 3, 2, 1, 1, b, None, 0)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, v) for k, v in zip(names, base)])

    odd = ctypes.c_void_p(131074)
    for name in calls:
        for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
            assert call(name, flags=flags) == EINVAL, (name, flags)
    for name, size in (("prepare", "evid_bytes"), ("prepare", "table_bytes"), ("score", "evid_bytes"), ("correlate", "table_bytes")):
        assert call(name, geom=None) == EINVAL and call(name, **{size: nb - 1}) == ENOSPC, name
        for g in (geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(dims=(0, 64, 32)), geom(dims=(64, 2049, 32))):
            assert call(name, geom=g) == EINVAL, name
    for kw in (dict(evid=None), dict(table=None), dict(table=evid), dict(evid=ctypes.c_void_p(4104)), dict(table=ctypes.c_void_p(8200)),
               dict(floor=-128), dict(floor=1), dict(unknown=-128), dict(unknown=1)):
        assert call("prepare", **kw) == EINVAL, kw
    for kw in (dict(evid=None), dict(floor=-128), dict(floor=1), dict(unknown=-128), dict(unknown=1), dict(points=None), dict(poses=None),
               dict(n=0), dict(n=(1 << 22) + 1), dict(b=0), dict(b=(1 << 22) + 1), dict(score=None), dict(used=None), dict(inside=None),
               dict(known=None), dict(used=a), dict(known=b), dict(score=pts), dict(inside=poses), dict(known=shifts), dict(score=evid),
               dict(score=odd), dict(points=odd), dict(shifts=odd)):
        assert call("score", **kw) == EINVAL, kw
    for kw in (dict(table=None), dict(unknown=-128), dict(unknown=1), dict(points=None), dict(poses=None), dict(n=0), dict(n=(1 << 22) + 1),
               dict(k=0), dict(k=257), dict(wx=-1), dict(wx=17), dict(wy=-1), dict(wy=17), dict(wz=-1), dict(wz=5), dict(scores=None),
               dict(used=None), dict(used=a), dict(scores=pts), dict(used=poses), dict(scores=table), dict(scores=odd), dict(poses=odd)):
        assert call("correlate", **kw) == EINVAL, kw
    assert call("correlate", scores_bytes=4 * 3 * 45 - 1) == ENOSPC
    for kw in (dict(scores=None), dict(best=None), dict(best=a), dict(k=0), dict(k=257), dict(wx=17), dict(wy=-1), dict(wz=5), dict(scores=odd),
               dict(best=odd)):
        assert call("best", **kw) == EINVAL, kw


def test_check_scan_match_names_every_refusal():
    import torch

    from trajectory_optimization_amd import ops

    class M(ops.EvidenceMap):   # a map's geometry without a device
        def __init__(self):
            self.origin, self.resolution, self.dims, _ = ops.check_los((0, 0, 0), 0.1, (8, 8, 4))
            self.device = torch.device("cuda:0")

    m = M()
    assert ops.check_scan_match(m) == (-127, 0, None) and ops.check_scan_match(m, -10, -3, (16, 0, 4), 256) == (-10, -3, (16, 0, 4))
    assert ops.check_scan_match(m, np.int64(0), np.int32(-127), [1, 2, 3], 1) == (0, -127, (1, 2, 3))
    for bad in (None, object(), ops.SpaceMap.__new__(ops.SpaceMap)):
        with pytest.raises(ValueError, match="the map must be an ops.EvidenceMap"):
            ops.check_scan_match(bad)
    for bad in (-128, 1, 0.0, "0", True):
        with pytest.raises(ValueError, match=r"floor must be None or an integer in \[-127, 0\]"):
            ops.check_scan_match(m, bad)
    for bad in (-128, 1, None, 0.5):
        with pytest.raises(ValueError, match=r"unknown_value must be an integer in \[-127, 0\]"):
            ops.check_scan_match(m, None, bad)
    for bad in ((17, 0, 0), (0, 17, 0), (0, 0, 5), (-1, 0, 0), (1, 1), (1.0, 1, 1), 3, "888"):
        with pytest.raises(ValueError, match="window must be three integers"):
            ops.check_scan_match(m, None, 0, bad)
    for bad in (0, 257, 1.0):
        with pytest.raises(ValueError, match="the rotations must number 1 .. 256"):
            ops.check_scan_match(m, None, 0, (1, 1, 1), bad)
    assert 256 * 33 * 33 * 9 <= ops.SCAN_MAX_CANDIDATES   # (the largest window with the most rotations still fits)
    # rotations: f64 on the host, rounded once
    q = np.array([[2.0, 0.0, 0.0, 0.0], [np.cos(0.2), 0.0, 0.0, np.sin(0.2)]])
    R = ops.scan_rotations(q)
    assert R.dtype == np.float32 and np.array_equal(R[0], np.eye(3, dtype=np.float32)) and np.array_equal(R[1], synth.scan_rotation(q[1]))
    assert np.array_equal(R[1], np.array([[np.cos(0.4), -np.sin(0.4), 0], [np.sin(0.4), np.cos(0.4), 0], [0, 0, 1]]).astype(np.float32))
    for bad in ([0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [[np.nan, 0, 0, 1]]):
        with pytest.raises(ValueError):
            ops.scan_rotations(bad)


# ---- yaw candidates and the parabola --------------------------------------------------------------------------------------------------

def test_yaw_candidates_are_symmetric_centred_and_hold_the_prior():
    from trajectory_optimization_amd import tools
    prior = synth.quat_mul(np.array([np.cos(0.35), 0.0, 0.0, np.sin(0.35)]), np.array([np.cos(0.05), np.sin(0.05), 0.0, 0.0]))
    for n, half in ((1, 0.3), (3, 0.1), (9, np.deg2rad(6.0)), (41, 0.2)):
        c = tools.yaw_candidates(3.0 * prior, half, n)
        assert c.shape == (n, 4) and c.dtype == np.float64
        assert np.array_equal(c[n // 2], prior / np.sqrt((prior * prior).sum()))          # the prior exactly, normalised
        rel = synth.quat_mul(c, prior * np.array([1.0, -1.0, -1.0, -1.0]))                   # c conj(prior): a pure turn about z
        assert np.abs(rel[:, 1:3]).max() < 1e-15
        ang = 2.0 * np.arctan2(rel[:, 3], rel[:, 0])
        if n > 1:
            np.testing.assert_allclose(ang, np.linspace(-half, half, n), atol=1e-14)
            np.testing.assert_allclose(ang, -ang[::-1], atol=1e-15)                          # symmetric about the prior
    for bad in (0, 2, 4, 257, 3.0):
        with pytest.raises(ValueError, match="n must be an odd integer"):
            tools.yaw_candidates(prior, 0.1, bad)
    for bad in (-0.1, 4.0, float("nan"), None):
        with pytest.raises(ValueError, match="half_range must be a finite angle"):
            tools.yaw_candidates(prior, bad, 3)


def test_parabola_vertex_is_exact_on_a_quadratic_volume_and_guarded():
    from trajectory_optimization_amd import tools
    dz, dy, dx = np.meshgrid(np.arange(-2, 3), np.arange(-4, 5), np.arange(-3, 4), indexing="ij")
    vx = (0.3, -0.45, 0.125)                                  # the true vertex, inside the best cell
    vol = 1000.0 - 7.0 * (dx - vx[0]) ** 2 - 3.0 * (dy - vx[1]) ** 2 - 11.0 * (dz - vx[2]) ** 2
    at = np.unravel_index(np.argmax(vol), vol.shape)
    assert at == (2, 4, 3)
    assert np.abs(tools.scan_refine(vol, at) - np.asarray(vx)).max() < 1e-12
    # a vertex beyond half a voxel is clamped
    far = 1000.0 - 7.0 * (dx - 0.9) ** 2 - 3.0 * dy ** 2 - 11.0 * dz ** 2
    assert tools.scan_refine(far, (2, 4, 3)).tolist() == [0.5, 0.0, 0.0]
    # best on the window's edge: no neighbour on one side of that axis
    assert tools.scan_refine(vol, (2, 4, 0))[0] == 0.0 and tools.scan_refine(vol, (2, 8, 3))[1] == 0.0 and tools.scan_refine(vol, (4, 4, 3))[2] == 0.0
    # a flat (and a positive) second difference
    flat = np.zeros((5, 9, 7))
    assert tools.scan_refine(flat, (2, 4, 3)).tolist() == [0.0, 0.0, 0.0]
    assert tools.scan_refine(-vol, (2, 4, 3)).tolist() == [0.0, 0.0, 0.0]
    ramp = np.broadcast_to(np.arange(7.0), (5, 9, 7))
    assert tools.scan_refine(ramp, (2, 4, 3)).tolist() == [0.0, 0.0, 0.0]
    # wz = 0: one level, no parabola along z
    assert tools.scan_refine(vol[2:3], (0, 4, 3))[2] == 0.0 and abs(tools.scan_refine(vol[2:3], (0, 4, 3))[0] - vx[0]) < 1e-12


# ---- the two restatements against each other ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,window", [((13, 10, 5), (3, 5, 1)), ((1, 1, 1), (2, 2, 1)), ((4, 4, 2), (16, 16, 4)), ((9, 7, 3), (0, 0, 0)),
                                         ((6, 5, 9), (1, 0, 4))])
def test_correlate_ref_equals_score_ref_per_candidate(dims, window):
    L, pts, quats = sc.random_log_odds(dims, 4), sc.random_scan(dims, 300, 4), sc.rotations(3)
    Rs = [synth.scan_rotation(q) for q in quats]
    scores, used = synth.scan_correlate_ref(L, sc.ORIGIN, sc.RES, pts, Rs, sc.T, window, floor=-25, unknown_value=-6, chunk=64)
    shifts = sc.window_shifts(window)
    assert scores.shape == (3, 2 * window[2] + 1, 2 * window[1] + 1, 2 * window[0] + 1) and scores.dtype == np.int32
    rng = np.random.default_rng(1)
    pick = np.arange(len(shifts)) if len(shifts) <= 300 else np.unique(np.concatenate([[0, len(shifts) - 1], rng.choice(len(shifts), 200)]))
    seen_outside = seen_unknown = False
    for k in range(3):
        for s in pick:
            score, n_used, inside, known = synth.scan_score_ref(L, sc.ORIGIN, sc.RES, pts, Rs[k], sc.T, shifts[s], floor=-25, unknown_value=-6)
            assert score == scores[k].reshape(-1)[s] and n_used == used[k], (k, shifts[s])
            assert known <= inside <= n_used < 300
            seen_outside |= inside < n_used
            seen_unknown |= known < inside
    assert seen_outside and (seen_unknown or dims == (1, 1, 1))


def test_voxels_ref_follows_the_definition():
    f32 = np.float32
    R = synth.scan_rotation([np.cos(0.15), 0.0, 0.0, np.sin(0.15)])
    pts = np.array([[0.3, -0.2, 0.1], [np.nan, 0, 0], [np.inf, 0, 0], [1e6, 0, 0], [-300.0, 0, 0]], dtype=f32)
    v, ok = synth.scan_voxels_ref(pts, R, (0.25, 0.5, 0.0), (0.0, 0.0, 0.0), 0.125)
    assert ok.tolist() == [True, False, False, False, False]
    p = pts[0]
    w = [f32(f32(f32(f32(R[a, 0] * p[0]) + f32(R[a, 1] * p[1])) + f32(R[a, 2] * p[2])) + f32(t)) for a, t in enumerate((0.25, 0.5, 0.0))]
    assert v[0].tolist() == [int(np.floor(f32(x / f32(0.125)) * 256)) >> 8 for x in w]
    # the apron takes part: -2048 voxels is in range, beyond it is not
    edge = np.array([[-2048 * 0.125, 0, 0], [-2048.5 * 0.125, 0, 0], [4095.5 * 0.125, 0, 0], [4096 * 0.125, 0, 0]], dtype=f32)
    v, ok = synth.scan_voxels_ref(edge, np.eye(3), (0, 0, 0), (0, 0, 0), 0.125)
    assert ok.tolist() == [True, False, True, False] and v[0, 0] == -2048 and v[2, 0] == 4095


def test_table_and_best_refs():
    L = np.array([[[-128, -127, 127], [-40, 0, 70]]], dtype=np.int64)        # (1, 2, 3)
    img = synth.scan_table_ref(L, floor=-10, unknown_value=-8)
    assert img.shape == (256 + 32 * 2,) and not img[:256].any()
    vals = img[256:].astype(np.int64) - 128
    back = vals.reshape(2, 1, 1, 2, 4, 4)   # (bz, by, bx, z&1, y&3, x&3)
    assert back[0, 0, 0, :, 0, 0].tolist() == [-8, -10] and back[1, 0, 0, 0, 0, 0] == 127 and back[0, 0, 0, :, 1, 0].tolist() == [-10, 0]
    assert back[1, 0, 0, 0, 1, 0] == 70 and back[1, 0, 0, 1].tolist() == [[-8] * 4] * 4          # the pad level z = 3
    assert (np.sort(np.unique(vals)) == [-10, -8, 0, 70, 127]).all()
    s = np.zeros((2, 3, 3, 3), dtype=np.int32)
    assert synth.scan_best_ref(s).tolist() == [13, 0, 0, 0, 0, 0, 54, 0]
    s[1, 0, 2, 1] = s[0, 2, 1, 2] = 4           # |s|^2 = 2 (dz -1, dy +1) in k = 1 and 2 (dz +1, dx +1) in k = 0: the lower index
    assert synth.scan_best_ref(s).tolist() == [2 * 9 + 1 * 3 + 2, 0, 1, 0, 1, 4, 2, 0]
    s[1, 1, 1, 0] = 4                           # |s|^2 = 1
    assert synth.scan_best_ref(s).tolist() == [27 + 9 + 3, 1, -1, 0, 0, 4, 3, 0]


# ---- the end-to-end scene, by the restatement alone -----------------------------------------------------------------------------------

def test_the_restatement_recovers_the_planted_offset_uniquely():
    from trajectory_optimization_amd import tools
    occ = sc.room_occupancy()
    L = sc.room_log_odds(occ)
    pts = sc.scene_scan_ref()
    assert len(pts) > 2000
    t, q, half = sc.prior_pose()
    cands = tools.yaw_candidates(q, half, sc.YAW_STEPS)
    Rs = [synth.scan_rotation(c) for c in cands]
    scores, used = synth.scan_correlate_ref(L, sc.ROOM["origin"], sc.ROOM["resolution"], pts, Rs, t, sc.WINDOW)
    best = synth.scan_best_ref(scores)
    k = sc.YAW_STEPS // 2 + sc.PLANTED_STEPS
    assert best[1] == k and tuple(best[2:5]) == sc.PLANTED_SHIFT and best[6] == 1
    assert best[5] == 70 * len(pts) and (used == len(pts)).all()       # every return lands on an occupied voxel, at that candidate only
    assert np.sort(scores.reshape(-1))[-2] < best[5]
    # every return is half a voxel from the faces of its voxel at the true pose: the f32 roundings cannot matter
    true_t, true_q = sc.true_pose()
    w = pts.astype(np.float64) @ synth.scan_rotation(true_q).astype(np.float64).T + true_t
    g = (w - np.asarray(sc.ROOM["origin"])) / sc.ROOM["resolution"]
    assert np.abs(g - np.floor(g) - 0.5).max() < 1e-3
