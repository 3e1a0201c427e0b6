"""CPU checks of free-space carving, the three-state map, frontiers and the ordered listing (no GPU): the new entry points are
declared in the header and in _lib's table at ABI 15; each refuses bad arguments before any launch; the host layer refuses by name;
and the numpy restatements (synth.carve_ref / state_ref / frontier_ref / occ_export_ref, what the kernels are compared against bit
for bit) are checked on hand cases, against los_fixed's trace, and on a scanned room with and without a doorway."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_occ_carve", "tohip_occ_state", "tohip_occ_frontier", "tohip_occ_export_workspace_bytes", "tohip_occ_count",
           "tohip_occ_export")
SCENE = dict(origin=(-0.5, -0.5, -0.5), resolution=0.125, dims=(28, 24, 16))
SCANNER = np.float32([1.03, 0.97, 0.52])


def test_header_and_table_declare_the_new_entries_at_abi_15():
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_occ_carve" in before
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert '#include "occupancy_kernels.hip"\n#include "frontier_kernels.hip"' in src


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    p, q, r, t = ctypes.c_void_p(64), ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(16384)   # pointers no call may reach
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))
    ok = geom()
    nb = L.tohip_occ_bytes(64, 64, 32)
    ws = L.tohip_occ_export_workspace_bytes(64, 64, 32)
    assert ws == 8 * (16 * 16 * 16 // 256 + 1) and L.tohip_occ_export_workspace_bytes(1, 1, 1) == 16
    for bad in ((0, 4, 4), (4, 4, 2049), (2048, 2048, 2048)):
        assert L.tohip_occ_export_workspace_bytes(*bad) == 0, bad
    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 64, 32)), geom(d=(64, 2049, 32))]
    calls = {
        "carve": (L.tohip_occ_carve, ("grid", "bytes", "geom", "origins", "stride", "points", "n", "R", "flags", "stats", "skipped", "stream"),
                  (p, nb, ok, q, 0, r, 10, 0, None, None, None, None)),
        "state": (L.tohip_occ_state, ("grid", "free", "bytes", "geom", "pos", "m", "out", "stream"), (p, q, nb, ok, r, 10, t, None)),
        "frontier": (L.tohip_occ_frontier, ("occ", "free", "grid", "bytes", "geom", "k", "stream"), (p, q, r, nb, ok, 1, None)),
        "count": (L.tohip_occ_count, ("grid", "bytes", "geom", "ws", "ws_bytes", "total", "stream"), (p, nb, ok, q, ws, None, None)),
        "export": (L.tohip_occ_export, ("grid", "bytes", "geom", "ws", "ws_bytes", "total", "capacity", "ijk", "centres", "stream"),
                   (p, nb, ok, q, ws, 7, 7, r, t, None)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name in calls:
        assert call(name, grid=None) == EINVAL, name
        assert call(name, geom=None) == EINVAL, name
        assert call(name, bytes=nb - 1) == ENOSPC, name
        for g in bad_geoms:
            assert call(name, geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    for kw in (dict(origins=None), dict(points=None), dict(n=-1), dict(stride=1), dict(stride=-3), dict(stride=4), dict(R=-1),
               dict(R=6144 * 256 + 1)):
        assert call("carve", **kw) == EINVAL, kw
    for kw in (dict(free=None), dict(pos=None), dict(out=None), dict(m=-1)):
        assert call("state", **kw) == EINVAL, kw
    for kw in (dict(occ=None), dict(free=None), dict(k=0), dict(k=7), dict(k=-1), dict(grid=p), dict(grid=q)):
        assert call("frontier", **kw) == EINVAL, kw
    assert call("count", ws=None) == EINVAL and call("count", ws_bytes=ws - 1) == ENOSPC
    for kw in (dict(ws=None), dict(total=-1), dict(capacity=-1), dict(ijk=None), dict(centres=None)):
        assert call("export", **kw) == EINVAL, kw
    assert call("export", ws_bytes=ws - 1) == ENOSPC and call("export", capacity=6) == ENOSPC   # a capacity short by one
    # (empty queries are fine and launch nothing)
    assert call("state", m=0, pos=None, out=None) == 0 and call("export", total=0, capacity=0, ijk=None, centres=None) == 0


def test_check_carve_and_space_map_name_what_is_wrong():
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.tools import space_map, frontier_points, known_free
    P = torch.zeros(5, 3)
    assert ops.check_carve(torch.zeros(3), P) == 0 and ops.check_carve(torch.zeros(1, 3), P) == 0 and ops.check_carve(P + 1, P) == 0
    assert ops.check_carve((0.0, 1.0, 2.0), P) == 0 and ops.check_carve(np.zeros(3), P, 1.5, 0.125) == 3072
    r = float(np.float32(0.1))
    assert ops.check_carve(torch.zeros(3), P, 1.5, 0.1) == math.floor(1.5 / r * 256) == synth.carve_range(1.5, 0.1)
    assert ops.check_carve(torch.zeros(3), P, 0.125 / 256, 0.125) == 1 and ops.check_carve(torch.zeros(3), P, 6144 * 0.125, 0.125) == 6144 * 256
    for bad in (torch.zeros(5, 2), torch.zeros(5), torch.zeros(5, 3, dtype=torch.int32), np.zeros((5, 3)), None):
        with pytest.raises(ValueError, match="points must be an \\(N,3\\) floating-point tensor"):
            ops.check_carve(torch.zeros(3), bad)
    for bad in (torch.zeros(2), torch.zeros(4, 3), torch.zeros(2, 3), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 1), "abc", None):
        with pytest.raises(ValueError, match="origins must be a \\(3,\\) or \\(1,3\\) floating-point tensor .* points' 5 rows"):
            ops.check_carve(bad, P)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 0.125 / 257, 6144 * 0.125 + 0.001, "x", True):
        with pytest.raises(ValueError, match="max_range must be None or a finite number of metres"):
            ops.check_carve(torch.zeros(3), P, bad, 0.125)
    for bad in (0, 7, 1.0, True, None):
        with pytest.raises(ValueError, match="min_unknown must be an integer in \\[1, 6\\]"):
            ops.check_min_unknown(bad)
    assert [ops.check_min_unknown(k) for k in (1, np.int64(6))] == [1, 6]

    class G(ops.OccupancyGrid):   # the planes' geometry without a device
        def __init__(self, origin=(0, 0, 0), resolution=0.1, dims=(8, 8, 4), device="cuda:0"):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, resolution, dims)
            self.device = torch.device(device)

    a = G()
    ops.check_space_planes(a, G())
    for free, what in ((G(origin=(0, 0, 0.5)), "origins differ"), (G(resolution=0.2), "resolutions differ"), (G(dims=(8, 8, 5)), "dims differ"),
                       (G(device="cuda:1"), "planes live on cuda:0 and cuda:1"), (a, "must not be the occupied grid itself"),
                       (object(), "free must be an ops.OccupancyGrid")):
        with pytest.raises(ValueError, match="SpaceMap: .*" + what):
            ops.SpaceMap(a, free)
    with pytest.raises(ValueError, match="SpaceMap: occupied must be an ops.OccupancyGrid"):
        space_map(None)
    with pytest.raises(ValueError, match="frontier_points: space must be an ops.SpaceMap"):
        frontier_points(a)
    with pytest.raises(ValueError, match="known_free: space must be an ops.SpaceMap"):
        known_free(a, P)


# ---- the restatement of the carve ------------------------------------------------------------------------------------------------

def _fx(*v):
    return np.array([int(round(c * 256)) for c in v], dtype=np.int64)


def _carve(a, b, R=0, dims=(8, 8, 8)):
    """One ray in fixed point -> (the set of free voxels, hit)."""
    free = np.zeros(dims, dtype=bool)
    Bc, hit = synth.carve_clip(a[None, :], b[None, :], R)
    synth.carve_fixed(a[None, :], Bc, hit, free)
    return [tuple(int(c) for c in v) for v in np.argwhere(free)], bool(hit[0])


def test_hand_cases_of_the_carve():
    # A = B: a hit in the origin's own voxel sets nothing
    assert _carve(_fx(2.5, 3.5, 1.5), _fx(2.5, 3.5, 1.5)) == ([], True)
    assert _carve(_fx(2.25, 3.5, 1.5), _fx(2.75, 3.25, 1.5)) == ([], True)
    # an axis ray over three voxels sets the first two
    assert _carve(_fx(1.5, 2.5, 3.5), _fx(3.5, 2.5, 3.5)) == ([(1, 2, 3), (2, 2, 3)], True)
    # the same ray truncated at R = 1.5 voxels from the voxel centre: B' = (3.0, ...) lies in voxel 3, and a truncated ray carves
    # its last voxel too — exactly the voxels up to and including B''s
    assert _carve(_fx(1.5, 2.5, 3.5), _fx(3.5, 2.5, 3.5), R=256 + 128) == ([(1, 2, 3), (2, 2, 3), (3, 2, 3)], False)
    assert _carve(_fx(1.5, 2.5, 3.5), _fx(7.5, 2.5, 3.5), R=256 + 127) == ([(1, 2, 3), (2, 2, 3)], False)
    # the (1,1,1) diagonal follows los_fixed's tie order: x, then y, then z at every corner
    got, hit = _carve(_fx(0.5, 0.5, 0.5), _fx(2.5, 2.5, 2.5))
    assert hit and got == sorted([(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1)])
    # a ray from the apron through dims and out into the apron again sets only the inside voxels
    got, _ = _carve(_fx(1.5, 0.5, 0.5), _fx(1.5, -1.5, 0.5), dims=(4, 4, 4))
    assert got == [(1, 0, 0)]
    got, _ = _carve(_fx(0.25, 0.75, 0.5), _fx(-0.75, 3.75, 0.5), dims=(4, 4, 4))               # out through x = 0 at y = 1.5
    assert got == [(0, 0, 0), (0, 1, 0)]
    got, _ = _carve(_fx(-0.5, 0.5, 0.5), _fx(3.5, -0.5, 0.5), dims=(4, 4, 4))                  # in through x = 0, out through y = 0
    assert got == [(0, 0, 0), (1, 0, 0)]
    got, _ = _carve(_fx(0.5, -0.25, 0.5), _fx(-0.25, 0.5, 0.5), dims=(4, 4, 4))                # apron -> corner voxel -> apron
    assert got == [(0, 0, 0)]
    # R = 1: B' = A to within a 256th of a voxel — the origin's voxel, carved because the ray is no hit
    assert _carve(_fx(2.5, 3.5, 1.5), _fx(6.5, 3.5, 1.5), R=1) == ([(2, 3, 1)], False)
    assert _carve(_fx(2.5, 3.5, 1.5), _fx(2.5, 3.5, 1.5), R=1) == ([], True)


def test_the_isqrt_boundaries_of_truncation():
    A = np.zeros((1, 3), dtype=np.int64)
    # D . D = R^2: not truncated; R^2 + 1 (L = R still): not truncated either; (R + 1)^2: truncated
    for D, R, cut in (((300, 400, 0), 500, False), ((300, 400, 1), 500, False), ((300, 400, 31), 500, False), ((300, 400, 32), 500, True),
                      ((0, 0, 501), 500, True), ((0, -501, 0), 500, True), ((1, 0, 0), 1, False), ((1, 1, 1), 1, False), ((2, 0, 0), 1, True),
                      ((10 ** 6, 10 ** 6, 10 ** 6), 0, False)):
        B = np.array([D], dtype=np.int64)
        Bc, hit = synth.carve_clip(A, B, R)
        assert bool(hit[0]) == (not cut), (D, R)
        if cut:
            L = math.isqrt(sum(d * d for d in D))
            assert Bc[0].tolist() == [int(np.sign(d)) * (abs(d) * R // L) for d in D]
        else:
            assert np.array_equal(Bc, B)
    assert synth.carve_clip(A, np.array([[-700, 0, 2400]]), 1000)[0].tolist() == [[-280, 0, 960]]


def test_carve_fixed_equals_the_trace_of_los_fixed():
    rng = np.random.default_rng(4)
    dims = (12, 10, 6)
    span = np.array(dims)[None, :] * 256
    n = 600
    A = rng.integers(-2 * 256, span + 2 * 256, size=(n, 3))
    B = rng.integers(-2 * 256, span + 2 * 256, size=(n, 3))
    A[:100] = (A[:100] >> 8) << 8   # origins on faces and corners
    for R in (0, 700, 3000):
        Bc, hit = synth.carve_clip(A, B, R)
        free = np.zeros(dims, dtype=bool)
        visits = synth.carve_fixed(A, Bc, hit, free)
        _, visited = synth.los_fixed(A, Bc, np.zeros(dims, dtype=bool), skip=(0, 0), trace=True)
        want = np.zeros(dims, dtype=bool)
        for i, vs in enumerate(visited):
            for v in (vs[:-1] if hit[i] else vs):
                if all(0 <= c < d for c, d in zip(v, dims)):
                    want[v] = True
        assert np.array_equal(free, want) and visits == sum(len(v) for v in visited), R
        assert (R == 0) == bool(hit.all()) and (R != 700 or not hit.all())
        # B' lies between A and B
        assert (np.abs(Bc - A) <= np.abs(B - A)).all() and (np.sign(Bc - A) * np.sign(B - A) >= 0).all()


def test_carve_ref_skips_counts_and_is_order_free():
    o, r, dims = (0.0, 0.0, 0.0), 0.125, (16, 16, 8)
    rng = np.random.default_rng(9)
    P = (rng.random((400, 3)) * np.array([3.0, 3.0, 1.5]) - 0.5).astype(np.float32)
    P[3], P[5], P[7] = [np.nan, 0, 0], [600.0, 0, 0], [0, np.inf, 0]
    org = np.float32([0.7, 0.6, 0.4])
    free, skipped, flags, _ = synth.carve_ref(org, P, o, r, dims, max_range=1.0)
    assert skipped == 3 and flags[[3, 5, 7]].tolist() == [2, 2, 2] and (flags == 1).any() and (flags == 0).any()
    perm = rng.permutation(400)
    f1, s1, _, _ = synth.carve_ref(org[None, :], P[perm][:150], o, r, dims, max_range=1.0)
    f2, s2, _, _ = synth.carve_ref(np.broadcast_to(org, (250, 3)), P[perm][150:], o, r, dims, max_range=1.0, free=f1)
    assert np.array_equal(f2, free) and s1 + s2 == 3
    assert np.array_equal(synth.carve_ref(org, P, o, r, dims, max_range=1.0, free=free)[0], free)
    # an origin out of range: every ray is skipped
    assert synth.carve_ref(np.float32([np.nan, 0, 0]), P, o, r, dims)[1] == 400


# ---- state, frontier, export -------------------------------------------------------------------------------------------------------

def test_state_ref_over_the_three_states():
    occ, free = np.zeros((4, 4, 2), dtype=bool), np.zeros((4, 4, 2), dtype=bool)
    occ[1, 1, 0] = free[1, 1, 0] = free[2, 1, 0] = True   # occupied wins
    pos = np.float32([[0.15, 0.15, 0.05], [0.25, 0.15, 0.05], [0.35, 0.15, 0.05], [0.45, 0.15, 0.05], [-0.05, 0.15, 0.05], [0.15, 0.15, 0.25],
                      [np.nan, 0, 0], [0, 500.0, 0], [0.15, np.inf, 0]])
    assert synth.state_ref(pos, (0, 0, 0), 0.1, occ, free).tolist() == [2, 1, 0, 3, 3, 3, 3, 3, 3]


def test_frontier_ref_hand_cases():
    dims = (5, 6, 3)
    none = np.zeros(dims, dtype=bool)
    for v, nbrs in (((0, 0, 0), 3), ((4, 5, 2), 3), ((2, 0, 0), 4), ((0, 3, 2), 4), ((2, 3, 1), 6), ((2, 3, 0), 5)):
        free = none.copy()
        free[v] = True
        for k in range(1, 7):
            fr = synth.frontier_ref(none, free, k)
            assert fr.sum() == (1 if k <= nbrs else 0) and (k > nbrs or fr[v]), (v, k)
    assert not synth.frontier_ref(none, ~none, 1).any()          # all free: the box's own boundary is not unknown
    assert not synth.frontier_ref(~none, ~none, 1).any()         # all occupied (occupied wins)
    free = none.copy()
    free[2, 3, 1] = True
    occ = none.copy()
    occ[1, 3, 1] = occ[2, 3, 2] = True                           # an occupied neighbour does not count
    assert synth.frontier_ref(occ, free, 4)[2, 3, 1] and not synth.frontier_ref(occ, free, 5).any()
    free[3, 3, 1] = True                                         # nor does a free one; and both free voxels are frontiers
    assert synth.frontier_ref(occ, free, 3).sum() == 2 and synth.frontier_ref(occ, free, 4).sum() == 1
    occ[2, 3, 1] = True                                          # an occupied voxel is no frontier, free bit or not
    assert not synth.frontier_ref(occ, free, 1)[2, 3, 1]


@pytest.mark.parametrize("origin,r", [((-20.2, 8188.9, 1e5), 0.1), ((-20.2, 8188.9, 1e5), 0.125), (SCENE["origin"], 0.125), ((0.0, 0.0, 0.0), 0.125),
                                      ((1024.0, -1024.0, 512.0), 0.125)])
def test_export_order_and_the_centres_round_trip(origin, r):
    rng = np.random.default_rng(2)
    dims = (21, 9, 7)
    g = rng.random(dims) < 0.3
    ijk, centres = synth.occ_export_ref(g, origin, r)
    assert ijk.dtype == np.int32 and centres.dtype == np.float32 and len(ijk) == g.sum()
    x, y, z = (ijk[:, k].astype(np.int64) for k in range(3))
    word = ((z >> 1) * 3 + (y >> 2)) * 6 + (x >> 2)
    key = word * 32 + ((x & 3) | ((y & 3) << 2) | ((z & 1) << 4))
    assert (np.diff(key) > 0).all() and g[x, y, z].all()
    # the centre of voxel i maps back to voxel i under occ_fixed, for every index a grid can have
    i = np.arange(2048)
    c = synth.occ_export_ref(np.ones((2048, 1, 1), bool), origin, r)[1]
    q, ok = synth.occ_fixed(c, origin, r)
    assert ok.all() and np.array_equal(np.sort(q[:, 0] >> 8), i)
    for ax in range(3):
        o3 = np.roll(np.asarray(origin, dtype=np.float32), -ax)
        c3 = synth.occ_export_ref(np.ones((2048, 1, 1), bool), o3, r)[1]
        assert np.array_equal(np.sort(synth.occ_fixed(c3, o3, r)[0][:, 0] >> 8), i)
    q, ok = synth.occ_fixed(centres, origin, r)
    assert ok.all() and np.array_equal(q >> 8, ijk)
    assert synth.occ_export_ref(np.zeros(dims, bool), origin, r)[0].shape == (0, 3)


# ---- the scanned room --------------------------------------------------------------------------------------------------------------

def _scan(points, max_range=None):
    free, skipped, flags, _ = synth.carve_ref(SCANNER, points, max_range=max_range, **SCENE)
    occ, _ = synth.occupancy_ref(points[flags != 1], SCENE["origin"], SCENE["resolution"], SCENE["dims"])
    return occ, free, skipped, flags


def test_a_closed_room_has_no_frontier_and_a_doorway_opens_one():
    closed = synth.box_room()
    assert closed.shape == (41006, 3)
    occ, free, skipped, flags = _scan(closed)
    assert skipped == 0 and (flags == 0).all()
    assert int(occ.sum()) == 1026 and int((free & ~occ).sum()) == 1575
    for k in range(1, 7):
        assert not synth.frontier_ref(occ, free, k).any()
    assert (free & occ).sum() > 0.3 * occ.sum()   # rays graze along the walls: occupied wins
    door = synth.box_room(doorway=True)
    assert door.shape == (40081, 3)
    occ, free, _, _ = _scan(door)
    fr = np.argwhere(synth.frontier_ref(occ, free, 1))
    assert len(fr) == 41
    assert (fr >= np.array([13, 10, 4])).all() and (fr <= np.array([19, 13, 10])).all()   # the unscanned cone towards the opening
    # the frontier's centres are known free, and their voxels come back under occ_fixed
    ijk, centres = synth.occ_export_ref(synth.frontier_ref(occ, free, 1), SCENE["origin"], SCENE["resolution"])
    assert (synth.state_ref(centres, SCENE["origin"], SCENE["resolution"], occ, free) == 1).all()
    assert np.array_equal(synth.occ_fixed(centres, SCENE["origin"], SCENE["resolution"])[0] >> 8, ijk)


def test_beams_through_the_doorway_carve_up_to_max_range_and_are_not_inserted():
    door = synth.box_room(doorway=True)
    beams = np.concatenate([synth.doorway_beams(SCANNER), synth.doorway_beams(SCANNER, far=1.9)])   # beyond dims, and inside
    rows = np.concatenate([door, beams])
    occ, free, skipped, flags = _scan(rows, max_range=1.5)
    assert skipped == 0 and (flags[len(door):] == 1).all()
    r = SCENE["resolution"]
    centres = (np.argwhere(free) + 0.5) * r + np.asarray(SCENE["origin"])
    assert np.linalg.norm(centres - SCANNER.astype(np.float64), axis=1).max() <= 1.5 + r   # nothing free beyond max_range + one voxel
    far_voxels = synth.occ_fixed(beams, SCENE["origin"], r)[0] >> 8
    inside = ((far_voxels >= 0) & (far_voxels < np.array(SCENE["dims"]))).all(axis=1)
    assert inside[63:].all() and not inside[:63].any() and not occ[tuple(far_voxels[inside].T)].any()
    occ_all, _ = synth.occupancy_ref(rows, SCENE["origin"], r, SCENE["dims"])
    assert occ_all[tuple(far_voxels[inside].T)].all() and occ.sum() < occ_all.sum()   # (an insert of every row would have held them)
    fr = np.argwhere(synth.frontier_ref(occ, free, 1))
    assert (fr[:, 0] >= 21).any()   # beyond the wall plane x = 2 (index 20): the map now ends outside the room
