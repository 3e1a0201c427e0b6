"""CPU checks of the evidence map (no GPU): the four entry points are declared in the header and in _lib's table at ABI 15; each
refuses bad arguments before any launch; ops.check_evidence refuses by name; and the numpy restatements (synth.evidence_fold_ref /
evidence_planes_ref / evidence_brick_order / evidence_scan_ref / pillar_scan, what the kernels are compared against bit for bit) are
checked on hand cases, on the order of scans, and on the scene of the moving obstacle: a pillar scanned twice, then gone."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_evid_bytes", "tohip_evid_init", "tohip_evid_fold", "tohip_evid_positions")
DIMS = (5, 6, 3)


def test_header_and_table_declare_the_new_entries_at_abi_15():
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_evid_fold" in before
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert '#include "field_kernels.hip"\n#include "evidence_kernels.hip"' in src


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    e, h, m, o, f, c, x = (ctypes.c_void_p(v) for v in (4096, 8192, 16384, 32768, 65536, 131072, 262144))   # pointers no call may reach
    geom = lambda org=(0.0, 0.0, 0.0), res=0.1, d=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*org), res, (ctypes.c_int32 * 3)(*d))
    ok = geom()
    nb, eb = L.tohip_occ_bytes(64, 64, 32), L.tohip_evid_bytes(64, 64, 32)
    assert eb == 256 + 32 * (16 * 16 * 16) and L.tohip_evid_bytes(5, 6, 3) == 256 + 32 * 8 and L.tohip_evid_bytes(1, 1, 1) == 288
    for bad in ((0, 4, 4), (4, 4, 2049), (2048, 2048, 2048)):
        assert L.tohip_evid_bytes(*bad) == 0, bad
    bad_geoms = [geom(org=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 64, 32)), geom(d=(64, 2049, 32))]
    calls = {
        "init": (L.tohip_evid_init, ("evid", "bytes", "geom", "stream"), (e, eb, ok, None)),
        "fold": (L.tohip_evid_fold, ("evid", "bytes", "hit_plane", "pass_plane", "occ", "free", "grid_bytes", "geom", "hit", "miss", "lmin", "lmax",
                                     "threshold", "clear", "counts", "stream"), (e, eb, h, m, o, f, nb, ok, 17, 8, -40, 70, 0, 1, c, None)),
        "positions": (L.tohip_evid_positions, ("evid", "bytes", "geom", "threshold", "pos", "m", "values", "state", "stream"),
                      (e, eb, ok, 0, h, 10, m, o, None)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name in calls:
        assert call(name, evid=None) == EINVAL, name
        assert call(name, geom=None) == EINVAL, name
        assert call(name, evid=ctypes.c_void_p(4100)) == EINVAL, name   # (the values move 16 bytes at a time)
        assert call(name, bytes=eb - 1) == ENOSPC, name
        for g in bad_geoms:
            assert call(name, geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    for kw in (dict(hit_plane=None), dict(pass_plane=None), dict(occ=None), dict(free=None),
               dict(hit=0), dict(hit=128), dict(hit=-17), dict(miss=0), dict(miss=128), dict(lmin=-128), dict(lmax=128), dict(lmin=1), dict(threshold=70),
               dict(threshold=71), dict(threshold=-41), dict(lmin=5, lmax=5, threshold=5),
               # any two of the planes, or a plane and the evidence buffer, are one buffer
               dict(pass_plane=h), dict(occ=h), dict(free=h), dict(occ=m), dict(free=m), dict(free=o), dict(hit_plane=e), dict(pass_plane=e),
               dict(occ=e), dict(free=e)):
        assert call("fold", **kw) == EINVAL, kw
    assert call("fold", grid_bytes=nb - 1) == ENOSPC
    for kw in (dict(pos=None), dict(m=-1), dict(values=None, state=None), dict(threshold=127), dict(threshold=-128)):
        assert call("positions", **kw) == EINVAL, kw
    assert call("positions", m=0, pos=None, values=None, state=None) == 0   # (an empty query launches nothing)


def test_check_evidence_names_every_refusal():
    from trajectory_optimization_amd import ops, tools

    class G(ops.OccupancyGrid):   # a grid's geometry without a device
        def __init__(self, origin=(0, 0, 0), resolution=0.1, dims=(8, 8, 4), device="cuda:0"):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, resolution, dims)
            self.device = torch.device(device)

    o, r, d, p = ops.check_evidence((0, 0, 0), 0.1, (8, 8, 4))
    assert d == (8, 8, 4) and p == (17, 8, -40, 70, 0) == synth.evidence_params() == tuple(ops.EVID_DEFAULTS.values())
    assert ops.check_evidence((0, 0, 0), 0.1, (8, 8, 4), np.int64(127), 127, -127, 127, 0)[3] == (127, 127, -127, 127, 0)
    assert ops.check_evidence((0, 0, 0), 0.1, (8, 8, 4), 1, 1, 5, 6, 5)[3] == (1, 1, 5, 6, 5)
    with pytest.raises(ValueError, match="dims must be three integers"):
        ops.check_evidence((0, 0, 0), 0.1, (8, 8))
    with pytest.raises(ValueError, match="resolution must be a finite number > 0"):
        ops.check_evidence((0, 0, 0), 0.0, (8, 8, 4))
    for name in ("hit", "miss"):
        for bad in (0, 128, -1, 17.0, True, None, "x"):
            with pytest.raises(ValueError, match=f"{name} must be an integer in \\[1, 127\\]"):
                ops.check_evidence((0, 0, 0), 0.1, (8, 8, 4), **{name: bad})
    for name in ("lmin", "lmax", "threshold"):
        for bad in (1.5, True, None, "x"):
            with pytest.raises(ValueError, match=f"{name} must be an integer, got"):
                ops.check_evidence((0, 0, 0), 0.1, (8, 8, 4), **{name: bad})
    for bad in (dict(lmin=-128), dict(lmax=128), dict(lmin=1), dict(threshold=70), dict(threshold=-41), dict(lmin=3, lmax=3, threshold=3)):
        with pytest.raises(ValueError, match="the clamps must satisfy -127 <= lmin <= threshold < lmax <= 127"):
            ops.check_evidence((0, 0, 0), 0.1, (8, 8, 4), **bad)
    own, a, b = G(), G(), G()
    kw = dict(like=own, own=(own,))
    assert ops.check_evidence(own.origin, own.resolution, own.dims, hit_plane=a, pass_plane=b, **kw)[2] == (8, 8, 4)
    with pytest.raises(ValueError, match="hit_plane and pass_plane must be given together"):
        ops.check_evidence(own.origin, own.resolution, own.dims, hit_plane=a, **kw)
    with pytest.raises(ValueError, match="pass_plane must be an ops.OccupancyGrid, got Tensor"):
        ops.check_evidence(own.origin, own.resolution, own.dims, hit_plane=a, pass_plane=torch.zeros(3), **kw)
    with pytest.raises(ValueError, match="hit_plane must be an ops.OccupancyGrid, got SpaceMap"):
        ops.check_evidence(own.origin, own.resolution, own.dims, hit_plane=ops.SpaceMap(a, b), pass_plane=b, **kw)
    with pytest.raises(ValueError, match="pass_plane must not be the hit plane itself"):
        ops.check_evidence(own.origin, own.resolution, own.dims, hit_plane=a, pass_plane=a, **kw)
    with pytest.raises(ValueError, match="hit_plane must not be one of the map's own planes"):
        ops.check_evidence(own.origin, own.resolution, own.dims, hit_plane=own, pass_plane=b, **kw)
    for other, what in ((G(origin=(0, 0, 0.5)), "origin"), (G(resolution=0.2), "resolution"), (G(dims=(8, 8, 5)), "dims"), (G(device="cuda:1"), "device")):
        with pytest.raises(ValueError, match=f"pass_plane: its {what} differs from the map's"):
            ops.check_evidence(own.origin, own.resolution, own.dims, hit_plane=a, pass_plane=other, **kw)
    with pytest.raises(ValueError, match="EvidenceMap.like: grid must be an ops.OccupancyGrid"):
        ops.EvidenceMap.like(torch.zeros(3))
    with pytest.raises(ValueError, match="EvidenceMap.from_space: space must be an ops.SpaceMap"):
        ops.EvidenceMap.from_space(own)
    with pytest.raises(ValueError, match="hit must be an integer in \\[1, 127\\]"):
        tools.evidence_map(own, hit=0)


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def _one(L0, h, m, params=None, at=(4, 5, 2)):
    """One voxel of a (5, 6, 3) grid holding L0, folded with its hit bit h and pass bit m -> (its new value, counts, every other value)."""
    L = np.full(DIMS, -128, dtype=np.int64)
    H, M = np.zeros(DIMS, dtype=bool), np.zeros(DIMS, dtype=bool)
    L[at], H[at], M[at] = L0, h, m
    out, counts = synth.evidence_fold_ref(L, H, M, params)
    assert out.dtype == np.int64 and counts.dtype == np.int64 and L[at] == L0   # (the input is not modified)
    rest = out.copy()
    rest[at] = -128
    assert (rest == -128).all()
    return int(out[at]), counts.tolist()


def test_the_fold_by_hand():
    assert _one(-128, True, False) == (17, [1, 1, 1, 0])      # unknown + hit
    assert _one(-128, False, True) == (-8, [1, 1, 0, 0])      # unknown + miss
    assert _one(-128, True, True) == (17, [1, 1, 1, 0])       # a hit wins within a scan
    assert _one(20, True, True) == (37, [1, 0, 0, 0])
    assert _one(70, True, False) == (70, [1, 0, 0, 0])        # the clamps
    assert _one(60, True, False) == (70, [1, 0, 0, 0])
    assert _one(-40, False, True) == (-40, [1, 0, 0, 0])
    assert _one(-35, False, True) == (-40, [1, 0, 0, 0])
    assert _one(5, False, False) == (5, [0, 0, 0, 0])         # not observed: unchanged
    assert _one(-128, False, False) == (-128, [0, 0, 0, 0])
    assert _one(0, False, True) == (-8, [1, 0, 0, 0]) and _one(0, True, False) == (17, [1, 0, 1, 0])   # a known 0 is not the unknown
    assert _one(5, False, True) == (-3, [1, 0, 0, 1])         # an occupied voxel vanishes
    # the threshold itself is free, threshold + 1 is occupied
    for t in (0, -7, 20):
        p = dict(hit=1, miss=1, lmin=-40, lmax=70, threshold=t)
        assert _one(t, True, False, p) == (t + 1, [1, 0, 1, 0]) and _one(t + 1, False, True, p) == (t, [1, 0, 0, 1])
        L = np.array([[[-128, t - 1, t, t + 1, 70]]], dtype=np.int64)
        occ, free = synth.evidence_planes_ref(L, t)
        assert occ.tolist() == [[[False, False, False, True, True]]] and free.tolist() == [[[False, True, True, False, False]]]
    # a whole grid at once, and the pad bytes of its buffer
    rng = np.random.default_rng(5)
    L = np.where(rng.random(DIMS) < 0.3, -128, rng.integers(-40, 71, DIMS))
    H, M = rng.random(DIMS) < 0.3, rng.random(DIMS) < 0.5
    out, counts = synth.evidence_fold_ref(L, H, M)
    for v in np.ndindex(*DIMS):
        assert (int(out[v]), ) == _one(int(L[v]), bool(H[v]), bool(M[v]), at=v)[:1]
    assert counts[0] == (H | M).sum() and counts[1] == ((H | M) & (L == -128)).sum() and (H & M).any()
    img = synth.evidence_brick_order(out)
    assert img.dtype == np.uint8 and img.shape == (256 + 32 * 2 * 2 * 2,) and not img[:256].any()
    back, pads = synth.evidence_from_brick_order(img, DIMS)
    assert np.array_equal(back, out) and len(pads) == 8 * 8 * 4 - 90 and (pads == -128).all()


@pytest.mark.parametrize("dims", [(1, 1, 1), DIMS, (37, 5, 20), (8, 8, 4)], ids=str)
def test_brick_order_round_trips(dims):
    rng = np.random.default_rng(dims[0])
    L = rng.integers(-128, 128, dims)
    img = synth.evidence_brick_order(L)
    nbx, nby, nbz = (dims[0] + 3) // 4, (dims[1] + 3) // 4, (dims[2] + 1) // 2
    assert img.shape == (256 + 32 * nbx * nby * nbz,)
    back, pads = synth.evidence_from_brick_order(img, dims)
    assert np.array_equal(back, L) and (pads == -128).all() and len(pads) == 32 * nbx * nby * nbz - L.size
    # byte 32 w + b, spelled out
    for x, y, z in ((0, 0, 0), (dims[0] - 1, dims[1] - 1, dims[2] - 1), (dims[0] // 2, dims[1] // 3, dims[2] // 2)):
        w = ((z >> 1) * nby + (y >> 2)) * nbx + (x >> 2)
        b = (x & 3) | ((y & 3) << 2) | ((z & 1) << 4)
        assert img[256 + 32 * w + b].view(np.int8) == L[x, y, z]


def test_scans_commute_until_a_clamp_is_reached():
    rng = np.random.default_rng(9)
    scans = [(rng.random(DIMS) < 0.4, rng.random(DIMS) < 0.6) for _ in range(3)]
    empty = np.full(DIMS, -128, dtype=np.int64)

    def run(order, params):
        L = empty
        for k in order:
            L, _ = synth.evidence_fold_ref(L, *scans[k], params)
        return L

    wide = dict(hit=17, miss=8, lmin=-127, lmax=127, threshold=0)
    want = run((0, 1, 2), wide)
    assert np.abs(want[want != -128]).max() < 127
    for order in ((0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        assert np.array_equal(run(order, wide), want), order
    # lmax = 10: a hit reaches the clamp.  One voxel, hit in one scan and passed in the other: 0 + 17 -> 10, - 8 = 2; but - 8, + 17 = 9
    tight = dict(hit=17, miss=8, lmin=-40, lmax=10, threshold=0)
    H = np.zeros(DIMS, dtype=bool)
    H[2, 3, 1] = True
    hit_scan, pass_scan = (H, np.zeros(DIMS, dtype=bool)), (np.zeros(DIMS, dtype=bool), H)
    a, _ = synth.evidence_fold_ref(synth.evidence_fold_ref(empty, *hit_scan, tight)[0], *pass_scan, tight)
    b, _ = synth.evidence_fold_ref(synth.evidence_fold_ref(empty, *pass_scan, tight)[0], *hit_scan, tight)
    assert a[2, 3, 1] == 2 and b[2, 3, 1] == 9
    a, _ = synth.evidence_fold_ref(synth.evidence_fold_ref(empty, *hit_scan, wide)[0], *pass_scan, wide)
    b, _ = synth.evidence_fold_ref(synth.evidence_fold_ref(empty, *pass_scan, wide)[0], *hit_scan, wide)
    assert a[2, 3, 1] == 9 == b[2, 3, 1]


def test_pillar_scan_moves_the_returns_to_the_entry_point():
    room = np.float32([[2.0, 1.0, 0.5], [2.0, 1.9, 0.5], [0.0, 1.0, 0.5], [1.15, 1.0, 1.0], [2.0, 1.0, 0.1]])
    got = synth.pillar_scan(room, (0.5, 1.0, 0.5), (1.0, 0.8, 0.0), (1.3, 1.2, 0.7))
    assert got.dtype == np.float32
    assert got[0].tolist() == [1.0, 1.0, 0.5] and np.array_equal(got[1:4], room[1:4])   # beside, away from and above the box: untouched
    assert np.allclose(got[4], [1.0, 1.0, 0.5 - 0.4 / 3], atol=1e-6)


def test_a_pillar_scanned_twice_is_gone_after_five_scans_without_it():
    S = synth.EVID_SCENE
    o, r, dims, scanner = S["origin"], S["resolution"], S["dims"], S["scanner"]
    room = synth.box_room(step=S["step"])
    with_pillar = synth.pillar_scan(room, scanner, *S["pillar"])
    assert len(room) == 10506 and 1400 < (with_pillar != room).any(axis=1).sum() < 1560
    L = np.full(dims, -128, dtype=np.int64)
    _, _, skipped, H_room, M_room = synth.evidence_scan_ref(L, scanner, room, o, r, dims)
    _, _, skipped_p, H_pillar, _ = synth.evidence_scan_ref(L, scanner, with_pillar, o, r, dims)
    assert skipped == 0 == skipped_p
    only = H_pillar & ~H_room   # the voxels only the pillar's returns occupy
    # (not vacuous: there are such voxels, and every one is crossed — not hit — by the rays of every scan of the empty room)
    assert only.sum() >= 20 and M_room[only].all() and not H_room[only].any()
    a, b = np.float32([S["leg"][0]]), np.float32([S["leg"][1]])
    for _ in range(2):
        L, counts, _, _, _ = synth.evidence_scan_ref(L, scanner, with_pillar, o, r, dims)
    assert (L[only] == 2 * 17).all()
    for k in range(1, 9):
        L, counts, _, _, _ = synth.evidence_scan_ref(L, scanner, room, o, r, dims)
        occ, free = synth.evidence_planes_ref(L)
        assert occ[H_room].all() and H_room.sum() > 1500, k        # the room's own surfaces never leave
        assert not (occ & free).any()
        if k <= 4:
            assert (L[only] == 34 - 8 * k).all() and occ[only].all() and synth.los_ref(a, b, o, r, occ).tolist() == [0], k
        else:
            assert (L[only] == max(34 - 8 * k, -40)).all() and free[only].all() and synth.los_ref(a, b, o, r, occ).tolist() == [1], k
        assert counts[3] == (only.sum() if k == 5 else 0)
