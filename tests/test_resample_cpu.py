"""Resampling maps without a GPU ("Resampling maps"): the numpy restatements (synth.evid_resample_ref /
occ_resample_ref) against a per-voxel loop in Python integers; ops.resample_affine's integers at the exact transforms, its error
bound over a 2048-voxel box and its refusals; what the rule reduces to at shifts, quarter turns and half the resolution; the cover
property checked in f64 from the geometry, independently of the integer rule; the default box, like= and merge_maps' union box and
routing; and the C entries' refusals."""
import ctypes
import math

import numpy as np
import pytest

import abi_cases
import resample_cases as cases
from trajectory_optimization_amd import synth

ENTRIES = ("tohip_occ_resample", "tohip_evid_resample")
F = 20
CASE_IDS = [c.name for c in cases.CASES]


def test_abi_entries():
    from trajectory_optimization_amd import _lib
    header, before = abi_cases.check_abi_entries(ENTRIES)
    assert "resample_kernels.hip" in header and "Resampling maps" in header and "new symbols only" in before
    C = _lib.CONSTANTS
    assert C["TOHIP_RESAMPLE_FRAC_BITS"] == F == synth.RESAMPLE_FRAC_BITS
    assert (C["TOHIP_RESAMPLE_NEAREST"], C["TOHIP_RESAMPLE_COVER"], C["TOHIP_RESAMPLE_ANY"], C["TOHIP_RESAMPLE_ALL"]) == (0, 1, 1, 2)
    assert [len(_lib.SIGNATURES[s][1]) for s in ENTRIES] == [13, 21]
    # the reserved flags word behind the stream keeps the entries out of tests/test_hip_contracts.py's count
    assert _lib.SIGNATURES[ENTRIES[0]][1][-2:] == _lib.SIGNATURES[ENTRIES[1]][1][-2:] == [ctypes.c_void_p, ctypes.c_int32]


# ------------------------------------------------------------------------------------------------------- the restatements

@pytest.mark.parametrize("case", cases.CASES, ids=CASE_IDS)
def test_restatements_equal_a_per_voxel_loop(case):
    fills = cases.FILLS if not case.name.startswith("axis rotation") else cases.FILLS[1:2]
    aff = cases.affine(case.name)
    for fill in fills:
        sb, db = cases.bits(case.src.dims, fill), cases.bits(case.dst.dims, 0.3, seed=1)
        L_src, L_dst = cases.values(case.src.dims, fill), cases.values(case.dst.dims, 0.6, seed=1)
        before = sb.copy(), db.copy(), L_src.copy(), L_dst.copy()
        want = cases.resample_loop(sb, db, L_src, L_dst, aff)
        for rule in cases.OCC_RULES:
            for mode in cases.OCC_MODES:
                new, count = synth.occ_resample_ref(sb, db, aff, rule, mode)
                assert new.dtype == bool and np.array_equal(new, want["plane", rule, mode][0]) and count == want["plane", rule, mode][1], (fill, rule, mode)
        for rule in cases.EVID_RULES:
            for mode in cases.EVID_MODES:
                new, counts = synth.evid_resample_ref(L_src, L_dst, aff, rule, mode, cases.PARAMS)
                assert np.array_equal(new, want["evid", rule, mode][0]) and np.array_equal(counts, want["evid", rule, mode][1]), (fill, rule, mode)
        for a, b in zip(before, (sb, db, L_src, L_dst)):
            assert np.array_equal(a, b)   # the inputs are not modified


def test_the_cases_reach_what_they_are_for():
    n = {c.name: synth.resample_nearest(cases.affine(c.name), c.dst.dims) for c in cases.CASES}
    inside = lambda c: np.all([(n[c.name][a] >= 0) & (n[c.name][a] < c.src.dims[a]) for a in range(3)], axis=0)   # noqa: E731
    by = cases.BY_NAME
    assert not inside(by["wholly outside"]).any()
    part = by["partial overlap, negative source indices"]
    assert inside(part).any() and not inside(part).all() and (n[part.name] < 0).any()
    assert (n["half a voxel on every axis, negative indices"] < 0).any()
    for c in cases.CASES:
        assert c.name == "wholly outside" or inside(c).mean() > 0.04, c.name          # every other case has something to read
    for c in cases.CASES:
        if c.name.startswith("axis rotation") or c.name in ("identity same box", "one brick", "twice as fine", "an eighth"):
            assert inside(c).all(), c.name
    L = cases.values(cases.SRC, 0.5)
    p = cases.PARAMS
    assert {synth.EVID_UNKNOWN, p["lmin"], p["threshold"], p["threshold"] + 1, p["lmax"]} <= set(L.reshape(-1).tolist())


def test_restatements_refuse_unknown_rules_and_modes():
    z, aff = np.zeros((2, 2, 2)), cases.affine("one brick")
    with pytest.raises(ValueError, match="rule must be 'nearest' or 'cover'"):
        synth.evid_resample_ref(z, z, aff, "any", "copy")
    with pytest.raises(ValueError, match="rule must be 'nearest', 'any' or 'all'"):
        synth.occ_resample_ref(z, z, aff, "cover", "copy")
    with pytest.raises(ValueError, match="mode must be 'copy' or 'or'"):
        synth.occ_resample_ref(z, z, aff, "any", "add")
    with pytest.raises(ValueError, match="mode must be 'copy', 'add' or 'confident'"):
        synth.evid_resample_ref(z, z, aff, "cover", "or")
    with pytest.raises(ValueError, match="exceeds"):
        synth.resample_nearest([1 << 22] + [0] * 11, (2, 2, 2))


# ------------------------------------------------------------------------------------------------------- the twelve integers

def test_affine_at_the_exact_transforms():
    from trajectory_optimization_amd import ops
    s = cases.Frame(cases.ORIGIN, cases.RES, cases.SRC)
    eye = ((1 << 19) * np.eye(3, dtype=np.int64)).reshape(9)
    a = ops.resample_affine(s, s, (0.0, 0.0, 0.0), cases.IDENTITY)
    assert a.dtype == np.int64 and a.shape == (12,) and np.array_equal(a[:9], eye) and not a[9:].any()
    assert np.array_equal(ops.resample_affine(s, s, (0, 0, 0), (-3.0, 0.0, 0.0, 0.0)), a)   # any length, either sign
    # dst voxel v is src voxel v + k: by the origin, and by the pose the other way round
    for k in ((2, -3, 1), (-7, 0, 4)):
        d = cases.Frame(cases.moved(cases.ORIGIN, k), cases.RES, cases.DST)
        a = ops.resample_affine(s, d, (0.0, 0.0, 0.0), cases.IDENTITY)
        assert np.array_equal(a[:9], eye) and a[9:].tolist() == [v << F for v in k]
        a = ops.resample_affine(s, s, cases.moved((0, 0, 0), k), cases.IDENTITY)
        assert np.array_equal(a[:9], eye) and a[9:].tolist() == [-v << F for v in k]
    # half a voxel: T is half a unit, and the centre of dst voxel i falls on the face between src voxels i - 1 and i
    a = cases.affine("half a voxel")
    assert np.array_equal(a[:9], eye) and a[9:].tolist() == [-(1 << 19), 0, 0]
    # a quarter turn about z: M = 2^19 R^T exactly, T a whole number of voxels
    q = cases.QUARTER_Z
    a = cases.affine(q.name)
    assert a[:9].tolist() == [0, 1 << 19, 0, -(1 << 19), 0, 0, 0, 0, 1 << 19] and not (a[9:] & ((1 << F) - 1)).any()
    for c in cases.CASES:
        if c.name.startswith("axis rotation"):
            a = cases.affine(c.name)
            assert np.array_equal(a[:9].reshape(3, 3), (1 << 19) * np.rint(cases.rotation(c.quat)).astype(np.int64).T), c.name
            assert not (a[9:] & ((1 << F) - 1)).any(), c.name
    # half the resolution: M halves, T moves by a quarter of a source voxel per axis... which is in the (2 i + 1) already: T = 0
    a = cases.affine("twice as fine")
    assert np.array_equal(a[:9], eye // 2) and not a[9:].any()
    assert np.array_equal(cases.affine("an eighth")[:9], eye // 8)


def test_the_floor_takes_the_upper_voxel_on_a_face():
    c = cases.BY_NAME["half a voxel"]
    n = synth.resample_nearest(cases.affine(c.name), c.dst.dims)
    i, j, k = np.meshgrid(*(np.arange(d) for d in c.dst.dims), indexing="ij")
    assert np.array_equal(n[0], i) and np.array_equal(n[1], j) and np.array_equal(n[2], k)   # u = i 2^F exactly: voxel [i, i + 1)
    c = cases.BY_NAME["half a voxel on every axis, negative indices"]
    n = synth.resample_nearest(cases.affine(c.name), c.dst.dims)
    assert np.array_equal(n[0], i - 3) and np.array_equal(n[1], j - 1) and np.array_equal(n[2], k - 2)   # -3 - 1/2 + 1/2, -2 + 1/2 + 1/2, -1 - 3/2 + 1/2
    assert (n < 0).any()                                                                       # >> floors below zero too


def test_affine_error_stays_within_a_128th_of_a_voxel_over_a_2048_box():
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(20)
    corners = np.array([[x, y, z] for x in (0, 2047) for y in (0, 2047) for z in (0, 2047)], dtype=np.int64)
    worst = 0.0
    for trial in range(200):
        ratio = (1.0, 0.5, 0.125, float(rng.uniform(0.125, 1.0)))[trial % 4]
        r_s = float(np.float32(rng.uniform(0.02, 0.5)))
        r_d = float(np.float32(r_s * ratio))
        if r_d > r_s:
            r_d = r_s
        quat = rng.normal(size=4)
        src = cases.Frame(tuple(np.float32(rng.uniform(-50, 50, 3)).tolist()), r_s, (2048, 2048, 2048))
        dst = cases.Frame(tuple(np.float32(rng.uniform(-50, 50, 3)).tolist()), r_d, (2048, 2048, 2048))
        c = cases.Case("random", src, dst, tuple(rng.uniform(-20, 20, 3).tolist()), tuple(quat.tolist()))
        a = ops.resample_affine(src, dst, c.pose, c.quat)
        M, T = a[:9].reshape(3, 3), a[9:]
        u = (2 * corners + 1) @ M.T + T
        worst = max(worst, float(np.abs(u / float(1 << F) - cases.source_position(c, corners)).max()))
    # |2 d + 1| <= 4095 on three axes at half a unit of 2^-19 each, and half a unit of 2^-20 for T: 3 * 4095 * 2^-20 + 2^-21 < 0.0118
    assert worst <= 2.0 ** -7, worst
    assert worst > 2.0 ** -12   # (the bound is not vacuous: the quantisation is seen)


def test_affine_refusals():
    from trajectory_optimization_amd import ops
    s = cases.Frame(cases.ORIGIN, cases.RES, cases.SRC)
    zero = (0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="coarser than the source's.*coarsening is a reduction"):
        ops.resample_affine(s, cases.Frame(cases.ORIGIN, 0.25, cases.DST), zero, cases.IDENTITY)
    with pytest.raises(ValueError, match="coarser"):
        ops.resample_affine(s, cases.Frame(cases.ORIGIN, cases.RES * (1 + 3e-6), cases.DST), zero, cases.IDENTITY)
    ops.resample_affine(s, cases.Frame(cases.ORIGIN, float(np.float32(cases.RES * (1 + 5e-7))), cases.DST), zero, cases.IDENTITY)   # within 1e-6
    with pytest.raises(ValueError, match="finer than an eighth"):
        ops.resample_affine(s, cases.Frame(cases.ORIGIN, cases.RES / 9, cases.DST), zero, cases.IDENTITY)
    ops.resample_affine(s, cases.Frame(cases.ORIGIN, cases.RES / 8, cases.DST), zero, cases.IDENTITY)
    with pytest.raises(ValueError, match=r"beyond 2\^20"):
        ops.resample_affine(s, s, ((2 ** 20 + 2) * cases.RES, 0.0, 0.0), cases.IDENTITY)
    ops.resample_affine(s, s, ((2 ** 20 - 2) * cases.RES, 0.0, 0.0), cases.IDENTITY)
    for pose, quat, text in ((zero, (0.0, 0.0, 0.0, 0.0), "a quaternion of length 0"), (zero, (1.0, 0.0, 0.0), "quat must be"),
                             ((0.0, float("nan"), 0.0), cases.IDENTITY, "pose must be"), ((0.0, 0.0), cases.IDENTITY, "pose must be")):
        with pytest.raises(ValueError, match=text):
            ops.resample_affine(s, s, pose, quat)
    with pytest.raises(ValueError, match="src_frame must be a map or carry origin, resolution and dims"):
        ops.resample_affine(object(), s, zero, cases.IDENTITY)


# ------------------------------------------------------------------------------------------------------- what the rule reduces to

def test_identity_and_integer_shifts_equal_the_transfer():
    from trajectory_optimization_amd import ops
    s = cases.Frame(cases.ORIGIN, cases.RES, cases.SRC)
    sb, db = cases.bits(cases.SRC, 0.3), cases.bits(cases.DST, 0.3, seed=1)
    L_src, L_dst = cases.values(cases.SRC, 0.5), cases.values(cases.DST, 0.6, seed=1)
    for k in ((0, 0, 0), (2, -3, 1), (-5, 2, -1), (13, 0, 0), (-9, -14, -5), (1, 1, 7)):
        aff = ops.resample_affine(s, cases.Frame(cases.moved(cases.ORIGIN, k), cases.RES, cases.DST), (0.0, 0.0, 0.0), cases.IDENTITY)
        for mode in cases.OCC_MODES:
            got, want = synth.occ_resample_ref(sb, db, aff, "nearest", mode), synth.occ_transfer_ref(sb, db, k, mode)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (k, mode)
        for mode in cases.EVID_MODES:
            got, want = synth.evid_resample_ref(L_src, L_dst, aff, "nearest", mode, cases.PARAMS), synth.evidence_transfer_ref(L_src, L_dst, k, mode, cases.PARAMS)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, mode)


def test_a_quarter_turn_is_rot90_of_the_dense_array():
    q = cases.QUARTER_Z
    L = cases.values(cases.SRC, 0.5)
    assert q.dst.dims == (cases.SRC[1], cases.SRC[0], cases.SRC[2])
    got = synth.evid_sample_ref(L, cases.affine(q.name), q.dst.dims, "nearest")
    # x' = -y, y' = x: new index (i', j') holds old (j', ny - 1 - i'), which is np.rot90 from axis 0 towards axis 1
    assert np.array_equal(got, np.rot90(L, 1, axes=(0, 1)))
    b = cases.bits(cases.SRC, 0.3)
    assert np.array_equal(synth.occ_resample_ref(b, np.zeros(q.dst.dims, bool), cases.affine(q.name), "nearest", "copy")[0], np.rot90(b, 1, axes=(0, 1)))
    # every axis rotation keeps the multiset of values: a permutation of the voxels
    for c in cases.CASES:
        if c.name.startswith("axis rotation"):
            got = synth.evid_sample_ref(L, cases.affine(c.name), c.dst.dims, "nearest")
            assert np.array_equal(np.sort(got.reshape(-1)), np.sort(L.reshape(-1))), c.name


def test_half_the_resolution_replicates_every_voxel():
    c = cases.BY_NAME["twice as fine"]
    L = cases.values(cases.SRC, 0.5)
    got = synth.evid_sample_ref(L, cases.affine(c.name), c.dst.dims, "nearest")
    assert np.array_equal(got, L.repeat(2, axis=0).repeat(2, axis=1).repeat(2, axis=2))
    c = cases.BY_NAME["an eighth"]
    L = cases.values(cases.ONE, 0.5)
    got = synth.evid_sample_ref(L, cases.affine(c.name), c.dst.dims, "nearest")
    assert np.array_equal(got, L.repeat(8, axis=0).repeat(8, axis=1).repeat(8, axis=2)[:19, :9, :6])


# ------------------------------------------------------------------------------------------------------- the cover property

def _touched(case, margin=2):
    """For every dst voxel, in f64 from the geometry alone: the source voxels whose cube its cube intersects in more than a face ->
    (cand (N, K, 3) int64 source voxels around the centre, hit (N, K) bool).  The separating-axis test between the unit cube of the
    source voxel and the dst voxel's cube seen in source voxels (centre c, half edges the columns of A / 2): 3 + 3 + 9 axes."""
    R = cases.rotation(case.quat)
    A = (case.dst.resolution / case.src.resolution) * R.T
    d = np.stack(np.meshgrid(*(np.arange(n) for n in case.dst.dims), indexing="ij"), axis=-1).reshape(-1, 3)
    c = cases.source_position(case, d)                                            # (N, 3)
    offs = np.stack(np.meshgrid(*(np.arange(-margin, margin + 1),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    cand = np.floor(c).astype(np.int64)[:, None, :] + offs[None, :, :]            # (N, K, 3)
    t = c[:, None, :] - (cand + 0.5)                                              # centre to centre
    h = 0.5 * A                                                                   # half edges of the dst cube: columns
    axes = [np.eye(3)[j] for j in range(3)] + [A[:, i] / np.linalg.norm(A[:, i]) for i in range(3)]
    axes += [np.cross(np.eye(3)[j], A[:, i]) for j in range(3) for i in range(3)]
    hit = np.ones(t.shape[:2], dtype=bool)
    for L in axes:
        if np.linalg.norm(L) < 1e-12:
            continue
        reach = np.abs(L @ h).sum() + 0.5 * np.abs(L).sum()
        hit &= np.abs(t @ L) < reach - 1e-9
    return d, cand, hit


COVER_CASES = [c for c in cases.CASES if not c.name.startswith("axis rotation")] + [c for c in cases.CASES if c.name.startswith("axis rotation")][::5]


@pytest.mark.parametrize("case", COVER_CASES, ids=[c.name for c in COVER_CASES])
def test_cover_loses_no_occupied_voxel_and_frees_nothing_it_should_not(case):
    thr = cases.PARAMS["threshold"]
    sd, dd = case.src.dims, case.dst.dims
    R = cases.rotation(case.quat)
    d, cand, hit = _touched(case)
    cand_in = np.all((cand >= 0) & (cand < np.asarray(sd)), axis=2)
    cc = np.clip(cand, 0, np.asarray(sd) - 1)
    assert hit.any(axis=1).all()                                                  # (every dst cube touches something: the test sees)
    edge = np.abs(cand - np.floor(cases.source_position(case, d)).astype(np.int64)[:, None, :]).max(axis=2) == 2
    assert not (hit & edge).any()                                                 # ... and nothing beyond the candidates' rim
    for fill in cases.FILLS:
        L = cases.values(sd, fill)
        S = synth.evid_sample_ref(L, cases.affine(case.name), dd, "cover", thr)
        occ_b, fre_b = L > thr, (L != synth.EVID_UNKNOWN) & (L <= thr)
        O = synth.occ_resample_ref(occ_b, np.zeros(dd, bool), cases.affine(case.name), "any", "copy")[0]
        Fr = synth.occ_resample_ref(fre_b, np.zeros(dd, bool), cases.affine(case.name), "all", "copy")[0]
        assert not (O & Fr).any()                                                 # the two planes stay disjoint
        assert np.array_equal(O, S > thr) and np.array_equal(Fr, (S != synth.EVID_UNKNOWN) & (S <= thr))   # ... and are the values' own
        # no occupied source voxel is lost: its centre, taken to dst in f64, lies in an occupied dst voxel (or outside the box)
        ijk = np.argwhere(occ_b)
        w = (np.asarray(case.src.origin) + (ijk + 0.5) * case.src.resolution) @ R.T + np.asarray(case.pose)
        at = np.floor((w - np.asarray(case.dst.origin)) / case.dst.resolution).astype(np.int64)
        held = np.all((at >= 0) & (at < np.asarray(dd)), axis=1)
        assert (S[tuple(at[held].T)] > thr).all(), fill
        # no dst voxel is free unless every source voxel its cube intersects is free (inside the box, known, at most the threshold)
        free_src = np.where(cand_in, fre_b[cc[..., 0], cc[..., 1], cc[..., 2]], False)
        all_free = np.where(hit, free_src, True).all(axis=1).reshape(dd)
        is_free = (S != synth.EVID_UNKNOWN) & (S <= thr)
        assert not (is_free & ~all_free).any(), fill


def test_nearest_can_open_a_pinhole_and_cover_cannot():
    """What the documentation says of NEAREST, shown once: a wall one voxel thick, turned, has gaps under 'nearest' for some angle;
    under 'any' every dst voxel whose cube meets the wall is set (the property above).  Nothing is asserted of NEAREST beyond that a
    set dst bit had a set source bit under its centre."""
    c = cases.BY_NAME["yaw 30"]
    wall = np.zeros(cases.SRC, bool)
    wall[6, :, :] = True
    aff = cases.affine(c.name)
    near = synth.occ_resample_ref(wall, np.zeros(c.dst.dims, bool), aff, "nearest", "copy")[0]
    cover = synth.occ_resample_ref(wall, np.zeros(c.dst.dims, bool), aff, "any", "copy")[0]
    assert (cover | ~near).all() and cover.sum() > near.sum() > 0


# ------------------------------------------------------------------------------------------------------- the host layer

def _stand_ins(monkeypatch=None, calls=None):
    """Maps that carry a geometry and no device memory; with monkeypatch, the map layer's two call helpers record the entry's name."""
    torch = pytest.importorskip("torch")
    from trajectory_optimization_amd import ops

    class Grid(ops.OccupancyGrid):
        def __init__(self, origin=(0.0, 0.0, 0.0), r=0.125, dims=(8, 8, 8), device=0):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, r, dims)
            self.device = torch.device("cuda", device)

        def _sizes(self):
            return None, 0, None

        def reframed(self, shift=None, dims=None, centre=None):
            s, d, o = ops.check_reframe(self, shift, dims, centre)
            calls.append(("reframed", s, d))
            return Grid(o, self.resolution, d)

    class Evid(ops.EvidenceMap):
        def __init__(self, origin=(0.0, 0.0, 0.0), r=0.125, dims=(8, 8, 8)):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, r, dims)
            self.device = torch.device("cuda", 0)

    if monkeypatch is not None:
        monkeypatch.setattr(ops, "_map_call", lambda device, name, *a: calls.append(name))
        monkeypatch.setattr(ops, "_map_call0", lambda device, name, *a: calls.append(name))
    return ops, Grid, Evid


def test_default_box_and_like():
    ops, Grid, Evid = _stand_ins()
    g = Grid((1.0, -2.0, 0.5), dims=(20, 11, 9))
    zero = (0.0, 0.0, 0.0)
    # identity: the box itself
    frame, aff = ops.check_transform(g, zero, cases.IDENTITY)
    assert frame.origin.dtype == np.float32 and frame.origin.tolist() == [1.0, -2.0, 0.5] and frame.dims == (20, 11, 9) and frame.resolution == g.resolution
    assert np.array_equal(aff, ops.resample_affine(g, g, zero, cases.IDENTITY))
    # a fractional shift: the origin is snapped DOWN to a multiple of the resolution and the box grows by a voxel
    frame, _ = ops.check_transform(g, (0.05, 0.0, -0.01), cases.IDENTITY)
    assert frame.origin.tolist() == [1.0, -2.0, 0.375] and frame.dims == (21, 11, 10)
    # a quarter turn about z: (x, y) -> (-y, x)
    frame, _ = ops.check_transform(g, zero, cases.QUARTER_Z.quat)
    assert frame.origin.tolist() == [2.0 - 11 * 0.125, 1.0, 0.5] and frame.dims == (11, 20, 9)
    # yaw 30 about the world's origin: the box around the eight corners, in f64
    q = cases.rpy_quat(0.0, 0.0, math.radians(30.0))
    frame, _ = ops.check_transform(g, (0.3, 0.2, 0.0), q)
    lo, hi = np.array([1.0, -2.0, 0.5]), np.array([1.0 + 2.5, -2.0 + 11 * 0.125, 0.5 + 9 * 0.125])
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]) @ cases.rotation(q).T + (0.3, 0.2, 0.0)
    o = frame.origin.astype(np.float64)
    assert np.array_equal(o / 0.125, np.rint(o / 0.125))                                   # on the lattice through 0
    assert (o <= corners.min(axis=0) + 1e-9).all() and (o > corners.min(axis=0) - 0.125 - 1e-9).all()
    far = o + 0.125 * np.asarray(frame.dims)
    assert (far >= corners.max(axis=0) - 1e-9).all() and (far < corners.max(axis=0) + 0.125 + 1e-9).all()
    # a finer resolution: the same box in finer voxels
    frame, _ = ops.check_transform(g, zero, cases.IDENTITY, resolution=0.0625)
    assert frame.dims == (40, 22, 18) and frame.resolution == 0.0625
    # origin alone: dims reach the far corners; dims alone: from the default origin
    frame, _ = ops.check_transform(g, zero, cases.IDENTITY, origin=(0.5, -2.0, 0.5))
    assert frame.dims == (24, 11, 9)
    frame, _ = ops.check_transform(g, zero, cases.IDENTITY, dims=(5, 5, 5))
    assert frame.origin.tolist() == [1.0, -2.0, 0.5] and frame.dims == (5, 5, 5)
    # like= takes a map's frame, and nothing else with it
    other = Evid((0.25, 0.5, 0.75), dims=(7, 6, 5))
    frame, aff = ops.check_transform(g, (0.1, 0.0, 0.0), q, like=other)
    assert frame.origin.tolist() == [0.25, 0.5, 0.75] and frame.dims == (7, 6, 5) and frame.resolution == other.resolution
    assert np.array_equal(aff, ops.resample_affine(g, other, (0.1, 0.0, 0.0), q))
    refused = [(dict(like=other, dims=(5, 5, 5)), "like= brings origin, resolution and dims"), (dict(rule="any"), "rule must be 'nearest' or 'cover'"),
               (dict(resolution=0.25), "coarser"), (dict(resolution=0.125 / 2048), "exceeds 2048 per axis"), (dict(dims=(0, 1, 1)), "dims")]
    for kw, text in refused:
        with pytest.raises(ValueError, match=text):
            ops.check_transform(g, zero, cases.IDENTITY, **kw)
    with pytest.raises(ValueError, match="map must be an ops.OccupancyGrid, SpaceMap or EvidenceMap"):
        ops.check_transform(cases.Frame(zero, 0.125, (4, 4, 4)), zero, cases.IDENTITY)


def test_merge_maps_routes_and_takes_the_union_over_the_transformed_boxes(monkeypatch):
    calls = []
    ops, Grid, Evid = _stand_ins(monkeypatch, calls)
    from trajectory_optimization_amd import tools
    a, b = Grid((1.0, -2.0, 0.5), dims=(20, 11, 9)), Grid((1.375, -2.5, 0.5), dims=(8, 8, 8))
    zero, q30 = (0.0, 0.0, 0.0), cases.rpy_quat(0.0, 0.0, math.radians(30.0))
    # without poses: today's route, no resample entry
    tools.merge_maps([a, b])
    assert calls == [("reframed", (0, -4, 0), (20, 15, 9)), "tohip_occ_transfer"]
    # an identity pose on the lattice: the same route, the same box
    calls.clear()
    tools.merge_maps([a, b], poses=[zero, zero], quats=[cases.IDENTITY, (2.0, 0.0, 0.0, 0.0)])
    assert calls == [("reframed", (0, -4, 0), (20, 15, 9)), "tohip_occ_transfer"]
    # an identity pose off the lattice, and a turned map: resampled
    calls.clear()
    out = tools.merge_maps([a, Grid((1.03, -2.0, 0.5), dims=(20, 11, 9))], poses=[zero, zero], quats=[cases.IDENTITY, cases.IDENTITY])
    assert calls == [("reframed", (0, 0, 0), (21, 11, 9)), "tohip_occ_resample"] and out.dims == (21, 11, 9)
    calls.clear()
    pose = (0.3, 0.2, 0.0)
    out = tools.merge_maps([a, b], poses=[zero, pose], quats=[cases.IDENTITY, q30])
    k, n = ops.transformed_box(b, pose, q30, a.resolution, anchor=a.origin)
    lo = tuple(min(0, v) for v in k)
    hi = tuple(max(d, v + m) for d, v, m in zip(a.dims, k, n))
    assert calls == [("reframed", lo, tuple(h - l for l, h in zip(lo, hi))), "tohip_occ_resample"]
    # the union holds b's transformed corners
    corners = np.array([[x, y, z] for x in (1.375, 2.375) for y in (-2.5, -1.5) for z in (0.5, 1.5)]) @ cases.rotation(q30).T + pose
    o = out.origin.astype(np.float64)
    assert (o <= corners.min(axis=0) + 1e-9).all() and (o + 0.125 * np.asarray(out.dims) >= corners.max(axis=0) - 1e-9).all()
    assert np.array_equal((o - a.origin) / 0.125, np.rint((o - a.origin) / 0.125))             # on map 0's lattice
    # evidence maps: the same routing through their own entries
    e, f = Evid((1.0, -2.0, 0.5)), Evid((1.5, -2.0, 0.5))
    monkeypatch.setattr(Evid, "reframed", lambda self, shift=None, dims=None, centre=None: Evid(ops.check_reframe(self, shift, dims, centre)[2], dims=dims), raising=False)
    monkeypatch.setattr(Evid, "params", (17, 8, -40, 70, 0), raising=False)
    monkeypatch.setattr(Evid, "_sizes", lambda self: (None, 0, None))
    for name in ("occupied", "free"):
        monkeypatch.setattr(Evid, name, type("P", (), {"buf": torch_empty()}), raising=False)
    monkeypatch.setattr(Evid, "_counts", torch_empty(), raising=False)
    calls.clear()
    tools.merge_maps([e, f])
    tools.merge_maps([e, f], mode="add", poses=[zero, pose], quats=[cases.IDENTITY, q30], rule="cover")
    assert calls == ["tohip_evid_transfer", "tohip_evid_resample"]
    refused = [(dict(poses=[zero, zero]), "poses and quats must be given together"),
               (dict(poses=[zero], quats=[cases.IDENTITY]), "2 maps need as many poses and quats"),
               (dict(poses=[pose, zero], quats=[cases.IDENTITY, cases.IDENTITY]), "row 0 must be the identity"),
               (dict(poses=[zero, zero], quats=[cases.IDENTITY, q30], rule="any"), "rule must be 'nearest' or 'cover'")]
    for kw, text in refused:
        with pytest.raises(ValueError, match=text):
            tools.merge_maps([a, b], **kw)
    with pytest.raises(ValueError, match="coarser"):
        tools.merge_maps([a, Grid(r=0.0625)], poses=[zero, pose], quats=[cases.IDENTITY, q30])   # map 0 would have to coarsen the finer map
    with pytest.raises(ValueError, match="exceeds 2048 per axis"):
        tools.merge_maps([a, b], poses=[zero, (300.0, 0.0, 0.0)], quats=[cases.IDENTITY, q30])


def torch_empty():
    import torch
    return torch.zeros(4, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------------- the C entries

def test_entries_refuse_bad_arguments_without_gpu():
    """Every argument check returns before anything is enqueued: bad calls come back with their code on a machine without a GPU."""
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    EINVAL, ENOSPC = _lib.CONSTANTS["TOHIP_EINVAL"], _lib.CONSTANTS["TOHIP_ENOSPC"]
    p, q, r, t, u, v = (ctypes.c_void_p(a) for a in (4096, 8192, 16384, 32768, 65536, 131072))   # 16-byte aligned pointers no call may reach
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(13, 10, 7): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))   # noqa: E731
    gs, gd = geom(), geom(d=(5, 6, 3))
    sb, db = L.tohip_occ_bytes(13, 10, 7), L.tohip_occ_bytes(5, 6, 3)
    se, de = L.tohip_evid_bytes(13, 10, 7), L.tohip_evid_bytes(5, 6, 3)
    aff = lambda a=cases.affine("yaw 30"): (ctypes.c_int64 * 12)(*[int(x) for x in a])   # noqa: E731
    calls = {
        "occ": (L.tohip_occ_resample, ("src", "src_bytes", "src_geom", "dst", "dst_bytes", "dst_geom", "affine", "frac_bits", "rule", "mode", "counts",
                                       "stream", "flags"), (p, sb, gs, q, db, gd, aff(), 20, 0, 0, None, None, 0)),
        "evid": (L.tohip_evid_resample, ("src", "src_bytes", "src_geom", "dst", "dst_bytes", "dst_geom", "occ", "free", "grid_bytes", "affine",
                                         "frac_bits", "rule", "mode", "lmin", "lmax", "threshold", "counts", "scratch", "scratch_bytes", "stream", "flags"),
                 (p, se, gs, q, de, gd, r, t, db, aff(), 20, 0, 0, -40, 70, 0, None, None, 0, None, 0)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    def with_entry(i, value):
        a = [int(x) for x in cases.affine("yaw 30")]
        a[i] = value
        return (ctypes.c_int64 * 12)(*a)

    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 6, 3)), geom(d=(5, 2049, 3))]
    for name in calls:
        for g in bad_geoms:
            assert call(name, src_geom=g) == EINVAL and call(name, dst_geom=g) == EINVAL, name
        bad = [dict(src=None), dict(dst=None), dict(src_geom=None), dict(dst_geom=None), dict(dst=p), dict(counts=p), dict(counts=q),
               dict(affine=None), dict(frac_bits=19), dict(frac_bits=21), dict(frac_bits=0), dict(rule=-1), dict(rule=3), dict(mode=-1), dict(flags=1),
               dict(affine=with_entry(0, (1 << 21) + 1)), dict(affine=with_entry(8, -(1 << 21) - 1)), dict(affine=with_entry(9, (1 << 40) + 1)),
               dict(affine=with_entry(11, -(1 << 40) - 1))]
        for kw in bad:
            assert call(name, **kw) == EINVAL, (name, kw)
        assert call(name, src_bytes=(sb if name == "occ" else se) - 1) == ENOSPC and call(name, dst_bytes=(db if name == "occ" else de) - 1) == ENOSPC
    assert call("occ", mode=2) == EINVAL and call("evid", mode=3) == EINVAL and call("evid", rule=2) == EINVAL
    for kw in (dict(occ=None), dict(free=None), dict(free=r), dict(occ=q), dict(free=p), dict(counts=r), dict(counts=t), dict(scratch=p), dict(scratch=q),
               dict(scratch=r), dict(scratch=t), dict(counts=u, scratch=u), dict(src=ctypes.c_void_p(4100)), dict(dst=ctypes.c_void_p(8200)),
               dict(lmin=-128), dict(lmax=128), dict(lmin=1), dict(threshold=70), dict(lmin=5, threshold=4)):
        assert call("evid", **kw) == EINVAL, kw
    assert call("evid", grid_bytes=db - 1) == ENOSPC
