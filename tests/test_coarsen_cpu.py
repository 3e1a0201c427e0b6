"""Coarsening maps without a GPU ("Coarsening maps"): the numpy restatements (synth.evid_coarsen_ref /
occ_coarsen_ref) against a per-voxel loop in Python integers; exact composition of factors; the pyramid; the conservativeness of
COVER checked from the definition, independently of the rule's key; ops.coarsen_offset / check_coarsen / check_merge_fine, their
default boxes and refusals; the C entries' refusals; and that the resampling calls still refuse a coarser destination."""
import ctypes
import itertools

import numpy as np
import pytest

import abi_cases
import coarsen_cases as cases
from trajectory_optimization_amd import synth

ENTRIES = ("tohip_occ_coarsen", "tohip_evid_coarsen")
U = synth.EVID_UNKNOWN


def test_abi_entries():
    from trajectory_optimization_amd import _lib, ops
    header, before = abi_cases.check_abi_entries(ENTRIES)
    assert "coarsen_kernels.hip" in header and "Coarsening maps" in header and "new symbols only" in before
    C = _lib.CONSTANTS
    assert C["TOHIP_COARSEN_MAX_FACTOR"] == 8 == synth.COARSEN_MAX_FACTOR == ops.COARSEN_MAX_FACTOR
    assert (C["TOHIP_COARSEN_COVER"], C["TOHIP_COARSEN_MAX"]) == tuple(ops.COARSEN_RULES[r] for r in cases.EVID_RULES)
    assert (C["TOHIP_COARSEN_ANY"], C["TOHIP_COARSEN_ALL"]) == tuple(ops.COARSEN_OCC_RULES[r] for r in cases.OCC_RULES)
    assert [len(_lib.SIGNATURES[s][1]) for s in ENTRIES] == [16, 21]
    # the reserved flags word behind the stream keeps the entries out of tests/test_hip_contracts.py's count
    assert _lib.SIGNATURES[ENTRIES[0]][1][-2:] == _lib.SIGNATURES[ENTRIES[1]][1][-2:] == [ctypes.c_void_p, ctypes.c_int32]


# ------------------------------------------------------------------------------------------------------- the restatements

@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_restatements_equal_a_per_voxel_loop(case):
    f, o = case.factor, case.offset
    for fill in cases.FILLS:
        sb, vb, db, L_src, L_dst = cases.inputs(case, fill)
        before = [a.copy() for a in (sb, vb, db, L_src, L_dst)]
        want = cases.coarsen_loop(sb, vb, db, L_src, L_dst, f, o)
        for rule in (*cases.OCC_RULES, "veto"):
            for mode in cases.OCC_MODES:
                new, count = synth.occ_coarsen_ref(sb, db, f, o, "any" if rule == "veto" else rule, mode, veto=vb if rule == "veto" else None)
                assert new.dtype == bool and np.array_equal(new, want["plane", rule, mode][0]) and count == want["plane", rule, mode][1], (fill, rule, mode)
        for rule in cases.EVID_RULES:
            for mode in cases.EVID_MODES:
                new, counts = synth.evid_coarsen_ref(L_src, L_dst, f, o, rule, mode, cases.PARAMS)
                assert np.array_equal(new, want["evid", rule, mode][0]) and np.array_equal(counts, want["evid", rule, mode][1]), (fill, rule, mode)
        for a, b in zip(before, (sb, vb, db, L_src, L_dst)):
            assert np.array_equal(a, b)   # the inputs are not modified


def test_the_cases_reach_what_they_are_for():
    p = cases.PARAMS
    assert {U, p["lmin"], p["threshold"], p["threshold"] + 1, p["lmax"]} <= set(cases.values(cases.SRC, 0.5).reshape(-1).tolist())
    for c in cases.CASES:
        inside = synth.coarsen_children(np.ones(c.src.dims, bool), c.dst.dims, c.factor, c.offset, False)
        if "wholly outside" in c.name:
            assert not inside.any(), c.name
        else:
            assert inside.any(), c.name
        if "bigger" in c.name:
            assert not inside.any(axis=-1).all(), c.name                      # dst voxels beyond the source's image
        if "odd" in c.name:
            assert (inside.any(axis=-1) & ~inside.all(axis=-1)).any(), c.name   # voxels with children on both sides of the source's edge
        if "brick-aligned" in c.name:
            assert c.offset[0] % 4 == 0 and c.offset[1] % 4 == 0 and c.offset[2] % 2 == 0
    assert {c.factor for c in cases.CASES} == set(cases.FACTORS)


def test_restatements_refuse_unknown_rules_modes_and_factors():
    z = np.zeros((2, 2, 2))
    for bad in (dict(rule="nearest", mode="copy"), dict(rule="cover", mode="or")):
        with pytest.raises(ValueError):
            synth.evid_coarsen_ref(z, z, 2, (0, 0, 0), **bad)
    for bad in (dict(rule="cover", mode="copy"), dict(rule="any", mode="add"), dict(rule="all", mode="copy", veto=z)):
        with pytest.raises(ValueError):
            synth.occ_coarsen_ref(z, z, 2, (0, 0, 0), **bad)
    for f, o in ((1, (0, 0, 0)), (9, (0, 0, 0)), (2, (0, (1 << 20) + 1, 0))):
        with pytest.raises(ValueError):
            synth.coarsen_children(z, (1, 1, 1), f, o, 0)


# ------------------------------------------------------------------------------------------------------- composition

@pytest.mark.parametrize("f1,f2", [(2, 2), (2, 4), (4, 2), (2, 3)])
def test_composition_is_exact(f1, f2):
    """Factor f1 then f2 equals factor f1 f2 once, bit for bit, where the composed offset is o1 + f1 o2 and the intermediate box holds
    every child: both key orders are total, so the maximum is associative."""
    src = cases.SRC
    for o1, o2, fill in itertools.product(((0, 0, 0), (-1, -3, -1), (4, -8, 2)), ((0, 0, 0), (-1, 2, -1)), cases.FILLS):
        o = tuple(a + f1 * b for a, b in zip(o1, o2))
        dims = cases.ceil_dims(src, o, f1 * f2)
        mid = tuple(f2 * n + max(b, 0) - min(b, 0) for n, b in zip(dims, o2))           # every child f2 d + o2 + e of the final box ...
        lo2 = tuple(min(b, 0) for b in o2)
        mid_o1 = tuple(a + f1 * l for a, l in zip(o1, lo2))                            # ... in an intermediate box that starts at min(o2, 0)
        mid_o2 = tuple(b - l for b, l in zip(o2, lo2))
        L, b = cases.values(src, fill), cases.bits(src, fill)
        for rule in cases.EVID_RULES:
            once = synth.evid_coarsen_sample_ref(L, dims, f1 * f2, o, rule)
            twice = synth.evid_coarsen_sample_ref(synth.evid_coarsen_sample_ref(L, mid, f1, mid_o1, rule), dims, f2, mid_o2, rule)
            assert np.array_equal(once, twice), (o1, o2, fill, rule)
        empty = np.zeros(dims, bool)
        for rule in cases.OCC_RULES:
            once = synth.occ_coarsen_ref(b, empty, f1 * f2, o, rule, "copy")[0]
            twice = synth.occ_coarsen_ref(synth.occ_coarsen_ref(b, np.zeros(mid, bool), f1, mid_o1, rule, "copy")[0], empty, f2, mid_o2, rule, "copy")[0]
            assert np.array_equal(once, twice), (o1, o2, fill, rule)


def test_two_then_four_is_eight():
    L = cases.values(cases.SRC, 0.5)
    for rule in cases.EVID_RULES:
        d8 = cases.ceil_dims(cases.SRC, (0, 0, 0), 8)
        d2 = tuple(4 * n for n in d8)                                                  # holds every child of the final box
        a = synth.evid_coarsen_sample_ref(synth.evid_coarsen_sample_ref(L, d2, 2, (0, 0, 0), rule), d8, 4, (0, 0, 0), rule)
        assert np.array_equal(a, synth.evid_coarsen_sample_ref(L, d8, 8, (0, 0, 0), rule))


# ------------------------------------------------------------------------------------------------------- conservativeness

@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_cover_is_conservative_from_the_definition(case):
    """Not through the key: an occupied source voxel whose parent lies in dst has an occupied parent; a free dst voxel has all its
    f^3 children inside the source and free; the planes of the coarse values are the coarse planes (ANY of occupied, ALL of free); a
    SpaceMap's planes stay disjoint under both rules."""
    f, o, thr = case.factor, case.offset, cases.PARAMS["threshold"]
    for fill in cases.FILLS:
        L = cases.values(case.src.dims, fill)
        S = synth.evid_coarsen_sample_ref(L, case.dst.dims, f, o, "cover", thr)
        for x, y, z in np.argwhere(L > thr):
            d = ((x - o[0]) // f, (y - o[1]) // f, (z - o[2]) // f)
            if all(0 <= d[a] < case.dst.dims[a] for a in range(3)):
                assert S[d] > thr and S[d] >= L[x, y, z]
        for d in np.argwhere((S != U) & (S <= thr)):
            for c in cases.children(tuple(int(v) for v in d), f, o):
                assert all(0 <= c[a] < case.src.dims[a] for a in range(3)) and L[c] != U and L[c] <= thr and L[c] <= S[tuple(d)]
        occ, free = synth.evidence_planes_ref(L, thr)
        empty = np.zeros(case.dst.dims, bool)
        c_occ, c_free = synth.evidence_planes_ref(S, thr)
        assert np.array_equal(c_occ, synth.occ_coarsen_ref(occ, empty, f, o, "any", "copy")[0])
        assert np.array_equal(c_free, synth.occ_coarsen_ref(free, empty, f, o, "all", "copy")[0])
        assert not (c_occ & c_free).any()
        # MAX: the planes of its values are ANY of occupied, and ANY of free vetoed by occupied
        m_occ, m_free = synth.evidence_planes_ref(synth.evid_coarsen_sample_ref(L, case.dst.dims, f, o, "max", thr), thr)
        assert np.array_equal(m_occ, c_occ)
        assert np.array_equal(m_free, synth.occ_coarsen_ref(free, empty, f, o, "any", "copy", veto=occ)[0])
        assert not (m_occ & m_free).any() and (m_free | ~c_free).all()


# ------------------------------------------------------------------------------------------------------- the host layer

def _stand_ins(monkeypatch=None, calls=None):
    """Maps that carry a geometry and no device memory; with monkeypatch, the map layer's call helper records what it is handed."""
    torch = pytest.importorskip("torch")
    from trajectory_optimization_amd import ops

    class Grid(ops.OccupancyGrid):
        def __init__(self, origin=(0.0, 0.0, 0.0), r=0.125, dims=(8, 8, 8), device=0):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, r, dims)
            self.device = torch.device("cuda", device)

    class Evid(ops.EvidenceMap):
        def __init__(self, origin=(0.0, 0.0, 0.0), r=0.125, dims=(8, 8, 8), device=0):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, r, dims)
            self.device = torch.device("cuda", device)

    return ops, Grid, Evid


def test_coarsen_offset_and_its_refusals():
    ops, Grid, _ = _stand_ins()
    F = ops.MapFrame
    g = Grid((1.0, -2.0, 0.5), dims=(20, 11, 9))
    assert ops.coarsen_offset(g, F((1.0, -2.0, 0.5), 0.25, (10, 6, 5)), 2) == (0, 0, 0)
    assert ops.coarsen_offset(g, F((0.875, -2.375, 0.625), 0.375, (3, 3, 3)), 3) == (-1, -3, 1)
    assert ops.coarsen_offset(g, F((1.0 + 0.125 / 300, -2.0, 0.5), 1.0, (3, 3, 3)), 8) == (0, 0, 0)      # within 1/256 voxel
    for c in cases.CASES:
        assert ops.coarsen_offset(c.src, c.dst, c.factor) == c.offset, c.name
    for factor in (1, 9, 0, -2, 2.0, True, None):
        with pytest.raises(ValueError, match=r"factor must be an integer in \[2, 8\]"):
            ops.coarsen_offset(g, F((1.0, -2.0, 0.5), 0.25, (1, 1, 1)), factor)
    with pytest.raises(ValueError, match="is not 2 times the fine one"):
        ops.coarsen_offset(g, F((1.0, -2.0, 0.5), 0.375, (1, 1, 1)), 2)
    with pytest.raises(ValueError, match="is not 3 times the fine one"):
        ops.coarsen_offset(g, F((1.0, -2.0, 0.5), 0.375 * (1 + 1e-5), (1, 1, 1)), 3)
    with pytest.raises(ValueError, match="not on the fine lattice: along y"):
        ops.coarsen_offset(g, F((1.0, -2.05, 0.5), 0.25, (1, 1, 1)), 2)
    with pytest.raises(ValueError, match="beyond 2\\^20"):
        ops.coarsen_offset(g, F((1.0 + 0.125 * ((1 << 20) + 8), -2.0, 0.5), 0.25, (1, 1, 1)), 2)


def test_check_coarsen_boxes_anchors_like_and_refusals():
    ops, Grid, Evid = _stand_ins()
    g = Grid((1.0, -2.0, 0.5), dims=(20, 11, 9))
    # anchor 'origin': o = 0, dims = ceil(n / f)
    for f, dims in ((2, (10, 6, 5)), (3, (7, 4, 3)), (8, (3, 2, 2))):
        frame, o, rule = ops.check_coarsen(g, f)
        assert o == (0, 0, 0) and frame.dims == dims and frame.origin.tolist() == [1.0, -2.0, 0.5] and rule == "any"
        assert frame.origin.dtype == np.float32 and frame.resolution == float(np.float32(f * 0.125))
    # anchor 'world': the coarse planes at multiples of f r.  The origin sits at (8, -16, 4) voxels: for f = 3, 8 mod 3 = 2, -16 mod 3 = 2, 4 mod 3 = 1
    frame, o, _ = ops.check_coarsen(g, 3, anchor="world")
    assert o == (-2, -2, -1) and frame.origin.tolist() == [0.75, -2.25, 0.375] and frame.dims == (8, 5, 4)
    assert np.array_equal(frame.origin / 0.375, np.rint(frame.origin / 0.375))
    frame, o, _ = ops.check_coarsen(g, 4, anchor="world")
    assert o == (0, 0, 0) and frame.dims == (5, 3, 3)
    # two sources on one fine lattice share the coarse lattice under 'world'
    h = Grid((1.0 + 5 * 0.125, -2.0 - 7 * 0.125, 0.5 + 0.125), dims=(9, 9, 9))
    fa, fb = ops.check_coarsen(g, 3, anchor="world")[0], ops.check_coarsen(h, 3, anchor="world")[0]
    assert ops.lattice_offset(Grid(*fa), Grid(*fb)) == (2, -2, 0)
    with pytest.raises(ValueError, match="anchor='world' needs the map's origin"):
        ops.check_coarsen(Grid((1.03, 0.0, 0.0)), 2, anchor="world")
    # origin= / dims= / like=
    frame, o, _ = ops.check_coarsen(g, 2, origin=(0.875, -2.375, 0.5))
    assert o == (-1, -3, 0) and frame.dims == (11, 7, 5)
    frame, o, _ = ops.check_coarsen(g, 2, dims=(4, 4, 4))
    assert o == (0, 0, 0) and frame.dims == (4, 4, 4)
    other = Evid((0.75, -2.0, 0.25), r=0.5, dims=(7, 6, 5))
    frame, o, rule = ops.check_coarsen(Evid((1.0, -2.0, 0.5), dims=(20, 11, 9)), 4, rule="max", like=other)
    assert o == (-2, 0, -2) and frame.dims == (7, 6, 5) and frame.origin.tolist() == [0.75, -2.0, 0.25] and frame.resolution == 0.5 and rule == "max"
    assert ops.check_coarsen(Evid(), 2)[2] == "cover"
    refused = [(dict(factor=1), "factor must be an integer"), (dict(factor=9), "factor must be an integer"), (dict(rule="cover"), "rule must be 'any' or 'all'"),
               (dict(anchor="map"), "anchor must be 'origin' or 'world'"), (dict(like=other, dims=(5, 5, 5)), "like= brings origin and dims"),
               (dict(like=other), "is not 2 times the fine one"), (dict(origin=(1.05, -2.0, 0.5)), "not on the fine lattice: along x"),
               (dict(origin=(1.0, float("nan"), 0.5)), "origin must be three finite numbers"), (dict(dims=(0, 1, 1)), "dims"),
               (dict(dims=(2049, 1, 1)), "dims")]
    for kw, text in refused:
        with pytest.raises(ValueError, match=text):
            ops.check_coarsen(g, **{"factor": 2, **kw})
    with pytest.raises(ValueError, match="rule must be 'cover' or 'max'"):
        ops.check_coarsen(Evid(), 2, rule="any")
    with pytest.raises(ValueError, match="map must be an ops.OccupancyGrid, SpaceMap or EvidenceMap"):
        ops.check_coarsen(ops.MapFrame((0.0, 0.0, 0.0), 0.125, (4, 4, 4)), 2)
    # a box over the limits: the default dims from an origin far below the map
    with pytest.raises(ValueError, match="exceeds 2048 per axis"):
        ops.check_coarsen(g, 2, origin=(1.0 - 0.125 * 8200, -2.0, 0.5))


def test_check_merge_fine():
    ops, Grid, Evid = _stand_ins()
    coarse, fine = Grid((0.75, -2.25, 0.375), r=0.375, dims=(8, 5, 4)), Grid((1.0, -2.0, 0.5), dims=(20, 11, 9))
    assert ops.check_merge_fine(coarse, fine) == (3, (-2, -2, -1), "any")
    assert ops.check_merge_fine(Evid((1.0, 0.0, 0.0), r=1.0), Evid((1.0, 0.0, 0.0)), "add", "max") == (8, (0, 0, 0), "max")
    refused = [((coarse, coarse), {}, "cannot be merged into itself"), ((coarse, Evid()), {}, "merges with its own kind"),
               ((coarse, fine), dict(mode="add"), "mode applies to evidence maps only"), ((coarse, Grid(r=0.375)), {}, "2 to 8 times finer"),
               ((Grid(r=2.0), fine), {}, "2 to 8 times finer"), ((Grid(r=0.3), fine), {}, "is not 2 times the fine one"),
               ((Grid((0.8, 0.0, 0.0), r=0.375), fine), {}, "not on the fine lattice"), ((Grid(r=0.25, device=1), fine), {}, "one device"),
               ((Evid(r=0.25), Evid()), {}, "mode must be 'confident' or 'add'"), ((coarse, fine), dict(rule="max"), "rule must be 'any' or 'all'")]
    for (a, b), kw, text in refused:
        with pytest.raises(ValueError, match=text):
            ops.check_merge_fine(a, b, **kw)


def test_the_public_calls_hand_the_entries_what_check_coarsen_says(monkeypatch):
    calls = []
    ops, Grid, Evid = _stand_ins()
    from trajectory_optimization_amd import tools
    monkeypatch.setattr(ops, "_map_call0", lambda device, name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops.OccupancyGrid, "_sizes", lambda self: ("buf", 0, "geom"))
    monkeypatch.setattr(ops, "ptr", lambda t: t)
    made = []

    def init(self, origin, resolution, dims, device=None):   # the grid coarsened() makes: a geometry and no device memory
        self.origin, self.resolution, self.dims, _ = ops.check_los(origin, resolution, dims)
        self.device = device
        made.append(self)

    monkeypatch.setattr(ops.OccupancyGrid, "__init__", init)
    g = Grid((1.0, -2.0, 0.5), dims=(20, 11, 9))
    g.skipped = 3
    out = tools.coarsen_map(g, 3, anchor="world")
    assert out is made[-1] and out.dims == (8, 5, 4) and out.resolution == 0.375 and out.skipped == 3
    name, a = calls[-1]
    assert name == "tohip_occ_coarsen" and a[3] is None and a[7:] == (3, -2, -2, -1, 0, 0, None)
    levels = tools.map_pyramid(g, 3, rule="all")
    assert [m.dims for m in levels] == [(20, 11, 9), (10, 6, 5), (5, 3, 3), (3, 2, 2)] and levels[0] is g
    assert [m.resolution for m in levels] == [0.125, 0.25, 0.5, 1.0] and all(c[1][7:12] == (2, 0, 0, 0, 1) for c in calls[-3:])
    assert tools.map_pyramid(g, 0) == [g]
    with pytest.raises(ValueError, match="levels must be an integer >= 0"):
        tools.map_pyramid(g, -1)
    # merge_fine: the factor and the offset from the two frames, mode OR
    calls.clear()
    coarse = Grid((0.75, -2.25, 0.375), r=0.375, dims=(8, 5, 4))
    assert coarse.merge_fine(g) is coarse
    assert calls[-1][0] == "tohip_occ_coarsen" and calls[-1][1][7:] == (3, -2, -2, -1, 0, 1, None)


def test_pyramid_levels_equal_one_coarsening_in_the_restatement():
    """map_pyramid's level l is l factor-2 steps at offset 0 with dims ceil(n / 2) each: equal to one step of 2^l, since
    ceil(ceil(n / 2) / 2) = ceil(n / 4) and a child beyond the source is EMPTY in both."""
    for fill in cases.FILLS:
        L, b = cases.values(cases.SRC, fill), cases.bits(cases.SRC, fill)
        for rule in cases.EVID_RULES:
            level = L
            for l in (1, 2, 3):
                level = synth.evid_coarsen_sample_ref(level, cases.ceil_dims(level.shape, (0, 0, 0), 2), 2, (0, 0, 0), rule)
                assert np.array_equal(level, synth.evid_coarsen_sample_ref(L, cases.ceil_dims(cases.SRC, (0, 0, 0), 2 ** l), 2 ** l, (0, 0, 0), rule)), (rule, l)
        for rule in cases.OCC_RULES:
            level = b
            for l in (1, 2, 3):
                d = cases.ceil_dims(level.shape, (0, 0, 0), 2)
                level = synth.occ_coarsen_ref(level, np.zeros(d, bool), 2, (0, 0, 0), rule, "copy")[0]
                d = cases.ceil_dims(cases.SRC, (0, 0, 0), 2 ** l)
                assert np.array_equal(level, synth.occ_coarsen_ref(b, np.zeros(d, bool), 2 ** l, (0, 0, 0), rule, "copy")[0]), (rule, l)


def test_the_resampling_calls_still_refuse_a_coarser_destination():
    ops, Grid, _ = _stand_ins()
    from trajectory_optimization_amd import tools
    g = Grid((1.0, -2.0, 0.5), dims=(20, 11, 9))
    zero, ident = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="coarser than the source's.*coarsening is a reduction.*coarsen_map"):
        tools.transform_map(g, zero, ident, resolution=0.25)
    with pytest.raises(ValueError, match="coarser"):
        ops.resample_affine(g, ops.MapFrame((1.0, -2.0, 0.5), 0.25, (10, 6, 5)), zero, ident)
    with pytest.raises(ValueError, match="resolutions differ"):
        tools.merge_maps([Grid(r=0.25), g])
    with pytest.raises(ValueError, match="coarser"):
        Grid(r=0.25).merge(g, pose=(0.01, 0.0, 0.0), quat=ident)


# ------------------------------------------------------------------------------------------------------- the C entries

def test_entries_refuse_bad_arguments_without_gpu():
    """Every argument check returns before anything is enqueued: bad calls come back with their code on a machine without a GPU."""
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    EINVAL, ENOSPC = _lib.CONSTANTS["TOHIP_EINVAL"], _lib.CONSTANTS["TOHIP_ENOSPC"]
    p, q, r, t, u = (ctypes.c_void_p(a) for a in (4096, 8192, 16384, 32768, 65536))   # 16-byte aligned pointers no call may reach
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(13, 10, 7): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))   # noqa: E731
    gs, gd = geom(), geom(res=0.2, d=(5, 6, 3))
    sb, db = L.tohip_occ_bytes(13, 10, 7), L.tohip_occ_bytes(5, 6, 3)
    se, de = L.tohip_evid_bytes(13, 10, 7), L.tohip_evid_bytes(5, 6, 3)
    calls = {
        "occ": (L.tohip_occ_coarsen, ("src", "src_bytes", "src_geom", "veto", "dst", "dst_bytes", "dst_geom", "factor", "ox", "oy", "oz", "rule", "mode",
                                      "counts", "stream", "flags"), (p, sb, gs, None, q, db, gd, 2, 0, 0, 0, 0, 0, None, None, 0)),
        "evid": (L.tohip_evid_coarsen, ("src", "src_bytes", "src_geom", "dst", "dst_bytes", "dst_geom", "occ", "free", "grid_bytes", "factor", "ox", "oy",
                                        "oz", "rule", "mode", "lmin", "lmax", "threshold", "counts", "stream", "flags"),
                 (p, se, gs, q, de, gd, r, t, db, 2, 0, 0, 0, 0, 0, -40, 70, 0, None, None, 0)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 6, 3)), geom(d=(5, 2049, 3))]
    far = (1 << 20) + 1
    for name in calls:
        for g in bad_geoms:
            assert call(name, src_geom=g) == EINVAL and call(name, dst_geom=g) == EINVAL, name
        bad = [dict(src=None), dict(dst=None), dict(src_geom=None), dict(dst_geom=None), dict(dst=p), dict(counts=p), dict(counts=q),
               dict(factor=1), dict(factor=9), dict(factor=0), dict(factor=-2), dict(ox=far), dict(oy=-far), dict(oz=far), dict(rule=-1), dict(rule=2),
               dict(mode=-1), dict(flags=1), dict(flags=-1)]
        for kw in bad:
            assert call(name, **kw) == EINVAL, (name, kw)
        assert call(name, src_bytes=(sb if name == "occ" else se) - 1) == ENOSPC and call(name, dst_bytes=(db if name == "occ" else de) - 1) == ENOSPC
    assert call("occ", mode=2) == EINVAL and call("evid", mode=3) == EINVAL
    for kw in (dict(veto=p), dict(veto=q), dict(veto=u, counts=u), dict(veto=u, rule=1)):
        assert call("occ", **kw) == EINVAL, kw
    for kw in (dict(occ=None), dict(free=None), dict(free=r), dict(occ=q), dict(free=p), dict(counts=r), dict(counts=t), dict(src=ctypes.c_void_p(4100)),
               dict(dst=ctypes.c_void_p(8200)), dict(lmin=-128), dict(lmax=128), dict(lmin=1), dict(threshold=70), dict(lmin=5, threshold=4)):
        assert call("evid", **kw) == EINVAL, kw
    assert call("evid", grid_bytes=db - 1) == ENOSPC
