"""Re-framing and merging maps without a GPU ("Re-framing and merging maps"): the numpy restatements
(synth.occ_transfer_ref / evidence_transfer_ref) against a per-voxel loop, the algebra of the two merge modes, the lattice rule, the
argument checks by message, follow_map's decision at the margin's boundary voxel, the re-framed origin, and the C entries' refusals."""
import ctypes

import numpy as np
import pytest

import abi_cases
import reframe_cases as cases
from trajectory_optimization_amd import synth

ENTRIES = ("tohip_occ_transfer", "tohip_evid_transfer")
f32 = np.float32


def test_abi_entries():
    header, before = abi_cases.check_abi_entries(ENTRIES)
    assert "reframe_kernels.hip" in header and "re-framing and merging maps" in header and "new symbols only" in before


# ------------------------------------------------------------------------------------------------------- the restatements

@pytest.mark.parametrize("pair", cases.LOOP_PAIRS, ids=str)
def test_restatements_equal_a_per_voxel_loop(pair):
    sd, dd = pair
    bits, dst_bits = cases.plane_bits(sd, 0.3), cases.plane_bits(dd, 0.3, seed=1)
    L_src, L_dst = cases.evid_values(sd, "wide"), cases.evid_values(dd, "default", seed=1)   # (sources beyond the destination's clamps)
    assert (L_src > cases.DEFAULT["lmax"]).any() and (L_src < cases.DEFAULT["lmin"]).any()
    before = bits.copy(), dst_bits.copy(), L_src.copy(), L_dst.copy()
    for shift in cases.LOOP_SHIFTS:
        want = cases.transfer_loop(bits, dst_bits, L_src, L_dst, shift, cases.DEFAULT)
        for mode in ("copy", "or"):
            new, count = synth.occ_transfer_ref(bits, dst_bits, shift, mode)
            assert new.dtype == bool and np.array_equal(new, want["plane", mode][0]) and count == want["plane", mode][1], (shift, mode)
        for mode in ("copy", "add", "confident"):
            new, counts = synth.evidence_transfer_ref(L_src, L_dst, shift, mode, cases.DEFAULT)
            assert np.array_equal(new, want["evid", mode][0]) and np.array_equal(counts, want["evid", mode][1]), (shift, mode)
    for a, b in zip(before, (bits, dst_bits, L_src, L_dst)):
        assert np.array_equal(a, b)   # the inputs are not modified


def test_a_shift_without_overlap_copies_nothing():
    for sd, dd in cases.PAIRS:
        for shift in cases.NO_OVERLAP:
            bits, dst = cases.plane_bits(sd, 1.0), cases.plane_bits(dd, 0.3)
            assert not synth.occ_transfer_ref(bits, dst, shift, "copy")[0].any()
            new, count = synth.occ_transfer_ref(bits, dst, shift, "or")
            assert np.array_equal(new, dst) and count == 0
            L = cases.evid_values(dd, "default")
            for mode in ("add", "confident"):
                new, counts = synth.evidence_transfer_ref(cases.evid_values(sd, "default"), L, shift, mode)
                assert np.array_equal(new, L) and not counts.any()


def test_restatements_refuse_unknown_modes():
    with pytest.raises(ValueError, match="mode must be 'copy' or 'or'"):
        synth.occ_transfer_ref(np.zeros((2, 2, 2), bool), np.zeros((2, 2, 2), bool), (0, 0, 0), "add")
    with pytest.raises(ValueError, match="mode must be 'copy', 'add' or 'confident'"):
        synth.evidence_transfer_ref(np.zeros((2, 2, 2)), np.zeros((2, 2, 2)), (0, 0, 0), "or")


def test_confident_is_a_lattice_join_and_add_commutes():
    rng = np.random.default_rng(3)
    dims, zero = (6, 5, 4), (0, 0, 0)
    for params in (cases.DEFAULT, cases.WIDE):
        lo, hi = params["lmin"], params["lmax"]
        A, B, C = (np.where(rng.random(dims) < 0.3, -128, rng.integers(lo, hi + 1, dims)) for _ in range(3))
        A[0, 0, :4], B[0, 0, :4] = [5, -5, 0, -128], [-5, 5, -128, 0]   # the tie and the unknown, both ways round
        join = lambda S, D: synth.evidence_transfer_ref(S, D, zero, "confident", params)[0]   # noqa: E731
        add = lambda S, D: synth.evidence_transfer_ref(S, D, zero, "add", params)[0]           # noqa: E731
        assert np.array_equal(join(A, B), join(B, A))                                  # commutative
        assert np.array_equal(join(C, join(B, A)), join(join(C, B), A))                # associative
        assert np.array_equal(join(A, A), A) and np.array_equal(join(B, join(B, A)), join(B, A))   # idempotent
        assert join(A, B)[0, 0, :4].tolist() == [5, 5, 0, 0]                           # +k beats -k; anything beats never observed
        assert np.array_equal(add(A, B), add(B, A))                                    # commutative
        assert not np.array_equal(add(A, add(A, B)), add(A, B))                        # ... and a map merged twice counts twice
    # the join picks by (|L|, L): exhaustively over the value range
    v = np.concatenate([[-128], np.arange(-127, 128)])
    S, D = (a.reshape(-1, 1, 1) for a in np.meshgrid(v, v, indexing="ij"))
    got = synth.evidence_transfer_ref(S, D, zero, "confident", cases.WIDE)[0].reshape(-1)
    order = {int(L): (-1, 0) if L == -128 else (abs(int(L)), int(L)) for L in v}
    want = [s if order[s] > order[d] else d for s, d in zip(S.reshape(-1).tolist(), D.reshape(-1).tolist())]
    assert got.tolist() == want


# ------------------------------------------------------------------------------------------------------- the host layer

def _stand_ins():
    """Maps that carry a geometry and no device memory."""
    torch = pytest.importorskip("torch")
    from trajectory_optimization_amd import ops

    class Grid(ops.OccupancyGrid):
        def __init__(self, origin=(0.0, 0.0, 0.0), r=0.125, dims=(8, 8, 8), device=0):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, r, dims)
            self.device = torch.device("cuda", device)

    class Evid(ops.EvidenceMap):
        def __init__(self, origin=(0.0, 0.0, 0.0), r=0.125, dims=(8, 8, 8)):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, r, dims)
            self.device = torch.device("cuda", 0)

    def space(*a, **kw):
        s = ops.SpaceMap.__new__(ops.SpaceMap)
        s.occupied, s.free = Grid(*a, **kw), Grid(*a, **kw)
        s.device = s.occupied.device
        return s

    return ops, Grid, Evid, space


def test_lattice_rule():
    ops, Grid, Evid, space = _stand_ins()
    a = Grid((1.0, -2.0, 0.5))
    assert ops.lattice_offset(a, Grid((1.0, -2.0, 0.5))) == (0, 0, 0)
    assert ops.lattice_offset(a, Grid((1.375, -2.5, 0.5))) == (3, -4, 0)
    assert ops.lattice_offset(space((1.375, -2.5, 0.5)), a) == (-3, 4, 0)
    # half a voxel off along y: refused, the axis and both origins named
    with pytest.raises(ValueError, match=r"not on one lattice: along y the origins \(1\.0, -2\.0, 0\.5\) and \(1\.0, -1\.9375, 0\.5\)"):
        ops.lattice_offset(a, Grid((1.0, -2.0 + 0.0625, 0.5)))
    # 1/512 of a voxel off (exact in f32): inside the 1/256 tolerance, rounded to the integer
    assert ops.lattice_offset(a, Grid((1.0 + 5 * 0.125 + 0.125 / 512, -2.0, 0.5 - 0.125 / 512))) == (5, 0, 0)
    with pytest.raises(ValueError, match="along z"):
        ops.lattice_offset(a, Grid((1.0, -2.0, 0.5 + 0.125 / 128)))   # 1/128: outside it
    with pytest.raises(ValueError, match="their resolutions differ"):
        ops.lattice_offset(a, Grid((1.0, -2.0, 0.5), r=0.25))
    # an origin that is no multiple of r: the rule looks at the difference only
    assert ops.lattice_offset(Grid((0.1, 0.1, 0.1), r=0.1), Grid(ops.reframed_origin((0.1, 0.1, 0.1), 0.1, (7, -3, 2)), r=0.1)) == (7, -3, 2)


def test_reframed_origin_snapped_and_unsnapped():
    ops, Grid, _, _ = _stand_ins()
    # snapped: origin and r exact in binary, the sum exact
    s, d, o = ops.check_reframe(Grid((1.0, -2.0, 0.5)), shift=(3, -4, 100))
    assert (s, d) == ((3, -4, 100), (8, 8, 8)) and o.dtype == f32 and o.tolist() == [1.375, -2.5, 13.0]
    # unsnapped: float32(float64(origin) + shift * float64(f32 r)), one rounding
    g = Grid((0.1, -0.3, 0.7), r=0.1)
    _, _, o = ops.check_reframe(g, shift=(7, -3, 2), dims=(5, 6, 3))
    want = (np.asarray([0.1, -0.3, 0.7], dtype=f32).astype(np.float64) + np.array([7.0, -3.0, 2.0]) * float(f32(0.1))).astype(f32)
    assert o.tobytes() == want.tobytes()
    # by centre: the position's voxel (f32 index rule) becomes voxel dims // 2
    g = Grid((1.0, -2.0, 0.5), dims=(9, 8, 5))
    s, d, o = ops.check_reframe(g, centre=(1.0 + 20.5 * 0.125, -2.0 - 0.01, 0.5))
    assert s == (20 - 4, -1 - 4, 0 - 2) and d == (9, 8, 5)
    s, d, _ = ops.check_reframe(g, centre=(1.0, -2.0, 0.5), dims=(4, 4, 2))
    assert s == (-2, -2, -1) and d == (4, 4, 2)


def test_check_reframe_and_check_merge_refuse_by_message():
    ops, Grid, Evid, space = _stand_ins()
    g = Grid()
    bad = [
        (dict(map=object(), shift=(0, 0, 0)), "map must be an ops.OccupancyGrid, SpaceMap or EvidenceMap"),
        (dict(), "give exactly one of shift and centre"),
        (dict(shift=(0, 0, 0), centre=(0.0, 0.0, 0.0)), "give exactly one of shift and centre"),
        (dict(shift=(0, 0)), "shift must be three integers"),
        (dict(shift=(0, 0.5, 0)), "shift must be three integers"),
        (dict(shift=7), "shift must be three integers"),
        (dict(shift=(0, 4097, 0)), r"the shift must lie in \[-4096, 4096\]"),
        (dict(shift=(0, 0, -4097)), r"the shift must lie in \[-4096, 4096\]"),
        (dict(shift=(0, 0, 0), dims=(0, 4, 4)), "dims must be three integers"),
        (dict(shift=(0, 0, 0), dims=(4, 4)), "dims must be three integers"),
        (dict(shift=(0, 0, 0), dims=(2048, 2048, 2048)), "at most 2\\^31 voxels"),
        (dict(centre=(0.0, float("nan"), 0.0)), "centre must be three finite numbers"),
        (dict(centre=(0.0, 0.0)), "centre must be three finite numbers"),
        (dict(centre=(0.0, 0.0, 4096 * 0.125)), "centre .* lies beyond the map's apron"),
        (dict(centre=(0.0, 4000 * 0.125, 0.0), dims=(2048, 8, 8)), None),   # fine: a shift of 4000 - 4
    ]
    for kw, text in bad:
        args = dict(map=g)
        args.update(kw)
        if text is None:
            assert ops.check_reframe(**args)[0] == (-1024, 3996, -4)
            continue
        with pytest.raises(ValueError, match=text):
            ops.check_reframe(**args)
    assert ops.check_reframe(g, shift=(4096, -4096, 0))[0] == (4096, -4096, 0)
    assert ops.check_reframe(space(), shift=np.array([1, 2, 3]))[0] == (1, 2, 3)
    assert ops.check_reframe(Evid(), centre=[0.5, 0.5, 0.5])[0] == (0, 0, 0)

    e = Evid()
    refused = [
        ((object(), g), {}, "a must be an ops.OccupancyGrid, SpaceMap or EvidenceMap"),
        ((g, None), {}, "other must be an ops.OccupancyGrid, SpaceMap or EvidenceMap"),
        ((g, space()), {}, "a Grid merges with its own kind, got SpaceMap"),
        ((e, g), dict(mode="add"), "merges with its own kind"),
        ((g, g), {}, "a map cannot be merged into itself"),
        ((g, Grid(device=1)), {}, "the maps must live on one device"),
        ((g, Grid(r=0.25)), {}, "their resolutions differ"),
        ((g, Grid((0.0625, 0.0, 0.0))), {}, "not on one lattice: along x"),
        ((g, Grid()), dict(mode="add"), "mode applies to evidence maps only"),
        ((e, Evid()), {}, "mode must be 'confident' or 'add'"),
        ((e, Evid()), dict(mode="max"), "mode must be 'confident' or 'add'"),
    ]
    for args, kw, text in refused:
        with pytest.raises(ValueError, match=text):
            ops.check_merge(*args, **kw)
    # a's voxel v takes b's voxel v + shift: b's origin 3 voxels up the x axis -> shift -3
    assert ops.check_merge(g, Grid((0.375, -0.25, 0.0))) == ((-3, 2, 0), True)
    assert ops.check_merge(e, Evid((0.375, -0.25, 0.0)), mode="confident") == ((-3, 2, 0), True)
    assert ops.check_merge(space(), space((1.0, 0.0, 0.0))) == ((-8, 0, 0), False)          # the boxes touch: no voxel in common
    assert ops.check_merge(g, Grid((-0.875, 0.0, 0.0))) == ((7, 0, 0), True)                # one layer in common
    assert ops.check_merge(g, Grid((-0.875, 0.0, 0.0), dims=(7, 8, 8))) == ((7, 0, 0), False)


def test_follow_map_stays_or_moves_at_the_margins_boundary_voxel():
    ops, Grid, _, _ = _stand_ins()
    from trajectory_optimization_amd import tools
    moved = []

    class Rolling(Grid):
        def reframed(self, shift=None, dims=None, centre=None):
            moved.append(ops.check_reframe(self, shift, dims, centre)[0])
            return "moved"

    g = Rolling((1.0, -2.0, 0.5), dims=(20, 11, 9))
    at = lambda i, j, k: (1.0 + (i + 0.5) * 0.125, -2.0 + (j + 0.5) * 0.125, 0.5 + (k + 0.5) * 0.125)   # noqa: E731  (a voxel's centre)
    m = 3
    # the boundary voxels: index margin on the low side, n - 1 - margin on the high side stay ...
    for v in ((3, 3, 3), (16, 7, 5), (3, 7, 3), (10, 5, 4)):
        assert tools.follow_map(g, at(*v), m) is g and not moved, v
    # ... one voxel further out on any one axis moves, and the position's voxel becomes the middle voxel dims // 2
    for v in ((2, 5, 4), (17, 5, 4), (10, 2, 4), (10, 8, 4), (10, 5, 2), (10, 5, 6), (-5, 30, 4)):
        assert tools.follow_map(g, at(*v), m) == "moved", v
        assert moved.pop() == (v[0] - 10, v[1] - 5, v[2] - 4) and not moved
    assert tools.follow_map(g, at(0, 0, 0), 0) is g and tools.follow_map(g, at(19, 10, 8), 0) is g   # margin 0: anywhere inside dims
    assert tools.follow_map(g, at(20, 10, 8), 0) == "moved" and moved.pop() == (10, 5, 4)
    # a margin per axis: 9 along x, none along z
    assert tools.follow_map(g, at(9, 3, 0), (9, 3, 0)) is g and tools.follow_map(g, at(10, 7, 8), (9, 3, 0)) is g
    for v in ((8, 5, 4), (11, 5, 4), (10, 2, 4), (10, 5, 9)):
        assert tools.follow_map(g, at(*v), (9, 3, 0)) == "moved" and moved.pop() == (v[0] - 10, v[1] - 5, v[2] - 4), v
    for margin, text in ((5, r"at most \(9, 5, 4\) for dims \(20, 11, 9\)"), (-1, "margin must be an integer or three integers"),
                         (1.5, "margin must be"), ((10, 0, 0), "margin must be"), ((1, 1), "margin must be"), ((1, 1, 0.5), "margin must be")):
        with pytest.raises(ValueError, match=text):
            tools.follow_map(g, at(5, 5, 4), margin)
    with pytest.raises(ValueError, match="position must be three finite numbers"):
        tools.follow_map(g, (0.0, float("inf"), 0.0), m)
    with pytest.raises(ValueError, match="map must be an ops.OccupancyGrid, SpaceMap or EvidenceMap"):
        tools.follow_map(object(), at(5, 5, 4), m)


def test_merge_maps_refuses_by_message():
    ops, Grid, Evid, _ = _stand_ins()
    from trajectory_optimization_amd import tools
    with pytest.raises(ValueError, match="at least two maps"):
        tools.merge_maps([Grid()])
    with pytest.raises(ValueError, match="merges with its own kind"):
        tools.merge_maps([Grid(), Evid()])
    with pytest.raises(ValueError, match="not on one lattice: along z"):
        tools.merge_maps([Grid(), Grid((0.0, 0.0, 0.03))])
    with pytest.raises(ValueError, match="mode applies to evidence maps only"):
        tools.merge_maps([Grid(), Grid()], mode="add")
    with pytest.raises(ValueError, match="mode must be 'confident' or 'add'"):
        tools.merge_maps([Evid(), Evid()], mode="or")
    with pytest.raises(ValueError, match=r"the union box of \(2049, 8, 8\) voxels exceeds 2048 per axis"):
        tools.merge_maps([Grid(), Grid((2041 * 0.125, 0.0, 0.0))])
    with pytest.raises(ValueError, match="exceeds 2048 per axis or 2\\^31 voxels"):
        tools.merge_maps([Grid(dims=(2048, 2048, 8)), Grid((0.0, 0.0, 505 * 0.125), dims=(8, 8, 8))])   # 2048 x 2048 x 512 = 2^31 fits: one more layer


# ------------------------------------------------------------------------------------------------------- the C entries

def test_entries_refuse_bad_arguments_without_gpu():
    """Every argument check returns before anything is enqueued: bad calls come back with their code on a machine without a GPU."""
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    EINVAL, ENOSPC = -1, -2
    assert (_lib.CONSTANTS["TOHIP_EINVAL"], _lib.CONSTANTS["TOHIP_ENOSPC"]) == (EINVAL, ENOSPC)
    p, q, r, t, u = (ctypes.c_void_p(a) for a in (4096, 8192, 16384, 32768, 65536))   # 16-byte aligned pointers no call may reach
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(13, 10, 7): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))   # noqa: E731
    gs, gd = geom(), geom(d=(5, 6, 3))
    sb, db = L.tohip_occ_bytes(13, 10, 7), L.tohip_occ_bytes(5, 6, 3)
    se, de = L.tohip_evid_bytes(13, 10, 7), L.tohip_evid_bytes(5, 6, 3)
    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 6, 3)), geom(d=(5, 2049, 3))]
    calls = {
        "occ": (L.tohip_occ_transfer, ("src", "src_bytes", "src_geom", "dst", "dst_bytes", "dst_geom", "sx", "sy", "sz", "mode", "counts", "stream"),
                (p, sb, gs, q, db, gd, 1, -2, 3, 0, None, None)),
        "evid": (L.tohip_evid_transfer, ("src", "src_bytes", "src_geom", "dst", "dst_bytes", "dst_geom", "occ", "free", "grid_bytes", "sx", "sy",
                                         "sz", "mode", "lmin", "lmax", "threshold", "counts", "stream"),
                 (p, se, gs, q, de, gd, r, t, db, 1, -2, 3, 0, -40, 70, 0, None, None)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name in calls:
        for kw in (dict(src=None), dict(dst=None), dict(src_geom=None), dict(dst_geom=None), dict(src=q), dict(dst=p), dict(mode=-1),
                   dict(mode=3), dict(sx=4097), dict(sy=-4097), dict(sz=1 << 20), dict(counts=p), dict(counts=q)):
            assert call(name, **kw) == EINVAL, (name, kw)
        assert call(name, src_bytes=calls[name][2][1] - 1) == ENOSPC and call(name, dst_bytes=calls[name][2][4] - 1) == ENOSPC, name
        for g in bad_geoms:
            assert call(name, src_geom=g) == EINVAL and call(name, dst_geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    assert call("occ", mode=2) == EINVAL   # (a plane has COPY and OR)
    for kw in (dict(occ=None), dict(free=None), dict(occ=p), dict(occ=q), dict(free=p), dict(free=q), dict(free=r), dict(counts=r), dict(counts=t),
               dict(src=ctypes.c_void_p(4104)), dict(dst=ctypes.c_void_p(8200)), dict(lmin=-128), dict(lmax=128), dict(lmin=1), dict(threshold=70),
               dict(lmin=5, threshold=4)):
        assert call("evid", **kw) == EINVAL, kw
    assert call("evid", grid_bytes=db - 1) == ENOSPC
    assert call("evid", counts=u, mode=2, lmin=-127, lmax=127, threshold=126, sx=4096, sy=-4096, sz=0, dst_geom=geom(d=(0, 6, 3))) == EINVAL
