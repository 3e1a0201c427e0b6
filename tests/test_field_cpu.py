"""CPU checks of the clearance field (no GPU): the new entry points are declared in the header and in _lib's table at ABI 15; each
refuses bad arguments before any launch; ops.check_field refuses by name; and the numpy restatements (synth.field_ref / field_brute /
field_segments_ref / field_need2 / field_nodes_ref, what the kernels are compared against bit for bit) are checked against each
other, on hand cases, against f64 point-segment distances in a scanned room and — for the centre metric — against scipy."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_field_bytes", "tohip_field_workspace_bytes", "tohip_field_build", "tohip_field_positions", "tohip_field_segments",
           "tohip_field_nodes")
SMALL = ((5, 6, 3), (1, 1, 1), (12, 9, 7), (16, 16, 8))


def test_header_and_table_declare_the_new_entries_at_abi_15():
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_field_build" in before
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert '#include "frontier_kernels.hip"\n#include "field_kernels.hip"' in src


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    p, q, r, t, u = (ctypes.c_void_p(v) for v in (64, 4096, 8192, 16384, 32768))   # pointers no call may reach
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))
    ok = geom()
    nb, fb = L.tohip_occ_bytes(64, 64, 32), L.tohip_field_bytes(64, 64, 32)
    assert fb == 2 * 64 * 64 * 32 == L.tohip_field_workspace_bytes(64, 64, 32) and L.tohip_field_bytes(5, 6, 3) == 180
    for bad in ((0, 4, 4), (4, 4, 2049), (2048, 2048, 2048)):
        assert L.tohip_field_bytes(*bad) == 0 and L.tohip_field_workspace_bytes(*bad) == 0, bad
    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 64, 32)), geom(d=(64, 2049, 32))]
    calls = {
        "build": (L.tohip_field_build, ("occ", "free", "grid_bytes", "geom", "D", "field", "bytes", "ws", "ws_bytes", "stream"),
                  (p, None, nb, ok, 8, q, fb, r, fb, None)),
        "positions": (L.tohip_field_positions, ("field", "bytes", "geom", "pos", "m", "d2", "dist", "stream"), (q, fb, ok, r, 10, t, None, None)),
        "segments": (L.tohip_field_segments, ("field", "bytes", "geom", "a", "b", "n", "d2", "vox", "need2", "ed", "ei", "stream"),
                     (q, fb, ok, r, t, 10, u, p, 0, None, None, None)),
        "nodes": (L.tohip_field_nodes, ("field", "bytes", "occ", "free", "nodes", "grid_bytes", "geom", "need2", "stride", "stream"),
                  (q, fb, None, None, r, nb, ok, 4, 1, None)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name in calls:
        assert call(name, field=None) == EINVAL, name
        assert call(name, geom=None) == EINVAL, name
        assert call(name, bytes=fb - 1) == ENOSPC, name
        for g in bad_geoms:
            assert call(name, geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    for kw in (dict(occ=None), dict(D=0), dict(D=255), dict(D=-1), dict(ws=None), dict(ws=q), dict(field=p), dict(ws=p), dict(free=p), dict(free=q),
               dict(free=r)):
        assert call("build", **kw) == EINVAL, kw
    assert call("build", grid_bytes=nb - 1) == ENOSPC and call("build", ws_bytes=fb - 1) == ENOSPC
    for kw in (dict(pos=None), dict(m=-1), dict(d2=None, dist=None)):
        assert call("positions", **kw) == EINVAL, kw
    for kw in (dict(a=None), dict(b=None), dict(n=-1), dict(d2=None), dict(vox=None), dict(ed=p), dict(ei=p), dict(ed=p, ei=q, need2=-1),
               dict(ed=p, ei=q, need2=65536)):
        assert call("segments", **kw) == EINVAL, kw
    for kw in (dict(nodes=None), dict(occ=p), dict(free=p), dict(nodes=q), dict(occ=p, free=r), dict(occ=r, free=p), dict(need2=-1),
               dict(need2=65536), dict(stride=0), dict(stride=-2), dict(stride=2049)):
        assert call("nodes", **kw) == EINVAL, kw
    assert call("nodes", grid_bytes=nb - 1) == ENOSPC
    # (empty queries are fine and launch nothing)
    assert call("positions", m=0, pos=None, d2=None) == 0 and call("segments", n=0, a=None, b=None, d2=None, vox=None) == 0


def test_check_field_names_every_refusal():
    from trajectory_optimization_amd import ops, tools

    class G(ops.OccupancyGrid):   # a grid's geometry without a device
        def __init__(self, origin=(0, 0, 0), resolution=0.1, dims=(8, 8, 4), device="cuda:0"):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, resolution, dims)
            self.device = torch.device(device)

    g = G()
    space = ops.SpaceMap(g, G())
    r = float(np.float32(0.1))
    occ, free, D, need2 = ops.check_field(g, 0.5)
    assert occ is g and free is None and D == int(np.ceil(0.5 / r)) == 5 == synth.field_max_dist_voxels(0.5, 0.1) and need2 is None
    assert ops.check_field(space, 0.5)[:3] == (g, None, 5) and ops.check_field(space, 0.5, "obstacle")[:3] == (g, space.free, 5)
    assert ops.check_field(g, 0.01)[2] == 1 and ops.check_field(g, 25.4)[2] == 254 and ops.check_field(G(resolution=0.125), 1.0)[2] == 8
    assert ops.check_field(g, D=np.int64(7))[2] == 7
    for bad in (None, object(), torch.zeros(4, 3)):
        with pytest.raises(ValueError, match="the map must be an ops.OccupancyGrid or an ops.SpaceMap"):
            ops.check_field(bad, 0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 25.5, 1e30, "x", True, None):
        with pytest.raises(ValueError, match="max_dist must be a finite number of metres > 0 and at most 254 voxels"):
            ops.check_field(g, bad)
    for bad in (0, 255, -3, 2.0, True):
        with pytest.raises(ValueError, match="D must be an integer number of voxels in \\[1, 254\\]"):
            ops.check_field(g, D=bad)
    for bad in ("unknown", None, 1):
        with pytest.raises(ValueError, match="unknown must be 'free' or 'obstacle'"):
            ops.check_field(g, 0.5, bad)
    with pytest.raises(ValueError, match="unknown='obstacle' needs an ops.SpaceMap"):
        ops.check_field(g, 0.5, "obstacle")
    # a radius: need2 = ceil((radius / r + 1/64)^2) <= D^2, and the error names the largest radius the field certifies
    assert ops.check_field(g, 0.5, radius=0.3)[3] == synth.field_need2(0.3, 0.1) == ops.field_need2(0.3, 0.1) == 10
    assert ops.check_field(g, D=5, radius=0.498)[3] == 25
    with pytest.raises(ValueError, match="clearance_radius 0.5 needs a squared gap of 26 voxels, this field is truncated at D = 5 \\(25\\): "
                                         "the largest radius it can certify is 0.498438 m"):
        ops.check_field(g, 0.5, radius=0.5)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clearance_radius must be a finite number > 0"):
            ops.check_field(g, 0.5, radius=bad)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="stride must be an integer >= 1"):
            ops.check_field(g, 0.5, stride=bad)
    assert ops.check_field(g, 0.5, stride=np.int32(5), space=space)[2] == 5
    with pytest.raises(ValueError, match="space must be an ops.SpaceMap or None"):
        ops.check_field(g, 0.5, space=g)
    for other, what in ((G(origin=(0, 0, 0.5)), "origin"), (G(resolution=0.2), "resolution"), (G(dims=(8, 8, 5)), "dims"),
                        (G(device="cuda:1"), "device")):
        with pytest.raises(ValueError, match=f"space: its {what} differs from the field's"):
            ops.check_field(g, 0.5, space=ops.SpaceMap(other, G(other.origin, other.resolution, other.dims, other.device)))
    with pytest.raises(ValueError, match="free_nodes: field must be an ops.ClearanceField"):
        tools.free_nodes(g, 0.3)
    with pytest.raises(ValueError, match="the map must be an ops.OccupancyGrid or an ops.SpaceMap"):
        tools.clearance_field(torch.zeros(4, 3), 0.5)
    # propose_views takes no field: its refusal is the one it has for anything that is no cloud
    with pytest.raises(ValueError, match="propose_views: points must be an \\(N,3\\) tensor"):
        tools._clearance_cloud(object.__new__(ops.ClearanceField), "propose_views")
    assert tools._clearance_cloud(f := object.__new__(ops.ClearanceField), "plan_path", field=True) == (f, None)


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def _planes(dims, p_occ, seed):
    rng = np.random.default_rng(seed)
    return rng.random(dims) < p_occ, rng.random(dims) < 0.7


@pytest.mark.parametrize("dims", SMALL)
def test_field_ref_is_the_brute_force_minimum(dims):
    for k, p_occ in enumerate((0.0, 0.02, 0.3, 1.0)):
        occ, free = _planes(dims, p_occ, 17 * k + dims[0])
        for D in (1, 3, 8, 254):
            for unknown in ("free", "obstacle"):
                ref = synth.field_ref(occ, free, D, unknown)
                assert ref.dtype == np.int64 and np.array_equal(ref, synth.field_brute(occ, free, D, unknown)), (dims, p_occ, D, unknown)
                assert ((ref <= D * D) | (ref == 65535)).all()
        if p_occ == 0.0:
            assert (synth.field_ref(occ, None, 8) == 65535).all()
        if p_occ == 1.0:
            assert (synth.field_ref(occ, None, 8) == 0).all()
    # occupied wins over a free bit set inside it; unknown (neither bit) is an obstacle only when asked
    occ, free = np.zeros(dims, dtype=bool), np.ones(dims, dtype=bool)
    occ[0, 0, 0] = True
    assert np.array_equal(synth.field_ref(occ, free, 8, "obstacle"), synth.field_ref(occ, None, 8))
    free[-1, -1, -1] = False
    if dims != (1, 1, 1):
        assert synth.field_ref(occ, free, 8, "obstacle")[-1, -1, -1] == 0 != synth.field_ref(occ, free, 8, "free")[-1, -1, -1]


def test_one_obstacle_by_hand_and_the_truncation():
    occ = np.zeros((5, 6, 3), dtype=bool)
    occ[2, 2, 1] = True
    # every k holds the same plane (|k - 1| <= 1): rows are j = 0 .. 5, columns i = 0 .. 4; the obstacle and its 26 neighbours hold 0
    plane = [[2, 1, 1, 1, 2],
             [1, 0, 0, 0, 1],
             [1, 0, 0, 0, 1],
             [1, 0, 0, 0, 1],
             [2, 1, 1, 1, 2],
             [5, 4, 4, 4, 5]]
    want = np.array([plane, plane, plane], dtype=np.int64).transpose(2, 1, 0)   # (k, j, i) -> (i, j, k)
    assert want.size == 90
    for D in (3, 8, 254):
        assert np.array_equal(synth.field_ref(occ, None, D), want), D
    # D = 2: 5 > 4 is dropped; D = 1: only 0 and 1 remain
    assert np.array_equal(synth.field_ref(occ, None, 2), np.where(want <= 4, want, 65535))
    d1 = synth.field_ref(occ, None, 1)
    assert np.array_equal(d1, np.where(want <= 1, want, 65535)) and (d1 == 65535).sum() == 3 * 9 and (d1 == 0).sum() == 27
    # a far corner, D larger than the grid: the gap is one less than the index difference per axis
    occ = np.zeros((37, 5, 20), dtype=bool)
    occ[36, 0, 19] = True
    f = synth.field_ref(occ, None, 254)
    assert f[0, 4, 0] == 35 ** 2 + 3 ** 2 + 18 ** 2 and f[35, 1, 18] == 0 and f[34, 0, 19] == 1
    assert synth.field_ref(occ, None, 8)[0, 4, 0] == 65535
    # the linear index and the distance in metres
    assert np.array_equal(synth.field_metres([0, 1, 2, 64516, 65535, -1], 0.125).view(np.uint32),
                          np.float32([0.0, 0.125, np.float32(np.sqrt(np.float32(2))) * np.float32(0.125), 254 * 0.125, np.inf, np.nan]).view(np.uint32))


def test_need2_at_whole_voxels_and_an_out_of_range_leg_is_blocked():
    # radius = k r with r exact in f32: (k + 1/64)^2 = k^2 + k / 32 + 1 / 4096 -> k^2 + 1 for k < 32, k^2 + 2 from there to 63
    for k in (1, 2, 3, 7, 31):
        assert synth.field_need2(k * 0.125, 0.125) == k * k + 1, k
    assert synth.field_need2(32 * 0.125, 0.125) == 32 * 32 + 2 and synth.field_need2(1e-9, 0.125) == 1
    # r = 0.1 is not exact: f32(0.1) > 0.1, so 0.3 m is just under 3 voxels
    assert synth.field_need2(0.3, 0.1) == 10 and synth.field_need2(0.15, 0.1) == 3
    field = np.full((8, 8, 4), 65535, dtype=np.int64)
    field[3, 3, 1] = 2
    a = np.float32([[0.05, 0.35, 0.15], [0.05, 0.35, 0.15], [0.05, 0.35, 0.15], [np.nan, 0, 0], [0.05, 0.05, 0.05], [-3.0, 0.35, 0.15]])
    b = np.float32([[0.75, 0.35, 0.15], [0.25, 0.35, 0.15], [0.75, 0.35, 500.0], [0.1, 0, 0], [0.05, 0.05, 0.05], [-2.0, 0.35, 0.15]])
    d2, vox = synth.field_segments_ref(a, b, (0, 0, 0), 0.1, field)
    assert d2.tolist() == [2, 65535, -1, -1, 65535, 65535] and vox.tolist() == [(1 * 8 + 3) * 8 + 3, -1, -1, -1, -1, -1]
    d, idx = synth.field_edges_ref(d2, vox, 3, 0.1)
    # open iff idx == -1: the leg that leaves the map's coordinate range (-2) is never certified
    assert idx.tolist() == [91, -1, -2, -2, -1, -1] and np.isinf(d[[1, 4, 5]]).all() and d[2] == 0 == d[3]
    assert d[0] == np.float32(np.sqrt(np.float32(2))) * np.float32(0.1)
    assert synth.field_edges_ref(d2, vox, 2, 0.1)[1].tolist() == [-1, -1, -2, -2, -1, -1]   # d2 >= need2 is open
    # first argmin in walk order: two voxels hold the minimum, the walk direction decides
    field[5, 3, 1] = 2
    d2, vox = synth.field_segments_ref(a[[0, 0]], np.stack([b[0], a[0]]), (0, 0, 0), 0.1, field)
    assert vox.tolist() == [91, -1]
    d2, vox = synth.field_segments_ref(b[[0]], a[[0]], (0, 0, 0), 0.1, field)
    assert vox.tolist() == [(1 * 8 + 3) * 8 + 5]
    assert synth.field_positions_ref(np.float32([[0.35, 0.35, 0.15], [0.95, 0.1, 0.1], [-0.01, 0.1, 0.1], [np.inf, 0, 0], [500.0, 0, 0]]),
                                     (0, 0, 0), 0.1, field).tolist() == [2, 65535, 65535, -1, -1]


def test_nodes_restated():
    field = np.arange(5 * 6 * 3, dtype=np.int64).reshape(5, 6, 3)
    m = synth.field_nodes_ref(field, 40)
    assert np.array_equal(m, field >= 40)
    m2 = synth.field_nodes_ref(field, 0, stride=2)   # indices 1, 3, ...
    assert np.argwhere(m2).tolist() == [[i, j, 1] for i in (1, 3) for j in (1, 3, 5)]
    m5 = synth.field_nodes_ref(field, 0, stride=5)   # index 2 alone
    assert np.argwhere(m5).tolist() == [[2, 2, 2]]
    state = np.ones((5, 6, 3), dtype=np.int64)
    state[1, 1, 1], state[3, 5, 1] = 0, 2
    assert np.argwhere(synth.field_nodes_ref(field, 0, 2, state)).tolist() == [[1, 3, 1], [1, 5, 1], [3, 1, 1], [3, 3, 1]]
    assert not synth.field_nodes_ref(field, 90).any()


def test_every_open_leg_keeps_the_radius_from_the_scanned_room():
    """The guarantee, in numpy alone: the occupied grid filled from box_room(doorway=True) at r = 0.1, 2 000 seeded legs; a leg the
    restated field calls open (d2 >= need2) is at least `radius` from every row of the cloud by f64 point-segment distances."""
    S = synth.FIELD_ROOM
    P = synth.box_room(doorway=True)
    occ, skipped = synth.occupancy_ref(P, S["origin"], S["resolution"], S["dims"])
    assert skipped == 0
    field = synth.field_ref(occ, None, synth.field_max_dist_voxels(0.5, S["resolution"]))
    a, b = synth.field_room_legs()
    d2, vox = synth.field_segments_ref(a, b, S["origin"], S["resolution"], field)
    assert (d2 >= 0).all()
    loose = d2 >= synth.field_need2(0.15, S["resolution"])
    true = synth.segment_point_distance(a[loose], b[loose], P)
    for radius in (0.15, 0.3):
        opened = d2[loose] >= synth.field_need2(radius, S["resolution"])
        assert opened.sum() >= 100, (radius, int(opened.sum()))   # (a condition on the seed: the GPU test asks the same legs)
        assert (true[opened] >= radius).all(), (radius, float(true[opened].min()))


def test_centre_metric_matches_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    occ = rng.random((64, 64, 32)) < 0.01
    D = 12
    ref = synth.field_ref(occ, None, D, metric="centre")
    edt2 = np.rint(ndi.distance_transform_edt(~occ) ** 2).astype(np.int64)
    assert np.array_equal(ref, np.where(edt2 <= D * D, edt2, 65535))
    small = occ[:12, :9, :7]
    assert np.array_equal(synth.field_ref(small, None, D, metric="centre"), synth.field_brute(small, None, D, metric="centre"))
