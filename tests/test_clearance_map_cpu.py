"""CPU checks of the clearance term asked of the map (no GPU): the two entry points and the flag bit under ABI 15, every bad argument
refused before a launch, the host's refusals by name, and the numpy restatement (clearance_map_cases.py) on a case worked out by hand."""
import ctypes

import numpy as np
import pytest

import clearance_map_cases as cases
from abi_cases import ABI, check_abi_entries

NEW = ("tohip_clearance_map", "tohip_clearance_map_segments")
EINVAL, ENOSPC = -1, -2
f32 = np.float32


def test_header_declares_the_map_abi():
    from trajectory_optimization_amd import _lib, ops
    header, before = check_abi_entries(NEW)
    still = [line for line in before.splitlines() if f"(still {ABI})" in line]
    assert any("tohip_clearance_map" in line and "TOHIP_TRAJ_CLEARANCE_PREFILLED" in line for line in still)
    assert "#define TOHIP_TRAJ_CLEARANCE_PREFILLED 8\n" in header
    assert _lib.CONSTANTS["TOHIP_TRAJ_CLEARANCE_PREFILLED"] == 8 == ops.CLEARANCE_PREFILLED
    for name in ("TrajLoss", "TrajOpt"):   # no struct change
        assert [f[0] for f in getattr(_lib, name)._fields_][-1] == "clearance_scratch_bytes"


def _host_args():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    dims = (13, 10, 7)
    grid_bytes = L.tohip_occ_bytes(*dims)
    keep = [(ctypes.c_uint8 * grid_bytes)(), (ctypes.c_uint8 * grid_bytes)(), (ctypes.c_float * 64)(), (ctypes.c_int32 * 64)(),
            (ctypes.c_double * 256)()]
    occ, fre, p, i, ws = (ctypes.cast(b, ctypes.c_void_p) for b in keep)

    def geom(origin=(0.23, -0.41, 0.07), res=0.1, dims=dims):
        return _lib.OccGeom((ctypes.c_float * 3)(*origin), res, (ctypes.c_int32 * 3)(*dims))
    return L, keep, occ, fre, p, i, ws, grid_bytes, geom


BAD_MAP = (dict(occ=None), dict(fre="occ"), dict(geom=None), dict(gb=8), dict(dims=(0, 10, 7)), dict(dims=(13, -1, 7)), dict(dims=(13, 10, 4096)),
           dict(dims=(2048, 2048, 1024)), dict(res=0.0), dict(res=-0.1), dict(res=float("nan")), dict(origin=(float("inf"), 0.0, 0.0)),
           dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")), dict(r=6.5), dict(r=0.5, res=0.0078), dict(w=-1.0),
           dict(w=float("nan")), dict(w=float("inf")))


def _map_head(a, occ, geom):
    g = None
    if a.get("geom", 1) is not None:
        g = ctypes.byref(geom(a.get("origin", (0.23, -0.41, 0.07)), a.get("res", 0.1), a.get("dims", (13, 10, 7))))
    return a["occ"], (occ if a["fre"] == "occ" else a["fre"]), a["gb"], g


def test_point_entry_rejects_bad_arguments_without_a_gpu():
    L, keep, occ, fre, p, i, ws, grid_bytes, geom = _host_args()
    ok = dict(occ=occ, fre=fre, gb=grid_bytes, q=p, n=8, r=0.5, w=1.0, d=p, idx=i, ws=ws, wsb=2048)
    assert L.tohip_clearance_workspace_bytes(8) == 256

    def call(**kw):
        a = dict(ok, **kw)
        return L.tohip_clearance_map(*_map_head(a, occ, geom), a["q"], a["n"], a["r"], a["w"], a["d"], a["idx"], None, None, 0, a["ws"], a["wsb"],
                                     None)
    for bad in BAD_MAP + (dict(q=None), dict(d=None), dict(idx=None), dict(ws=None), dict(n=0), dict(n=-5), dict(n=2 ** 31)):
        assert call(**bad) == (ENOSPC if "gb" in bad else EINVAL), bad
    assert call(wsb=8) == ENOSPC and call(wsb=255) == ENOSPC
    assert call(r=6.4, n=-1) == EINVAL   # (64 voxels is allowed: what is refused here is the count)


def test_segment_entry_rejects_bad_arguments_without_a_gpu():
    L, keep, occ, fre, p, i, ws, grid_bytes, geom = _host_args()
    ok = dict(occ=occ, fre=fre, gb=grid_bytes, q=p, W=8, B=1, r=0.5, w=1.0, d=p, idx=i, s=p, ws=ws, wsb=2048)
    assert L.tohip_clearance_segments_workspace_bytes(8, 1) == 768

    def call(**kw):
        a = dict(ok, **kw)
        return L.tohip_clearance_map_segments(*_map_head(a, occ, geom), a["q"], a["W"], a["B"], a["r"], a["w"], a["d"], a["idx"], a["s"], None,
                                              None, a["ws"], a["wsb"], None)
    for bad in BAD_MAP + (dict(q=None), dict(d=None), dict(idx=None), dict(s=None), dict(ws=None), dict(W=1), dict(W=0), dict(W=-2), dict(B=0),
                          dict(B=-1), dict(W=2 ** 20, B=2 ** 20)):
        assert call(**bad) == (ENOSPC if "gb" in bad else EINVAL), bad
    assert call(wsb=8) == ENOSPC and call(wsb=767) == ENOSPC
    assert call(B=2, W=4, wsb=511) == ENOSPC


def test_one_call_step_takes_the_prefilled_bit_without_a_gpu():
    """The bit is part of tohip_traj_opt_step's mask now: with it the step still checks the scratch (ENOSPC for a short one, in either
    mode; EINVAL for one that is another buffer of the struct: it holds the caller's rows while the step writes the others), and the
    next bit up is still refused."""
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    W, B = 23, 2
    c = _lib.TrajOpt()
    c.packed, c.n_points, c.n_wps, c.wps_step, c.n_traj, c.n_steps = p, 1000, W, 1, B, 1
    for name in ("traj_offsets", "poses", "quats", "poses0", "exp_avg_p", "exp_avg_sq_p", "exp_avg_q", "exp_avg_sq_q", "poses_grad", "quats_grad",
                 "lo_sum", "minmax", "rewards", "scalars", "loss_log", "state_log", "workspace", "scratch", "clearance_scratch"):
        setattr(c, name, p)
    own = (ctypes.c_float * 64)()
    c.clearance_scratch = ctypes.cast(own, ctypes.c_void_p).value
    c.scratch_bytes = L.tohip_traj_opt_scratch_bytes(W, B)
    c.clearance_radius, c.clearance_weight = 0.5, 1.0
    c.flags = ops.CLEARANCE_PREFILLED
    c.clearance_scratch_bytes = L.tohip_traj_clearance_scratch_bytes(W, B) - 1
    assert L.tohip_traj_opt_step(ctypes.byref(c), 0, None) == ENOSPC
    for other in ("poses", "quats", "poses_grad", "workspace", "scratch", "rewards"):   # the scratch is a buffer of its own
        mine = getattr(c, other)
        setattr(c, other, c.clearance_scratch)
        assert L.tohip_traj_opt_step(ctypes.byref(c), 0, None) == EINVAL, other
        setattr(c, other, mine)
    assert L.tohip_traj_opt_step(ctypes.byref(c), 0, None) == ENOSPC
    c.flags = ops.CLEARANCE_PREFILLED | ops.CLEARANCE_SEGMENTS
    c.clearance_scratch_bytes = L.tohip_traj_clearance_scratch_bytes(W, B)
    assert L.tohip_traj_opt_step(ctypes.byref(c), 0, None) == ENOSPC
    c.flags = ops.CLEARANCE_PREFILLED | 16
    assert L.tohip_traj_opt_step(ctypes.byref(c), 0, None) == EINVAL


def test_host_refuses_by_name_without_a_gpu():
    from trajectory_optimization_amd import ops, optimizer
    from trajectory_optimization_amd.model import ModelTraj
    grid = object.__new__(ops.OccupancyGrid)   # (no GPU here: what the host checks read of a grid is its type and its resolution)
    grid.resolution = 0.1
    other = object.__new__(ops.OccupancyGrid)
    other.resolution = 0.1
    space = object.__new__(ops.SpaceMap)
    space.occupied, space.free = grid, other
    with pytest.raises(ValueError, match="unknown='obstacle' needs"):
        ops.MapObstacles(grid, "obstacle")
    for unknown in ("occupied", None, 1):
        with pytest.raises(ValueError, match="unknown must be"):
            ops.MapObstacles(grid, unknown)
        with pytest.raises(ValueError, match="unknown must be"):
            ops.MapObstacles(space, unknown)
    for bad in (3, "grid", object(), np.zeros((4, 4, 4), bool)):
        with pytest.raises(ValueError, match="clearance_map"):
            ops.MapObstacles(bad)
        with pytest.raises(ValueError, match="clearance_map"):
            ModelTraj(None, None, None, None, 1, 1, clearance_map=bad)
    with pytest.raises(ValueError, match="unknown='obstacle' needs"):
        ModelTraj(None, None, None, None, 1, 1, clearance_map=grid, clearance_unknown="obstacle")
    src = ops.MapObstacles(space, "obstacle")
    assert src.occupied is grid and src.free is other and ops.MapObstacles(space).free is None
    assert src.same_as(ops.MapObstacles(space, "obstacle")) and not src.same_as(ops.MapObstacles(space)) and not src.same_as(None)
    assert ops.MapObstacles(grid).same_as(ops.MapObstacles(space)) and not ops.MapObstacles(grid).same_as(ops.MapObstacles(other))
    # the radius cap: 64 voxels
    ops.MapObstacles(grid).check_radius(6.4)
    with pytest.raises(ValueError, match="clearance_radius"):
        ops.MapObstacles(grid).check_radius(6.5)
    with pytest.raises(ValueError, match="clearance_radius"):
        ops.MapObstacles(grid).check_radius(float("nan"))

    # team / batched members with different maps
    class Member:
        _clearance_on = True
        clearance_radius, clearance_weight, clearance_mode = 0.5, 1.0, "waypoints"
        smoothness_weight, traj_length_weight, _flags, _rig, _occlusion = 14.0, 0.02, 0, None, None
        device, eps = "cuda:0", 1e-6

        class _shard:
            world_size = 1

        class _cloud:
            n = 10

        class _cam:
            c = (ctypes.c_float * 4)()

        class poses:
            shape = (8, 3)

        class points:
            @staticmethod
            def data_ptr():
                return 1

        def __init__(self, clr_map):
            self._clr_map = clr_map

        def _wps_step(self, dist):
            return 1
    for what, (a, b) in {"different maps": (ops.MapObstacles(grid), ops.MapObstacles(other)),
                         "a map and none": (ops.MapObstacles(grid), None), "none and a map": (None, ops.MapObstacles(grid)),
                         "different unknown": (ops.MapObstacles(space), ops.MapObstacles(space, "obstacle"))}.items():
        with pytest.raises(ValueError, match="clearance_map"):
            optimizer._check_same_setup([Member(a), Member(b)], 0.5, "optimize_team")
    optimizer._check_same_setup([Member(ops.MapObstacles(grid)), Member(ops.MapObstacles(space))], 0.5, "optimize_team")
    optimizer._check_same_setup([Member(None), Member(None)], 0.5, "optimize_team")


def test_restatement_on_the_hand_computed_corner():
    """Grid 3 x 3 x 3 of 1 m voxels at the origin, the eight voxels (0..1)^3 occupied, the waypoint on their shared corner (1, 1, 1):
    every centre is at (+-0.5, +-0.5, +-0.5) from it, d2 = 0.25 + 0.25 + 0.25 = 0.75 exactly in float32 for all eight, so the key
    decides by index and voxel (0, 0, 0), linear index 0, wins.  d = fl(sqrt(0.75)); with r = 1, w = 2: term = (1 - sqrt(0.75))^2 and the
    gradient row is -2 w (r - d) (t - c) / d = -4 (1 - sqrt(.75)) 0.5 / sqrt(.75) per axis."""
    H = cases.HAND
    lin, C = cases.obstacles(cases.hand_grid(), origin=H["origin"], res=H["res"])
    assert lin.tolist() == [0, 1, 3, 4, 9, 10, 12, 13] and C[0].tolist() == [0.5, 0.5, 0.5] and C[-1].tolist() == [1.5, 1.5, 1.5]
    d2 = cases.point_d2(H["t"], C)
    assert (d2 == f32(0.75)).all()
    assert cases.winner(d2, lin, H["r"]) == (0, f32(0.75))
    assert cases.winner(d2[::-1].copy(), lin[::-1].copy(), H["r"])[0] == 7   # (whatever order they are met in: lin 0 again)
    assert cases.winner(d2, lin, np.sqrt(f32(0.75)))[0] == -1                # fl(r r) <= 0.75: strict '<', not a hit
    out = cases.query_points(lin, C, [H["t"]], H["r"], H["w"])
    root = np.sqrt(np.float64(0.75))
    assert out["idx"].tolist() == [0] and out["d"][0] == f32(root)
    assert out["term"][0] == (1.0 - root) ** 2 and out["value"] == f32(2.0 * (1.0 - root) ** 2)
    g = f32(-4.0 * (1.0 - root) * 0.5 / root)
    assert g < 0 and out["grad"].tolist() == [[g, g, g]]
    # the same corner as a degenerate segment (the point query), then a segment that leaves it along +x to (3, 1, 1): e = (2, 0, 0),
    # the four centres at x = 1.5 project to s = 0.25 and lie at (0, +-0.5, +-0.5) from the segment, d2 = 0.5: the lowest of them is
    # voxel (1, 0, 0), index 1; g_b = -2 w (1 - sqrt(.5)) s (c - x) / |c - x| with c - x = (0, 0.5, 0.5)
    seg = cases.query_segments(lin, C, [H["t"], H["t"], (3.0, 1.0, 1.0)], H["r"], H["w"])
    half = np.sqrt(np.float64(0.5))
    assert seg["idx"].tolist() == [0, 1] and seg["d"].tolist() == [f32(root), f32(half)] and seg["s"].tolist() == [0.0, 0.25]
    gb = f32(-4.0 * (1.0 - half) / half * 0.25 * 0.5)
    assert seg["grad"][0].tolist() == [g, g, g] and seg["grad"][2].tolist() == [0.0, gb, gb]
    assert seg["term"].tolist() == [(1.0 - root) ** 2, (1.0 - half) ** 2, 0.0]
    # unknown as obstacle: with a free plane that covers nothing, every voxel inside dims is one; the corner's nearest are the same eight
    lin_u, C_u = cases.obstacles(cases.hand_grid(), np.zeros(H["dims"], bool), origin=H["origin"], res=H["res"])
    assert len(lin_u) == 27 and cases.query_points(lin_u, C_u, [H["t"]], H["r"])["idx"].tolist() == [0]


def test_case_1_is_what_the_gpu_tests_expect():
    """The shared grid: about 40 voxels with some in every partial brick and at the three far corners; the ties of the corner and the
    face query are exact in float32; the strict '<' query exists for every radius."""
    vox = cases.case1_voxels()
    assert len(vox) == 40 and {(12, 0, 0), (0, 9, 0), (0, 0, 6)} <= set(map(tuple, vox.tolist()))
    assert (vox[:, 0] >= 12).any() and (vox[:, 1] >= 8).any() and (vox[:, 2] >= 6).any()
    lin, C = cases.obstacles(cases.dense(vox))
    assert (np.diff(lin) > 0).all() and np.array_equal(lin, np.sort(cases.linear(vox)))
    for r in cases.RADII:
        names, q = cases.case1_points(r)
        d2 = cases.point_d2(q[names.index("corner")], C)
        assert (d2 == d2.min()).sum() == 8
        d2 = cases.point_d2(q[names.index("face")], C)
        assert (d2 == d2.min()).sum() == 2
        d2 = cases.point_d2(q[names.index("exactly r")], C)
        assert (d2 == f32(r) * f32(r)).sum() >= 1
    out = cases.query_points(lin, C, cases.case1_points(0.04)[1], 0.04)
    assert out["idx"][cases.case1_points(0.04)[0].index("exactly r")] == -1
