"""CPU checks of the swept clearance term's C ABI and host settings (no GPU): new symbols and one flag bit under ABI 15, the sizes,
tohip_clearance_segments refusing bad arguments before any launch, and ModelTraj's clearance_mode."""
import ctypes

import pytest

from abi_cases import ABI, check_abi_entries

NEW = ("tohip_clearance_segments", "tohip_clearance_segments_workspace_bytes", "tohip_traj_clearance_segments_scratch_bytes")


def test_header_declares_the_segments_abi():
    from trajectory_optimization_amd import _lib, ops
    header, _ = check_abi_entries(NEW)
    for sym in NEW:
        assert sym + "(" in header and sym in _lib.SIGNATURES
    assert "#define TOHIP_TRAJ_CLEARANCE_SEGMENTS 4" in header and ops.CLEARANCE_SEGMENTS == 4
    still = [line for line in header.splitlines() if f"(still {ABI})" in line]
    assert any("tohip_clearance_segments" in line for line in still)
    for struct in ("tohip_traj_loss", "tohip_traj_opt"):
        body = header[header.index(f"typedef struct {struct} {{"):]
        body = body[:body.index(f"}} {struct};")]
        assert body.rstrip().endswith("size_t clearance_scratch_bytes;")
    for name in ("TrajLoss", "TrajOpt"):
        assert [f[0] for f in getattr(_lib, name)._fields_][-1] == "clearance_scratch_bytes"


def test_sizes():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    ws, sc, old = L.tohip_clearance_segments_workspace_bytes, L.tohip_traj_clearance_segments_scratch_bytes, L.tohip_traj_clearance_scratch_bytes
    for W, B in ((0, 1), (-3, 1), (4, 0), (4, -1), (1, 1)):   # (one waypoint has no segment)
        assert ws(W, B) == 0 and sc(W, B) == 0, (W, B)
    # workspace: terms (B W) f64 | per-segment g_a, g_b (B (W-1), 6) f64, each 256-aligned
    assert ws(2, 1) == 256 + 256 and ws(100, 2) == 1792 + 9728
    # scratch: rows (B W, 3) f32 | terms (B W) f64 at the offsets of the point term's scratch, then the per-segment parts
    assert sc(100, 2) == 2560 + 1792 + 9728
    for W, B in ((2, 1), (23, 1), (100, 2), (128, 8)):
        assert sc(W, B) >= old(W, B) and sc(W, B) - old(W, B) == ws(W, B) - L.tohip_clearance_workspace_bytes(W * B)


def test_segments_rejects_bad_arguments_without_a_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    ib = (ctypes.c_int32 * 64)()
    wsb = (ctypes.c_double * 128)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i = ctypes.cast(ib, ctypes.c_void_p)
    ws = ctypes.cast(wsb, ctypes.c_void_p)
    EINVAL, ENOSPC = -1, -2
    ok = dict(packed=p, n=1000, q=p, W=8, B=1, r=0.5, w=1.0, d=p, idx=i, s=p, value=None, grad=None, ws=ws, wsb=1024)
    assert L.tohip_clearance_segments_workspace_bytes(8, 1) == 768 <= ok["wsb"]

    def call(**kw):
        a = dict(ok, **kw)
        return L.tohip_clearance_segments(a["packed"], a["n"], a["q"], a["W"], a["B"], a["r"], a["w"], a["d"], a["idx"], a["s"], a["value"],
                                          a["grad"], a["ws"], a["wsb"], None)
    for bad in (dict(packed=None), dict(q=None), dict(d=None), dict(idx=None), dict(s=None), dict(ws=None), dict(n=0), dict(n=-5),
                dict(n=2 ** 31), dict(W=1), dict(W=0), dict(W=-2), dict(B=0), dict(B=-1), dict(W=2 ** 20, B=2 ** 20), dict(r=0.0),
                dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")), dict(w=-1.0), dict(w=float("nan")), dict(w=float("inf"))):
        assert call(**bad) == EINVAL, bad
    assert call(wsb=8) == ENOSPC and call(wsb=767) == ENOSPC
    assert call(B=2, W=4, wsb=511) == ENOSPC


def test_one_call_entry_points_check_the_segments_scratch_without_a_gpu():
    """With the flag bit the one-call step asks for the larger scratch (ENOSPC with the point term's size), and the bit is accepted."""
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
    c.scratch_bytes = L.tohip_traj_opt_scratch_bytes(W, B)
    c.clearance_radius, c.clearance_weight = 0.5, 1.0
    c.flags = ops.CLEARANCE_SEGMENTS
    c.clearance_scratch_bytes = L.tohip_traj_clearance_scratch_bytes(W, B)
    assert L.tohip_traj_clearance_segments_scratch_bytes(W, B) > c.clearance_scratch_bytes
    assert L.tohip_traj_opt_step(ctypes.byref(c), 0, None) == -2
    c.flags = 8   # an unknown bit is still refused
    assert L.tohip_traj_opt_step(ctypes.byref(c), 0, None) == -1


def test_model_validates_the_mode_without_a_gpu():
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelTraj
    assert ops.check_clearance_mode("waypoints") == "waypoints" and ops.check_clearance_mode("segments") == "segments"
    for mode in ("edges", "", None, 1):
        with pytest.raises(ValueError, match="clearance_mode"):
            ops.check_clearance_mode(mode)
    with pytest.raises(ValueError, match="clearance_mode"):
        ModelTraj(None, None, None, None, 1, 1, clearance_radius=1.0, clearance_weight=1.0, clearance_mode="edges")
    with pytest.raises(ValueError, match="clearance_mode"):   # validated with the term off, too
        ModelTraj(None, None, None, None, 1, 1, clearance_mode="edges")
    with pytest.raises(ValueError):   # radius and weight are still checked with the mode
        ModelTraj(None, None, None, None, 1, 1, clearance_radius=None, clearance_weight=1.0, clearance_mode="segments")

    class PointShard:   # what ModelTraj reads of distributed.PointShard
        kind = "points"
    with pytest.raises(ValueError, match="PointShard"):
        ModelTraj(None, None, None, None, 1, 1, shard=PointShard(), clearance_radius=1.0, clearance_weight=1.0, clearance_mode="segments")
