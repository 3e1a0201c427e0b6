"""CPU checks of the clearance term's C ABI (no GPU): the new struct fields come after every existing one, and tohip_clearance
refuses null or bad arguments before any launch."""
import ctypes

import pytest

from abi_cases import check_abi_entries


def _prefix_layout(struct, upto):
    """(name, offset, size) of the fields of `struct` before `upto`."""
    out = []
    for f in struct._fields_:
        if f[0] == upto:
            break
        d = getattr(struct, f[0])
        out.append((f[0], d.offset, d.size))
    return out


@pytest.mark.parametrize("name", ["TrajLoss", "TrajOpt"])
def test_new_fields_come_last(name):
    from trajectory_optimization_amd import _lib
    S = getattr(_lib, name)
    names = [f[0] for f in S._fields_]
    new = ["clearance_radius", "clearance_weight", "clearance_scratch", "clearance_scratch_bytes"]
    assert names[-4:] == new
    old_fields = S._fields_[:-4]

    class Old(ctypes.Structure):
        _fields_ = old_fields
    assert _prefix_layout(S, "clearance_radius") == _prefix_layout(Old, None)
    assert getattr(S, "clearance_radius").offset >= ctypes.sizeof(Old) - 8
    assert ctypes.sizeof(S) > ctypes.sizeof(Old)
    # a zero-initialised struct means "off"
    s = S()
    assert s.clearance_weight == 0.0 and s.clearance_radius == 0.0 and not s.clearance_scratch


def test_header_declares_the_clearance_abi():
    from trajectory_optimization_amd import _lib
    entries = ("tohip_clearance", "tohip_clearance_workspace_bytes", "tohip_traj_clearance_scratch_bytes", "tohip_traj_regularizers_clearance",
               "tohip_traj_step_tail_clearance")
    header, _ = check_abi_entries(entries)
    for sym in entries:
        assert sym + "(" in header and sym in _lib.SIGNATURES
    for struct in ("tohip_traj_loss", "tohip_traj_opt"):
        body = header[header.index(f"typedef struct {struct} {{"):]
        body = body[:body.index(f"}} {struct};")]
        assert body.rstrip().endswith("size_t clearance_scratch_bytes;")


def test_sizes():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    assert L.tohip_clearance_workspace_bytes(0) == 0 and L.tohip_clearance_workspace_bytes(-3) == 0
    assert L.tohip_clearance_workspace_bytes(1) == 256 and L.tohip_clearance_workspace_bytes(33) == 512
    assert L.tohip_traj_clearance_scratch_bytes(0, 1) == 0 and L.tohip_traj_clearance_scratch_bytes(4, 0) == 0
    assert L.tohip_traj_clearance_scratch_bytes(100, 2) == 2560 + 1792   # rows (200, 3) f32 | terms 200 f64, 256-aligned


def test_clearance_rejects_bad_arguments_without_a_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    ib = (ctypes.c_int32 * 64)()
    wsb = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i = ctypes.cast(ib, ctypes.c_void_p)
    ws = ctypes.cast(wsb, ctypes.c_void_p)
    EINVAL, ENOSPC = -1, -2
    ok = dict(packed=p, n=1000, q=p, nq=8, r=0.5, w=1.0, d=p, idx=i, value=None, grad=None, acc=0, ws=ws, wsb=512)

    def call(**kw):
        a = dict(ok, **kw)
        return L.tohip_clearance(a["packed"], a["n"], a["q"], a["nq"], a["r"], a["w"], a["d"], a["idx"], a["value"], a["grad"],
                                 a["acc"], a["ws"], a["wsb"], None)
    for bad in (dict(packed=None), dict(q=None), dict(d=None), dict(idx=None), dict(ws=None), dict(n=0), dict(n=-5),
                dict(nq=0), dict(nq=-1), dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")), dict(w=-1.0),
                dict(w=float("nan")), dict(w=float("inf")), dict(n=2 ** 31)):
        assert call(**bad) == EINVAL, bad
    assert call(wsb=8) == ENOSPC
    # the split path's step tail
    f = ctypes.c_float
    null = None
    args = [p, p, p, 23, 1, p, p, 23, 1, p, p, p, p, p, p, 14.0, 0.02, 1e-6, 0.1, 0.0, 0.9, 0.999, 1e-8, 1.2, 0.9, p, p, 0, p]
    assert L.tohip_traj_step_tail_clearance(*args, 1.0, null, ws, None) == EINVAL
    assert L.tohip_traj_step_tail_clearance(*args, 1.0, p, null, None) == EINVAL
    assert L.tohip_traj_step_tail_clearance(*args, float("nan"), p, ws, None) == EINVAL
    assert L.tohip_traj_step_tail_clearance(*args, -1.0, p, ws, None) == EINVAL
    del f


def test_model_refuses_bad_settings_without_a_gpu():
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelTraj
    for r, w in ((None, 1.0), (0.0, 1.0), (-1.0, 1.0), (float("inf"), 1.0), (1.0, -0.5), (1.0, float("nan")), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            ops.check_clearance(r, w)
        with pytest.raises(ValueError):
            ModelTraj(None, None, None, None, 1, 1, clearance_radius=r, clearance_weight=w)
    assert ops.check_clearance(None, 0.0)[1] == 0.0

    class PointShard:   # what ModelTraj reads of distributed.PointShard
        kind = "points"
    with pytest.raises(ValueError, match="PointShard"):
        ModelTraj(None, None, None, None, 1, 1, shard=PointShard(), clearance_radius=1.0, clearance_weight=1.0)


def test_single_regulariser_gradient_with_the_term_on():
    """A gradient that reaches one regulariser entry alone (no dL/d loss, no dL/d clearance) with the term on: only that term's rows."""
    import torch
    from trajectory_optimization_amd.model import _assemble_grads
    W = 5
    reg_sum = torch.full((W, 3), 7.0)
    reg_terms = torch.stack([torch.full((W, 3), float(k + 1)) for k in range(3)])
    clr = torch.ones((W, 3))
    for k in range(3):
        g_terms = tuple(torch.tensor(2.0) if j == k else None for j in range(3))
        pg, qg = _assemble_grads(1, W, None, None, None, g_terms, reg_sum, reg_terms, clr, None)
        assert torch.equal(pg, 2.0 * reg_terms[k]) and torch.equal(qg, torch.zeros((W, 4)))
    # dL/d clearance alone, and with dL/d loss
    pg, _ = _assemble_grads(1, W, None, None, None, (None, None, None), reg_sum, reg_terms, clr, torch.tensor(3.0))
    assert torch.equal(pg, 3.0 * clr)
    pg, _ = _assemble_grads(1, W, None, None, torch.tensor(1.0), (None, None, None), reg_sum, reg_terms, clr, None)
    assert torch.equal(pg, reg_sum + clr)


def test_regularizers_clearance_rejects_bad_arguments_without_a_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    wsb = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws = ctypes.cast(wsb, ctypes.c_void_p)
    args = [p, p, 5, 14.0, 0.02, 1e-6, p, p, p, 0, None, None]
    assert L.tohip_traj_regularizers_clearance(*args, 1.0, None, None) == -1
    assert L.tohip_traj_regularizers_clearance(*args, float("nan"), ws, None) == -1
    assert L.tohip_traj_regularizers_clearance(*args, -1.0, ws, None) == -1
    assert L.tohip_traj_regularizers_clearance(p, p, 2, 14.0, 0.02, 1e-6, p, p, p, 0, None, None, 1.0, ws, None) == -1
