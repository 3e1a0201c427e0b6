"""CPU checks of the tour planner (no GPU): the three entry points are declared in the header and in _lib's table with matching
argument counts and without a new ABI version; tohip_tour_bytes follows the documented layout; each entry refuses bad arguments
before any launch; every argument the host layer does not accept is refused with a ValueError that names it, before any GPU call;
the numpy restatement of the definition (synth.tour_plan) gives the orders geometry dictates."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from abi_cases import check_abi_entries

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_clearance_edges", "tohip_tour_bytes", "tohip_tour_plan")


def test_header_and_table_declare_the_tour_entries():
    from trajectory_optimization_amd import ops
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_tour_plan" in before
    assert f"#define TOHIP_TOUR_MAX_NODES {ops.TOUR_MAX_NODES}\n" in header
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert '#include "tour_kernels.hip"' in src


def test_tour_bytes_is_the_documented_layout():
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for n in (2, 33, 256):
        want = 256 + up(4 * n) + up(n) + up(8 * n * n) + up(4 * n * n)
        lay = ops.tour_layout(n)
        assert L.tohip_tour_bytes(n) == want == lay["total"], n
        assert lay["header"] == 0 and lay["order"] == 256 and lay["unreachable"] == 256 + up(4 * n)
        assert lay["D"] == lay["unreachable"] + up(n) and lay["nxt"] == lay["D"] + up(8 * n * n)
    for bad in (1, 257, 0, -1, -(1 << 40)):
        assert L.tohip_tour_bytes(bad) == 0, bad


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)   # a non-null pointer no call may reach: every case below fails its checks first

    names = ("packed", "n_points", "a", "b", "n_edges", "radius", "d", "idx", "s", "stream")
    base = dict(zip(names, (p, 5000, p, p, 10, 0.5, p, p, p, None)))
    edges = lambda **kw: L.tohip_clearance_edges(*[kw.get(k, base[k]) for k in names])
    for k in ("packed", "a", "b"):
        assert edges(**{k: None}) == EINVAL, k
    assert edges(n_points=0) == EINVAL and edges(n_points=1 << 31) == EINVAL
    assert edges(n_edges=0) == EINVAL and edges(n_edges=-3) == EINVAL and edges(n_edges=1 << 31) == EINVAL
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert edges(radius=r) == EINVAL, r

    n = 12
    tb = L.tohip_tour_bytes(n)
    names = ("nodes", "n", "edge_idx", "closed", "max_moves", "buf", "bytes", "stream")
    base = dict(zip(names, (p, n, None, 0, 4 * n, p, tb, None)))
    plan = lambda **kw: L.tohip_tour_plan(*[kw.get(k, base[k]) for k in names])
    assert plan(nodes=None) == EINVAL and plan(buf=None) == EINVAL
    assert plan(n=1) == EINVAL and plan(n=257) == EINVAL and plan(n=0) == EINVAL and plan(n=-5) == EINVAL
    assert plan(max_moves=-1) == EINVAL
    assert plan(bytes=tb - 1) == ENOSPC and plan(edge_idx=p, bytes=0) == ENOSPC


class _Shard:
    def __init__(self, kind="waypoints", world_size=1, collective=False):
        self.kind, self.world_size, self.collective = kind, world_size, collective


def test_host_refusals_come_before_any_gpu_call():
    from trajectory_optimization_amd.ops import check_tour
    from trajectory_optimization_amd.tools import edge_clearance, plan_tour
    pts = torch.zeros(50, 3)
    P, Q = torch.zeros(6, 3), torch.ones(6, 4)
    assert check_tour(P) == (6, None, 24) and check_tour(P, Q, 0.5, True, 0) == (6, 0.5, 0)
    bad = [
        (dict(poses=[[0, 0, 0], [1, 1, 1]]), "poses must be a floating-point tensor"),
        (dict(poses=torch.zeros(6, 3, dtype=torch.int64)), "poses must be a floating-point tensor"),
        (dict(poses=torch.zeros(6, 2)), r"poses must be a floating-point tensor of shape \(n,3\)"),
        (dict(poses=torch.zeros(6)), r"poses must be a floating-point tensor of shape \(n,3\)"),
        (dict(poses=torch.zeros(1, 3), quats=None), "n >= 2"),
        (dict(poses=torch.zeros(0, 3), quats=None), "n >= 2"),
        (dict(poses=torch.zeros(257, 3), quats=None), "at most 256 nodes, got n = 257"),
        (dict(quats=torch.ones(5, 4)), r"quats must be None or a floating-point tensor of shape \(6,4\)"),
        (dict(quats=torch.ones(6, 3)), "quats must be None"),
        (dict(clearance_radius=0.0), "clearance_radius must be a finite number > 0"),
        (dict(clearance_radius=-0.5), "clearance_radius"), (dict(clearance_radius=float("nan")), "clearance_radius"),
        (dict(clearance_radius=float("inf")), "clearance_radius"), (dict(clearance_radius="wide"), "clearance_radius"),
        (dict(max_moves=-1), "max_moves must be None or an integer >= 0"), (dict(max_moves=2.5), "max_moves"),
        (dict(max_moves=True), "max_moves"), (dict(closed=1), "closed must be True or False"),
    ]
    for kw, msg in bad:
        args = dict(poses=P, quats=Q, clearance_radius=0.5, closed=False, max_moves=None)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            plan_tour(pts, **args)
    for shard in (_Shard("points"), _Shard("waypoints", 2, True)):
        model = types.SimpleNamespace(_cloud=types.SimpleNamespace(n=50), _shard=shard)
        with pytest.raises(ValueError, match="plan_tour: a sharded model"):
            plan_tour(model, P, Q, 0.5)
        with pytest.raises(ValueError, match="edge_clearance: a sharded model"):
            edge_clearance(model, P, P, 0.5)
    with pytest.raises(ValueError, match=r"plan_tour: points must be an \(N,3\) tensor"):
        plan_tour(torch.zeros(50, 2), P, Q, 0.5)
    with pytest.raises(ValueError, match=r"plan_tour: points must be an \(N,3\) tensor"):
        plan_tour("cloud.pcd", P, Q, 0.5)
    with pytest.raises(ValueError, match="points must live on a HIP device"):
        plan_tour(pts, P, Q, 0.5)   # every argument is fine: the last check before the first GPU call
    with pytest.raises(ValueError, match=r"a and b must both be \(E,3\)"):
        edge_clearance(pts, P, torch.zeros(5, 3), 0.5)
    with pytest.raises(ValueError, match=r"a and b must both be \(E,3\)"):
        edge_clearance(pts, torch.zeros(0, 3), torch.zeros(0, 3), 0.5)
    with pytest.raises(ValueError, match="clearance_radius must be a finite number > 0"):
        edge_clearance(pts, P, P, 0.0)
    with pytest.raises(ValueError, match=r"edge_clearance: points must be an \(N,3\) tensor"):
        edge_clearance(torch.zeros(3), P, P, 0.5)


def test_restatement_orders_a_circle():
    from trajectory_optimization_amd import synth
    th = 2 * np.pi * np.arange(16) / 16
    ring = np.stack([5 * np.cos(th), 5 * np.sin(th), np.zeros(16)], axis=1).astype(np.float32)
    for seed in range(4):
        perm = np.random.default_rng(seed).permutation(16)
        r = synth.tour_plan(ring[perm], closed=True)
        assert r["m"] == 16 and not r["unreachable"].any() and r["converged"] and r["order"][0] == 0
        pos = perm[r["order"]]   # positions on the ring in visiting order
        step = np.diff(np.append(pos, pos[0])) % 16
        assert (step == 1).all() or (step == 15).all(), (seed, pos)
        assert r["length_fixed"] <= r["nn_length_fixed"] and r["walk"] == r["order"].tolist() + [0]
        assert r["length_fixed"] == sum(int(r["w"][a, b]) for a, b in zip(r["walk"], r["walk"][1:]))


def test_restatement_sorts_collinear_points():
    from trajectory_optimization_amd import synth
    for seed in range(4):
        rng = np.random.default_rng(seed)
        x = np.concatenate([[-3.0], rng.permutation(40)[:12] * 0.75])   # the start at one end, the others shuffled
        P = (np.float32([[1.0, 2.0, 0.5]]) + x[:, None] * np.float32([[0.6, 0.0, 0.8]])).astype(np.float32)
        r = synth.tour_plan(P, closed=False)
        assert r["order"].tolist() == np.argsort(x, kind="stable").tolist() and r["converged"], seed
        assert synth.tour_plan(P, closed=False, max_moves=0)["moves"] == 0


def test_restatement_visits_the_lower_of_two_identical_nodes_first():
    from trajectory_optimization_amd import synth
    P = np.float32([[0, 0, 0], [4, 0, 0], [2, 1, 0], [2, 1, 0], [4, 0, 0]])
    for closed in (False, True):
        o = synth.tour_plan(P, closed=closed)["order"].tolist()
        assert o.index(2) < o.index(3) and o.index(1) < o.index(4), o
    # a blocked direct leg: the route goes through the node in between, and a node with no open leg is unreachable
    P = np.float32([[0, 0, 0], [2, 0, 0], [1, 1, 0], [9, 9, 9]])
    blocked = np.zeros((4, 4), dtype=bool)
    blocked[0, 1] = blocked[1, 0] = True
    blocked[3, :] = blocked[:, 3] = True
    r = synth.tour_plan(P, blocked)
    assert r["unreachable"].tolist() == [False, False, False, True] and r["order"].tolist() == [0, 2, 1, -1]
    assert r["D"][0, 1] == r["w"][0, 2] + r["w"][2, 1] > r["w"][0, 1] and r["nxt"][0, 1] == 2 and r["nxt"][0, 3] == -1
    assert synth.tour_plan(P, blocked, closed=True)["walk"] == [0, 2, 1, 2, 0]
    P[1] = np.nan   # a node that is not finite has no open edge
    assert synth.tour_plan(P)["unreachable"].tolist() == [False, True, False, False]
