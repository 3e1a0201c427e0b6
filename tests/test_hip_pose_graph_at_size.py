"""Pose-graph optimisation on the GPU at size (posegraph_kernels.hip): 274 blocks of nodes and 275 of edges — pg_sum's serial pass over
more than 256 partials — a hub whose CSR row of 1 028 entries is longer than a block, and the limit of 2^22 nodes and edges in the
size arithmetic.  Every stage equals the restatement of synth with np.array_equal, as in tests/test_hip_pose_graph.py, on the graphs
of tests/localise_size_cases.py, whose conditions tests/test_localise_at_size_cpu.py checks without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import localise_size_cases as lc
import pose_graph_cases as pc

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _graph(c, dev):
    from trajectory_optimization_amd import ops
    g = ops.PoseGraph(c["t"], c["q"], fixed=c["fixed"], device=dev)
    return g.add_edges(c["ab"][:, 0], c["ab"][:, 1], c["zt"], c["zq"], c["omega"])


def _normalised(q):
    return q / np.sqrt((q * q).sum(axis=1, keepdims=True))


def _same_result(r, s, what):
    """A PoseGraphResult against a state of the restatement."""
    assert r.status == synth.POSEGRAPH_STATUS[s["status"]], what
    assert (r.iterations, r.accepted, r.cg_iterations) == (s["iterations"], s["accepted"], s["cg_iterations"]), what
    assert np.array_equal(r.poses, s["t"]) and np.array_equal(r.quats, _normalised(s["q"])), what
    assert r.cost == s["cost"] and r.initial_cost == s["initial_cost"] and r.lam == s["lam"], what
    assert np.array_equal(r.chi2, s["rec"][:, synth.PG_S]) and np.array_equal(r.weights, s["rec"][:, synth.PG_W]), what


def _stages(c, dev, stages):
    """linearize, gradient and one conjugate-gradient solve of 10 iterations against the restatement's."""
    rec, (D, grad, cost), cg = stages
    g = _graph(c, dev)
    got = g.linearize()
    assert got.shape == rec.shape == (len(c["ab"]), 100) and np.array_equal(got, rec)
    gD, gg, gcost = g.gradient()
    assert np.array_equal(gD, D) and np.array_equal(gg, grad) and gcost == cost
    out = g.cg(cg_iterations=10)
    assert out["status"] == "RUNNING" and out["iterations"] == cg["iterations"] and out["small"] == cg["small"]
    assert np.array_equal(out["x"], cg["x"])
    return g


def test_c1_more_than_256_blocks(dev):
    """70 000 nodes, 70 399 edges: the cost's, the dot products' and the flags' partials number 274 and 275."""
    c = lc.c1_case()
    stages, s = lc.c1_reference()
    g = _stages(c, dev, stages)
    for run in range(2):
        _same_result(g.optimize(iterations=2, cg_iterations=10), s, ("70000 nodes", run))


def test_c2_a_hub_beyond_a_block(dev):
    """Node 7 with 1 025 relative edges, as a and as b in turn, 40 of them duplicates, and three absolute edges: k_pg_gather and
    k_pg_spmv read a CSR row of 1 028 entries."""
    c = lc.c2_case()
    stages, shots = lc.c2_reference()
    g = _stages(c, dev, stages)
    for iterations in pc.SNAPSHOTS:
        _same_result(g.optimize(iterations=iterations, cg_iterations=c["cg_iterations"]), shots[iterations], ("hub", iterations))
    assert np.array_equal(g.t, c["t"]) and np.array_equal(g.q, c["q"])


def test_c3_the_limit_of_two_to_the_22(dev):
    """Size arithmetic only: 2^22 nodes and edges are taken by tohip_posegraph_workspace_bytes, tohip_posegraph_layout and
    ops.PoseGraph, 2^22 + 1 of either refused by name; the layout's offsets are pg_layout restated (lc.pg_layout_ref)."""
    from trajectory_optimization_amd import _lib, ops
    lib, top = _lib.lib(), lc.limits()["pg_max"]
    assert top == ops.POSE_GRAPH_MAX_NODES == ops.POSE_GRAPH_MAX_EDGES == 1 << 22
    want = lc.pg_layout_ref(top, top, ops.POSE_GRAPH_SCALARS)
    got = ops.pose_graph_layout(top, top)
    assert [got[k] for k in ops.POSE_GRAPH_REGIONS] == want and lib.tohip_posegraph_workspace_bytes(top, top, 0) == 8 * want[-1]
    for n, e in ((top - 1, 3), (257, top), (top, 1)):
        assert [ops.pose_graph_layout(n, e)[k] for k in ops.POSE_GRAPH_REGIONS] == lc.pg_layout_ref(n, e, ops.POSE_GRAPH_SCALARS)
    off = (ctypes.c_int64 * len(ops.POSE_GRAPH_REGIONS))()
    EINVAL = _lib.CONSTANTS["TOHIP_EINVAL"]
    for n, e in ((top + 1, top), (top, top + 1), (0, 1), (1, 0)):
        assert lib.tohip_posegraph_workspace_bytes(n, e, 0) == 0 and lib.tohip_posegraph_layout(n, e, off, 0) == EINVAL
        with pytest.raises(RuntimeError, match="tohip_posegraph_layout"):
            ops.pose_graph_layout(n, e)
    q = np.tile(np.asarray([1.0, 0.0, 0.0, 0.0]), (top + 1, 1))
    g = ops.PoseGraph(np.zeros((top, 3)), q[:top], device=dev)
    assert g.n_nodes == top
    with pytest.raises(ValueError, match=r"the nodes must number 1 \.\. 2\^22, got 4194305"):
        ops.PoseGraph(np.zeros((top + 1, 3)), q, device=dev)
    with pytest.raises(ValueError, match=r"the nodes must number 1 \.\. 2\^22, got 4194305"):
        ops.check_pose_graph(top + 1, np.asarray([[0, 1]], dtype=np.int32), fixed=(0,))
    with pytest.raises(ValueError, match=r"1 <= E <= 2\^22"):
        ops.check_pose_graph(2, np.zeros((top + 1, 2), dtype=np.int32), fixed=(0,))
