"""The three contracts of tests/test_hip_contracts.py applied to the pose-graph entry points, whose reserved `flags` word behind the
stream keeps them out of that file's count: (a) two plain runs agree bit for bit; (b) with every buffer an exact-size arena between
canary bands (tests/guarded_alloc.py) and every `empty` one — the workspace, the result — poisoned with 0xFF and again with 0x00 the
outputs stay the same and no canary byte changes; (c) on a side stream behind a sleeping kernel, over input buffers that held another
seed's graph until the copy behind the sleep, they stay the same again.  Everything a case reads is an input the harness places on
the device — the seven arrays of ops.PoseGraphProblem — so nothing is copied from the host and nothing synchronises with it between the
first launch and the last.  The decoy is a whole, valid graph of the same sizes (other closures, another fixed node, other values):
a launch that ran early would index within bounds.  Coverage is counted here as it is there."""
import re

import numpy as np
import pytest
import torch

import contract_cases as cc
import test_hip_contracts as hc
from test_hip_contracts import cycles_per_ms, dev, side_stream   # noqa: F401  (module-scoped fixtures)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
ITERATIONS, CG = 3, 40
ENTRIES = {"tohip_posegraph_" + n for n in ("start", "linearize", "gather", "step", "optimize", "result")}
SIZES = ((259, 6), (5, 1))          # (nodes, closures): beyond one block of 256, and a ring


def graph_inputs(n, closures):
    """seed -> the seven arrays: a loop of n nodes with `closures` closures, whose places, noise and fixed node are the seed's."""
    def make(seed):
        g = synth.pose_graph_loop(n, 1, 0.02, 0.01, closures, seed=seed)
        ab = g["ab"].copy()
        ab[n - 1:, 0] += seed                                  # the closures start at node 0, 1 .. or at node 1, 2 ..
        row_ptr, incident = synth.pose_graph_incidence(ab, n)
        omega = g["omega"].copy()
        omega[n - 1:] *= 1.0 + 3.0 * seed                      # (the loop's information is the same for every seed: the closures' differs)
        return dict(nodes=np.concatenate([g["t"], g["q"]], axis=1), ab=ab, meas=np.concatenate([g["zt"], g["zq"]], axis=1), omega=omega,
                    row_ptr=row_ptr, incident=incident, free_mask=synth.pose_graph_free_masks(n, [seed], "xyzrpw"))
    return make


def _outputs(d):
    from trajectory_optimization_amd import ops
    p = ops.PoseGraphProblem(**d)
    records = p.start().linearize().region("edges").view(2, p.e, ops.POSE_GRAPH_EDGE)[1].clone()
    node = p.gather().region("nodes").view(2, p.n, 27)[1].clone()
    x = p.step(CG).region("x").clone()
    result = p.start().optimize(ITERATIONS, CG).result()
    return {"records": records, "blocks": node, "x": x, "result": result, "the nodes are not modified": d["nodes"].clone()}


CASES = [cc.Case(f"pose_graph_{n}_{k}", graph_inputs(n, k), _outputs) for n, k in SIZES]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):   # noqa: F811
    hc.test_contracts(dev, cycles_per_ms, side_stream, case)


def _ref(d):
    n = len(d["nodes"])
    t, q, zt, zq = d["nodes"][:, :3], d["nodes"][:, 3:], d["meas"][:, :3], d["meas"][:, 3:]
    rec = synth.pose_graph_linearize_ref(t, q, d["ab"], zt, zq, d["omega"], d["free_mask"])
    D, g, cost = synth.pose_graph_gather_ref(rec, d["ab"], n, d["free_mask"])
    x = synth.pose_graph_cg_ref(D, g, rec, d["ab"], synth.POSEGRAPH_LAMBDA0, d["free_mask"], CG)["x"]
    st = synth.pose_graph_start_ref(t, q)
    for _ in range(ITERATIONS):
        synth.pose_graph_step_ref(st, d["ab"], zt, zq, d["omega"], d["free_mask"], CG)
    return rec, np.concatenate([D, g], axis=1), x, st


def test_the_cases_have_something_to_lose(dev):   # noqa: F811
    """The plain run is the restatement's; the decoys differ from the inputs, and each decoy input over the real others changes the
    result (the graph's structure — ab, row_ptr, incident — as one): a launch on the wrong stream, or one that read a buffer it should
    not, would be seen."""
    from trajectory_optimization_amd import ops
    F = ops.POSE_GRAPH_FIELDS
    for case in CASES:
        assert case.decoys.keys() == case.inputs.keys()
        rec, blocks, x, st = _ref(case.inputs)
        got = hc._to_host(case.run(hc._on_device(case.inputs, dev)))
        n, e = len(case.inputs["nodes"]), len(case.inputs["ab"])
        assert np.array_equal(got["records"], rec) and np.array_equal(got["blocks"], blocks) and np.array_equal(got["x"].reshape(n, 6), x)
        assert np.array_equal(got["the nodes are not modified"], case.inputs["nodes"])
        out = got["result"]
        assert out.shape == (16 + 7 * n + 2 * e,)
        ints = out[:16].view(np.int64)
        assert (ints[F["iterations"]], ints[F["accepted"]], ints[F["cg_iterations"]], ints[F["status"]]) == (ITERATIONS, st["accepted"], st["cg_iterations"], 0)
        assert out[F["cost"]] == st["cost"] and out[F["lam"]] == st["lam"] and st["accepted"] >= 1 and st["cg_iterations"] > 0
        assert np.array_equal(out[16:16 + 7 * n].reshape(n, 7), np.concatenate([st["t"], st["q"]], axis=1))
        assert np.array_equal(out[16 + 7 * n:16 + 7 * n + e], st["rec"][:, 6]) and np.array_equal(out[16 + 7 * n + e:], st["rec"][:, 7])
        assert x.any() and (rec[:, 6] > 0).all()
        for keys in (("nodes",), ("meas",), ("omega",), ("free_mask",), ("ab", "row_ptr", "incident")):
            mixed = dict(case.inputs, **{k: case.decoys[k] for k in keys})
            assert not np.array_equal(_ref(mixed)[3]["t"], st["t"]), keys
    ops.release_scratch()


def test_every_posegraph_entry_point_with_a_stream_is_driven(dev):   # noqa: F811
    from trajectory_optimization_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    entries = {m.group(1) for m in re.finditer(r"\b(tohip_posegraph_\w+)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\b[^;{}]*\)\s*;", text, flags=re.S)}
    assert entries == ENTRIES and entries < {n for n in _lib.SIGNATURES if n.startswith("tohip_posegraph_")}
    real, seen = _lib.lib(), set()
    _lib._lib = hc._Recorder(real, seen)
    try:
        for case in CASES:
            case.run(hc._on_device(case.inputs, dev))
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
        ops.release_scratch()
    assert _lib.lib() is real
    assert entries - seen == set(), sorted(entries - seen)
