"""The three contracts of tests/test_hip_contracts.py applied to relocalisation's entry points, whose reserved `flags` word behind the
stream keeps them out of that file's count: (a) two plain runs agree bit for bit; (b) with every buffer an exact-size arena between
canary bands (tests/guarded_alloc.py) and every `empty` one — the level tables, the workspaces, the records — poisoned with 0xFF and
again with 0x00 the outputs stay the same and no canary byte changes; (c) on a side stream behind a sleeping kernel, over input
buffers that held another seed's values until the copy behind the sleep, they stay the same again.  Everything a case reads is an
input that the harness places on the device: the map's bytes, the scan, the (K,12) poses and the (M,4) int32 nodes; the calls take
them through `poses12=` and a device `nodes`, so that nothing is copied from the host and nothing synchronises with it between the
first call and the last: prepare, levels, bounds and the search's launches are all enqueued behind the sleep.  Coverage is counted
here as it is there."""
import re

import numpy as np
import pytest
import torch

import contract_cases as cc
import scan_search_cases as ss
import test_hip_contracts as hc
import test_hip_scan_match_contracts as mc
from test_hip_contracts import cycles_per_ms, dev, side_stream   # noqa: F401  (module-scoped fixtures)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
WINDOW, LEVELS, BOUND_LEVEL, FLOOR, UNKNOWN = (21, 9, 1), 3, 2, mc.FLOOR, mc.UNKNOWN
ENTRIES = {"tohip_reloc_levels", "tohip_reloc_bounds", "tohip_reloc_search"}
GRIDS = (cc.GRID_A, cc.GRID_B, cc.GRID_1)


def search_inputs(dims, n, m):
    """scan matching's inputs — the map's bytes, a scan, three poses — and m explicit nodes of three interleaved rotations in and around
    the box (the decoys': other shifts)."""
    base = mc.scan_inputs(dims, n)

    def make(seed):
        d = base(seed)
        del d["shifts"]
        d["nodes"] = ss.probe_nodes(dims, BOUND_LEVEL, 3, m, seed=seed).astype(np.int32)
        return d
    return make


def _search_outputs(d, dims):
    from trajectory_optimization_amd import ops
    dev = d["points"].device
    em = ops.EvidenceMap(cc.ORIGIN, cc.RES, dims, device=dev)
    em.buf[256:].copy_(d["evidence bytes"])
    matcher = ops.ScanMatcher(em, floor=FLOOR, unknown_value=UNKNOWN)
    out = {"levels": matcher.levels(LEVELS)}
    out["bounds"], out["used"] = matcher.bound(d["points"], d["nodes"], BOUND_LEVEL, poses12=d["poses12"])
    out["record"] = matcher.search(d["points"], None, None, WINDOW, levels=LEVELS, poses12=d["poses12"], capacity=1 << 12)
    out["record without levels"] = matcher.search(d["points"], None, None, (2, 1, 1), levels=0, poses12=d["poses12"], capacity=256)
    return out


CASES = [cc.Case(f"scan_search_{'_'.join(map(str, dims))}", search_inputs(dims, n, m), (lambda dims: lambda d: _search_outputs(d, dims))(dims))
         for dims, n, m in ((cc.GRID_A, 259, 300), (cc.GRID_B, 259, 300), (cc.GRID_1, 1, 7))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):   # noqa: F811
    hc.test_contracts(dev, cycles_per_ms, side_stream, case)


def _ref(inputs, dims):
    L, _ = synth.evidence_from_brick_order(np.concatenate([np.zeros(256, dtype=np.uint8), inputs["evidence bytes"]]), dims)
    P = inputs["poses12"]
    Rs, t = P[:, :9].reshape(3, 3, 3), P[0, 9:]
    bounds, used = synth.scan_bound_ref(L, cc.ORIGIN, cc.RES, inputs["points"], Rs, t, inputs["nodes"], BOUND_LEVEL, FLOOR, UNKNOWN)
    record = synth.scan_search_ref(L, cc.ORIGIN, cc.RES, inputs["points"], Rs, t, WINDOW, LEVELS, FLOOR, UNKNOWN, capacity=1 << 12)
    return bounds, used, record


def test_the_cases_have_something_to_lose(dev):   # noqa: F811
    """The plain run is the restatement's; the decoys differ from the inputs, and each decoy input over the real others changes an
    output: a launch on the wrong stream, or one that read a buffer it should not, would be seen."""
    for case, dims in zip(CASES, GRIDS):
        assert case.decoys.keys() == case.inputs.keys()
        bounds, used, record = _ref(case.inputs, dims)
        got = hc._to_host(case.run(hc._on_device(case.inputs, dev)))
        assert np.array_equal(got["bounds"], bounds) and np.array_equal(got["used"], used) and np.array_equal(got["record"], record)
        assert record[7] == 0 and got["record without levels"][7] == 0 and got["record without levels"][11] == 3 * 5 * 3 * 3
        if dims == cc.GRID_1:
            assert not np.array_equal(_ref(case.decoys, dims)[2], record)
            continue
        assert (used > 0).all() and (used < 259).all() and len(np.unique(bounds)) > 50
        assert record[11] > 256 and (record[11:12 + LEVELS] > 0).all()   # (every level held nodes, the last more than one chunk)
        for k in case.inputs:   # one decoy input over the real others: another output
            b2, u2, r2 = _ref(dict(case.inputs, **{k: case.decoys[k]}), dims)
            assert not np.array_equal(b2, bounds), k
            assert k == "nodes" or not np.array_equal(r2, record), k
    from trajectory_optimization_amd import ops
    ops.release_scratch()


def test_every_reloc_entry_point_with_a_stream_is_driven(dev):   # noqa: F811
    from trajectory_optimization_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    entries = {m.group(1) for m in re.finditer(r"\b(tohip_reloc_\w+)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\b[^;{}]*\)\s*;", text, flags=re.S)}
    assert entries == {n for n in _lib.SIGNATURES if n.startswith("tohip_reloc_")} - {"tohip_reloc_workspace_bytes"} == ENTRIES
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
    assert "tohip_reloc_workspace_bytes" in seen
