"""The three contracts of tests/test_hip_contracts.py applied to scan registration's entry points, whose reserved `flags` word behind
the stream keeps them out of that file's count: (a) two plain runs agree bit for bit; (b) with every buffer an exact-size arena between
canary bands (tests/guarded_alloc.py) and every `empty` one — the table, the records — poisoned with 0xFF and again with 0x00 the
outputs stay the same and no canary byte changes; (c) on a side stream behind a sleeping kernel, over input buffers that held another
seed's values until the copy behind the sleep, they stay the same again.  Everything a case reads is an input that the harness
places on the device: the map's bytes, the scan, the (3,12) poses and the (3,64) int64 starting state; the calls take them through
`poses12=` and `state=`, so that nothing is copied from the host and nothing synchronises with it between the first call and the
last: prepare, the normal launch and every iteration of the registration are enqueued behind the sleep.  Coverage is counted here as
it is there."""
import re

import numpy as np
import pytest
import torch

import contract_cases as cc
import scan_match_cases as sc
import test_hip_contracts as hc
import test_hip_scan_match_contracts as mc
from test_hip_contracts import cycles_per_ms, dev, side_stream   # noqa: F401  (module-scoped fixtures)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
ITERATIONS, FLOOR, UNKNOWN = 4, mc.FLOOR, mc.UNKNOWN
ENTRIES = {"tohip_scanreg_normal", "tohip_scanreg_step"}
GRIDS = (cc.GRID_A, cc.GRID_B, cc.GRID_1)


def register_inputs(dims, n):
    """scan matching's map bytes and scan, and three starting poses — rotations about all three axes, a translation of the seed's own —
    as the state and the (3,12) rows synth.scan_register_init_ref builds on the host."""
    base = mc.scan_inputs(dims, n)

    def make(seed):
        d = base(seed)
        del d["shifts"]
        t = np.tile(np.asarray(mc.translation(seed), dtype=np.float64), (3, 1))
        d["state"], d["poses12"] = synth.scan_register_init_ref(t, sc.rotations(3))
        return d
    return make


def _register_outputs(d, dims):
    from trajectory_optimization_amd import ops
    dev = d["points"].device
    em = ops.EvidenceMap(cc.ORIGIN, cc.RES, dims, device=dev)
    em.buf[256:].copy_(d["evidence bytes"])
    matcher = ops.ScanMatcher(em, floor=FLOOR, unknown_value=UNKNOWN)
    return {"records": matcher.normal(d["points"], poses12=d["poses12"]),
            "state": matcher.register(d["points"], iterations=ITERATIONS, state=d["state"], poses12=d["poses12"]),
            "the start is not modified": d["state"].clone()}


CASES = [cc.Case(f"scan_register_{'_'.join(map(str, dims))}", register_inputs(dims, n), (lambda dims: lambda d: _register_outputs(d, dims))(dims))
         for dims, n in ((cc.GRID_A, 259), (cc.GRID_B, 259), (cc.GRID_1, 1))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):   # noqa: F811
    hc.test_contracts(dev, cycles_per_ms, side_stream, case)


def _ref(inputs, dims):
    L, _ = synth.evidence_from_brick_order(np.concatenate([np.zeros(256, dtype=np.uint8), inputs["evidence bytes"]]), dims)
    records = synth.scan_normal_ref(L, cc.ORIGIN, cc.RES, inputs["points"], inputs["poses12"], FLOOR, UNKNOWN)
    # the registration continued from the given state and rows: scan_register_ref's loop
    state, poses12 = inputs["state"].copy(), inputs["poses12"].copy()
    for _ in range(ITERATIONS):
        live = np.flatnonzero(state[:, synth.SR_STATUS] == 0)
        rec = np.zeros((len(state), 32), dtype=np.int64)
        if len(live):
            rec[live] = synth.scan_normal_ref(L, cc.ORIGIN, cc.RES, inputs["points"], poses12[live], FLOOR, UNKNOWN)
        state, new = synth.scan_step_ref(rec, state, cc.RES)
        for b, row in enumerate(new):
            if row is not None:
                poses12[b] = row
    return records, state


def test_the_cases_have_something_to_lose(dev):   # noqa: F811
    """The plain run is the restatement's; the decoys differ from the inputs, and each decoy input over the real others changes an
    output: a launch on the wrong stream, or one that read a buffer it should not, would be seen."""
    for case, dims in zip(CASES, GRIDS):
        assert case.decoys.keys() == case.inputs.keys()
        records, state = _ref(case.inputs, dims)
        got = hc._to_host(case.run(hc._on_device(case.inputs, dev)))
        assert np.array_equal(got["records"], records) and np.array_equal(got["state"], state)
        assert np.array_equal(got["the start is not modified"], case.inputs["state"])
        assert (state[:, synth.SR_ITER] >= 1).all()
        if dims == cc.GRID_1:
            assert not np.array_equal(_ref(case.decoys, dims)[1], state)
            continue
        assert (records[:, 28] > 0).all() and (records[:, 28] < 259).all() and (records[:, :28] != 0).all()
        assert (state[:, synth.SR_ITER] == ITERATIONS).any()
        for k in case.inputs:   # one decoy input over the real others: another output
            r2, s2 = _ref(dict(case.inputs, **{k: case.decoys[k]}), dims)
            assert not np.array_equal(s2, state), k
            assert k == "state" or not np.array_equal(r2, records), k
    from trajectory_optimization_amd import ops
    ops.release_scratch()


def test_every_scanreg_entry_point_with_a_stream_is_driven(dev):   # noqa: F811
    from trajectory_optimization_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    entries = {m.group(1) for m in re.finditer(r"\b(tohip_scanreg_\w+)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\b[^;{}]*\)\s*;", text, flags=re.S)}
    assert entries == {n for n in _lib.SIGNATURES if n.startswith("tohip_scanreg_")} == ENTRIES
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
