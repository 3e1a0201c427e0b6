"""The three contracts of tests/test_hip_contracts.py applied to scan matching's four entry points, whose reserved `flags` word behind
the stream keeps them out of that file's count: (a) two plain runs agree bit for bit; (b) with every buffer an exact-size arena between
canary bands (tests/guarded_alloc.py) and every `empty` one poisoned with 0xFF and again with 0x00 the outputs stay the same and no
canary byte changes; (c) on a side stream behind a sleeping kernel, over input buffers that held another seed's values until the copy
behind the sleep, they stay the same again.  Everything a case reads is an input that the harness places on the device: the map's
bytes, written into the map with a plain copy, the scan, the (K,12) poses — built on the host when the case is made — and the (B,3)
int32 shifts; the calls take them through `poses12=` and a device `shifts`, so that nothing is copied from the host and nothing
synchronises with it between the first call and the last: prepare, correlate, best and score are all enqueued behind the sleep.
Coverage is counted here as it is there."""
import re

import numpy as np
import pytest
import torch

import contract_cases as cc
import scan_match_cases as sc
import test_hip_contracts as hc
from test_hip_contracts import cycles_per_ms, dev, side_stream   # noqa: F401  (module-scoped fixtures)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
WINDOW, FLOOR, UNKNOWN = (5, 2, 1), -20, -3
SHIFTS = ((0, 0, 0), (5, -2, 1), (-5, 2, -1))
ENTRIES = {"tohip_scan_prepare", "tohip_scan_score", "tohip_scan_correlate", "tohip_scan_best"}


def translation(seed):
    return (0.01 + 0.05 * seed, -0.02, 0.03)


def poses12(seed):
    """The (3,12) f32 rows of ops.ScanMatcher.poses, on the host: R row-major (f64, rounded once), then t."""
    Rs = np.stack([synth.scan_rotation(q) for q in sc.rotations(3)]).reshape(3, 9)
    return np.concatenate([Rs, np.tile(f32(translation(seed)), (3, 1))], axis=1).astype(f32)


def scan_inputs(dims, n=259):
    """A map of `dims` as its evidence bytes in brick order — values over [-40, 70], a third never observed — and a scan in and around
    its box (one row out of range, one NaN); three poses (rotations about all three axes, a translation of the seed's own) as the
    (3,12) f32 rows the kernels take, and three shifts (the decoys' negated)."""
    def make(seed):
        rng = np.random.default_rng(1400 + seed + dims[0])
        L = rng.integers(-40, 71, dims).astype(np.int64)
        L[rng.random(dims) < 0.33] = synth.EVID_UNKNOWN
        if dims == (1, 1, 1):   # (one voxel: 70 for the inputs, -40 for the decoys)
            L[:] = 70 if seed == 0 else -40
        lo, hi = cc._box(dims)
        pts = rng.uniform(lo - 2 * cc.RES, hi + 2 * cc.RES, (n, 3)).astype(f32)
        if n >= 4:
            pts[1] = (1.0e6, 0.0, 0.0)
            pts[2] = (np.nan, 0.0, 0.0)
        return {"evidence bytes": synth.evidence_brick_order(L)[synth.EVID_HEADER:].copy(), "points": pts, "poses12": poses12(seed),
                "shifts": (np.asarray(SHIFTS, dtype=np.int32) * (1 if seed == 0 else -1))[::1 if seed == 0 else -1].copy()}
    return make


def _scan_outputs(d, dims):
    from trajectory_optimization_amd import ops
    dev = d["points"].device
    em = ops.EvidenceMap(cc.ORIGIN, cc.RES, dims, device=dev)
    em.buf[256:].copy_(d["evidence bytes"])
    matcher = ops.ScanMatcher(em, floor=FLOOR, unknown_value=UNKNOWN)
    scores, used = matcher.correlate(d["points"], None, None, WINDOW, poses12=d["poses12"])
    out = {"table": matcher.table, "scores": scores, "used": used, "best": matcher.best(scores)}
    out["score"], out["score used"], out["inside"], out["known"] = matcher.score(d["points"], None, None, shifts=d["shifts"], poses12=d["poses12"])
    return out


CASES = [cc.Case(f"scan_match_{'_'.join(map(str, dims))}", scan_inputs(dims, n), (lambda dims: lambda d: _scan_outputs(d, dims))(dims))
         for dims, n in ((cc.GRID_A, 259), (cc.GRID_B, 259), (cc.GRID_1, 1))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):   # noqa: F811
    hc.test_contracts(dev, cycles_per_ms, side_stream, case)


def _ref(inputs, dims):
    L, _ = synth.evidence_from_brick_order(np.concatenate([np.zeros(256, dtype=np.uint8), inputs["evidence bytes"]]), dims)
    P = inputs["poses12"]
    return synth.scan_correlate_ref(L, cc.ORIGIN, cc.RES, inputs["points"], P[:, :9].reshape(3, 3, 3), P[0, 9:], WINDOW, FLOOR, UNKNOWN)


def ops_poses(t):
    """ops.ScanMatcher.poses' own host arithmetic, without a device: what a caller would hand over as poses12."""
    from trajectory_optimization_amd import ops
    R = ops.scan_rotations(sc.rotations(3)).reshape(3, 9)
    return np.concatenate([R, np.tile(np.asarray(t, dtype=np.float64).astype(f32), (3, 1))], axis=1)


def test_the_cases_have_something_to_lose():
    """The decoys differ from the inputs and give other scores; the scans have rows in range and rows that are skipped: a launch on the
    wrong stream, or one that read a buffer it should not, would change an output."""
    for case, dims in zip(CASES, (cc.GRID_A, cc.GRID_B, cc.GRID_1)):
        assert case.decoys.keys() == case.inputs.keys()
        scores, used = _ref(case.inputs, dims)
        decoy_scores, _ = _ref(case.decoys, dims)
        assert not np.array_equal(scores, decoy_scores)
        if dims != cc.GRID_1:
            assert (used > 0).all() and (used < 259).all() and len(np.unique(scores)) > 100
            for k in ("points", "poses12"):   # one decoy input over the real others: other scores again
                assert not np.array_equal(_ref(dict(case.inputs, **{k: case.decoys[k]}), dims)[0], scores), k
            # the decoy shifts give other explicit scores
            L, _ = synth.evidence_from_brick_order(np.concatenate([np.zeros(256, dtype=np.uint8), case.inputs["evidence bytes"]]), dims)
            P = case.inputs["poses12"]
            one = lambda sh: [synth.scan_score_ref(L, cc.ORIGIN, cc.RES, case.inputs["points"], P[b, :9].reshape(3, 3), P[b, 9:], sh[b], FLOOR,   # noqa: E731
                                                   UNKNOWN)[0] for b in range(3)]
            assert one(case.inputs["shifts"]) != one(case.decoys["shifts"])
            assert np.array_equal(poses12(0), ops_poses(translation(0)))


def test_every_scan_entry_point_with_a_stream_is_driven(dev):   # noqa: F811
    from trajectory_optimization_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    entries = {m.group(1) for m in re.finditer(r"\b(tohip_scan_\w+)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\b[^;{}]*\)\s*;", text, flags=re.S)}
    assert entries == {n for n in _lib.SIGNATURES if n.startswith("tohip_scan_")} == ENTRIES
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
