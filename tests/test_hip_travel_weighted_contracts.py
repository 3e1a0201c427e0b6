"""The three contracts of tests/test_hip_contracts.py applied to the weighted travel entries, whose reserved `flags` word behind the
stream keeps them out of that file's count: (a) two plain runs agree bit for bit; (b) with every buffer an exact-size arena between
canary bands (tests/guarded_alloc.py) and every `empty` one — the cost volumes, the worklist's workspace, the layer a gather writes —
poisoned with 0xFF and again with 0x00 the outputs stay the same and no canary byte changes; (c) on a side stream behind a sleeping
kernel, over input buffers that held another seed's scan, layer and table until the copy behind the sleep, they stay the same again.
Coverage is counted here as it is there."""
import ctypes
import re

import numpy as np
import pytest
import torch

import contract_cases as cc
import test_hip_contracts as hc
import travel_cases as tc
from test_hip_contracts import cycles_per_ms, dev, side_stream   # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu
ENTRIES = {"tohip_travel_weights_build", "tohip_travel_build_weighted", "tohip_travel_paths_weighted"}
GRIDS = {"37_5_20": cc.GRID_A, "13_10_7": cc.GRID_B}
RES = cc.RES


def weighted_inputs(dims, S=4):
    """seed -> contract_cases' map inputs (a scan of few returns, so that most of the box is traversable), sources with a NaN row and
    goals as its travel cases make them, a layer of the caller's own and a table."""
    base = cc.map_inputs(dims, fill=0.01)

    def make(seed):
        d = base(seed)
        lo, hi = cc._box(dims)
        rng = np.random.default_rng(1100 + seed)
        src = rng.uniform(lo, hi, (S, 3)).astype(np.float32)
        src[0] = d["sensor"][0]
        src[-1] = (np.nan, 0.0, 0.0)
        d["sources"] = src
        d["goals"] = rng.uniform(lo, hi, (cc.W5, 3)).astype(np.float32)
        d["kappa"] = rng.integers(16, 256, dims).astype(np.uint8)
        d["lut"] = np.sort(rng.integers(16, 256, 7).astype(np.uint8))[::-1].copy()   # dear next to an obstacle, cheaper beyond
        return d
    return make


def _outputs(dims):
    def run(d):
        from trajectory_optimization_amd import ops
        space, field = cc._travel_field_of(d, dims)
        device = field.device
        out = {}
        # the gather, straight through the C entry: the table is read where the harness placed it
        for name, planes, add in (("gather", (None, None), 0), ("gather unknown", (ops.ptr(space.occupied.buf), ops.ptr(space.free.buf)), 120)):
            kappa = torch.empty(int(np.prod(dims)), dtype=torch.uint8, device=device)
            ops._map_call0(device, "tohip_travel_weights_build", ops.ptr(field.buf), field.buf.numel(), *planes, space.occupied.buf.numel(),
                           ctypes.byref(field.geom), ops.ptr(d["lut"]), d["lut"].numel(), add, ops.ptr(kappa), kappa.numel())
            out[name] = kappa
        gathered = ops.TravelWeights(field, lut=d["lut"], space=space, unknown_add=120)
        out["gather through ops"] = gathered.buf.clone()
        own = ops.TravelWeights.from_dense(field, d["kappa"])
        # the single build and its paths
        tf = ops.TravelField(field, tc.RADIUS, d["sources"], max_dist=40 * RES, rounds_per_check=3, weights=own)
        out.update({"seeded": tf.seeded, "dense": tf.dense(), "cost": tf.cost(d["positions"])})
        cc.flat(out, "paths", tf.paths(d["goals"]))
        tf.rebuild(d["sources"][:1])
        out["rebuilt dense"] = tf.dense()
        # the batch over the gathered layer
        src = d["sources"][:3].contiguous()
        tfs = ops.TravelFields(field, tc.RADIUS, src, space=space, rounds_per_check=3, weights=gathered)
        out.update({"batch seeded": tfs.seeded, "batch dense": tfs.dense()})
        gf = torch.arange(d["goals"].shape[0], device=device) % 4 - 1    # -1, 0, 1, 2, -1
        cc.flat(out, "batch paths", tfs.paths(d["goals"], gf))
        return out
    return run


CASES = [cc.Case("travel_weighted_" + name, weighted_inputs(dims), _outputs(dims)) for name, dims in GRIDS.items()]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):   # noqa: F811
    hc.test_contracts(dev, cycles_per_ms, side_stream, case)


def test_the_cases_have_something_to_lose(dev):   # noqa: F811
    """The decoys differ from the inputs, and the decoy layer or table over the real others changes an output: a launch on the wrong
    stream, or one that read a buffer it should not, would be seen.  At kappa = 16 the weighted outputs are the unweighted ones."""
    from trajectory_optimization_amd import ops
    for case, dims in zip(CASES, GRIDS.values()):
        assert case.decoys.keys() == case.inputs.keys()
        want = hc._to_host(case.run(hc._on_device(case.inputs, dev)))
        assert (want["dense"] > 0).sum() > 50 and (want["batch dense"] > 0).sum() > 3, ((want["dense"] > 0).sum(), (want["batch dense"] > 0).sum())
        for key, outputs in (("kappa", ("dense", "rebuilt dense")), ("lut", ("gather", "gather unknown", "batch dense"))):
            mixed = hc._to_host(case.run(hc._on_device(dict(case.inputs, **{key: case.decoys[key]}), dev)))
            for name in outputs:
                assert not np.array_equal(mixed[name], want[name]), (case.name, key, name)
        d = hc._on_device(dict(case.inputs, kappa=np.full(dims, 16, dtype=np.uint8)), dev)
        neutral = hc._to_host(case.run(d))
        space, field = cc._travel_field_of(d, dims)
        plain = ops.TravelField(field, tc.RADIUS, d["sources"], max_dist=40 * RES)
        assert np.array_equal(neutral["dense"], plain.dense().cpu().numpy()) and not np.array_equal(neutral["dense"], want["dense"])
    ops.release_scratch()


def test_every_weighted_entry_point_with_a_stream_is_driven(dev):   # noqa: F811
    from trajectory_optimization_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    entries = {m.group(1) for m in re.finditer(r"\b(tohip_travel_\w*weight\w*)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\b[^;{}]*\)\s*;", text, flags=re.S)}
    assert entries == ENTRIES == {n for n in _lib.SIGNATURES if n.startswith("tohip_travel_") and "weight" in n} - {"tohip_travel_weights_bytes"}
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
