"""The three contracts of tests/test_hip_contracts.py applied to the coarsen entry points, whose reserved `flags` word behind the
stream keeps them out of that file's count: (a) two plain runs agree bit for bit; (b) with every buffer an exact-size arena between
canary bands (tests/guarded_alloc.py) and every `empty` one — the planes a COPY derives — poisoned with 0xFF and again with 0x00 the
outputs stay the same and no canary byte changes; (c) on a side stream behind a sleeping kernel, over input buffers that held another
seed's maps until the copy behind the sleep, they stay the same again.  Everything a case reads on the device is an input the harness
places there — the byte images of the two evidence buffers and the words of the four planes.  The decoys are valid maps of the same
boxes.  Coverage is counted here as it is there."""
import ctypes
import re

import numpy as np
import pytest
import torch

import coarsen_cases as cases
import contract_cases as cc
import reframe_cases as rfc
import test_hip_contracts as hc
from test_hip_contracts import cycles_per_ms, dev, side_stream   # noqa: F401  (module-scoped fixtures)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
ENTRIES = {"tohip_occ_coarsen", "tohip_evid_coarsen"}
NAMES = ("f=2 box an odd offset", "f=3 box into a bigger map", "f=8 box a brick-aligned offset", "f=4 one brick into a bigger map")


def map_inputs(name):
    """seed -> the images of a source and a destination map of the case's two boxes: evidence buffers (header, values, pads) and the
    words of an occupied and a free plane each, as bytes."""
    case = cases.BY_NAME[name]

    def make(seed):
        L_src, L_dst = cases.values(case.src.dims, 0.5, seed=2 * seed), cases.values(case.dst.dims, 0.6, seed=2 * seed + 1)
        out = {"src": synth.evidence_brick_order(L_src), "dst": synth.evidence_brick_order(L_dst)}
        for key, L in (("src", L_src), ("dst", L_dst)):
            occ, free = synth.evidence_planes_ref(L, 0)
            out[key + " occupied"], out[key + " free"] = rfc.plane_words(occ).view(np.uint8), rfc.plane_words(free).view(np.uint8)
        return out
    return make


def _geom(frame):
    from trajectory_optimization_amd import _lib
    return _lib.OccGeom((ctypes.c_float * 3)(*frame.origin), frame.resolution, (ctypes.c_int32 * 3)(*frame.dims))


def _outputs(name):
    case = cases.BY_NAME[name]

    def run(d):
        from trajectory_optimization_amd import ops
        device = d["src"].device
        gs, gd = _geom(case.src), _geom(case.dst)
        p = cases.PARAMS
        header = torch.zeros(256, dtype=torch.uint8, device=device)
        plane = lambda words: torch.cat([header, words])   # noqa: E731  (a grid buffer: header, then the words' bytes)
        src_planes = {k: plane(d["src " + k]) for k in ("occupied", "free")}
        out = {}
        for rule, r in ops.COARSEN_RULES.items():
            for mode in cases.EVID_MODES:
                dst = d["dst"].clone()
                if mode == "copy":   # every word of the planes is written: they may start as anything
                    occ, free = (torch.empty(256 + d["dst occupied"].numel(), dtype=torch.uint8, device=device) for _ in range(2))
                    occ[:256], free[:256] = 0, 0
                else:
                    occ, free = plane(d["dst occupied"]), plane(d["dst free"])
                counts = torch.zeros(4, dtype=torch.int64, device=device)
                ops._map_call0(device, "tohip_evid_coarsen", ops.ptr(d["src"]), d["src"].numel(), ctypes.byref(gs), ops.ptr(dst), dst.numel(),
                               ctypes.byref(gd), ops.ptr(occ), ops.ptr(free), occ.numel(), case.factor, *case.offset, r, ops.XFER_MODES[mode],
                               p["lmin"], p["lmax"], p["threshold"], ops.ptr(counts))
                out.update({f"evid {rule} {mode}": dst, f"evid {rule} {mode} occupied": occ, f"evid {rule} {mode} free": free,
                            f"evid {rule} {mode} counts": counts})
        for rule, r, key, veto in (("any", 0, "occupied", None), ("all", 1, "free", None), ("veto", 0, "free", "occupied")):
            for mode in cases.OCC_MODES:
                dst = torch.empty(256 + d["dst " + key].numel(), dtype=torch.uint8, device=device) if mode == "copy" else plane(d["dst " + key])
                dst[:256] = 0
                counts = torch.zeros(1, dtype=torch.int64, device=device)
                ops._map_call0(device, "tohip_occ_coarsen", ops.ptr(src_planes[key]), src_planes[key].numel(), ctypes.byref(gs),
                               ops.ptr(src_planes[veto]) if veto else None, ops.ptr(dst), dst.numel(), ctypes.byref(gd), case.factor, *case.offset, r,
                               ops.XFER_MODES[mode], ops.ptr(counts))
                out.update({f"plane {rule} {mode}": dst, f"plane {rule} {mode} count": counts})
        out["the source is not modified"] = d["src"].clone()
        return out
    return run


CASES = [cc.Case("coarsen " + name, map_inputs(name), _outputs(name)) for name in NAMES]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):   # noqa: F811
    hc.test_contracts(dev, cycles_per_ms, side_stream, case)


def test_the_cases_have_something_to_lose(dev):   # noqa: F811
    """The plain run is the restatement's; the decoys differ from the inputs, and each decoy input over the real others changes an
    output: a launch on the wrong stream, or one that read a buffer it should not, would be seen."""
    for case, name in zip(CASES, NAMES):
        c = cases.BY_NAME[name]
        assert case.decoys.keys() == case.inputs.keys()
        got = hc._to_host(case.run(hc._on_device(case.inputs, dev)))

        def ref(inp):
            L_src, L_dst = (synth.evidence_from_brick_order(inp[k], f.dims)[0] for k, f in (("src", c.src), ("dst", c.dst)))
            out = {}
            for rule in cases.EVID_RULES:
                for mode in cases.EVID_MODES:
                    want, counts = synth.evid_coarsen_ref(L_src, L_dst, c.factor, c.offset, rule, mode, cases.PARAMS)
                    out[f"evid {rule} {mode}"], out[f"evid {rule} {mode} counts"] = synth.evidence_brick_order(want), counts
            return out
        want = ref(case.inputs)
        for k, v in want.items():
            assert np.array_equal(got[k], v), (name, k)
        assert np.array_equal(got["the source is not modified"], case.inputs["src"])
        for key in ("src", "dst"):
            mixed = ref(dict(case.inputs, **{key: case.decoys[key]}))
            assert any(not np.array_equal(mixed[k], want[k]) for k in want), (name, key)


def test_every_coarsen_entry_point_with_a_stream_is_driven(dev):   # noqa: F811
    from trajectory_optimization_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    entries = {m.group(1) for m in re.finditer(r"\b(tohip_\w+_coarsen)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\b[^;{}]*\)\s*;", text, flags=re.S)}
    assert entries == ENTRIES == {n for n in _lib.SIGNATURES if n.endswith("_coarsen")}
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
