"""The three contracts of tests/test_hip_contracts.py applied to the ground layer's two entry points, whose reserved `flags` word
behind the stream keeps them out of that file's count: (a) two plain runs agree bit for bit; (b) with every buffer an exact-size arena
between canary bands (tests/guarded_alloc.py) and every `empty` one poisoned with 0xFF and again with 0x00 the outputs stay the same
and no canary byte changes; (c) on a side stream behind a sleeping kernel, over input buffers that held another seed's values until
the copy behind the sleep, they stay the same again.  The cases write the map's words with plain copies, so that nothing synchronises
with the host before the build and the snap are enqueued.  Coverage is counted here as it is there."""
import re

import numpy as np
import pytest
import torch

import contract_cases as cc
import test_hip_contracts as hc
from test_hip_contracts import cycles_per_ms, dev, side_stream   # noqa: F401  (module-scoped fixtures)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
PLANES = ("support", "ground", "obstacles", "drive")


def ground_inputs(dims, M=259):
    """A map of `dims` as its two planes' words — a solid bottom, a terrace over half of it and random clutter; nine tenths of the
    rest known free — and query positions in and around the box (one out of range, one NaN, one on a voxel face)."""
    def make(seed):
        rng = np.random.default_rng(1300 + seed + dims[0])
        occ = rng.random(dims) < 0.04
        occ[:, :, 0] = True
        occ[dims[0] // 2:, :, :min(2 + seed, dims[2])] = True
        free = (rng.random(dims) < 0.9) & ~occ
        if dims == (1, 1, 1):   # (one voxel: occupied for the inputs, free for the decoys)
            occ[:], free[:] = seed == 0, seed != 0
        lo, hi = cc._box(dims)
        pos = rng.uniform(lo - 3 * cc.RES, hi + 3 * cc.RES, (M, 3)).astype(f32)
        if M >= 4:
            pos[1] = (1.0e6, 0.0, 0.0)
            pos[2] = (np.nan, 0.0, 0.0)
            pos[3] = np.asarray(cc.ORIGIN, dtype=f32) + f32(cc.RES) * (np.asarray(dims) // 2).astype(f32)
        return {"occupied words": synth.ground_pack(occ).view(np.int32), "free words": synth.ground_pack(free).view(np.int32), "positions": pos}
    return make


def _ground_outputs(d, dims):
    from trajectory_optimization_amd import ops
    dev = d["positions"].device
    grid = ops.OccupancyGrid(cc.ORIGIN, cc.RES, dims, device=dev)
    space = ops.SpaceMap(grid)
    grid.buf[256:].view(torch.int32).copy_(d["occupied words"])
    space.free.buf[256:].view(torch.int32).copy_(d["free words"])
    out = {}
    for unknown in ("free", "obstacle"):
        layer = ops.GroundLayer(space, H=3, step=1, unknown=unknown)
        for k in PLANES:
            out[f"{unknown}.{k}"] = getattr(layer, k).buf   # (the whole buffer: header, words, pad bits)
        out[f"{unknown}.standing"], out[f"{unknown}.drop"] = layer.snap(d["positions"], 4)
    return out


CASES = [cc.Case(f"ground_{'_'.join(map(str, dims))}", ground_inputs(dims, M), (lambda dims: lambda d: _ground_outputs(d, dims))(dims))
         for dims, M in ((cc.GRID_A, 259), (cc.GRID_B, 259), (cc.GRID_1, 1))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):   # noqa: F811
    hc.test_contracts(dev, cycles_per_ms, side_stream, case)


def test_the_cases_have_something_to_lose():
    """The decoys differ from the inputs, the larger maps have ground and a row that snaps: a build that ran on the wrong stream, or
    read a buffer it should not, would change an output."""
    for case, dims in zip(CASES[:2], (cc.GRID_A, cc.GRID_B)):
        assert case.decoys.keys() == case.inputs.keys()
        nb = [(n + k - 1) // k for n, k in zip(dims, (4, 4, 2))]
        words = case.inputs["occupied words"].view(np.uint32).reshape(nb[2], nb[1], nb[0])
        occ = np.zeros(dims, dtype=bool)
        for x, y, z in np.ndindex(*dims):
            occ[x, y, z] = (words[z >> 1, y >> 2, x >> 2] >> ((x & 3) | (y & 3) << 2 | (z & 1) << 4)) & 1
        ref = synth.ground_ref(occ, None, 3, 1)
        assert ref["ground"].any() and ref["drive"].any()
        _, drop = synth.ground_snap_ref(case.inputs["positions"], cc.ORIGIN, cc.RES, ref["ground"], ref["drive"], 4)
        assert (drop >= 0).any() and (drop == -1).any() and (drop == -2).any()


def test_every_ground_entry_point_with_a_stream_is_driven(dev):   # noqa: F811
    from trajectory_optimization_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    entries = {m.group(1) for m in re.finditer(r"\b(tohip_ground_\w+)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\b[^;{}]*\)\s*;", text, flags=re.S)}
    assert entries == {n for n in _lib.SIGNATURES if n.startswith("tohip_ground_")} == {"tohip_ground_build", "tohip_ground_snap"}
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
