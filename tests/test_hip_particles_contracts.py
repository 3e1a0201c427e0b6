"""The three contracts of tests/test_hip_contracts.py applied to the particle filter's seven entry points, whose reserved `flags` word
behind the stream keeps them out of that file's count, through contract_cases / guarded_alloc exactly as
tests/test_hip_scan_match_contracts.py applies them to scan matching: (a) two plain runs agree bit for bit; (b) with every buffer an
exact-size arena between canary bands and every `empty` one poisoned with 0xFF and again with 0x00 the outputs stay the same and no
canary byte changes; (c) on a side stream behind a sleeping kernel, over input buffers that held another seed's values until the copy
behind the sleep, they stay the same again.  What a case reads from the device — the map's bytes, the scan, the free positions of a
global start — the harness places there; priors, motions, sigmas and the attitude are host numbers that travel by value.  The filter
reads nothing back between its first call and its last."""
import re

import numpy as np
import pytest
import torch

import contract_cases as cc
import particle_cases as pc
import test_hip_contracts as hc
from test_hip_contracts import cycles_per_ms, dev, side_stream   # noqa: F401  (module-scoped fixtures)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
FLOOR, UNKNOWN, BETA_Q, SEED = -20, -3, 300, (7 << 32) | 11
SIGMA, DELTA, MOTION_SIGMA = [300.0, 250.0, 120.0, 700.0], [200, -90, 30, 500], [40.0, 40.0, 20.0, 60.0]
ENTRIES = {"tohip_mcl_seed_gaussian", "tohip_mcl_seed_positions", "tohip_mcl_predict", "tohip_mcl_poses", "tohip_mcl_weigh", "tohip_mcl_weights",
           "tohip_mcl_resample_systematic"}


def prior(dims):
    return [128 * dims[0], 128 * dims[1], 128 * dims[2], 1000]


def moved(dims, n):
    """The particles after the seeding and the one motion update of every case: they depend on no device input."""
    state = synth.mcl_seed_gaussian_ref(n, prior(dims), synth.mcl_sigma_q8(SIGMA), SEED, 0)
    return synth.mcl_predict_ref(state, DELTA, synth.mcl_sigma_q8(MOTION_SIGMA), SEED, 1)


def particle_inputs(dims, n_points):
    """A map of `dims` as its evidence bytes in brick order — values over [-40, 70], a third never observed — a scan in and around its
    box (one row out of range, one NaN) and free positions for a global start."""
    def make(seed):
        rng = np.random.default_rng(1500 + seed + dims[0])
        L = rng.integers(-40, 71, dims).astype(np.int64)
        L[rng.random(dims) < 0.33] = synth.EVID_UNKNOWN
        if dims == (1, 1, 1):   # (one voxel: 70 for the inputs, -40 for the decoys)
            L[:] = 70 if seed == 0 else -40
        lo, hi = cc._box(dims)
        pts = (rng.uniform(lo - 2 * cc.RES, hi + 2 * cc.RES, (n_points, 3)) - 0.5 * (lo + hi)).astype(f32)   # sensor frame: about the prior
        if n_points >= 4:
            pts[1] = (1.0e6, 0.0, 0.0)
            pts[2] = (np.nan, 0.0, 0.0)
        if dims == (1, 1, 1):   # (one particle, one point: the point the particle's pose takes to the voxel's centre; the decoy three voxels off)
            T = synth.mcl_poses_ref(moved(dims, 1), cc.ORIGIN, cc.RES, pc.attitude())[0].astype(np.float64)
            pts[0] = T[:9].reshape(3, 3).T @ (0.5 * (lo + hi) + 3 * cc.RES * seed - T[9:])
        positions = rng.uniform(lo, hi, (max(1, n_points // 7), 3)).astype(f32)
        if dims == (1, 1, 1) and seed == 1:   # (the decoy's one position: in the voxel before the only one)
            positions -= f32(cc.RES)
        return {"evidence bytes": synth.evidence_brick_order(L)[synth.EVID_HEADER:].copy(), "points": pts, "positions": positions}
    return make


def _outputs(d, dims, n):
    from trajectory_optimization_amd import ops
    dev = d["points"].device
    em = ops.EvidenceMap(cc.ORIGIN, cc.RES, dims, device=dev)
    em.buf[256:].copy_(d["evidence bytes"])
    pf = ops.ParticleFilter(em, n, seed=SEED, beta_q=BETA_Q, floor=FLOOR, unknown_value=UNKNOWN)
    out = {"global start": pf.seed_positions(d["positions"]).state.clone()}
    out["seeded"] = pf.seed_gaussian(prior(dims), None, SIGMA[:3], SIGMA[3], units="state").state.clone()
    out["moved"] = pf.predict(DELTA, MOTION_SIGMA, units="state").state.clone()
    A = pc.attitude()
    out["poses12"] = pf.poses12(A)
    pf.weigh(d["points"], A)
    out["scores"], out["log-weights"], out["weights"], out["record"] = pf.scores.clone(), pf.log_weight.clone(), pf.weights().clone(), pf.record.clone()
    pf.resample(1.0)
    out["state"], out["ancestors"], out["log-weights after"], out["cumulative"] = pf.state, pf.ancestors, pf.log_weight, pf._cumulative
    out["record after"] = pf.record
    return out


SHAPES = ((cc.GRID_A, 259, 259), (cc.GRID_B, 70, 1300), (cc.GRID_1, 1, 1))
CASES = [cc.Case(f"particles_{'_'.join(map(str, dims))}", particle_inputs(dims, p), (lambda dims, n: lambda d: _outputs(d, dims, n))(dims, n))
         for dims, p, n in SHAPES]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contracts(dev, cycles_per_ms, side_stream, case):   # noqa: F811
    hc.test_contracts(dev, cycles_per_ms, side_stream, case)


def _ref(inputs, dims, n):
    L, _ = synth.evidence_from_brick_order(np.concatenate([np.zeros(256, dtype=np.uint8), inputs["evidence bytes"]]), dims)
    start = synth.mcl_seed_positions_ref(n, inputs["positions"], cc.ORIGIN, cc.RES, True, SEED, 0)
    state = moved(dims, n)
    score, used, known = synth.mcl_weigh_ref(L, cc.ORIGIN, cc.RES, inputs["points"], state, pc.attitude(), FLOOR, UNKNOWN)
    return start, state, score, used, known


def test_the_cases_have_something_to_lose():
    """The decoys differ from the inputs and give other starts and other scores; the scans have rows in range and rows that are
    skipped: a launch on the wrong stream, or one that read a buffer it should not, would change an output."""
    for case, (dims, p, n) in zip(CASES, SHAPES):
        assert case.decoys.keys() == case.inputs.keys()
        start, state, score, used, known = _ref(case.inputs, dims, n)
        for k in case.inputs:   # one decoy input over the real others: another start or other scores
            other = _ref(dict(case.inputs, **{k: case.decoys[k]}), dims, n)
            assert not (np.array_equal(other[0], start) and np.array_equal(other[2], score)), (case.name, k)
        if dims != cc.GRID_1:
            assert (used > 0).all() and (used < p).all() and (known < used).any() and len(np.unique(score)) > n // 8


def test_the_contract_cases_match_the_restatement(dev):   # noqa: F811
    for case, (dims, p, n) in zip(CASES, SHAPES):
        out = case.run(hc._on_device(case.inputs, dev))
        start, state, score, used, known = _ref(case.inputs, dims, n)
        assert np.array_equal(out["global start"].cpu().numpy(), start) and np.array_equal(out["moved"].cpu().numpy(), state)
        assert np.array_equal(out["scores"].cpu().numpy(), np.stack([score, used, known]))
        lw, w, rec = synth.mcl_weights_ref(state, np.zeros(n, dtype=np.int64), score, BETA_Q, 0.5 * n, used, known)
        assert np.array_equal(out["weights"].cpu().numpy(), w) and np.array_equal(out["record"].cpu().numpy(), rec)
        new_state, new_lw, anc, verdict = synth.mcl_resample_ref(state, lw, w, 1.0 * n, SEED, 1)
        assert np.array_equal(out["state"].cpu().numpy(), new_state) and np.array_equal(out["ancestors"].cpu().numpy(), anc)
        assert out["record after"].cpu().numpy()[11] == verdict


def test_every_particle_entry_point_with_a_stream_is_driven(dev):   # noqa: F811
    from trajectory_optimization_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    entries = {m.group(1) for m in re.finditer(r"\b(tohip_mcl_\w+)\s*\(([^;{}]*?)\bvoid\s*\*\s*stream\b[^;{}]*\)\s*;", text, flags=re.S)}
    assert entries == {n for n in _lib.SIGNATURES if n.startswith("tohip_mcl_")} == ENTRIES
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
