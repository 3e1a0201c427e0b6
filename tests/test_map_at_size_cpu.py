"""CPU checks behind tests/test_hip_map_at_size.py (no GPU): the window method — the restatements on a small dense window with shifted
fixed-point ends — equals the full-grid synth references where both are affordable; synth.occ_export_sparse equals occ_export_ref;
the vectorised synth.field_segments_ref equals its definition voxel by voxel over los_fixed's trace; and the conditions the seeded
cases of tests/map_size_cases.py must meet hold on the references."""
import numpy as np
import pytest

import map_size_cases as mc
from map_size_cases import DIMS, N, ORIGIN, RES

from trajectory_optimization_amd import synth

GRIDS = [(5, 6, 3), (64, 64, 32), (1, 1, 1), (70, 9, 33)]   # (those of tests/test_hip_frontier.py's listing)


@pytest.mark.parametrize("dims", GRIDS, ids=str)
def test_sparse_export_equals_the_dense_one(dims):
    bits = np.random.default_rng(dims[0] + 1).random(dims) < 0.3
    for origin, r in ((ORIGIN, RES), ((-20.2, 8188.9, 1e5), 0.1)):
        ijk, centres = synth.occ_export_ref(bits, origin, r)
        rows = np.random.default_rng(1).permutation(np.argwhere(bits))   # (any order in)
        got_ijk, got_centres = synth.occ_export_sparse(rows, dims, origin, r)
        assert got_ijk.dtype == np.int32 and got_centres.dtype == np.float32
        assert np.array_equal(got_ijk, ijk) and np.array_equal(got_centres.view(np.int32), centres.view(np.int32))
    assert synth.occ_export_sparse(np.zeros((0, 3), dtype=np.int64), dims, ORIGIN, RES)[0].shape == (0, 3)


def test_the_window_method_equals_the_full_grid_references():
    dims, win = mc.SMALL_DIMS, mc.SMALL_WINDOW
    c = mc.window_case(dims, win)
    off = c["off"]
    assert off.tolist() == [38, 37, 19]
    occ, skipped = synth.occupancy_ref(c["centres"], ORIGIN, RES, dims)
    assert skipped == 0 and occ.sum() == len(c["distinct"]) and occ[0, 0, 0] and occ[-1, 0, 0] and occ[-1, -1, -1]
    occ[0, 0, 0] = occ[-1, 0, 0] = False
    assert np.array_equal(occ, mc.embed(c["occ"], dims, off))
    occ[0, 0, 0] = occ[-1, 0, 0] = True
    assert np.array_equal(occ[tuple(c["win_ijk"].T)], c["occ"].ravel())
    # the world points are the fixed-point ends, exactly
    for world, q in ((c["a"], c["qa"]), (c["b"], c["qb"])):
        got, ok = synth.occ_fixed(world, ORIGIN, RES)
        assert ok.all() and np.array_equal(got, q)
    # the listing
    ijk, centres = synth.occ_export_ref(occ, ORIGIN, RES)
    got = synth.occ_export_sparse(c["distinct"], dims, ORIGIN, RES)
    assert np.array_equal(got[0], ijk) and np.array_equal(got[1], centres)
    # line of sight
    for skip, want in c["los"].items():
        assert np.array_equal(synth.los_ref(c["a"], c["b"], ORIGIN, RES, occ, skip), want), skip
        assert (want == 0).sum() > 500 and (want == 1).sum() > 500
    # carve
    for max_range, (plane, flags, visits) in c["carve"].items():
        free, skipped, flags_full, visits_full = synth.carve_ref(c["a"], c["b"], ORIGIN, RES, dims, max_range=max_range)
        assert skipped == 0 and visits_full == visits and np.array_equal(flags_full, flags)
        assert np.array_equal(free, mc.embed(plane, dims, off)), max_range
    assert (c["carve"][mc.WINDOW_RANGE][1] == 1).sum() > 500 and (c["carve"][mc.WINDOW_RANGE][1] == 0).sum() > 500
    assert len(c["leaves"]) > 1000 and (c["qb"][c["leaves"]] >= np.asarray(dims) * 256).any(axis=1).all()
    # state and frontier
    free = mc.embed(c["carve"][None][0], dims, off)
    assert np.array_equal(synth.state_ref(c["pos"], ORIGIN, RES, occ, free), c["state"]) and set(c["state"].tolist()) == {0, 1, 2, 3}
    fr = synth.frontier_ref(occ, free, 1)
    assert fr.sum() > 1000 and np.array_equal(np.argwhere(fr), c["frontier"])


def test_the_big_window_case_meets_its_conditions():
    c = mc.window_case(mc.BIG_DIMS, mc.BIG_WINDOW)
    assert c["off"].tolist() == [1983, 1981, 479] and len(c["distinct"]) == int(c["occ"].sum()) + 2
    for world, q in ((c["a"], c["qa"]), (c["b"], c["qb"])):
        got, ok = synth.occ_fixed(world, ORIGIN, RES)
        assert ok.all() and np.array_equal(got, q)   # (256 m x 2048 = 2^19: f32 holds every coordinate)
    centres = synth.occ_export_sparse(c["distinct"], mc.BIG_DIMS, ORIGIN, RES)[1]
    assert np.array_equal(synth.occ_fixed(centres, ORIGIN, RES)[0] >> 8, synth.occ_export_sparse(c["distinct"], mc.BIG_DIMS, ORIGIN, RES)[0])
    for want in c["los"].values():
        assert (want == 0).sum() > 500 and (want == 1).sum() > 500
    assert len(c["frontier"]) > 1000 and set(c["state"].tolist()) == {0, 1, 2, 3}
    assert (c["frontier"] >= c["off"] + 1).all()


def test_field_segments_ref_equals_its_definition_over_the_trace():
    """The minimum over the visited voxels inside dims, the first that attains it: voxel by voxel over los_fixed(trace=True)."""
    dims, origin = (37, 5, 20), (-1.0, 2.0, 0.5)
    rng = np.random.default_rng(3)
    field = synth.field_ref(rng.random(dims) < 0.02, None, 8)
    o, ext = np.asarray(origin), np.asarray(dims) * RES
    a = rng.uniform(o - 3 * RES, o + ext + 3 * RES, (3000, 3)).astype(np.float32)
    b = rng.uniform(o - 3 * RES, o + ext + 3 * RES, (3000, 3)).astype(np.float32)
    a[5], b[6], a[7] = [np.nan, 0, 0], [0, np.inf, 0], o + 4096 * RES
    a[8], b[8] = o - 30 * RES, o - 30 * RES + [5 * RES, 0, 0]   # wholly outside dims
    d2, vox = synth.field_segments_ref(a, b, origin, RES, field)
    qa, oka = synth.occ_fixed(a, origin, RES)
    qb, okb = synth.occ_fixed(b, origin, RES)
    ok = oka & okb
    _, visited = synth.los_fixed(qa[ok], qb[ok], np.zeros(dims, dtype=bool), (0, 0), trace=True)
    nx, ny, nz = dims
    want_d2, want_vox = np.full(3000, -1), np.full(3000, -1)
    for e, vs in zip(np.flatnonzero(ok), visited):
        best, arg = synth.FIELD_SENTINEL, -1
        for (i, j, k) in vs:
            if 0 <= i < nx and 0 <= j < ny and 0 <= k < nz and field[i, j, k] < best:
                best, arg = int(field[i, j, k]), (k * ny + j) * nx + i
        want_d2[e], want_vox[e] = best, arg
    assert d2.dtype == np.int32 == vox.dtype and np.array_equal(d2, want_d2) and np.array_equal(vox, want_vox)
    assert d2[5:8].tolist() == [-1, -1, -1] and (d2[8], vox[8]) == (65535, -1) and (d2 == 65535).sum() > 10 and ((d2 >= 0) & (d2 < 65535)).sum() > 1000


def test_the_cases_past_one_pass_meet_their_conditions():
    assert N > 2048 * 256 and N % 256
    c = mc.insert_case()
    assert 0 < c["skipped"] < N and c["ref"].any() and not c["ref"].all()
    assert not np.isfinite(c["P"][mc.LANES:]).all() and np.isfinite(c["P"][:N - mc.TAIL]).all()
    c = mc.los_case()
    for skip, want in c["want"].items():
        assert (want == 0).sum() >= 0.05 * N and (want == 1).sum() >= 0.05 * N, (skip, np.bincount(want))
        assert np.array_equal(np.flatnonzero(want == 2), c["bad"]) and c["bad"].min() >= mc.LANES
    v = np.abs((synth.occ_fixed(c["B"], ORIGIN, RES)[0] >> 8) - (synth.occ_fixed(c["A"], ORIGIN, RES)[0] >> 8))
    assert v[c["want"][(0, 0)] != 2].max() <= 7   # (at most 6 voxels long: the end voxel is at most 7 away)
    for max_range in (None, 0.3):
        c = mc.carve_case(max_range)
        assert 0.1 <= c["free"].mean() <= 0.9 and c["skipped"] == 4 and c["visits"] > 2 * N
    assert (c["flags"] == 0).sum() > 0.2 * N and (c["flags"] == 1).sum() > 0.2 * N
    m = mc.listing_case()
    assert m["frontier"][1].sum() > m["frontier"][2].sum() > 100_000 and 50 < m["frontier"][6].sum() < 1000
    assert min(np.bincount(mc.state_case()["want"], minlength=4)) > 1000


def test_the_field_cases_hold_the_large_values():
    ref = mc.field_case("corner")
    finite = ref[ref < 65535]
    assert len(finite) == 411_290 and finite.max() == 64_516 and int((finite > 8899).sum()) == 353_158 and int((ref == 65535).sum()) == 260_710
    assert 63 ** 2 + 63 ** 2 + 31 ** 2 == 8899
    need2 = synth.field_need2(mc.NODE_RADIUS, RES)
    assert 8899 < need2 == 9220 <= 254 * 254
    c = mc.field_query_case()
    tail = slice(mc.LANES, None)
    for v in (c["look"], c["d2"]):
        assert ((v[tail] > 8899) & (v[tail] < 65535)).any() and (v[tail] == 65535).any() and (v[tail] == -1).sum() == 4


def test_the_long_rays_cross_dims_and_reach_the_clip():
    c = mc.long_case()
    n = len(c["a"])
    for world, q in ((c["a"], c["qa"]), (c["b"], c["qb"])):
        got, ok = synth.occ_fixed(world, ORIGIN, RES)
        assert ok.all() and np.array_equal(got, q)
    assert n == 256 and c["crosses"].sum() >= n // 2
    steps = np.abs((c["qb"] >> 8) - (c["qa"] >> 8)).sum(axis=1)
    assert steps.max() > 12_000 and np.median(steps) > 6000
    assert int(np.abs(c["qb"] - c["qa"]).max()) * mc.LONG_R > 1 << 40 and mc.LONG_R <= synth.CARVE_MAX_RANGE
    assert synth.carve_range(mc.LONG_RANGE, RES) == mc.LONG_R
    assert (c["carve"][mc.LONG_R][2] == 1).sum() > n // 2 and c["carve"][0][0].sum() > c["carve"][mc.LONG_R][0].sum() > 0
    assert (c["los"] == 0).sum() >= 20 and (c["los"] == 1).sum() >= 20
    assert c["carve"][0][0].shape == DIMS
