"""CPU checks behind tests/test_hip_scan_search_at_size.py, tests/test_hip_scan_register_at_size.py and
tests/test_hip_pose_graph_at_size.py (no GPU): every case of tests/localise_size_cases.py meets the condition it exists for, computed
from the constants read out of the kernels' text and shown on the restatements' own output.  A change of kRelocItems, kOccBlocks,
kScanBlocks, kRegMaxPoses or TO_BLOCK that takes a case out of its regime fails here, by name."""
import numpy as np
import pytest

import localise_size_cases as lc
import map_size_cases as mc
import pose_graph_cases as pc
import scan_match_cases as sc
import scan_match_size_cases as zc
import scan_register_cases as rc
import scan_search_cases as ss

from trajectory_optimization_amd import synth


def test_limits_finds_every_pattern():
    lim = lc.limits()
    assert lim == dict(block=256, wave=64, occ_blocks=2048, scan_blocks=2048, max_points=1 << 22, max_k=256, reloc_items=4096, reloc_block=1024,
                       reloc_capacity=1 << 24, reloc_levels=6, reg_max_poses=256, pg_max=1 << 22, pg_node=27)
    assert lim["reloc_capacity"] == synth.RELOC_MAX_CAPACITY and lim["reloc_levels"] == synth.RELOC_MAX_LEVELS
    assert lim["max_points"] == synth.SCAN_MAX_POINTS and lim["max_k"] == synth.SCAN_MAX_ROTATIONS == lc.A_K
    assert lim["pg_max"] == synth.POSEGRAPH_MAX_NODES and lim["block"] == synth.POSEGRAPH_BLOCK and lim["reg_max_poses"] == lc.B_POSES


# ---- A. relocalisation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [0, 1])
def test_a1_a_share_walks_several_tiles(shape):
    """kRelocItems: n_chunks n_tiles > kRelocItems and ysplit < n_tiles.  With 4 097 points share 0 alone walks two tiles, 0 and 16,
    and tile 16 is one point — in range under every rotation — so the tiles of one share that each hold points in and out of range
    are asserted on the 8 193 points, where every share walks two tiles or three."""
    lim, p = lc.limits(), lc.a1_plan(shape)
    m, n = lc.A1_SHAPES[shape]
    assert p["n_chunks"] == 256 and p["n_chunks"] * p["n_tiles"] > lim["reloc_items"], "kRelocItems"
    assert p["ysplit"] == 16 < p["n_tiles"] == (17, 33)[shape], "kRelocItems / TO_BLOCK"
    assert sorted(set(p["trips"])) == ([1, 2], [2, 3])[shape] and p["trips"][0] == (2, 3)[shape]
    for level in lc.A1_LEVELS[shape]:
        nodes = lc.a1_nodes(shape, level)
        assert len(nodes) == m and (np.bincount(nodes[:, 0], minlength=256) == m // 256).all()
        assert (np.diff(nodes[:, 0]) != 0).all()                                        # no two neighbours of one rotation
    ok = lc.a_in_range(n)
    used = ok.sum(axis=1)
    assert len(np.unique(used)) >= 20 and ok[:, -1].all(), "`used` must differ between rotations"
    mixed = p["mixed"]
    if shape == 0:
        assert mixed[:, :16].all() and not mixed[:, 16].any()
    else:
        shares = [int(sum(mixed[k, part::p["ysplit"]].sum() >= 2 for part in range(p["ysplit"]))) for k in range(256)]
        assert min(shares) == 16                                                        # every share, under every rotation
    for level in lc.A1_LEVELS[shape]:
        bounds, want_used = lc.a1_reference(shape, level)
        assert np.array_equal(want_used, used) and len(np.unique(bounds)) > m // 2


@pytest.mark.parametrize("i", [0, 1])
def test_a2_every_list_of_the_search_has_256_chunks(i):
    lim = lc.limits()
    rec, exhaustive, plans = lc.a2_reference(i)
    window, H = lc.A2_SEARCHES[i]
    assert sorted(plans) == list(range(H + 1)) and rec[7] == 0 and rec[10] == H
    for h, p in plans.items():
        assert p["n_chunks"] >= 256 and p["n_chunks"] * p["n_tiles"] > lim["reloc_items"] and p["ysplit"] < p["n_tiles"], (h, p, "kRelocItems")
        assert max(p["trips"]) >= 2
    assert np.array_equal(rec[:7], exhaustive)
    assert rec[11 + H] == 256 * (2 * window[2] + 1) * -(-(2 * window[0] + 1) // (1 << H)) * -(-(2 * window[1] + 1) // (1 << H))


def test_a3_the_scaling_argument_and_int32():
    """The record of 4 x 64 points is the record of 64 with its score and incumbent times 4, by the restatement itself; the sums of
    2^22 points stay inside int32 before and after - 128 used."""
    lim = lc.limits()
    n = 64 * lc.A3_FACTOR
    assert n == lim["max_points"] == 1 << 22
    assert 255 * n <= lc.INT32_MAX and 128 * n <= lc.INT32_MAX and 127 * n == 532_676_608      # partial and total sums; less 128 used
    assert len(np.unique(lc.a3_cells(), axis=0)) == 64
    for name, _, _ in lc.A3_MAPS:
        one, four = lc.a3_reference(name), lc.a3_reference(name, 4)
        assert np.array_equal(lc.a3_scaled(one, 4), four), name
        assert one[7] == 0 and one[8] == one[5] > 0 and abs(int(one[5])) * lc.A3_FACTOR <= lc.INT32_MAX
        assert tuple(one[1:5]) == (1,) + lc.A3_PLANTED if name == "planted" else one[5] == 127 * 64
    assert lc.a3_reference("planted")[6] == 1 and lc.a3_reference("planted")[5] == 127 * 64
    plan = lc.bound_plan([18, 18, 18], n)                                            # the top list: 3 chunks over 16 384 tiles
    assert lc.a3_reference("planted")[11 + lc.A3_H] == 54 and plan["n_tiles"] == 16384 and plan["ysplit"] == 1366 and min(plan["trips"]) >= 11
    assert -(-n // lim["reloc_block"]) == 4096                                        # trips of a lane of k_reloc_step


def test_a4_the_level_tables_leave_one_pass():
    lim, p = lc.limits(), lc.a4_plan()
    assert p["words"] == 257 * 256 * 9 == 592_128 > lim["occ_blocks"] * lim["block"], "kOccBlocks / TO_BLOCK"
    assert p["passes"] == 2 and p["q"] == 8 and p["bricks"][0] > p["q"] and p["bricks"][1] > p["q"]
    assert all(v != 0 for v in p["partial"]) and lc.A4_DIMS[0] > 64 and lc.A4_DIMS[1] > 64 and lc.A4_H == lim["reloc_levels"]


def test_a5_the_arithmetic_is_the_restatements_record():
    """constant_record reproduces synth.scan_search_ref on the 198 147-leaf case of tests/test_hip_scan_search.py, `evaluated`
    included, and on both of its refusals; then the sizes at the capacity."""
    lim = lc.limits()
    L, pts = np.zeros(lc.A5_DIMS, dtype=np.int64), sc.random_scan(lc.A5_DIMS, lc.A5_N, 9)
    for H, capacity in ((6, 1 << 22), (6, 1024), (2, 1024)):
        want = synth.scan_search_ref(L, sc.ORIGIN, sc.RES, pts, ss.rotation_matrices(3), sc.T, (128, 128, 0), H, capacity=capacity)
        assert np.array_equal(lc.constant_record(3, (128, 128, 0), H, capacity), want), (H, capacity)
    cap = lim["reloc_capacity"]
    leaves = [lc.A5_K * (2 * w[0] + 1) * (2 * w[1] + 1) for w in lc.A5_WINDOWS]
    assert leaves == [16_760_836, 16_777_212, 16_793_604] and leaves[1] <= cap < leaves[2] == cap + 16_388
    recs = [lc.constant_record(lc.A5_K, w, lc.A5_H, cap) for w in lc.A5_WINDOWS]
    assert [int(r[0]) for r in recs] == [1023 * 2047 + 1023, 1023 * 2049 + 1024, -1] and [int(r[6]) for r in recs] == leaves[:2] + [0]
    assert recs[2][7] == (leaves[2] << 3) | 1 and recs[2][11] == leaves[2] and recs[2][12] == 4 * 1025 * 1025
    assert lc.list_passes(leaves[0], cap) == lc.list_passes(leaves[1], cap) == 32, "kOccBlocks"
    assert lc.bound_plan([leaves[1] // 4] * 4, lc.A5_N)["n_chunks"] > 16 * lim["scan_blocks"], "kScanBlocks"     # items a block of the bound launch


def test_what_the_constant_map_search_of_the_small_tests_does_make():
    """tests/test_hip_scan_search.py's constant-map search: one pass of every list kernel (198 147 nodes for 524 288 lanes) and 777
    items for the 2 048 blocks of its bound launch, as its docstring now says."""
    assert lc.list_passes(198_147, 1 << 22) == 1 and lc.bound_plan([66_049] * 3, 64)["items"] == 777 < lc.limits()["scan_blocks"]


def test_l6_the_moved_origin_is_the_largest_grid():
    """The stand-in's origin lies on the 1/8 m lattice, so the same points under the same pose have the same fixed-point coordinates
    in both frames, less the shift — for the search's three rotations, for the registration's starts and for its last trial poses."""
    assert lc.L6_SMALL_DIMS == (96, 96, 64) and tuple(lc.L6_SHIFT) == (1951, 1949, 447)
    assert mc.RES == 0.125 and all(float(np.float32(o)) == o and o % mc.RES == 0.0 for o in lc.L6_SMALL_ORIGIN)
    for q in sc.rotations(zc.S6_K):
        agree, _, ok = lc.l6_frames_agree(synth.scan_rotation(q), zc.s6_translation())
        assert agree and ok.sum() == 3000
    poses, quats = lc.b4_starts()
    _, p12 = synth.scan_register_init_ref(poses, quats)
    _, state = lc.b4_reference()
    F = state.view(np.float64)
    last = [synth.scan_pose12_ref(F[b, synth.SR_TRIAL_T:synth.SR_TRIAL_T + 3], F[b, synth.SR_TRIAL_Q:synth.SR_TRIAL_Q + 4]) for b in range(lc.L6_POSES)]
    for row in list(p12) + last:
        assert lc.l6_frames_agree(row[:9], row[9:12])[0]


def test_a6_the_search_reads_the_last_bricks():
    rec, lists = lc.a6_reference()
    far = lc.a6_far_lookups()
    assert rec[7] == 0 and rec[0] >= 0 and sorted(lists) == list(range(lc.L6_H + 1))
    assert far["beyond"] > 1000 and min(far["last_x"], far["last_y"], far["last_z"]) > 10, far
    # the rim of the level check lies inside the stand-in's margin and reaches the window
    for h in range(1, lc.L6_H + 1):
        off, want = lc.a6_level_check(h)
        assert len(off) == (64 + (1 << h)) ** 2 * (32 + (1 << h)) and off.max() >= 1 << 31 and len(np.unique(want)) > 100


def test_b4_the_rows_reach_the_end_of_the_table():
    poses, quats = lc.b4_starts()
    _, p12 = synth.scan_register_init_ref(poses, quats)
    for row in p12:
        r = lc.b4_rows(row)
        assert r["first_max"] > 1 << 28 and r["first_max"] < 1 << 29 and r["outside"] > 100 and min(r["last"]) > 10, r
    records, state = lc.b4_reference()
    assert (records[:, 28] == 3000).all() and (records[:, 29] < 3000).all() and (records[:, 29] > 0).all()
    assert (state[:, synth.SR_ITER] == lc.L6_ITERATIONS).all() and (state[:, synth.SR_ACCEPTED] >= 1).all()


# ---- B. registration --------------------------------------------------------------------------------------------------------------------

def test_b1_every_block_of_the_step_holds_every_status():
    lim = lc.limits()
    records, state, kind = lc.b1_steps()
    want, want12 = lc.b1_reference()
    assert len(state) == lim["reg_max_poses"] == 4 * lim["wave"], "kRegMaxPoses / TO_WAVE"
    crafted = [0, 3, 0, 1, 1, 2, 4, 0, 0]
    assert [int(v) for v in want[:, synth.SR_STATUS]] == [crafted[k] for k in kind]
    for block in range(4):
        rows = slice(block * lim["wave"], (block + 1) * lim["wave"])
        assert set(kind[rows].tolist()) == set(range(9)) and set(want[rows, synth.SR_STATUS].tolist()) == {0, 1, 2, 3, 4}
    assert len(np.unique(state, axis=0)) == 256
    assert [row is None for row in want12] == [k in (1, 3, 4, 5, 6) for k in kind]


def test_b2_every_block_of_the_normal_kernel_walks_two_tiles():
    lim = lc.limits()
    n = len(rc.room()[1])
    per, fewest = lc.b2_plan(n)
    assert lim["scan_blocks"] // lim["reg_max_poses"] == 8 == per and fewest >= 2, "kScanBlocks / kRegMaxPoses / TO_BLOCK"
    state, rows = lc.b2_frozen_state()
    assert 80 <= len(rows) <= 90 and set(state[rows, synth.SR_STATUS].tolist()) == {1, 2, 3, 4} and (np.diff(rows) <= 3).all()
    plain, frozen, bad = (lc.b2_reference(v) for v in ("plain", "frozen", "bad"))
    assert plain.any(axis=1).all() and len(np.unique(plain, axis=0)) == 256
    live = np.setdiff1d(np.arange(256), rows)
    assert not frozen[rows].any() and np.array_equal(frozen[live], plain[live])
    good = np.setdiff1d(np.arange(256), lc.B2_BAD)
    assert not bad[list(lc.B2_BAD)].any() and np.array_equal(bad[good], plain[good])


def test_b3_twenty_five_iterations_are_the_fewest_with_three_statuses():
    before, at = lc.b3_reference(lc.B3_ITERATIONS - 1), lc.b3_reference()
    count = lambda st: np.bincount(st[:, synth.SR_STATUS], minlength=5).tolist()
    assert count(before)[2:] == [0, 0, 0] and count(before)[0] > 0 and count(before)[1] > 0
    assert count(at)[0] > 50 and count(at)[1] > 50 and count(at)[2] >= 1 and sum(v > 0 for v in count(at)) == 3, count(at)
    assert len(lc.b3_points()) == 1051
    alone = at[list(lc.B3_ALONE), synth.SR_STATUS]
    assert [b // lc.limits()["wave"] for b in lc.B3_ALONE] == [0, 0, 1, 1, 2, 2, 3, 3] and len(set(alone.tolist())) >= 2


# ---- C. the pose graph --------------------------------------------------------------------------------------------------------------------

def test_c1_more_than_256_blocks_of_nodes_and_edges():
    lim, c = lc.limits(), lc.c1_case()
    n, e = len(c["t"]), len(c["ab"])
    assert (n, e) == (70_000, 70_399) and n % lim["block"] and e % lim["block"]
    assert -(-n // lim["block"]) == 274 > 256 and -(-e // lim["block"]) == 275 > 256, "TO_BLOCK"
    (rec, (D, grad, cost), cg), s = lc.c1_reference()
    assert cg["iterations"] == 10 and cg["x"].any() and np.isfinite(cost)
    assert s["status"] == 0 and s["iterations"] == 2 and s["accepted"] == 1 and s["cg_iterations"] == 20 and s["cost"] < s["initial_cost"]


def test_c2_the_hubs_row_is_longer_than_a_block():
    lim, c = lc.limits(), lc.c2_case()
    row_ptr, incident = synth.pose_graph_incidence(c["ab"], len(c["t"]))
    degree = np.diff(row_ptr)
    assert degree[lc.C2_HUB] == 1028 > lim["block"] and row_ptr[lc.C2_HUB] > 0 and np.delete(degree, lc.C2_HUB).max() < 10, "TO_BLOCK"
    mine = incident[row_ptr[lc.C2_HUB]:row_ptr[lc.C2_HUB + 1]]
    rel = mine[c["ab"][mine >> 1, 0] >= 0]
    assert len(rel) == 1025 and (rel & 1).tolist() == [k % 2 for k in range(1025)]          # a and b in turn
    assert (c["ab"][:, 0] < 0).sum() == 3 and (c["ab"][c["ab"][:, 0] < 0, 1] == lc.C2_HUB).all()
    pairs = np.sort(c["ab"][rel >> 1], axis=1)
    assert len(pairs) - len(np.unique(pairs, axis=0)) == lc.C2_DUPLICATES
    (rec, (D, grad, cost), cg), shots = lc.c2_reference()
    assert cg["iterations"] == 10 and sorted(shots) == list(pc.SNAPSHOTS)
    assert shots[30]["iterations"] == 30 and shots[30]["accepted"] >= 5 and shots[30]["cost"] < 1e-3 * shots[1]["cost"]


def test_c3_the_layout_restated_is_the_librarys_at_small_sizes():
    """pg_layout_ref against tohip_posegraph_layout needs no GPU: the sizes of the cases, and the limit."""
    from trajectory_optimization_amd import ops
    for n, e in ((1, 1), (300, 311), (70_000, 70_399), (1 << 22, 1 << 22)):
        got = ops.pose_graph_layout(n, e)
        assert [got[k] for k in ops.POSE_GRAPH_REGIONS] == lc.pg_layout_ref(n, e, ops.POSE_GRAPH_SCALARS), (n, e)
