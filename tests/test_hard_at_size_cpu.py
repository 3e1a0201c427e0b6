"""CPU checks behind tests/test_hip_hard_at_size.py (no GPU): the sizes of tests/hard_size_cases.py reach the paths they are named for
by the thresholds read from the kernels' text; the seeded and hand-built inputs meet the conditions the GPU tests rely on, shown on
the references' own output; and the references themselves are held to known answers — the z-buffer oracle's tie rule against its
opposite, the new oracle.occlusion_masks(method="zbuffer") on a two-wall scene, occ_row_ref on hand-made rows."""
import numpy as np
import pytest

import hard_size_cases as hc
from hard_size_cases import IH, IW, K


# ---------------------------------------------------------------------------------------------------------------- A. the frustum cull

def test_the_frustum_sizes_reach_their_paths():
    lim = hc.limits()
    tile, two, waves = lim["cull_tile"], lim["two_launch_tiles"], lim["block"] // lim["wave"]
    per_round = 4 * lim["scan_threads"]                      # k_scan_tiles: four counts per thread and round
    strided = lim["write_blocks"] * waves                    # k_frustum_write: a wave per tile, the grid capped
    assert [(n, hc.tiles(n)) for n, t, _, _ in hc.FRUSTUM_SIZES] == [(n, t) for n, t, _, _ in hc.FRUSTUM_SIZES]
    (n0, t0, _, _), (n1, t1, _, _), (n2, t2, _, _), (n3, t3, _, _), (n4, t4, _, _) = hc.FRUSTUM_SIZES
    assert t0 < two and 64 * 22 < t0 <= 64 * 23              # the last wave adds up to 23 counts per lane
    assert t1 == two and n1 == two * tile                    # the last size of the two-launch path, no ragged tile
    assert t2 == two + 1 and n2 == n1 + 1 and t2 <= per_round and t2 % 4 == 1
    assert per_round < t3 <= 2 * per_round and t3 % 4 == 2 and n3 % tile
    assert t4 > strided and t4 - strided < waves + 1         # the smallest number of tiles with a second trip, its last tile ragged
    assert n4 % tile == 1 and n4 < 2 ** 31


@pytest.mark.parametrize("n", [n for n, _, _, inputs in hc.FRUSTUM_SIZES if "pattern" in inputs])
def test_the_pattern_has_every_kind_of_tile(n):
    tile = hc.limits()["cull_tile"]
    kind = hc.pattern_kind(n)
    assert kind.dtype == np.uint8 and set(np.unique(kind).tolist()) == {0, 1, 2}
    nt = hc.tiles(n)
    kept = np.zeros(nt * tile, bool)
    kept[:n] = kind == 0
    per_tile = kept.reshape(nt, tile)
    counts = per_tile.sum(axis=1)
    full = min(tile, n - (nt - 1) * tile)
    assert (counts[:-1] == 0).any() and (counts[:-1] == tile).any()
    only = np.flatnonzero(counts[:-1] == 1)
    assert per_tile[only, 0].any() and per_tile[only, tile - 1].any()         # its only kept point the first row / the last row
    assert ((counts[:-1] > 0) & (counts[:-1] < tile)).sum() > nt // 4
    assert kind[-1] == 0 and counts[-1] <= full
    per_round = 4 * hc.limits()["scan_threads"]
    if nt > per_round:   # counts on both sides of the scan's round boundary, and the carry is not zero
        assert counts[:per_round].sum() > 0 and counts[per_round:].sum() > 0
    # the three kinds are what the oracle says of them
    from oracle import oracle
    d, f = oracle.frustum_masks(np.ascontiguousarray(hc.KIND_ROWS.T), K, IW, IH, *hc.FRUSTUM_LIMITS)
    assert d.tolist() == [True, False, True] and f.tolist() == [True, True, False]


def test_the_device_builder_equals_the_host_one():
    import torch
    n = 2_097_153
    assert np.array_equal(hc.pattern_kind_torch(n, torch.device("cpu")).numpy(), hc.pattern_kind(n))
    p = hc.pattern_points(np.array([0, 1, 2, 0], np.uint8))
    assert p.shape == (3, 4) and p.dtype == np.float32 and p[:, 1].tolist() == [0.0, 0.0, 20.0] and p[:, 2].tolist() == [100.0, 0.0, 5.0]


@pytest.mark.parametrize("n", [n for n, _, _, inputs in hc.FRUSTUM_SIZES if "real" in inputs])
def test_the_real_predicate_case_keeps_points_in_every_part(n):
    c = hc.real_frustum_case(n)
    tile, per_round = hc.limits()["cull_tile"], 4 * hc.limits()["scan_threads"]
    assert 10_000 < len(c["idx"]) < n // 10 and c["dist"].sum() > len(c["idx"]) and c["fov"].sum() > len(c["idx"])
    t = c["idx"] // tile
    assert len(np.unique(t)) > hc.tiles(n) // 2 and t.max() >= hc.tiles(n) - 2
    if hc.tiles(n) > per_round:
        assert (t < per_round).any() and (t >= per_round).any()


# ------------------------------------------------------------------------------------------------------------ B. the cull of many poses

def test_the_cull_cases_reach_the_second_rounds():
    lim = hc.limits()
    c = hc.cull_case("scan")
    n, W = len(c["pts"]), len(c["poses"])
    assert (n, W) == (300_007, 3) and lim["block"] < hc.tiles(n) == 293        # k_cull_wps_scan: TO_BLOCK counts a round
    counts = [len(c["ref"][w][0]) for w in range(W)]
    assert counts[1] == 0 and min(counts[0], counts[2]) > 10_000
    for w in (0, 2):   # kept points on both sides of the round boundary
        t = c["ref"][w][0] // lim["cull_tile"]
        assert (t < lim["block"]).sum() > 1000 and (t >= lim["block"]).sum() > 1000
    c = hc.cull_case("offsets")
    n, W = len(c["pts"]), len(c["poses"])
    assert (n, W) == (3_000, 300) and lim["block"] < W                          # k_cull_wps_offsets: TO_BLOCK poses a round
    counts = np.array([len(c["ref"][w][0]) for w in range(W)])
    assert np.flatnonzero(counts == 0).tolist() == [0, 255, 256, 299] == list(c["away"])
    assert counts[:lim["block"]].sum() > 0 and counts[lim["block"]:].sum() > 0


def test_the_grid_case_goes_past_the_grid_limit():
    c = hc.grid_case()
    cap = hc.limits()["max_poses"]
    assert cap == 65_535 and len(c["poses"]) == hc.GRID_POSES == cap + 2 and len(c["pts"]) == 8
    assert hc.GRID_LOOKED_AT == (0, cap - 1, cap, cap + 1)
    for w in hc.GRID_LOOKED_AT:
        assert 0 < len(c["ref"][w][0]) < 8, w
    assert not np.array_equal(c["ref"][0][0], c["ref"][cap][0])


# ---------------------------------------------------------------------------------------------------------------------- C. the z-buffer

def _pixels(owner, rows):
    return int(np.isin(owner, rows).sum())


def test_the_edge_scene_has_every_edge():
    v, rows = hc.edge_scene()
    img, owner, own = hc.owners(v)
    Z = v[:, 2]
    H, W = hc.SMALL_H, hc.SMALL_W
    # ties: identical depth bits, overlapping discs, and the pixels both cover go to the smaller row number
    for label in ("tie_ascending", "tie_descending", "tie_triple"):
        r = rows[label]
        assert len(set(Z[r].view(np.int32).tolist())) == 1
        alone = [hc.owners(v[[k]])[1] >= 0 for k in r]
        both = np.logical_and.reduce(alone[:2])
        assert both.sum() >= 2 and (owner[both] == r[0]).all(), label
        assert all(k in own for k in r), label                    # each still owns what the lower-numbered ones leave
    assert v[rows["tie_ascending"][0], 0] < v[rows["tie_ascending"][1], 0] and v[rows["tie_descending"][0], 0] > v[rows["tie_descending"][1], 0]
    everyone = np.logical_and.reduce([hc.owners(v[[k]])[1] >= 0 for k in rows["tie_triple"]])
    assert everyone.any() and (owner[everyone] == rows["tie_triple"][0]).all()
    a, b = rows["duplicate"]
    assert np.array_equal(v[a].view(np.int32), v[b].view(np.int32)) and a in own and b not in own
    assert rows["behind"][0] not in own and _pixels(hc.owners(v[rows["behind"]])[1], [0]) > 0
    # the clip planes: on them owns, one ulp outside does not
    assert Z[rows["on_znear"][0]] == np.float32(hc.PARAMS["znear"]) and Z[rows["on_zfar"][0]] == np.float32(hc.PARAMS["zfar"])
    assert rows["on_znear"][0] in own and rows["on_zfar"][0] in own
    assert Z[rows["before_znear"][0]] == np.nextafter(np.float32(1.0), np.float32(0.0)) and rows["before_znear"][0] not in own
    assert Z[rows["beyond_zfar"][0]] == np.nextafter(np.float32(10.0), np.float32(np.inf)) and rows["beyond_zfar"][0] not in own
    # discs cut by the borders: they own pixels of the border row / column, and fewer than the whole disc away from it
    whole = _pixels(hc.owners(np.array([hc._at(60.5, 40.5, 1.5)], np.float32))[1], [0])
    for label, on_border in (("cut_left", owner[:, 0]), ("cut_right", owner[:, W - 1]), ("cut_top", owner[0, :]), ("cut_bottom", owner[H - 1, :])):
        r = rows[label][0]
        assert (on_border == r).any() and 0 < _pixels(owner, [r]) < whole, label
    c0, c1 = rows["cut_corner"]
    assert owner[0, 0] == c0 and owner[H - 1, W - 1] == c1 and max(_pixels(owner, [c0]), _pixels(owner, [c1])) < whole / 2
    # centres outside the image
    bw, bh, area = hc.boxes(v, **hc.PARAMS)
    r = rows["centre_outside_reaches_in"][0]
    assert v[r, 0] * 80.0 / Z[r] + 64.0 < 0 and r in own and (owner[:, 0] == r).any()
    r = rows["centre_outside_misses"][0]
    assert v[r, 0] * 80.0 / Z[r] + 64.0 < 0 and r not in own and area[r] > 0     # its box reaches in, its disc covers no pixel centre
    r = rows["between_centres"][0]
    assert r not in own and area[r] > 0
    # the point in front of znear: clipped by PARAMS, every pixel by COVER_PARAMS
    r = rows["covers_all"][0]
    assert r not in own and area[r] == 0
    cover = hc.owners(v, hc.COVER_PARAMS)
    assert (cover[1] == r).all() and cover[2].tolist() == [r]
    assert hc.boxes(v, **hc.COVER_PARAMS)[2][r] == H * W


def test_the_rows_that_are_not_finite_splat_nothing():
    v, rows = hc.edge_scene(True)
    plain, plain_rows = hc.edge_scene()
    bad = rows["nonfinite"]
    assert len(bad) == len(hc.NONFINITE_ROWS) and not np.isfinite(v[bad[:-1]]).all(axis=1).any() and np.isfinite(v[bad[-1]]).all()
    img, owner, own = hc.owners(v)
    assert not np.isin(own, bad).any() and np.isnan(img[owner >= 0]).all()        # (the colours: min / max over a tensor with a NaN)
    # the same picture as without them, the later rows renumbered
    keep = np.setdiff1d(np.arange(len(v)), bad)
    assert np.array_equal(v[keep].view(np.int32), plain.view(np.int32))
    want = hc.owners(plain)[1]
    assert np.array_equal(np.where(owner >= 0, np.searchsorted(keep, owner), -1), want)
    assert (hc.boxes(v, **hc.PARAMS)[2][bad] == 0).all()


def test_the_edge_scene_tells_the_tie_rule_from_its_opposite():
    """The oracle on the rows in reverse order, the row numbers mapped back: where two discs tie, the other one wins."""
    v, rows = hc.edge_scene()
    owner = hc.owners(v)[1]
    rev = hc.owners(v[::-1])[1]
    back = np.where(rev >= 0, len(v) - 1 - rev, -1)
    assert np.array_equal(back >= 0, owner >= 0)
    differ = back != owner
    assert differ.sum() >= 6
    tied = sum((rows[k] for k in ("tie_ascending", "tie_descending", "tie_triple", "duplicate")), [])
    assert np.isin(owner[differ], tied).all() and np.isin(back[differ], tied).all() and (back[differ] > owner[differ]).all()


def test_the_threshold_cloud_has_the_four_groups():
    small_max = hc.limits()["splat_small"]
    v, area = hc.threshold_cloud()
    assert small_max == 24 and len(v) == 4 * 64 + 37
    bw, bh, again = hc.boxes(v, **hc.PARAMS)
    assert np.array_equal(area, again) and np.array_equal(area, bw * bh)
    g = [area[64 * k:64 * (k + 1)] for k in range(5)]
    assert (g[0] == small_max).sum() >= 8 and (g[0] == small_max + 1).sum() >= 8
    assert ((g[1] > 0) & (g[1] <= small_max)).sum() == 32 and (g[1] > small_max).sum() == 32
    assert (g[2] > small_max).all() and ((g[3] > 0) & (g[3] <= small_max)).all()
    assert len(g[4]) == 37 and (g[4] == 0).sum() == 7 and (g[4] > small_max).any() and ((g[4] > 0) & (g[4] <= small_max)).any()
    # boxes of exactly 24 and of exactly 25 pixels own pixels: a path that dropped either would be seen
    own = hc.owners(v)[2]
    assert np.isin(np.flatnonzero(area == small_max), own).sum() >= 4 and np.isin(np.flatnonzero(area == small_max + 1), own).sum() >= 4
    # the formulas are the oracle's: the pixels a lone point owns lie inside its box, and a row without a box owns nothing
    for r in (0, 64, 128, 200, 270):
        o = hc.owners(v[[r]])[1]
        ii, jj = np.nonzero(o >= 0)
        assert (area[r] == 0 and len(ii) == 0) or (np.ptp(ii) + 1 <= bh[r] and np.ptp(jj) + 1 <= bw[r]), r


def test_the_batched_clouds_and_the_second_trips():
    lim = hc.limits()
    clouds = hc.batched_clouds()
    assert [len(c) for c in clouds[3:]] == list(hc.RAGGED_COUNTS) == [0, 1, 63, 64, 65, 4097]
    assert max(len(c) for c in clouds) == 4097
    for k in (7, 8):   # the larger random scenes hide and show
        own = hc.reference_owners(k)[2]
        assert 0 < len(own) < len(clouds[k])
    for stride, blocks in ((lim["splat_batched_blocks"] * lim["block"], 1024), (lim["splat_blocks"] * lim["block"], 4096)):
        assert stride == blocks * 256
        v, img, owner, own = hc.second_trip_cloud(stride)
        assert len(v) == stride + hc.PAST_STRIDE
        in_range = np.flatnonzero((v[:, 2] >= 1.0) & (v[:, 2] <= 10.0))
        assert len(in_range) == hc.IN_RANGE_HEAD + hc.PAST_STRIDE and in_range[hc.IN_RANGE_HEAD] == stride
        assert (own >= stride).sum() > 100 and (own < stride).sum() > 100       # rows past the stride own pixels, and so do early ones


# --------------------------------------------------------------------------------------------------- C'. the pipeline: cull -> z-buffer

def test_oracle_zbuffer_occlusion_masks_on_two_walls():
    from oracle import oracle
    pts, poses, quats, want = hc.two_wall_case()
    got = oracle.occlusion_masks(pts, poses, quats, K, IW, IH, *hc.CULL_LIMITS, method="zbuffer")
    assert got.dtype == np.float32 and np.array_equal(got, want) and (want == 0).sum() == 81
    # fewer than 4 kept points: the row of ones, whatever hides what
    few = np.array([[0.0, 0.0, 3.0], [0.0, 0.0, 6.0], [0.0, 0.0, 9.0], [0.0, 0.0, 30.0]], np.float32)
    assert oracle.occlusion_masks(few, poses, quats, K, IW, IH, *hc.CULL_LIMITS, method="zbuffer").tolist() == [[1.0, 1.0, 1.0, 1.0]]
    four = np.concatenate([few[:3], [[0.5, 0.5, 4.0]]]).astype(np.float32)
    assert oracle.occlusion_masks(four, poses, quats, K, IW, IH, *hc.CULL_LIMITS, method="zbuffer").tolist() == [[1.0, 0.0, 0.0, 1.0]]
    with pytest.raises(ValueError):
        oracle.occlusion_masks(few, poses, quats, K, IW, IH, method="pulsar")


def test_the_rows_case_has_its_poses():
    c = hc.rows_case()
    assert len(c["pts"]) == hc.ROWS_N == 20_000 and hc.ROWS_N % 2048 and c["want"].shape == (hc.ROWS_W, hc.ROWS_N)
    assert c["counts"][hc.ROWS_NOTHING] == 0 and c["counts"][hc.ROWS_THREE] == 3
    assert (c["want"][[hc.ROWS_NOTHING, hc.ROWS_THREE]] == 1).all()
    for w in set(range(hc.ROWS_W)) - {hc.ROWS_NOTHING, hc.ROWS_THREE}:
        hidden = int((c["want"][w] == 0).sum())
        assert 0.05 * c["counts"][w] < hidden < 0.95 * c["counts"][w], (w, hidden, c["counts"][w])
        assert (c["want"][w][np.setdiff1d(np.arange(hc.ROWS_N), c["kept"][w])] == 1).all()


# ------------------------------------------------------------------------------------------------- D. tohip_occlusion_rows_masked

def test_occ_row_ref_on_hand_made_rows():
    n, npad = 40, 64
    kept = np.array([3, 5, 39, 31, 32])
    inv = np.arange(n)[::-1].copy()                       # caller's row r sits at packed position 39 - r
    # index lists: kept rows 5 and 31 visible
    words = hc.occ_row_ref(n, npad, inv, kept, np.array([1, 3])).view(np.uint32)
    bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).ravel()
    hidden = 39 - np.array([3, 39, 32])
    assert np.flatnonzero(bits[:n] == 0).tolist() == sorted(hidden.tolist()) and (bits[n:] == 1).all()
    # the same from a visibility vector; -0.0 hides, any other value shows
    vis = np.array([0.0, 0.25, -0.0, 1.0, 0.0], np.float32)
    assert np.array_equal(hc.occ_row_ref(n, npad, inv, kept, visible=vis).view(np.uint32), words)
    # no permutation: packed positions; the last sorted point hidden: pad bits 0
    words = hc.occ_row_ref(n, npad, None, kept, visible=vis).view(np.uint32)
    bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).ravel()
    assert np.flatnonzero(bits == 0).tolist() == [3, 32, 39] + list(range(40, 64))
    # min_points
    ones = np.full(2, -1, np.int32)
    assert np.array_equal(hc.occ_row_ref(n, npad, None, kept[:3], visible=np.zeros(3), min_points=4), ones)
    assert not np.array_equal(hc.occ_row_ref(n, npad, None, kept[:4], visible=np.zeros(4), min_points=4), ones)


def test_the_rows_cases_have_their_runs():
    lim = hc.limits()
    n, m = hc.OCC_N, hc.OCC_KEPT
    stride = lim["rows_blocks"] * 256
    assert stride == hc.OCC_STRIDE and 2 * stride < m <= 3 * stride and n % 2048 and hc.OCC_BLOCK[0] % 32 == 0
    assert hc.OCC_SEG_OFF[0] != 0 and hc.OCC_SEG_OFF[1] > hc.OCC_SEG_OFF[0] + m
    for in_order in (True, False):
        c = hc.occ_rows_case(in_order)
        assert c["npad"] == 200_704 and c["want"].shape == (2, c["npad"] // 32) and (c["inv"] is None) == in_order
        for w in range(2):
            k = c["kept"][w, :m].astype(np.int64)
            vis = c["visible"][hc.OCC_SEG_OFF[w]:hc.OCC_SEG_OFF[w] + m]
            assert len(np.unique(k)) == m and (np.all(np.diff(k) > 0) if in_order else not np.all(np.diff(k) > 0))
            pos = k if in_order else c["inv"][k]
            j_last = int(np.flatnonzero(pos == n - 1)[0])
            assert (vis[j_last] == 0) == (w == 0)
            pad = c["want"][w].view(np.uint32)[-1] >> np.uint32(31)
            assert pad == (0 if w == 0 else 1)
            hid = np.flatnonzero(vis == 0)
            assert set((hid // stride).tolist()) == {0, 1, 2} and np.signbit(vis[hid]).any() and len(set(vis[vis != 0].tolist())) > 1
    c = hc.occ_rows_case(True)
    st = hc.run_stats(c["kept"][0, :m], c["visible"][hc.OCC_SEG_OFF[0]:hc.OCC_SEG_OFF[0] + m])
    assert st["lengths"] == set(range(1, 33)) and st["hvh"] and st["crosses_word"] and st["crosses_wave"] and st["full_word"]
    assert st["trips"] == {0, 1, 2}
    assert (c["want"][0] == 0).any()                       # a word hidden completely
