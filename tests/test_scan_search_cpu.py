"""CPU checks of relocalisation (no GPU): the four entry points are declared in the header and in _lib's table at ABI 15 and refuse bad
arguments — a non-zero `flags` among them — before any launch; check_scan_search names every refusal; the numpy restatement of the
branch-and-bound search gives the exhaustive search's flat index, score and ties on random maps — windows larger than the map and a tie
among them — and, where correlate's window reaches, scan_best_ref(scan_correlate_ref(...)); every bound is an upper bound of its
children's and the score itself at level 0; on the end-to-end scene the restatement alone recovers the planted offset with fewer than a
hundredth of the candidates left at level 0; and the default levels and the full window are what their definitions say."""
import ctypes

import numpy as np
import pytest

import scan_match_cases as sc
import scan_search_cases as ss
from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

EINVAL, ENOSPC = -1, -2
ENTRIES = ["tohip_reloc_levels", "tohip_reloc_bounds", "tohip_reloc_workspace_bytes", "tohip_reloc_search"]


def test_header_and_table_declare_the_new_entries_at_abi_15():
    from trajectory_optimization_amd import _lib
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_reloc_levels / tohip_reloc_bounds / tohip_reloc_workspace_bytes / tohip_reloc_search" in before
    for sym in ENTRIES:   # `..., void *stream, uint32_t flags)`: the reserved word comes last
        tail = " ".join(header.split(sym + "(")[-1].split(";")[0].split())
        assert tail.endswith("void *stream, uint32_t flags)") or sym == "tohip_reloc_workspace_bytes", sym
    assert [len(_lib.SIGNATURES[s][1]) for s in ENTRIES] == [9, 17, 1, 20]
    assert _lib.SIGNATURES["tohip_reloc_workspace_bytes"][0] is ctypes.c_size_t
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("tohip_scan_")) == ["tohip_scan_best", "tohip_scan_correlate", "tohip_scan_prepare",
                                                                                  "tohip_scan_score"]


def test_entries_refuse_bad_arguments_and_flags_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    table, levels, pts, poses, nodes, a, b, work = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 24, 1 << 28, 1 << 29, 1 << 30, 1 << 31, 1 << 32,
                                                                                 1 << 33))
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, dims=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*dims))
    ok, nb = geom(), L.tohip_evid_bytes(64, 64, 32)
    ws = L.tohip_reloc_workspace_bytes
    assert ws(0) == 0 and ws(-1) == 0 and ws((1 << 24) + 1) == 0
    assert ws(1) > 4 * 4 * 256 and ws(1 << 24) >= (1 << 24) * 40 and ws(1000) <= ws(1001) < ws(2000) and ws(5) % 256 == 0
    calls = {
        "levels": (L.tohip_reloc_levels, ("table", "table_bytes", "geom", "unknown", "h", "levels", "levels_bytes", "stream", "flags"),
                   (table, nb, ok, 0, 3, levels, 3 * nb, None, 0)),
        "bounds": (L.tohip_reloc_bounds, ("table", "table_bytes", "geom", "unknown", "level", "points", "n", "poses", "k", "nodes", "m", "bounds",
                                          "used", "workspace", "workspace_bytes", "stream", "flags"),
                   (table, nb, ok, 0, 2, pts, 100, poses, 3, nodes, 50, a, b, work, ws(50), None, 0)),
        "search": (L.tohip_reloc_search, ("table", "table_bytes", "levels", "levels_bytes", "geom", "unknown", "h", "points", "n", "poses", "k", "wx",
                                          "wy", "wz", "capacity", "record", "workspace", "workspace_bytes", "stream", "flags"),
                   (table, nb, levels, 3 * nb, ok, 0, 3, pts, 100, poses, 3, 40, 30, 1, 1000, a, work, ws(1000), None, 0)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, v) for k, v in zip(names, base)])

    odd = ctypes.c_void_p((1 << 31) + 2)
    for name in calls:
        for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
            assert call(name, flags=flags) == EINVAL, (name, flags)
        assert call(name, geom=None) == EINVAL and call(name, table_bytes=nb - 1) == ENOSPC, name
        for g in (geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(dims=(0, 64, 32)), geom(dims=(64, 2049, 32))):
            assert call(name, geom=g) == EINVAL, name
        for kw in (dict(table=None), dict(table=ctypes.c_void_p((1 << 20) + 8)), dict(unknown=-128), dict(unknown=1)):
            assert call(name, **kw) == EINVAL, (name, kw)
    for kw in (dict(h=0), dict(h=7), dict(levels=None), dict(levels=ctypes.c_void_p((1 << 24) + 8)), dict(levels=table),
               dict(levels=ctypes.c_void_p((1 << 20) + 32)), dict(levels=ctypes.c_void_p((1 << 20) - 32))):
        assert call("levels", **kw) == EINVAL, kw
    assert call("levels", levels_bytes=3 * nb - 1) == ENOSPC and call("levels", h=6, levels_bytes=6 * nb - 1) == ENOSPC
    for kw in (dict(level=-1), dict(level=7), dict(points=None), dict(poses=None), dict(nodes=None), dict(bounds=None), dict(used=None),
               dict(workspace=None), dict(n=0), dict(n=(1 << 22) + 1), dict(k=0), dict(k=257), dict(m=0), dict(m=(1 << 22) + 1), dict(used=a),
               dict(workspace=a), dict(workspace=b), dict(bounds=pts), dict(used=poses), dict(workspace=nodes), dict(bounds=table),
               dict(bounds=odd), dict(points=odd), dict(nodes=ctypes.c_void_p((1 << 30) + 4)), dict(workspace=ctypes.c_void_p((1 << 33) + 8))):
        assert call("bounds", **kw) == EINVAL, kw
    assert call("bounds", workspace_bytes=ws(50) - 1) == ENOSPC
    for kw in (dict(h=-1), dict(h=7), dict(levels=None), dict(levels=ctypes.c_void_p((1 << 24) + 8)), dict(points=None), dict(poses=None),
               dict(record=None), dict(workspace=None), dict(n=0), dict(n=(1 << 22) + 1), dict(k=0), dict(k=257), dict(wx=-1), dict(wx=2049),
               dict(wy=-1), dict(wy=2049), dict(wz=-1), dict(wz=5), dict(capacity=0), dict(capacity=(1 << 24) + 1), dict(workspace=a),
               dict(record=pts), dict(workspace=poses), dict(record=table), dict(record=levels), dict(record=ctypes.c_void_p((1 << 31) + 4)),
               dict(workspace=ctypes.c_void_p((1 << 33) + 8)), dict(poses=odd)):
        assert call("search", **kw) == EINVAL, kw
    assert call("search", levels_bytes=3 * nb - 1) == ENOSPC and call("search", workspace_bytes=ws(1000) - 1) == ENOSPC
    assert call("search", capacity=2000) == ENOSPC   # (the workspace is sized for 1000)
    assert call("search", h=0, levels=None, levels_bytes=0, table_bytes=nb - 1) == ENOSPC   # (no levels are needed for h = 0: the next check)


def test_check_scan_search_names_every_refusal():
    import torch

    from trajectory_optimization_amd import ops

    class M(ops.EvidenceMap):   # a map's geometry without a device
        def __init__(self):
            self.origin, self.resolution, self.dims, _ = ops.check_los((0, 0, 0), 0.1, (8, 8, 4))
            self.device = torch.device("cuda:0")

    m = M()
    assert ops.check_scan_search(m) == (None, None, None, None)
    assert ops.check_scan_search(m, (2048, 0, 4), 6, 1 << 24, 256) == ((2048, 0, 4), 6, 1 << 24, 256)
    assert ops.check_scan_search(m, [np.int64(24), 20, 1], None, np.int32(7), 1) == ((24, 20, 1), 2, 7, 1)
    for bad in (None, object(), ops.SpaceMap.__new__(ops.SpaceMap)):
        with pytest.raises(ValueError, match="the map must be an ops.EvidenceMap"):
            ops.check_scan_search(bad)
    for bad in ((2049, 0, 0), (0, 2049, 0), (0, 0, 5), (-1, 0, 0), (1, 1), (1.0, 1, 1), 3, "888"):
        with pytest.raises(ValueError, match="window must be three integers"):
            ops.check_scan_search(m, bad)
    for bad in (-1, 7, 1.0, "3", True):
        with pytest.raises(ValueError, match=r"levels must be None or an integer in \[0, 6\]"):
            ops.check_scan_search(m, (1, 1, 1), bad)
    for bad in (0, (1 << 24) + 1, 1.5, "9"):
        with pytest.raises(ValueError, match=r"capacity must be an integer in \[1, 2\^24\]"):
            ops.check_scan_search(m, (1, 1, 1), 1, bad)
    for bad in (0, 257, 1.0):
        with pytest.raises(ValueError, match="the rotations must number 1 .. 256"):
            ops.check_scan_search(m, (1, 1, 1), 1, 8, bad)
    assert ops.scan_search_status(0) is None and ops.scan_search_status((198147 << 3) | 1) == (0, 198147)
    assert ops.SCAN_SEARCH_RECORD == synth.RELOC_RECORD and ops.SCAN_SEARCH_MAX_WINDOW == synth.RELOC_MAX_WINDOW
    assert ops.SCAN_SEARCH_MAX_CAPACITY == synth.RELOC_MAX_CAPACITY and ops.SCAN_SEARCH_MAX_LEVELS == synth.RELOC_MAX_LEVELS


def test_default_levels_and_the_full_window():
    from trajectory_optimization_amd import ops
    for window, H in (((0, 0, 0), 0), ((7, 7, 4), 0), ((8, 7, 0), 0), ((8, 8, 0), 1),((24, 20, 1), 2), ((64, 64, 1), 4), ((202, 202, 0), 5), ((404, 404, 0), 6),
                      ((2048, 2048, 0), 6), ((2048, 0, 0), 5)):
        assert ops.scan_search_levels(window) == synth.reloc_default_levels(window) == H, window
        blocks = lambda h: -(-(2 * window[0] + 1) // (1 << h)) * -(-(2 * window[1] + 1) // (1 << h))   # noqa: E731
        assert H == 6 or blocks(H) <= 256
        assert H == 0 or blocks(H - 1) > 256
    for voxel, dims, want in (((0, 0, 0), (405, 405, 45), (404, 404, 0)), ((202, 100, 7), (405, 405, 45), (202, 304, 0)),
                              ((-5, 9999, 3), (48, 40, 12), (47, 39, 0)), ((0, 0, 0), (1, 1, 1), (0, 0, 0))):
        assert ops.scan_search_window(voxel, dims) == synth.reloc_full_window(voxel, dims) == want
        i = np.clip(voxel[:2], 0, np.asarray(dims[:2]) - 1)   # every voxel of dims is reached from the clamped prior
        assert (i - want[:2] <= 0).all() and (i + want[:2] >= np.asarray(dims[:2]) - 1).all()


@pytest.mark.parametrize("p", ss.SEARCH_PARAMS, ids=ss.search_id)
def test_the_search_is_the_exhaustive_search(p):
    i, v, K = p
    dims, window, H, _, _ = ss.SEARCHES[i]
    L, P = ss.inputs(i)
    Rs = ss.rotation_matrices(K)
    rec = ss.search_ref(i, v, K)
    want = synth.scan_exhaustive_ref(L, sc.ORIGIN, sc.RES, P, Rs, sc.T, window, *ss.VALUES[v])
    assert rec[7] == 0 and rec[10] == H
    assert (rec[0], rec[5], rec[6]) == (want[0], want[5], want[6])
    assert np.array_equal(rec[:7], want)
    S = (2 * window[0] + 1) * (2 * window[1] + 1) * (2 * window[2] + 1)
    assert 1 <= rec[6] <= rec[11] <= K * S and rec[8] <= rec[5] and rec[9] >= rec[11:12 + H].sum()
    assert rec[11 + H] == K * (2 * window[2] + 1) * -(-(2 * window[0] + 1) // (1 << H)) * -(-(2 * window[1] + 1) // (1 << H))
    if all(w <= m for w, m in zip(window, synth.SCAN_MAX_WINDOW)):
        scores, _ = synth.scan_correlate_ref(L, sc.ORIGIN, sc.RES, P, Rs, sc.T, window, *ss.VALUES[v])
        assert np.array_equal(rec[:7], synth.scan_best_ref(scores)[:7])
    if dims == (4, 4, 2) and K == 3:
        assert rec[6] == 2   # (the tie the case was chosen for)


def test_a_level_over_the_capacity_stops_the_search():
    dims, window, H, _, _ = ss.SEARCHES[1]
    L, P = ss.inputs(1)
    full = ss.search_ref(1, 0, 3)
    for level in range(H + 1):
        rec = synth.scan_search_ref(L, sc.ORIGIN, sc.RES, P, ss.rotation_matrices(3), sc.T, window, H, capacity=int(full[11 + level]) - 1)
        assert rec[0] == -1 and rec[7] == (full[11 + level] << 3) | (level + 1) and rec[11 + level] == full[11 + level]
        assert np.array_equal(rec[12 + level:12 + H], full[12 + level:12 + H]) and not rec[11:11 + level].any() and not rec[1:7].any()


@pytest.mark.parametrize("level", range(7))
def test_a_bound_covers_its_children_and_is_the_score_at_level_0(level):
    dims, K = (13, 10, 5), 3
    L, P = ss.inputs(0)
    Rs = ss.rotation_matrices(K)
    nodes = ss.probe_nodes(dims, level, K, 400)
    floor, unknown = ss.VALUES[1]
    bound, used = synth.scan_bound_ref(L, sc.ORIGIN, sc.RES, P, Rs, sc.T, nodes, level, floor, unknown)
    assert (used > 0).all() and (used < len(P)).all()
    if level == 0:
        for (k, sx, sy, sz), b in zip(nodes[:60], bound[:60]):
            assert b == synth.scan_score_ref(L, sc.ORIGIN, sc.RES, P, Rs[k], sc.T, (sx, sy, sz), floor, unknown)[0]
        return
    half = 1 << (level - 1)
    kids = np.full(len(nodes), -(1 << 40), dtype=np.int64)
    for j in range(4):
        c = nodes.copy()
        c[:, 1] += (j & 1) * half
        c[:, 2] += (j >> 1) * half
        kids = np.maximum(kids, synth.scan_bound_ref(L, sc.ORIGIN, sc.RES, P, Rs, sc.T, c, level - 1, floor, unknown)[0])
    assert (bound >= kids).all() and (bound > kids).any()


def test_level_tables_are_sliding_maxima_with_the_edge_rule():
    L, _ = ss.inputs(4)
    floor, unknown = ss.VALUES[1]
    T = synth.scan_levels_ref(L, 6, floor, unknown)
    nx, ny, nz = L.shape
    u = 128 + unknown
    big = np.full((nx + 64, ny + 64, nz), u, dtype=np.int64)
    big[:nx, :ny] = T[0]
    for h in range(1, 7):
        views = np.lib.stride_tricks.sliding_window_view(big, (1 << h, 1 << h), axis=(0, 1))
        assert np.array_equal(T[h], views[:nx, :ny].max(axis=(3, 4)))
        img = synth.scan_level_bytes_ref(T[h], unknown)
        assert img.dtype == np.uint8 and len(img) == len(synth.scan_table_ref(L, floor, unknown)) and not img[:256].any()
    assert np.array_equal(synth.scan_level_bytes_ref(T[0], unknown), synth.scan_table_ref(L, floor, unknown))
    assert (T[6][0, 0] == np.maximum(T[0].max(axis=(0, 1)), u)).all()   # (37 x 29 lies inside one 64 x 64 block, with the outside's u)


def test_the_scene_is_recovered_with_a_hundredth_of_the_candidates():
    L, pts, t, quats = ss.scene()
    rec = ss.scene_ref()
    candidates = len(quats) * 49 * 41 * 3
    assert candidates == 54243
    assert tuple(rec[2:5]) == sc.PLANTED_SHIFT and rec[1] == sc.YAW_STEPS // 2 + sc.PLANTED_STEPS == 6
    assert rec[6] == 1 and rec[5] == 70 * len(pts) and rec[7] == 0 and rec[10] == 3
    assert rec[11 + 3] == 9 * 3 * 7 * 6
    print("nodes per level 0 .. 3:", rec[11:15], "evaluated", rec[9], "of", candidates, "candidates; incumbent", rec[8])
    assert rec[11] <= candidates / 100
    assert rec[9] < candidates / 10
