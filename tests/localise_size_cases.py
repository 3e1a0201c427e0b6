"""The inputs shared by the tests of relocalisation, fine registration and the pose graph at capacity and at size
(tests/test_localise_at_size_cpu.py without a GPU; tests/test_hip_scan_search_at_size.py, tests/test_hip_scan_register_at_size.py and
tests/test_hip_pose_graph_at_size.py on one) and what the numpy restatements of synth say of them, computed once per process and
never modified.  Numpy only.  Every case names the CONDITION it exists for; the CPU test asserts it from the constants read out of
the kernels' text (limits()), so that a change of a constant fails there by name and does not quietly empty a GPU test.

A1  explicit nodes in 256 chunks over scans of 17 and 33 tiles: a share of k_reloc_bound walks two and three tiles.
A2  searches over 256 rotations whose every list has 256 chunks: every bound launch of the search has shares of several tiles.
A3  a scan of 2^22 points, the cap, through the search: 64 points tiled 65 536 times, the reference scaled.
A4  the level tables of a grid of 592 128 brick words: past one grid-stride pass, the stride-32 neighbour on both axes.
A5  the lists at the capacity of 2^24 nodes, and 16 388 over it: arithmetic on a constant map.
L6  the (2047, 2045, 511) grid of tests/scan_match_size_cases.py for the search (A6) and for registration (B4): the stand-in is the
    window on a small grid whose ORIGIN is moved, so that the same points under the same poses fall into the same voxels.
B1  the nine crafted rows of k_scan_step over 256 poses, every status in each of its four blocks.
B2  256 poses through k_scan_normal: eight tile blocks a pose, each over two tiles and more.
B3  256 registrations to three statuses.
C1  a pose graph of 70 000 nodes and 70 399 edges: 274 and 275 blocks.
C2  a hub whose CSR row is longer than a block."""
import functools
import os
import re

import numpy as np

import map_size_cases as mc
import pose_graph_cases as pc
import scan_match_cases as sc
import scan_match_size_cases as zc
import scan_register_cases as rc
import scan_search_cases as ss

from trajectory_optimization_amd import synth

f32 = np.float32
INT32_MAX = (1 << 31) - 1


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def limits():
    """The constants the cases depend on, read from the kernels' text (an assertion names the pattern that is gone)."""
    names = ("common.hpp", "occupancy_kernels.hip", "scanmatch_kernels.hip", "scansearch_kernels.hip", "scanreg_kernels.hip", "posegraph_kernels.hip")
    text = {name: open(os.path.join(zc.CSRC, name)).read() for name in names}

    def one(name, pattern):
        m = re.search(pattern, text[name])
        assert m, (name, pattern)
        return int(m.group(1))

    return dict(
        block=one("common.hpp", r"#define TO_BLOCK\s+(\d+)"),
        wave=one("common.hpp", r"#define TO_WAVE\s+(\d+)"),
        occ_blocks=one("occupancy_kernels.hip", r"constexpr int kOccBlocks = (\d+);"),
        scan_blocks=one("scanmatch_kernels.hip", r"constexpr int kScanBlocks = (\d+);"),
        max_points=1 << one("scanmatch_kernels.hip", r"constexpr long long kScanMaxPoints = 1ll << (\d+);"),
        max_k=one("scanmatch_kernels.hip", r"constexpr int kScanMaxK = (\d+);"),
        reloc_items=one("scansearch_kernels.hip", r"constexpr int kRelocItems = (\d+);"),
        reloc_block=one("scansearch_kernels.hip", r"constexpr int kRelocBlock = (\d+);"),
        reloc_capacity=1 << one("scansearch_kernels.hip", r"constexpr long long kRelocMaxCapacity = 1ll << (\d+);"),
        reloc_levels=one("scansearch_kernels.hip", r"constexpr int kRelocMaxLevels = (\d+);"),
        reg_max_poses=one("scanreg_kernels.hip", r"constexpr int kRegMaxPoses = (\d+);"),
        pg_max=1 << one("posegraph_kernels.hip", r"constexpr long long kPgMax = 1ll << (\d+);"),
        pg_node=one("posegraph_kernels.hip", r"constexpr int kPgNode = (\d+);"),
    )


def bound_plan(counts, n):
    """How k_reloc_offsets and k_reloc_bound split a list whose rotations hold `counts` nodes over a scan of n points -> dict(n_tiles,
    n_chunks, ysplit, items, trips): a chunk is up to TO_BLOCK nodes of one rotation, ysplit = min(ceil(kRelocItems / n_chunks),
    n_tiles) shares of the tiles per chunk, share `part` walks the tiles part, part + ysplit, ...; trips[part] counts them."""
    lim = limits()
    n_tiles = -(-int(n) // lim["block"])
    n_chunks = int(sum(-(-int(c) // lim["block"]) for c in counts))
    y = -(-lim["reloc_items"] // n_chunks) if n_chunks > 0 else 1
    ysplit = min(y, n_tiles)
    return dict(n_tiles=n_tiles, n_chunks=n_chunks, ysplit=ysplit, items=n_chunks * ysplit,
                trips=[len(range(part, n_tiles, ysplit)) for part in range(ysplit)])


def list_passes(count, capacity):
    """Grid-stride passes the list kernels of a search make over a list of `count` nodes: their launch holds occ_grid_blocks(capacity)
    blocks."""
    lim = limits()
    blocks = min(max(-(-int(capacity) // lim["block"]), 1), lim["occ_blocks"])
    return -(-int(count) // (blocks * lim["block"]))


# ---- A. relocalisation ------------------------------------------------------------------------------------------------------------------

A_DIMS, A_SEED, A_FLOOR, A_UNKNOWN, A_K = (37, 29, 9), 3, -10, -8, 256
A1_SHAPES = ((256, 4097), (1280, 8193))          # (nodes, points)
A1_LEVELS = (tuple(range(7)), (1, 4))
A2_SEARCHES = (((2, 2, 0), 1), ((3, 2, 1), 2))   # (window, H)


def a_quats():
    """256 yaws in steps of 0.2 degrees around the identity (row 128): close enough that no rotation's nodes are all pruned."""
    return zc.s3_quats()


@functools.lru_cache(maxsize=None)
def a_rotations():
    return _frozen(np.stack([synth.scan_rotation(q) for q in a_quats()]))


@functools.lru_cache(maxsize=None)
def a_log_odds():
    return _frozen(sc.random_log_odds(A_DIMS, A_SEED))


@functools.lru_cache(maxsize=None)
def a_scan(n):
    """sc.random_scan over A_DIMS with, in every run of 16 rows, one row out of range (1e6 or NaN in turn) and one on a ring of 3900 ..
    4300 voxels around the sensor, which a yaw takes across the range's faces at -2048 and 4096 voxels: every full tile holds points
    in range and points out of range, and `used` differs between rotations.  The last row is in range under every rotation."""
    P = sc.random_scan(A_DIMS, n, 11).astype(f32)
    rng = np.random.default_rng(9100 + n)
    rows = np.arange(n - 1)
    out, rim = rows[rows % 16 == 9], rows[rows % 16 == 3]
    P[out[0::2]] = f32([1.0e6, 0.0, 0.0])
    P[out[1::2], 1] = np.nan
    rho, phi = rng.uniform(3900.0, 4300.0, len(rim)) * sc.RES, rng.uniform(0.0, 2.0 * np.pi, len(rim))
    P[rim] = np.stack([rho * np.cos(phi), rho * np.sin(phi), rng.uniform(0.0, 1.0, len(rim))], axis=1).astype(f32)
    return _frozen(P)


@functools.lru_cache(maxsize=None)
def a_in_range(n):
    """(256, n) bool: the points of a_scan(n) in range under each rotation."""
    return _frozen(np.stack([synth.scan_voxels_ref(a_scan(n), R, sc.T, sc.ORIGIN, sc.RES)[1] for R in a_rotations()]))


@functools.lru_cache(maxsize=None)
def a1_nodes(shape, level):
    """m nodes (m,4) int64 (k, sx, sy, sz) of one level over three voxels around the box.  Shape 0: one node per rotation, the
    rotations in a seeded order; shape 1: five per rotation, interleaved (k = i mod 256).  Either way the list has 256 chunks."""
    m, _ = A1_SHAPES[shape]
    rng = np.random.default_rng(9200 + 31 * shape + level)
    nx, ny, nz = A_DIMS
    b = (1 << level) - 1
    k = rng.permutation(A_K) if shape == 0 else np.arange(m) % A_K
    nodes = np.stack([k, rng.integers(-nx - b - 3, nx + 4, m), rng.integers(-ny - b - 3, ny + 4, m), rng.integers(-nz - 1, nz + 2, m)], axis=1)
    return _frozen(nodes.astype(np.int64))


@functools.lru_cache(maxsize=None)
def a1_reference(shape, level):
    """-> (bounds (m,) int32, used (256,) int32) by synth.scan_bound_ref."""
    _, n = A1_SHAPES[shape]
    return _frozen(*synth.scan_bound_ref(a_log_odds(), sc.ORIGIN, sc.RES, a_scan(n), a_rotations(), sc.T, a1_nodes(shape, level), level, A_FLOOR,
                                         A_UNKNOWN))


def a1_plan(shape, level=0):
    """CONDITION of A1 -> bound_plan of the list, and `mixed` (256, n_tiles) bool: the tiles that hold points in range and points out
    of range under each rotation."""
    _, n = A1_SHAPES[shape]
    plan = bound_plan(np.bincount(a1_nodes(shape, level)[:, 0], minlength=A_K), n)
    block, ok = limits()["block"], a_in_range(n)
    pad = np.zeros((A_K, plan["n_tiles"] * block), dtype=bool)
    pad[:, :n] = ok
    inside = pad.reshape(A_K, plan["n_tiles"], block).sum(axis=2)
    size = np.minimum(block, n - block * np.arange(plan["n_tiles"]))
    plan["mixed"] = (inside > 0) & (inside < size[None, :])
    return plan


@functools.lru_cache(maxsize=None)
def a2_reference(i):
    """Search i of A2_SEARCHES over a_scan(4097) -> (the record by synth.scan_search_ref, scan_exhaustive_ref's seven words, {level:
    bound_plan of that level's list}).  CONDITION: every list has at least 256 chunks."""
    window, H = A2_SEARCHES[i]
    n = A1_SHAPES[0][1]
    lists = {}
    args = (a_log_odds(), sc.ORIGIN, sc.RES, a_scan(n), a_rotations(), sc.T, window)
    rec = synth.scan_search_ref(*args, H, A_FLOOR, A_UNKNOWN, lists=lists)
    plans = {h: bound_plan(np.bincount(nodes[:, 0], minlength=A_K), n) for h, nodes in lists.items()}
    return _frozen(rec), _frozen(synth.scan_exhaustive_ref(*args, A_FLOOR, A_UNKNOWN)), plans


# A3: the longest scan
A3_DIMS, A3_WINDOW, A3_H, A3_K, A3_FACTOR = (13, 10, 5), (5, 3, 1), 2, 3, 1 << 16
A3_PLANTED = (3, -2, 1)
A3_MAPS = (("planted", -10, -8), ("full", None, 0))     # (name, floor, unknown_value)


def a3_quats():
    """Three yaws; the middle one is the identity, the true heading."""
    return np.stack([sc.yaw_quat(a) for a in (-0.3, 0.0, 0.3)])


@functools.lru_cache(maxsize=None)
def a3_cells():
    """64 distinct voxels of A3_DIMS, at least one voxel from every face in x and y."""
    rng = np.random.default_rng(9300)
    nx, ny, nz = A3_DIMS
    flat = rng.choice((nx - 2) * (ny - 2) * nz, 64, replace=False)
    return _frozen(np.stack([1 + flat % (nx - 2), 1 + (flat // (nx - 2)) % (ny - 2), flat // ((nx - 2) * (ny - 2))], axis=1).astype(np.int64))


def a3_log_odds(name):
    """'planted': random values of at most 60, a third never observed, and 127 in the 64 cells; 'full': 127 everywhere — every table
    byte 255, scored with unknown_value 0."""
    if name == "full":
        return np.full(A3_DIMS, 127, dtype=np.int64)
    L = np.minimum(sc.random_log_odds(A3_DIMS, 9), 60)
    L[tuple(a3_cells().T)] = 127
    return L


def a3_translation():
    """The prior: the true translation sc.T moved back by the planted shift, so that the shift A3_PLANTED wins under rotation 1."""
    return np.asarray(sc.T, dtype=np.float64) - sc.RES * np.asarray(A3_PLANTED, dtype=np.float64)


def a3_points(copies=1):
    """The centres of the 64 cells in the sensor frame of the true pose, `copies` times over (dyadic: no rounding)."""
    return np.tile(zc.centre_points(a3_cells()), (copies, 1))


def a3_scaled(rec, factor):
    """A record of the 64 points -> the record of `factor` copies of them: the score and the incumbent are multiplied, the node counts,
    `evaluated`, the ties and the winner stay — every comparison of the search is between sums that all scale alike."""
    out = np.array(rec, dtype=np.int64)
    out[5] *= factor
    out[8] *= factor
    return out


@functools.lru_cache(maxsize=None)
def a3_reference(name, copies=1):
    """The restatement's record on `copies` x 64 points -> (18,) int64."""
    _, floor, unknown = next(m for m in A3_MAPS if m[0] == name)
    Rs = np.stack([synth.scan_rotation(q) for q in a3_quats()])
    return _frozen(synth.scan_search_ref(a3_log_odds(name), sc.ORIGIN, sc.RES, a3_points(copies), Rs, a3_translation(), A3_WINDOW, A3_H, floor,
                                         unknown))


# A4: the level tables past one pass
A4_DIMS, A4_H, A4_SEED = (1027, 1021, 17), 6, 5


@functools.lru_cache(maxsize=None)
def a4_log_odds():
    return _frozen(sc.random_log_odds(A4_DIMS, A4_SEED))


def a4_level_bytes(value):
    """The byte images of T_0 .. T_6 for the value pair ss.VALUES[value] -> a list of seven (256 + 32 words,) uint8 arrays (not
    cached: 19 MB each)."""
    floor, unknown = ss.VALUES[value]
    return [synth.scan_level_bytes_ref(T, unknown) for T in synth.scan_levels_ref(a4_log_odds(), A4_H, floor, unknown)]


def a4_plan():
    """CONDITION of A4 -> dict(words, passes of k_reloc_level's word loop, bricks per axis, q: the stride-32 neighbour's distance in
    bricks, partial: the voxels of the last brick per axis)."""
    lim = limits()
    nbx, nby, nbz = (A4_DIMS[0] + 3) // 4, (A4_DIMS[1] + 3) // 4, (A4_DIMS[2] + 1) // 2
    words = nbx * nby * nbz
    return dict(words=words, passes=-(-words // (lim["occ_blocks"] * lim["block"])), bricks=(nbx, nby, nbz), q=(1 << (A4_H - 1)) // 4,
                partial=(A4_DIMS[0] % 4, A4_DIMS[1] % 4, A4_DIMS[2] % 2))


# A5: the lists at the capacity
A5_DIMS, A5_K, A5_H, A5_N = (16, 12, 4), 4, 6, 64
A5_WINDOWS = ((1023, 1023, 0), (1024, 1023, 0), (1024, 1024, 0))   # the last: 16 388 leaves over the capacity


def a5_quats():
    return np.stack([sc.yaw_quat(0.1 * k) for k in range(A5_K)])


def a5_inputs():
    """A map that holds 0 everywhere, scored with unknown_value 0, and 64 points of sc.random_scan: every candidate scores 0."""
    return np.zeros(A5_DIMS, dtype=np.int64), sc.random_scan(A5_DIMS, A5_N, 9)


def constant_record(K, window, H, capacity):
    """The record of a search in which every bound and every score is 0, by arithmetic -> (18,) int64.  Nothing is ever pruned: level
    h holds K (2wz+1) ceil((2wx+1) / 2^h) ceil((2wy+1) / 2^h) nodes.  The best node of every list is the lowest (k, sz, sy, sx) = (0,
    -wz, -wy, -wx), and so is the best child of each descent step, which evaluates (1 + [2^lev <= 2wx]) (1 + [2^lev <= 2wy]) children
    at level lev; `evaluated` is the lists' sizes plus those.  The winner: score 0, the smallest |s|^2 — the shift (0, 0, 0) — of
    rotation 0; ties counts every leaf.  A list of more than `capacity` nodes stops it: flat index -1, status = count << 3 | level + 1,
    the counts and `evaluated` up to there."""
    wx, wy, wz = window
    nxw, nyw, nzw = 2 * wx + 1, 2 * wy + 1, 2 * wz + 1
    count = [K * nzw * -(-nxw // (1 << h)) * -(-nyw // (1 << h)) for h in range(H + 1)]
    rec = np.zeros(synth.RELOC_RECORD, dtype=np.int64)
    rec[8], rec[10] = synth.RELOC_NO_INCUMBENT, H
    if count[H] > capacity:
        rec[0], rec[7], rec[11 + H] = -1, (count[H] << 3) | (H + 1), count[H]
        return rec
    rec[9] = count[H]
    for h in range(H, 0, -1):
        rec[11 + h] = count[h]
        rec[9] += sum((1 + (1 << lev <= 2 * wx)) * (1 + (1 << lev <= 2 * wy)) for lev in range(h))
        rec[8] = 0
        if count[h - 1] > capacity:
            rec[0], rec[7], rec[11 + h - 1] = -1, (count[h - 1] << 3) | h, count[h - 1]
            return rec
        rec[9] += count[h - 1]
    rec[11] = count[0]
    rec[0] = (wz * nyw + wy) * nxw + wx
    rec[5], rec[6] = 0, count[0]
    return rec


# ---- L6. the largest grid: the stand-in with a moved origin ------------------------------------------------------------------------------

L6_SMALL_DIMS = tuple(int(c) for c in np.asarray(zc.S6_WIN) + zc.S6_SMALL_MARGIN)      # (96, 96, 64)
L6_SHIFT = zc.S6_OFF - zc.S6_SMALL_MARGIN                                               # the stand-in's first voxel in the largest grid
L6_SMALL_ORIGIN = tuple(float(o + mc.RES * s) for o, s in zip(mc.ORIGIN, L6_SHIFT))     # (multiples of 1/8: exact)
L6_WINDOW, L6_H = (16, 16, 4), 1      # (one level, to keep the search's test on the largest grid short)
L6_POSES, L6_ITERATIONS = 3, 5


@functools.lru_cache(maxsize=None)
def l6_small_log_odds():
    """The window's log-odds in the far corner of the (96, 96, 64) stand-in, never observed elsewhere."""
    L = np.full(L6_SMALL_DIMS, synth.EVID_UNKNOWN, dtype=np.int64)
    m = zc.S6_SMALL_MARGIN
    L[m[0]:, m[1]:, m[2]:] = zc.s6_window_log_odds()
    return _frozen(L)


@functools.lru_cache(maxsize=None)
def l6_points():
    """The 3000 points of the S6 scan over the window and eight voxels of its far apron, and three rows that are in no range (NaN,
    inf, 1e6).  (The S6 scan's points in the voxels around (0, 0, 0), and its rows just outside the range of the largest grid, are
    left out: seen from the moved origin they are 1951 voxels nearer, where the first meet no voxel (0, 0, 0) and the second are in
    range.)"""
    P = np.concatenate([zc.s6_points()[:3000], f32([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1.0e6, 0.0, 0.0]])])
    return _frozen(P)


def l6_frames_agree(R, t):
    """Whether the points under the pose (R, t) have the same fixed-point coordinates from the largest grid's origin, less L6_SHIFT, as
    from the stand-in's origin, and are in range in both or in neither -> (agree, q (n,3) int64 in the largest grid, ok)."""
    q, ok = synth.scan_fixed_ref(l6_points(), R, t, mc.ORIGIN, mc.RES)
    qs, oks = synth.scan_fixed_ref(l6_points(), R, t, L6_SMALL_ORIGIN, mc.RES)
    return bool(np.array_equal(ok, oks) and np.array_equal((q - 256 * L6_SHIFT)[ok], qs[ok])), q, ok


@functools.lru_cache(maxsize=None)
def a6_reference():
    """The search over the stand-in -> (the record by synth.scan_search_ref, {level: that level's nodes})."""
    lists = {}
    Rs = np.stack([synth.scan_rotation(q) for q in sc.rotations(zc.S6_K)])
    rec = synth.scan_search_ref(l6_small_log_odds(), L6_SMALL_ORIGIN, mc.RES, l6_points(), Rs, zc.s6_translation(), L6_WINDOW, L6_H, zc.S6_FLOOR,
                                zc.S6_UNKNOWN, lists=lists)
    return _frozen(rec), lists


def a6_level_check(h):
    """Level h of the largest grid over the window and a rim of 2^h voxels inside dims -> (offsets (m,) int64 into the level's buffer,
    bytes (m,) uint8): T_h of the stand-in, whose margin is wider than the rim."""
    T = synth.scan_levels_ref(l6_small_log_odds(), h, zc.S6_FLOOR, zc.S6_UNKNOWN)[h]
    lo = zc.S6_SMALL_MARGIN - (1 << h)
    vox = np.argwhere(np.ones(tuple(np.asarray(L6_SMALL_DIMS) - lo), dtype=bool)) + lo
    return zc.byte_offsets(vox + L6_SHIFT, zc.S6_DIMS), T[vox[:, 0], vox[:, 1], vox[:, 2]].astype(np.uint8)


def a6_last_word(h):
    """The last 32 bytes of level h: brick (511, 511, 255) = voxels (2044 .. 2047, 2044 .. 2047, 510 .. 511), of which (2044 .. 2046,
    2044, 510) lie inside dims; the rest is pad."""
    T = synth.scan_levels_ref(l6_small_log_odds(), h, zc.S6_FLOOR, zc.S6_UNKNOWN)[h]
    out = np.full(32, 128 + zc.S6_UNKNOWN, dtype=np.uint8)
    first = (np.asarray(zc.S6_DIMS, dtype=np.int64) - 1) // np.asarray([4, 4, 2]) * np.asarray([4, 4, 2])
    for x in range(first[0], zc.S6_DIMS[0]):
        for y in range(first[1], zc.S6_DIMS[1]):
            for z in range(first[2], zc.S6_DIMS[2]):
                v = np.asarray([x, y, z]) - L6_SHIFT
                out[(x & 3) | ((y & 3) << 2) | ((z & 1) << 4)] = T[v[0], v[1], v[2]]
    return out


def a6_far_lookups():
    """CONDITION of A6 -> dict(beyond: how many (leaf, point) lookups of the level-0 list read a byte at or beyond 2^31 from the
    table's first byte — 256 bytes of header, then 32 bytes a word: the last eight words; last_x, last_y, last_z, last_brick: the
    winner's shifted voxels in the last brick along each axis, and in brick (511, 511, 255) itself)."""
    rec, lists = a6_reference()
    Rs = [synth.scan_rotation(q) for q in sc.rotations(zc.S6_K)]
    dims = np.asarray(zc.S6_DIMS, dtype=np.int64)
    beyond = 0
    for k, R in enumerate(Rs):
        v, ok = synth.scan_voxels_ref(l6_points(), R, zc.s6_translation(), mc.ORIGIN, mc.RES)
        s = lists[0][lists[0][:, 0] == k][:, 1:]
        for i in range(0, len(s), 256):
            at = (v[ok][None, :, :] + s[i:i + 256, None, :]).reshape(-1, 3)
            at = at[((at >= 0) & (at < dims)).all(axis=1)]
            beyond += int((zc.byte_offsets(at, zc.S6_DIMS) >= 1 << 31).sum())
    v, ok = synth.scan_voxels_ref(l6_points(), Rs[int(rec[1])], zc.s6_translation(), mc.ORIGIN, mc.RES)
    at = v[ok] + rec[2:5]
    at = at[((at >= 0) & (at < dims)).all(axis=1)]
    last = at >= (dims - 1) // np.asarray([4, 4, 2]) * np.asarray([4, 4, 2])
    return dict(beyond=beyond, last_x=int(last[:, 0].sum()), last_y=int(last[:, 1].sum()), last_z=int(last[:, 2].sum()),
                last_brick=int(last.all(axis=1).sum()))


def b4_starts():
    """Three starting poses around the S6 pose (the translation zc.s6_translation(), no rotation) -> (poses (3,3) f64, quats (3,4))."""
    truth = (zc.s6_translation().astype(np.float64), np.array([1.0, 0.0, 0.0, 0.0]))
    return rc.starts(L6_POSES, seed=6, truth=truth, resolution=mc.RES)


@functools.lru_cache(maxsize=None)
def b4_reference():
    """-> (records (3,32) of the starting poses by synth.scan_normal_ref, the state (3,64) after five iterations by
    synth.scan_register_ref), both over the stand-in."""
    poses, quats = b4_starts()
    _, p12 = synth.scan_register_init_ref(poses, quats)
    args = (l6_small_log_odds(), L6_SMALL_ORIGIN, mc.RES, l6_points())
    records = synth.scan_normal_ref(*args, p12, zc.S6_FLOOR, zc.S6_UNKNOWN)
    state = synth.scan_register_ref(*args, poses, quats, L6_ITERATIONS, floor=zc.S6_FLOOR, unknown_value=zc.S6_UNKNOWN)
    return _frozen(records, state)


def b4_rows(pose12):
    """CONDITION of B4 for one pose (12 f32) -> dict(first_max: the largest dword index `first` k_scan_normal forms for a row inside
    dims; outside: the points in range with a corner outside dims on a far face; last: those with a corner in the last brick along
    x, y and z, one count per axis)."""
    pose12 = np.asarray(pose12, dtype=f32)
    q, ok = synth.scan_fixed_ref(l6_points(), pose12[:9], pose12[9:12], mc.ORIGIN, mc.RES)
    b = (q[ok] - 128) >> 8
    nx, ny, nz = zc.S6_DIMS
    nbx, nby = (nx + 3) // 4, (ny + 3) // 4
    first = 0
    for j in (0, 1):
        for k in (0, 1):
            y, z, xb = b[:, 1] + j, b[:, 2] + k, b[:, 0] >> 2
            row = (y >= 0) & (y < ny) & (z >= 0) & (z < nz) & (xb >= 0) & (xb < nbx)
            if row.any():
                first = max(first, int(((((z >> 1) * nby + (y >> 2)) * nbx + xb) * 8 + ((y & 3) | ((z & 1) << 2)))[row].max()))
    far = b + 1
    dims = np.asarray(zc.S6_DIMS, dtype=np.int64)
    start = (dims - 1) // np.asarray([4, 4, 2]) * np.asarray([4, 4, 2])
    return dict(first_max=first, outside=int((far >= dims).any(axis=1).sum()), last=[int(((far[:, a] >= start[a]) & (b[:, a] < dims[a])).sum()) for a in range(3)])


# ---- B. registration --------------------------------------------------------------------------------------------------------------------

ROOM = (sc.ROOM["origin"], sc.ROOM["resolution"])
B_POSES = 256
B2_BAD = (3, 64, 127, 200, 255)          # the poses whose translation is out of range
B3_STRIDE, B3_ITERATIONS = 4, 25
B3_ALONE = (0, 63, 64, 127, 128, 191, 192, 255)   # two poses from each block of k_scan_step


@functools.lru_cache(maxsize=None)
def b1_steps():
    """The nine crafted rows of rc.crafted_steps() over 256 poses -> (records (256,32), state (256,64), kind (256,): the crafted row
    each pose copies).  Each run of 64 poses — a block of k_scan_step — holds all nine in a seeded order; every pose's trial
    translation is moved by its own 1e-5 m multiple, so that no two rows are alike."""
    records, state = rc.crafted_steps()
    rng = np.random.default_rng(9500)
    wave = limits()["wave"]
    kind = np.concatenate([rng.permutation(np.concatenate([np.tile(np.arange(9), wave // 9), rng.integers(0, 9, wave % 9)])) for _ in range(B_POSES // wave)])
    state = state[kind].copy()
    state.view(np.float64)[:, synth.SR_TRIAL_T:synth.SR_TRIAL_T + 3] += 1.0e-5 * np.arange(B_POSES)[:, None]
    return _frozen(records[kind].copy(), state, kind)


@functools.lru_cache(maxsize=None)
def b1_reference():
    """-> (state (256,64) int64, poses12 rows: a list of 256, None where a pose wrote none) by synth.scan_step_ref."""
    records, state, _ = b1_steps()
    want, want12 = synth.scan_step_ref(records, state, ROOM[1])
    return _frozen(want), want12


@functools.lru_cache(maxsize=None)
def b2_inputs():
    """The room's scan with 256 starts -> (poses (256,3), quats (256,4), state (256,64) int64, poses12 (256,12) f32)."""
    poses, quats = rc.starts(B_POSES)
    state, p12 = synth.scan_register_init_ref(poses, quats)
    return _frozen(poses, quats, state, p12)


def b2_frozen_state():
    """The starting state with a scattered third of the poses frozen, by every status but RUNNING in turn."""
    state = b2_inputs()[2].copy()
    rows = np.flatnonzero((np.arange(B_POSES) * 7) % 3 == 0)
    state[rows, synth.SR_STATUS] = 1 + np.arange(len(rows)) % 4
    return state, rows


def b2_bad_poses():
    p12 = b2_inputs()[3].copy()
    p12[list(B2_BAD), 9 + np.arange(len(B2_BAD)) % 3] = f32(1.0e7)
    return p12


@functools.lru_cache(maxsize=None)
def b2_reference(variant):
    """The records (256,32) by synth.scan_normal_ref: 'plain'; 'frozen': zero for the poses of b2_frozen_state; 'bad': with
    b2_bad_poses."""
    L, P = rc.room()
    p12 = b2_bad_poses() if variant == "bad" else b2_inputs()[3]
    rec = synth.scan_normal_ref(L, *ROOM, P, p12)
    if variant == "frozen":
        rec[b2_frozen_state()[1]] = 0
    return _frozen(rec)


def b2_plan(n, B=B_POSES):
    """CONDITION of B2 -> (per: tile blocks a pose, the fewest tiles a block walks)."""
    lim = limits()
    n_tiles = -(-n // lim["block"])
    per = min(-(-lim["scan_blocks"] // B), n_tiles)
    return per, min(len(range(x, n_tiles, per)) for x in range(per))


def b3_points():
    return rc.room()[1][::B3_STRIDE]


@functools.lru_cache(maxsize=None)
def b3_reference(iterations=B3_ITERATIONS):
    """The state (256,64) after `iterations` rounds over every fourth point of the room's scan, by synth.scan_register_ref."""
    poses, quats = b2_inputs()[:2]
    return _frozen(synth.scan_register_ref(rc.room()[0], *ROOM, b3_points(), poses, quats, iterations))


# ---- C. the pose graph --------------------------------------------------------------------------------------------------------------------

C2_NODES, C2_HUB, C2_PARTNERS, C2_DUPLICATES = 1100, 7, 985, 40
C2_CG = 4     # conjugate-gradient iterations a solve of the 30-iteration run (the restatement takes 64 ms for one on this graph)


@functools.lru_cache(maxsize=None)
def c1_case():
    """70 000 nodes and 70 399 edges, neither a multiple of 256: 274 blocks of nodes, 275 of edges."""
    return pc._loop("loop_70000_400_closures", 35000, 2, 400, 13)


@functools.lru_cache(maxsize=None)
def c2_case():
    """1 100 nodes.  Node 7, the hub, has 1 025 relative edges — to 985 partners, 40 of them twice — in which it is a and b in turn,
    and three absolute edges: a CSR row of 1 028 entries, longer than a block, behind the rows of nodes 0 .. 6.  The other 114 nodes
    hang off the partners in chains."""
    others = [i for i in range(C2_NODES) if i != C2_HUB]
    partners, rest = others[:C2_PARTNERS], others[C2_PARTNERS:]
    chain = [(partners[i % 7] if i < 7 else rest[i - 7], r) for i, r in enumerate(rest)]
    hub = [(C2_HUB, p) if k % 2 == 0 else (p, C2_HUB) for k, p in enumerate(partners + partners[100:100 + C2_DUPLICATES])]
    return pc._graph("hub_1028", 21, C2_NODES, chain[:50] + hub + chain[50:], absolute=(C2_HUB,) * 3, fixed=(0,), cg_iterations=C2_CG)


def c_reference_stages(c, cg_iterations):
    """-> (rec, (D, grad, cost), the conjugate-gradient answer) of the restatement at the case's start."""
    mask, n = pc.free_mask(c), len(c["t"])
    rec = synth.pose_graph_linearize_ref(c["t"], c["q"], c["ab"], c["zt"], c["zq"], c["omega"], mask, c["robust"])
    D, grad, cost = synth.pose_graph_gather_ref(rec, c["ab"], n, mask)
    cg = synth.pose_graph_cg_ref(D, grad, rec, c["ab"], synth.POSEGRAPH_LAMBDA0, mask, cg_iterations, 1e-8, 1e-5, 1e-6)
    return rec, (D, grad, cost), cg


@functools.lru_cache(maxsize=None)
def c1_reference():
    c = c1_case()
    stages = c_reference_stages(c, 10)
    s = synth.pose_graph_optimize_ref(c["t"], c["q"], c["ab"], c["zt"], c["zq"], c["omega"], fixed=c["fixed"], iterations=2, cg_iterations=10)
    return stages, s


@functools.lru_cache(maxsize=None)
def c2_reference():
    c = c2_case()
    stages = c_reference_stages(c, 10)
    shots = synth.pose_graph_optimize_ref(c["t"], c["q"], c["ab"], c["zt"], c["zq"], c["omega"], fixed=c["fixed"], iterations=max(pc.SNAPSHOTS),
                                          cg_iterations=c["cg_iterations"], snapshots=pc.SNAPSHOTS)
    return stages, shots


def pg_layout_ref(n, e, scalars):
    """pg_layout restated: the workspace's seventeen offsets in 8-byte words, the last the total."""
    lim = limits()
    nbn, nbe = -(-n // lim["block"]), -(-e // lim["block"])
    size = [3 * scalars, 8 * n, 6 * n, 2 * e * synth.POSEGRAPH_EDGE, 2 * n * lim["pg_node"], 21 * n, 6 * n, 6 * n, 12 * n, 6 * n, nbe, nbn, nbn, nbn,
            nbn, 2]
    return [int(v) for v in np.concatenate([[0], np.cumsum(np.asarray(size, dtype=np.int64))])]
