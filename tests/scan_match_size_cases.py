"""The seeded inputs shared by the two tests of scan matching at capacity and on the largest grid (tests/test_scan_match_at_size_cpu.py
without a GPU, tests/test_hip_scan_match_at_size.py on one) and what the numpy restatements of synth say of them, computed once per
process and never modified.  Numpy only.

S1  tiles of exactly 256 points in range over maps whose table bytes are 255: every 16-bit field of k_scan_correlate at 65 280.
S2  a grid 51 bricks long: the one-address fast path of the span load at all four byte shifts, and the slow path on either side.
S3  K = 256 rotations x the (16, 16, 4) window = 2 509 056 candidates: correlate and best next to the cap of 2^22.
S4  2^20 + 4097 explicit candidates: more than the 2^20 blocks k_scan_score's grid gets along x.
S5  a scan of 2^22 points, the cap.
S6  the (2047, 2045, 511) grid of tests/map_size_cases.py through the window in its far corner.

The caps and tiles are read from the kernel's text (limits())."""
import functools
import os
import re

import numpy as np

import map_size_cases as mc
import scan_match_cases as sc

from trajectory_optimization_amd import synth

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trajectory_optimization_amd", "csrc")
PARAMS = sc.PARAMS   # lmin = -127, lmax = 127: the map takes every value


@functools.lru_cache(maxsize=None)
def limits():
    """The caps and tiles of scanmatch_kernels.hip, read from its text (an assertion names the pattern that is gone)."""
    text = {name: open(os.path.join(CSRC, name)).read() for name in ("common.hpp", "scanmatch_kernels.hip")}

    def one(name, pattern):
        m = re.search(pattern, text[name])
        assert m, (name, pattern)
        return int(m.group(1)) if m.groups() else None

    k = "scanmatch_kernels.hip"
    return dict(
        block=one("common.hpp", r"#define TO_BLOCK\s+(\d+)"),
        max_wxy=one(k, r"constexpr int kScanMaxWxy = (\d+);"),
        max_wz=one(k, r"constexpr int kScanMaxWz = (\d+);"),
        max_k=one(k, r"constexpr int kScanMaxK = (\d+);"),
        max_points=1 << one(k, r"constexpr long long kScanMaxPoints = 1ll << (\d+);"),
        max_candidates=1 << one(k, r"constexpr long long kScanMaxCandidates = 1ll << (\d+);"),
        blocks=one(k, r"constexpr int kScanBlocks = (\d+);"),
        score_grid_x=1 << one(k, r"const dim3 grid\(\(unsigned\)\(b < \(1ll << (\d+)\) \? b : \(1ll << \1\)\),"),
        best_block=one(k, r"constexpr int kScanBestBlock = (\d+);"),
    )


def window_plan(window):
    """How k_scan_correlate splits a window -> dict(S, rows, split, G): rows = (2wy+1)(2wz+1), split = max(1, block / rows) shares
    of a tile's points per row, G = ceil((2wx+1) / 4) groups of four along x."""
    wx, wy, wz = window
    rows, block = (2 * wy + 1) * (2 * wz + 1), limits()["block"]
    return dict(S=(2 * wx + 1) * rows, rows=rows, split=1 if rows >= block else block // rows, G=(2 * wx + 1 + 3) // 4)


def word_index(v, dims):
    """The brick word of voxels (...,3) inside dims, in int64."""
    nbx, nby = (int(dims[0]) + 3) // 4, (int(dims[1]) + 3) // 4
    v = np.asarray(v, dtype=np.int64)
    return ((v[..., 2] >> 1) * nby + (v[..., 1] >> 2)) * nbx + (v[..., 0] >> 2)


def byte_offsets(v, dims):
    """The offset of voxels (...,3) inside dims in an evidence buffer or a score table, in int64: 256 + 32 word + bit."""
    v = np.asarray(v, dtype=np.int64)
    return 256 + 32 * word_index(v, dims) + ((v[..., 0] & 3) | ((v[..., 1] & 3) << 2) | ((v[..., 2] & 1) << 4))


def centre_points(vox, origin=sc.ORIGIN, res=sc.RES, t=sc.T):
    """Sensor-frame points on the centres of voxels (n,3) for the identity rotation and translation t (dyadic: no rounding)."""
    p = np.asarray(origin, dtype=np.float64) + res * (np.asarray(vox, dtype=np.float64) + 0.5) - np.asarray(t, dtype=np.float64)
    assert np.array_equal(p.astype(f32).astype(np.float64), p)
    return p.astype(f32)


# ---- the restatement's body on voxels already computed --------------------------------------------------------------------------------

def correlate_from_voxels(V, v, ok, window, unknown_value, chunk=2048):
    """The body of synth.scan_correlate_ref for one rotation whose voxels are computed already (synth.scan_voxels_ref) and a value
    volume V that covers only part of the grid: v (N,3) are voxel indices RELATIVE TO V's first voxel, ok (N,) the points that take
    part; everything outside V is unknown_value -> (scores (2wz+1, 2wy+1, 2wx+1) int64, used)."""
    V = np.asarray(V, dtype=np.int64)
    w = np.asarray([int(c) for c in window], dtype=np.int64)
    dims = np.asarray(V.shape, dtype=np.int64)
    pad = np.full(tuple(dims + 4 * w), int(unknown_value), dtype=np.int64)
    pad[2 * w[0]:2 * w[0] + dims[0], 2 * w[1]:2 * w[1] + dims[1], 2 * w[2]:2 * w[2] + dims[2]] = V
    views = np.lib.stride_tricks.sliding_window_view(pad, tuple(2 * w + 1))
    v = np.asarray(v, dtype=np.int64)[np.asarray(ok, dtype=bool)]
    near = ((v >= -w) & (v < dims + w)).all(axis=1)
    acc = np.full(tuple(2 * w + 1), int(unknown_value) * int((~near).sum()), dtype=np.int64)
    b = v[near] + w
    for i in range(0, len(b), chunk):
        c = b[i:i + chunk]
        acc += views[c[:, 0], c[:, 1], c[:, 2]].sum(axis=0)
    return acc.transpose(2, 1, 0), len(v)


def score_from_voxels(lookup, dims, v, ok, shifts, floor, unknown_value):
    """The body of synth.scan_score_ref, vectorised over shifts (B,3), for voxels computed already -> (B,4) int64 rows (score, used,
    inside, known).  lookup: voxels (m,3) inside dims -> their log-odds (m,) int64; dims: the grid's true dims."""
    v = np.asarray(v, dtype=np.int64)[np.asarray(ok, dtype=bool)]
    shifts = np.asarray(shifts, dtype=np.int64).reshape(-1, 3)
    fl = -127 if floor is None else int(floor)
    out = np.zeros((len(shifts), 4), dtype=np.int64)
    out[:, 1] = len(v)
    if not len(v):
        return out
    vs = v[None, :, :] + shifts[:, None, :]
    ins = ((vs >= 0) & (vs < np.asarray(dims, dtype=np.int64))).all(axis=2)
    L = np.full(ins.shape, synth.EVID_UNKNOWN, dtype=np.int64)
    L[ins] = lookup(vs[ins])
    known = L != synth.EVID_UNKNOWN
    out[:, 0] = np.where(known, np.maximum(L, fl), int(unknown_value)).sum(axis=1)
    out[:, 2], out[:, 3] = ins.sum(axis=1), known.sum(axis=1)
    return out


def dense_lookup(L):
    L = np.asarray(L, dtype=np.int64)
    return lambda vox: L[vox[:, 0], vox[:, 1], vox[:, 2]]


# ---- S1. full fields --------------------------------------------------------------------------------------------------------------------

S1_DIMS = (56, 48, 16)
S1_BASE = ((16, 40), (16, 32), (4, 12))     # the base voxels' box: every shift of (16, 16, 4) stays inside dims
S1_TILES = 3
S1_WINDOWS = ((16, 16, 4), (16, 7, 4), (14, 5, 4), (3, 0, 0))
S1_MAPS = ("full", "stripes")


def s1_log_odds(name):
    """'full': 127 everywhere (every table byte 255); 'stripes': 127 at even x, -127 at odd x (bytes 255 and 1, no floor)."""
    L = np.full(S1_DIMS, 127, dtype=np.int64)
    if name == "stripes":
        L[1::2] = -127
    return L


@functools.lru_cache(maxsize=None)
def s1_voxels():
    """256 x 3 base voxels in S1_BASE, in the scan's order: a tile of even x, a tile of odd x, a tile of either — so that under
    'stripes' the first tile's fields hold 256 x 255 at even dx and 256 x 1 at odd dx, the second's the other way round."""
    rng = np.random.default_rng(8101)
    n = limits()["block"] * S1_TILES
    v = np.stack([rng.integers(lo, hi, n) for lo, hi in S1_BASE], axis=1)
    tile = np.arange(n) // limits()["block"]
    v[:, 0] = np.where(tile == 0, v[:, 0] & ~1, np.where(tile == 1, v[:, 0] | 1, v[:, 0]))
    return v


def s1_points():
    return centre_points(s1_voxels())


@functools.lru_cache(maxsize=None)
def s1_reference(name, window):
    """-> (scores (1, 2wz+1, 2wy+1, 2wx+1) int32, used (1,) int32) by synth.scan_correlate_ref."""
    R = [synth.scan_rotation(sc.rotations(1)[0])]
    return synth.scan_correlate_ref(s1_log_odds(name), sc.ORIGIN, sc.RES, s1_points(), R, sc.T, window)


# ---- S2. the fast path at every shift -----------------------------------------------------------------------------------------------------

S2_DIMS = (203, 6, 3)
S2_N = 4000   # (1000 points leave about 1000 x 8/12 x 1/3 x 0.8 / 4 = 44 per byte shift on the fast path: fewer than the 100 asked)
S2_WINDOWS = ((16, 1, 0), (14, 1, 0), (12, 1, 0), (7, 1, 0))
S2_SEED, S2_FLOOR, S2_UNKNOWN = 21, -10, -8


def s2_inputs():
    """-> (L, points (n,3) f32, quats (2,4)): random log-odds, sc.random_scan's points and special rows, the identity and a yaw."""
    return sc.random_log_odds(S2_DIMS, S2_SEED), sc.random_scan(S2_DIMS, S2_N, S2_SEED), sc.rotations(2)


@functools.lru_cache(maxsize=None)
def s2_reference(window):
    L, pts, quats = s2_inputs()
    Rs = [synth.scan_rotation(q) for q in quats]
    return synth.scan_correlate_ref(L, sc.ORIGIN, sc.RES, pts, Rs, sc.T, window, S2_FLOOR, S2_UNKNOWN)


def s2_paths(window):
    """Which path of the span load the identity rotation's points take -> (fast (4,) counts per (x - wx) & 3, slow_left, slow_right):
    points in range with at least one row (dy, dz) of the window inside dims; fast: 0 <= xb and xb + G < nbx for xb = (x - wx) >> 2;
    slow_left: xb < 0; slow_right: xb + G >= nbx."""
    L, pts, quats = s2_inputs()
    v, ok = synth.scan_voxels_ref(pts, synth.scan_rotation(quats[0]), sc.T, sc.ORIGIN, sc.RES)
    v = v[ok]
    wx, wy, wz = window
    nx, ny, nz = S2_DIMS
    row = (v[:, 1] + wy >= 0) & (v[:, 1] - wy < ny) & (v[:, 2] + wz >= 0) & (v[:, 2] - wz < nz)
    xs = v[row, 0] - wx
    xb, G, nbx = xs >> 2, window_plan(window)["G"], (nx + 3) // 4
    fast = (xb >= 0) & (xb + G < nbx)
    return np.bincount(xs[fast] & 3, minlength=4), int((xb < 0).sum()), int((xb + G >= nbx).sum())


# ---- S3. the caps of K S ----------------------------------------------------------------------------------------------------------------

S3_DIMS, S3_WINDOW, S3_K, S3_N = (37, 29, 9), (16, 16, 4), 256, 48
S3_SEED, S3_FLOOR, S3_UNKNOWN = 31, -10, -8
S3_RANGE = 7   # the random scores of the second set come from {0 .. 6}


def s3_quats():
    """256 yaws in steps of 0.2 degrees around the identity, which is row 128."""
    return np.stack([sc.yaw_quat(np.deg2rad(0.2) * (k - S3_K // 2)) for k in range(S3_K)])


def s3_inputs():
    return sc.random_log_odds(S3_DIMS, S3_SEED), sc.random_scan(S3_DIMS, S3_N, S3_SEED), s3_quats()


@functools.lru_cache(maxsize=None)
def s3_reference():
    """-> (scores (256, 9, 33, 33) int32, used (256,), best int32[8])."""
    L, pts, quats = s3_inputs()
    Rs = [synth.scan_rotation(q) for q in quats]
    scores, used = synth.scan_correlate_ref(L, sc.ORIGIN, sc.RES, pts, Rs, sc.T, S3_WINDOW, S3_FLOOR, S3_UNKNOWN)
    return scores, used, synth.scan_best_ref(scores)


@functools.lru_cache(maxsize=None)
def s3_tied_scores():
    """Random scores from {0 .. 6} of shape (256, 9, 33, 33): a seventh of them share the maximum.  No candidate within one voxel of
    the centre holds it, in any rotation, but (dx, dy, dz) = (-1, 0, 0) and (+1, 0, 0) of the LAST rotation: the smallest |s|^2 among
    the maxima is theirs, twice, and the lower flat index — above 2^21 — decides -> (scores int32, best int32[8] by scan_best_ref)."""
    wx, wy, wz = S3_WINDOW
    s = np.random.default_rng(8303).integers(0, S3_RANGE, (S3_K, 2 * wz + 1, 2 * wy + 1, 2 * wx + 1)).astype(np.int32)
    top = S3_RANGE - 1
    for dx, dy, dz in ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        cell = s[:, wz + dz, wy + dy, wx + dx]
        cell[cell == top] = top - 1
    s[-1, wz, wy, wx - 1] = s[-1, wz, wy, wx + 1] = top
    return s, synth.scan_best_ref(s)


# ---- S4. candidates beyond 2^20 -----------------------------------------------------------------------------------------------------------

S4_DIMS = (13, 10, 5)
S4_SEED, S4_FLOOR, S4_UNKNOWN = 41, -20, -5
S4_POSES = 5


def s4_count():
    return limits()["score_grid_x"] + 4097


@functools.lru_cache(maxsize=None)
def s4_inputs():
    """-> dict(L, points (7,3), quats (5,4), trans (5,3), pose_of (B,), shifts (B,3) int64).  The points under pose 0: three on voxel
    centres inside dims, one in the apron, one NaN, one out of range, one exactly on a voxel corner inside dims."""
    B = s4_count()
    o = np.asarray(sc.ORIGIN, dtype=np.float64)
    pts = np.concatenate([centre_points([(2, 3, 1), (7, 5, 2), (12, 9, 4), (-2, 4, 2)]),
                          f32([[np.nan, 0.0, 0.0], [1.0e6, 0.0, 0.0]]),
                          (o + sc.RES * np.array([5.0, 5.0, 2.0]) - np.asarray(sc.T))[None].astype(f32)])
    quats = np.stack([sc.rotations(3)[0], sc.rotations(3)[1], sc.rotations(3)[2], sc.yaw_quat(-0.2), sc.rotations(3)[0]])
    trans = np.asarray(sc.T)[None, :] + sc.RES * np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, -1, 0], [-1, 2, 1]], dtype=np.float64)
    rng = np.random.default_rng(8400 + S4_SEED)
    shifts = rng.integers(-3, 4, (B, 3)).astype(np.int64)
    big = 2 ** 31 - 1
    far = np.array([[big, 0, 0], [0, -big - 1, 0], [big, big, -big - 1], [0, 0, big]], dtype=np.int64)
    rows = np.arange(0, B, 1000)
    shifts[rows] = far[np.arange(len(rows)) % len(far)]
    return dict(L=sc.random_log_odds(S4_DIMS, S4_SEED), points=pts, quats=quats, trans=trans, pose_of=np.arange(B) % S4_POSES, shifts=shifts)


@functools.lru_cache(maxsize=None)
def s4_reference():
    """(B,4) int64 rows (score, used, inside, known): per distinct pose, score_from_voxels over all of its shifts."""
    c = s4_inputs()
    out = np.zeros((s4_count(), 4), dtype=np.int64)
    for j in range(S4_POSES):
        v, ok = synth.scan_voxels_ref(c["points"], synth.scan_rotation(c["quats"][j]), c["trans"][j], sc.ORIGIN, sc.RES)
        rows = np.flatnonzero(c["pose_of"] == j)
        out[rows] = score_from_voxels(dense_lookup(c["L"]), S4_DIMS, v, ok, c["shifts"][rows], S4_FLOOR, S4_UNKNOWN)
    return out


def s4_sample():
    """64 candidates: the ends, both sides of 2^20, and a seeded rest."""
    B, edge = s4_count(), limits()["score_grid_x"]
    keep = {0, edge - 1, edge, edge + 1, B - 1, 1000, 2000, 3000}
    rng = np.random.default_rng(8499)
    while len(keep) < 64:
        keep.add(int(rng.integers(0, B)))
    return np.array(sorted(keep))


# ---- S5. the largest scan -----------------------------------------------------------------------------------------------------------------

S5_DIMS, S5_WINDOW = (37, 29, 9), (1, 0, 0)


def s5_log_odds():
    """127 where x + y + z is even, 126 where it is odd; no voxel unknown."""
    x, y, z = np.meshgrid(*(np.arange(d) for d in S5_DIMS), indexing="ij")
    return np.where((x + y + z) % 2 == 0, 127, 126).astype(np.int64)


@functools.lru_cache(maxsize=None)
def s5_points():
    """2^22 points uniform over the box and one voxel of apron, a seeded 0.1 % of them out of range."""
    n = limits()["max_points"]
    rng = np.random.default_rng(8500)
    o, d = np.asarray(sc.ORIGIN, dtype=f32), np.asarray(S5_DIMS, dtype=f32)
    P = o - f32(sc.RES) + rng.random((n, 3), dtype=f32) * ((d + 2) * f32(sc.RES)) - np.asarray(sc.T, dtype=f32)
    P[rng.random(n) < 0.001] = f32([1.0e6, 0.0, 0.0])
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def s5_reference():
    """-> (scores (1, 1, 1, 3) int32, used (1,) int32, rows (3,4) int64 of (score, used, inside, known) at the three shifts)."""
    L, P = s5_log_odds(), s5_points()
    R = synth.scan_rotation(sc.rotations(1)[0])
    scores, used = synth.scan_correlate_ref(L, sc.ORIGIN, sc.RES, P, [R], sc.T, S5_WINDOW, chunk=1 << 16)
    v, ok = synth.scan_voxels_ref(P, R, sc.T, sc.ORIGIN, sc.RES)
    rows = np.concatenate([score_from_voxels(dense_lookup(L), S5_DIMS, v, ok, s[None], None, 0) for s in sc.window_shifts(S5_WINDOW)])
    return scores, used, rows


# ---- S6. the largest grid through a window ------------------------------------------------------------------------------------------------

S6_DIMS, S6_WIN = mc.BIG_DIMS, mc.BIG_WINDOW
S6_OFF = np.asarray(S6_DIMS, dtype=np.int64) - np.asarray(S6_WIN, dtype=np.int64)
S6_WINDOWS = ((16, 16, 4), (3, 5, 1))
S6_SEED, S6_FLOOR, S6_UNKNOWN = 61, -10, -8
S6_FIRST = 70                                             # the value of voxel (0, 0, 0): word 0 is not all-unknown
S6_CENTRE = (S6_OFF + np.asarray(S6_WIN) // 2) * 256 + 128   # the rotation centre in fixed point: a voxel centre inside the window
S6_K = 3


@functools.lru_cache(maxsize=None)
def s6_window_log_odds():
    """The window's log-odds (64, 64, 32): random, the grid's last voxel 127."""
    L = sc.random_log_odds(S6_WIN, S6_SEED).copy()
    L[-1, -1, -1] = 127
    L.setflags(write=False)
    return L


def s6_lookup(vox):
    """The log-odds of voxels (m,3) inside S6_DIMS: the window's, 70 at (0, 0, 0), never observed elsewhere."""
    vox = np.asarray(vox, dtype=np.int64)
    out = np.full(len(vox), synth.EVID_UNKNOWN, dtype=np.int64)
    w = vox - S6_OFF
    inw = (w >= 0).all(axis=1)
    Lw = s6_window_log_odds()
    out[inw] = Lw[w[inw, 0], w[inw, 1], w[inw, 2]]
    out[(vox == 0).all(axis=1)] = S6_FIRST
    return out


@functools.lru_cache(maxsize=None)
def s6_points():
    """Sensor-frame points for the translation S6_CENTRE, on the 1/2048 m lattice -> (n,3) f32: 3000 with base voxels over the window
    and eight voxels of the far apron (a tenth of them on voxel faces), 8 in the voxels (0..1)^3 and 4 out of range."""
    rng = np.random.default_rng(8600 + S6_SEED)
    q = rng.integers(S6_OFF * 256, np.asarray(S6_DIMS) * 256 + 8 * 256, size=(3000, 3))
    snap = rng.random(3000) < 0.1
    q[snap] = (q[snap] >> 8) << 8
    first = np.array([[128 + 256 * i, 128 + 256 * j, 128 + 256 * k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.int64)
    q = np.concatenate([q, first])
    assert np.abs(q - S6_CENTRE).max() < 1 << 24
    P = ((q - S6_CENTRE).astype(np.float64) / 2048.0).astype(f32)
    c = S6_CENTRE.astype(np.float64) / 2048.0
    out = (np.array([[600.0, 1.0, 1.0], [1.0, -300.0, 1.0], [1.0, 1.0, 520.0], [-257.0, 1.0, 1.0]]) - c).astype(f32)
    P = np.concatenate([P, out])
    P.setflags(write=False)
    return P


def s6_translation():
    return (S6_CENTRE.astype(np.float64) / 2048.0).astype(f32)


@functools.lru_cache(maxsize=None)
def s6_voxels():
    """Per rotation of sc.rotations(3): (voxels (n,3) int64 in the full grid's numbering, ok (n,)) from the true origin and translation."""
    return tuple(synth.scan_voxels_ref(s6_points(), synth.scan_rotation(q), s6_translation(), mc.ORIGIN, mc.RES) for q in sc.rotations(S6_K))


@functools.lru_cache(maxsize=None)
def s6_reference(window):
    """-> (scores (3, 2wz+1, 2wy+1, 2wx+1) int32, used (3,) int32): correlate_from_voxels on the window's values with the voxels
    shifted by -S6_OFF, plus what voxel (0, 0, 0) adds over unknown_value (a second volume of one voxel: the score is a sum)."""
    V = synth.scan_values_ref(s6_window_log_odds(), S6_FLOOR, S6_UNKNOWN)
    V0 = np.full((1, 1, 1), max(S6_FIRST, S6_FLOOR) - S6_UNKNOWN, dtype=np.int64)
    scores, used = [], []
    for v, ok in s6_voxels():
        a, n = correlate_from_voxels(V, v - S6_OFF, ok, window, S6_UNKNOWN)
        b, _ = correlate_from_voxels(V0, v, ok, window, 0)
        scores.append(a + b)
        used.append(n)
    return np.stack(scores).astype(np.int32), np.asarray(used, dtype=np.int32)


def s6_candidates(window):
    """32 sampled candidates and the window's corners in the first and last rotation -> (k (m,), flat shift index (m,))."""
    S = window_plan(window)["S"]
    rng = np.random.default_rng(8650 + window[0])
    flat = set(rng.choice(S6_K * S, 32, replace=False).tolist())
    wx, wy, wz = window
    for k in (0, S6_K - 1):
        for iz in (0, 2 * wz):
            for iy in (0, 2 * wy):
                for ix in (0, 2 * wx):
                    flat.add(k * S + (iz * (2 * wy + 1) + iy) * (2 * wx + 1) + ix)
    flat = np.array(sorted(flat))
    return flat // S, flat % S


@functools.lru_cache(maxsize=None)
def s6_score_reference(window):
    """(m,4) int64 rows (score, used, inside, known) of s6_candidates(window); inside is tested against the true dims."""
    ks, ss = s6_candidates(window)
    shifts = sc.window_shifts(window)
    out = np.zeros((len(ks), 4), dtype=np.int64)
    for k, (v, ok) in enumerate(s6_voxels()):
        rows = np.flatnonzero(ks == k)
        out[rows] = score_from_voxels(s6_lookup, S6_DIMS, v, ok, shifts[ss[rows]], S6_FLOOR, S6_UNKNOWN)
    return out


def s6_spans(window):
    """What the identity rotation's points meet on the largest grid -> dict(far_x, far_y, far_z: points whose window leaves dims through
    that far face while some of it lies inside; inside: points whose whole window lies inside dims; max_word: the largest brick word
    any of their lookups falls in)."""
    v, ok = s6_voxels()[0]
    v, w, d = v[ok], np.asarray(window, dtype=np.int64), np.asarray(S6_DIMS, dtype=np.int64)
    touches = ((v + w >= 0) & (v - w < d)).all(axis=1)
    far = [int((touches & (v[:, a] + w[a] >= d[a])).sum()) for a in range(3)]
    whole = ((v - w >= 0) & (v + w < d)).all(axis=1)
    last = np.minimum(v[touches] + w, d - 1)   # the farthest voxel of a window that lies inside dims
    return dict(far_x=far[0], far_y=far[1], far_z=far[2], inside=int(whole.sum()), max_word=int(word_index(last, S6_DIMS).max()))


def s6_map_bytes():
    """What the test writes into the fresh evidence buffer -> (offsets (m,) int64, values (m,) uint8): the window's bytes and voxel
    (0, 0, 0), by the documented layout."""
    win = np.argwhere(np.ones(S6_WIN, dtype=bool)) + S6_OFF
    vox = np.concatenate([win, [[0, 0, 0]]])
    return byte_offsets(vox, S6_DIMS), s6_lookup(vox).astype(np.int8).view(np.uint8)


def s6_table_check():
    """The table's bytes over the window and a one-voxel rim inside dims -> (offsets (m,) int64, bytes (m,) uint8 by scan_values_ref)."""
    lo, hi = S6_OFF - 1, np.asarray(S6_DIMS, dtype=np.int64)
    vox = np.argwhere(np.ones(tuple(hi - lo), dtype=bool)) + lo
    return byte_offsets(vox, S6_DIMS), (synth.scan_values_ref(s6_lookup(vox), S6_FLOOR, S6_UNKNOWN) + 128).astype(np.uint8)


def s6_last_word():
    """The table's last 32 bytes: brick (511, 511, 255) = voxels (2044 .. 2047, 2044 .. 2047, 510 .. 511), most of them pad."""
    x, y, z = np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing="ij")
    vox = np.stack([x, y, z], axis=-1).reshape(-1, 3) + np.array([2044, 2044, 510])
    inside = (vox < np.asarray(S6_DIMS)).all(axis=1)
    L = np.full(len(vox), synth.EVID_UNKNOWN, dtype=np.int64)
    L[inside] = s6_lookup(vox[inside])
    out = np.zeros(32, dtype=np.uint8)
    out[(vox[:, 0] & 3) | ((vox[:, 1] & 3) << 2) | ((vox[:, 2] & 1) << 4)] = (synth.scan_values_ref(L, S6_FLOOR, S6_UNKNOWN) + 128).astype(np.uint8)
    return out, int(inside.sum())


# ---- S6 moved to the origin: the case's own shifting arithmetic ---------------------------------------------------------------------------

S6_SMALL_MARGIN = np.array([32, 32, 32], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def s6_small(window):
    """The window's content and the 3000 points on a (64 + 32, 64 + 32, 32 + 32) grid at the origin, identity rotation: the window sits
    in that grid's far corner as it does in the largest grid's, and the margin is wider than the search window -> (scores, used) by
    synth.scan_correlate_ref, and the rows of s6_candidates(window) with k = 0 by synth.scan_score_ref."""
    dims = tuple(int(c) for c in np.asarray(S6_WIN) + S6_SMALL_MARGIN)
    L = np.full(dims, synth.EVID_UNKNOWN, dtype=np.int64)
    m = S6_SMALL_MARGIN
    L[m[0]:, m[1]:, m[2]:] = s6_window_log_odds()
    move = (S6_OFF - m) * 256
    P = s6_points()[:3000]
    t = ((S6_CENTRE - move).astype(np.float64) / 2048.0).astype(f32)
    R = synth.scan_rotation(sc.rotations(1)[0])
    scores, used = synth.scan_correlate_ref(L, mc.ORIGIN, mc.RES, P, [R], t, window, S6_FLOOR, S6_UNKNOWN)
    ks, ss = s6_candidates(window)
    shifts = sc.window_shifts(window)
    rows = [synth.scan_score_ref(L, mc.ORIGIN, mc.RES, P, R, t, shifts[s], S6_FLOOR, S6_UNKNOWN) for s in ss[ks == 0]]
    return scores, used, np.asarray(rows, dtype=np.int64)
