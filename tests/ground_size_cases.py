"""The seeded inputs shared by the two tests of the ground layer at size (tests/test_ground_at_size_cpu.py without a GPU,
tests/test_hip_ground_at_size.py on one) and what synth.ground_ref / ground_snap_ref say of them, computed once per process and never
modified.  Numpy only.

G1  tall columns: (5, 6, 511) with a solid block 501 voxels high — a floor run of 250 brick words — next to two columns broken on
    either side of the word boundary z = 255 | 256; (9, 9, 130) with slabs 64, 65 and 66 levels above two floors, H = 64.
G2  the (2047, 2045, 511) grid of tests/map_size_cases.py through the window in its far corner: word indices next to 2^26, brick
    masks at far edges that are no brick multiple."""
import functools

import numpy as np

import map_size_cases as mc
from map_size_cases import ORIGIN, RES

from trajectory_optimization_amd import synth

f32 = np.float32
PLANES = ("support", "ground", "obstacles", "drive")
G1_SETTINGS = ((64, 0), (64, 4), (3, 2), (1, 0))

# ---- G1. tall columns -----------------------------------------------------------------------------------------------------------------------

TALL_DIMS, TALL_TOP = (5, 6, 511), 500
TALL_A, TALL_B = (1, 2), (3, 3)           # interior columns, broken at z = 255 (the upper level of word 127) and z = 256 (word 128)
TALL_SOLID = (2, 2)
SLAB_DIMS = (9, 9, 130)


def tall_scene():
    """-> (occ, free): every column solid from z = 0 to 500, column A free at z = 255, column B at z = 256; everything else is known
    free but one voxel two levels above the block's top."""
    occ = np.zeros(TALL_DIMS, dtype=bool)
    occ[:, :, :TALL_TOP + 1] = True
    occ[TALL_A[0], TALL_A[1], 255] = False
    occ[TALL_B[0], TALL_B[1], 256] = False
    free = ~occ
    free[0, 5, TALL_TOP + 2] = False
    return occ, free


def slab_scene():
    """-> (occ, free): a floor at z = 0, raised to z = 1 where y >= 5; a slab at z = 66 over x < 4 and one at z = 65 over x > 4.  With
    H = 64 the floor voxel (x, y, 0) needs levels 1 .. 64 clear — met under both slabs — and (x, y, 1) levels 2 .. 65: met exactly
    under the slab at 66, missed by one under the slab at 65.  One voxel under the higher slab is unknown."""
    occ = np.zeros(SLAB_DIMS, dtype=bool)
    occ[:, :, 0] = True
    occ[:, 5:, 1] = True
    occ[:4, :, 66] = True
    occ[5:, :, 65] = True
    free = ~occ
    free[1, 2, 30] = False
    return occ, free


SCENES = {"tall": tall_scene, "slabs": slab_scene}


@functools.lru_cache(maxsize=None)
def g1_reference(scene, H, s, unknown):
    occ, free = SCENES[scene]()
    return synth.ground_ref(occ, free, H, s, unknown)


# ---- G2. the largest grid through the window ------------------------------------------------------------------------------------------------

G2_DIMS, G2_WIN = mc.BIG_DIMS, mc.BIG_WINDOW
G2_OFF = np.asarray(G2_DIMS, dtype=np.int64) - np.asarray(G2_WIN, dtype=np.int64)
G2_SETTINGS = ((5, 1, "free"), (5, 1, "obstacle"), (64, 4, "free"))
G2_DROPS = (0, 5, 2048)
G2_N = 2000


def window_scene():
    """The window's occupied voxels (64, 64, 32) in its own numbering: a floor two voxels thick, a ramp of one level per two voxels
    along x that ends in a brink, a thin table and a pit through the floor."""
    occ = np.zeros(G2_WIN, dtype=bool)
    occ[:, :, :2] = True
    for x in range(20, 41):
        occ[x, 10:30, :2 + min((x - 20) // 2, 8)] = True
    occ[45:55, 40:52, 8] = True
    occ[8:12, 44:48, :2] = False
    return occ


def g2_pad(s):
    """The layers added before the window's inner faces: one on x and y, s + 2 on z (the far faces are the dims' edge)."""
    return np.array([1, 1, s + 2], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def g2_reference(H, s, unknown):
    """synth.ground_ref on the window padded by empty, unknown layers on its inner sides -> dict(planes: the five padded planes, lo:
    the padded box's first voxel in the full grid, ijk: every voxel of the padded box in C order (int64), count: {plane: the bits of
    the whole grid's plane})."""
    occ, pad = window_scene(), g2_pad(s)
    widths = tuple((int(p), 0) for p in pad)
    occ_p, free_p = np.pad(occ, widths), np.pad(~occ, widths)
    planes = synth.ground_ref(occ_p, free_p, H, s, unknown)
    lo = G2_OFF - pad
    inner = tuple(slice(int(p), None) for p in pad)
    count = {k: int(planes[k][inner].sum()) for k in PLANES}
    padding = np.ones(occ_p.shape, dtype=bool)
    padding[inner] = False
    for k in PLANES:   # nothing but unknown obstacles in the padding
        assert planes[k][padding].all() if (k == "obstacles" and unknown == "obstacle") else not planes[k][padding].any(), k
    if unknown == "obstacle":   # every voxel outside the window is unknown: an obstacle
        total, win = int(np.prod(np.asarray(G2_DIMS, dtype=np.int64))), int(np.prod(G2_WIN))
        count["obstacles"] += total - win
    return dict(planes=planes, lo=lo, ijk=np.argwhere(np.ones(occ_p.shape, dtype=bool)) + lo, count=count)


@functools.lru_cache(maxsize=None)
def g2_positions():
    """2000 positions on the 1/2048 m lattice over the window and eight voxels of the far apron, half of them in the window's lowest
    eight levels -> (n,3) f32 world."""
    rng = np.random.default_rng(9200)
    lo, hi = G2_OFF * 256, np.asarray(G2_DIMS, dtype=np.int64) * 256 + 8 * 256
    q = rng.integers(lo, hi, size=(G2_N, 3))
    low = rng.random(G2_N) < 0.5
    q[low, 2] = rng.integers(lo[2], lo[2] + 8 * 256, size=int(low.sum()))
    return mc._world(q)


@functools.lru_cache(maxsize=None)
def g2_snap(H, s, unknown, max_drop):
    """-> (standing (n,3) f32, drop (n,) int32): synth.ground_snap_ref on the padded window with the origin moved to its first voxel
    (every position lies in it or beyond the far faces; below it the grid is empty), the standing voxel's centre then taken from the
    true origin by the rule fl(origin + fl(fl(i + 0.5) r))."""
    ref, pos = g2_reference(H, s, unknown), g2_positions()
    moved = (ref["lo"].astype(np.float64) * RES).astype(f32)
    standing, drop = synth.ground_snap_ref(pos, moved, RES, ref["planes"]["ground"], ref["planes"]["drive"], max_drop)
    q, ok = synth.occ_fixed(pos, ORIGIN, RES)
    at = (q >> 8).astype(f32)
    at[:, 2] -= np.maximum(drop, 0).astype(f32)
    true = (np.asarray(ORIGIN, dtype=f32) + ((at + f32(0.5)).astype(f32) * f32(RES)).astype(f32)).astype(f32)
    true[drop < 0] = np.nan
    assert ok.all()
    return true, drop, standing
