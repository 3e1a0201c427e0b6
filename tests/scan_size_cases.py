"""The seeded inputs shared by the two tests of the view volume, the view pick and the ray casts at size (tests/test_scan_at_size_cpu.py
without a GPU, tests/test_hip_scan_at_size.py on one), the numpy restatements of them, computed once per process and never modified,
and the composition oracle of a view's revealed volume (tests/test_hip_view_volume.py uses the same one).

The sizes: (16, 16, 64) untouched = two slabs of 8192 unknown, kept voxels each, the LDS queue of k_view_volume at its capacity;
(515, 510, 73) = 610 944 brick words = 2386 slabs and a 128-word tail, more than the 2048 slab blocks a launch gets; the
(2047, 2045, 511) grid of tests/map_size_cases.py through its far-corner window; (2048, 2048, 512) = 2^31 voxels, whose far corner has
the linear index 2^31 - 1; 300 candidates and up to 100 000 gains for the pick's 256 lanes; images 8192 pixels wide or high and
65 535 views of one pixel, the launch limits of k_depth_scan.  The thresholds are read from the kernels' text (limits())."""
import functools
import os
import re
from fractions import Fraction

import numpy as np

import map_size_cases as mc
import raycast_cases as rc
from map_size_cases import ORIGIN, RES

from trajectory_optimization_amd import synth

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trajectory_optimization_amd", "csrc")
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT


@functools.lru_cache(maxsize=None)
def limits():
    """The tiles, capacities and caps of the volume and ray-cast kernels, read from their text (an assertion names the pattern that
    is gone)."""
    text = {name: open(os.path.join(CSRC, name)).read() for name in ("common.hpp", "occupancy_kernels.hip", "volume_kernels.hip", "raycast_kernels.hip")}

    def one(name, pattern):
        m = re.search(pattern, text[name])
        assert m, (name, pattern)
        return int(m.group(1)) if m.groups() else None

    block = one("common.hpp", r"#define TO_BLOCK\s+(\d+)")
    one("volume_kernels.hip", r"constexpr int kVolSlab = TO_BLOCK;")
    one("volume_kernels.hip", r"unsigned short s_queue\[kVolQueue\]")
    one("volume_kernels.hip", r"\(threadIdx\.x << 5\) \| b")
    one("volume_kernels.hip", r"i = threadIdx\.x; i < n; i \+= TO_BLOCK")
    return dict(
        block=block,
        vol_slab=block,
        vol_queue=block * one("volume_kernels.hip", r"constexpr int kVolQueue = kVolSlab \* (\d+);"),
        vol_max_slab_blocks=one("volume_kernels.hip", r"constexpr int kVolMaxSlabBlocks = (\d+);"),
        vol_max_views=one("volume_kernels.hip", r"n_views < 1 \|\| n_views > (\d+)\) return TOHIP_EINVAL;\s*if \(mark &&"),
        scan_tile=one("raycast_kernels.hip", r"constexpr int kScanTile = (\d+);"),
        scan_max_side=one("raycast_kernels.hip", r"constexpr int kScanMaxSide = (\d+);"),
        scan_max_views=one("raycast_kernels.hip", r"!flags \|\| n_views < 1 \|\| n_views > (\d+)\) return TOHIP_EINVAL;"),
        occ_max_dim=one("occupancy_kernels.hip", r"constexpr int kOccMaxDim = (\d+);"),
        occ_blocks=one("occupancy_kernels.hip", r"constexpr int kOccBlocks = (\d+);"),
    )


# ---- geometry helpers -------------------------------------------------------------------------------------------------------------

Q_PLUS_X = synth.Q_OPTICAL.astype(f32)                                                                  # the camera looks along +x
Q_PLUS_Y = synth.quat_mul(np.array([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]), synth.Q_OPTICAL).astype(f32)   # ... along +y
Q_PLUS_Z = f32([1.0, 0.0, 0.0, 0.0])                                                                    # ... along +z (camera = world axes)


def rotation(q):
    """The matrix R of a quaternion wxyz (any norm) in f64: world = R cam + t, what scan_rays_ref applies operation by operation."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64))
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def project64(points, t, q):
    """World points (N,3) -> (u, v, depth) in f64 with synth.K_INTRINS: cam = R^T (p - t), u = fx X / Z + cx, v = fy Y / Z + cy."""
    cam = (np.asarray(points, dtype=np.float64) - np.asarray(t, dtype=np.float64)) @ rotation(q)
    Kd = K.astype(np.float64)
    return Kd[0, 0] * cam[:, 0] / cam[:, 2] + Kd[0, 2], Kd[1, 1] * cam[:, 1] / cam[:, 2] + Kd[1, 2], cam[:, 2]


def frustum_box64(t, q, max_dist):
    """The f64 bounding box (lo, hi) of everything the cull can keep from pose (t, q): the apex and the four corner rays of the pixel
    rectangle widened by two pixels on every side, at depth max_dist (the kept set lies in their convex hull)."""
    Kd, R = K.astype(np.float64), rotation(q)
    pts = [np.asarray(t, dtype=np.float64)]
    for u in (-2.0, float(IW) + 2.0):
        for v in (-2.0, float(IH) + 2.0):
            cam = np.array([(u - Kd[0, 2]) / Kd[0, 0], (v - Kd[1, 2]) / Kd[1, 1], 1.0]) * float(max_dist)
            pts.append(R @ cam + np.asarray(t, dtype=np.float64))
    pts = np.array(pts)
    return pts.min(axis=0), pts.max(axis=0)


def word_index(ijk, dims):
    """The brick word of voxels (N,3) of a grid of dims: ((z >> 1) nby + (y >> 2)) nbx + (x >> 2)."""
    nbx, nby = (int(dims[0]) + 3) // 4, (int(dims[1]) + 3) // 4
    ijk = np.asarray(ijk, dtype=np.int64).reshape(-1, 3)
    return ((ijk[:, 2] >> 1) * nby + (ijk[:, 1] >> 2)) * nbx + (ijk[:, 0] >> 2)


def n_words(dims):
    return ((int(dims[0]) + 3) // 4) * ((int(dims[1]) + 3) // 4) * ((int(dims[2]) + 1) // 2)


# ---- the composition oracle of a view's revealed volume (needs a GPU) -------------------------------------------------------------

def composition_oracle(space, P, Q, limits, dev, rows=None):
    """The composition of calls that are pinned elsewhere -> (revealed masks (M, nx,ny,nz) bool on the device, kept counts list,
    unknown count): space.unknown().export() gives the centres, ops.cull_waypoints(normalize=True) the kept rows,
    tools.line_of_sight(space.occupied, t, centre, skip=(1, 0)) == 1 is counted.  rows: a list that receives, per view, (the kept
    voxels' ijk (k,3) int64, which of them are seen (k,) bool), on the device."""
    import torch
    from trajectory_optimization_amd import ops, tools
    ijk, centres = space.unknown().export()
    M = len(P)
    masks = torch.zeros((M,) + tuple(space.occupied.dims), dtype=torch.bool, device=dev)
    if not len(ijk):
        return masks, [0] * M, 0
    p, q = torch.from_numpy(np.ascontiguousarray(P)).to(dev), torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    kept_idx, _, counts, _ = ops.cull_waypoints(centres, p, q, ops.Camera(K, IW, IH, *limits), limits[0], limits[1], normalize=True)
    for w in range(M):
        kept = kept_idx[w, :counts[w]].long()
        c = centres[kept]
        see = tools.line_of_sight(space.occupied, p[w].expand_as(c).contiguous(), c, skip=(1, 0)) == 1
        v = ijk[kept].long()
        if rows is not None:
            rows.append((v, see))
        v = v[see]
        masks[w, v[:, 0], v[:, 1], v[:, 2]] = True
    return masks, counts, len(ijk)


# ---- A1. the full queue -----------------------------------------------------------------------------------------------------------

A1_DIMS, A1_LIMITS = (16, 16, 64), (0.5, 10.0)
A1_POSE, A1_QUAT = f32([[1.0, 1.0, -1.5]]), Q_PLUS_Z[None]   # on the grid's z axis, 12 voxels in front of the face z = 0, looking along +z
A1_OCCUPIED = (8, 8, 2)


def a1_claimed():
    """One voxel of every brick of A1_DIMS, a different bit from brick to brick -> (16, 16, 64) bool with 512 set."""
    bits = np.zeros(A1_DIMS, dtype=bool)
    for bz in range(32):
        for by in range(4):
            for bx in range(4):
                b = (bx + 4 * by + 16 * bz) % 32
                bits[4 * bx + (b & 3), 4 * by + ((b >> 2) & 3), 2 * bz + (b >> 4)] = True
    return bits


def a1_projection():
    """(u, v, depth, off-axis distance) in f64 of all 16 384 centres from A1's camera."""
    centres = synth.voxel_centres(A1_DIMS, ORIGIN, RES).reshape(-1, 3).astype(np.float64)
    u, v, z = project64(centres, A1_POSE[0], A1_QUAT[0])
    return u, v, z, np.abs(centres[:, :2] - A1_POSE[0, :2].astype(np.float64)).max(axis=1)


# ---- A2. past 2048 slabs ----------------------------------------------------------------------------------------------------------

A2_DIMS, A2_LIMITS = (515, 510, 73), (0.01, 80.0)
A2_CORNERS = np.array([[x, y, z] for x in (0, A2_DIMS[0] - 1) for y in (0, A2_DIMS[1] - 1) for z in (0, A2_DIMS[2] - 1)])


@functools.lru_cache(maxsize=None)
def a2_planes():
    """The mostly known map of A2_DIMS -> (occ, free) bool: 0.5 % occupied, 0.2 % unknown, the rest free; the eight corners unknown."""
    u = np.random.default_rng(73).random(A2_DIMS, dtype=np.float32)
    occ = u < 0.005
    unknown = (u >= 0.005) & (u < 0.007)
    cx, cy, cz = A2_CORNERS.T
    occ[cx, cy, cz] = False
    unknown[cx, cy, cz] = True
    return occ, ~occ & ~unknown


def a2_views():
    """[0] one metre outside the face x = 0 at its middle looking along +x, [1] inside near the top (voxel layer 68) looking along +y,
    [2] inside at low z looking up, [3] out of range."""
    ext = np.asarray(A2_DIMS, dtype=np.float64) * RES
    P = f32([[-1.0, ext[1] / 2, ext[2] / 2], [32.03, 5.01, 8.55], [30.3, 31.7, 0.7], [600.0, 1.0, 1.0]])
    return P, f32([Q_PLUS_X, Q_PLUS_Y, Q_PLUS_Z, Q_PLUS_X])


# ---- A3. the largest grid through a window ----------------------------------------------------------------------------------------

A3_LIMITS = (0.3, 1.75)
A3_LOCAL = np.array([[30.5, 33.25, 20.5], [40.25, 20.5, 21.0], [52.5, 44.25, 8.5]])   # in voxels from the window's inner corner


def a3_views(off):
    """Three views inside the window at voxel offset `off`, on the 1/2048 m lattice: looking along +x, +y and +z."""
    P = mc._world(((np.asarray(off, dtype=np.float64) + A3_LOCAL) * 256).astype(np.int64))
    return P, f32([Q_PLUS_X, Q_PLUS_Y, Q_PLUS_Z])


# ---- B. the pick ------------------------------------------------------------------------------------------------------------------

PICK_SIZES = (1, 255, 256, 257, 1000, 65_535, 100_000)
PICK_TIES = ((300, 50), (5 + 256, 5))   # (higher, lower): equal maxima in different lanes (44 and 50), and in one lane on two trips
ROOM_CANDIDATES, ROOM_TILES, ROOM_K = 12, 25, 5


def pick_ref(gains, taken, min_gain):
    """One round of the pick -> the chosen index, or None where the selection stops: the masked argmax, the first of equal values."""
    g = np.where(np.asarray(taken) != 0, -1, np.asarray(gains, dtype=np.int64))
    best = int(np.argmax(g))
    return best if g[best] >= int(min_gain) else None


def pick_cases(n):
    """The one-round cases of n candidates -> a list of dict(name, gains (n,) int64, taken (n,) int32, min_gain, stop)."""
    rng = np.random.default_rng(1000 + n)
    base = rng.integers(0, 1000, size=n).astype(np.int64)
    none = np.zeros(n, dtype=np.int32)
    out = []
    g = base.copy()
    g[n - 1] = 5000
    out.append(dict(name="unique maximum at the last index", gains=g, taken=none, min_gain=1, stop=0))
    for hi, lo in PICK_TIES:
        if n > hi:
            g = base.copy()
            g[[hi, lo]] = 7000
            out.append(dict(name=f"tie at {hi} and {lo}", gains=g, taken=none, min_gain=1, stop=0))
    g = base.copy()
    top = rng.choice(n, size=max(1, n // 3), replace=False)
    g[top] += 10_000
    taken = np.zeros(n, dtype=np.int32)
    taken[top] = 1
    out.append(dict(name="the maximum among taken entries only", gains=g, taken=taken, min_gain=1, stop=0))
    out.append(dict(name="all taken", gains=base + 1, taken=np.ones(n, dtype=np.int32), min_gain=1, stop=0))
    out.append(dict(name="the best gain below min_gain", gains=base, taken=none, min_gain=int(base.max()) + 1, stop=0))
    out.append(dict(name="the best gain exactly min_gain", gains=base, taken=none, min_gain=int(base.max()), stop=0))
    out.append(dict(name="a pre-set stop word", gains=base + 1, taken=none, min_gain=1, stop=1))
    return out


@functools.lru_cache(maxsize=None)
def pick_rounds(n=1000, rounds=10):
    """Random gains from {0..7}: heavy ties -> (gains, the numpy greedy order of `rounds` rounds)."""
    gains = np.random.default_rng(77).integers(0, 8, size=n).astype(np.int64)
    taken, order = np.zeros(n, dtype=np.int32), []
    for _ in range(rounds):
        i = pick_ref(gains, taken, 1)
        order.append(i)
        taken[i] = 1
    return gains, order


def room_candidates():
    """The 12 candidates of tests/test_hip_view_volume.py's selection, tiled to 300 rows: row i is candidate i % 12."""
    P, Q = synth.candidate_grid([0.6, 1.0, 1.4], [0.8, 1.0], 0.5, 2)
    assert len(P) == ROOM_CANDIDATES
    return np.tile(P, (ROOM_TILES, 1)), np.tile(Q, (ROOM_TILES, 1))


# ---- C1. the entry parameter from geometry ----------------------------------------------------------------------------------------

def entry_exact(A, B, v):
    """Where the integer segment A -> B enters the closed box [256 v, 256 (v + 1)] -> the parameter as a Fraction: the maximum over
    the axes with D != 0 of (near face - A) / D, the near face the one on A's side; 0 where A lies inside the box."""
    t = Fraction(0)
    for a in range(3):
        d = int(B[a]) - int(A[a])
        if d != 0:
            near = 256 * int(v[a]) if d > 0 else 256 * (int(v[a]) + 1)
            t = max(t, Fraction(near - int(A[a]), d))
    return t


def entry_inside(A, B, v, t):
    """Does the point A + t (B - A) lie in the closed box of voxel v on all three axes?  Exact."""
    return all(256 * int(v[a]) <= int(A[a]) + t * (int(B[a]) - int(A[a])) <= 256 * (int(v[a]) + 1) for a in range(3))


@functools.lru_cache(maxsize=None)
def random_ray_case():
    """tests/test_raycast_cpu.py's random rays: 5000 segments over the (64, 64, 32) grid at 2 % -> (occ, A, B) in fixed point."""
    occ = rc.plane(rc.MAIN, "p2")
    a, b = rc.segments(rc.MAIN, 5000, seed=3)
    qa, oka = synth.occ_fixed(a, rc.ORIGIN, rc.R)
    qb, okb = synth.occ_fixed(b, rc.ORIGIN, rc.R)
    ok = oka & okb
    return occ, qa[ok], qb[ok]


# ---- C2. rays that span the range -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_cast(skip):
    """long_case()'s 256 rays cast through its 2 % grid -> dict(fixed: cast_fixed's dict, num, den, voxel, lam, visits): one walk of
    the restatement, put together as synth.cast_ref puts it together (every end is in range)."""
    c = mc.long_case()
    fixed = synth.cast_fixed(c["qa"], c["qb"], c["occ"], skip)
    num, den = synth.cast_entry(c["qa"], c["qb"], fixed["steps"])
    v, nx, ny = fixed["voxel"], mc.DIMS[0], mc.DIMS[1]
    voxel = np.where(fixed["hit"], v[:, 0] + nx * (v[:, 1] + ny * v[:, 2]), -1).astype(np.int32)
    lam = np.where(fixed["hit"], synth.cast_lam(num, den), f32(1)).astype(f32)
    return dict(fixed=fixed, num=num, den=den, voxel=voxel, lam=lam, visits=int(fixed["visits"].sum()))


# ---- C3. the largest grid through the window --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def window_cast(skip):
    """window_case(BIG_DIMS, BIG_WINDOW)'s rays cast through the window's plane, the ends shifted -> (voxel (n,) int32 in the full
    grid's numbering, lam (n,) f32, visits)."""
    c = mc.window_case(mc.BIG_DIMS, mc.BIG_WINDOW)
    off = c["off"]
    Aw, Bw = c["qa"] - off * 256, c["qb"] - off * 256
    fixed = synth.cast_fixed(Aw, Bw, c["occ"], skip)
    num, den = synth.cast_entry(Aw, Bw, fixed["steps"])
    v = fixed["voxel"] + off
    nx, ny, _ = mc.BIG_DIMS
    index = v[:, 0] + nx * (v[:, 1] + ny * v[:, 2])
    assert index.dtype == np.int64 and (index[fixed["hit"]] < 1 << 31).all() and (index[fixed["hit"]] >= 0).all()
    voxel = np.where(fixed["hit"], index, -1).astype(np.int32)
    lam = np.where(fixed["hit"], synth.cast_lam(num, den), f32(1)).astype(f32)
    return voxel, lam, int(fixed["visits"].sum())


# ---- C4. the index at exactly 2^31 voxels -----------------------------------------------------------------------------------------

FULL_DIMS = (2048, 2048, 512)
FULL_CORNER = (2047, 2047, 511)
FULL_INDEX = (1 << 31) - 1
FULL_SCAN = dict(min_dist=0.1, max_dist=2.0)


def full_segments():
    """Two segments along +x at ORIGIN / RES, from seven voxels before the far corner voxel into the apron behind it: [0] through the
    corner voxel's middle, [1] one voxel lower in y, past it -> (a, b) f32 world, (A, B) fixed point."""
    A = np.array([[2040 * 256 + 128, 2047 * 256 + 128, 511 * 256 + 128], [2040 * 256 + 128, 2046 * 256 + 128, 511 * 256 + 128]], dtype=np.int64)
    B = A + np.array([10 * 256, 0, 0])
    return mc._world(A), mc._world(B), A, B


# ---- C5. depth scans at the launch limits -----------------------------------------------------------------------------------------

SCAN_DIMS = (37, 5, 20)
SCAN_IMAGES = {"wide": (8192, 1), "tall": (1, 8192), "ragged": (4100, 3)}
SCAN_VIEWS = 65_535
SCAN_MIN_DIST = 1.0   # half of max_dist: the returns of a view inside the thin grid fall on both sides of it


def scan_camera(W, H):
    """fx = fy = half the longer side, the principal point in the image's middle: 90 degrees along the longer side."""
    f = max(W, H) / 2.0
    return f32([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]])


def scan_poses():
    """Two views: inside a voxel near the middle of SCAN_DIMS looking along +x; and six voxels from the end of the apron on x and z
    (grid coordinate 4090 of 4096) looking along +y, so that part of its far points, along either image side, lie out of range."""
    t, q = rc.poses(SCAN_DIMS, 1)
    lo, _ = rc.extent(SCAN_DIMS)
    edge = lo + rc.R * np.array([4090.3, 2.6, 4090.45])
    return f32([t[0], edge]), f32([q[0], Q_PLUS_Y])


def many_poses():
    """65 535 poses uniform over the box of SCAN_DIMS and a four-voxel rim, random quaternions that are not unit, every 97th pose out
    of range."""
    rng = np.random.default_rng(65)
    lo, hi = rc.extent(SCAN_DIMS)
    t = rng.uniform(lo - 4 * rc.R, hi + 4 * rc.R, (SCAN_VIEWS, 3)).astype(f32)
    q = (rng.standard_normal((SCAN_VIEWS, 4)) * (0.5 + rng.random((SCAN_VIEWS, 1)))).astype(f32)
    t[96::97] = [1.0e4, 0.0, 0.0]
    return t, q


@functools.lru_cache(maxsize=None)
def scan_case(name):
    """-> dict(kw: the keywords of synth.depth_scan_ref, ref: what it returns).  name: 'wide', 'tall', 'ragged' or 'views'."""
    if name == "views":
        t, q = many_poses()
        W, H, Kc = 1, 1, rc.camera(1, 1)
    else:
        t, q = scan_poses()
        W, H = SCAN_IMAGES[name]
        Kc = scan_camera(W, H)
    kw = dict(poses=t, quats=q, K=Kc, img_width=W, img_height=H, min_dist=SCAN_MIN_DIST, max_dist=rc.MAX_DIST, origin=rc.ORIGIN, resolution=rc.R,
              occ=rc.plane(SCAN_DIMS, "p10"))
    return dict(kw=kw, ref=synth.depth_scan_ref(**kw))
