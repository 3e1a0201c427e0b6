"""The inputs shared by the two tests of the hard visibility path at size (tests/test_hard_at_size_cpu.py without a GPU,
tests/test_hip_hard_at_size.py on one) and what the CPU references say of them, computed once per process and never modified.

The hard path builds the occlusion rows of ModelTraj(occlusion=...): hard_kernels.hip (frustum cull, cull of many poses),
render_kernels.hip (z-buffer, batched z-buffer) and k_occ_rows_masked of traj_kernels.hip.  Every size below is the smallest that
reaches the path it is named for; limits() reads the thresholds from the kernels' text, and the CPU test holds the sizes against
them, so a changed tile or cap fails there instead of silently un-testing a path.  Nothing here touches a GPU."""
import functools
import os
import re

import numpy as np

from trajectory_optimization_amd import synth

f32 = np.float32
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "trajectory_optimization_amd", "csrc")


@functools.lru_cache(maxsize=None)
def limits():
    """The tiles, caps and thresholds of the hard path, read from the kernels' text (an assertion names the pattern that is gone)."""
    text = {name: open(os.path.join(CSRC, name)).read() for name in ("common.hpp", "hard_kernels.hip", "render_kernels.hip", "traj_kernels.hip")}

    def one(name, pattern):
        m = re.search(pattern, text[name])
        assert m, (name, pattern)
        return int(m.group(1))
    return dict(
        block=one("common.hpp", r"#define TO_BLOCK\s+(\d+)"),
        wave=one("common.hpp", r"#define TO_WAVE\s+(\d+)"),
        cull_tile=one("hard_kernels.hip", r"#define TO_CULL_TILE\s+(\d+)"),
        two_launch_tiles=one("hard_kernels.hip", r"if \(ntiles <= (\d+) && \(kept_idx \|\| kept_count\)\)"),
        scan_threads=one("hard_kernels.hip", r"ntiles > \d+ \? (\d+) : TO_BLOCK"),
        write_blocks=one("hard_kernels.hip", r"wblocks < (\d+) \? wblocks : \1"),
        max_poses=one("hard_kernels.hip", r"n_wps > (\d+)\)\s*return TOHIP_EINVAL"),
        splat_small=one("render_kernels.hip", r"#define TO_SPLAT_SMALL\s+(\d+)"),
        splat_blocks=one("render_kernels.hip", r"if \(nb > (\d+)\) nb = \1;\s*k_minmax_all<<<\(int\)nb, TO_BLOCK, 0, st>>>\(verts, 3 \* n, mm\);\s*"
                                               r"TO_HIP_CHECK_LAUNCH\(\);\s*k_splat<<<\(int\)nb, TO_BLOCK, 0, st>>>\(verts, n, rp, zbuf\);\s*TO_HIP_CHECK_LAUNCH\(\);\s*\}\s*k_resolve"),
        splat_batched_blocks=one("render_kernels.hip", r"if \(nb > (\d+)\) nb = \1;\s*for \(int64_t w0 = 0"),
        rows_blocks=one("traj_kernels.hip", r"if \(nb > (\d+)\) nb = \1;\s*k_occ_rows_masked<<<dim3\(\(unsigned\)nb, \(unsigned\)n_wps\), (?:\1)"),
    )


def tiles(n):
    return -(-n // limits()["cull_tile"])


# ---------------------------------------------------------------------------------------------------------------- A. the frustum cull

# (n, tiles, what the size reaches, inputs)
FRUSTUM_SIZES = (
    (1_500_001, 1_465, "two launches, up to 23 counts per lane", ("real",)),
    (2_097_152, 2_048, "the last size of the two-launch path", ("pattern",)),
    (2_097_153, 2_049, "the scan launch, one round, ntiles % 4 == 1", ("pattern",)),
    (4_200_003, 4_102, "the scan's second round: carry, buffer swap, ntiles % 4 == 2", ("pattern", "real")),
    (33_557_505, 32_772, "the write pass strides over tiles", ("device",)),
)
FRUSTUM_LIMITS = (1.0, 10.0)                    # (those of tests/test_hip_hard.py::test_frustum_edge_cases)
KIND_ROWS = np.array([[0.0, 0.0, 5.0],          # kind 0: kept
                      [0.0, 0.0, 20.0],         # kind 1: fails the distance test only
                      [100.0, 0.0, 5.0]], f32)  # kind 2: fails the field of view only
FRUSTUM_POSE = (np.array([0.9, 0.1, -0.3, 0.2], f32), np.array([6.0, 2.0, 0.0], f32))   # (tools/time_frustum.py's)
TILE_MODES = ("empty", "full", "first row only", "last row only", "half", "random density")


@functools.lru_cache(maxsize=None)
def pattern_tiles(n, seed=7):
    """Per 1 024-point tile of a pattern input: its mode (TILE_MODES), the 16-bit threshold a point's hash must stay under to be
    kept, and the one row kept whatever its hash (-1: none).  The first six tiles take the six modes in turn."""
    nt = tiles(n)
    rng = np.random.default_rng(seed)
    mode = rng.integers(0, len(TILE_MODES), nt)
    mode[:len(TILE_MODES)] = np.arange(len(TILE_MODES))[:nt]
    dens = rng.integers(1, 65536, nt)
    thresh = np.select([mode == 0, mode == 1, mode == 2, mode == 3, mode == 4], [0, 65536, 0, 0, 32768], default=dens).astype(np.int32)
    one = np.where(mode == 2, 0, np.where(mode == 3, limits()["cull_tile"] - 1, -1)).astype(np.int32)
    return mode, thresh, one


def pattern_kind(n, seed=7):
    """kind (n,) uint8 of every point of the pattern input: an integer hash of the row against its tile's threshold, the tile's one
    row, and the very last point kept."""
    tile = limits()["cull_tile"]
    _, thresh, one = pattern_tiles(n, seed)
    i = np.arange(n, dtype=np.int64)
    x = (i * 2654435761) & 0xffffffff
    t = i // tile
    kept = (((x >> 13) & 0xffff) < thresh[t]) | ((i % tile) == one[t])
    kept[-1] = True
    return np.where(kept, 0, 1 + ((x >> 30) & 1)).astype(np.uint8)


def pattern_kind_torch(n, device, seed=7):
    """pattern_kind with plain torch ops on `device` (the largest case is built where it is used)."""
    import torch
    tile = limits()["cull_tile"]
    _, thresh, one = pattern_tiles(n, seed)
    thresh, one = torch.from_numpy(thresh).to(device), torch.from_numpy(one).to(device)
    i = torch.arange(n, dtype=torch.int64, device=device)
    x = (i * 2654435761) & 0xffffffff
    t = torch.div(i, tile, rounding_mode="floor")
    kept = (((x >> 13) & 0xffff) < thresh[t]) | ((i % tile) == one[t])
    kept[-1] = True
    return torch.where(kept, torch.zeros_like(x), 1 + ((x >> 30) & 1)).to(torch.uint8)


def pattern_points(kind):
    """(3, n) f32 camera-frame rows of the kinds."""
    return np.ascontiguousarray(KIND_ROWS[kind].T)


@functools.lru_cache(maxsize=None)
def real_frustum_case(n):
    """A synth.make_cloud cloud in one camera frame -> dict(cam3 (3, n), dist, fov, idx) by the oracle."""
    from oracle import oracle
    pts = synth.make_cloud(n, seed=n % 1000)
    cam = oracle.to_camera_frame(pts, FRUSTUM_POSE[0], FRUSTUM_POSE[1], normalize=True)
    cam3 = np.ascontiguousarray(cam.T)
    d, f = oracle.frustum_masks(cam3, K, IW, IH, *FRUSTUM_LIMITS)
    return dict(cam3=cam3, dist=d, fov=f, idx=np.flatnonzero(d & f).astype(np.int32))


# ------------------------------------------------------------------------------------------------------------ B. the cull of many poses

CULL_LIMITS = (1.0, 15.0)
AWAY = 1000.0


def cull_reference(pts, poses, quats, which=None):
    """{w: (kept indices int32 ascending, their camera-frame rows f32)} by the oracle: to_camera_frame (bit-exact with the kernels
    already) -> frustum_masks -> flatnonzero."""
    from oracle import oracle
    out = {}
    for w in (range(len(poses)) if which is None else which):
        cam = oracle.to_camera_frame(pts, quats[w], poses[w], normalize=True)
        d, f = oracle.frustum_masks(np.ascontiguousarray(cam.T), K, IW, IH, *CULL_LIMITS)
        kept = np.flatnonzero(d & f)
        out[int(w)] = (kept.astype(np.int32), np.ascontiguousarray(cam[kept]))
    return out


@functools.lru_cache(maxsize=None)
def cull_case(name):
    """'scan': n = 300 007 x 3 poses, 293 tiles per pose — the second round of k_cull_wps_scan (256 counts a round); pose 1 is moved
    1 000 m away.  'offsets': n = 3 000 x 300 poses — the second round of k_cull_wps_offsets; poses 0, 255, 256 and 299 see nothing.
    -> dict(pts, poses, quats, away, ref)."""
    n, W, away = {"scan": (300_007, 3, (1,)), "offsets": (3_000, 300, (0, 255, 256, 299))}[name]
    pts = synth.make_cloud(n, seed=n % 1000)
    poses, quats = synth.make_path(W, optical=True, jitter_seed=W)
    poses[list(away)] += f32(AWAY)
    return dict(pts=pts, poses=poses, quats=quats, away=away, ref=cull_reference(pts, poses, quats))


GRID_POSES = 65_537
GRID_LOOKED_AT = (0, 65_534, 65_535, 65_536)


@functools.lru_cache(maxsize=None)
def grid_case():
    """n = 8 points, W = 65 537 poses along synth.make_path: one pose more than two chunks of the grid.y limit hold.  The points lie
    2 to 9 m ahead of the path's two ends and of three poses between -> dict(pts, poses, quats, ref: the oracle on GRID_LOOKED_AT)."""
    W = GRID_POSES
    poses, quats = synth.make_path(W, optical=True)
    s = np.arange(W, dtype=np.float64) / (W - 1)
    yaw = 0.5 * np.cos(6.0 * s)
    ahead = np.stack([np.cos(yaw), np.sin(yaw), np.zeros(W)], axis=1)
    at = [(0, 3.0), (0, 8.0), (W // 3, 5.0), (W // 2, 4.0), (2 * W // 3, 6.0), (W - 1, 2.0), (W - 1, 5.0), (W - 1, 9.0)]
    pts = np.array([poses[k].astype(np.float64) + d * ahead[k] + [0.0, 0.05 * d, -0.03 * d] for k, d in at]).astype(f32)
    return dict(pts=pts, poses=poses, quats=quats, ref=cull_reference(pts, poses, quats, GRID_LOOKED_AT))


# ---------------------------------------------------------------------------------------------------------------------- C. the z-buffer

SMALL_H, SMALL_W = 96, 128
SMALL_K = np.array([[80.0, 0.0, SMALL_W / 2], [0.0, 82.0, SMALL_H / 2], [0.0, 0.0, 1.0]], f32)   # (tests/test_render.py's)
PARAMS = dict(radius=0.03, znear=1.0, zfar=10.0)        # the discs: rho = 2.4 / Z pixels
COVER_PARAMS = dict(radius=0.06, znear=0.05, zfar=10.0)   # rho = 96 pixels at Z = 0.05: the whole image, 80 pixels from centre to corner


def _at(u, v, Z):
    """The camera-frame row that projects to pixel coordinates (u, v) at depth Z (to f32 rounding: the tests read the oracle)."""
    Z = f32(Z)
    return [f32((u - SMALL_K[0, 2]) * Z / SMALL_K[0, 0]), f32((v - SMALL_K[1, 2]) * Z / SMALL_K[1, 1]), Z]


NONFINITE_ROWS = np.array([[np.nan, 0, 2], [0, np.nan, 2], [0, 0, np.nan], [np.inf, 0, 2], [-np.inf, 0, 2], [0, np.inf, 2], [0, -np.inf, 2],
                           [0, 0, np.inf], [0, 0, -np.inf], [3e38, 0, 1.5]], f32)


@functools.lru_cache(maxsize=None)
def edge_scene(nonfinite=False):
    """The hand-built scene on the 96 x 128 image -> (v (n, 3) f32, rows {label: [row numbers]}).  With PARAMS a disc has
    rho = 2.4 / Z pixels.  nonfinite: NONFINITE_ROWS in the middle of it (they splat nothing, and move the later rows' numbers)."""
    one, far = f32(1.0), f32(10.0)
    parts = [
        ("tie_ascending", [_at(20.5, 20.5, 2.0), _at(21.5, 20.5, 2.0)]),              # same Z bits, overlapping: left one first ...
        ("tie_descending", [_at(31.5, 20.5, 2.0), _at(30.5, 20.5, 2.0)]),             # ... right one first
        ("tie_triple", [_at(41.5, 20.5, 1.5), _at(42.5, 20.5, 1.5), _at(40.5, 20.5, 1.5)]),
        ("behind", [_at(20.5, 20.5, 5.0)]),                                           # inside the first pair's discs, deeper: owns nothing
        ("duplicate", [_at(50.5, 20.5, 2.5), _at(50.5, 20.5, 2.5)]),
        ("on_znear", [_at(60.5, 20.5, one)]),
        ("on_zfar", [_at(70.5, 20.5, far)]),
        ("before_znear", [_at(80.5, 20.5, np.nextafter(one, f32(0)))]),
        ("beyond_zfar", [_at(90.5, 20.5, np.nextafter(far, f32(np.inf)))]),
        ("cut_left", [_at(0.5, 40.5, 1.5)]),
        ("cut_right", [_at(127.5, 40.5, 1.5)]),
        ("cut_top", [_at(60.5, 0.5, 1.5)]),
        ("cut_bottom", [_at(60.5, 95.5, 1.5)]),
        ("cut_corner", [_at(0.4, 0.3, 1.5), _at(127.7, 95.6, 1.5)]),
        ("centre_outside_reaches_in", [_at(-1.0, 60.5, 1.2)]),                        # rho = 2: covers the centre of pixel 0
        ("centre_outside_misses", [_at(-1.7, 70.5, 1.2)]),                            # reaches u = 0.3, short of the pixel centre at 0.5
        ("between_centres", [_at(70.0, 70.0, 9.0)]),                                  # rho = 0.27, 0.71 from the four centres around it
        ("covers_all", [_at(64.0, 48.0, 0.05)]),                                      # clipped by PARAMS, the whole image by COVER_PARAMS
    ]
    if nonfinite:
        parts.insert(len(parts) // 2, ("nonfinite", NONFINITE_ROWS.tolist()))
    rows, v = {}, []
    for label, pts in parts:
        rows[label] = list(range(len(v), len(v) + len(pts)))
        v.extend(pts)
    return np.array(v, f32), rows


def boxes(v, Kc=SMALL_K, height=SMALL_H, width=SMALL_W, radius=0.03, znear=1.0, zfar=10.0):
    """The clamped bounding box of every row's disc by the kernels' f32 formulas -> (bw, bh, area) int arrays; 0 for a row that
    splats nothing (out of the depth range, off the image, not finite)."""
    v = np.asarray(v, f32)
    fx, cx, fy, cy = f32(Kc[0][0]), f32(Kc[0][2]), f32(Kc[1][1]), f32(Kc[1][2])
    with np.errstate(all="ignore"):
        X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
        u, w_ = fx * X / Z + cx, fy * Y / Z + cy
        rho = fx * f32(radius) / Z
        ok = (Z >= f32(znear)) & (Z <= f32(zfar)) & (u + rho >= 0) & (u - rho <= f32(width)) & (w_ + rho >= 0) & (w_ - rho <= f32(height))
        half = f32(0.5)
        z = np.zeros_like(u)
        j0 = np.maximum(0, np.floor(np.where(ok, u - rho - half, z)).astype(np.int64))
        j1 = np.minimum(width - 1, np.ceil(np.where(ok, u + rho - half, z)).astype(np.int64))
        i0 = np.maximum(0, np.floor(np.where(ok, w_ - rho - half, z)).astype(np.int64))
        i1 = np.minimum(height - 1, np.ceil(np.where(ok, w_ + rho - half, z)).astype(np.int64))
    bw, bh = np.where(ok, np.maximum(j1 - j0 + 1, 0), 0), np.where(ok, np.maximum(i1 - i0 + 1, 0), 0)
    return bw, bh, bw * bh


def _candidates(rng, n, depth=(1.0, 10.0)):
    """n rows that project to uniform pixel coordinates over the image and a rim of 3 pixels, 1 / Z uniform."""
    u, v_ = rng.uniform(-3.0, SMALL_W + 3.0, n), rng.uniform(-3.0, SMALL_H + 3.0, n)
    Z = 1.0 / rng.uniform(1.0 / depth[1], 1.0 / depth[0], n)
    return np.stack([(u - SMALL_K[0, 2]) * Z / SMALL_K[0, 0], (v_ - SMALL_K[1, 2]) * Z / SMALL_K[1, 1], Z], axis=1).astype(f32)


THRESHOLD_GROUPS = ("exactly 24 and exactly 25", "small and large", "all large", "all small", "ragged")


@functools.lru_cache(maxsize=None)
def threshold_cloud():
    """Rows chosen by their box: a wave of k_splat_batched takes 64 consecutive rows, and a lane walks its own disc when the box has
    at most TO_SPLAT_SMALL pixels, else the wave walks it.  Groups of 64 rows in THRESHOLD_GROUPS' order (the last one 37 rows with
    rows that splat nothing among them) -> (v, area)."""
    small_max = limits()["splat_small"]
    rng = np.random.default_rng(24)
    cand = _candidates(rng, 400_000)
    area = boxes(cand, **PARAMS)[2]
    pick = lambda sel, k: cand[rng.choice(np.flatnonzero(sel), k, replace=False)]
    small, large = (area >= 1) & (area <= small_max), area > small_max
    groups = [np.concatenate([pick(area == small_max, 8), pick(area == small_max + 1, 8), pick(small, 24), pick(large, 24)]),
              np.concatenate([pick(small, 32), pick(large, 32)]),
              pick(large, 64),
              pick(small, 64),
              np.concatenate([pick(small, 15), pick(area == 0, 7), pick(large, 15)])]
    v = np.concatenate([g[rng.permutation(len(g))] for g in groups])
    return v, boxes(v, **PARAMS)[2]


def small_scene(n, seed):
    """(tests/test_render.py's random scene: depths 0 to 11 m, both clip planes crossed)"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * np.array([6.0, 6.0, 11.0]) - np.array([3.0, 3.0, 0.0])).astype(f32)


RAGGED_COUNTS = (0, 1, 63, 64, 65, 4097)


@functools.lru_cache(maxsize=None)
def batched_clouds():
    """The clouds of the batched z-buffer test, in order: the edge scene, the same with the rows that are not finite, the threshold
    cloud, and random scenes of RAGGED_COUNTS rows -> tuple of (n, 3) f32."""
    return (edge_scene()[0], edge_scene(True)[0], threshold_cloud()[0]) + tuple(small_scene(c, 100 + c) for c in RAGGED_COUNTS)


def owners(v, params=PARAMS, Kc=SMALL_K, height=SMALL_H, width=SMALL_W):
    """-> (image, owner (H, W) int64, the rows that own a pixel ascending) by oracle/render_oracle.py."""
    from oracle import render_oracle
    with np.errstate(invalid="ignore"):
        img, owner = render_oracle.render_points(v, Kc, height, width, **params)
    return img, owner, np.unique(owner[owner >= 0])


@functools.lru_cache(maxsize=None)
def reference_owners(which, cover=False):
    """owners() of batched_clouds()[which], computed once."""
    return owners(batched_clouds()[which], COVER_PARAMS if cover else PARAMS)


IN_RANGE_HEAD, PAST_STRIDE = 2_700, 321


@functools.lru_cache(maxsize=None)
def second_trip_cloud(stride):
    """stride + 321 rows on the small image: all at Z = 50 (beyond zfar: the oracle skips them at once) but the first 2 700 rows,
    at 1 to 10 m, and the 321 rows past `stride`, at 1 to 2 m — those a kernel reaches only in its second trip
    -> (v, image, owner, owning rows)."""
    n = stride + PAST_STRIDE
    rng = np.random.default_rng(stride % 1000)
    v = np.zeros((n, 3), f32)
    v[:, :2] = rng.uniform(-30.0, 30.0, (n, 2))
    v[:, 2] = 50.0
    v[:IN_RANGE_HEAD] = _candidates(rng, IN_RANGE_HEAD)
    v[stride:] = _candidates(rng, PAST_STRIDE, depth=(1.0, 2.0))
    return (v,) + owners(v)


# --------------------------------------------------------------------------------------------------- C'. the pipeline: cull -> z-buffer

@functools.lru_cache(maxsize=None)
def two_wall_case():
    """A camera at the origin looking along +Z (the identity pose) at a wall at Z = 3 m, 35 x 35 points 3.5 cm apart (discs of 7.58
    pixels radius 8.84 pixels apart: no gap between four of them, and no disc reaches a neighbour's centre pixel), a
    wall of 9 x 9 points at Z = 6 m wholly behind it, and four points outside the frustum -> (pts, poses, quats, want (1, n))."""
    g = np.arange(-17, 18) * 0.035
    front = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.full((35, 35), 3.0)], axis=-1).reshape(-1, 3)
    h = np.arange(-4, 5) * 0.2
    back = np.stack(list(np.meshgrid(h, h, indexing="ij")) + [np.full((9, 9), 6.0)], axis=-1).reshape(-1, 3)
    outside = np.array([[0.0, 0.0, -3.0], [0.0, 0.0, 0.5], [0.0, 0.0, 20.0], [30.0, 0.0, 3.0]])
    rng = np.random.default_rng(2)
    pts = np.concatenate([front, back, outside])
    order = rng.permutation(len(pts))
    want = np.concatenate([np.ones(len(front)), np.zeros(len(back)), np.ones(len(outside))]).astype(f32)
    return pts[order].astype(f32), np.zeros((1, 3), f32), np.array([[1.0, 0.0, 0.0, 0.0]], f32), want[order][None, :]


ROWS_N, ROWS_W = 20_000, 5
ROWS_NOTHING, ROWS_THREE = 1, 3


@functools.lru_cache(maxsize=None)
def rows_case():
    """n = 20 000 (no multiple of the 2 048-point tile: pad bits exist) x 5 poses at the real image: a 12 x 12 x 4 m block of points
    seen from a short path inside it, pose 1 moved 1 000 m away (keeps nothing), pose 3 moved 500 m away in front of three points
    of its own (keeps exactly those) -> dict(pts, poses, quats, counts, want (5, n))."""
    from oracle import oracle
    pts = synth.make_cloud(ROWS_N - 3, seed=20, extent=(12.0, 12.0, 4.0))
    poses, quats = synth.make_path(ROWS_W, optical=True, jitter_seed=20, scale=0.2)
    poses[ROWS_NOTHING] += np.array([0.0, -AWAY, 0.0], f32)
    poses[ROWS_THREE], quats[ROWS_THREE] = [495.0, 500.0, 0.0], synth.Q_OPTICAL.astype(f32)   # looks along +x
    three = np.array([[500.0, 500.0, 0.0], [500.5, 500.3, 0.2], [501.0, 499.6, -0.2]], f32)
    pts = np.concatenate([pts[:7000], three[:1], pts[7000:15000], three[1:], pts[15000:]])
    ref = cull_reference(pts, poses, quats)
    want = oracle.occlusion_masks(pts, poses, quats, K, IW, IH, *CULL_LIMITS, method="zbuffer")
    return dict(pts=pts, poses=poses, quats=quats, counts=[len(ref[w][0]) for w in range(ROWS_W)], kept=[ref[w][0] for w in range(ROWS_W)], want=want)


# ------------------------------------------------------------------------------------------------- D. tohip_occlusion_rows_masked

def occ_row_ref(n, npad, inv, kept, vis_pos=None, visible=None, min_points=0):
    """The header's statement of an occlusion bit row: all ones; clear each kept point's bit; set the visible kept points' bits
    again; pads := bit n-1.  The visible ones are positions in `kept` (vis_pos) or the non-zero entries of a vector over the kept
    points (visible); inv = None: `kept` holds packed positions already; fewer than min_points kept: the row of ones."""
    kept = np.asarray(kept, np.int64)
    if visible is not None:
        vis_pos = np.flatnonzero(np.asarray(visible)[:len(kept)] != 0)
    pos = kept if inv is None else np.asarray(inv)[kept]
    b = np.ones(npad, np.uint32)
    if len(kept) >= min_points:
        b[pos] = 0
        b[pos[vis_pos]] = 1
    b[n:] = b[n - 1]
    words = (b.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return words.view(np.int32)


OCC_N, OCC_KEPT, OCC_STRIDE = 200_000, 150_001, 65_536
OCC_SEG_OFF = (7, 7 + OCC_KEPT + 13)
OCC_BLOCK = (70_016, 110_016)        # packed positions all kept in the sorted case (starts on a word): the hand-made pattern's home


def _hand_pattern():
    """Hidden flags over positions from a word boundary on: for L = 1 .. 32 three words with a run of L hidden neighbours at the
    start, the middle and the end of the word; a word with hidden, visible, hidden; runs over the boundary of two words; 200 hidden
    in a row (whole words, and over the boundary of any two waves)."""
    w = []
    for L in range(1, 33):
        for o in (0, (32 - L) // 2, 32 - L):
            word = np.zeros(32, bool)
            word[o:o + L] = True
            w.append(word)
    w.append(np.array([1, 0, 1] + [0] * 26 + [1, 0, 1], bool))
    cross = np.zeros(96, bool)
    cross[27:39] = True      # 5 bits of one word, 7 of the next
    cross[63:65] = True
    w.append(cross)
    w.append(np.concatenate([np.zeros(32, bool), np.ones(200, bool), np.zeros(24, bool)]))
    return np.concatenate(w)


@functools.lru_cache(maxsize=None)
def occ_rows_case(in_packed_order):
    """Two waypoints over n = 200 000 points, 150 001 kept each (a third trip over the 65 536 rows a launch covers), their visibility
    values at OCC_SEG_OFF in one vector.  in_packed_order: kept = ascending packed positions, inv_perm NULL, waypoint 0 with
    _hand_pattern() in OCC_BLOCK; else unsorted kept rows and a random inv_perm.  The last sorted point is kept by both, hidden by
    waypoint 0 (pad bits 0) and visible to waypoint 1 (pad bits 1).  Hidden values are 0.0 and -0.0, visible ones 1.0 and others
    -> dict(inv, kept (2, n) int32, visible f32, want (2, npad / 32) int32)."""
    n, m = OCC_N, OCC_KEPT
    npad = -(-n // 2048) * 2048
    rng = np.random.default_rng(150 + int(in_packed_order))
    inv = None if in_packed_order else rng.permutation(n).astype(np.int32)
    last = n - 1 if in_packed_order else int(np.flatnonzero(inv == n - 1)[0])
    kept = np.zeros((2, n), np.int32)
    visible = np.full(OCC_SEG_OFF[1] + m + 64, 1.0, f32)
    want = []
    for w in range(2):
        block = np.arange(*OCC_BLOCK) if in_packed_order and w == 0 else np.zeros(0, np.int64)
        rest = np.setdiff1d(np.arange(n), np.concatenate([block, [last]]))
        k = np.concatenate([block, [last], rng.choice(rest, m - len(block) - 1, replace=False)])
        k = np.sort(k) if in_packed_order else rng.permutation(k)
        hidden = rng.random(m) < 0.5
        if len(block):
            j0 = int(np.searchsorted(k, OCC_BLOCK[0]))
            pat = _hand_pattern()
            hidden[j0:j0 + len(pat)] = pat
        hidden[np.flatnonzero(k == last)[0]] = w == 0
        vals = np.where(hidden, np.where(rng.random(m) < 0.1, f32(-0.0), f32(0.0)), np.where(rng.random(m) < 0.1, f32(0.25), f32(1.0))).astype(f32)
        kept[w, :m] = k
        visible[OCC_SEG_OFF[w]:OCC_SEG_OFF[w] + m] = vals
        want.append(occ_row_ref(n, npad, inv, k, visible=vals, min_points=4))
    return dict(inv=inv, kept=kept, visible=visible, want=np.stack(want), npad=npad)


def run_stats(kept, visible):
    """Of ascending packed positions and their visibility values: the runs the kernel's segmented scan forms — hidden points on
    consecutive rows j whose bits fall into one word -> dict(lengths: set of run lengths, hvh: a word with hidden, visible, hidden,
    crosses_word / crosses_wave: hidden neighbours on both sides of a word / of a 64-row boundary, full_word, trips: set of j // 65 536
    with a hidden row)."""
    kept, hid = np.asarray(kept, np.int64), np.asarray(visible) == 0
    j = np.flatnonzero(hid)
    word = kept[j] >> 5
    new = np.ones(len(j), bool)
    new[1:] = (np.diff(j) != 1) | (np.diff(word) != 0)
    lengths = np.diff(np.flatnonzero(np.concatenate([new, [True]])))
    nb = (np.diff(j) == 1)
    hvh = False
    for a in np.flatnonzero((np.diff(j) == 2) & (np.diff(word) == 0)):
        hvh = hvh or (kept[j[a] + 1] >> 5) == word[a]
    return dict(lengths=set(lengths.tolist()), hvh=bool(hvh),
                crosses_word=bool((nb & (np.diff(word) == 1) & (np.diff(kept[j]) == 1)).any()),
                crosses_wave=bool((nb & (j[:-1] % 64 == 63)).any()),
                full_word=bool(32 in lengths), trips=set((j // OCC_STRIDE).tolist()))
