"""Shared inputs of the ray-cast tests (tests/test_raycast_cpu.py, tests/test_hip_raycast.py): grids, planes, segments and scan cases,
all from fixed seeds.  The CPU file checks the conditions these inputs must meet (every flag present in the main scene, the
out-of-range case all skipped), so the GPU comparisons cannot pass vacuously."""
import numpy as np

from trajectory_optimization_amd import synth

R = 0.125
ORIGIN = (-1.0, -0.5, -0.25)   # dyadic, like R: voxel faces are exact f32 numbers
GRIDS = [(1, 1, 1), (5, 6, 3), (37, 5, 20), (64, 64, 32)]
PLANES = ("empty", "full", "p2", "p10")
MAIN = (64, 64, 32)
SKIPS = [(0, 0), (1, 0), (2, 3)]
IMAGES = [(1, 1), (17, 9), (70, 33)]   # one pixel; a ragged single tile; 5 x 3 tiles, ragged on both sides
MIN_DIST, MAX_DIST = 0.6, 2.0


def plane(dims, kind, seed=5):
    if kind == "empty":
        return np.zeros(dims, dtype=bool)
    if kind == "full":
        return np.ones(dims, dtype=bool)
    rng = np.random.default_rng(seed + sum(dims))
    return rng.random(dims) < {"p2": 0.02, "p10": 0.10}[kind]


def extent(dims):
    lo = np.asarray(ORIGIN, dtype=np.float64)
    return lo, lo + R * np.asarray(dims, dtype=np.float64)


def segments(dims, n, seed=1, short=False):
    """n rays (a, b) f32: ends inside the box grown by four voxels (so some lie in the apron), every 53rd ray with an end far out of
    range, every 61st with a NaN; short: b within three voxels of a (a large count stays cheap to restate)."""
    rng = np.random.default_rng(seed)
    lo, hi = extent(dims)
    a = rng.uniform(lo - 4 * R, hi + 4 * R, (n, 3))
    b = a + rng.uniform(-3 * R, 3 * R, (n, 3)) if short else rng.uniform(lo - 4 * R, hi + 4 * R, (n, 3))
    a, b = a.astype(np.float32), b.astype(np.float32)
    b[52::53, 0] = 1.0e6
    a[60::61, 2] = np.nan
    return a, b


def camera(W, H, integral=True):
    """K of matching scale: fx = fy = W / 2 with the principal point in the image's middle, or a non-integral variant."""
    if integral:
        fx, fy, cx, cy = W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0
    else:
        fx, fy, cx, cy = 0.5185 * W, 0.4815 * W, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2
    return np.float32([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])


def _yaw(deg):
    h = np.deg2rad(deg) / 2.0
    return synth.quat_mul(np.array([np.cos(h), 0.0, 0.0, np.sin(h)]), synth.Q_OPTICAL)


def poses(dims, V=3):
    """V views of the grid `dims`: inside a voxel near the middle looking along +x; on a voxel face (an exact multiple of R from the
    origin on every axis) looking along +y, its quaternion of norm 3; in the apron two voxels in front of the box looking in."""
    lo, hi = extent(dims)
    mid = lo + R * (np.asarray(dims) // 2) + np.array([0.3, 0.6, 0.45]) * R
    face = lo + R * (np.asarray(dims) // 3)
    apron = np.array([lo[0] - 2.2 * R, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
    t = np.float32([mid, face, apron])[:V]
    q = np.float32([_yaw(0.0), 3.0 * _yaw(90.0), _yaw(10.0)])[:V]
    return t, q


def out_of_range_poses():
    """Cameras beyond the apron: every ray is skipped."""
    return np.float32([[1.0e4, 0.0, 0.0], [0.0, -1.0e5, 0.0]]), np.float32([_yaw(0.0), _yaw(45.0)])


def main_scene():
    """The main random scene: MAIN at 2 %, three views, 70 x 33 pixels -> keywords of synth.depth_scan_ref."""
    t, q = poses(MAIN)
    W, H = IMAGES[2]
    return dict(poses=t, quats=q, K=camera(W, H), img_width=W, img_height=H, min_dist=MIN_DIST, max_dist=MAX_DIST, origin=ORIGIN, resolution=R,
                occ=plane(MAIN, "p2"))


# the theorems' scenes: tests/test_view_volume_cpu.py's box
ROOM = dict(origin=(-0.5, -0.5, -0.5), resolution=0.125, dims=(28, 24, 16))
ROOM_POSE = np.float32([1.03, 0.97, 0.52])
ROOM_CAMERA = dict(intrins=camera(48, 36), img_width=48, img_height=36, min_dist=0.05, max_dist=4.0)


def room_world(doorway):
    occ, _ = synth.occupancy_ref(synth.box_room(doorway=doorway), ROOM["origin"], ROOM["resolution"], ROOM["dims"])
    return occ


def room_views():
    """Four views from ROOM_POSE, 90 degrees of yaw apart (the camera's horizontal field is 90 degrees: together they look all round)."""
    return np.tile(ROOM_POSE, (4, 1)), np.float32([_yaw(d) for d in (0.0, 90.0, 180.0, 270.0)])
