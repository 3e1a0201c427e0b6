"""Shared inputs of the relocalisation tests (tests/test_scan_search_cpu.py, tests/test_hip_scan_search.py): numpy only.  The maps,
scans and rotations are those of tests/scan_match_cases.py; the references are computed once per process and never modified."""
import functools

import numpy as np

import scan_match_cases as sc
from trajectory_optimization_amd import synth

# (dims, window, levels, points in the scan, seed): the last — a window larger than its map — is chosen so that K = 3 gives ties == 2
SEARCHES = (((13, 10, 5), (5, 3, 1), 2, 150, 1), ((13, 10, 5), (16, 16, 2), 3, 150, 1), ((13, 10, 5), (16, 16, 4), 5, 150, 1),
            ((4, 4, 2), (7, 6, 4), 3, 5, 2), ((37, 29, 9), (16, 13, 1), 4, 150, 1),
            ((13, 10, 5), (11, 6, 0), 3, 150, 1))   # (2wx+1 = 23, 2wy+1 = 13: no multiple of 2^3 on either axis)
VALUES = ((None, 0), (-10, -8))
KS = (1, 3)
SEARCH_PARAMS = [(i, v, K) for i in range(len(SEARCHES)) for v in range(len(VALUES)) for K in KS]

SCENE_WINDOW, SCENE_LEVELS = (24, 20, 1), 3


def search_id(p):
    dims, window, H, _, _ = SEARCHES[p[0]]
    return f"{'x'.join(map(str, dims))}-w{'_'.join(map(str, window))}-H{H}-v{p[1]}-K{p[2]}"


def rotation_matrices(K):
    return np.stack([synth.scan_rotation(q) for q in sc.rotations(K)])


@functools.lru_cache(maxsize=None)
def inputs(i):
    """-> (L, points) of search i."""
    dims, _, _, n, seed = SEARCHES[i]
    L, P = sc.random_log_odds(dims, seed), sc.random_scan(dims, n, seed)
    L.setflags(write=False), P.setflags(write=False)
    return L, P


@functools.lru_cache(maxsize=None)
def search_ref(i, v, K):
    """The record of search i by the restatement."""
    dims, window, H, _, _ = SEARCHES[i]
    L, P = inputs(i)
    rec = synth.scan_search_ref(L, sc.ORIGIN, sc.RES, P, rotation_matrices(K), sc.T, window, H, *VALUES[v])
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def scene():
    """The end-to-end scene of scan_match_cases -> (L, sensor-frame points, prior t, the nine candidate quaternions)."""
    L = sc.room_log_odds(sc.room_occupancy())
    pts = sc.scene_scan_ref()
    t, q, half = sc.prior_pose()
    from trajectory_optimization_amd import tools
    return L, pts, t, tools.yaw_candidates(q, half, sc.YAW_STEPS)


@functools.lru_cache(maxsize=None)
def scene_ref():
    L, pts, t, quats = scene()
    Rs = np.stack([synth.scan_rotation(q) for q in quats])
    return synth.scan_search_ref(L, sc.ROOM["origin"], sc.ROOM["resolution"], pts, Rs, t, SCENE_WINDOW, SCENE_LEVELS)


def probe_nodes(dims, level, K, m, seed=0):
    """m nodes (m,4) int64 (k, sx, sy, sz) of one level, rotations interleaved: first those that hang off each face of dims for a voxel
    near the origin — shifts that start at -(2^level - 1), at -2^level, at n - 1 and at n on x and on y, sz below 0 and at nz — then
    random ones over three voxels around the box."""
    rng = np.random.default_rng(7300 + seed + 17 * level + m)
    nx, ny, nz = dims
    b = (1 << level) - 1
    edge = [(sx, sy, sz) for sx in (-b - 2, -b - 1, -b, -1, 0, nx - 3, nx - 2, nx - 1, nx, nx + 1) for sy in (-b - 1, -b, 0, ny - 2, ny)
            for sz in (-nz - 1, -1, 0, nz - 1, nz)]
    rows = [(i % K,) + e for i, e in enumerate(edge)]
    nodes = np.asarray(rows, dtype=np.int64)
    if m > len(nodes):
        extra = np.stack([rng.integers(0, K, m - len(nodes)), rng.integers(-nx - b - 3, nx + 4, m - len(nodes)),
                          rng.integers(-ny - b - 3, ny + 4, m - len(nodes)), rng.integers(-nz - 1, nz + 2, m - len(nodes))], axis=1)
        nodes = np.concatenate([nodes, extra])
    return nodes[rng.permutation(len(nodes))[:m]] if m < len(nodes) else nodes
