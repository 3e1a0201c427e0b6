"""Shared inputs of the weighted travel field's tests (tests/test_travel_weighted_cpu.py, tests/test_hip_travel_weighted.py,
tests/test_hip_travel_weighted_contracts.py): the grids with their traversable sets, the three fills of the weight layer kappa, the
sources with travel_cases' three bad rows, a plain heapq Dijkstra over the step rule written independently of
synth.travel_weighted_ref, and the hand case of two routes."""
import heapq

import numpy as np

import travel_cases as tc

ORIGIN, RES, RADIUS, D = tc.ORIGIN, tc.RES, tc.RADIUS, tc.D
# (20, 19, 18): 3 x 3 x 3 tiles, partial on every axis — a minimum must cross tile faces, edges and corners; (37, 5, 20): travel_cases'
GRIDS = [(5, 6, 3), (20, 19, 18), (37, 5, 20)]
FILLS = ["neutral", "random", "moat"]
MAX_DISTS = [None, 10 * RES]      # none, and 10 voxels: limit 640
WEIGHTS = (64, 91, 111)           # face, edge, corner


def traversable_of(dims, seed=0):
    """T (nx,ny,nz) bool: nine voxels in ten, so that the move rule refuses some diagonals."""
    return np.random.default_rng(40 + seed + dims[0]).random(dims) < 0.9


def moat_band(dims):
    """The x range of the moat: two voxels across the tile border x = 8 where the grid reaches it, else across its middle."""
    x0 = 7 if dims[0] > 9 else dims[0] // 2 - 1
    return x0, x0 + 2


def kappa_of(dims, fill, seed=0):
    """The layer (nx,ny,nz) uint8: all 16; random in [16, 255]; or a moat — 255 in a band of two voxels across a tile border, over
    every y and z but for one neutral gap."""
    if fill == "neutral":
        return np.full(dims, 16, dtype=np.uint8)
    if fill == "random":
        return np.random.default_rng(50 + seed + dims[1]).integers(16, 256, dims).astype(np.uint8)
    assert fill == "moat"
    k = np.full(dims, 16, dtype=np.uint8)
    x0, x1 = moat_band(dims)
    k[x0:x1] = 255
    k[x0:x1, dims[1] // 2, dims[2] // 2] = 16
    return k


def sources_of(T, n):
    """travel_cases.sources_of: n good sources and the three bad rows every build must ignore."""
    return tc.sources_of(T, n)


def step(w, ka, kb):
    return (w * (int(ka) + int(kb)) + 16) >> 5


def dijkstra(T, seeds, kappa, limit=(1 << 31) - 1):
    """cost (nx,ny,nz) int64, -1 unreachable: a textbook heapq Dijkstra over the move rule with the weighted step, voxel by voxel."""
    T = np.asarray(T, dtype=bool)
    dims = T.shape
    cost = np.full(dims, -1, dtype=np.int64)
    heap = []
    for s in np.asarray(seeds, dtype=np.int64).reshape(-1, 3):
        s = tuple(int(k) for k in s)
        if all(0 <= s[a] < dims[a] for a in range(3)) and T[s]:
            heapq.heappush(heap, (0, s))
    while heap:
        c, v = heapq.heappop(heap)
        if cost[v] >= 0:
            continue
        cost[v] = c
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    n_axes = (dx != 0) + (dy != 0) + (dz != 0)
                    u = (v[0] + dx, v[1] + dy, v[2] + dz)
                    if n_axes == 0 or not all(0 <= u[a] < dims[a] for a in range(3)) or cost[u] >= 0:
                        continue
                    box = [(v[0] + ex, v[1] + ey, v[2] + ez) for ex in {0, dx} for ey in {0, dy} for ez in {0, dz}]
                    if not all(T[b] for b in box):
                        continue
                    to = c + step(WEIGHTS[n_axes - 1], kappa[v], kappa[u])
                    if to <= limit:
                        heapq.heappush(heap, (to, u))
    return cost


def two_routes():
    """The hand case.  Dims (9, 14, 1): a wall at x = 4 with two openings, each one voxel wide, at y = 2 and y = 10.  The source
    (1, 2, 0) and the goal (7, 2, 0) face each other through the near opening: 6 face moves, 384.  The voxels in front of and behind
    that opening, x = 3 and x = 5 for y = 1 .. 3, hold kappa = 255, the opening itself and everything else 16 — the opening is a
    neutral gap one voxel wide between them, and no diagonal gets into it past the wall's corners, so the short route must step on
    (3, 2, 0) and (5, 2, 0): 64 + 4 x 542 + 64 = 2296 weighted.  The long route through (4, 10, 0) lies in the open: two diagonals
    and six face moves to (3, 10, 0), one face move into the opening (a diagonal would cut the wall's corner), and the same back:
    2 (2 x 91 + 7 x 64) = 1260 under either metric.  -> dict(T, kappa, source, goal, near, far, and the four costs)."""
    dims = (9, 14, 1)
    T = np.ones(dims, dtype=bool)
    T[4] = False
    T[4, 2, 0] = T[4, 10, 0] = True
    kappa = np.full(dims, 16, dtype=np.uint8)
    kappa[3, 1:4, 0] = kappa[5, 1:4, 0] = 255
    return dict(T=T, kappa=kappa, source=(1, 2, 0), goal=(7, 2, 0), near=(4, 2, 0), far=(4, 10, 0), short_plain=384, long_plain=1260,
                short_weighted=2296, long_weighted=1260)


def voxels_of(rows, origin=ORIGIN, r=RES):
    """The voxels whose centres a path's rows (L,3) are."""
    return [tuple(int(k) for k in v) for v in np.floor((np.asarray(rows, dtype=np.float64) - np.asarray(origin, dtype=np.float64)) / r).astype(int)]
