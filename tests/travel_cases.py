"""Shared inputs of the travel field's tests (tests/test_travel_cpu.py, tests/test_hip_travel.py): the grids and fills, the sources
with their three bad rows, the hand cases of the move rule, the serpentine, and a plain heapq Dijkstra over the move rule."""
import heapq

import numpy as np

from trajectory_optimization_amd import synth

f32 = np.float32
ORIGIN, RES = (-1.0, 2.0, 0.5), 0.125
RADIUS, D = 0.1, 3            # need2 = ceil((0.8 + 1/64)^2) = 1: T = the voxels with no obstacle among their 27 neighbours
GRIDS = [(1, 1, 1), (5, 6, 3), (37, 5, 20), (64, 64, 32)]
FILLS = ["empty", "2%", "30%", "full"]
MAX_DISTS = [None, 10 * RES]  # none, and 10 voxels: limit 640


def occ_of(dims, fill, seed=0):
    rng = np.random.default_rng(seed + dims[0])
    return rng.random(dims) < {"2%": 0.02, "30%": 0.3, "empty": 0.0, "full": 1.0}[fill]


def free_of(dims, seed=7):
    return np.random.default_rng(seed + dims[1]).random(dims) < 0.9


def centre(v, origin=ORIGIN, r=RES):
    """The world centre of voxel v (any shape (..., 3)), f32 as the map computes it."""
    v = np.asarray(v, dtype=f32)
    return (np.asarray(origin, dtype=f32) + ((v + f32(0.5)).astype(f32) * f32(r)).astype(f32)).astype(f32)


def sources_of(T, n, seed=3):
    """n good sources at voxels of T where it has any (else the grid's first voxel), then the three bad rows every build must ignore:
    one in a voxel outside T (where one exists; else a second out-of-dims row), one outside dims, one NaN -> (S,3) f32."""
    rng = np.random.default_rng(seed)
    inT, out = np.argwhere(T), np.argwhere(~T)
    good = inT[rng.choice(len(inT), size=n, replace=len(inT) < n)] if len(inT) else np.zeros((n, 3), dtype=np.int64)
    rows = [centre(good)]
    rows.append(centre(out[rng.integers(len(out))])[None] if len(out) else centre(np.asarray(T.shape) + 2)[None])
    rows.append(centre(np.asarray(T.shape) + 1)[None])                     # in range, outside dims
    rows.append(np.array([[np.nan, 0.0, 0.0]], dtype=f32))
    return np.concatenate(rows).astype(f32)


def dijkstra(T, seeds, limit=synth.TRAVEL_MAX_LIMIT):
    """cost (nx,ny,nz) int64, -1 unreachable: a textbook heapq Dijkstra over the move rule written voxel by voxel."""
    T = np.asarray(T, dtype=bool)
    dims = T.shape
    cost = np.full(dims, -1, dtype=np.int64)
    heap = []
    for s in np.asarray(seeds, dtype=np.int64).reshape(-1, 3):
        s = tuple(int(k) for k in s)
        if all(0 <= s[a] < dims[a] for a in range(3)) and T[s]:
            heapq.heappush(heap, (0, s))
    inside = lambda p: all(0 <= p[a] < dims[a] for a in range(3))   # noqa: E731
    while heap:
        c, v = heapq.heappop(heap)
        if cost[v] >= 0:
            continue
        cost[v] = c
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    k = (dx != 0) + (dy != 0) + (dz != 0)
                    if k == 0:
                        continue
                    u = (v[0] + dx, v[1] + dy, v[2] + dz)
                    if not inside(u) or cost[u] >= 0:
                        continue
                    box = [(v[0] + ex, v[1] + ey, v[2] + ez) for ex in {0, dx} for ey in {0, dy} for ez in {0, dz}]
                    if all(T[b] for b in box) and c + synth.TRAVEL_WEIGHTS[k - 1] <= limit:
                        heapq.heappush(heap, (c + synth.TRAVEL_WEIGHTS[k - 1], u))
    return cost


# ---- hand cases of the move rule: (T, source voxel, {voxel: expected cost}) ------------------------------------------------------------

def hand_cases():
    cases = {}
    # a diagonal between two T voxels whose shared side voxels are not both in T is refused: the way round costs three face moves
    T = np.ones((3, 2, 1), dtype=bool)
    T[1, 0, 0] = False                        # (0,0,0) -> (1,1,0) would cut the corner of (1,0,0)
    cases["edge_diagonal_refused"] = (T, (0, 0, 0), {(0, 1, 0): 64, (1, 1, 0): 128, (2, 1, 0): 192, (2, 0, 0): 256, (1, 0, 0): -1})
    # with both side voxels in T the same diagonal is taken
    cases["edge_diagonal_open"] = (np.ones((2, 2, 1), dtype=bool), (0, 0, 0), {(1, 1, 0): 91, (1, 0, 0): 64, (0, 1, 0): 64})
    # a 2 x 2 x 2 block with one voxel missing allows no corner move: the far corner costs a face and an edge move
    T = np.ones((2, 2, 2), dtype=bool)
    T[1, 0, 0] = False
    cases["corner_move_refused"] = (T, (0, 0, 0), {(1, 1, 1): 64 + 91, (0, 1, 1): 91, (1, 1, 0): 128, (1, 0, 1): 128})
    cases["corner_move_open"] = (np.ones((2, 2, 2), dtype=bool), (0, 0, 0), {(1, 1, 1): 111})
    # a pocket whose only entrance is a cut corner stays unreachable
    T = np.zeros((4, 4, 1), dtype=bool)
    T[0:2, 0:2, 0] = True
    T[2:4, 2:4, 0] = True                     # two rooms that touch at the corner (1,1) / (2,2) only
    cases["pocket_behind_a_cut_corner"] = (T, (0, 0, 0), {(1, 1, 0): 91, (2, 2, 0): -1, (3, 3, 0): -1})
    return cases


def serpentine():
    """Dims (66, 41, 3): every fourth y row (y = 1, 5, ... 37) is an open lane one voxel wide, the three rows between two lanes are
    wall but for a gap at alternating ends of x.  The one path from the first lane's start to the last lane's end runs the length of
    every lane — some 680 hops that cross tile borders back and forth.  -> (T, source voxel, goal voxel)."""
    T = np.zeros((66, 41, 3), dtype=bool)
    lanes = list(range(1, 41, 4))
    for k, y in enumerate(lanes):
        T[:, y, :] = True
        if y + 4 < 41:
            T[65 if k % 2 == 0 else 0, y + 1:y + 4, :] = True
    return T, (0, lanes[0], 1), (65 if len(lanes) % 2 else 0, lanes[-1], 1)
