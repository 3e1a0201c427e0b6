"""Shared inputs of the batched travel fields' tests (tests/test_travel_batch_cpu.py, tests/test_hip_travel_batch.py): the sources of a
batch with their field numbers, the doorway world of the tour, random cost matrices with ties, and a brute-force greedy assignment."""
import functools

import numpy as np

import travel_cases as tc
from trajectory_optimization_amd import synth

f32 = np.float32


def batch_sources(T, B, seed=3):
    """The sources of a batch of B fields over T -> (src (S,3) f32, source_field (S,) int32).  Of tc.sources_of(T, 8)'s good rows g,
    field b < min(B, 4) gets g[b], field 1 also g[5], field 2 also g[0] (two fields seeded in one voxel); field 4 (B = 5) gets none.
    Then the three bad rows (naming field 0), g[6] naming field -1 and g[7] naming field B.  The rows of a field do not depend on B,
    so a reference computed for one B serves the others."""
    rows = tc.sources_of(T, 8, seed)
    pick = [(b, b) for b in range(min(B, 4))] + [(5, 1), (0, 2)]
    pick = [(g, b) for g, b in pick if b < B] + [(8, 0), (9, 0), (10, 0), (6, -1), (7, B)]
    return rows[[g for g, _ in pick]].astype(f32), np.asarray([b for _, b in pick], dtype=np.int32)


def batch_seeds_ref(src, source_field, B, origin, r, T):
    """-> (seeded (S,) uint8, [the seeded voxels of field b for b in range(B)]) by the batch's rule: the single build's seeding rule
    and 0 <= source_field < B."""
    seeded, vox = synth.travel_seeds_ref(src, origin, r, T)
    seeded = (seeded.astype(bool) & (source_field >= 0) & (source_field < B)).astype(np.uint8)
    return seeded, [vox[(seeded == 1) & (source_field == b)] for b in range(B)]


# ---- the tour's world: (48, 32, 8), a wall at x = 24 with one doorway ---------------------------------------------------------------------
DOOR_DIMS, DOOR_ORIGIN = (48, 32, 8), (0.0, 0.0, 0.0)
DOOR_VIEWS = [(8, 12, 4), (40, 12, 4), (10, 28, 4), (40, 29, 3)]   # node 0 the start; every straight leg across the wall misses the doorway


@functools.lru_cache(maxsize=None)
def doorway_world():
    """-> dict(T, P, blocked, cost, seeded, via): T the traversable set (everything but the wall x = 24, open at y = 2 .. 5), P
    the four views' positions, blocked (4,4) bool by the field's own segment walk (a field of 65535 in T and 0 in the wall, need2 =
    1), cost / seeded = travel_matrix_ref, via = tour_travel_units(cost)."""
    T = np.ones(DOOR_DIMS, dtype=bool)
    T[24, :, :] = False
    T[24, 2:6, :] = True
    P = tc.centre(DOOR_VIEWS, DOOR_ORIGIN)
    field = np.where(T, 65535, 0)
    n = len(P)
    blocked = np.zeros((n, n), dtype=bool)
    i, j = np.triu_indices(n, 1)
    d2, _ = synth.field_segments_ref(P[i], P[j], DOOR_ORIGIN, tc.RES, field)
    blocked[i, j] = blocked[j, i] = d2 < 1
    cost, seeded = synth.travel_matrix_ref(P, DOOR_ORIGIN, tc.RES, T)
    return dict(T=T, P=P, blocked=blocked, cost=cost, seeded=seeded, via=synth.tour_travel_units(cost, tc.RES))


# ---- assignment ------------------------------------------------------------------------------------------------------------------------

def random_costs(R, C, seed, ld=None):
    """(R, ld or C) int64 with few distinct values (ties) and many -1; the columns past C, where ld > C, hold 0: a candidate if read."""
    rng = np.random.default_rng(seed)
    cost = rng.integers(-3, 6, (R, ld or C)) * 64
    cost[cost < 0] = -1
    cost[:, C:] = 0
    return cost.astype(np.int64)


def assign_brute(cost, min_cost=0):
    """The greedy rule restated another way: every candidate pair sorted once by (cost, r, c), taken in that order when both its
    row and its column are still free."""
    cost = np.asarray(cost)
    R, C = cost.shape
    pairs = sorted((int(cost[r, c]), r, c) for r in range(R) for c in range(C) if cost[r, c] >= min_cost)
    col_of_row, row_of_col = np.full(R, -1, dtype=np.int32), np.full(C, -1, dtype=np.int32)
    for _, r, c in pairs:
        if col_of_row[r] < 0 and row_of_col[c] < 0:
            col_of_row[r], row_of_col[c] = c, r
    return col_of_row, row_of_col
