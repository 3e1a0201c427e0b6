"""Shared inputs of the connected-component tests (tests/test_components_cpu.py, tests/test_hip_components.py): the grids, fills and
connectivities, the hand cases with their component counts, the two serpentines and the two-room world of the frontier clusters."""
import numpy as np

from travel_cases import GRIDS, ORIGIN, RES, centre, serpentine  # noqa: F401  (the tests read them from here)

CONNECTIVITIES = (6, 18, 26)
FILLS = {"empty": 0.0, "2%": 0.02, "30%": 0.3, "60%": 0.6, "full": 1.0}


def plane_of(dims, fill, seed=11):
    return np.random.default_rng(seed + dims[0]).random(dims) < FILLS[fill]


def checkerboard(dims=(64, 64, 32)):
    i, j, k = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    return (i + j + k) % 2 == 0


def _pair(dims, a, b):
    P = np.zeros(dims, dtype=bool)
    P[a] = P[b] = True
    return P


def hand_cases():
    """{name: (plane, {connectivity: the number of components})}."""
    dims = (20, 18, 17)
    cases = {}
    # two voxels that share a face, an edge, a corner: one component from c = 6, 18, 26 on — across a brick border (x = 3 | 4), a tile
    # border (7 | 8) and a tile corner ((7,7,7) | (8,8,8))
    for where, lo in (("brick", 3), ("tile", 7)):
        cases[f"face_across_a_{where}_border"] = (_pair(dims, (lo, 5, 5), (lo + 1, 5, 5)), {6: 1, 18: 1, 26: 1})
        cases[f"edge_across_a_{where}_border"] = (_pair(dims, (lo, 5, 5), (lo + 1, 6, 5)), {6: 2, 18: 1, 26: 1})
        cases[f"corner_across_a_{where}_border"] = (_pair(dims, (lo, 5, 5), (lo + 1, 6, 6)), {6: 2, 18: 2, 26: 1})
    cases["face_across_a_tile_corner"] = (_pair(dims, (7, 7, 7), (7, 7, 8)), {6: 1, 18: 1, 26: 1})
    cases["edge_across_a_tile_corner"] = (_pair(dims, (7, 7, 7), (7, 8, 8)), {6: 2, 18: 1, 26: 1})
    cases["corner_across_a_tile_corner"] = (_pair(dims, (7, 7, 7), (8, 8, 8)), {6: 2, 18: 2, 26: 1})
    # a chain along the main diagonal: under c = 26 the lowest index has to cross two tile corners, one round after the other
    P = np.zeros((24, 24, 24), dtype=bool)
    P[np.arange(24), np.arange(24), np.arange(24)] = True
    cases["diagonal_chain_through_tile_corners"] = (P, {6: 24, 18: 24, 26: 1})
    # a staircase of edge moves in the xy plane across three tiles: one component from c = 18 on
    P = np.zeros((24, 24, 3), dtype=bool)
    P[np.arange(24), np.arange(24), 1] = True
    cases["edge_chain_through_tile_edges"] = (P, {6: 24, 18: 1, 26: 1})
    # a voxel at each of the eight corners of dims (no multiple of the brick or the tile)
    P = np.zeros((37, 5, 20), dtype=bool)
    for x in (0, 36):
        for y in (0, 4):
            for z in (0, 19):
                P[x, y, z] = True
    cases["eight_corners_of_dims"] = (P, {6: 8, 18: 8, 26: 8})
    cases["full_plane"] = (np.ones((37, 5, 20), dtype=bool), {6: 1, 18: 1, 26: 1})
    return cases


def serpentines():
    """travel_cases.serpentine() as a plane — one component whose root lies at one end of the 680-voxel lane — and its copy flipped
    along x and y, whose lowest index lies at the other end: the minimum travels the whole path against the sweep order."""
    T, _, _ = serpentine()
    return {"forward": T, "reversed": np.ascontiguousarray(T[::-1, ::-1, :])}


def canonical(labels, plane):
    """Any labelling (nx,ny,nz) of `plane` whose labels differ between components -> (ids, roots) as the project defines them: each
    label replaced by the minimum linear index v = (z ny + y) nx + x of its voxels, then ranked."""
    nx, ny, nz = plane.shape
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    lin = ((z * ny + y) * nx + x)[plane]
    lab = np.asarray(labels)[plane]
    low = np.full(int(lab.max()) + 1 if lab.size else 0, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(low, lab, lin)
    roots = np.unique(low[lab])
    ids = np.full(plane.shape, -1, dtype=np.int64)
    ids[plane] = np.searchsorted(roots, low[lab])
    return ids, roots


def slit_world():
    """(40, 16, 8) at r = 0.125, origin 0: a wall at x = 24 with a slit one voxel wide at y = 8 — narrower than the robot.  Room A
    (x < 24) is known free but for an unknown 4 x 4 x 4 blob near x = 0; of the hall (x > 24) only x = 25 .. 30 is known free, as seen
    through the slit, the rest of it is unknown.  Three stray rays have each left one free voxel deep in the unknown part of the
    hall.  -> (occ, free, robot voxel)."""
    dims = (40, 16, 8)
    occ = np.zeros(dims, dtype=bool)
    occ[24, :, :] = True
    occ[24, 8, :] = False
    free = np.zeros(dims, dtype=bool)
    free[:24] = True
    free[2:6, 6:10, 2:6] = False            # the blob: a closed frontier shell around it, in room A
    free[24, 8, :] = True
    free[25:31] = True                      # the hall's known part: its frontier is the sheet x = 30
    for v in ((34, 3, 2), (36, 11, 5), (38, 6, 6)):
        free[v] = True                      # the stray singletons
    return occ, free, (13, 8, 4)
