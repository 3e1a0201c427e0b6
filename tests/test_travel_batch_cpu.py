"""Travel fields in batches without a GPU: the numpy restatements (synth.assign_greedy_ref, travel_batch_ref, travel_matrix_ref,
tour_travel_units, tour_plan with the map's routes as via_D), ops.check_travel_batch's errors by name, the ABI entries, and the C
entries' argument checks, which return before anything is enqueued."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import abi_cases
import travel_batch_cases as bc
import travel_cases as tc
from trajectory_optimization_amd import synth

ENTRIES = ["tohip_travel_batch_bytes", "tohip_travel_batch_workspace_bytes", "tohip_travel_build_batch", "tohip_travel_positions_batch",
           "tohip_travel_paths_batch", "tohip_assign_greedy"]


def _assign(cost, min_cost=0):
    col, row = synth.assign_greedy_ref(np.asarray(cost), min_cost)
    return col.tolist(), row.tolist()


def test_assign_greedy_ref_by_hand():
    # the global minimum (1) is robot 1's only option and robot 0's first choice: robot 1 takes it, robot 0 gets its second choice
    assert _assign([[2, 7], [1, -1]]) == ([1, 0], [1, 0])
    # greedy, not optimal: robot 0 takes the opening that is robot 1's only option, and robot 1 goes without
    assert _assign([[5, 3], [-1, 3]]) == ([1, -1], [-1, 0])
    # ties: the lower row first, then the lower column
    assert _assign([[4, 4], [4, 4]]) == ([0, 1], [0, 1])
    assert _assign([[9, 4, 4], [4, 9, 4]]) == ([1, 0], [1, 0, -1])
    # a row of all -1 gets -1
    assert _assign([[-1, -1, -1], [6, 5, -1]]) == ([-1, 1], [-1, 1, -1])
    # more rows than columns: the dearest rows go without
    assert _assign([[3], [1], [2]]) == ([-1, 0, -1], [1])
    # min_cost excludes a 0 (the opening the robot stands in)
    assert _assign([[0, 8], [5, 9]]) == ([0, 1], [0, 1])
    assert _assign([[0, 8], [5, 9]], min_cost=1) == ([1, 0], [1, 0])
    col, row = synth.assign_greedy_ref(np.zeros((2, 3), dtype=np.int64))
    assert col.dtype == np.int32 and row.dtype == np.int32 and col.tolist() == [0, 1] and row.tolist() == [0, 1, -1]


@pytest.mark.parametrize("seed", range(8))
def test_assign_greedy_ref_equals_sorting_all_pairs(seed):
    cost = bc.random_costs(5, 7, seed)
    assert (cost == -1).any() and len(np.unique(cost)) < 8            # ties and holes
    for min_cost in (0, 1, 128):
        got, want = synth.assign_greedy_ref(cost, min_cost), bc.assign_brute(cost, min_cost)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (seed, min_cost)
        for r, c in enumerate(got[0]):
            assert c < 0 or (got[1][c] == r and cost[r, c] >= min_cost)


def test_assign_min_cost_fixed():
    assert synth.assign_min_cost_fixed(0.0, 0.125) == 0 and synth.assign_min_cost_fixed(1e-9, 0.125) == 1
    assert synth.assign_min_cost_fixed(0.125, 0.125) == 64 and synth.assign_min_cost_fixed(0.126, 0.125) == 65


@pytest.mark.parametrize("fill", ["empty", "2%", "30%"])
@pytest.mark.parametrize("dims", tc.GRIDS[:3], ids=str)
def test_travel_matrix_ref_is_symmetric_where_seeded(dims, fill):
    T = ~tc.occ_of(dims, fill)
    pos = tc.sources_of(T, 5)                                          # five good rows, then outside T, outside dims, NaN
    cost, seeded = synth.travel_matrix_ref(pos, tc.ORIGIN, tc.RES, T)
    M = len(pos)
    inside = synth.travel_positions_ref(pos, tc.ORIGIN, tc.RES, np.zeros(dims)) != -2      # the position's voxel lies inside dims
    assert cost.shape == (M, M) and cost.dtype == np.int64 and seeded[:5].all() == T.any() and seeded[5:].tolist() == [0, 0, 0]
    assert inside[:5].all() and inside[-2:].tolist() == [False, False]
    s = seeded == 1
    assert np.array_equal(cost[np.ix_(s, s)], cost[np.ix_(s, s)].T)
    assert np.array_equal(np.diag(cost), np.where(s, 0, np.where(inside, -1, -2)))
    assert (cost[:, ~inside] == -2).all() and (cost[~s][:, inside] == -1).all()  # an unseeded row: -1, or -2 in the columns out of range
    # row i is the single field of source i, looked up
    seeds = synth.travel_seeds_ref(pos, tc.ORIGIN, tc.RES, T)[1]
    assert np.array_equal(cost[1], synth.travel_positions_ref(pos, tc.ORIGIN, tc.RES, synth.travel_ref(T, seeds[1:2])))
    fields = synth.travel_batch_ref(T, [seeds[0:1], [], seeds[1:3]])
    assert fields.shape == (3,) + dims and (fields[1] == -1).all() and np.array_equal(fields[2], synth.travel_ref(T, seeds[1:3]))


@pytest.mark.parametrize("r", [0.1, 0.125])
def test_tour_travel_units_equal_exact_rationals(r):
    """round_half_even(cost (f32 r) 2^14) in Python integers and exact rationals.  (f32 r) 2^14 is exact in f64 and the product is
    rounded once: below 2^53 / 2^14 units it is exact, and at cost 2^31 - 1 it is within 2^-11 of the exact value, which lies further
    than that from a half here — so the two roundings agree."""
    costs = [0, 1, 64, (1 << 31) - 1]
    exact = Fraction(float(np.float32(r))) * (1 << 14)
    want = [round(c * exact) for c in costs]                            # (Fraction's round is half to even)
    for c in costs:
        assert abs((c * exact) % 1 - Fraction(1, 2)) > Fraction(1, 1 << 10) or c < 1 << 20
    got = synth.tour_travel_units(np.asarray(costs), r)
    assert got.dtype == np.int64 and got.tolist() == want
    assert synth.tour_travel_units([-1, -2, 64], r).tolist() == [synth.TOUR_INF, synth.TOUR_INF, want[2]]
    assert synth.tour_travel_units(np.asarray([[64]]), 0.125).tolist() == [[1 << 17]]   # one voxel edge of 1/8 m = 2^17 units


def test_tour_plan_takes_the_map_route_where_a_wall_forces_it():
    w = bc.doorway_world()
    P, blocked, via = w["P"], w["blocked"], w["via"]
    assert blocked[0, 1] and blocked[0, 3] and blocked[2, 1] and blocked[2, 3] and not blocked[0, 2] and not blocked[1, 3]
    assert w["seeded"].tolist() == [1, 1, 1, 1] and (w["cost"] >= 0).all()
    plain = synth.tour_plan(P, blocked)
    assert plain["unreachable"].tolist() == [False, True, False, True] and plain["m"] == 2      # the wall cuts the straight-leg graph
    tour = synth.tour_plan(P, blocked, via_D=via)
    assert not tour["unreachable"].any() and tour["m"] == 4 and sorted(tour["order"].tolist()) == [0, 1, 2, 3]
    # the wall forces the map route on every leg across it; on the open legs the straight line wins (26-connected >= Euclidean)
    assert np.array_equal(tour["via_flag"], blocked)
    direct = synth.tour_edge_lengths(P)
    assert (via[~blocked] >= direct[~blocked]).all()
    assert tour["D"][0, 1] == via[0, 1] and tour["D"][0, 2] == direct[0, 2]
    steps = list(zip(tour["walk"], tour["walk"][1:]))
    assert any(tour["via_flag"][u, v] for u, v in steps)
    assert tour["length_fixed"] == sum(int(tour["D"][u, v]) for u, v in steps)


def test_abi_entries():
    header, before = abi_cases.check_abi_entries(ENTRIES)
    assert "#define TOHIP_TRAVEL_MAX_FIELDS 256\n" in header and "TOHIP_TRAVEL_MAX_FIELDS" in before
    from trajectory_optimization_amd import _lib
    assert _lib.CONSTANTS["TOHIP_TRAVEL_MAX_FIELDS"] == synth.TRAVEL_MAX_FIELDS == 256


def test_check_travel_batch_errors_by_name():
    torch = pytest.importorskip("torch")
    from trajectory_optimization_amd import ops

    class Grid(ops.OccupancyGrid):
        def __init__(self, dims=(8, 8, 8), r=0.125):   # a grid's geometry without a device
            self.origin, self.resolution, self.dims, _ = ops.check_los((0.0, 0.0, 0.0), r, dims)
            self.device = torch.device("cuda", 0)

    class Field(ops.ClearanceField):
        def __init__(self, grid, D):
            self.occupied, self.free, self.D = grid, None, D
            self.origin, self.resolution, self.dims, self.device = grid.origin, grid.resolution, grid.dims, grid.device

    field = Field(Grid(), 3)
    src = torch.zeros(3, 3)
    assert ops.check_travel_batch(field, 0.1, src) == (1, (1 << 31) - 1, 3, 3)
    assert ops.check_travel_batch(field, 0.1, src, torch.tensor([4, -1, 0])) == (1, (1 << 31) - 1, 3, 5)
    assert ops.check_travel_batch(field, 0.1, src, torch.tensor([-1, -1, -3]))[3] == 1
    assert ops.check_travel_batch(field, 0.1, src, torch.tensor([0, 9, 1], dtype=torch.int32), n_fields=2, max_dist=1.25)[1:] == (640, 3, 2)
    assert ops.check_travel_batch(field, 0.1, src, n_fields=256)[3] == 256
    bad = [
        (dict(field=object()), "field must be an ops.ClearanceField"),                   # check_travel's rules come first
        (dict(sources=torch.zeros(0, 3)), "sources must have shape (S,3)"),
        (dict(max_dist=-1.0), "max_dist must be None or a finite number"),
        (dict(rounds_per_check=0), "rounds_per_check must be an integer"),
        (dict(source_field=[0, 1, 2]), "source_field must be an integer tensor of shape (3,)"),
        (dict(source_field=torch.zeros(3)), "source_field must be an integer tensor of shape (3,)"),
        (dict(source_field=torch.zeros(3, dtype=torch.bool)), "source_field must be an integer tensor of shape (3,)"),
        (dict(source_field=torch.zeros(2, dtype=torch.int64)), "source_field must be an integer tensor of shape (3,)"),
        (dict(source_field=torch.zeros((3, 1), dtype=torch.int64)), "source_field must be an integer tensor of shape (3,)"),
        (dict(n_fields=0), "n_fields must be an integer in [1, 256]"),
        (dict(n_fields=257), "n_fields must be an integer in [1, 256]"),
        (dict(n_fields=2.0), "n_fields must be an integer in [1, 256]"),
        (dict(source_field=torch.tensor([0, 1, 256])), "n_fields must be an integer in [1, 256]"),
    ]
    for kw, text in bad:
        args = dict(field=field, radius=0.1, sources=src)
        args.update(kw)
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")):
            ops.check_travel_batch(**args)
    # the list entry packs field and tile in 31 bits: fake dims of 256^3 tiles
    fake = (2048, 2048, 2048)
    assert ops.travel_tiles(fake) == 1 << 24 and ops.travel_tiles((5, 6, 3)) == 1 and ops.travel_tiles((9, 8, 17)) == 6
    assert ops.check_travel_batch(field, 0.1, src, n_fields=127, dims=fake)[3] == 127
    with pytest.raises(ValueError, match="must fit 31 bits"):
        ops.check_travel_batch(field, 0.1, src, n_fields=128, dims=fake)


def test_entries_refuse_bad_arguments_without_gpu():
    """Every argument check returns before anything is enqueued: bad calls come back with their code on a machine without a GPU."""
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    EINVAL, ENOSPC = -1, -2
    p, q, r, t, u, v = (ctypes.c_void_p(a) for a in (64, 4096, 8192, 16384, 32768, 65536))   # pointers no call may reach
    ok = _lib.OccGeom((ctypes.c_float * 3)(0.0, 0.0, 0.0), 0.1, (ctypes.c_int32 * 3)(64, 64, 32))
    nb, fb, cb1 = (fn(64, 64, 32) for fn in (L.tohip_occ_bytes, L.tohip_field_bytes, L.tohip_travel_bytes))
    B = 3
    cb, wb = L.tohip_travel_batch_bytes(64, 64, 32, B), L.tohip_travel_batch_workspace_bytes(64, 64, 32, B)
    assert cb == B * cb1 == B * 4 * 64 * 64 * 32
    assert wb == 256 + 2 * 256 + 3 * 4 * 256                             # 8 x 8 x 4 tiles: a header, two bitmaps of 3 x 8 words, 768 entries
    assert L.tohip_travel_batch_workspace_bytes(64, 64, 32, 1) == L.tohip_travel_workspace_bytes(64, 64, 32)
    assert L.tohip_travel_batch_bytes(2047, 2045, 511, 256) == 256 * 4 * 2047 * 2045 * 511
    for bad in ((0, 4, 4, 1), (4, 4, 2049, 1), (4, 4, 4, 0), (4, 4, 4, 257), (4, 4, 4, -1)):
        assert L.tohip_travel_batch_bytes(*bad) == 0 and L.tohip_travel_batch_workspace_bytes(*bad) == 0, bad
    rounds = ctypes.c_int64(-7)
    names = ("field", "fbytes", "occ", "free", "grid_bytes", "geom", "need2", "src", "src_field", "S", "B", "limit", "rpc", "cost", "bytes", "ws",
             "ws_bytes", "seeded", "rounds", "stream")
    base = (p, fb, None, None, nb, ok, 1, q, v, 2, B, 640, 16, r, cb, t, wb, None, ctypes.byref(rounds), None)

    def build(**kw):
        assert set(kw) <= set(names), kw
        return L.tohip_travel_build_batch(*[kw.get(k, b) for k, b in zip(names, base)])

    for kw in (dict(B=0), dict(B=257), dict(B=-1), dict(bytes=cb - 1), dict(bytes=cb1), dict(ws_bytes=wb - 1),
               dict(ws_bytes=L.tohip_travel_workspace_bytes(64, 64, 32)), dict(src_field=None), dict(src=None), dict(S=0), dict(cost=None),
               dict(ws=None), dict(geom=None), dict(limit=-1), dict(limit=1 << 31), dict(rpc=0), dict(need2=0), dict(cost=p), dict(ws=r),
               dict(occ=u)):
        assert build(**kw) == EINVAL, kw
    assert build(fbytes=fb - 1) == ENOSPC and rounds.value == -7
    # the lookups and the paths
    pos = lambda **kw: L.tohip_travel_positions_batch(*[kw.get(k, b) for k, b in zip(   # noqa: E731
        ("cost", "bytes", "geom", "B", "pos", "m", "out", "dist", "stream"), (r, cb, ok, B, q, 10, t, None, None))])
    for kw in (dict(B=0), dict(B=257), dict(cost=None), dict(geom=None), dict(pos=None), dict(out=None), dict(m=-1)):
        assert pos(**kw) == EINVAL, kw
    assert pos(bytes=cb - 1) == ENOSPC and pos(m=0) == 0 and pos(m=0, pos=None, out=None) == 0
    paths = lambda **kw: L.tohip_travel_paths_batch(*[kw.get(k, b) for k, b in zip(   # noqa: E731
        ("cost", "bytes", "field", "fbytes", "occ", "free", "grid_bytes", "geom", "need2", "B", "goals", "goal_field", "G", "max_rows", "rows",
         "counts", "stream"), (r, cb, p, fb, None, None, nb, ok, 1, B, q, v, 4, 100, t, u, None))])
    for kw in (dict(B=0), dict(B=257), dict(cost=None), dict(goal_field=None), dict(goals=None), dict(rows=None), dict(counts=None),
               dict(max_rows=0), dict(G=-1)):
        assert paths(**kw) == EINVAL, kw
    assert paths(bytes=cb - 1) == ENOSPC and paths(G=0) == 0
    # the assignment
    assign = lambda **kw: L.tohip_assign_greedy(*[kw.get(k, b) for k, b in zip(   # noqa: E731
        ("cost", "R", "C", "ld", "min_cost", "col", "row", "stream"), (p, 3, 5, 5, 0, q, r, None))])
    for kw in (dict(cost=None), dict(col=None), dict(row=None), dict(R=0), dict(R=65), dict(C=0), dict(C=4097), dict(ld=4), dict(min_cost=-1)):
        assert assign(**kw) == EINVAL, kw
