"""The information a view gains and the greedy selection by it, on the GPU.  Every comparison is exact (torch.equal or integer
equality).  The oracle of a view is a composition of calls that are pinned elsewhere: the candidate voxels (weight > 0, from
EvidenceMap.dense()) as a grid whose export() gives the centres, ops.cull_waypoints(normalize=True) the kept rows,
tools.line_of_sight(map.occupied, t, centre, skip=(1, 0)) == 1 the seen ones, EvidenceMap.log_odds their values, a table gather and a
sum.  At the smallest case the numpy restatement synth.view_information_ref is compared too."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import scan_size_cases as ssc

from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
ORIGIN, RES = (0.0, 0.0, 0.0), 0.125
WHOLE, USUAL = (0.01, 50.0), (0.5, 5.0)
SCENE = dict(origin=(-0.5, -0.5, -0.5), resolution=0.125, dims=(28, 24, 16))
SCANNER = np.float32([1.03, 0.97, 0.52])
CAMERA = dict(intrins=torch.from_numpy(K), img_width=IW, img_height=IH)
LMIN, LMAX, THRESHOLD = -40, 70, 0
UNIT = np.zeros(256, dtype=np.int64)
UNIT[0] = 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cam(limits):
    from trajectory_optimization_amd import ops
    return ops.Camera(K, IW, IH, *limits)


def _values(dims, seed, unknown=0.3, occupied=0.1):
    """Random evidence values (nx,ny,nz) int8: -128 for a share `unknown`, (threshold, lmax] for a share `occupied`, else [lmin,
    threshold]."""
    rng = np.random.default_rng(seed + 31 * dims[0])
    u = rng.random(dims)
    L = rng.integers(LMIN, THRESHOLD + 1, dims)
    L = np.where(u < unknown + occupied, rng.integers(THRESHOLD + 1, LMAX + 1, dims), L)
    return np.where(u < unknown, -128, L).astype(np.int8)


def _table(seed, zeros=0.3):
    rng = np.random.default_rng(seed)
    W = rng.integers(1, 65536, 256)
    W[rng.random(256) < zeros] = 0
    W[[LMIN + 128, 255]] = 65535, 65535
    return W.astype(np.int64)


def _map(L, dev, origin=ORIGIN):
    from trajectory_optimization_amd import ops
    return ops.EvidenceMap(origin, RES, L.shape, lmin=LMIN, lmax=LMAX, threshold=THRESHOLD, device=dev).load(_t(L.astype(np.int64), dev))


def _grid_of(bits, origin, dev):
    """An OccupancyGrid holding exactly the voxels of `bits` (their centres inserted)."""
    from trajectory_optimization_amd import ops
    g = ops.OccupancyGrid(origin, RES, bits.shape, device=dev)
    _, centres = synth.occ_export_ref(bits, origin, RES)
    if len(centres):
        assert g.insert(_t(centres, dev)) == 0
    return g


def _views(dims, M, seed=1):
    """M views of a grid at ORIGIN / RES: [0] from the apron in front of the face x = 0 looking along +x at the grid's middle, [1] a
    position exactly on voxel faces inside dims, [2] out of range, the rest uniform over the box and a rim around it with random
    orientations whose quaternions are not unit."""
    rng = np.random.default_rng(seed + 7 * dims[1])
    ext = np.asarray(dims, dtype=np.float64) * RES
    n = max(M, 3)
    P = rng.random((n, 3)) * ext * 1.6 - 0.3 * ext
    Q = rng.standard_normal((n, 4)) * (0.5 + rng.random((n, 1)))
    P[0], Q[0] = [-0.5, ext[1] / 2, ext[2] / 2], synth.Q_OPTICAL
    P[1] = np.minimum(np.floor(np.asarray(dims) / 2), np.asarray(dims) - 1) * RES
    P[2] = [600.0, 0.1, 0.1]
    return P[:M].astype(np.float32), Q[:M].astype(np.float32)


def composition(m, W, P, Q, limits, dev, origin=ORIGIN):
    """The oracle -> (gains (M,) int64, informed masks (M, nx,ny,nz) bool, kept counts), on the device, from existing ops only."""
    from trajectory_optimization_amd import ops, tools
    Wd = _t(W, dev)
    weights = Wd[m.dense().long() + 128]
    ijk, centres = _grid_of((weights > 0).cpu().numpy(), origin, dev).export()
    M = len(P)
    masks = torch.zeros((M,) + tuple(m.dims), dtype=torch.bool, device=dev)
    gains = torch.zeros(M, dtype=torch.int64, device=dev)
    if not len(ijk):
        return gains, masks, [0] * M
    p, q = _t(P, dev), _t(Q, dev)
    kept_idx, _, counts, _ = ops.cull_waypoints(centres, p, q, _cam(limits), limits[0], limits[1], normalize=True)
    for w in range(M):
        kept = kept_idx[w, :counts[w]].long()
        c = centres[kept]
        see = tools.line_of_sight(m.occupied, p[w].expand_as(c).contiguous(), c, skip=(1, 0)) == 1
        if not bool(see.any()):
            continue
        values, _ = m.log_odds(c[see].contiguous())
        gains[w] = Wd[values.long() + 128].sum()
        v = ijk[kept].long()[see]
        masks[w, v[:, 0], v[:, 1], v[:, 2]] = True
    return gains, masks, counts


def _gain_of(masks, weights):
    return (masks.long() * weights[None]).reshape(len(masks), -1).sum(dim=1)


# --------------------------------------------------------------------------------------------------------- pads and the map level

def test_single_voxel_grid(dev):
    from trajectory_optimization_amd import ops
    W = np.zeros(256, dtype=np.int64)
    W[0] = 7
    m = _map(np.full((1, 1, 1), -128, np.int8), dev)
    assert int(m.information(W)) == 7 and m.uncertain(W).count() == 1
    assert m.uncertain(W).buf[256:].view(torch.int32).tolist() == [1]           # one bit: 31 pad voxels of the brick hold -128 too
    p = _t(np.float32([[-0.5, 0.0625, 0.0625], [-0.5, 0.0625, 0.0625]]), dev)
    q = _t(np.stack([ssc.Q_PLUS_X, synth.quat_mul(np.array([0.0, 0.0, 0.0, 1.0]), synth.Q_OPTICAL).astype(np.float32)]), dev)
    assert ops.view_information(m, p, q, _cam(WHOLE), *WHOLE, table=W).tolist() == [7, 0]
    m.load(torch.full((1, 1, 1), LMAX, device=dev))
    W[LMAX + 128] = 9
    assert int(m.information(W)) == 9 and ops.view_information(m, p, q, _cam(WHOLE), *WHOLE, table=W).tolist() == [9, 0]   # occupied, informed


def test_pads_never_count(dev):
    """(5, 6, 3) untouched, W[0] = 7: the 2 x 2 x 2 bricks hold 256 bytes of -128, 90 of them inside dims."""
    from trajectory_optimization_amd import ops
    dims = (5, 6, 3)
    W = np.zeros(256, dtype=np.int64)
    W[0] = 7
    L = np.full(dims, -128, np.int8)
    m = _map(L, dev)
    assert int(m.information(W)) == 7 * 90
    plane = m.uncertain(W)
    assert plane.count() == 90 and bool(plane.dense().all()) and not bool(plane.buf[:256].any())
    words = plane.buf[256:].view(torch.int32)
    assert sum(int(((words >> b) & 1).sum()) for b in range(32)) == 90
    P, Q = _views(dims, 12)
    cam = _cam(WHOLE)
    mark = m.occupied.empty_like()
    got = ops.view_information(m, _t(P, dev), _t(Q, dev), cam, *WHOLE, table=W, mark=mark)
    ii = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), axis=-1).reshape(-1, 3)
    centres = synth.voxel_centres(dims, ORIGIN, RES).reshape(-1, 3)
    kept_idx, _, counts, _ = ops.cull_waypoints(_t(centres, dev), _t(P, dev), _t(Q, dev), cam, *WHOLE, normalize=True)
    union = np.zeros(dims, bool)
    for w in range(len(P)):
        kept = np.zeros(dims, bool)
        rows = ii[kept_idx[w, :counts[w]].cpu().numpy()]
        kept[rows[:, 0], rows[:, 1], rows[:, 2]] = True
        gain, informed = synth.view_information_ref(kept, P[w], ORIGIN, RES, L, np.zeros(dims, bool), W)
        assert int(got[w]) == gain and gain % 7 == 0, w
        union |= informed
    assert int(got.sum()) > 0 and torch.equal(mark.dense().cpu(), torch.from_numpy(union)) and mark.count() == int(union.sum())


@pytest.mark.parametrize("dims", [(5, 6, 3), (37, 21, 20), (64, 64, 32)], ids=str)
def test_information_and_uncertain_equal_numpy(dev, dims):
    L = _values(dims, 0)
    m = _map(L, dev)
    for W in (_table(1), _table(2, zeros=0.9), np.zeros(256, dtype=np.int64), np.full(256, 65535)):
        weights = synth.information_weights_ref(m.dense().cpu().numpy(), W)
        assert np.array_equal(m.dense().cpu().numpy(), L)
        total = m.information(W)
        assert total.dtype == torch.int64 and total.dim() == 0 and total.device == m.device and int(total) == int(weights.sum())
        plane = m.uncertain(W)
        assert torch.equal(plane.dense().cpu(), torch.from_numpy(weights > 0)) and plane.count() == int((weights > 0).sum())   # (no pad bit)
        assert not bool(plane.buf[:256].any())
        assert int(m.information(_t(W, dev).to(torch.int32))) == int(total)       # a device table of another integer dtype
    # the default table: information_table of the map's settings
    from trajectory_optimization_amd import tools
    T = tools.information_table(m)
    assert int(m.information()) == int(m.information(T)) == int(synth.information_weights_ref(L, T.to(torch.int64).numpy()).sum()) > 0
    settled = _map(np.where(L > THRESHOLD, LMAX, LMIN).astype(np.int8), dev)
    assert int(settled.information()) == 0 and settled.uncertain().count() == 0   # a finished map


# --------------------------------------------------------------------------------------------------------- the unit table

@pytest.fixture(scope="module")
def room(dev):
    """The doorway room of tests/test_hip_view_volume.py, one scan into an evidence map."""
    from trajectory_optimization_amd import tools
    em = tools.evidence_map(tools.occupancy_grid(origin=SCENE["origin"], dims=SCENE["dims"], resolution=SCENE["resolution"], device=dev))
    assert em.integrate(_t(SCANNER, dev), _t(synth.box_room(doorway=True), dev)) == 0
    return em


def _candidates():
    return synth.candidate_grid([0.6, 1.0, 1.4], [0.8, 1.0], 0.5, 2)   # M = 12; every second one looks towards the doorway


def test_unit_table_gives_the_volume(dev, room):
    from trajectory_optimization_amd import ops
    cases = [(room, *_candidates(), USUAL)]
    for dims in ((37, 21, 20), (64, 64, 32)):
        cases.append((_map(_values(dims, 3), dev), *_views(dims, 17), WHOLE))
    for m, P, Q, limits in cases:
        p, q, cam = _t(P, dev), _t(Q, dev), _cam(limits)
        mark_v, mark_i = m.occupied.empty_like(), m.occupied.empty_like()
        want = ops.view_volume(m.space, p, q, cam, *limits, mark=mark_v)
        got = ops.view_information(m, p, q, cam, *limits, table=UNIT, mark=mark_i)
        assert torch.equal(got, want) and torch.equal(mark_i.buf, mark_v.buf) and int(want.sum()) > 0
        assert torch.equal(m.uncertain(UNIT).buf, m.space.unknown().buf) and int(m.information(UNIT)) == m.space.unknown().count()
        for k in (1, 3, len(P)):
            a = ops.view_volume_select(m.space, p, q, cam, *limits, k)
            b = ops.view_information_select(m, p, q, cam, *limits, k, table=UNIT)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].buf, b[2].buf) and int(a[0][0]) >= 0


# --------------------------------------------------------------------------------------------------------- random maps, random tables

@pytest.mark.parametrize("M", [1, 3, 17])
@pytest.mark.parametrize("dims", [(5, 6, 3), (37, 21, 20), (64, 64, 32)], ids=str)
def test_gains_equal_the_composition(dev, dims, M):
    """(37, 21, 20): 600 brick words, no axis a multiple of the brick; (64, 64, 32): 4096 words, every axis one — both more than one
    slab of 256 words under WHOLE, whose window is the whole grid."""
    from trajectory_optimization_amd import ops
    L, W = _values(dims, 5), _table(6)
    m = _map(L, dev)
    P, Q = _views(dims, M)
    p, q = _t(P, dev), _t(Q, dev)
    before = m.buf.clone(), m.occupied.buf.clone(), m.free.buf.clone()
    weights = _t(synth.information_weights_ref(L, W), dev)
    claimed_bits = np.random.default_rng(5).random(dims) < 0.5
    claimed = _grid_of(claimed_bits, ORIGIN, dev)
    for limits in ((WHOLE, USUAL) if M <= 3 else (WHOLE,)):
        want, masks, kept = composition(m, W, P, Q, limits, dev)
        assert torch.equal(want, _gain_of(masks, weights))
        cam = _cam(limits)
        stats, stats_all = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
        mark, mark_all = m.occupied.empty_like(), m.occupied.empty_like()
        got = ops.view_information(m, p, q, cam, *limits, table=W, mark=mark, stats=stats)
        print(dims, M, limits, "gains", got.tolist()[:6], "kept", list(kept)[:6], "stats", stats.tolist())
        assert got.dtype == torch.int64 and torch.equal(got, want), (limits, got.tolist(), want.tolist())
        assert torch.equal(mark.dense(), masks.any(dim=0)) and mark.count() == int(masks.any(dim=0).sum())
        in_range = synth.occ_fixed(P, ORIGIN, RES)[1]
        assert int(stats[1]) == sum(int(k) for k, ok in zip(kept, in_range) if ok)      # rays walked = the oracle's kept rows
        got_all = ops.view_information(m, p, q, cam, *limits, table=W, mark=mark_all, window=False, stats=stats_all)
        assert torch.equal(got_all, got) and torch.equal(mark_all.buf, mark.buf)            # window off: the same gains, the same plane
        assert stats_all.tolist()[1:] == stats.tolist()[1:] and int(stats[0]) <= int(stats_all[0])
        assert int(stats_all[0]) == int((weights > 0).sum()) * int(in_range.sum())
        assert torch.equal(ops.view_information(m, p, q, cam, *limits, table=W), got)       # twice: the same tensor
        # a claimed plane: each gain drops by exactly the claimed informed voxels' weights
        cl = _t(claimed_bits, dev)
        got_cl = ops.view_information(m, p, q, cam, *limits, table=W, claimed=claimed)
        assert torch.equal(got_cl, _gain_of(masks & ~cl[None], weights)) and torch.equal(got - got_cl, _gain_of(masks & cl[None], weights))
        if M >= 3:
            assert int(got[2]) == 0   # a camera out of range informs nothing
    assert int(ops.view_information(m, p, q, _cam(WHOLE), *WHOLE, table=W)[0]) > 0           # (the first view does look at the grid)
    occ = torch.from_numpy(L > THRESHOLD).to(dev)
    assert bool((masks.any(dim=0) & occ).any()) or M == 1 or dims == (5, 6, 3)              # occupied voxels are among the informed
    assert all(torch.equal(a, b) for a, b in zip(before, (m.buf, m.occupied.buf, m.free.buf)))


def test_smallest_case_against_the_numpy_restatement(dev):
    from trajectory_optimization_amd import ops
    dims = (5, 6, 3)
    L, W = _values(dims, 5, unknown=0.2, occupied=0.2), _table(6, zeros=0.1)
    m = _map(L, dev)
    occ = L > THRESHOLD
    P, Q = _views(dims, 12)
    cam = _cam(WHOLE)
    got = ops.view_information(m, _t(P, dev), _t(Q, dev), cam, *WHOLE, table=W).tolist()
    ii = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), axis=-1).reshape(-1, 3)
    centres = synth.voxel_centres(dims, ORIGIN, RES).reshape(-1, 3)
    kept_idx, _, counts, _ = ops.cull_waypoints(_t(centres, dev), _t(P, dev), _t(Q, dev), cam, *WHOLE, normalize=True)
    informed_occupied = 0
    for w in range(len(P)):
        kept = np.zeros(dims, bool)
        rows = ii[kept_idx[w, :counts[w]].cpu().numpy()]
        kept[rows[:, 0], rows[:, 1], rows[:, 2]] = True
        gain, informed = synth.view_information_ref(kept, P[w], ORIGIN, RES, L, occ, W)
        one = ops.view_information(m, _t(P[w:w + 1], dev), _t(Q[w:w + 1], dev), cam, *WHOLE, table=W, mark=(mk := m.occupied.empty_like()))
        assert got[w] == gain == int(one[0]) and torch.equal(mk.dense().cpu(), torch.from_numpy(informed)), w
        informed_occupied += int((informed & occ).sum())
    assert sum(got) > 0 and informed_occupied > 0


# --------------------------------------------------------------------------------------------------------- capacity and 64 bits

def test_the_queue_at_capacity(dev):
    """tests/scan_size_cases.py A1: (16, 16, 64), two slabs of 256 bricks, every voxel a candidate and kept, nothing in the way — 8192
    entries per slab, the LDS queue's capacity, in the weighted instantiation."""
    from trajectory_optimization_amd import ops
    dims, limits = ssc.A1_DIMS, ssc.A1_LIMITS
    rng = np.random.default_rng(16)
    L = rng.integers(LMIN, THRESHOLD + 1, dims).astype(np.int8)   # every voxel observed and free: nothing blocks
    L[rng.random(dims) < 0.25] = -128
    W = rng.integers(1, 65536, 256).astype(np.int64)              # no zero: every voxel is a candidate
    m = _map(L, dev)
    assert m.uncertain(W).count() == 16384 == 2 * ssc.limits()["vol_queue"] and ssc.n_words(dims) == 2 * ssc.limits()["vol_slab"]
    stats = torch.zeros(3, dtype=torch.int64, device=dev)
    mark = m.occupied.empty_like()
    p, q = _t(ssc.A1_POSE, dev), _t(ssc.A1_QUAT, dev)
    got = ops.view_information(m, p, q, _cam(limits), *limits, table=W, mark=mark, stats=stats)
    want, masks, kept = composition(m, W, ssc.A1_POSE, ssc.A1_QUAT, limits, dev)
    assert int(kept[0]) == 16384 and stats.tolist()[:2] == [16384, 16384]
    assert torch.equal(got, want) and int(got[0]) == int(synth.information_weights_ref(L, W).sum()) and mark.count() == 16384
    assert torch.equal(ops.view_information(m, p, q, _cam(limits), *limits, table=W, window=False), got)


def test_gains_beyond_32_bits(dev):
    from trajectory_optimization_amd import ops
    dims = (64, 64, 64)
    m = ops.EvidenceMap(ORIGIN, RES, dims, device=dev)            # untouched: every byte -128, nothing blocks
    W = np.full(256, 65535, dtype=np.int64)
    P, Q = np.float32([[-3.0, 4.0, 4.0]]), ssc.Q_PLUS_X[None]
    centres = _t(synth.voxel_centres(dims, ORIGIN, RES).reshape(-1, 3), dev)
    _, _, counts, _ = ops.cull_waypoints(centres, _t(P, dev), _t(Q, dev), _cam(WHOLE), *WHOLE, normalize=True)
    ref = int(counts[0]) * 65535
    assert int(counts[0]) > 65537 and ref > 1 << 32
    got = ops.view_information(m, _t(P, dev), _t(Q, dev), _cam(WHOLE), *WHOLE, table=W)
    assert int(got[0]) == ref
    assert int(m.information(W)) == 65535 * 64 ** 3 > 1 << 32


# --------------------------------------------------------------------------------------------------------- claimed and mark

def test_mark_is_claimed_only_for_one_view(dev):
    import ctypes

    from trajectory_optimization_amd import _lib, ops
    from trajectory_optimization_amd._lib import ptr
    dims = (37, 21, 20)
    L, W = _values(dims, 8), _table(9)
    m = _map(L, dev)
    weights = _t(synth.information_weights_ref(L, W), dev)
    P, Q = _views(dims, 3)
    p, q, cam = _t(P, dev), _t(Q, dev), _cam(WHOLE)
    plane = m.occupied.empty_like()
    with pytest.raises(ValueError, match="mark may be the claimed plane itself only for one view"):
        ops.view_information(m, p, q, cam, *WHOLE, table=W, claimed=plane, mark=plane)
    gains = torch.zeros(3, dtype=torch.int64, device=dev)
    t = ops.check_information_table(W, dev)
    cand = m.uncertain(W)
    rc = _lib.lib().tohip_view_information(ptr(m.occupied.buf), ptr(m.free.buf), ptr(plane.buf), ptr(plane.buf), plane.buf.numel(),
                                           ctypes.byref(m.geom), ptr(m.buf), m.buf.numel(), ptr(t), ptr(cand.buf), ptr(p), ptr(q), 3, None, cam.ref(),
                                           0.01, 50.0, 1, ptr(gains), None, None, None, 0)
    assert rc == -1 and plane.count() == 0
    # one view: it claims what it counts, and a second launch finds nothing left
    first = ops.view_information(m, p[:1], q[:1], cam, *WHOLE, table=W, claimed=plane, mark=plane)
    assert int(first[0]) > 0 and int(first[0]) == int((weights * plane.dense()).sum())
    n = plane.count()
    assert int(ops.view_information(m, p[:1], q[:1], cam, *WHOLE, table=W, claimed=plane, mark=plane)[0]) == 0 and plane.count() == n


# --------------------------------------------------------------------------------------------------------- selection

@pytest.fixture(scope="module")
def selection_case(dev):
    """A random map in the room's box, the 12 candidates of the volume tests, their informed sets from the composition."""
    L, W = _values(SCENE["dims"], 11, unknown=0.4, occupied=0.03), _table(12)
    m = _map(L, dev, SCENE["origin"])
    P, Q = _candidates()
    gains, masks, _ = composition(m, W, P, Q, USUAL, dev, SCENE["origin"])
    return m, L, W, P, Q, masks.cpu().numpy(), synth.information_weights_ref(L, W)


@pytest.mark.parametrize("k", [1, 3, 12])
def test_selection_equals_the_restatement(dev, selection_case, k):
    from trajectory_optimization_amd import tools
    m, L, W, P, Q, masks, weights = selection_case
    rng = np.random.default_rng(3)
    for claimed_bits in (None, rng.random(SCENE["dims"]) < 0.3):
        claimed = None if claimed_bits is None else _grid_of(claimed_bits, SCENE["origin"], dev)
        kept = None if claimed is None else claimed.buf.clone()
        order, gains, mask = synth.information_select_ref(masks, weights, k, 1, claimed_bits)
        sel = tools.select_views_information(m, _t(P, dev), _t(Q, dev), k, table=W, claimed=claimed, min_dist=0.5, max_dist=5.0, **CAMERA)
        print("selection", k, claimed is not None, sel.order.tolist(), sel.gains.tolist())
        assert sel.order.dtype == torch.int64 and sel.gains.dtype == torch.int64
        assert sel.order.tolist() == order and sel.gains.tolist() == gains and sel.n_selected == len(order) >= 1
        assert torch.equal(sel.revealed.dense().cpu(), torch.from_numpy(mask)) and sel.total == sum(gains)
        assert torch.equal(sel.poses.cpu(), torch.from_numpy(P[order])) and torch.equal(sel.quats.cpu(), torch.from_numpy(Q[order]))
        assert sel.travel is None and sel.table.dtype == torch.uint16 and sel.table.to(torch.int64).tolist() == W.tolist()
        if claimed is not None:
            assert torch.equal(claimed.buf, kept)   # the caller's plane is not modified
        assert gains == sorted(gains, reverse=True)   # (submodular: marginal gains only fall)


def test_selection_ties_duplicates_min_gain_zero_table_and_a_team(dev, selection_case):
    from trajectory_optimization_amd import ops, tools
    m, L, W, P, Q, masks, weights = selection_case
    cam = dict(min_dist=0.5, max_dist=5.0, **CAMERA)
    single = np.array([int(weights[s].sum()) for s in masks])
    best = int(np.argmax(single))
    # the best candidate twice, in front: the lower index wins the tie, and the twin is never chosen
    P2, Q2 = np.concatenate([P[[best, best]], P]), np.concatenate([Q[[best, best]], Q])
    sel = tools.select_views_information(m, _t(P2, dev), _t(Q2, dev), 14, table=W, **cam)
    order = sel.order.tolist()
    assert order[0] == 0 and 1 not in order and 2 + best not in order and len(set(order)) == len(order) and int(sel.gains[0]) == single[best]
    # min_gain above the best gain: nothing; exactly the best gain: that view and no other
    none = tools.select_views_information(m, _t(P, dev), _t(Q, dev), 3, min_gain=int(single.max()) + 1, table=W, **cam)
    assert none.n_selected == 0 and none.total == 0 and none.revealed.count() == 0
    one = tools.select_views_information(m, _t(P, dev), _t(Q, dev), 3, min_gain=int(single.max()), table=W, **cam)
    assert one.order.tolist() == [best]
    # an all-zero table: the selection stops at round 0
    order, picked, revealed = ops.view_information_select(m, _t(P, dev), _t(Q, dev), _cam(USUAL), *USUAL, 5, table=np.zeros(256, dtype=np.int64))
    assert order.tolist() == [-1] * 5 and picked.tolist() == [0] * 5 and revealed.count() == 0
    # a team: the second robot is handed the first's revealed plane as claimed and chooses disjoint voxels
    a = tools.select_views_information(m, _t(P, dev), _t(Q, dev), 2, table=W, **cam)
    b = tools.select_views_information(m, _t(P, dev), _t(Q, dev), 2, table=W, claimed=a.revealed, **cam)
    both = tools.select_views_information(m, _t(P, dev), _t(Q, dev), 4, table=W, **cam)
    assert a.order.tolist() + b.order.tolist() == both.order.tolist() and a.gains.tolist() + b.gains.tolist() == both.gains.tolist()
    assert torch.equal(b.revealed.buf, both.revealed.buf) and not (set(a.order.tolist()) & set(b.order.tolist()))
    new = b.revealed.dense() & ~a.revealed.dense()
    assert b.total == int((_t(weights, dev) * new).sum()) > 0


def test_travel_prices_the_trip(dev, selection_case):
    from trajectory_optimization_amd import ops
    m, L, W, P, Q, masks, weights = selection_case
    p, q = _t(P, dev), _t(Q, dev)
    cost = torch.arange(12, dtype=torch.int64, device=dev) * 64
    cost[0] = -1                                                   # (unreachable)
    order, picked, _ = ops.view_information_select(m, p, q, _cam(USUAL), *USUAL, 1, table=W, travel_cost=cost, travel_m=3)
    single = np.array([int(weights[s].sum()) for s in masks])
    score = np.where(cost.cpu().numpy() < 0, -1 << 62, single * (1 << 20) - 3 * cost.cpu().numpy())
    assert int(order[0]) == int(np.argmax(score)) != 0 and int(picked[0]) == single[int(order[0])]


# --------------------------------------------------------------------------------------------------------- the map changes between calls

def test_an_integrate_between_two_calls_is_seen(dev):
    from trajectory_optimization_amd import tools
    m = tools.evidence_map(tools.occupancy_grid(origin=SCENE["origin"], dims=SCENE["dims"], resolution=SCENE["resolution"], device=dev))
    m.integrate(_t(SCANNER, dev), _t(synth.box_room(doorway=True), dev))
    P, Q = _candidates()
    p, q = _t(P, dev), _t(Q, dev)
    cam = dict(min_dist=0.5, max_dist=5.0, **CAMERA)
    T = tools.information_table(m).to(torch.int64).numpy()
    results = []
    for scan in (None, synth.doorway_beams(SCANNER), synth.box_room(doorway=True)):
        if scan is not None:
            m.integrate(_t(SCANNER, dev), _t(scan, dev), 1.5 if len(results) == 1 else None)
        got = tools.view_information(m, p, q, **cam)
        want, _, _ = composition(m, T, P, Q, USUAL, dev, SCENE["origin"])
        assert torch.equal(got, want) and int(got.sum()) > 0
        results.append((got, int(m.information())))
    assert not torch.equal(results[0][0], results[1][0]) and not torch.equal(results[1][0], results[2][0])
    assert results[0][1] > results[1][1] > results[2][1]          # every scan leaves less to learn


def test_the_example_runs(dev, capsys):
    spec = importlib.util.spec_from_file_location("information_exploration_sample", os.path.join(REPO, "examples", "information_exploration_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["-k", "3", "--rounds", "1"])
    assert out["volume_views"] == 0 and out["information_views"][0] >= 1
    assert out["information"][1] < out["information"][0]
    text = capsys.readouterr().out
    assert "by volume: 0 views" in text and "by information, round 0" in text and "information left" in text
