"""Re-framing and merging maps on the GPU (reframe_kernels.hip; ops.*.reframed / merge, tools.reframe_map / follow_map / merge_maps):
every comparison is torch.equal against the numpy restatements (synth.occ_transfer_ref / evidence_transfer_ref, themselves checked
against a per-voxel loop in tests/test_reframe_cpu.py) — a plane's words after the header, pads included; an evidence buffer byte
for byte with pads and header, both derived planes word for word, and the counts.  Then the maps as the rest of the chain sees them.

Through the chain every point lies on the 1/1024 m lattice at r = 1/8 and origins that are multiples of r: there every f32
subtraction and division of the index rule is exact, so the two frames index — and walk — identically."""
import ctypes

import numpy as np
import pytest
import torch

import reframe_cases as cases
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
ORIGIN, RES = (-1.0, 2.0, 0.5), 0.125
PAIR_IDS = [f"{a}->{b}" for a, b in cases.PAIRS]
SHIFTS = cases.RESIDUE_SHIFTS + cases.NO_OVERLAP[:4]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _moved(origin, shift):
    """The origin `shift` voxels from `origin` (exact at these origins and RES)."""
    return tuple(float(o + s * RES) for o, s in zip(origin, shift))


def _words(bits):
    return torch.from_numpy(cases.plane_words(bits).view(np.uint8).copy())


def _plane(bits, dev, origin=ORIGIN):
    """An OccupancyGrid holding exactly `bits`: its words written behind the header."""
    from trajectory_optimization_amd import ops
    g = ops.OccupancyGrid(origin, RES, bits.shape, device=dev)
    g.buf[256:] = _words(bits).to(dev)
    return g


def _evid(L, dev, params, origin=ORIGIN):
    """An EvidenceMap holding exactly the values L, its two planes exact."""
    from trajectory_optimization_amd import ops
    m = ops.EvidenceMap(origin, RES, L.shape, device=dev, **params)
    m.buf.copy_(_t(synth.evidence_brick_order(L), dev))
    occ, free = synth.evidence_planes_ref(L, m.threshold)
    m.occupied.buf[256:] = _words(occ).to(dev)
    m.free.buf[256:] = _words(free).to(dev)
    return m


def _assert_plane_is(g, bits, what=""):
    assert not bool(g.buf[:256].any()), what                       # the header as init leaves it
    assert torch.equal(g.buf[256:].cpu(), _words(bits)), what      # word for word, the pads included


def _assert_map_is(m, L, what=""):
    """The map holds exactly the values L: the buffer byte for byte (header and pads included) and both derived planes word for word."""
    assert torch.equal(m.buf.cpu(), torch.from_numpy(synth.evidence_brick_order(L))), what
    occ, free = synth.evidence_planes_ref(L, m.threshold)
    assert torch.equal(m.occupied.buf[256:].cpu(), _words(occ)) and torch.equal(m.free.buf[256:].cpu(), _words(free)), what
    assert torch.equal(m.dense().cpu(), torch.from_numpy(np.asarray(L).astype(np.int8))), what
    for plane in (m._scan.occupied, m._scan.free):
        assert not bool(plane.buf.any()), what                     # the scratch planes are empty


def _occ_transfer(src, dst, shift, mode, counts):
    from trajectory_optimization_amd import ops
    ops._map_call(dst.device, "tohip_occ_transfer", *src._sizes(), *dst._sizes(), *shift, mode, ops.ptr(counts))


# ------------------------------------------------------------------------------------------------------------ planes

@pytest.mark.parametrize("pair", cases.PAIRS, ids=PAIR_IDS)
def test_plane_transfer_equals_the_restatement(dev, pair):
    sd, dd = pair
    for fill in cases.FILLS:
        bits, old = cases.plane_bits(sd, fill), cases.plane_bits(dd, 0.3, seed=1)
        src = _plane(bits, dev)
        before = src.buf.clone()
        for shift in SHIFTS:
            what = (fill, shift)
            want, count = synth.occ_transfer_ref(bits, old, shift, "copy")
            # COPY through the public method: a new grid, its origin moved by the shift
            out = src.reframed(shift=shift, dims=dd)
            assert out is not src and out.dims == dd and out.resolution == src.resolution and out.device == src.device, what
            assert out.origin.tobytes() == np.asarray(_moved(ORIGIN, shift), dtype=f32).tobytes(), what
            _assert_plane_is(out, want, what)
            # COPY through the entry into a destination full of ones, pads too: every word is written, the count is the bits set
            dst = _plane(old, dev)
            dst.buf[256:] = 0xFF
            counts = torch.zeros(1, dtype=torch.int64, device=dev)
            _occ_transfer(src, dst, shift, 0, counts)
            _assert_plane_is(dst, want, what)
            assert int(counts) == count, what
            # OR through merge: the source's origin is the shift away, the count adds up over two calls
            want, count = synth.occ_transfer_ref(bits, old, shift, "or")
            dst, other = _plane(old, dev), _plane(bits, dev, _moved(ORIGIN, [-s for s in shift]))
            assert dst.merge(other, counts=counts) is dst, what
            _assert_plane_is(dst, want, what)
            assert int(counts) == synth.occ_transfer_ref(bits, old, shift, "copy")[1] + count, what
            assert torch.equal(other.buf, before), what
            if shift in cases.NO_OVERLAP:
                assert not want.any() or np.array_equal(want, old), what
                assert not bool(out.buf.any()) and count == 0, what   # an empty copy, an unchanged union
        assert torch.equal(src.buf, before), fill   # the source is only read
    if min(sd) > 1 and min(dd) > 1:
        assert synth.occ_transfer_ref(cases.plane_bits(sd, 1.0), cases.plane_bits(dd, 0.0), (0, 0, 0), "copy")[1] == np.prod(np.minimum(sd, dd))


def test_space_map_reframed_and_merge(dev):
    from trajectory_optimization_amd import ops, tools
    sd, dd, shift = (13, 10, 7), (9, 11, 5), (3, -2, 1)
    occ, free = cases.plane_bits(sd, 0.2), cases.plane_bits(sd, 0.6, seed=1)
    space = ops.SpaceMap(_plane(occ, dev), _plane(free, dev))
    before = space.occupied.buf.clone(), space.free.buf.clone()
    out = tools.reframe_map(space, shift=shift, dims=dd)
    assert isinstance(out, ops.SpaceMap) and out.occupied is not space.occupied and out.free is not space.free and out.free is not out.occupied
    _assert_plane_is(out.occupied, synth.occ_transfer_ref(occ, np.zeros(dd, bool), shift, "copy")[0])
    _assert_plane_is(out.free, synth.occ_transfer_ref(free, np.zeros(dd, bool), shift, "copy")[0])
    # merge: the union of both planes over the overlap, the other map only read
    old_o, old_f = cases.plane_bits(dd, 0.3, seed=2), cases.plane_bits(dd, 0.3, seed=3)
    mine = ops.SpaceMap(_plane(old_o, dev, _moved(ORIGIN, shift)), _plane(old_f, dev, _moved(ORIGIN, shift)))
    assert mine.merge(space) is mine
    _assert_plane_is(mine.occupied, synth.occ_transfer_ref(occ, old_o, shift, "or")[0])
    _assert_plane_is(mine.free, synth.occ_transfer_ref(free, old_f, shift, "or")[0])
    assert torch.equal(space.occupied.buf, before[0]) and torch.equal(space.free.buf, before[1])


# ------------------------------------------------------------------------------------------------------------ evidence

@pytest.mark.parametrize("name", list(cases.PARAMS))
@pytest.mark.parametrize("pair", cases.PAIRS, ids=PAIR_IDS)
def test_evidence_transfer_equals_the_restatement(dev, pair, name):
    sd, dd = pair
    params = cases.PARAMS[name]
    # the source holds values over the whole byte range: beyond the destination's clamps under the default parameters
    L_src, L_dst = cases.evid_values(sd, "wide"), cases.evid_values(dd, name, seed=1)
    src = _evid(L_src, dev, cases.WIDE)
    before = src.buf.clone(), src.occupied.buf.clone(), src.free.buf.clone()
    clamped = {"add": [False, False], "confident": [False, False]}
    for shift in SHIFTS:
        # COPY through the public method: a new map of the source's parameters
        want, counts = synth.evidence_transfer_ref(L_src, L_dst, shift, "copy", cases.WIDE)
        out = src.reframed(shift=shift, dims=dd)
        assert out is not src and out.params == src.params and out.dims == dd and out.buf.data_ptr() != src.buf.data_ptr(), shift
        assert out.origin.tobytes() == np.asarray(_moved(ORIGIN, shift), dtype=f32).tobytes(), shift
        assert out.space.occupied is out.occupied and out.space.free is out.free
        _assert_map_is(out, want, shift)
        assert out.last_counts() == tuple(counts.tolist()), shift
        for mode in ("add", "confident"):
            want, counts = synth.evidence_transfer_ref(L_src, L_dst, shift, mode, params)
            dst, other = _evid(L_dst, dev, params, _moved(ORIGIN, shift)), src   # (merge computes the shift from the two origins)
            assert dst.merge(other, mode=mode) is dst, (shift, mode)
            _assert_map_is(dst, want, (shift, mode))
            assert dst.last_counts() == tuple(counts.tolist()), (shift, mode)
            given = torch.zeros(4, dtype=torch.int64, device=dev)
            again = _evid(L_dst, dev, params, _moved(ORIGIN, shift))
            again.merge(other, mode=mode, counts=given).merge(other, mode=mode, counts=given)   # (+= over two calls)
            twice, counts2 = synth.evidence_transfer_ref(L_src, want, shift, mode, params)
            _assert_map_is(again, twice, (shift, mode, "twice"))
            assert given.cpu().tolist() == (counts + counts2).tolist(), (shift, mode)
            if mode == "confident":
                assert np.array_equal(twice, want) and not counts2.any(), shift   # idempotent
            S = synth.shifted_window(L_src, dd, shift, -128)
            known = S != -128
            base = np.where(L_dst == -128, 0, L_dst) + S if mode == "add" else S
            clamped[mode][0] |= bool((known & (base > params["lmax"])).any())
            clamped[mode][1] |= bool((known & (base < params["lmin"])).any())
            if shift in cases.NO_OVERLAP:
                assert np.array_equal(want, L_dst) and not counts.any(), (shift, mode)
    if min(sd) > 1 and min(dd) > 1:
        assert clamped["add"] == [True, True], "ADD reaches both clamps"
        assert name == "wide" or clamped["confident"] == [True, True], "a source beyond the destination's clamps is clamped"
    for a, b in zip(before, (src.buf, src.occupied.buf, src.free.buf)):
        assert torch.equal(a, b)   # the source is only read


def test_confident_tie_and_clamps_by_value(dev):
    dims = (5, 6, 3)
    S = np.full(dims, -128, dtype=np.int64)
    D = np.full(dims, -128, dtype=np.int64)
    # along x: the tie both ways round, a stronger negative, a source above lmax and one below lmin; then an unknown source, an
    # unknown destination, and zero against unknown
    S[:, 0, 0], D[:, 0, 0] = [9, -9, -30, 127, -127], [-9, 9, 20, 60, -39]
    S[:3, 1, 1], D[:3, 1, 1] = [-128, 5, 0], [7, -128, -128]
    for shift in ((0, 0, 0), (1, 1, 1)):
        src = _evid(S, dev, cases.WIDE)
        Dm = np.roll(D, [-s for s in shift], axis=(0, 1, 2)) if any(shift) else D   # (the planted voxels meet again under the shift)
        dst = _evid(Dm, dev, cases.DEFAULT, _moved(ORIGIN, shift))
        want, counts = synth.evidence_transfer_ref(S, Dm, shift, "confident", cases.DEFAULT)
        dst.merge(src, mode="confident")
        _assert_map_is(dst, want, shift)
        assert dst.last_counts() == tuple(counts.tolist())
        if not any(shift):
            assert want[:, 0, 0].tolist() == [9, 9, -30, 70, -40] and want[:3, 1, 1].tolist() == [7, 5, 0]


# ------------------------------------------------------------------------------------------------------------ at size

@pytest.mark.parametrize("grow", [True, False], ids=["into_the_large_box", "into_the_small_box"])
def test_planes_at_size(dev, grow):
    """More destination words than one pass of the launch covers, a ragged tail, an unaligned shift."""
    c = cases.size_case()
    sd, dd = (cases.SIZE_SMALL, cases.SIZE_BIG) if grow else (cases.SIZE_BIG, cases.SIZE_SMALL)
    shift = cases.SIZE_SHIFT if grow else tuple(-s for s in cases.SIZE_SHIFT)
    bits, old = c["bits"][sd], c["bits"][dd]
    src = _plane(bits, dev)
    before = src.buf.clone()
    want, count = synth.occ_transfer_ref(bits, old, shift, "copy")
    _assert_plane_is(src.reframed(shift=shift, dims=dd), want)
    want_or, count_or = synth.occ_transfer_ref(bits, old, shift, "or")
    dst = _plane(old, dev, _moved(ORIGIN, shift))
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    dst.merge(src, counts=counts)
    _assert_plane_is(dst, want_or)
    assert int(counts) == count_or and count > 0 and 0 < count_or < count
    assert torch.equal(src.buf, before)


@pytest.mark.parametrize("grow", [True, False], ids=["into_the_large_box", "into_the_small_box"])
def test_evidence_at_size(dev, grow):
    c = cases.size_case()
    sd, dd = (cases.SIZE_SMALL, cases.SIZE_BIG) if grow else (cases.SIZE_BIG, cases.SIZE_SMALL)
    shift = cases.SIZE_SHIFT if grow else tuple(-s for s in cases.SIZE_SHIFT)
    L_src, L_dst = c["vals"][sd], c["vals"][dd]
    src = _evid(L_src, dev, cases.DEFAULT)
    before = src.buf.clone()
    if not grow:   # (COPY into the large box: test_planes_at_size; here the references of 21 M values are kept to one)
        want, counts = synth.evidence_transfer_ref(L_src, L_dst, shift, "copy")
        out = src.reframed(shift=shift, dims=dd)
        _assert_map_is(out, want)
        assert out.last_counts() == tuple(counts.tolist())
    mode = "add" if grow else "confident"
    want, counts = synth.evidence_transfer_ref(L_src, L_dst, shift, mode)
    dst = _evid(L_dst, dev, cases.DEFAULT, _moved(ORIGIN, shift))
    dst.merge(src, mode=mode)
    _assert_map_is(dst, want)
    assert dst.last_counts() == tuple(counts.tolist()) and counts[0] > 0
    assert torch.equal(src.buf, before)


# ------------------------------------------------------------------------------------------------------------ through the chain

def _lattice_points(rng, lo, hi, n):
    """n points uniform over [lo, hi) on the 1/1024 m lattice."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return (np.floor((lo + rng.random((n, 3)) * (hi - lo)) * 1024.0) / 1024.0).astype(f32)


def test_insert_then_reframed_equals_insert_into_the_new_box(dev):
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(21)
    sd, dd, shift = (13, 10, 7), (9, 11, 5), (3, -2, 1)
    ext = np.asarray(sd) * RES
    P = _lattice_points(rng, np.asarray(ORIGIN) - 0.3, np.asarray(ORIGIN) + ext + 0.3, 3000)   # a rim outside the old box: skipped rows
    old = ops.OccupancyGrid(ORIGIN, RES, sd, device=dev)
    skipped = old.insert(_t(P, dev))
    q, ok = synth.occ_fixed(P, ORIGIN, RES)
    kept = ok & (((q >> 8) >= 0) & ((q >> 8) < np.asarray(sd))).all(axis=1)
    assert skipped == int((~kept).sum()) > 0
    new = old.reframed(shift=shift, dims=dd)
    direct = ops.OccupancyGrid(_moved(ORIGIN, shift), RES, dd, device=dev)
    direct.insert(_t(P[kept], dev))
    assert new.origin.tobytes() == direct.origin.tobytes() and new.dims == direct.dims
    assert torch.equal(new.buf[256:], direct.buf[256:]) and bool(new.buf[256:].any())
    _assert_plane_is(new, synth.occupancy_ref(P[kept], _moved(ORIGIN, shift), RES, dd)[0])
    # by centre: the position's voxel lands on the middle voxel
    centre = np.asarray(ORIGIN) + (np.asarray([7, 3, 4]) + 0.5) * RES
    by_centre = old.reframed(centre=centre, dims=dd)
    assert torch.equal(by_centre.buf, old.reframed(shift=(7 - 4, 3 - 5, 4 - 2), dims=dd).buf)
    v = torch.tensor([[4, 5, 2]], device=dev)
    assert int(by_centre.lookup(v)) == int(old.lookup(torch.tensor([[7, 3, 4]], device=dev)))


def test_evidence_reframed_then_integrate_equals_the_restatement(dev):
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(22)
    dims, shift = (24, 24, 14), (5, -3, 2)
    origin = (-0.25, -0.25, -0.25)
    scanner = np.asarray([0.5, 1.0, 0.5], dtype=f32)
    scan1 = _lattice_points(rng, (0.0, 0.0, 0.0), (2.5, 2.5, 1.25), 400)
    scan2 = _lattice_points(rng, (0.5, 0.0, 0.25), (2.5, 2.0, 1.25), 400)
    L0 = np.full(dims, -128, dtype=np.int64)
    L1, _, skipped1, _, _ = synth.evidence_scan_ref(L0, scanner, scan1, origin, RES, dims)
    m = ops.EvidenceMap(origin, RES, dims, device=dev)
    assert m.integrate(_t(scanner, dev), _t(scan1, dev)) == skipped1
    _assert_map_is(m, L1, "the old map")
    new = m.reframed(shift=shift)
    _assert_map_is(m, L1, "the old map is untouched")
    new_origin = tuple(float(o + s * RES) for o, s in zip(origin, shift))
    L1s = synth.shifted_window(L1, dims, shift, -128)
    _assert_map_is(new, L1s, "re-framed")
    L2, counts, skipped2, _, _ = synth.evidence_scan_ref(L1s, scanner, scan2, new_origin, RES, dims)
    assert new.integrate(_t(scanner, dev), _t(scan2, dev)) == skipped2
    _assert_map_is(new, L2, "re-framed, then a scan")
    assert new.last_counts() == tuple(counts.tolist())


def test_line_of_sight_and_frontier_over_a_reframed_space_map(dev):
    from trajectory_optimization_amd import ops
    rng = np.random.default_rng(23)
    dims, shift = (13, 10, 7), (2, -1, 1)
    occ, free = cases.plane_bits(dims, 0.05, seed=4), cases.plane_bits(dims, 0.6, seed=5)
    space = ops.SpaceMap(_plane(occ, dev), _plane(free, dev))
    moved = space.reframed(shift=shift)
    # the overlap of the two boxes in the old frame's voxels, and segments with both ends inside it
    lo, hi = np.maximum(0, shift), np.minimum(dims, np.asarray(dims) + shift)
    a = _lattice_points(rng, np.asarray(ORIGIN) + lo * RES, np.asarray(ORIGIN) + hi * RES, 2000)
    b = _lattice_points(rng, np.asarray(ORIGIN) + lo * RES, np.asarray(ORIGIN) + hi * RES, 2000)
    for skip in ((0, 0), (1, 1)):
        want = synth.los_ref(a, b, ORIGIN, RES, occ, skip)
        assert 0 < int((want == 0).sum()) < len(want)
        assert torch.equal(space.occupied.line_of_sight(_t(a, dev), _t(b, dev), skip).cpu(), torch.from_numpy(want))
        assert torch.equal(moved.occupied.line_of_sight(_t(a, dev), _t(b, dev), skip).cpu(), torch.from_numpy(want))
    assert torch.equal(moved.state(_t(a, dev)), space.state(_t(a, dev)))
    # the frontier of the re-framed map is the restatement's over the shifted planes ...
    occ_s, free_s = (synth.occ_transfer_ref(p, np.zeros(dims, bool), shift, "copy")[0] for p in (occ, free))
    fr = moved.frontier()
    want = synth.frontier_ref(occ_s, free_s, 1)
    assert torch.equal(fr.grid.buf[256:].cpu(), _words(want))
    assert fr.n == int(want.sum()) > 0
    # ... and, a voxel away from the overlap's faces, the original's frontier shifted by the offset
    old = synth.frontier_ref(occ, free, 1)
    inner = tuple(slice(l + 1, h - 1) for l, h in zip(lo, hi))
    inner_new = tuple(slice(l + 1 - s, h - 1 - s) for l, h, s in zip(lo, hi, shift))
    assert np.array_equal(want[inner_new], old[inner]) and old[inner].any()


def _room_maps(dev, kind):
    """Two robots' maps of synth.box_room, each from its own half of the scan and in its own box, and one map over the union box
    that took both scans -> (a, b, whole)."""
    from trajectory_optimization_amd import ops
    room = (np.round(synth.box_room(step=0.05).astype(np.float64) * 1024.0) / 1024.0).astype(f32)   # (onto the 1/1024 m lattice)
    half = room[:, 1] < 1.0   # (the second scanner stands at y = 0.75: its rays cross voxels the first robot's rays crossed)
    scans = [(np.asarray([0.5, 1.0, 0.5], dtype=f32), room[half]), (np.asarray([1.5, 0.75, 0.375], dtype=f32), room[~half])]
    frames = [((-0.5, -0.5, -0.25), (28, 28, 14)), ((-0.125, -0.75, -0.125), (24, 26, 12)), ((-0.5, -0.75, -0.25), (28, 30, 14))]

    def new(origin, dims):
        if kind == "space":
            return ops.SpaceMap(ops.OccupancyGrid(origin, RES, dims, device=dev))
        return ops.EvidenceMap(origin, RES, dims, device=dev)

    a, b, whole = (new(*f) for f in frames)
    for m, (scanner, pts) in zip((a, b), scans):
        assert m.integrate(_t(scanner, dev), _t(pts, dev)) == 0
        assert whole.integrate(_t(scanner, dev), _t(pts, dev)) == 0
    return a, b, whole


def test_merge_maps_of_two_half_scans_equals_one_map_of_both(dev):
    from trajectory_optimization_amd import ops, tools
    a, b, whole = _room_maps(dev, "space")
    before = [m.occupied.buf.clone() for m in (a, b)] + [m.free.buf.clone() for m in (a, b)]
    merged = tools.merge_maps([a, b])
    assert isinstance(merged, ops.SpaceMap) and merged is not a and merged.occupied.dims == (28, 30, 14)
    assert merged.occupied.origin.tobytes() == whole.occupied.origin.tobytes()
    for got, want in ((merged.occupied, whole.occupied), (merged.free, whole.free)):
        assert torch.equal(got.buf[256:], want.buf[256:]) and bool(got.buf[256:].any())
    assert torch.equal(tools.merge_maps([b, a]).free.buf, merged.free.buf)
    for x, y in zip(before, [m.occupied.buf for m in (a, b)] + [m.free.buf for m in (a, b)]):
        assert torch.equal(x, y)   # the inputs are only read
    # evidence, independent scans added: the default steps stay inside the clamps over two scans, so the sum is the one map's value
    a, b, whole = _room_maps(dev, "evidence")
    merged = tools.merge_maps([a, b], mode="add")
    assert isinstance(merged, ops.EvidenceMap) and merged.params == a.params and merged.dims == (28, 30, 14)
    assert torch.equal(merged.buf, whole.buf) and torch.equal(merged.occupied.buf[256:], whole.occupied.buf[256:])
    assert torch.equal(merged.free.buf[256:], whole.free.buf[256:]) and bool(merged.occupied.buf[256:].any())
    both = bool(((a.reframed(shift=(0, -2, 0), dims=(28, 30, 14)).dense() != -128) & (b.reframed(shift=(-3, 0, -1), dims=(28, 30, 14)).dense() != -128)).any())
    assert both, "some voxel was observed by both robots"
    # confident: any order and any repetition give the same bytes
    one = tools.merge_maps([a, b])
    for maps in ([b, a], [a, b, a, b], [b, b, a]):
        other = tools.merge_maps(maps, mode="confident")
        assert torch.equal(other.buf, one.buf) and torch.equal(other.occupied.buf, one.occupied.buf) and torch.equal(other.free.buf, one.free.buf)
    assert not torch.equal(tools.merge_maps([a, b, a], mode="add").buf, merged.buf)   # ADD counts a map given twice twice
    # the fused map goes where a map goes
    clusters = tools.frontier_clusters(one)
    assert clusters is not None


def test_follow_map_returns_the_identical_object_inside_the_margin(dev):
    from trajectory_optimization_amd import ops, tools
    dims = (20, 11, 9)
    L = cases.evid_values(dims, "default")
    m = _evid(L, dev, cases.DEFAULT)
    at = lambda i, j, k: tuple(float(o + (v + 0.5) * RES) for o, v in zip(ORIGIN, (i, j, k)))   # noqa: E731
    for v in ((3, 3, 3), (16, 7, 5), (10, 5, 4)):
        assert tools.follow_map(m, at(*v), 3) is m
        assert tools.follow_map(m.space, torch.tensor(at(*v), device=dev), 3) is m.space
    moved = tools.follow_map(m, at(17, 5, 4), 3)
    assert moved is not m and isinstance(moved, ops.EvidenceMap) and moved.dims == dims
    _assert_map_is(moved, synth.shifted_window(L, dims, (7, 0, 0), -128))
    _assert_map_is(m, L)
    assert tools.follow_map(moved, at(17, 5, 4), 3) is moved      # the robot's voxel is the middle one now
    values, state = moved.log_odds(_t(np.asarray([at(17, 5, 4)], dtype=f32), dev))
    assert int(values) == int(L[17, 5, 4]) and int(state) == (0 if L[17, 5, 4] == -128 else (2 if L[17, 5, 4] > 0 else 1))


# ------------------------------------------------------------------------------------------------------------ the C entries

def test_entries_refuse_bad_arguments_and_leave_the_destination(dev):
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    EINVAL, ENOSPC = -1, -2
    sd, dd = (13, 10, 7), (5, 6, 3)
    src, dst = _plane(cases.plane_bits(sd, 0.3), dev), _plane(cases.plane_bits(dd, 0.3, seed=1), dev)
    es, ed = _evid(cases.evid_values(sd, "default"), dev, cases.DEFAULT), _evid(cases.evid_values(dd, "default", seed=1), dev, cases.DEFAULT)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    keep = [t.clone() for t in (dst.buf, ed.buf, ed.occupied.buf, ed.free.buf, src.buf, es.buf)]
    stream = _lib.stream_ptr()
    p = ops.ptr

    def occ(**kw):
        a = dict(src=p(src.buf), src_bytes=src.buf.numel(), src_geom=ctypes.byref(src.geom), dst=p(dst.buf), dst_bytes=dst.buf.numel(),
                 dst_geom=ctypes.byref(dst.geom), sx=1, sy=-2, sz=1, mode=1, counts=p(counts))
        a.update(kw)
        return L.tohip_occ_transfer(*a.values(), stream)

    def evid(**kw):
        a = dict(src=p(es.buf), src_bytes=es.buf.numel(), src_geom=ctypes.byref(es.geom), dst=p(ed.buf), dst_bytes=ed.buf.numel(),
                 dst_geom=ctypes.byref(ed.geom), occ=p(ed.occupied.buf), free=p(ed.free.buf), grid_bytes=ed.occupied.buf.numel(), sx=1, sy=-2, sz=1,
                 mode=1, lmin=-40, lmax=70, threshold=0, counts=p(counts))
        a.update(kw)
        return L.tohip_evid_transfer(*a.values(), stream)

    for call, d, s in ((occ, dst, src), (evid, ed, es)):
        for kw in (dict(src=None), dict(dst=None), dict(src_geom=None), dict(dst_geom=None), dict(src=p(d.buf)), dict(dst=p(s.buf)),
                   dict(counts=p(d.buf)), dict(counts=p(s.buf)), dict(mode=-1), dict(mode=3), dict(sx=4097), dict(sy=-4097), dict(sz=4097)):
            assert call(**kw) == EINVAL, (call.__name__, kw)
        assert call(src_bytes=s.buf.numel() - 1) == ENOSPC and call(dst_bytes=d.buf.numel() - 1) == ENOSPC, call.__name__
    assert occ(mode=2) == EINVAL
    for kw in (dict(occ=None), dict(free=None), dict(occ=p(ed.buf)), dict(free=p(ed.occupied.buf)), dict(free=p(es.buf)), dict(counts=p(ed.free.buf)),
               dict(lmin=-128), dict(lmax=128), dict(threshold=70), dict(lmin=1)):
        assert evid(**kw) == EINVAL, kw
    assert evid(grid_bytes=ed.occupied.buf.numel() - 1) == ENOSPC
    torch.cuda.synchronize()
    for a, b in zip(keep, (dst.buf, ed.buf, ed.occupied.buf, ed.free.buf, src.buf, es.buf)):
        assert torch.equal(a, b)
    assert not bool(counts.any())
    # ... and the same calls with nothing wrong go through
    assert occ() == 0 and evid() == 0 and occ(counts=None) == 0 and evid(counts=None) == 0
    torch.cuda.synchronize()
    assert not torch.equal(keep[0], dst.buf) and not torch.equal(keep[1], ed.buf)
