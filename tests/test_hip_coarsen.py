"""Coarsening maps on the GPU (coarsen_kernels.hip; ops.*.coarsened / merge_fine, tools.coarsen_map / map_pyramid): every comparison
is torch.equal against the numpy restatements (synth.evid_coarsen_ref / occ_coarsen_ref, themselves checked against a per-voxel loop
in tests/test_coarsen_cpu.py) — an evidence buffer byte for byte with header and pads, both derived planes word for word and the four
counts; a plane's words, pads included, and its count.  Then the maps through the public calls, and the clearance field over a
COVER-coarsened map against the fine map's, exact in integers."""
import ctypes

import numpy as np
import pytest
import torch

import coarsen_cases as cases
import reframe_cases as rfc
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
U = synth.EVID_UNKNOWN


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _words(bits):
    return torch.from_numpy(rfc.plane_words(bits).view(np.uint8).copy())


def _plane(bits, dev, frame):
    """An OccupancyGrid of `frame` holding exactly `bits`."""
    from trajectory_optimization_amd import ops
    g = ops.OccupancyGrid(frame.origin, frame.resolution, bits.shape, device=dev)
    g.buf[256:] = _words(bits).to(dev)
    return g


def _evid(L, dev, frame, params=cases.PARAMS):
    """An EvidenceMap of `frame` holding exactly the values L, its two planes exact."""
    from trajectory_optimization_amd import ops
    m = ops.EvidenceMap(frame.origin, frame.resolution, L.shape, device=dev, **params)
    m.buf.copy_(_t(synth.evidence_brick_order(L), dev))
    occ, free = synth.evidence_planes_ref(L, m.threshold)
    m.occupied.buf[256:] = _words(occ).to(dev)
    m.free.buf[256:] = _words(free).to(dev)
    return m


def _assert_plane_is(g, bits, what=""):
    assert not bool(g.buf[:256].any()), what                       # the header as init leaves it
    assert torch.equal(g.buf[256:].cpu(), _words(bits)), what      # word for word, the pads included


def _assert_map_is(m, L, what=""):
    assert torch.equal(m.buf.cpu(), torch.from_numpy(synth.evidence_brick_order(L))), what   # header and pads included
    occ, free = synth.evidence_planes_ref(L, m.threshold)
    assert torch.equal(m.occupied.buf[256:].cpu(), _words(occ)) and torch.equal(m.free.buf[256:].cpu(), _words(free)), what


def _empty(dims):
    return np.full(dims, U, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------ the two entries

@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_entries_equal_the_restatement(dev, case):
    f, o = case.factor, case.offset
    for fill in cases.FILLS:
        sb, vb, db, L_src, L_dst = cases.inputs(case, fill)
        src_p, veto_p, src_e = _plane(sb, dev, case.src), _plane(vb, dev, case.src), _evid(L_src, dev, case.src)
        before = [b.clone() for b in (src_p.buf, veto_p.buf, src_e.buf, src_e.occupied.buf, src_e.free.buf)]
        for rule, veto in (("any", None), ("all", None), ("any", veto_p)):
            for mode in cases.OCC_MODES:
                want, count = synth.occ_coarsen_ref(sb, db, f, o, rule, mode, veto=None if veto is None else vb)
                dst = _plane(db, dev, case.dst)
                if mode == "copy":
                    dst.buf[256:] = 0xFF                             # ones, pads too: every word is written
                counts = torch.zeros(1, dtype=torch.int64, device=dev)
                dst._coarsen(src_p, f, o, rule, mode, counts, veto)
                _assert_plane_is(dst, want, (fill, rule, mode, veto is not None))
                assert int(counts) == count, (fill, rule, mode, veto is not None)
        for rule in cases.EVID_RULES:
            for mode in cases.EVID_MODES:
                want, count4 = synth.evid_coarsen_ref(L_src, L_dst, f, o, rule, mode, cases.PARAMS)
                dst = _evid(L_dst, dev, case.dst)
                if mode == "copy":
                    dst.buf[256:] = 0x11                             # stale values, pads too, and stale planes: everything is written
                    dst.occupied.buf[256:] = 0xFF
                    dst.free.buf[256:] = 0xFF
                counts = torch.zeros(4, dtype=torch.int64, device=dev)
                dst._coarsen(src_e, f, o, rule, mode, counts)
                _assert_map_is(dst, want, (fill, rule, mode))
                assert counts.cpu().tolist() == count4.tolist(), (fill, rule, mode)
        for a, b in zip(before, (src_p.buf, veto_p.buf, src_e.buf, src_e.occupied.buf, src_e.free.buf)):
            assert torch.equal(a, b), fill                           # the sources are only read


@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_a_merge_equals_a_copy_and_then_the_transfer(dev, case):
    """CONFIDENT / ADD into a populated dst = COPY into an empty map of dst's box, then tohip_evid_transfer at shift 0 in that mode:
    the bytes, both planes and the second step's counts."""
    L_src, L_dst = cases.values(case.src.dims, 0.5), cases.values(case.dst.dims, 0.6, seed=1)
    src = _evid(L_src, dev, case.src)
    for rule in cases.EVID_RULES:
        middle = _evid(_empty(case.dst.dims), dev, case.dst)
        middle._coarsen(src, case.factor, case.offset, rule, "copy", None)
        for mode in ("add", "confident"):
            one, two = _evid(L_dst, dev, case.dst), _evid(L_dst, dev, case.dst)
            c1, c2 = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
            one._coarsen(src, case.factor, case.offset, rule, mode, c1)
            two._transfer(middle, (0, 0, 0), mode, c2)
            assert torch.equal(one.buf, two.buf) and torch.equal(one.occupied.buf, two.occupied.buf) and torch.equal(one.free.buf, two.free.buf), (rule, mode)
            assert torch.equal(c1, c2), (rule, mode)


@pytest.mark.parametrize("rule", cases.EVID_RULES)
def test_confident_is_idempotent(dev, rule):
    case = cases.BY_NAME["f=3 box an odd offset"]
    src = _evid(cases.values(case.src.dims, 0.5), dev, case.src)
    dst = _evid(cases.values(case.dst.dims, 0.6, seed=1), dev, case.dst)
    dst.merge_fine(src, mode="confident", rule=rule)
    once = dst.buf.clone(), dst.occupied.buf.clone(), dst.free.buf.clone()
    assert dst.last_counts()[0] > 0
    dst.merge_fine(src, mode="confident", rule=rule)
    assert dst.last_counts() == (0, 0, 0, 0)
    for a, b in zip(once, (dst.buf, dst.occupied.buf, dst.free.buf)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["add", "confident"])
@pytest.mark.parametrize("f", [2, 8])
def test_a_brick_with_nothing_to_merge_is_not_written(dev, mode, f):
    """The source's image covers a part of dst only: in ADD and CONFIDENT the bricks whose source values are all -128 keep whatever
    their plane words held — poison here — and the others are rewritten from the new values."""
    case = cases.BY_NAME[f"f={f} box into a bigger map"]
    L_src, L_dst = cases.values(case.src.dims, 1.0), cases.values(case.dst.dims, 0.6, seed=1)
    S = synth.evid_coarsen_sample_ref(L_src, case.dst.dims, f, case.offset, "max")
    nb = tuple((n + s - 1) // s for n, s in zip(case.dst.dims, (4, 4, 2)))
    pad = np.zeros((4 * nb[0], 4 * nb[1], 2 * nb[2]), bool)
    pad[:case.dst.dims[0], :case.dst.dims[1], :case.dst.dims[2]] = S != U
    written = pad.reshape(nb[0], 4, nb[1], 4, nb[2], 2).any(axis=(1, 3, 5)).transpose(2, 1, 0).reshape(-1)   # word order: z, y, x
    assert written.any() and not written.all()
    dst = _evid(L_dst, dev, case.dst)
    poison = torch.full((int((~written).sum()),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    skip = _t(~written, dev)
    for plane in (dst.occupied, dst.free):
        plane.buf[256:].view(torch.int32)[skip] = poison
    dst._coarsen(_evid(L_src, dev, case.src), f, case.offset, "max", mode, None)
    want, _ = synth.evid_coarsen_ref(L_src, L_dst, f, case.offset, "max", mode, cases.PARAMS)
    assert torch.equal(dst.buf.cpu(), torch.from_numpy(synth.evidence_brick_order(want)))
    for plane, bits in zip((dst.occupied, dst.free), synth.evidence_planes_ref(want, 0)):
        words = plane.buf[256:].view(torch.int32)
        assert torch.equal(words[skip], poison)
        assert torch.equal(words[~skip].cpu(), _words(bits).view(torch.int32)[torch.from_numpy(written)])


# ------------------------------------------------------------------------------------------------------------ sizes

def _torch_sample(L, dst_dims, f, o, rule, thr):
    """The source values S (dst_dims, int64) by torch ops on L's device: the dst voxels the source's image touches are padded to whole
    groups of f^3 children, reshaped and reduced under the rule's key; every other voxel is -128."""
    dev, ns = L.device, tuple(L.shape)
    S = torch.full(dst_dims, U, dtype=torch.int64, device=dev)
    lo = [max(0, (-oa) // f) for oa in o]
    hi = [min(nd, (n - 1 - oa) // f + 1) for nd, n, oa in zip(dst_dims, ns, o)]
    if any(h <= l for l, h in zip(lo, hi)):
        return S
    m = [h - l for l, h in zip(lo, hi)]
    first = [f * l + oa for l, oa in zip(lo, o)]                   # the source voxel of the window's voxel 0
    win = torch.full([f * n for n in m], U, dtype=torch.int64, device=dev)
    to = [slice(max(0, -s), min(f * n, k - s)) for s, n, k in zip(first, m, ns)]
    frm = [slice(t.start + s, t.stop + s) for t, s in zip(to, first)]
    win[to[0], to[1], to[2]] = L[frm[0], frm[1], frm[2]].to(torch.int64)
    C = win.reshape(m[0], f, m[1], f, m[2], f).permute(0, 2, 4, 1, 3, 5).reshape(*m, f ** 3)
    if rule == "max":
        best = C.amax(dim=-1)
    else:
        key = torch.where(C == U, torch.full_like(C, 256), torch.where(C > thr, 640 + C, 128 + C)).amax(dim=-1)
        best = torch.where(key > 512, key - 640, torch.where(key == 256, torch.full_like(key, U), key - 128))
    S[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = best
    return S


def test_the_torch_reference_is_the_restatement(dev):
    for name in ("f=3 box an odd offset", "f=8 box into a bigger map", "f=2 box wholly outside", "f=4 box a brick-aligned offset"):
        c = cases.BY_NAME[name]
        L = cases.values(c.src.dims, 0.5)
        for rule in cases.EVID_RULES:
            assert np.array_equal(_torch_sample(_t(L, dev), c.dst.dims, c.factor, c.offset, rule, 0).cpu().numpy(),
                                  synth.evid_coarsen_sample_ref(L, c.dst.dims, c.factor, c.offset, rule, 0)), (name, rule)


@pytest.mark.parametrize("f", cases.FACTORS)
def test_beyond_one_grid_stride_pass(dev, f):
    """More dst bricks than a launch's blocks hold, a ragged tail, for each block shape (8, 4, 2, 1 dst bricks a block); the source
    is small and its image covers dst's last bricks.  The reference comes from torch ops on the device."""
    from trajectory_optimization_amd import ops
    case = cases.big_case(f)
    L = _t(cases.big_values(case.src.dims), dev)
    src = ops.EvidenceMap(case.src.origin, case.src.resolution, case.src.dims, device=dev, **cases.PARAMS).load(L)
    for rule in cases.EVID_RULES:
        S = _torch_sample(L, case.dst.dims, f, case.offset, rule, 0)
        if rule == "max":   # the last brick (voxels 160.., 160.., 20) holds something, the first nothing: the second trip's tail is written
            assert bool((S[160:, 160:, 20:] != U).any()) and bool((S[160:, 160:, 20:] > 0).any()) and bool((S[:4, :4, :2] == U).all())
        want = ops.EvidenceMap(case.dst.origin, case.dst.resolution, case.dst.dims, device=dev, **cases.PARAMS).load(S)
        out = src.coarsened(f, rule=rule, like=case.dst)
        assert torch.equal(out.buf, want.buf) and torch.equal(out.occupied.buf, want.occupied.buf) and torch.equal(out.free.buf, want.free.buf), rule
        known, occ = int((S != U).sum()), int((S > 0).sum())
        assert out.last_counts() == (known, known, occ, 0) and known > 0
    # the plane kernel on the occupied plane: ANY of it is the occupied plane of the values under either rule
    got = src.occupied.coarsened(f, "any", like=case.dst)
    assert torch.equal(got.buf, want.occupied.buf) and bool(got.buf[-4:].any())


@pytest.mark.parametrize("f", cases.FACTORS)
def test_at_the_per_axis_limit(dev, f):
    case = cases.limit_case(f)
    L_src, L_dst = cases.values(case.src.dims, 0.5), cases.values(case.dst.dims, 0.6, seed=1)
    src = _evid(L_src, dev, case.src)
    for rule in cases.EVID_RULES:
        want, count4 = synth.evid_coarsen_ref(L_src, L_dst, f, case.offset, rule, "add", cases.PARAMS)
        dst = _evid(L_dst, dev, case.dst)
        dst.merge_fine(src, mode="add", rule=rule)
        _assert_map_is(dst, want, rule)
        assert dst.last_counts() == tuple(count4.tolist())
    sb = L_src > 0
    for rule in cases.OCC_RULES:
        want, _ = synth.occ_coarsen_ref(sb, np.zeros(case.dst.dims, bool), f, case.offset, rule, "copy")
        _assert_plane_is(src.occupied.coarsened(f, rule, like=case.dst), want, rule)


def test_argument_errors_leave_the_outputs_untouched(dev):
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    EINVAL, ENOSPC = _lib.CONSTANTS["TOHIP_EINVAL"], _lib.CONSTANTS["TOHIP_ENOSPC"]
    case = cases.BY_NAME["f=2 box an odd offset"]
    src_e, dst_e = _evid(cases.values(case.src.dims, 0.5), dev, case.src), _evid(cases.values(case.dst.dims, 0.6, seed=1), dev, case.dst)
    src_p, dst_p = _plane(cases.bits(case.src.dims, 0.5), dev, case.src), _plane(cases.bits(case.dst.dims, 0.3, seed=1), dev, case.dst)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    outs = (dst_e.buf, dst_e.occupied.buf, dst_e.free.buf, dst_p.buf, counts)
    before = [o.clone() for o in outs]
    s = ops.stream_ptr()
    far = (1 << 20) + 1

    def evid(**kw):
        a = dict(src=ops.ptr(src_e.buf), src_bytes=src_e.buf.numel(), dst=ops.ptr(dst_e.buf), dst_bytes=dst_e.buf.numel(), occ=ops.ptr(dst_e.occupied.buf),
                 free=ops.ptr(dst_e.free.buf), grid_bytes=dst_e.occupied.buf.numel(), factor=2, o=case.offset, rule=0, mode=2, lmin=-40, lmax=70,
                 threshold=0, counts=ops.ptr(counts), flags=0)
        a.update(kw)
        return L.tohip_evid_coarsen(a["src"], a["src_bytes"], ctypes.byref(src_e.geom), a["dst"], a["dst_bytes"], ctypes.byref(dst_e.geom), a["occ"],
                                    a["free"], a["grid_bytes"], a["factor"], *a["o"], a["rule"], a["mode"], a["lmin"], a["lmax"], a["threshold"],
                                    a["counts"], s, a["flags"])

    def occ(**kw):
        a = dict(src=ops.ptr(src_p.buf), src_bytes=src_p.buf.numel(), veto=None, dst=ops.ptr(dst_p.buf), dst_bytes=dst_p.buf.numel(), factor=2,
                 o=case.offset, rule=0, mode=1, counts=ops.ptr(counts), flags=0)
        a.update(kw)
        return L.tohip_occ_coarsen(a["src"], a["src_bytes"], ctypes.byref(src_p.geom), a["veto"], a["dst"], a["dst_bytes"], ctypes.byref(dst_p.geom),
                                   a["factor"], *a["o"], a["rule"], a["mode"], a["counts"], s, a["flags"])

    with torch.cuda.device(dev):
        for fn in (evid, occ):
            for kw in (dict(factor=1), dict(factor=9), dict(o=(far, 0, 0)), dict(o=(0, -far, 0)), dict(o=(0, 0, far)), dict(rule=-1), dict(rule=2),
                       dict(mode=-1), dict(mode=3), dict(flags=1), dict(src=None), dict(dst=None),
                       dict(counts=ops.ptr(dst_e.buf if fn is evid else dst_p.buf))):
                assert fn(**kw) == EINVAL, (fn.__name__, kw)
            assert fn(dst=ops.ptr(src_e.buf if fn is evid else src_p.buf)) == EINVAL      # src and dst the same buffer
            assert fn(src_bytes=100) == ENOSPC and fn(dst_bytes=100) == ENOSPC
        for kw in (dict(occ=ops.ptr(dst_e.free.buf)), dict(free=None), dict(lmin=-128), dict(threshold=70)):
            assert evid(**kw) == EINVAL, kw
        assert evid(grid_bytes=100) == ENOSPC
        for kw in (dict(veto=ops.ptr(dst_p.buf)), dict(veto=ops.ptr(src_p.buf)), dict(veto=ops.ptr(src_e.occupied.buf), rule=1)):
            assert occ(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for a, b in zip(before, outs):
        assert torch.equal(a, b)
    with torch.cuda.device(dev):
        assert evid() == 0 and occ() == 0                                                # ... and the good calls do write
    torch.cuda.synchronize()
    assert not torch.equal(before[0], dst_e.buf) and not torch.equal(before[3], dst_p.buf) and bool(counts.any())


# ------------------------------------------------------------------------------------------------------------ the public calls

@pytest.mark.parametrize("rule", cases.EVID_RULES)
def test_coarsened_of_each_map_class(dev, rule):
    from trajectory_optimization_amd import ops, tools
    src = cases.Frame(cases.ORIGIN, cases.RES, cases.SRC)
    L = cases.values(cases.SRC, 0.5)
    occ_b, fre_b = synth.evidence_planes_ref(L, 0)
    m = _evid(L, dev, src)
    before = m.buf.clone()
    for f, anchor in ((2, "origin"), (3, "world"), (8, "origin")):
        frame, o, _ = ops.check_coarsen(m, f, rule, anchor)
        out = tools.coarsen_map(m, f, rule=rule, anchor=anchor)
        assert isinstance(out, ops.EvidenceMap) and out is not m and out.params == m.params and out.dims == frame.dims
        assert out.origin.tobytes() == frame.origin.tobytes() and out.resolution == float(np.float32(f * cases.RES)) and out.space.occupied is out.occupied
        want, counts = synth.evid_coarsen_ref(L, _empty(frame.dims), f, o, rule, "copy", cases.PARAMS)
        _assert_map_is(out, want, (rule, f))
        assert out.last_counts() == tuple(counts.tolist()) and counts[0] > 0
        for plane in (out._scan.occupied, out._scan.free):
            assert not bool(plane.buf.any())
        # a space map: the planes of the values coarsened under the same rule; a grid: ANY and ALL
        space = tools.coarsen_map(m.space, f, rule=rule, anchor=anchor)
        assert isinstance(space, ops.SpaceMap) and space.occupied is not m.occupied and space.free is not space.occupied
        w_occ, w_free = synth.evidence_planes_ref(want, 0)
        _assert_plane_is(space.occupied, w_occ, (rule, f))
        _assert_plane_is(space.free, w_free, (rule, f))
        assert not bool((space.occupied.buf[256:] & space.free.buf[256:]).any())
        empty = np.zeros(frame.dims, bool)
        for plane_rule in cases.OCC_RULES:
            grid = tools.coarsen_map(m.free, f, rule=plane_rule, anchor=anchor)
            assert isinstance(grid, ops.OccupancyGrid) and grid.dims == frame.dims
            _assert_plane_is(grid, synth.occ_coarsen_ref(fre_b, empty, f, o, plane_rule, "copy")[0], (plane_rule, f))
    assert torch.equal(m.buf, before)
    # origin= and dims=, and like=
    boxed = m.coarsened(2, rule=rule, origin=cases.moved(cases.ORIGIN, (-1, -3, -1)), dims=(5, 9, 3))
    _assert_map_is(boxed, synth.evid_coarsen_ref(L, _empty((5, 9, 3)), 2, (-1, -3, -1), rule, "copy", cases.PARAMS)[0])
    liked = m.coarsened(2, rule=rule, like=boxed)
    assert torch.equal(liked.buf, boxed.buf) and liked.dims == boxed.dims


@pytest.mark.parametrize("rule", cases.EVID_RULES)
def test_the_pyramid_equals_one_coarsening_a_level(dev, rule):
    from trajectory_optimization_amd import ops, tools
    m = _evid(cases.values(cases.SRC, 0.5), dev, cases.Frame(cases.ORIGIN, cases.RES, cases.SRC))
    levels = tools.map_pyramid(m, 3, rule=rule)
    assert len(levels) == 4 and levels[0] is m
    for l in (1, 2, 3):
        once = m.coarsened(2 ** l, rule=rule)
        assert levels[l].dims == once.dims and levels[l].resolution == once.resolution and levels[l].origin.tobytes() == once.origin.tobytes()
        assert torch.equal(levels[l].buf, once.buf) and torch.equal(levels[l].occupied.buf, once.occupied.buf) and torch.equal(levels[l].free.buf, once.free.buf)
    planes = tools.map_pyramid(m.space, 2, rule=rule)
    for l in (1, 2):
        assert isinstance(planes[l], ops.SpaceMap) and torch.equal(planes[l].occupied.buf, levels[l].occupied.buf)
        assert torch.equal(planes[l].free.buf, levels[l].free.buf)
    grids = tools.map_pyramid(m.occupied, 2)
    assert torch.equal(grids[2].buf, levels[2].occupied.buf)


@pytest.mark.parametrize("mode", ["confident", "add"])
def test_merge_fine_of_each_map_class(dev, mode):
    from trajectory_optimization_amd import ops
    case = cases.BY_NAME["f=3 box into a bigger map"]
    L_src, L_dst = cases.values(case.src.dims, 0.5), cases.values(case.dst.dims, 0.6, seed=1)
    fine, coarse = _evid(L_src, dev, case.src), _evid(L_dst, dev, case.dst)
    assert ops.check_merge_fine(coarse, fine, mode) == (3, case.offset, "cover")
    before = fine.buf.clone()
    for rule in cases.EVID_RULES:
        coarse = _evid(L_dst, dev, case.dst)
        assert coarse.merge_fine(fine, mode=mode, rule=rule) is coarse
        want, counts = synth.evid_coarsen_ref(L_src, L_dst, 3, case.offset, rule, mode, cases.PARAMS)
        _assert_map_is(coarse, want, rule)
        assert coarse.last_counts() == tuple(counts.tolist()) and counts[0] > 0
        mine = torch.zeros(4, dtype=torch.int64, device=dev)
        _evid(L_dst, dev, case.dst).merge_fine(fine, mode=mode, rule=rule, counts=mine)
        assert mine.cpu().tolist() == counts.tolist()
    assert torch.equal(fine.buf, before)
    # planes: OR; a SpaceMap under both rules
    (o_s, f_s), (o_d, f_d) = synth.evidence_planes_ref(L_src, 0), synth.evidence_planes_ref(L_dst, 0)
    grid = _plane(o_d, dev, case.dst)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    grid.merge_fine(fine.occupied, counts=count)
    want, n = synth.occ_coarsen_ref(o_s, o_d, 3, case.offset, "any", "or")
    _assert_plane_is(grid, want)
    assert int(count) == n > 0
    for rule in cases.EVID_RULES:
        space = ops.SpaceMap(_plane(o_d, dev, case.dst), _plane(f_d, dev, case.dst))
        space.merge_fine(fine.space, rule=rule)
        _assert_plane_is(space.occupied, want, rule)
        free = synth.occ_coarsen_ref(f_s, f_d, 3, case.offset, "all", "or")[0] if rule == "cover" else synth.occ_coarsen_ref(f_s, f_d, 3, case.offset, "any", "or", veto=o_s)[0]
        _assert_plane_is(space.free, free, rule)
    with pytest.raises(ValueError, match="2 to 8 times finer"):
        fine.merge_fine(coarse)
    with pytest.raises(ValueError, match="resolutions differ"):
        coarse.merge(fine)                                                            # .merge itself stays as it is


def test_coarse_maps_of_one_fine_lattice_merge_as_they_are(dev):
    """anchor='world': two sources at different origins of one fine lattice coarsen onto one coarse lattice, and merge_maps takes them."""
    from trajectory_optimization_amd import ops, tools
    a = _evid(cases.values(cases.SRC, 0.5), dev, cases.Frame(cases.ORIGIN, cases.RES, cases.SRC))
    b = _evid(cases.values(cases.DST, 0.5, seed=1), dev, cases.Frame(cases.moved(cases.ORIGIN, (5, -7, 1)), cases.RES, cases.DST))
    ca, cb = (tools.coarsen_map(m, 3, anchor="world") for m in (a, b))
    k = ops.lattice_offset(ca, cb)
    merged = tools.merge_maps([ca, cb])
    assert merged.resolution == ca.resolution and all(d >= max(x, y) for d, x, y in zip(merged.dims, ca.dims, cb.dims)) and isinstance(k, tuple)


# ------------------------------------------------------------------------------------------------------------ planning on a coarse map

def _room_values():
    """Outer walls, an L-shaped inner wall and a pillar; walls lmax, inside lmin, outside never observed, and a patch of the inside
    never observed either — the same on every z layer."""
    p = cases.PARAMS
    L = np.full((48, 40, 6), U, dtype=np.int64)
    L[2:46, 2:38, :] = p["lmin"]
    for sl in ((slice(2, 46), 2), (slice(2, 46), 37), (2, slice(2, 38)), (45, slice(2, 38)), (slice(14, 30), 14), (29, slice(14, 28)), (slice(8, 11), slice(26, 30))):
        L[sl[0], sl[1], :] = p["lmax"]
    L[36:41, 20:23, :] = U
    return L


@pytest.mark.parametrize("unknown", ["free", "obstacle"])
@pytest.mark.parametrize("f", [2, 3])
def test_the_coarse_clearance_field_never_overstates_the_fine_one(dev, f, unknown):
    """c2: the clearance field over the COVER-coarsened map at a voxel's parent; g2: the fine field at the voxel; both squared gaps
    in their own voxels, 65535 beyond their truncation D.  Per axis u - v - 1 >= f (U - V - 1) for a fine obstacle u of parent U, and
    every fine obstacle's parent is a coarse obstacle under COVER, so f^2 c2 <= g2 wherever both are known, and where the coarse field
    sees no obstacle within D_c the fine one sees none within f D_c ("Coarsening maps")."""
    from trajectory_optimization_amd import tools
    m = _evid(_room_values(), dev, cases.Frame((-3.0, -2.5, 0.0), cases.RES, (48, 40, 6)))
    coarse = tools.coarsen_map(m, f, rule="cover")
    max_dist = 0.375
    fine_field, coarse_field = tools.clearance_field(m.space, max_dist, unknown), tools.clearance_field(coarse.space, max_dist, unknown)
    D_c = synth.field_max_dist_voxels(max_dist, coarse.resolution)
    g2 = fine_field.dense().to(torch.int64)
    parent = [torch.arange(n, device=dev) // f for n in m.dims]
    c2 = coarse_field.dense().to(torch.int64)[parent[0][:, None, None], parent[1][None, :, None], parent[2][None, None, :]]
    INF = synth.FIELD_SENTINEL
    near, far = c2 != INF, c2 == INF
    assert bool(((g2 == INF) | (f * f * c2 <= g2))[near].all())
    assert bool(((g2 == INF) | (g2 > f * f * D_c * D_c))[far].all())
    # the room has voxels of every kind: neither statement is vacuous
    assert int((near & (g2 != INF) & (c2 > 0)).sum()) > 0 and int(far.sum()) > 0 and int((c2 == 0).sum()) > 0


def test_the_example_plans_on_a_coarse_level(dev):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "coarse_planning_sample.py")
    spec = importlib.util.spec_from_file_location("coarse_planning_sample", path)
    sample = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sample)
    out = sample.run(device=str(dev), verbose=False, small=True)
    assert out["levels"] == 3 and out["level_dims"][0] == tuple(sample.SMALL["dims"])
    assert all(c <= -(-n // 2) for a, b in zip(out["level_dims"], out["level_dims"][1:]) for n, c in zip(a, b))
    assert out["reachable"] and out["path_rows"] >= 2 and out["fine_legs_clear"]
    assert out["merged_known"] >= out["coarse_known"]
