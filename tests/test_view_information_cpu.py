"""CPU checks of the information gain of a view and the greedy selection by it (no GPU): the two new entry points are declared in the
header and in _lib's table at ABI 15; each refuses bad arguments before any launch; ops.check_view_information and
ops.check_information_table refuse by name; the numpy restatements (synth.view_information_ref / information_select_ref, what the
kernels are compared against bit for bit) are checked on hand cases; and the default table has the shape its definition gives it."""
import ctypes

import numpy as np
import pytest
import torch

from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_evid_weight_plane", "tohip_view_information")


def test_header_and_table_declare_the_new_entries_at_abi_15():
    from trajectory_optimization_amd import _lib
    header, before = check_abi_entries(ENTRIES)
    assert "tohip_view_volume_pick" in before   # the earlier paragraphs stay
    vp = ctypes.c_void_p
    assert _lib.SIGNATURES["tohip_evid_weight_plane"] == (ctypes.c_int, [vp, ctypes.c_size_t, ctypes.POINTER(_lib.OccGeom), vp, vp, ctypes.c_size_t,
                                                                          vp, vp, ctypes.c_int32])
    assert len(_lib.SIGNATURES["tohip_view_information"][1]) == len(_lib.SIGNATURES["tohip_view_volume"][1]) + 5   # + evidence, its size,
    # the table, the plane and the reserved word
    for phrase in ("CANDIDATE", "INFORMED", "L + 128", "the target voxel itself is not tested", "65535 x voxels x 2^20"):
        assert phrase in header, phrase


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    # pointers no call may reach
    occ, free, ev, tab, plane, poses, quats, gains, other = (ctypes.c_void_p(a) for a in (4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288,
                                                                                           1048576))
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))
    ok = geom()
    nb, eb = L.tohip_occ_bytes(64, 64, 32), L.tohip_evid_bytes(64, 64, 32)
    cam = _lib.make_camera(synth.K_INTRINS.reshape(-1).tolist(), synth.IMG_WIDTH, synth.IMG_HEIGHT, 1.0, 5.0)
    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 64, 32)), geom(d=(64, 2049, 32))]
    calls = {
        "plane": (L.tohip_evid_weight_plane, ("evid", "evid_bytes", "geom", "table", "plane", "bytes", "total", "stream", "flags"),
                  (ev, eb, ok, tab, plane, nb, None, None, 0)),
        "info": (L.tohip_view_information, ("occ", "free", "claimed", "mark", "bytes", "geom", "evid", "evid_bytes", "table", "plane", "poses", "quats",
                                            "n", "view_index", "cam", "dmin", "dmax", "window", "gains", "stop", "stats", "stream", "flags"),
                 (occ, free, None, None, nb, ok, ev, eb, tab, plane, poses, quats, 3, None, ctypes.byref(cam), 0.5, 5.0, 1, gains, None, None, None,
                  0)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name, first in (("plane", "evid"), ("info", "occ")):
        assert call(name, **{first: None}) == EINVAL, name
        assert call(name, geom=None) == EINVAL, name
        assert call(name, bytes=nb - 1) == ENOSPC, name        # a plane too small
        assert call(name, evid_bytes=eb - 1) == ENOSPC, name   # an evidence buffer too small
        assert call(name, table=None) == EINVAL, name
        assert call(name, table=ctypes.c_void_p(32769)) == EINVAL, name   # 16-bit words at an odd address
        assert call(name, plane=None) == EINVAL, name
        assert call(name, plane=ev) == EINVAL, name            # the plane is the evidence buffer
        assert call(name, evid=ctypes.c_void_p(16392)) == EINVAL, name    # the values are moved 16 bytes at a time
        assert call(name, flags=1) == EINVAL, name             # (reserved)
        for g in bad_geoms:
            assert call(name, geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    for kw in (dict(evid=None), dict(free=None), dict(free=occ), dict(poses=None), dict(quats=None), dict(cam=None), dict(gains=None),
               dict(n=0), dict(n=-1), dict(n=65536),
               dict(plane=occ), dict(plane=free),        # the plane is one of the map's planes
               dict(mark=occ), dict(mark=free), dict(mark=plane),
               dict(claimed=other, mark=other),          # mark == claimed with three views
               dict(claimed=other, mark=other, n=2)):
        assert call("info", **kw) == EINVAL, kw


def _fake_map(**kw):
    """An EvidenceMap's settings and geometry without a device."""
    from trajectory_optimization_amd import ops

    class G(ops.OccupancyGrid):
        def __init__(self, origin=(0, 0, 0), resolution=0.1, dims=(8, 8, 4), device="cuda:0"):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, resolution, dims)
            self.device = torch.device(device)

    class M(ops.EvidenceMap):
        def __init__(self, dims=(8, 8, 4), params=(17, 8, -40, 70, 0)):
            self.params = params
            self.occupied, self.free = G(dims=dims), G(dims=dims)
            self.space = ops.SpaceMap(self.occupied, self.free)
            self.origin, self.resolution, self.dims, self.device = self.occupied.origin, self.occupied.resolution, self.occupied.dims, self.occupied.device
    return M(**kw), G


def test_check_view_information_names_what_is_wrong():
    from trajectory_optimization_amd import ops, tools
    m, G = _fake_map()
    P, Q = torch.zeros(3, 3), torch.tensor([[1.0, 0, 0, 0]] * 3)
    table = np.arange(256)
    claimed = G()
    assert ops.check_view_information(m, P, Q) == (3, None, 1)
    assert ops.check_view_information(m, P, Q, table, 5, np.int64(7), claimed, G()) == (3, 3, 7)
    assert ops.check_view_information(m, P[:1], Q[:1], table, 1, 1, claimed, claimed) == (1, 1, 1)   # one view may claim what it counts
    for bad in (m.space, m.occupied, None):
        with pytest.raises(ValueError, match="map must be an ops.EvidenceMap \\(a SpaceMap has no evidence bytes"):
            ops.check_view_information(bad, P, Q)
    with pytest.raises(ValueError, match="the map must be an ops.EvidenceMap \\(a SpaceMap has no evidence bytes"):
        tools.view_information(m.space, P, Q, intrins=synth.K_INTRINS, img_width=10, img_height=10)
    with pytest.raises(ValueError, match="select_views_information: the map must be an ops.EvidenceMap"):
        tools.select_views_information(m.space, P, Q, 2, intrins=synth.K_INTRINS, img_width=10, img_height=10)
    with pytest.raises(ValueError, match="select_views_information: the camera is needed: \\['img_height'\\] missing"):
        tools.select_views_information(m, P, Q, 2, intrins=synth.K_INTRINS, img_width=10)
    with pytest.raises(ValueError, match="information_table: the map must be an ops.EvidenceMap"):
        tools.information_table(m.space)
    # the table
    for bad, why in ((np.arange(255), "shape \\(256,\\)"), (np.zeros((2, 128), int), "shape \\(256,\\)"), (np.zeros(256), "256 integers"),
                     (torch.zeros(256), "must hold integers"), (np.full(256, -1), "\\[0, 65535\\]"), (np.full(256, 65536), "\\[0, 65535\\]"),
                     ("table", "256 integers"), (torch.zeros(255, dtype=torch.int16), "shape \\(256,\\)")):
        with pytest.raises(ValueError, match="table.*" + why):
            ops.check_view_information(m, P, Q, bad)
    got = ops.check_information_table(np.arange(65280, 65536))
    assert got.dtype == torch.int16 and got.view(torch.uint16).to(torch.int64).tolist() == list(range(65280, 65536))
    assert ops.check_information_table(torch.from_numpy(np.arange(256, dtype=np.uint16))).tolist() == list(range(256))
    # what check_view_volume checks, through it
    with pytest.raises(ValueError, match="poses holds 3 views, quats 2"):
        ops.check_view_information(m, P, Q[:2])
    with pytest.raises(ValueError, match="k must be an integer >= 1"):
        ops.check_view_information(m, P, Q, table, 0)
    many = torch.zeros(65536, 3), torch.ones(65536, 4)
    assert ops.check_view_information(m, *many) == (65536, None, 1)   # (scoring chunks by 65 535)
    with pytest.raises(ValueError, match="poses holds 65536 candidates, a selection \\(k given\\) takes at most 65535"):
        ops.check_view_information(m, *many, table, 2)
    for bad in (0, -1, 0.5, True, None):
        with pytest.raises(ValueError, match="min_gain must be an integer >= 1 \\(in the table's units\\)"):
            ops.check_view_information(m, P, Q, table, 1, bad)
    for plane in (m.occupied, m.free):
        with pytest.raises(ValueError, match="claimed must not be one of the map's own planes"):
            ops.check_view_information(m, P, Q, claimed=plane)
    with pytest.raises(ValueError, match="mark: its dims differs from the map's"):
        ops.check_view_information(m, P, Q, mark=G(dims=(8, 8, 5)))
    with pytest.raises(ValueError, match="mark may be the claimed plane itself only for one view, got 3 views"):
        ops.check_view_information(m, P, Q, claimed=claimed, mark=claimed)
    # travel=: gain 2^20 must fit 63 bits whatever the table holds
    big, _ = _fake_map(dims=(2048, 2048, 32))   # 2^27 voxels: 65535 x 2^27 x 2^20 < 2^63
    assert ops.check_view_information(big, P, Q, travel=True) == (3, None, 1)
    assert 65535 * (2048 * 2048 * 32) << 20 < 1 << 63 <= 65535 * (2048 * 2048 * 33) << 20
    over, _ = _fake_map(dims=(2048, 2048, 33))
    assert ops.check_view_information(over, P, Q) == (3, None, 1)    # without travel= nothing is multiplied
    with pytest.raises(ValueError, match="travel: a map of 138412032 voxels is too large for a selection with travel="):
        ops.check_view_information(over, P, Q, travel=True)


# ------------------------------------------------------------------------------------------------------------ the restatements

PARAMS = dict(hit=17, miss=8, lmin=-40, lmax=70, threshold=0)


def _corridor(second_wall):
    """Three voxels along x at r = 1, seen from voxel 0: voxel 0 free and settled (lmin), voxel 1 free after one miss (or, with
    second_wall, occupied after one hit), voxel 2 a surface seen once (L = 17): weakly occupied."""
    L = np.array([-40, 17 if second_wall else -8, 17], dtype=np.int8).reshape(3, 1, 1)
    return L, synth.evidence_planes_ref(L, 0)[0]


def test_a_weak_occupied_voxel_is_informed_unless_another_stands_before_it():
    table = np.zeros(256, dtype=np.int64)
    table[[-8 + 128, 17 + 128]] = 5, 300
    kept, t = np.ones((3, 1, 1), bool), [0.5, 0.5, 0.5]
    L, occ = _corridor(False)
    assert occ[:, 0, 0].tolist() == [False, False, True]
    gain, informed = synth.view_information_ref(kept, t, (0, 0, 0), 1.0, L, occ, table)
    assert gain == 305 and informed[:, 0, 0].tolist() == [False, True, True]   # the end of the corridor is occupied and informed
    L, occ = _corridor(True)
    gain, informed = synth.view_information_ref(kept, t, (0, 0, 0), 1.0, L, occ, table)
    assert gain == 300 and informed[:, 0, 0].tolist() == [False, True, False]  # the same voxel behind a second occupied one is not
    # the cull's verdict and the claimed plane take voxels out; a camera out of range informs nothing
    L, occ = _corridor(False)
    assert synth.view_information_ref(kept & (np.arange(3) != 2).reshape(3, 1, 1), t, (0, 0, 0), 1.0, L, occ, table)[0] == 5
    claimed = np.zeros((3, 1, 1), bool)
    claimed[1] = True
    gain, informed = synth.view_information_ref(kept, t, (0, 0, 0), 1.0, L, occ, table, claimed)
    assert gain == 300 and informed[:, 0, 0].tolist() == [False, False, True]
    assert synth.view_information_ref(kept, [5000.0, 0.5, 0.5], (0, 0, 0), 1.0, L, occ, table)[0] == 0
    # the unit table restates view_volume_ref
    unit = np.zeros(256, dtype=np.int64)
    unit[0] = 1
    rng = np.random.default_rng(0)
    L = rng.choice(np.array([-128, -40, -8, 17, 70], dtype=np.int8), size=(6, 5, 3))
    occ, free = synth.evidence_planes_ref(L, 0)
    kept = rng.random(L.shape) < 0.8
    want = synth.view_volume_ref(kept, [0.4, 2.2, 1.6], (0, 0, 0), 1.0, occ, free)
    got = synth.view_information_ref(kept, [0.4, 2.2, 1.6], (0, 0, 0), 1.0, L, occ, unit)
    assert got[0] == want[0] > 0 and np.array_equal(got[1], want[1])


def test_information_select_ref_on_hand_sets():
    S = np.zeros((4, 6, 1, 1), bool)
    S[0, [0, 1, 2]] = True
    S[1, [2, 3, 4]] = True
    S[2, [3, 4, 5]] = True
    S[3, [0]] = True
    w = np.array([1, 1, 10, 1, 1, 1], dtype=np.int64).reshape(6, 1, 1)
    order, gains, mask = synth.information_select_ref(S, w, 4)
    assert order == [0, 2] and gains == [12, 3] and mask.all()      # views 0 and 1 tie at 12: the lower index; then 1 adds 2, 2 adds 3
    assert synth.information_select_ref(S, w, 1)[:2] == ([0], [12])
    assert synth.information_select_ref(S, w, 4, min_gain=4)[:2] == ([0], [12])
    assert synth.information_select_ref(S, w, 4, min_gain=13)[:2] == ([], [])
    claimed = np.zeros((6, 1, 1), bool)
    claimed[2] = True
    order, gains, mask = synth.information_select_ref(S, w, 4, claimed=claimed)
    assert order == [2, 0] and gains == [3, 2] and mask.all() and claimed.sum() == 1
    # weights of one: the count's selection; all-zero weights: nothing is chosen
    ones = np.ones((6, 1, 1), dtype=np.int64)
    assert synth.information_select_ref(S, ones, 4)[:2] == synth.volume_select_ref(S, 4)[:2]
    assert synth.information_select_ref(S, 0 * ones, 4)[:2] == ([], [])
    # 64-bit sums
    assert synth.information_select_ref(S, ones * (1 << 40), 1)[1] == [3 << 40]


def test_the_default_table():
    from trajectory_optimization_amd import ops, tools
    m, _ = _fake_map()
    T = tools.information_table(m)
    assert T.dtype == torch.uint16 and tuple(T.shape) == (256,) and not T.is_cuda
    W = T.to(torch.int64).numpy()
    lmin, lmax, thr = -40, 70, 0
    assert W[0] == 4096 and W[lmin + 128] == 0 and W[lmax + 128] == 0
    assert (W[1:lmin + 128] == 0).all() and (W[lmax + 129:] == 0).all()                # values the map never holds
    assert (np.diff(W[lmin + 128:thr + 129]) >= 0).all() and W[thr + 128] > 0           # free side: the nearer the threshold the more is left
    assert (np.diff(W[thr + 129:lmax + 129]) <= 0).all() and W[thr + 129] > 0           # occupied side: the nearer lmax the less
    assert W.max() <= 65535

    def H(p):
        return -(p * np.log2(p) + (1 - p) * np.log2(1 - p))
    sig = lambda L: 1.0 / (1.0 + np.exp(-0.05 * L))   # noqa: E731
    assert W[-8 + 128] == round(4096 * (H(sig(-8.0)) - H(sig(-40.0)))) and W[17 + 128] == round(4096 * (H(sig(17.0)) - H(sig(70.0))))
    assert W[-8 + 128] > 1600   # one graze at 14 m leaves a voxel far from settled
    # the keywords
    assert int(tools.information_table(m, scale=1000, unknown_bits=2.5)[0]) == 2500
    assert int(tools.information_table(m, scale=65535)[0]) == 65535
    assert tools.information_table(m, unknown_bits=0.0).to(torch.int64)[0] == 0
    with pytest.raises(ValueError, match="the weights do not fit 16 bits"):
        tools.information_table(m, scale=65536)
    for kw in (dict(unit=0.0), dict(unit=float("nan")), dict(scale=-1), dict(unknown_bits=float("inf"))):
        with pytest.raises(ValueError, match="information_table: " + next(iter(kw))):
            tools.information_table(m, **kw)
    # other clamps: still 0 at both
    W2 = ops.information_table((17, 8, -100, 100, 20)).to(torch.int64).numpy()
    assert W2[28] == 0 and W2[228] == 0 and W2[128] > 0 and W2.max() <= 4096
