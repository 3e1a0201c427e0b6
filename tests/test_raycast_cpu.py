"""CPU checks of the ray casts and depth scans (no GPU): the two entry points are declared in the header and in _lib's table; each
refuses bad arguments before any launch; ops.check_depth_scan refuses by name; the numpy restatements (synth.cast_fixed / cast_entry /
scan_rays_ref / depth_scan_ref, what the kernels are compared against bit for bit) are checked on hand cases and against
los_fixed(trace=True); and the shared inputs of the GPU tests meet the conditions that keep those tests from passing vacuously."""
import ctypes
import os

import numpy as np
import pytest
import torch

import raycast_cases as rc
from abi_cases import check_abi_entries

from trajectory_optimization_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_cast_segments", "tohip_depth_scan")


def test_header_and_table_declare_the_new_entries():
    header, before = check_abi_entries(ENTRIES)
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert src.index('#include "volume_kernels.hip"') < src.index('#include "raycast_kernels.hip"')
    for phrase in ("ENTRY PARAMETER", "n_a0 + 256 (k_a - 1)", "-2 an endpoint out of range", "A flag-3 ray marks nothing", "!(depth > min_dist)"):
        assert phrase in header, phrase


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    p, q, r, t, u, v, w, x = (ctypes.c_void_p(a) for a in (64, 4096, 8192, 16384, 32768, 65536, 131072, 262144))   # no call may reach them
    geom = lambda o=(0.0, 0.0, 0.0), res=0.1, d=(64, 64, 32): _lib.OccGeom((ctypes.c_float * 3)(*o), res, (ctypes.c_int32 * 3)(*d))
    ok = geom()
    nb = L.tohip_occ_bytes(64, 64, 32)
    bad_geoms = [geom(o=(0.0, float("nan"), 0.0)), geom(res=0.0), geom(res=float("inf")), geom(d=(0, 64, 32)), geom(d=(64, 2049, 32))]

    def cam(K=None, W=64.0, H=48.0):
        return _lib.make_camera(rc.camera(64, 48).reshape(-1).tolist() if K is None else K, W, H, 1.0, 5.0)

    good = cam()
    calls = {
        "cast": (L.tohip_cast_segments, ("grid", "bytes", "geom", "a", "b", "n", "ss", "es", "voxel", "lam", "stats", "stream"),
                 (p, nb, ok, q, r, 7, 1, 0, t, u, None, None)),
        "scan": (L.tohip_depth_scan, ("grid", "bytes", "geom", "poses", "quats", "n", "cam", "dmin", "dmax", "hit", "pass", "voxel", "depth",
                                      "flags", "points", "stats", "stream"),
                 (p, nb, ok, q, r, 3, ctypes.byref(good), 0.5, 5.0, None, None, t, u, v, None, None, None)),
    }

    def call(name, **kw):
        fn, names, base = calls[name]
        assert set(kw) <= set(names), kw
        return fn(*[kw.get(k, b) for k, b in zip(names, base)])

    for name in calls:
        assert call(name, grid=None) == EINVAL and call(name, geom=None) == EINVAL, name
        assert call(name, bytes=nb - 1) == ENOSPC, name   # grid_bytes too small
        for g in bad_geoms:
            assert call(name, geom=g) == EINVAL, (name, list(g.origin), g.resolution, list(g.dims))
    for kw in (dict(a=None), dict(b=None), dict(voxel=None), dict(lam=None), dict(n=-1), dict(n=(1 << 40) + 1), dict(ss=-1), dict(es=-1),
               dict(ss=8193), dict(es=8193)):
        assert call("cast", **kw) == EINVAL, kw
    assert call("cast", n=0, a=None, b=None, voxel=None, lam=None) == 0   # nothing to do is not an error
    K = rc.camera(64, 48).reshape(-1).tolist()
    edit = lambda i, val: K[:i] + [val] + K[i + 1:]
    bad_cams = [cam(edit(1, 0.5)), cam(edit(3, 0.1)), cam(edit(6, 1e-3)), cam(edit(7, 1e-3)), cam(edit(8, 2.0)), cam(edit(0, 0.0)),
                cam(edit(4, -3.0)), cam(edit(0, float("inf"))), cam(edit(2, float("nan"))),
                cam(W=64.5), cam(H=47.25), cam(W=0.0), cam(H=0.0), cam(W=8193.0), cam(H=float("nan")), cam(W=-4.0)]
    for c in bad_cams:
        assert call("scan", cam=ctypes.byref(c)) == EINVAL, (list(c.K), c.img_width, c.img_height)
    big = cam(W=8192.0, H=8192.0)
    assert call("scan", cam=ctypes.byref(big), n=32) == EINVAL   # 2^31 pixels
    for kw in (dict(poses=None), dict(quats=None), dict(cam=None), dict(voxel=None), dict(depth=None), dict(flags=None), dict(n=0), dict(n=-1),
               dict(n=65536), dict(dmin=5.0), dict(dmin=6.0), dict(dmin=-0.1), dict(dmin=float("nan")), dict(dmax=float("inf")),
               dict(dmax=float("nan")), dict(hit=p), dict({"pass": p}), dict({"hit": w, "pass": w})):
        assert call("scan", **kw) == EINVAL, kw


def test_check_depth_scan_names_what_is_wrong():
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd import tools

    class G(ops.OccupancyGrid):   # a plane's geometry without a device
        def __init__(self, origin=(0, 0, 0), resolution=0.1, dims=(8, 8, 4), device="cuda:0"):
            self.origin, self.resolution, self.dims, _ = ops.check_los(origin, resolution, dims)
            self.device = torch.device(device)

    grid, K = G(), rc.camera(64, 48)
    P, Q = torch.zeros(3, 3), torch.tensor([[1.0, 0, 0, 0]] * 3)
    chk = lambda **kw: ops.check_depth_scan(**{**dict(grid=grid, poses=P, quats=Q, intrins=K, img_width=64, img_height=48, min_dist=0.5,
                                                     max_dist=5.0), **kw})
    assert chk() == (3, 64, 48) and chk(img_width=64.0, hit_plane=G(), pass_plane=G()) == (3, 64, 48) and chk(min_dist=0) == (3, 64, 48)
    assert chk(hit_plane=G()) == (3, 64, 48) and chk(pass_plane=G()) == (3, 64, 48)   # each plane alone
    with pytest.raises(ValueError, match="grid must be an ops.OccupancyGrid"):
        chk(grid=torch.zeros(3))
    for bad in (None, np.zeros((3, 3)), torch.zeros(3, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="poses must be a floating-point tensor"):
            chk(poses=bad)
    for bad in (torch.zeros(3), torch.zeros(3, 4), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match="poses must have shape \\(V,3\\) with V >= 1"):
            chk(poses=bad)
    with pytest.raises(ValueError, match="quats must have shape \\(V,4\\) with V >= 1"):
        chk(quats=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="poses must be finite"):
        chk(poses=P * float("nan"))
    with pytest.raises(ValueError, match="quats must be finite"):
        chk(quats=Q * float("inf"))
    with pytest.raises(ValueError, match="poses holds 3 views, quats 2"):
        chk(quats=Q[:2])
    with pytest.raises(ValueError, match="poses holds 65536 views, a scan takes at most 65535"):
        chk(poses=torch.zeros(65536, 3), quats=torch.ones(65536, 4), img_width=1, img_height=1)
    for bad in (None, "K", np.zeros(8), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="intrins must be 9 finite numbers"):
            chk(intrins=bad)
    for i in (0, 4):
        Kb = K.copy().reshape(-1)
        Kb[i] = 0.0
        with pytest.raises(ValueError, match="intrins must have fx > 0 and fy > 0"):
            chk(intrins=Kb)
    for i, val in ((1, 0.5), (3, 0.5), (6, 0.1), (7, 0.1), (8, 2.0)):
        Kb = K.copy().reshape(-1)
        Kb[i] = val
        with pytest.raises(ValueError, match="no skew and K\\[2\\]\\[2\\] = 1"):
            chk(intrins=Kb)
    for name in ("img_width", "img_height"):
        for bad in (0, -1, 64.5, 8193, None, "64", True, float("nan")):
            with pytest.raises(ValueError, match=name + " must be an integral number in \\[1, 8192\\]"):
                chk(**{name: bad})
    with pytest.raises(ValueError, match="must stay below 2\\^31 pixels, got 8192 x 8192 x 32"):
        chk(poses=torch.zeros(32, 3), quats=torch.ones(32, 4), img_width=8192, img_height=8192)
    for bad in (-0.5, float("nan"), float("inf"), None, "1"):
        with pytest.raises(ValueError, match="min_dist must be a finite number >= 0"):
            chk(min_dist=bad)
    for bad in (0.5, 0.25, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="max_dist must be a finite number > min_dist"):
            chk(max_dist=bad)
    for name in ("hit_plane", "pass_plane"):
        with pytest.raises(ValueError, match=name + " must be an ops.OccupancyGrid or None"):
            chk(**{name: torch.zeros(3)})
        with pytest.raises(ValueError, match=name + " must not be the scanned grid itself"):
            chk(**{name: grid})
        for g, what in ((G(origin=(0, 0, 0.5)), "origin"), (G(resolution=0.2), "resolution"), (G(dims=(8, 8, 5)), "dims"),
                        (G(device="cuda:1"), "device")):
            with pytest.raises(ValueError, match=f"{name}: its {what} differs from the scanned grid's"):
                chk(**{name: g})
    same = G()
    with pytest.raises(ValueError, match="pass_plane must not be the hit plane itself"):
        chk(hit_plane=same, pass_plane=same)
    # the tools layer: the map, the camera keywords and `into`
    cam = dict(intrins=K, img_width=64, img_height=48)
    with pytest.raises(ValueError, match="depth_scan: the map must be an ops.OccupancyGrid, an ops.SpaceMap or an ops.EvidenceMap"):
        tools.depth_scan(torch.zeros(3), P, Q, **cam)
    with pytest.raises(ValueError, match="cast_rays: the map must be an ops.OccupancyGrid"):
        tools.cast_rays(None, P, P)
    with pytest.raises(ValueError, match="depth_scan: the camera is needed: \\['img_height'\\] missing"):
        tools.depth_scan(grid, P, Q, intrins=K, img_width=64)
    with pytest.raises(ValueError, match="depth_scan: unknown keyword\\(s\\) \\['rig'\\]"):
        tools.depth_scan(grid, P, Q, rig=None, **cam)
    with pytest.raises(ValueError, match="depth_scan: into must be an ops.SpaceMap or an ops.EvidenceMap"):
        tools.depth_scan(grid, P, Q, into=G(), **cam)
    with pytest.raises(ValueError, match="depth_scan: into must be a different map"):
        tools.depth_scan(grid, P, Q, into=ops.SpaceMap(grid, G()), **cam)
    space = ops.SpaceMap(grid, G())
    with pytest.raises(ValueError, match="depth_scan: into must be a different map"):
        tools.depth_scan(space, P, Q, into=space, **cam)
    with pytest.raises(ValueError, match="hit_plane: its dims differs"):
        tools.depth_scan(grid, P, Q, into=ops.SpaceMap(G(dims=(8, 8, 5)), G(dims=(8, 8, 5))), **cam)


# ------------------------------------------------------------------------------------------------------------ the restatements

def _line(occupied, skip, A=(128, 128, 128), B=(640, 128, 128)):
    occ = np.zeros((3, 1, 1), bool)
    occ[list(occupied)] = True
    c = synth.cast_fixed([A], [B], occ, skip)
    num, den = synth.cast_entry([A], [B], c["steps"])
    return bool(c["hit"][0]), tuple(int(v) for v in c["voxel"][0]), (int(num[0]), int(den[0])), int(c["visits"][0])


def test_three_voxel_line_under_each_skip_rule():
    """Voxels 0, 1, 2 along x at one unit per voxel; the ray runs from the middle of 0 to the middle of 2."""
    # the hit in voxel 0: tested only with start_skip 0, entered at 0/1
    assert _line([0], (0, 0)) == (True, (0, 0, 0), (0, 1), 1)
    assert _line([0], (1, 0))[0] is False and _line([0], (1, 0))[3] == 2   # voxels 0 and 1 are looked at, the end voxel is not
    # the hit in voxel 1: entered at 128 / 512
    for skip in ((0, 0), (1, 0)):
        assert _line([1], skip) == (True, (1, 0, 0), (128, 512), 2), skip
    assert _line([1], (2, 0))[0] is False      # cheb(v, v0) = 1 < 2
    assert _line([1], (1, 1))[0] is False      # cheb(v, e) = 1 is not > 1: the walk stops before it
    assert _line([1], (1, 1))[3] == 1
    # the hit in voxel 2, the end voxel: never tested with end_skip 0
    for skip in ((0, 0), (1, 0), (2, 3)):
        assert _line([2], skip)[0] is False, skip
    # the first of two wins
    assert _line([0, 1], (0, 0))[1] == (0, 0, 0) and _line([0, 1], (1, 0))[1] == (1, 0, 0)
    assert synth.cast_lam([128], [512]).tolist() == [0.25] and synth.cast_lam([0], [1]).tolist() == [0.0]


def test_cast_ref_codes():
    occ = np.zeros((3, 1, 1), bool)
    occ[1] = True
    a = np.float32([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [5000.0, 0.5, 0.5], [np.nan, 0.5, 0.5], [2.5, 0.5, 0.5]])
    b = np.float32([[2.5, 0.5, 0.5], [0.5, 0.9, 0.5], [2.5, 0.5, 0.5], [2.5, 0.5, 0.5], [-1.5, 0.5, 0.5]])
    voxel, lam, visits = synth.cast_ref(a, b, (0, 0, 0), 1.0, occ)
    assert voxel.tolist() == [1, -1, -2, -2, 1] and visits == 2 + 0 + 2
    assert lam[:2].tolist() == [0.25, 1.0] and np.isnan(lam[2:4]).all() and lam[4] == np.float32(0.125)
    los = synth.los_ref(a, b, (0, 0, 0), 1.0, occ, (1, 0))
    assert ((voxel == -1) == (los == 1)).all() and ((voxel == -2) == (los == 2)).all()


def test_diagonal_through_corners_ties():
    """(1, 1, 1) direction from a voxel's middle: all three faces are crossed at the same parameter, the walk takes x, y, z in turn,
    and the entry of each voxel on the way is that one rational whichever axis stepped last."""
    A, B = [(128, 128, 128)], [(640, 640, 640)]
    for voxel, last in (((1, 0, 0), 0), ((1, 1, 0), 1), ((1, 1, 1), 2)):
        occ = np.zeros((3, 3, 3), bool)
        occ[voxel] = True
        c = synth.cast_fixed(A, B, occ, (1, 0))
        assert c["hit"][0] and tuple(c["voxel"][0]) == voxel and c["last"][0] == last
        n1, d1 = synth.cast_entry(A, B, c["steps"], c["last"])
        n2, d2 = synth.cast_entry(A, B, c["steps"])
        assert (int(n1[0]), int(d1[0])) == (128, 512) == (int(n2[0]), int(d2[0]))
    # tied crossings with different numerators: 128 / 512 along x and 64 / 256 along y are one rational and one f32 quotient
    A, B = [(128, 192, 128)], [(640, 448, 128)]
    occ = np.zeros((3, 2, 1), bool)
    occ[1, 1, 0] = True
    c = synth.cast_fixed(A, B, occ, (1, 0))
    assert c["hit"][0] and c["steps"][0].tolist() == [1, 1, 0] and c["last"][0] == 1
    (n1, d1), (n2, d2) = synth.cast_entry(A, B, c["steps"], c["last"]), synth.cast_entry(A, B, c["steps"])
    assert (int(n1[0]), int(d1[0])) == (64, 256) and (int(n2[0]), int(d2[0])) == (128, 512)
    assert synth.cast_lam(n1, d1).tobytes() == synth.cast_lam(n2, d2).tobytes()


def test_start_on_a_face_moving_down():
    """A on the face x = 1 moving towards -x: its voxel is 1, the face is 0 away, the first step happens at parameter 0 — the hit in
    voxel 0 is entered at the rational 0, however it is written."""
    A, B = [(256, 128, 128)], [(-128, 128, 128)]
    occ = np.zeros((3, 1, 1), bool)
    occ[0] = True
    c = synth.cast_fixed(A, B, occ, (1, 0))
    assert c["hit"][0] and tuple(c["voxel"][0]) == (0, 0, 0) and c["steps"][0].tolist() == [1, 0, 0]
    (n1, d1), (n2, d2) = synth.cast_entry(A, B, c["steps"], c["last"]), synth.cast_entry(A, B, c["steps"])
    assert int(n1[0]) == 0 and int(d1[0]) == 384 and (int(n2[0]), int(d2[0])) == (0, 1)
    assert synth.cast_lam(n1, d1).tolist() == synth.cast_lam(n2, d2).tolist() == [0.0]
    # a scan reports it as blocked nearer than the minimum even with min_dist = 0: !(0 > 0)
    s = synth.depth_scan_ref(np.float32([[1.0, 0.5, 0.5]]), [synth.quat_mul([0.0, 0.0, 0.0, 1.0], synth.Q_OPTICAL)], rc.camera(1, 1), 1, 1, 0.0, 1.5,
                             (0, 0, 0), 1.0, occ)
    assert s["flags"].tolist() == [[[3]]] and s["voxel"].tolist() == [[[0]]] and s["depth"].tolist() == [[[0.0]]]
    assert np.isnan(s["points"]).all() and not s["hit_plane"].any() and not s["pass_plane"].any()


@pytest.fixture(scope="module")
def random_rays():
    occ = rc.plane(rc.MAIN, "p2")
    a, b = rc.segments(rc.MAIN, 5000, seed=3)
    qa, oka = synth.occ_fixed(a, rc.ORIGIN, rc.R)
    qb, okb = synth.occ_fixed(b, rc.ORIGIN, rc.R)
    return occ, a, b, qa, qb, oka & okb


def test_random_rays_against_the_traced_walk(random_rays):
    occ, a, b, qa, qb, ok = random_rays
    A, B = qa[ok], qb[ok]
    assert 4500 < len(A) < 5000
    for skip in ((1, 0), (2, 3)):
        c = synth.cast_fixed(A, B, occ, skip)
        n1, d1 = synth.cast_entry(A, B, c["steps"], c["last"])
        n2, d2 = synth.cast_entry(A, B, c["steps"])
        hit = c["hit"]
        assert 0.2 < hit.mean() < 0.9
        assert (n1[hit] * d2[hit] == n2[hit] * d1[hit]).all()   # the last step's parameter is the maximum over the axes
        assert (synth.cast_lam(n1, d1)[hit] == synth.cast_lam(n2, d2)[hit]).all()
        lam = synth.cast_lam(n2, d2)[hit]
        assert (lam >= 0).all() and (lam <= 1).all() and (n2[hit] <= d2[hit]).all() and (d2 < 1 << 21).all() and (n2 < 1 << 21).all()
        blocked, traces = synth.los_fixed(A, B, occ, skip, trace=True)
        assert (blocked == hit).all()
        dims = np.asarray(occ.shape)
        for r in np.flatnonzero(hit)[:400]:
            tr, v0, e = np.asarray(traces[r]), np.asarray(traces[r][0]), np.asarray(traces[r][-1])
            tested = (np.abs(tr - v0).max(axis=1) >= skip[0]) & (np.abs(tr - e).max(axis=1) > skip[1]) & ((tr >= 0) & (tr < dims)).all(axis=1)
            first = next(k for k in np.flatnonzero(tested) if occ[tuple(tr[k])])
            assert tuple(tr[first]) == tuple(c["voxel"][r]) and c["visits"][r] == first + 1 and c["steps"][r].sum() == first
    voxel, lam, _ = synth.cast_ref(a, b, rc.ORIGIN, rc.R, occ, (1, 0))
    los = synth.los_ref(a, b, rc.ORIGIN, rc.R, occ, (1, 0))
    assert ((voxel == -1) == (los == 1)).all() and ((voxel == -2) == (los == 2)).all() and (voxel == -2).sum() >= 100
    assert (lam[voxel == -1] == 1).all() and np.isnan(lam[voxel == -2]).all()


def test_scan_rays_point_where_the_camera_looks():
    """The convention without a GPU: a pixel right of the image's middle lies to the camera's right (-y of a body looking along +x),
    a pixel below it lies down, the middle pixel's far point is max_dist straight ahead; a quaternion of norm 3 is the same view."""
    K = rc.camera(5, 3)
    t = np.float32([[0.25, -0.5, 1.0]])
    far = synth.scan_rays_ref(t, [synth.Q_OPTICAL], K, 5, 3, 2.0)
    assert far.shape == (1, 3, 5, 3) and far.dtype == np.float32
    np.testing.assert_allclose(far[0, 1, 2], t[0] + [2.0, 0, 0], atol=1e-6)
    np.testing.assert_allclose(far[0, 1, 4] - far[0, 1, 2], [0, -2.0 * 2 / 2.5, 0], atol=1e-6)
    np.testing.assert_allclose(far[0, 2, 2] - far[0, 1, 2], [0, 0, -2.0 * 1 / 2.5], atol=1e-6)
    np.testing.assert_allclose(synth.scan_rays_ref(t, [3 * synth.Q_OPTICAL], K, 5, 3, 2.0), far, atol=1e-6)


def test_depth_scan_ref_on_a_wall():
    """A wall three voxels ahead: depth is the distance to its near face (the ends are snapped to 1/256 voxel), the point its voxel's
    centre, the planes what the rays hit and passed."""
    occ = np.zeros((8, 3, 3), bool)
    occ[4] = True
    s = synth.depth_scan_ref(np.float32([[1.5, 1.5, 1.5]]), [synth.Q_OPTICAL], rc.camera(1, 1), 1, 1, 0.5, 6.0, (0, 0, 0), 1.0, occ)
    assert s["flags"].tolist() == [[[0]]] and s["voxel"].tolist() == [[[4 + 8 * (1 + 3 * 1)]]]
    assert abs(float(s["depth"][0, 0, 0]) - 2.5) < 1e-6 and s["points"][0, 0, 0].tolist() == [4.5, 1.5, 1.5]
    assert np.argwhere(s["hit_plane"]).tolist() == [[4, 1, 1]] and np.argwhere(s["pass_plane"]).tolist() == [[1, 1, 1], [2, 1, 1], [3, 1, 1]]
    assert s["rays"] == 1 and s["visits"] == 4
    # nearer than the minimum: blocked, nothing valid, nothing marked; beyond the maximum: no return, the far point, its voxel unmarked
    s = synth.depth_scan_ref(np.float32([[1.5, 1.5, 1.5]]), [synth.Q_OPTICAL], rc.camera(1, 1), 1, 1, 2.5, 6.0, (0, 0, 0), 1.0, occ)
    assert s["flags"].tolist() == [[[3]]] and not s["hit_plane"].any() and not s["pass_plane"].any() and np.isnan(s["points"]).all()
    s = synth.depth_scan_ref(np.float32([[1.5, 1.5, 1.5]]), [synth.Q_OPTICAL], rc.camera(1, 1), 1, 1, 0.5, 2.0, (0, 0, 0), 1.0, occ)
    assert s["flags"].tolist() == [[[1]]] and s["voxel"].tolist() == [[[-1]]] and np.isinf(s["depth"]).all()
    assert s["points"][0, 0, 0].tolist() == [3.5, 1.5, 1.5] and np.argwhere(s["pass_plane"]).tolist() == [[1, 1, 1], [2, 1, 1]]


# ------------------------------------------------------------------------------------------ conditions on the GPU tests' inputs

def test_main_scene_holds_every_flag():
    s = synth.depth_scan_ref(**rc.main_scene())
    n = s["flags"].size
    share = {f: float((s["flags"] == f).sum()) / n for f in (0, 1, 2, 3)}
    print("main scene flag shares", share)
    for f in (0, 1, 3):
        assert share[f] >= 0.05, share
    assert s["hit_plane"].any() and s["pass_plane"].any() and not (s["hit_plane"] & ~rc.plane(rc.MAIN, "p2")).any()
    for v in range(3):   # every view contributes returns
        assert (s["flags"][v] == 0).any(), v


def test_out_of_range_cameras_skip_every_ray():
    t, q = rc.out_of_range_poses()
    W, H = rc.IMAGES[1]
    s = synth.depth_scan_ref(t, q, rc.camera(W, H), W, H, rc.MIN_DIST, rc.MAX_DIST, rc.ORIGIN, rc.R, rc.plane(rc.MAIN, "p10"))
    assert (s["flags"] == 2).all() and (s["voxel"] == -2).all() and np.isnan(s["depth"]).all() and np.isnan(s["points"]).all()
    assert s["rays"] == 0 and not s["hit_plane"].any() and not s["pass_plane"].any()


def test_segment_cases_hold_every_outcome():
    for dims in rc.GRIDS[1:]:
        a, b = rc.segments(dims, 5000)
        for kind in ("p2", "p10"):
            voxel, _, _ = synth.cast_ref(a, b, rc.ORIGIN, rc.R, rc.plane(dims, kind), (1, 0))
            assert (voxel >= 0).sum() >= 50 and (voxel == -1).sum() >= 50 and (voxel == -2).sum() >= 50, (dims, kind)
    a, b = rc.segments(rc.MAIN, 5000)
    q, ok = synth.occ_fixed(a, rc.ORIGIN, rc.R)
    v = q[ok] >> 8
    assert (((v < 0) | (v >= np.asarray(rc.MAIN))).any(axis=1)).sum() >= 100   # ends in the apron


def test_room_theorems_in_the_restatement():
    """Closed room: from inside no ray escapes.  Doorway: some do, and only through the doorway's voxels."""
    t, q = rc.room_views()
    cam = rc.ROOM_CAMERA
    kw = dict(K=cam["intrins"], img_width=cam["img_width"], img_height=cam["img_height"], min_dist=cam["min_dist"], max_dist=cam["max_dist"],
              origin=rc.ROOM["origin"], resolution=rc.ROOM["resolution"])
    closed = synth.depth_scan_ref(t, q, occ=rc.room_world(False), **kw)
    assert not (closed["flags"] == 1).any() and not (closed["flags"] == 2).any() and (closed["flags"] == 0).mean() > 0.9
    world = rc.room_world(True)
    door = synth.depth_scan_ref(t, q, occ=world, **kw)
    assert (door["flags"] == 1).any()
    assert not (door["hit_plane"] & ~world).any() and not (door["hit_plane"] & door["pass_plane"]).any()
    cam_voxel = tuple(synth.occ_fixed(rc.ROOM_POSE[None], rc.ROOM["origin"], rc.ROOM["resolution"])[0][0] >> 8)
    both = np.argwhere(door["pass_plane"] & world)
    assert all(tuple(v) == cam_voxel for v in both)
