"""CPU checks of greedy view selection (no GPU): the four entry points are declared in the header and in _lib's table with matching
argument counts and without a new ABI version; tohip_views_bytes follows the documented layout; each entry refuses bad arguments
before any launch; every argument the host layer does not accept is refused with a ValueError that names what is wrong, before any
GPU call; the candidate grid is the documented recipe."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from abi_cases import ABI, check_abi_entries

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_views_bytes", "tohip_views_append", "tohip_views_select", "tohip_views_row")


def test_header_and_table_declare_the_views_entries():
    from trajectory_optimization_amd import ops
    header, before = check_abi_entries(ENTRIES)
    assert f"(still {ABI})" in header and "tohip_views_select" in before
    assert f"#define TOHIP_VIEWS_MAX_CHUNK {ops.VIEWS_MAX_CHUNK}\n" in header
    assert f"#define TOHIP_VIEWS_MAX_CANDIDATES {ops.VIEWS_MAX_CANDIDATES}\n" in header
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert '#include "views_kernels.hip"' in src


def test_views_bytes_is_the_documented_layout():
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for n, M, cap in ((5, 1, 1), (20_000, 144, 30_000), (1_000_000, 1024, 10_485_760), (2049, 65536, 77)):
        npad = L.tohip_padded_points(n)
        nseg = (npad + 8191) // 8192
        want = 256 + up(8 * (M + 1)) + up(4 * M) + up(8 * M) + up(4 * M) + up(4 * 256 * nseg) + 2 * up(4 * cap)
        assert L.tohip_views_bytes(n, M, cap) == want == ops.views_layout(npad, M, cap)["total"], (n, M, cap)
    lay = ops.views_layout(L.tohip_padded_points(20_000), 144, 30_000)
    assert lay["header"] == 0 and lay["offsets"] == 256 and lay["val"] - lay["idx"] == up(4 * 30_000)
    for bad in ((0, 4, 4), (-1, 4, 4), (10, 0, 4), (10, 65537, 4), (10, 4, 0), (10, 4, -3), ((1 << 30) + 1, 4, 4)):
        assert L.tohip_views_bytes(*bad) == 0, bad


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)   # a non-null pointer no call may reach: every case below fails its checks first
    n, M, cap = 5000, 12, 4000
    vb = L.tohip_views_bytes(n, M, cap)

    names = ("views", "bytes", "n", "M", "cap", "rows", "first", "n_rows", "needed", "stream")
    base = dict(zip(names, (p, vb, n, M, cap, p, 0, 4, None, None)))
    app = lambda **kw: L.tohip_views_append(*[kw.get(k, base[k]) for k in names])
    assert app(views=None) == EINVAL and app(rows=None) == EINVAL
    assert app(n=0) == EINVAL and app(M=0) == EINVAL and app(M=65537) == EINVAL and app(cap=0) == EINVAL
    assert app(first=-1) == EINVAL and app(n_rows=0) == EINVAL and app(n_rows=257) == EINVAL
    assert app(first=10, n_rows=4) == ENOSPC       # more rows than the set has candidates
    assert app(bytes=vb - 1) == ENOSPC

    names = ("views", "bytes", "n", "M", "cap", "prior", "k", "min_gain", "S", "order", "gain", "n_sel", "stream")
    base = dict(zip(names, (p, vb, n, M, cap, None, 3, 0.0, p, p, p, p, None)))
    sel = lambda **kw: L.tohip_views_select(*[kw.get(k, base[k]) for k in names])
    for k in ("views", "S", "order", "gain", "n_sel"):
        assert sel(**{k: None}) == EINVAL, k
    assert sel(k=0) == EINVAL and sel(k=M + 1) == EINVAL and sel(n=0) == EINVAL and sel(M=0) == EINVAL and sel(cap=0) == EINVAL
    assert sel(min_gain=-1e-9) == EINVAL and sel(min_gain=float("nan")) == EINVAL and sel(min_gain=float("inf")) == EINVAL
    assert sel(bytes=vb - 1) == ENOSPC

    names = ("views", "bytes", "n", "M", "cap", "c", "row", "stream")
    base = dict(zip(names, (p, vb, n, M, cap, 0, p, None)))
    row = lambda **kw: L.tohip_views_row(*[kw.get(k, base[k]) for k in names])
    assert row(views=None) == EINVAL and row(row=None) == EINVAL and row(c=-1) == EINVAL and row(c=M) == EINVAL and row(n=0) == EINVAL
    assert row(bytes=vb - 1) == ENOSPC


def test_check_views_names_what_is_wrong():
    from trajectory_optimization_amd.ops import check_views
    P, Q = torch.zeros(6, 3), torch.ones(6, 4)
    assert check_views(P, Q, 4) == (6, 4, 0.0) and check_views(P, Q, 9, 0.25, 3) == (6, 6, 0.25)   # k is clipped to M
    bad = [
        (dict(cand_poses=[[0, 0, 0]]), "cand_poses must be a floating-point tensor"),
        (dict(cand_poses=torch.zeros(6, 3, dtype=torch.int32)), "cand_poses must be a floating-point tensor"),
        (dict(cand_poses=torch.zeros(6, 2)), r"cand_poses must have shape \(M,3\)"),
        (dict(cand_poses=torch.zeros(0, 3)), r"cand_poses must have shape \(M,3\)"),
        (dict(cand_quats=torch.zeros(6, 3)), r"cand_quats must have shape \(M,4\)"),
        (dict(cand_quats=torch.ones(5, 4)), "6 candidates, cand_quats 5"),
        (dict(cand_poses=torch.full((6, 3), float("nan"))), "cand_poses must be finite"),
        (dict(cand_quats=torch.full((6, 4), float("inf"))), "cand_quats must be finite"),
        (dict(cand_poses=torch.zeros(65537, 3), cand_quats=torch.ones(65537, 4)), "at most 65536"),
        (dict(k=0), "k must be an integer >= 1"), (dict(k=2.0), "k must be an integer >= 1"), (dict(k=True), "k must be an integer >= 1"),
        (dict(min_gain=-0.1), "min_gain must be a finite number >= 0"), (dict(min_gain=float("nan")), "min_gain"),
        (dict(min_gain="x"), "min_gain"), (dict(chunk=0), "chunk must be None or an integer"), (dict(chunk=257), "chunk"),
        (dict(chunk=1.5), "chunk"),
    ]
    for kw, msg in bad:
        args = dict(cand_poses=P, cand_quats=Q, k=4, min_gain=0.0, chunk=None)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            check_views(**args)


class _Shard:
    def __init__(self, kind="waypoints", world_size=1, collective=False):
        self.kind, self.world_size, self.collective = kind, world_size, collective


def _model(shard=None, occlusion=None):
    return types.SimpleNamespace(_cloud=types.SimpleNamespace(n=50), _shard=shard or _Shard(), _cam=None, _rig=None, _flags=0, _prior=None,
                                 _occlusion=occlusion, _occlusion_limits=(1.0, 15.0))


def test_select_views_refusals_come_before_any_gpu_call():
    from trajectory_optimization_amd.tools import select_views
    P, Q = torch.zeros(6, 3), torch.ones(6, 4)
    cam = dict(intrins=torch.eye(3), img_width=64.0, img_height=48.0)
    pts = torch.zeros(50, 3)
    for shard in (_Shard("points"), _Shard("waypoints", 2, True)):
        with pytest.raises(ValueError, match="sharded model"):
            select_views(_model(shard), P, Q, 3)
    with pytest.raises(ValueError, match="ModelTraj brings its own camera"):
        select_views(_model(), P, Q, 3, **cam)
    with pytest.raises(ValueError, match="the model has None"):
        select_views(_model(), P, Q, 3, occlusion="hpr")
    with pytest.raises(ValueError, match="k must be an integer"):
        select_views(_model(), P, Q, 0)
    with pytest.raises(ValueError, match="camera is needed"):
        select_views(pts, P, Q, 3)
    with pytest.raises(ValueError, match="unknown keyword"):
        select_views(pts, P, Q, 3, fov=3, **cam)
    with pytest.raises(ValueError, match="occlusion must be None, 'hpr' or 'zbuffer'"):
        select_views(pts, P, Q, 3, occlusion="raycast", **cam)
    with pytest.raises(ValueError, match=r"points must be an \(N,3\) tensor"):
        select_views(torch.zeros(50, 2), P, Q, 3, **cam)
    with pytest.raises(ValueError, match=r"prior_log_odds must have shape \(50,\)"):
        select_views(pts, P, Q, 3, prior_log_odds=torch.zeros(49), **cam)
    with pytest.raises(ValueError, match="prior_log_odds must be >= 0"):
        select_views(pts, P, Q, 3, prior_log_odds=-torch.ones(50), **cam)
    with pytest.raises(ValueError, match=r"cand_quats must have shape \(M,4\)"):
        select_views(pts, P, P, 3, **cam)
    with pytest.raises(ValueError, match="min_gain"):
        select_views(pts, P, Q, 3, min_gain=-1.0, **cam)
    with pytest.raises(ValueError, match="clamp_max must be a number >= 0"):
        select_views(pts, P, Q, 3, clamp_max=-1.0, **cam)
    with pytest.raises(ValueError, match="chunk"):
        select_views(pts, P, Q, 3, chunk=1000, **cam)


def test_candidate_grid_is_the_documented_recipe():
    from trajectory_optimization_amd import synth
    p, q = synth.candidate_grid(np.linspace(-15, 15, 6), np.linspace(-15, 15, 6), 0.0, 4)
    assert p.shape == (144, 3) and q.shape == (144, 4) and p.dtype == q.dtype == np.float32
    ix, iy, j = 2, 5, 3
    c = (ix * 6 + iy) * 4 + j
    assert np.allclose(p[c], [-15 + 6 * ix, -15 + 6 * iy, 0.0])
    a = 2 * np.pi * j / 4 + 0.1
    assert np.allclose(q[c], synth.quat_mul([np.cos(a / 2), 0, 0, np.sin(a / 2)], synth.Q_OPTICAL), atol=1e-7)
    # the camera's +z axis (the optical axis) points along the heading
    w, x, y, z = q[c].astype(np.float64)
    zaxis = np.array([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)])
    assert np.allclose(zaxis, [np.cos(a), np.sin(a), 0.0], atol=1e-6)
    d = np.load(os.path.join(REPO, "tests", "golden", "views_bundled_144.npz"))
    b = np.load(os.path.join(REPO, "tests", "golden", "bundled.npz"))
    gp, gq = synth.bundled_candidate_grid(b["pts"], b["poses"])
    assert np.array_equal(gp, d["cand_poses"]) and np.array_equal(gq, d["cand_quats"])
    assert float(d["margins"].min()) >= 100.0 * float(d["bound"]) and d["order"].tolist() == [52, 77, 79, 83, 111, 102, 130, 28]
