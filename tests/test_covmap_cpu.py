"""CPU checks of the voxel-keyed log-odds map (no GPU): the eight entry points are declared in the header and in _lib's table with
matching argument counts and without a new ABI version; tohip_covmap_bytes follows the documented layout; each entry refuses bad
arguments before any launch; every argument the host layer does not accept is refused with a ValueError that names what is wrong,
before any GPU call."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from abi_cases import ABI, check_abi_entries

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
ENTRIES = ("tohip_covmap_bytes", "tohip_covmap_init", "tohip_covmap_integrate", "tohip_covmap_lookup", "tohip_covmap_merge",
           "tohip_covmap_rehash", "tohip_covmap_export", "tohip_covmap_read_header")


def test_header_and_table_declare_the_covmap_entries():
    from trajectory_optimization_amd import ops
    header, before = check_abi_entries(ENTRIES)
    assert f"(still {ABI})" in header and "tohip_covmap_integrate" in before
    assert f"#define TOHIP_COVMAP_MAX {ops.COVMAP_MODES['max']}\n" in header
    assert f"#define TOHIP_COVMAP_ADD {ops.COVMAP_MODES['add']}\n" in header
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert '#include "covmap_kernels.hip"' in src


def test_covmap_bytes_is_the_documented_layout():
    """[header 256 B][capacity slots of 16 B]; capacity a power of two in [16, 2^32]."""
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    for cap in (16, 64, 1 << 16, 1 << 21, 1 << 32):
        assert L.tohip_covmap_bytes(cap) == 256 + 16 * cap == ops.covmap_layout(cap)["total"], cap
    lay = ops.covmap_layout(1024)
    assert lay["header"] == 0 and lay["slots"] == 256 and lay["slot_bytes"] == 16
    for bad in (0, -16, 8, 15, 17, 48, 1000, (1 << 32) + 1, 1 << 33):
        assert L.tohip_covmap_bytes(bad) == 0, bad


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)   # a non-null pointer no call may reach: every case below fails its checks first
    q = ctypes.c_void_p(4096)
    cap = 1024
    nb = L.tohip_covmap_bytes(cap)
    org = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan3 = (ctypes.c_float * 3)(0.0, float("nan"), 0.0)

    names = ("map", "bytes", "cap", "origin", "res", "clamp", "stream")
    base = dict(zip(names, (p, nb, cap, org, 0.1, float("inf"), None)))
    init = lambda **kw: L.tohip_covmap_init(*[kw.get(k, base[k]) for k in names])
    assert init(map=None) == EINVAL and init(cap=1000) == EINVAL and init(cap=8) == EINVAL and init(origin=None) == EINVAL
    assert init(res=0.0) == EINVAL and init(res=-0.1) == EINVAL and init(res=float("nan")) == EINVAL and init(res=float("inf")) == EINVAL
    assert init(clamp=-1.0) == EINVAL and init(clamp=float("nan")) == EINVAL and init(origin=nan3) == EINVAL
    assert init(bytes=nb - 1) == ENOSPC

    names = ("map", "bytes", "cap", "points", "row", "n", "mode", "fold", "hdr", "stream")
    base = dict(zip(names, (p, nb, cap, p, p, 100, 0, 1, None, None)))
    integ = lambda **kw: L.tohip_covmap_integrate(*[kw.get(k, base[k]) for k in names])
    assert integ(map=None) == EINVAL and integ(points=None) == EINVAL and integ(row=None) == EINVAL and integ(n=-1) == EINVAL
    assert integ(mode=2) == EINVAL and integ(mode=-1) == EINVAL and integ(cap=cap + 1) == EINVAL and integ(bytes=nb - 1) == ENOSPC

    names = ("map", "bytes", "cap", "points", "n", "out", "stream")
    base = dict(zip(names, (p, nb, cap, p, 100, p, None)))
    look = lambda **kw: L.tohip_covmap_lookup(*[kw.get(k, base[k]) for k in names])
    assert look(map=None) == EINVAL and look(points=None) == EINVAL and look(out=None) == EINVAL and look(n=-1) == EINVAL
    assert look(cap=0) == EINVAL and look(bytes=nb - 1) == ENOSPC

    names = ("map", "bytes", "cap", "other", "obytes", "ocap", "mode", "hdr", "stream")
    base = dict(zip(names, (p, nb, cap, q, nb, cap, 1, None, None)))
    merge = lambda **kw: L.tohip_covmap_merge(*[kw.get(k, base[k]) for k in names])
    assert merge(map=None) == EINVAL and merge(other=None) == EINVAL and merge(other=p) == EINVAL and merge(mode=7) == EINVAL
    assert merge(ocap=100) == EINVAL and merge(bytes=nb - 1) == ENOSPC and merge(obytes=nb - 1) == ENOSPC
    names = ("map", "bytes", "cap", "other", "obytes", "ocap", "hdr", "stream")
    base = dict(zip(names, (p, nb, cap, q, nb, cap, None, None)))
    rehash = lambda **kw: L.tohip_covmap_rehash(*[kw.get(k, base[k]) for k in names])
    assert rehash(map=None) == EINVAL and rehash(other=None) == EINVAL and rehash(other=p) == EINVAL and rehash(obytes=0) == ENOSPC

    names = ("map", "bytes", "cap", "out_cap", "keys", "values", "centres", "stream")
    base = dict(zip(names, (p, nb, cap, 10, p, p, p, None)))
    exp = lambda **kw: L.tohip_covmap_export(*[kw.get(k, base[k]) for k in names])
    assert exp(map=None) == EINVAL and exp(out_cap=-1) == EINVAL and exp(bytes=nb - 1) == ENOSPC
    for k in ("keys", "values", "centres"):
        assert exp(**{k: None}) == EINVAL, k

    w = (ctypes.c_int64 * 8)()
    assert L.tohip_covmap_read_header(None, w, None, None) == EINVAL and L.tohip_covmap_read_header(p, None, None, None) == EINVAL


def test_check_covmap_names_what_is_wrong():
    from trajectory_optimization_amd.ops import check_covmap, check_covmap_mode
    o, r, c, cap = check_covmap((1.0, -2.0, 0.5), 0.1, 3.5, 1000)
    assert o.dtype == np.float32 and o.tolist() == [1.0, -2.0, 0.5] and r == float(np.float32(0.1)) and c == 3.5 and cap == 1024
    assert check_covmap(torch.zeros(3), 0.25)[2:] == (float("inf"), None) and check_covmap((0, 0, 0), 1, None, 1)[3] == 16
    bad = [
        (dict(resolution=0.0), "resolution must be a finite number > 0"), (dict(resolution=-0.1), "resolution must be"),
        (dict(resolution=float("nan")), "resolution must be"), (dict(resolution=float("inf")), "resolution must be"),
        (dict(resolution="x"), "resolution must be"), (dict(resolution=1e-60), "resolution must be"),
        (dict(origin=(0.0, 0.0)), "origin must be 3 finite numbers"), (dict(origin=(0.0, float("nan"), 0.0)), "origin must be"),
        (dict(origin="abc"), "origin must be"),
        (dict(clamp_max=-1.0), "clamp_max must be a number >= 0"), (dict(clamp_max=float("nan")), "clamp_max must be"),
        (dict(clamp_max="high"), "clamp_max must be"), (dict(clamp_max=[1.0, 2.0]), "clamp_max must be"),
        (dict(capacity=0), "capacity must be None or an integer"), (dict(capacity=2.5), "capacity must be"),
        (dict(capacity=True), "capacity must be"), (dict(capacity=(1 << 32) + 1), "capacity must be"),
    ]
    for kw, msg in bad:
        args = dict(origin=(0.0, 0.0, 0.0), resolution=0.1, clamp_max=None, capacity=None)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            check_covmap(**args)
    assert check_covmap_mode("max") == 0 and check_covmap_mode("add") == 1
    with pytest.raises(ValueError, match="mode must be 'max' or 'add'"):
        check_covmap_mode("sum")


def test_coverage_map_refuses_its_settings_before_any_gpu_call():
    from trajectory_optimization_amd import ops, tools
    with pytest.raises(ValueError, match="resolution must be a finite number > 0"):
        ops.CoverageMap((0.0, 0.0, 0.0), 0.0)
    with pytest.raises(ValueError, match="resolution must be a finite number > 0"):
        tools.coverage_map(resolution=-1.0)
    with pytest.raises(ValueError, match="clamp_max must be a number >= 0"):
        tools.coverage_map(clamp_max=-3.5)
    with pytest.raises(RuntimeError, match="lives on a HIP device"):
        ops.CoverageMap((0.0, 0.0, 0.0), 0.1, device="cpu")
    import inspect
    assert inspect.signature(tools.coverage_map).parameters["resolution"].default == 0.1   # the reference's VoxelGrid leaf
    from trajectory_optimization_amd.pointcloud_utils import voxel_grid_filter
    assert inspect.signature(voxel_grid_filter).parameters["leaf_size"].default == 0.1


class _Shard:
    def __init__(self, kind="waypoints", world_size=1, collective=False):
        self.kind, self.world_size, self.collective = kind, world_size, collective


def test_rows_and_points_are_checked_before_any_gpu_call():
    from trajectory_optimization_amd.ops import check_covmap_rows, covmap_points
    cpu = torch.device("cpu")
    pts, row = torch.zeros(50, 3), torch.ones(50)
    p, r = check_covmap_rows(pts.double(), row.double(), cpu)
    assert p.dtype == r.dtype == torch.float32 and p.shape == (50, 3) and r.shape == (50,)
    with pytest.raises(ValueError, match=r"^log_odds must have shape \(50,\)"):
        check_covmap_rows(pts, torch.ones(49), cpu)
    with pytest.raises(ValueError, match=r"^log_odds must have shape \(50,\)"):
        check_covmap_rows(pts, torch.ones(50, 1), cpu)
    with pytest.raises(ValueError, match="^log_odds must be >= 0"):
        check_covmap_rows(pts, -row, cpu)
    nan_row = row.clone()
    nan_row[7] = float("nan")
    with pytest.raises(ValueError, match="^log_odds must be finite"):
        check_covmap_rows(pts, nan_row, cpu)
    with pytest.raises(ValueError, match="^log_odds must be finite"):
        check_covmap_rows(pts, row * float("inf"), cpu)
    with pytest.raises(ValueError, match="^log_odds must be a floating-point tensor"):
        check_covmap_rows(pts, torch.ones(50, dtype=torch.int64), cpu)
    for bad in (torch.zeros(50, 2), torch.zeros(50), torch.zeros(50, 3, dtype=torch.int32), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match=r"points must be an \(N,3\) floating-point tensor"):
            covmap_points(bad, cpu)
    # a wrong device: the points on the host, the map on a HIP device (and the row likewise)
    with pytest.raises(ValueError, match="the points live on cpu, the map on cuda:0"):
        covmap_points(pts, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="the points live on cpu, the map on cuda:0"):
        check_covmap_rows(pts, row, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="^log_odds lives on cpu, the map on meta"):   # (the row alone on another device)
        check_covmap_rows(pts.to("meta"), row, torch.device("meta"))
    # a sharded model is refused by name; an unsharded one hands over its cloud's points
    for shard in (_Shard("points"), _Shard("waypoints", 2, True)):
        with pytest.raises(ValueError, match="sharded model"):
            covmap_points(types.SimpleNamespace(_cloud=types.SimpleNamespace(points=pts), _shard=shard), cpu)
    with pytest.raises(ValueError, match=r"points must be an \(N,3\)"):   # (a stand-in cloud is no PackedCloud)
        covmap_points(types.SimpleNamespace(_cloud=types.SimpleNamespace(points=pts), _shard=_Shard()), cpu)


def test_commit_coverage_refuses_a_sharded_model():
    from trajectory_optimization_amd.model import ModelTraj, TeamTraj
    for shard in (_Shard("points"), _Shard("waypoints", 2, True)):
        with pytest.raises(ValueError, match="sharded model"):
            ModelTraj.commit_coverage(types.SimpleNamespace(_shard=shard), object())
    assert callable(TeamTraj.commit_coverage)


def test_merge_refuses_maps_that_do_not_match():
    from trajectory_optimization_amd.ops import check_covmap_merge
    mk = lambda o=(0.0, 0.0, 0.0), r=0.1, d="cuda:0": types.SimpleNamespace(origin=np.asarray(o, np.float32), resolution=r, device=torch.device(d))
    check_covmap_merge(mk(), mk())
    a = mk()
    with pytest.raises(ValueError, match="cannot be merged into itself"):
        check_covmap_merge(a, a)
    with pytest.raises(ValueError, match="the maps' origins differ"):
        check_covmap_merge(mk(), mk(o=(0.0, 0.05, 0.0)))
    with pytest.raises(ValueError, match="the maps' resolutions differ"):
        check_covmap_merge(mk(), mk(r=0.2))
    with pytest.raises(ValueError, match="the maps live on"):
        check_covmap_merge(mk(), mk(d="cuda:1"))


def test_a_tensor_prior_takes_todays_path():
    from trajectory_optimization_amd.ops import resolve_prior
    t = torch.ones(5)
    assert resolve_prior(t, None) is t and resolve_prior(None, None) is None
