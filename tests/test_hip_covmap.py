"""The voxel-keyed log-odds map on the device (covmap_kernels.hip) against a plain numpy / dict restatement of its
definition, kept in this file:

  key of a point     per axis i = floor((x - origin) / r) in float32; the indices + 2^20 packed 21 bits each (x highest); a non-finite
                     coordinate or an index outside [-2^20, 2^20) skips the point
  integrate          the observation of a voxel = the maximum over the call's points in it; 'max': min(max(old, obs), clamp),
                     'add': min(old + obs, clamp) — one f32 operation per voxel and call; unseen voxels start from 0
  lookup             the voxel's value, 0.0 for an unknown voxel and for a skipped point
  merge              every voxel of the other map as one observation
  export             centres origin + (i + 1/2) r, values, keys, in ascending key order

Every comparison is exact (torch.equal / array_equal): nothing here has a tolerance."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
BIAS = 1 << 20
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bundled():
    d = np.load(os.path.join(GOLDEN, "bundled.npz"))
    return np.ascontiguousarray(d["pts"], dtype=F32), np.ascontiguousarray(d["poses"], dtype=F32)


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def np_keys(pts, origin, r):
    """-> (keys int64, -1 for a skipped point; ok bool)."""
    pts, o, r = np.asarray(pts, dtype=F32), np.asarray(origin, dtype=F32), F32(r)
    with np.errstate(all="ignore"):
        f = np.floor((pts - o) / r)
    assert f.dtype == F32
    ok = ((f >= -BIAS) & (f < BIAS)).all(axis=1)   # (False for NaN)
    i = np.where(ok[:, None], f, 0).astype(np.int64) + BIAS
    return np.where(ok, (i[:, 0] << 42) | (i[:, 1] << 21) | i[:, 2], -1), ok


class RefMap:
    def __init__(self, origin=(0.0, 0.0, 0.0), r=0.1, clamp=None):
        self.o, self.r = np.asarray(origin, dtype=F32), F32(r)
        self.clamp = F32(np.inf if clamp is None else clamp)
        self.d = {}
        self.skipped = 0

    def _fold(self, keys, obs, mode):
        for k, v in zip(keys.tolist(), obs):
            old = self.d.get(k, F32(0))
            new = max(old, v) if mode == "max" else F32(old + v)
            self.d[k] = F32(min(new, self.clamp))

    def integrate(self, pts, row, mode):
        keys, ok = np_keys(pts, self.o, self.r)
        self.skipped += int((~ok).sum())
        uk, inv = np.unique(keys[ok], return_inverse=True)
        obs = np.zeros(len(uk), dtype=F32)
        np.maximum.at(obs, inv.ravel(), np.asarray(row, dtype=F32)[ok])
        self._fold(uk, obs, mode)

    def merge(self, other, mode):
        ks = sorted(other.d)
        self._fold(np.asarray(ks, dtype=np.int64), [other.d[k] for k in ks], mode)

    def lookup(self, pts):
        keys, _ = np_keys(pts, self.o, self.r)
        return np.asarray([self.d.get(k, F32(0)) for k in keys.tolist()], dtype=F32)

    def export(self):
        keys = np.asarray(sorted(self.d), dtype=np.int64)
        vals = np.asarray([self.d[k] for k in keys.tolist()], dtype=F32)
        idx = np.stack([keys >> 42, (keys >> 21) & 0x1fffff, keys & 0x1fffff], axis=1) - BIAS
        centres = self.o + (idx.astype(F32) + F32(0.5)) * self.r
        assert centres.dtype == F32
        return centres.reshape(-1, 3), vals, keys


def _assert_same_map(cmap, ref):
    c, v, k = cmap.export()
    rc, rv, rk = ref.export()
    assert cmap.n_voxels == len(rk) == len(ref.d)
    assert np.array_equal(k.cpu().numpy(), rk), "keys"
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32)), "values"
    assert np.array_equal(c.cpu().numpy().view(np.uint32), rc.view(np.uint32)), "centres"
    assert k.dtype == torch.int64 and v.dtype == torch.float32 and c.dtype == torch.float32 and c.shape == (len(rk), 3)


def _same_export(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.export(), b.export())) and a.n_voxels == b.n_voxels


def _row(n, seed, top=5.0):
    rng = np.random.default_rng(seed)
    row = (rng.random(n) * top).astype(F32)
    row[rng.random(n) < 0.2] = 0.0
    return row


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1. keys -------------------------------------------------------------------------------------------------------------------

def _hand_made(o, r):
    """(points, number skipped): negative coordinates, points exactly on voxel faces, the index limits and what lies beyond them."""
    o = np.asarray(o, dtype=F32)
    rows = [o + F32(r) * F32(k) for k in range(-8, 9)]                          # on the faces, all three axes at once
    rows += [o + np.asarray([F32(r) * F32(k), 0, 0], dtype=F32) for k in (-3, -2, -1, 1, 2, 3)]
    rows += [np.asarray(p, dtype=F32) for p in ((-0.01, -0.01, -0.01), (-7.3, -11.9, -2.2), (0.0, 0.0, 0.0), (-0.0, 1e-30, -1e-30))]
    top, bottom = o + F32(r) * F32(BIAS - 1), o - F32(r) * F32(BIAS)           # indices 2^20 - 1 and -2^20: the last ones kept
    rows += [top, bottom, np.asarray([top[0], o[1], bottom[2]], dtype=F32)]
    beyond = [o + F32(r) * F32(BIAS), o - F32(r) * F32(BIAS + 1), np.asarray([o[0], 3e38, o[2]], dtype=F32),
              np.asarray([-3e38, o[1], o[2]], dtype=F32)]
    bad = [np.asarray(p, dtype=F32) for p in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (np.nan, np.nan, np.nan))]
    pts = np.stack(rows + beyond + bad).astype(F32)
    return pts, len(beyond) + len(bad)


@pytest.mark.parametrize("case", ["synth100k", "bundled", "bundled_offset", "hand"])
def test_keys_are_numpy_float32_keys(dev, case):
    from trajectory_optimization_amd import ops
    o, r, n_skip = (0.0, 0.0, 0.0), 0.1, 0
    if case == "synth100k":
        pts = synth.make_cloud(100_000, 0)
    elif case == "bundled":
        pts = _bundled()[0]
    elif case == "bundled_offset":
        pts, o, r = _bundled()[0], (0.3, -1.7, 0.05), 0.07
    else:
        o, r = (1.0, -2.0, 0.5), 0.25
        pts, n_skip = _hand_made(o, r)
        # the index limits: rows 27 and 28 are the highest and the lowest voxel a map can hold (the values are representable)
        assert float(pts[27][0]) == 1.0 + 0.25 * (BIAS - 1) and float(pts[28][2]) == 0.5 - 0.25 * BIAS
        assert np_keys(pts, o, r)[0][27:29].tolist() == [(1 << 63) - 1, 0]
    keys, ok = np_keys(pts, o, r)
    assert int((~ok).sum()) == n_skip
    cmap = ops.CoverageMap(o, r, device=dev)
    cmap.integrate(_t(pts, dev), torch.ones(len(pts), device=dev))
    want = np.unique(keys[ok])
    c, v, k = cmap.export()
    assert np.array_equal(k.cpu().numpy(), want) and cmap.n_voxels == len(want)
    assert cmap.skipped == (n_skip, 0)
    assert bool((v == 1.0).all())
    words, geom = cmap.header()
    assert words[0] == len(want) and words[1] == cmap.capacity and words[2] == 0 and words[3] == len(want) and words[4] == n_skip
    assert geom[:4] == [float(F32(x)) for x in (*o, r)] and geom[4] == float("inf")
    # every point reads its own voxel back; a skipped one reads 0
    got = cmap.lookup(_t(pts, dev)).cpu().numpy()
    assert np.array_equal(got, ok.astype(F32))
    ref = RefMap(o, r)
    ref.integrate(pts, np.ones(len(pts), dtype=F32), "max")
    _assert_same_map(cmap, ref)


def test_c_call_skips_and_counts_invalid_rows(dev):
    """At the C level a negative or non-finite log-odds entry is skipped and counted; through Python it never gets that far."""
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    pts = synth.make_cloud(5_000, 2)
    row = _row(len(pts), 3)
    bad = {10: -1.0, 11: np.nan, 12: np.inf, 13: -np.inf, 4000: -1e-30}
    for i, v in bad.items():
        row[i] = v
    pts[12] = np.nan   # (a row skipped on both counts is counted in both)
    good = np.ones(len(pts), dtype=bool)
    good[list(bad)] = False
    cmap = ops.CoverageMap(resolution=0.5, device=dev)
    h = (ctypes.c_int64 * 8)()
    P, R = _t(pts, dev), _t(row, dev)
    rc = L.tohip_covmap_integrate(*cmap._sizes(), _lib.ptr(P), _lib.ptr(R), len(pts), 0, 1, h, _lib.stream_ptr())
    assert rc == 0 and h[2] == 0 and h[4] == 1 and h[5] == len(bad)
    cmap.n_voxels = int(h[0])
    ref = RefMap(r=0.5)
    ref.integrate(pts[good], row[good], "max")
    _assert_same_map(cmap, ref)
    with pytest.raises(ValueError, match="^log_odds must be"):
        cmap.integrate(P, R)


# ---- 2. integrate, lookup, export ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["max", "add"])
@pytest.mark.parametrize("clamp", [None, 3.5])
def test_integrate_lookup_export_match_the_restatement(dev, mode, clamp):
    from trajectory_optimization_amd import ops
    A = synth.make_cloud(100_000, 0)                       # r = 0.5: several points per voxel
    B = synth.make_cloud(80_000, 1) + F32(3.0)             # another cloud that overlaps it
    rowA, rowB = _row(len(A), 10), _row(len(B), 11)
    far = synth.make_cloud(1_000, 4) + F32(500.0)          # voxels nobody has seen
    cmap, ref = ops.CoverageMap((0.0, 0.0, 0.0), 0.5, clamp_max=clamp, device=dev), RefMap(r=0.5, clamp=clamp)
    cmap.integrate(_t(A, dev), _t(rowA, dev), mode)
    ref.integrate(A, rowA, mode)
    assert len(ref.d) < len(A) // 2
    _assert_same_map(cmap, ref)
    cmap.integrate(_t(B, dev), _t(rowB, dev), mode)
    ref.integrate(B, rowB, mode)
    _assert_same_map(cmap, ref)
    for pts in (A, B, far, np.concatenate([B[::7], far, A[::5]])):
        assert np.array_equal(_bits(cmap.lookup(_t(pts, dev))), ref.lookup(pts).view(np.uint32))
    assert float(cmap.lookup(_t(far, dev)).abs().max()) == 0.0
    if clamp is not None:
        assert float(cmap.export()[1].max()) == clamp
    # a third pass over A: 'max' changes nothing (idempotent), 'add' adds once more per voxel
    before = [x.clone() for x in cmap.export()]
    cmap.integrate(_t(A, dev), _t(rowA, dev), mode)
    ref.integrate(A, rowA, mode)
    _assert_same_map(cmap, ref)
    if mode == "max":
        assert all(torch.equal(x, y) for x, y in zip(before, cmap.export()))
    assert cmap.skipped == (0, 0)


def test_a_zero_observation_still_creates_its_voxel(dev):
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(3_000, 5)
    cmap = ops.CoverageMap(resolution=0.1, device=dev).integrate(_t(pts, dev), torch.zeros(len(pts), device=dev), "add")
    assert cmap.n_voxels == len(np.unique(np_keys(pts, (0, 0, 0), 0.1)[0])) and float(cmap.export()[1].abs().max()) == 0.0


def test_packed_cloud_and_model_are_their_caller_order_points(dev):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelTraj
    pts = synth.make_cloud(20_000, 6)
    row = _t(_row(len(pts), 7), dev)
    poses, quats = synth.make_path(5, optical=True, jitter_seed=1)
    cloud = ops.PackedCloud(_t(pts, dev))
    model = ModelTraj(cloud, torch.from_numpy(poses), torch.from_numpy(quats), torch.from_numpy(K), IW, IH, device=dev)
    maps = [ops.CoverageMap(resolution=0.2, device=dev).integrate(x, row) for x in (_t(pts, dev), cloud, model)]
    assert _same_export(maps[0], maps[1]) and _same_export(maps[0], maps[2])
    assert torch.equal(maps[0].lookup(cloud), maps[0].lookup(_t(pts, dev))) and torch.equal(maps[0].lookup(model), maps[0].lookup(cloud))


# ---- 3. order and run independence ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["max", "add"])
def test_rows_permuted_runs_repeated_and_folding_give_one_map(dev, mode):
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(200_000, 8)
    row = _row(len(pts), 9)
    order = np.argsort(np_keys(pts, (0, 0, 0), 0.5)[0], kind="stable")   # sorted by voxel: the longest runs of equal keys a wave can meet
    perms = [np.arange(len(pts)), np.random.default_rng(0).permutation(len(pts)), order, order[::-1].copy()]
    probe = _t(np.concatenate([pts[::3], pts[:100] + F32(900.0)]), dev)
    maps = []
    for fold in (True, False):
        for p in perms + perms[:1]:   # (the first order once more: the same call in a fresh map twice)
            m = ops.CoverageMap(resolution=0.5, clamp_max=4.0, device=dev)
            m.fold = fold
            m.integrate(_t(pts[p], dev), _t(row[p], dev), mode)
            q = p[p % 2 == 0]   # (the even rows, in this order's sequence: the same set for every order)
            m.integrate(_t(pts[q] + F32(0.25), dev), _t(row[q], dev), mode)
            maps.append(m)
    first, look = maps[0], maps[0].lookup(probe)
    for m in maps[1:]:
        assert _same_export(first, m) and torch.equal(look, m.lookup(probe))
    ref = RefMap(r=0.5, clamp=4.0)
    ref.integrate(pts, row, mode)
    ref.integrate(pts[::2] + F32(0.25), row[::2], mode)
    _assert_same_map(first, ref)


# ---- 4. round trip ---------------------------------------------------------------------------------------------------------------

def _one_point_per_voxel(pts, o=(0.0, 0.0, 0.0), r=0.1):
    keys, ok = np_keys(pts, o, r)
    assert ok.all()
    _, first = np.unique(keys, return_index=True)
    return np.sort(first)


def _model(dev, pts, poses, quats, **kw):
    from trajectory_optimization_amd.model import ModelTraj
    return ModelTraj(torch.from_numpy(pts), torch.from_numpy(poses), torch.from_numpy(quats), torch.from_numpy(K), IW, IH, device=dev, **kw)


def test_round_trip_row_plan_and_view_selection(dev):
    from trajectory_optimization_amd import ops, tools
    full = synth.make_cloud(90_000, seed=41)
    pts = np.ascontiguousarray(full[_one_point_per_voxel(full)])
    assert 30_000 < len(pts) < len(full)
    row = _row(len(pts), 12, top=3.0)
    cmap = ops.CoverageMap(resolution=0.1, device=dev).integrate(_t(pts, dev), _t(row, dev))
    assert cmap.n_voxels == len(pts)
    assert np.array_equal(_bits(cmap.lookup(_t(pts, dev))), row.view(np.uint32))
    # a plan with the map as its prior is the plan with the row as its prior
    poses, quats = synth.make_path(17, optical=True, jitter_seed=41)
    a, b = _model(dev, pts, poses, quats, prior_log_odds=_t(row, dev)), _model(dev, pts, poses, quats, prior_log_odds=cmap)
    assert torch.equal(a.prior_log_odds, b.prior_log_odds)
    la, lb = a(vis_wps_dist=0.0), b(vis_wps_dist=0.0)
    la.backward()
    lb.backward()
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(a.rewards, b.rewards)
    for k in ("vis", "l2", "length", "smooth"):
        assert float(a.loss[k].detach()) == float(b.loss[k].detach()), k
    assert torch.equal(a.poses.grad, b.poses.grad) and torch.equal(a.quats.grad, b.quats.grad)
    assert float(a.poses.grad.abs().max()) > 0
    # the setter takes a map as well
    a.prior_log_odds = cmap
    assert torch.equal(a.prior_log_odds, _t(row, dev))
    # view selection: with a model, with points and with a packed cloud
    cp, cq = synth.candidate_grid(np.linspace(-15, 15, 4), np.linspace(-15, 15, 4), 0.0, 4)
    cp, cq = _t(cp, dev), _t(cq, dev)
    plain = _model(dev, pts, poses, quats)
    cam = dict(intrins=torch.from_numpy(K), img_width=IW, img_height=IH)
    want = tools.select_views(plain, cp, cq, 6, prior_log_odds=_t(row, dev))
    assert want.n_selected >= 1
    for first, kw in ((plain, {}), (_t(pts, dev), cam), (plain._cloud, cam)):
        got = tools.select_views(first, cp, cq, 6, prior_log_odds=cmap, **kw)
        assert torch.equal(got.order, want.order) and torch.equal(got.gain_fixed, want.gain_fixed)
        assert torch.equal(got.coverage_log_odds, want.coverage_log_odds)


# ---- 5. across clouds ------------------------------------------------------------------------------------------------------------

def test_coverage_crosses_from_one_cloud_to_another(dev):
    from trajectory_optimization_amd import ops, tools
    from trajectory_optimization_amd.model import TeamTraj
    allp, path = _bundled()
    rng = np.random.default_rng(5)
    ia = rng.permutation(np.flatnonzero(np.linalg.norm(allp - path[0], axis=1) < 12.0))
    ib = rng.permutation(np.flatnonzero(np.linalg.norm(allp - path[20], axis=1) < 12.0))
    A, B = np.ascontiguousarray(allp[ia]), np.ascontiguousarray(allp[ib])
    shared = len(np.intersect1d(ia, ib))
    assert 1000 < shared < min(len(A), len(B)) and len(A) != len(B)
    ident = np.tile(np.asarray([1, 0, 0, 0], dtype=F32), (12, 1))
    cmap = tools.coverage_map(clamp_max=3.5, device=dev)
    ma = _model(dev, A, path[:12].copy(), ident)
    ma(vis_wps_dist=0.0)
    cov = ma.coverage_log_odds(upto=8, clamp_max=3.5, vis_wps_dist=0.0)
    assert ma.commit_coverage(cmap, upto=8, vis_wps_dist=0.0) is cmap
    assert float(cov.max()) > 0
    ref = RefMap(r=0.1, clamp=3.5)
    ref.integrate(A, cov.cpu().numpy(), "max")
    _assert_same_map(cmap, ref)
    # commit_coverage is integrate(model, coverage_log_odds(...), 'max')
    twin = tools.coverage_map(clamp_max=3.5, device=dev).integrate(ma, cov, mode="max")
    assert _same_export(cmap, twin)
    # B reads its prior from the map: the restatement's lookup, and the existing prior path given that tensor
    mb = _model(dev, B, path[8:20].copy(), ident, prior_log_odds=cmap)
    want = ref.lookup(B)
    assert np.array_equal(_bits(mb.prior_log_odds), want.view(np.uint32))
    assert 0 < int((want > 0).sum()) < len(B)
    mt = _model(dev, B, path[8:20].copy(), ident, prior_log_odds=_t(want, dev))
    lb, lt = mb(vis_wps_dist=0.0), mt(vis_wps_dist=0.0)
    assert torch.equal(mb.rewards, mt.rewards) and torch.equal(lb.detach(), lt.detach())
    # committing B's plan: its row holds the prior read from the map, so no voxel loses anything
    before = cmap.lookup(_t(allp, dev))
    mb.commit_coverage(cmap, vis_wps_dist=0.0)
    ref.integrate(B, mb.coverage_log_odds(clamp_max=3.5, vis_wps_dist=0.0).cpu().numpy(), "max")
    _assert_same_map(cmap, ref)
    assert bool((cmap.lookup(_t(allp, dev)) >= before).all())
    # a team commits its one shared row the same way
    m1, m2 = _model(dev, A, path[:6].copy(), ident[:6]), None
    m2 = type(m1).sharing_cloud_of(m1, torch.from_numpy(path[6:12].copy()), torch.from_numpy(ident[:6]))
    team = TeamTraj([m1, m2])
    tmap = tools.coverage_map(clamp_max=3.5, device=dev)
    team.commit_coverage(tmap, vis_wps_dist=0.0)
    tref = RefMap(r=0.1, clamp=3.5)
    tref.integrate(A, team.coverage_log_odds(clamp_max=3.5, vis_wps_dist=0.0).cpu().numpy(), "max")
    _assert_same_map(tmap, tref)


# ---- 6. growth -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_new", [25, 60_000])
def test_a_call_that_does_not_fit_writes_nothing_and_the_public_call_grows(dev, n_new):
    """n_new = 25: 13 + 25 voxels fit the 64 slots but not half of them — the needed count is exact.  60 000: the table fills up
    while the call runs — a probe gives up, the count is a lower bound."""
    from trajectory_optimization_amd import _lib, ops
    L = _lib.lib()
    grid = lambda n, x0: np.stack([x0 + 0.05 + 0.1 * np.arange(n), np.full(n, 0.05), np.full(n, 0.05)], axis=1).astype(F32)
    first, more = grid(13, 0.0), grid(n_new, 100.0)
    assert len(np.unique(np_keys(np.concatenate([first, more]), (0, 0, 0), 0.1)[0])) == 13 + n_new
    r1, r2 = _row(13, 1) + F32(0.5), _row(n_new, 2)
    small = ops.CoverageMap(resolution=0.1, capacity=64, device=dev).integrate(_t(first, dev), _t(r1, dev))
    assert small.capacity == 64 and small.n_voxels == 13
    before = [x.clone() for x in small.export()]
    look = small.lookup(_t(first, dev)).clone()
    h = (ctypes.c_int64 * 8)()
    P, R = _t(more, dev), _t(r2, dev)
    for fold in (1, 0):
        rc = L.tohip_covmap_integrate(*small._sizes(), _lib.ptr(P), _lib.ptr(R), n_new, 0, fold, h, _lib.stream_ptr())
        assert rc == _lib.ENOSPC and h[0] == 13 and h[1] == 64
        if n_new == 25:
            assert h[2] == 1 and h[3] == 38
        else:
            assert h[2] & 2 and 13 < h[3] <= 13 + n_new
        assert all(torch.equal(x, y) for x, y in zip(before, small.export()))
        assert torch.equal(look, small.lookup(_t(first, dev))) and float(small.lookup(P).abs().max()) == 0.0
    # a merge that does not fit: the same rule
    other = ops.CoverageMap(resolution=0.1, device=dev).integrate(P, R)
    rc = L.tohip_covmap_merge(*small._sizes(), *other._sizes(), 1, h, _lib.stream_ptr())
    assert rc == _lib.ENOSPC and h[0] == 13 and all(torch.equal(x, y) for x, y in zip(before, small.export()))
    # the public calls grow, and end with the contents of a map that was large from the start
    large = ops.CoverageMap(resolution=0.1, capacity=1 << 18, device=dev).integrate(_t(first, dev), _t(r1, dev)).integrate(P, R)
    small.integrate(P, R)
    assert small.capacity >= 2 * (13 + n_new) and small.capacity < large.capacity and small.n_voxels == 13 + n_new
    assert _same_export(small, large)
    ref = RefMap(r=0.1)
    ref.integrate(first, r1, "max")
    ref.integrate(more, r2, "max")
    _assert_same_map(small, ref)
    tiny = ops.CoverageMap(resolution=0.1, capacity=16, device=dev).integrate(_t(first, dev), _t(r1, dev)).merge(other, "max")
    assert _same_export(tiny, large)
    assert small.header()[0][2] == 0


# ---- 7. merge --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clamp", [None, 3.5])
def test_merge_matches_the_restatement(dev, clamp):
    from trajectory_optimization_amd import ops
    A, B = synth.make_cloud(60_000, 20), synth.make_cloud(50_000, 21) + F32(2.0)
    rowA, rowB = _row(len(A), 22), _row(len(B), 23)
    mk = lambda: ops.CoverageMap(resolution=0.25, clamp_max=clamp, device=dev)
    a = lambda: mk().integrate(_t(A, dev), _t(rowA, dev), "add")
    b = lambda: mk().integrate(_t(B, dev), _t(rowB, dev), "add")

    def refs():
        ra, rb = RefMap(r=0.25, clamp=clamp), RefMap(r=0.25, clamp=clamp)
        ra.integrate(A, rowA, "add")
        rb.integrate(B, rowB, "add")
        return ra, rb
    for mode in ("add", "max"):
        m = a().merge(b(), mode)
        ra, rb = refs()
        ra.merge(rb, mode)
        _assert_same_map(m, ra)
        assert len(ra.d) > max(len(rb.d), len(refs()[0].d))   # (they overlap in part only)
    assert _same_export(a().merge(b(), "add"), b().merge(a(), "add"))   # 'add' commutes
    for mode in ("add", "max"):                                          # an empty map changes nothing
        assert _same_export(a().merge(mk(), mode), a()) and _same_export(mk().merge(a(), mode), a())
    # what does not match is refused by name
    with pytest.raises(ValueError, match="resolutions differ"):
        a().merge(ops.CoverageMap(resolution=0.5, device=dev))
    with pytest.raises(ValueError, match="origins differ"):
        a().merge(ops.CoverageMap((0.1, 0.0, 0.0), 0.25, device=dev))
    m = a()
    with pytest.raises(ValueError, match="itself"):
        m.merge(m)


def test_exported_centres_and_values_rebuild_the_map(dev):
    """How a map travels as plain arrays: integrate(export's centres, values) into an empty map of the same geometry gives the map
    back — where the origin is small against the coordinates' own rounding, as here (origin 0, and an offset one of a few metres)."""
    from trajectory_optimization_amd import ops
    pts = _bundled()[0]
    row = _row(len(pts), 40, top=3.0)
    for o, r in (((0.0, 0.0, 0.0), 0.1), ((0.3, -1.7, 0.05), 0.07)):
        a = ops.CoverageMap(o, r, clamp_max=3.5, device=dev).integrate(_t(pts, dev), _t(row, dev), "add")
        centres, values, keys = a.export()
        assert np.array_equal(np_keys(centres.cpu().numpy(), o, r)[0], keys.cpu().numpy())
        b = ops.CoverageMap(o, r, clamp_max=3.5, device=dev).integrate(centres, values, "add")
        assert _same_export(a, b) and b.skipped == (0, 0)


# ---- 8. the example --------------------------------------------------------------------------------------------------------------

def test_changing_map_example_runs(dev, capsys):
    spec = importlib.util.spec_from_file_location("changing_map_sample", os.path.join(REPO, "examples", "changing_map_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--plans", "4", "--opt-steps", "15"])
    committed, voxels, npts = out["committed_mean_reward"], out["n_voxels"], out["n_points"]
    assert len(committed) == 4 and len(set(npts)) > 1                       # the cloud changed from plan to plan
    assert all(b >= a for a, b in zip(committed, committed[1:])) and committed[-1] > committed[0] > 0.5
    assert all(b >= a for a, b in zip(voxels, voxels[1:])) and voxels[0] > 0
    text = capsys.readouterr().out
    lines = text.strip().split("\n")
    assert len(lines) == 4 and all(ln.startswith(f"plan {i}:") and "voxels" in ln and "points seen" in ln for i, ln in enumerate(lines))


# ---- 9. size ---------------------------------------------------------------------------------------------------------------------

def test_one_million_points(dev):
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(1_000_000, 0)
    row = _row(len(pts), 30)
    cmap = ops.CoverageMap(resolution=0.1, clamp_max=3.5, device=dev).integrate(_t(pts, dev), _t(row, dev), "add")
    ref = RefMap(r=0.1, clamp=3.5)
    ref.integrate(pts, row, "add")
    _assert_same_map(cmap, ref)
    probe = np.concatenate([pts[::2], pts[:1000] + F32(0.31)])
    assert np.array_equal(_bits(cmap.lookup(_t(probe, dev))), ref.lookup(probe).view(np.uint32))


def _np_sorted_map(pts, row, r):
    """The restatement of ONE integrate into an empty map, vectorised for sizes a dict is too slow for: sorted keys and their values."""
    keys, ok = np_keys(pts, (0.0, 0.0, 0.0), r)
    assert ok.all()
    uk, inv = np.unique(keys, return_inverse=True)
    obs = np.zeros(len(uk), dtype=F32)
    np.maximum.at(obs, inv.ravel(), row)
    return uk, obs, keys


def test_sixteen_million_points(dev):
    """Above 1 M: the table is 0.5 GiB, far beyond the caches; keys, values and lookup against numpy, once, folded and unfolded."""
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(16_000_000, 0)
    row = _row(len(pts), 31, top=3.0)
    uk, obs, keys = _np_sorted_map(pts, row, 0.1)
    P, R = _t(pts, dev), _t(row, dev)
    for fold in (True, False):
        cmap = ops.CoverageMap(resolution=0.1, device=dev)
        cmap.fold = fold
        cmap.integrate(P, R, "add")
        _, v, k = cmap.export()
        assert cmap.n_voxels == len(uk) and np.array_equal(k.cpu().numpy(), uk)
        assert np.array_equal(_bits(v), obs.view(np.uint32))
        assert np.array_equal(_bits(cmap.lookup(P)), obs[np.searchsorted(uk, keys)].view(np.uint32))
        assert cmap.skipped == (0, 0) and cmap.capacity >= 2 * len(uk)
        del cmap
