"""The hard visibility path on the GPU at its thresholds and against oracles (hard_kernels.hip, render_kernels.hip, k_occ_rows_masked
of traj_kernels.hip): the frustum cull on each of its ways to a tile's offset, the cull of many poses past its scan rounds and the
grid.y limit, the z-buffer — one cloud and batched — against the numpy oracle on hand-built edges, at the lane / wave threshold and
past one trip, the cull -> z-buffer -> bit rows pipeline against oracle.occlusion_masks(method="zbuffer"), and
tohip_occlusion_rows_masked through the C ABI on both of its branches.  The inputs and references are those of
tests/hard_size_cases.py (checked without a GPU in tests/test_hard_at_size_cpu.py).  Every comparison is exact; the one exception is
the rendered colours, at tests/test_render.py's rtol 1e-6, atol 1e-7."""
import numpy as np
import pytest
import torch

import hard_size_cases as hc
from hard_size_cases import IH, IW, K

pytestmark = pytest.mark.gpu
IDX_SENTINEL, MASK_SENTINEL, ROW_SENTINEL = -7, 0x5a, 0x5a5a5a5a
NAN_BITS = 0x7fc00001   # a quiet NaN no kernel produces: the float sentinel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _abi():
    from trajectory_optimization_amd import _lib
    from trajectory_optimization_amd._lib import check, ptr, stream_ptr
    return _lib.lib(), check, ptr, stream_ptr


def _camera():
    from trajectory_optimization_amd import ops
    return ops.Camera(K, IW, IH)


# ---------------------------------------------------------------------------------------------------------------- A. the frustum cull

def _frustum(dev, cam3, n, masks=True, indices=True, count=True):
    """tohip_frustum_cull through the C ABI, NULL for what is not asked for; every buffer 64 entries longer than n, pre-filled."""
    L, check, ptr, stream_ptr = _abi()
    dm = torch.full((n + 64,), MASK_SENTINEL, dtype=torch.uint8, device=dev) if masks else None
    fm = torch.full((n + 64,), MASK_SENTINEL, dtype=torch.uint8, device=dev) if masks else None
    idx = torch.full((n + 64,), IDX_SENTINEL, dtype=torch.int32, device=dev) if indices else None
    cnt = torch.full((1,), IDX_SENTINEL, dtype=torch.int32, device=dev) if count else None
    wsb = L.tohip_frustum_workspace_bytes(n)
    ws = torch.full((wsb,), 0xa5, dtype=torch.uint8, device=dev)
    cam = _camera()
    check(L.tohip_frustum_cull(ptr(cam3), n, cam.ref(), hc.FRUSTUM_LIMITS[0], hc.FRUSTUM_LIMITS[1], ptr(dm), ptr(fm), ptr(idx), ptr(cnt), ptr(ws),
                               wsb, stream_ptr()), "tohip_frustum_cull")
    torch.cuda.synchronize()
    return dm, fm, idx, cnt


def _first_difference(got, want):
    bad = torch.nonzero(got != want).flatten()
    tile = hc.limits()["cull_tile"]
    return f"{bad.numel()} differ, the first at {bad[:3].tolist()} (entry // {tile} = {[int(b) // tile for b in bad[:3]]})" if bad.numel() else "equal"


def _check_frustum(dev, cam3, dist, fov, idx):
    """cam3 (3, n) f32, dist / fov (n,) bool, idx (m,) int32 ascending — all on the device."""
    n, m = cam3.shape[1], idx.numel()
    assert cam3.is_contiguous() and 0 < m < n

    def masks_ok(dm, fm):
        assert torch.equal(dm[:n], dist.to(torch.uint8)), _first_difference(dm[:n], dist.to(torch.uint8))
        assert torch.equal(fm[:n], fov.to(torch.uint8)), _first_difference(fm[:n], fov.to(torch.uint8))
        assert bool((dm[n:] == MASK_SENTINEL).all()) and bool((fm[n:] == MASK_SENTINEL).all())

    def indices_ok(got):
        assert torch.equal(got[:m], idx), _first_difference(got[:m], idx)
        assert bool((got[m:] == IDX_SENTINEL).all()), "an entry from kept_count on lost its sentinel"
    dm, fm, got, cnt = _frustum(dev, cam3, n)                                   # masks, indices and count
    masks_ok(dm, fm)
    assert int(cnt.item()) == m
    indices_ok(got)
    dm, fm, _, cnt = _frustum(dev, cam3, n, indices=False)                      # count only (the call the binary fov mask makes)
    masks_ok(dm, fm)
    assert int(cnt.item()) == m
    _, _, got, _ = _frustum(dev, cam3, n, masks=False, count=False)             # indices only
    indices_ok(got)


_PATTERN = [n for n, _, _, inputs in hc.FRUSTUM_SIZES if "pattern" in inputs]
_REAL = [n for n, _, _, inputs in hc.FRUSTUM_SIZES if "real" in inputs]
_DEVICE = [n for n, _, _, inputs in hc.FRUSTUM_SIZES if "device" in inputs]


@pytest.mark.parametrize("n", _PATTERN)
def test_frustum_cull_pattern(dev, n):
    kind = hc.pattern_kind(n)
    _check_frustum(dev, _t(hc.pattern_points(kind), dev), _t(kind != 1, dev), _t(kind != 2, dev), _t(np.flatnonzero(kind == 0).astype(np.int32), dev))


@pytest.mark.parametrize("n", _REAL)
def test_frustum_cull_real_predicate(dev, n):
    c = hc.real_frustum_case(n)
    assert np.array_equal(c["idx"], np.flatnonzero(c["dist"] & c["fov"]))
    _check_frustum(dev, _t(c["cam3"], dev), _t(c["dist"], dev), _t(c["fov"], dev), _t(c["idx"], dev))


@pytest.mark.parametrize("n", _DEVICE)
def test_frustum_cull_strided_write_pass(dev, n):
    """More tiles than the write pass has waves: input and expectation built on the device with plain torch ops."""
    kind = hc.pattern_kind_torch(n, dev)
    rows = _t(hc.KIND_ROWS, dev)
    cam3 = torch.stack([torch.where(kind == 2, rows[2, 0], rows[0, 0]), torch.zeros(n, device=dev), torch.where(kind == 1, rows[1, 2], rows[0, 2])])
    idx = torch.nonzero(kind == 0).flatten().to(torch.int32)
    strided = hc.limits()["write_blocks"] * 4 * hc.limits()["cull_tile"]
    assert int(idx[-1]) == n - 1 and int((idx >= strided).sum()) > 0          # kept points in the tiles of the second trip
    _check_frustum(dev, cam3.contiguous(), kind != 1, kind != 2, idx)
    del kind, cam3, idx
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ B. the cull of many poses

def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", ["scan", "offsets"])
def test_cull_of_many_poses_against_the_oracle(dev, name):
    from trajectory_optimization_amd import ops
    c = hc.cull_case(name)
    W = len(c["poses"])
    pts, poses, quats = _t(c["pts"], dev), _t(c["poses"], dev), _t(c["quats"], dev)
    want_counts = [len(c["ref"][w][0]) for w in range(W)]
    ki, kp, counts, kc = ops.cull_waypoints(pts, poses, quats, _camera(), *hc.CULL_LIMITS)
    ki2, cat, counts2, kc2, offs = ops.cull_waypoints(pts, poses, quats, _camera(), *hc.CULL_LIMITS, packed=True)
    assert counts == want_counts and counts2 == want_counts and kc.cpu().tolist() == want_counts and kc2.cpu().tolist() == want_counts
    offs = offs.cpu().numpy()
    assert offs.dtype == np.int64 and np.array_equal(offs, np.concatenate([[0], np.cumsum(want_counts)]))
    assert cat.shape == (sum(want_counts), 3)
    ki, kp, ki2, cat = ki.cpu().numpy(), kp.cpu().numpy(), ki2.cpu().numpy(), cat.cpu().numpy()
    for w in range(W):
        idx, rows = c["ref"][w]
        m = len(idx)
        assert np.array_equal(ki[w, :m], idx) and np.array_equal(ki2[w, :m], idx), w
        assert np.array_equal(_bits(kp[w, :m]), _bits(rows)), w
        assert np.array_equal(_bits(cat[offs[w]:offs[w + 1]]), _bits(rows)), w
    for w in c["away"]:
        assert want_counts[w] == 0


def test_cull_of_more_poses_than_one_grid_holds(dev):
    from trajectory_optimization_amd import ops
    c = hc.grid_case()
    W, cap = hc.GRID_POSES, hc.limits()["max_poses"]
    pts, poses, quats = _t(c["pts"], dev), _t(c["poses"], dev), _t(c["quats"], dev)
    cam = _camera()
    ki, kp, counts, kc = ops.cull_waypoints(pts, poses, quats, cam, *hc.CULL_LIMITS)
    assert ki.shape == (W, 8) and kp.shape == (W, 8, 3) and len(counts) == W and kc.cpu().tolist() == counts
    a = ops.cull_waypoints(pts, poses[:cap], quats[:cap], cam, *hc.CULL_LIMITS)
    b = ops.cull_waypoints(pts, poses[cap:], quats[cap:], cam, *hc.CULL_LIMITS)
    assert counts == a[2] + b[2] and 0 < sum(b[2])
    live = torch.arange(8, device=dev)[None, :] < kc[:, None]
    assert torch.equal(ki[live], torch.cat([a[0], b[0]])[live])
    assert torch.equal(kp[live].view(torch.int32), torch.cat([a[1], b[1]])[live].view(torch.int32))
    ki_h, kp_h = ki.cpu().numpy(), kp.cpu().numpy()
    for w in hc.GRID_LOOKED_AT:
        idx, rows = c["ref"][w]
        assert counts[w] == len(idx) and np.array_equal(ki_h[w, :len(idx)], idx) and np.array_equal(_bits(kp_h[w, :len(idx)]), _bits(rows)), w
    # end to end: as many poses as one call takes, and one more
    ki2, cat, counts2, kc2, offs = ops.cull_waypoints(pts, poses[:cap], quats[:cap], cam, *hc.CULL_LIMITS, packed=True)
    assert counts2 == counts[:cap] and np.array_equal(offs.cpu().numpy(), np.concatenate([[0], np.cumsum(counts2)]))
    assert torch.equal(ki2[live[:cap]], ki[:cap][live[:cap]])
    assert torch.equal(cat.reshape(-1, 3).view(torch.int32), kp[:cap][live[:cap]].view(torch.int32))
    with pytest.raises(ValueError):
        ops.cull_waypoints(pts, poses[:cap + 1], quats[:cap + 1], cam, *hc.CULL_LIMITS, packed=True)


# ---------------------------------------------------------------------------------------------------------------------- C. the z-buffer

def _render_against_the_oracle(dev, v, ref, params, colours=True):
    from trajectory_optimization_amd import ops
    ref_img, ref_owner, ref_own = ref
    img, owner, owns = ops.render_points(_t(v, dev), hc.SMALL_K, hc.SMALL_H, hc.SMALL_W, want_owner=True, **params)
    got = owner.cpu().numpy()
    assert np.array_equal(got, ref_owner), f"{(got != ref_owner).sum()} pixels differ, the first at {np.argwhere(got != ref_owner)[:3].tolist()}"
    assert np.array_equal(np.flatnonzero(owns.cpu().numpy()), ref_own)
    if colours:
        np.testing.assert_allclose(img.cpu().numpy(), ref_img, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("scene", ["edges", "edges_cover", "edges_nonfinite"])
def test_render_edge_scene_against_the_oracle(dev, scene):
    v = hc.edge_scene(scene == "edges_nonfinite")[0]
    params = hc.COVER_PARAMS if scene == "edges_cover" else hc.PARAMS
    # the rows that are not finite: owners and `owns` only (the colours are NaN by the min / max rule)
    _render_against_the_oracle(dev, v, hc.owners(v, params), params, colours=scene != "edges_nonfinite")


def test_render_threshold_cloud_against_the_oracle(dev):
    v = hc.threshold_cloud()[0]
    _render_against_the_oracle(dev, v, hc.owners(v), hc.PARAMS)


def test_render_second_trip_against_the_oracle(dev):
    stride = hc.limits()["splat_blocks"] * hc.limits()["block"]
    v, img, owner, own = hc.second_trip_cloud(stride)
    assert (own >= stride).any()
    _render_against_the_oracle(dev, v, (img, owner, own), hc.PARAMS)


def _batched(dev, clouds, params, one_buffer):
    """tohip_zbuffer_visible_batched of the clouds, n_stride = the longest; the rows past a cloud's count hold a point that would own
    pixels if it were read -> visible (B, n_stride) on the host."""
    L, check, ptr, stream_ptr = _abi()
    B, n_stride = len(clouds), max(1, max(len(c) for c in clouds))
    verts = torch.tensor([0.0, 0.0, 1.25], device=dev).repeat(B, n_stride, 1).contiguous()
    for w, c in enumerate(clouds):
        if len(c):
            verts[w, :len(c)] = _t(c, dev)
    cnt = torch.tensor([len(c) for c in clouds], dtype=torch.int32, device=dev)
    one = hc.SMALL_W * hc.SMALL_H * 8
    wsb = one if one_buffer else L.tohip_zbuffer_batched_workspace_bytes(hc.SMALL_W, hc.SMALL_H, B)
    assert one_buffer or wsb == B * one
    ws = torch.full((wsb,), 0xa5, dtype=torch.uint8, device=dev)
    vis = torch.full((B * n_stride + 64,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    import ctypes
    K9 = (ctypes.c_float * 9)(*hc.SMALL_K.reshape(9).tolist())
    check(L.tohip_zbuffer_visible_batched(ptr(verts), n_stride, ptr(cnt), B, K9, hc.SMALL_W, hc.SMALL_H, params["radius"], params["znear"], params["zfar"],
                                          ptr(vis), ptr(ws), wsb, stream_ptr()), "tohip_zbuffer_visible_batched")
    torch.cuda.synchronize()
    assert bool((vis[B * n_stride:].view(torch.int32) == NAN_BITS).all())
    return vis[:B * n_stride].view(B, n_stride).cpu().numpy()


def _check_batched(vis, clouds, own_sets):
    for w, (c, own) in enumerate(zip(clouds, own_sets)):
        assert set(np.unique(vis[w]).tolist()) <= {0.0, 1.0}
        assert np.array_equal(np.flatnonzero(vis[w, :len(c)]), own), (w, np.setxor1d(np.flatnonzero(vis[w, :len(c)]), own)[:8])
        assert not vis[w, len(c):].any(), w


def test_batched_zbuffer_against_the_oracle(dev):
    """Every cloud's visible set = the rows that own a pixel in the oracle's picture of that cloud alone; with room for every
    z-buffer and with room for exactly one (as many chunks as clouds), the same."""
    clouds = hc.batched_clouds()
    own_sets = [hc.reference_owners(k)[2] for k in range(len(clouds))]
    assert sum(len(o) for o in own_sets[:3]) > 100
    vis = _batched(dev, clouds, hc.PARAMS, one_buffer=False)
    _check_batched(vis, clouds, own_sets)
    again = _batched(dev, clouds, hc.PARAMS, one_buffer=True)
    assert np.array_equal(vis, again)
    # the point in front of everything, its disc over the whole image: a box of 12 288 pixels walked by the wave
    cover = [clouds[0], clouds[3], clouds[0]]
    own_sets = [hc.owners(c, hc.COVER_PARAMS)[2] for c in cover]
    assert own_sets[0].tolist() == hc.edge_scene()[1]["covers_all"]
    for one_buffer in (False, True):
        _check_batched(_batched(dev, cover, hc.COVER_PARAMS, one_buffer), cover, own_sets)


def test_batched_zbuffer_second_trip(dev):
    stride = hc.limits()["splat_batched_blocks"] * hc.limits()["block"]
    v, _, _, own = hc.second_trip_cloud(stride)
    assert (own >= stride).any()
    clouds = [hc.small_scene(65, 165), v]
    _check_batched(_batched(dev, clouds, hc.PARAMS, one_buffer=False), clouds, [hc.reference_owners(7)[2], own])


# --------------------------------------------------------------------------------------------------- C'. the pipeline: cull -> z-buffer

@pytest.mark.parametrize("sort", [True, False])
def test_zbuffer_occlusion_rows_against_the_oracle(dev, sort):
    """ops.occlusion_bits(..., "zbuffer") — cull of all poses, batched z-buffer at the real image, bit rows — unpacked to the caller's
    order against oracle.occlusion_masks(method="zbuffer"), and word for word (pad bits included) against occ_row_ref."""
    from trajectory_optimization_amd import ops
    c = hc.rows_case()
    n, W = hc.ROWS_N, hc.ROWS_W
    cloud = ops.PackedCloud(_t(c["pts"], dev), sort=sort)
    assert cloud.npad > n
    rows = ops.occlusion_bits(cloud, cloud.points, _t(c["poses"], dev), _t(c["quats"], dev), _camera(), *hc.CULL_LIMITS, "zbuffer")
    assert rows.shape == (W, cloud.npad // 32) and rows.dtype == torch.int32
    occ = ops.unpack_occlusion_rows(cloud, rows).cpu().numpy()
    for w in range(W):
        bad = np.flatnonzero(occ[w] != c["want"][w])
        assert len(bad) == 0, (w, c["counts"][w], len(bad), bad[:8].tolist())
    assert np.array_equal(occ, c["want"]) and occ.dtype == np.float32
    inv, got = cloud.inv_perm.cpu().numpy(), rows.cpu().numpy()
    for w in range(W):
        want = hc.occ_row_ref(n, cloud.npad, inv, c["kept"][w], visible=c["want"][w][c["kept"][w]], min_points=4)
        assert np.array_equal(got[w], want), w
    assert (got[[hc.ROWS_NOTHING, hc.ROWS_THREE]] == -1).all()


# ------------------------------------------------------------------------------------------------- D. tohip_occlusion_rows_masked

def _rows_masked(dev, n, npad, inv, kept, counts, visible, seg_off, min_points):
    L, check, ptr, stream_ptr = _abi()
    W, roww = len(counts), npad // 32
    rows = torch.full((W * roww + 16,), ROW_SENTINEL, dtype=torch.int32, device=dev)
    kc = torch.tensor(counts, dtype=torch.int32, device=dev)
    so = torch.tensor(seg_off, dtype=torch.int64, device=dev)
    inv_d = None if inv is None else _t(inv, dev)
    kept_d, vis_d = _t(kept, dev), _t(visible, dev)
    check(L.tohip_occlusion_rows_masked(n, ptr(inv_d), ptr(kept_d), ptr(kc), ptr(vis_d), ptr(so), min_points, W, ptr(rows), stream_ptr()),
          "tohip_occlusion_rows_masked")
    torch.cuda.synchronize()
    out = rows.cpu().numpy()
    assert (out[W * roww:] == ROW_SENTINEL).all()
    return out[:W * roww].reshape(W, roww)


@pytest.mark.parametrize("in_packed_order", [False, True], ids=["inv_perm", "packed_order"])
def test_occlusion_rows_masked_directly(dev, in_packed_order):
    c = hc.occ_rows_case(in_packed_order)
    n, m = hc.OCC_N, hc.OCC_KEPT
    got = _rows_masked(dev, n, c["npad"], c["inv"], c["kept"], [m, m], c["visible"], hc.OCC_SEG_OFF, 4)
    for w in range(2):
        bad = np.flatnonzero(got[w] != c["want"][w])
        assert len(bad) == 0, (w, len(bad), "words", bad[:8].tolist())
    # three kept points against four, all "hidden": the row of ones against four cleared bits
    hidden = np.zeros_like(c["visible"])
    got = _rows_masked(dev, n, c["npad"], c["inv"], c["kept"], [3, 4], hidden, hc.OCC_SEG_OFF, 4)
    want = [hc.occ_row_ref(n, c["npad"], c["inv"], c["kept"][w, :k], visible=np.zeros(k), min_points=4) for w, k in ((0, 3), (1, 4))]
    assert (want[0] == -1).all() and np.array_equal(got[0], want[0])
    ones = int(np.unpackbits(want[1].view(np.uint8)).sum())
    pos = c["kept"][1, :4] if c["inv"] is None else c["inv"][c["kept"][1, :4]]
    assert ones == c["npad"] - 4 - (c["npad"] - n if n - 1 in pos.tolist() else 0) and np.array_equal(got[1], want[1])
