"""CPU checks of the view proposal (no GPU): the two entry points are declared in the header and in _lib's table without a new ABI
version and refuse every bad argument before any launch; ops.check_propose and tools.propose_views refuse by name before any GPU
call; synth.propose_tables holds the f32 values of the definition; the numpy restatement of the pair test (synth.propose_hist_ref)
agrees with an independent f64 atan2 binning on inputs kept clear of every boundary and gate; the boundary predicates are monotone in
k on pairs placed on a boundary or one ulp beside it, which is what lets the kernel search instead of count; and
synth.propose_headings_ref gives what the definition dictates on rows small enough to work out by hand."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from abi_cases import ABI, check_abi_entries

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ENTRIES = ("tohip_view_histogram", "tohip_view_headings")
f32 = np.float32


def test_header_and_table_declare_the_view_entries():
    from trajectory_optimization_amd import ops, synth
    header, before = check_abi_entries(ENTRIES)
    assert re.search(rf"\(still {ABI}\) \+ tohip_view_histogram", before)
    for name, v in (("POSITIONS", 65536), ("PER_POSITION", 8)):
        assert f"#define TOHIP_VIEW_MAX_{name} {v}\n" in header
        assert getattr(ops, f"VIEW_MAX_{name}") == v == getattr(synth, f"VIEW_MAX_{name}")
    assert "#define TOHIP_VIEW_MAX_SECTORS 128\n" in header and ops.VIEW_SECTORS == synth.VIEW_SECTORS == (8, 16, 32, 64, 128)
    src = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "trajopt_hip.hip")).read()
    assert '#include "propose_kernels.hip"' in src
    kern = open(os.path.join(REPO, "trajectory_optimization_amd", "csrc", "propose_kernels.hip")).read()
    assert "atomicAdd((float" not in kern and "unsafeAtomicAdd" not in kern   # integer sums only


def test_entries_refuse_bad_arguments_without_gpu():
    from trajectory_optimization_amd import _lib, synth
    L = _lib.lib()
    p = ctypes.c_void_p(64)   # a non-null pointer no call may reach: every case below fails its checks first
    table = lambda S, poison=None: (ctypes.c_float * (2 * (S // 4 - 1)))(*[poison if poison is not None and i == 2 * (S // 4 - 1) - 1 else v for i, v in
                                                                           enumerate(synth.propose_tables(S)[0].reshape(-1).tolist())])
    names = ("packed", "n_points", "positions", "open", "n_positions", "weights", "sectors", "table_host", "min_dist", "max_dist", "tan_v",
             "prune", "hist", "stream")
    base = dict(zip(names, (p, 1000, p, p, 10, p, 32, table(32), 1.0, 5.0, 1.0, 1, p, None)))
    call = lambda **kw: L.tohip_view_histogram(*[kw.get(k, base[k]) for k in names])
    for k in ("packed", "positions", "open", "table_host", "hist"):
        assert call(**{k: None}) == EINVAL, k
    for v in (0, -1, 1 << 31, 1 << 40):
        assert call(n_points=v) == EINVAL, v
    for v in (0, -1, 65537, 1 << 40):
        assert call(n_positions=v) == EINVAL, v
    for v in (0, 4, 12, 31, 33, 256, -8):
        assert call(sectors=v) == EINVAL, v
    for mn, mx in ((0.0, 5.0), (9e-4, 5.0), (-1.0, 5.0), (5.0, 5.0), (6.0, 5.0), (float("nan"), 5.0), (1.0, float("nan")), (1.0, float("inf")),
                   (float("-inf"), 5.0)):
        assert call(min_dist=mn, max_dist=mx) == EINVAL, (mn, mx)
    for v in (-0.5, float("nan"), float("inf")):
        assert call(tan_v=v) == EINVAL, v
    for S in (8, 128):   # a table entry that is not finite is the last check: weights may be NULL on the way to it
        for poison in (float("nan"), float("inf")):
            assert call(sectors=S, table_host=table(S, poison), weights=None) == EINVAL, (S, poison)

    names = ("hist", "n_positions", "sectors", "half_window", "n_per", "sep", "min_score", "heading", "score", "stream")
    base = dict(zip(names, (p, 10, 32, 3, 2, 6, 0, p, p, None)))
    call = lambda **kw: L.tohip_view_headings(*[kw.get(k, base[k]) for k in names])
    for k in ("hist", "heading", "score"):
        assert call(**{k: None}) == EINVAL, k
    for k, vals in (("n_positions", (0, -1, 65537)), ("sectors", (0, 4, 24, 256)), ("half_window", (-1, 16, 1 << 30)), ("n_per", (0, -1, 9)),
                    ("sep", (-1, 33)), ("min_score", (-1, -(1 << 40)))):
        for v in vals:
            assert call(**{k: v}) == EINVAL, (k, v)
    assert call(sectors=8, half_window=4, sep=0) == EINVAL and call(sectors=128, half_window=64) == EINVAL   # 2 hw + 1 <= S


def test_check_propose_refuses_by_name():
    from trajectory_optimization_amd import ops
    P = torch.zeros(40, 3)
    assert ops.check_propose(100, P) == (40, 32, 1.0, 5.0, 1.0, 0, 2, 0, 0)
    w = torch.randint(0, 32769, (100,), dtype=torch.int32)
    w[0], w[1] = 0, 32768
    got = ops.check_propose(100, P.double(), torch.ones(40, dtype=torch.bool), w, 128, 0.001, 7, 0.0, 63, 8, 128, 1 << 40)
    assert got == (40, 128, float(f32(0.001)), 7.0, 0.0, 63, 8, 128, 1 << 40)
    assert ops.check_propose(100, torch.full((1, 3), float("nan")), hw=3)[7] == 6   # sep defaults to 2 hw; a NaN position is allowed
    bad = [
        (dict(positions=[[0, 0, 0]]), "positions must be a floating-point tensor"),
        (dict(positions=torch.zeros(40, 3, dtype=torch.int32)), "positions must be a floating-point tensor"),
        (dict(positions=torch.zeros(40, 2)), r"positions must be a floating-point tensor of shape \(M,3\)"),
        (dict(positions=torch.zeros(0, 3)), "1 <= M <= 65536 rows, got M = 0"), (dict(positions=torch.zeros(65537, 3)), "got M = 65537"),
        (dict(open=torch.ones(40)), r"open must be None or a bool / uint8 tensor of shape \(40,\)"),
        (dict(open=torch.ones(39, dtype=torch.bool)), "open must be"), (dict(open=[1] * 40), "open must be"),
        (dict(weights=torch.ones(100)), r"weights must be None or an int32 tensor of shape \(100,\)"),
        (dict(weights=torch.ones(99, dtype=torch.int32)), "weights must be None or an int32"),
        (dict(weights=torch.ones(100, dtype=torch.int64)), "weights must be None or an int32"),
        (dict(weights=torch.full((100,), -1, dtype=torch.int32)), r"weights must lie in \[0, 32768\], got -1\.\.-1"),
        (dict(weights=torch.tensor([0] * 99 + [32769], dtype=torch.int32)), r"weights must lie in \[0, 32768\], got 0\.\.32769"),
        (dict(sectors=4), "sectors must be one of"), (dict(sectors=24), "sectors must be one of"), (dict(sectors=32.0), "sectors must be one of"),
        (dict(sectors=256), "sectors must be one of"), (dict(sectors=True), "sectors must be one of"),
        (dict(min_dist=float("nan")), "min_dist must be a finite number"), (dict(min_dist="near"), "min_dist must be a finite number"),
        (dict(max_dist=float("inf")), "max_dist must be a finite number"), (dict(max_dist=1e60), "max_dist must be a finite number"),
        (dict(min_dist=0.0), "1e-3 <= min_dist < max_dist"), (dict(min_dist=9e-4), "1e-3 <= min_dist < max_dist"),
        (dict(min_dist=5.0), "1e-3 <= min_dist < max_dist"), (dict(min_dist=6.0, max_dist=5.5), "1e-3 <= min_dist < max_dist"),
        (dict(tan_v=-0.1), "tan_v must be >= 0"), (dict(tan_v=float("nan")), "tan_v must be a finite number"),
        (dict(tan_v=float("inf")), "tan_v must be a finite number"),
        (dict(hw=-1), r"hw must be an integer >= 0 with 2 hw \+ 1 <= sectors = 32"), (dict(hw=16), "hw must be"), (dict(hw=1.0), "hw must be"),
        (dict(hw=True), "hw must be"),
        (dict(n_per=0), r"n_per must be an integer in 1\.\.8"), (dict(n_per=9), "n_per must be"), (dict(n_per=2.0), "n_per must be"),
        (dict(sep=-1), r"sep must be None or an integer in 0\.\.32"), (dict(sep=33), "sep must be"), (dict(sep=1.5), "sep must be"),
        (dict(min_score=-1), "min_score must be an integer >= 0"), (dict(min_score=0.5), "min_score must be"),
        (dict(min_score=1 << 63), "min_score must be"),
    ]
    for kw, msg in bad:
        args = dict(n_points=100, positions=P, open=None, weights=None, sectors=32, min_dist=1.0, max_dist=5.0, tan_v=1.0, hw=3, n_per=2,
                    sep=None, min_score=0)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.check_propose(**args)
    with pytest.raises(ValueError, match="hist must be a contiguous"):
        ops.view_headings(torch.zeros(4, 32), 3, 2)
    with pytest.raises(ValueError, match="sectors must be one of"):
        ops.view_headings(torch.zeros(4, 24, dtype=torch.int64), 3, 2)
    with pytest.raises(RuntimeError, match="hist must live on a HIP device"):
        ops.view_headings(torch.zeros(4, 32, dtype=torch.int64), 3, 2)


class _Shard:
    def __init__(self, kind="waypoints", world_size=1, collective=False):
        self.kind, self.world_size, self.collective = kind, world_size, collective


def test_propose_views_refuses_before_any_gpu_call():
    from trajectory_optimization_amd import ops, synth
    from trajectory_optimization_amd.tools import propose_views
    pts, P = torch.zeros(50, 3), torch.zeros(40, 3)
    cam = dict(K=torch.from_numpy(synth.K_INTRINS), img_width=synth.IMG_WIDTH, img_height=synth.IMG_HEIGHT)
    for kw, msg in ((dict(positions=torch.zeros(40, 2)), "positions must be"), (dict(n_per_position=9), "n_per must be"),
                    (dict(n_per_position=0), "n_per must be"), (dict(sectors=20), "sectors must be one of"),
                    (dict(prior_log_odds=torch.zeros(49)), r"prior_log_odds must have shape \(50,\)"),
                    (dict(prior_log_odds=-torch.ones(50)), "prior_log_odds must be >= 0"),
                    (dict(clearance_radius=0.0), "clearance_radius"), (dict(clearance_radius=float("nan")), "clearance_radius"),
                    (dict(max_views=0), "max_views must be None or an integer >= 1"), (dict(max_views=2.5), "max_views must be"),
                    (dict(min_score=-1), "min_score must be"), (dict(min_dist=0.0), "1e-3 <= min_dist < max_dist"),
                    (dict(min_dist=5.0, max_dist=2.0), "1e-3 <= min_dist < max_dist"), (dict(K=None), r"the camera is needed: \['K'\] missing"),
                    (dict(img_width=None, img_height=None), r"\['img_width', 'img_height'\] missing"),
                    (dict(K=torch.eye(2)), "K must hold 3 x 3 intrinsics"), (dict(K=torch.zeros(3, 3)), "focal lengths"),
                    (dict(img_width=0.0), "img_width, img_height and the focal lengths"), (dict(img_height=float("nan")), "img_width, img_height")):
        args = dict(positions=P, **cam)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            propose_views(pts, **args)
    for shard in (_Shard("points"), _Shard("waypoints", 2, True)):
        model = types.SimpleNamespace(_cloud=types.SimpleNamespace(n=50), _shard=shard)
        with pytest.raises(ValueError, match="propose_views: a sharded model"):
            propose_views(model, P)
    packed = ops.PackedCloud.__new__(ops.PackedCloud)   # (no GPU here: an empty shell is enough to reach the check)
    packed.n = 50
    model = types.SimpleNamespace(_cloud=packed, _shard=_Shard())
    with pytest.raises(ValueError, match=r"\['max_dist', 'K'\] belong to the call with points"):
        propose_views(model, P, max_dist=4.0, K=cam["K"])
    with pytest.raises(ValueError, match=r"propose_views: points must be an \(N,3\) tensor"):
        propose_views("cloud.pcd", P, **cam)
    # every argument is fine: the last check before the first GPU call
    with pytest.raises(ValueError, match="propose_views: points must live on a HIP device"):
        propose_views(pts, P, prior_log_odds=torch.zeros(50), clearance_radius=0.3, max_views=10, **cam)


def test_propose_tables():
    from trajectory_optimization_amd import synth
    for S in (8, 16, 32, 64, 128):
        b, q = synth.propose_tables(S)
        Q = S // 4
        assert b.dtype == f32 and b.shape == (2, Q - 1) and q.dtype == f32 and q.shape == (S, 4)
        for k in range(1, Q):
            assert b[0, k - 1] == f32(np.cos(2 * np.pi * k / S)) and b[1, k - 1] == f32(np.sin(2 * np.pi * k / S))
        assert b[0, S // 8 - 1] == b[1, S // 8 - 1]                     # 45 degrees: the boundary is the diagonal exactly
        assert (np.diff(b[0]) < 0).all() and (np.diff(b[1]) > 0).all() and (b > 0).all()
        assert np.array_equal(b[0], b[1][::-1])                         # cos(x) = sin(90 - x), in f32 as well
        # heading h looks along the centre of sector h: candidate_grid's convention (heading 2 pi j / n + 0.1 there)
        for h in (0, 3, S - 1):
            a = (h + 0.5) * 2 * np.pi / S
            want = synth.quat_mul(np.array([np.cos(a / 2), 0, 0, np.sin(a / 2)]), synth.Q_OPTICAL)
            assert np.array_equal(q[h], want.astype(f32))
        assert np.allclose(np.linalg.norm(q.astype(np.float64), axis=1), 1.0, atol=1e-6)
    _, q4 = synth.candidate_grid([0.0], [0.0], 0.0, 4)
    a = 0.1   # candidate_grid's first heading: the same composition
    assert np.array_equal(q4[0], synth.quat_mul(np.array([np.cos(a / 2), 0, 0, np.sin(a / 2)]), synth.Q_OPTICAL).astype(f32))
    with pytest.raises(ValueError, match="sectors must be one of"):
        synth.propose_tables(12)


def clear_pairs(rng, n, S, mn, mx, tv):
    """n offsets (f64) at least 1e-3 rad from every sector boundary, 1e-3 relative from both range gates and from the elevation gate."""
    w = 2 * np.pi / S
    sector = rng.integers(0, S, n)
    bearing = (sector + rng.uniform(0.0, 1.0, n) * (1 - 2e-3 / w) + 1e-3 / w) * w
    rng_ok = rng.uniform(mn * 1.002, mx * 0.998, n)
    rng_out = np.where(rng.random(n) < 0.5, rng.uniform(0.05 * mn, mn * 0.998, n), rng.uniform(mx * 1.002, 3 * mx, n))
    r = np.where(rng.random(n) < 0.7, rng_ok, rng_out)
    lim = np.arctan(tv)
    el_in = rng.uniform(-1, 1, n) * lim * 0.998
    el_out = np.sign(rng.uniform(-1, 1, n)) * rng.uniform(lim * 1.002 + 1e-4, np.pi / 2 - 1e-3, n)
    el = np.where(rng.random(n) < 0.7, el_in, el_out)
    return np.stack([r * np.cos(el) * np.cos(bearing), r * np.cos(el) * np.sin(bearing), r * np.sin(el)], axis=1)


def atan2_hist(pts, pos, open_, w, S, mn, mx, tv):
    """The definition read in f64 with atan2: independent of the quadrant table and of the boundary predicates."""
    out = np.zeros((len(pos), S), dtype=np.int64)
    fin = np.isfinite(pts).all(axis=1)
    for c, t in enumerate(pos.astype(np.float64)):
        if not open_[c] or not np.isfinite(t).all():
            continue
        d = pts[fin].astype(np.float64) - t
        hh, zz = d[:, 0] ** 2 + d[:, 1] ** 2, d[:, 2] ** 2
        g = (hh + zz >= mn * mn) & (hh + zz <= mx * mx) & (zz <= tv * tv * hh)
        sec = np.floor(np.mod(np.arctan2(d[g, 1], d[g, 0]), 2 * np.pi) / (2 * np.pi / S)).astype(np.int64)
        np.add.at(out[c], sec, w[fin][g])
    return out


def test_restatement_agrees_with_an_atan2_binning_away_from_the_boundaries():
    from trajectory_optimization_amd import synth
    rng = np.random.default_rng(11)
    for S in (8, 32, 128):
        mn, mx, tv = 1.0, 6.0, 0.8
        pos = rng.uniform(-3, 3, (5, 3)).astype(f32)
        pos[3] = np.nan
        open_ = np.array([1, 1, 0, 1, 1])
        # per position its own well-separated points: the margins are relative to the position they were placed around.  Every
        # other position sees them at arbitrary offsets, so the comparison below is per position over its own points
        for c in (0, 1, 4):
            off = clear_pairs(rng, 4000, S, mn, mx, tv)
            pts = (pos[c].astype(np.float64) + off).astype(f32)
            # the f32 rounding of the sum moves a point by <= 6e-7 m at |x| <= 21: far inside the 1e-3 margins at range >= 0.05 m
            pts[::97] = np.nan
            w = rng.integers(0, 32769, len(pts))
            for weights in (None, w):
                got = synth.propose_hist_ref(pts, pos[c:c + 1], [1], weights, S, mn, mx, tv)
                want = atan2_hist(pts, pos[c:c + 1], [1], np.ones(len(pts), dtype=np.int64) if weights is None else w, S, mn, mx, tv)
                assert np.array_equal(got, want) and got.sum() > 0 and (got > 0).all()
        pts = (pos[0].astype(np.float64) + clear_pairs(rng, 2000, S, mn, mx, tv)).astype(f32)
        got = synth.propose_hist_ref(pts, pos, open_, None, S, mn, mx, tv)
        assert not got[2].any() and not got[3].any() and got[0].sum() > 0   # closed, not finite


def test_boundary_predicates_are_monotone_in_k():
    """For a > 0, b >= 0 the predicate fl(b c_k) >= fl(a s_k) must hold for k = 1 .. count and fail beyond, also for pairs on a boundary
    or one ulp beside it: then the largest k that holds (a binary search) is the count."""
    from trajectory_optimization_amd import synth
    rng = np.random.default_rng(12)
    for S in (8, 16, 32, 64, 128):
        (c, s), Q = synth.propose_tables(S)[0], S // 4
        n = 40_000
        r = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n))
        k = rng.integers(0, Q + 1, n)
        ang = 2 * np.pi * k / S
        a, b = (r * np.cos(ang)).astype(f32), (r * np.sin(ang)).astype(f32)
        b[k == 0], a[k == Q] = 0, np.abs(a[k == Q])   # exactly on the axes
        which = rng.integers(0, 5, n)
        a = np.where(which == 1, np.nextafter(a, f32(np.inf)), np.where(which == 2, np.nextafter(a, f32(0)), a)).astype(f32)
        b = np.where(which == 3, np.nextafter(b, f32(np.inf)), np.where((which == 4) & (b > 0), np.nextafter(b, f32(0)), b)).astype(f32)
        free = rng.random(n) < 0.3
        a[free], b[free] = np.abs(rng.standard_normal(free.sum())).astype(f32) + f32(1e-3), np.abs(rng.standard_normal(free.sum())).astype(f32)
        a = np.maximum(a, f32(1e-30))   # a > 0 in every quadrant of the table
        pred = (b[:, None] * c[None, :]) >= (a[:, None] * s[None, :])
        count = pred.sum(axis=1)
        assert (pred == (np.arange(1, Q)[None, :] <= count[:, None])).all()
        # and the count is the sector: against f64 where the pair is clear of every boundary
        th = np.arctan2(b.astype(np.float64), a.astype(np.float64)) / (2 * np.pi / S)
        clear = np.abs(th - np.rint(th)) > 1e-3
        assert (np.floor(th[clear]) == count[clear]).all() and clear.sum() > n // 10
        sec = synth.propose_sectors(a, b, S, (c, s))
        assert (sec == count).all()                                                            # quadrant 0
        assert (synth.propose_sectors(-b, a, S, (c, s)) == count + Q).all()                    # a quarter turn on: quadrant 1
        assert (synth.propose_sectors(-a, -b, S, (c, s)) == count + 2 * Q).all()
        assert (synth.propose_sectors(b, -a, S, (c, s)) == count + 3 * Q).all()
    assert synth.propose_sectors([0.0, np.nan], [0.0, 1.0], 8, synth.propose_tables(8)[0]).tolist() == [-1, -1]


def test_headings_restatement_by_hand():
    from trajectory_optimization_amd import synth
    R = synth.propose_headings_ref
    h, s = R(np.array([[3, 1, 4, 1, 5, 9, 2, 6]]), 0, 3)               # hw = 0: the bins themselves, no suppression beyond the winner
    assert h.tolist() == [[5, 7, 4]] and s.tolist() == [[9, 6, 5]] and h.dtype == np.int32 and s.dtype == np.int64
    h, s = R(np.array([[3, 1, 4, 1, 5, 9, 2, 6]]), 1, 3)               # windows: 10 8 6 10 15 16 17 11; sep = 2
    assert h.tolist() == [[6, 3, -1]] and s.tolist() == [[17, 10, 0]]  # 6 suppresses 4..0 (0 is 2 from 6), then 3 suppresses 1..5
    h, s = R(np.full((1, 32), 5), 3, 8)                                # all equal: the lowest heading, then every 7th while room is left
    assert h.tolist() == [[0, 7, 14, 21, -1, -1, -1, -1]] and s.tolist() == [[35] * 4 + [0] * 4]
    row = np.zeros((1, 16), dtype=np.int64)
    row[0, 15] = 4
    h, s = R(row, 2, 2)                                                # the window wraps: 13, 14, 15, 0, 1 all see it; lowest is 0
    assert h.tolist() == [[0, -1]] and s.tolist() == [[4, 0]]
    h, s = R(np.arange(16)[None], 7, 2)                                # 2 hw + 1 = 15: everything but the sector opposite
    assert h.tolist() == [[8, -1]] and s.tolist() == [[120, 0]]
    h, s = R(np.array([[7, 0, 0, 0, 3, 0, 0, 0]]), 0, 3, sep=1, min_score=5)
    assert h.tolist() == [[0, -1, -1]] and s.tolist() == [[7, 0, 0]]
    h, s = R(np.array([[7, 0, 0, 0, 3, 0, 0, 0]]), 0, 3, sep=1, min_score=3)
    assert h.tolist() == [[0, 4, -1]]
    assert R(np.zeros((2, 8)), 1, 2)[0].tolist() == [[-1, -1]] * 2     # a score of 0 is never proposed
    big = np.zeros((1, 32), dtype=np.int64)
    big[0, 10:13] = (1 << 45) + 1
    h, s = R(big, 1, 1)
    assert h.tolist() == [[11]] and s.tolist() == [[3 * ((1 << 45) + 1)]]
