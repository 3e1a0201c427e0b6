"""The C entry points that only C hosts call (INTEGRATION.md's piecewise routes), each through the ABI against a plain
reference: numpy slicing for the gathers, exact index arithmetic for the permutation and the occlusion bit row, torch.optim.Adam
and an f64 restatement of its update, an np.float32 restatement of the reference's early-stop rule, the fused step tail against
the calls it stands for, and the fused reward + backward of several trajectories against single-trajectory calls and the f64
oracle.  Every output buffer carries sentinels where the call must not write."""
import numpy as np
import pytest
import torch

from conftest import rel_inf
from hard_size_cases import occ_row_ref as _occ_row_ref   # (the header's statement of a bit row, shared with tests/test_hip_hard_at_size.py)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
EINVAL = -1
NAN_BITS = 0x7fc00001   # a quiet NaN no kernel produces: the float sentinel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _L():
    from trajectory_optimization_amd import _lib
    return _lib.lib()


def _p(t):
    from trajectory_optimization_amd._lib import ptr
    return ptr(t)


def _s():
    from trajectory_optimization_amd._lib import stream_ptr
    return stream_ptr()


def _ok(code, what):
    from trajectory_optimization_amd._lib import check
    check(code, what)


def _sentinel_f32(shape, dev):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    """The raw 32-bit words of a float or int32 tensor, on the host (bitwise comparisons, NaN sentinels included)."""
    t = t.detach().contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy()


def _assert_bits(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), what


def _rand_f32(rng, shape, dev):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)


# ---- 1. gathers: bitwise against numpy slicing ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [3, 4, 7])
@pytest.mark.parametrize("step", [1, 2, 5])
def test_rows_strided_gather_and_scatter(dev, cols, step):
    L = _L()
    rng = np.random.default_rng(cols * 10 + step)
    for n_rows in (1, 63, 64, 65, 1000):
        full = (n_rows - 1) * step + 1 + 3   # rows past the last selected one: never read, never written
        src = _rand_f32(rng, (full, cols), dev)
        dst = _sentinel_f32((n_rows + 5, cols), dev)
        _ok(L.tohip_rows_strided(_p(src), n_rows, cols, step, 0, _p(dst), _s()), "gather")
        torch.cuda.synchronize()
        want = _bits(src)[::step][:n_rows]
        _assert_bits(_bits(dst)[:n_rows], want, ("gather", n_rows))
        assert np.all(_bits(dst)[n_rows:] == NAN_BITS)

        comp = _rand_f32(rng, (n_rows, cols), dev)
        out = _sentinel_f32((full, cols), dev)
        _ok(L.tohip_rows_strided(_p(comp), n_rows, cols, step, 1, _p(out), _s()), "scatter")
        torch.cuda.synchronize()
        ob = _bits(out)
        sel = np.zeros(full, bool)
        sel[np.arange(n_rows) * step] = True
        _assert_bits(ob[sel], _bits(comp), ("scatter", n_rows))
        assert np.all(ob[~sel] == NAN_BITS), ("scatter touched a row between", n_rows)
    assert L.tohip_rows_strided(_p(src), 4, cols, 0, 0, _p(dst), _s()) == EINVAL


@pytest.mark.parametrize("step", [1, 2, 5])
def test_gather_waypoints(dev, step):
    L = _L()
    rng = np.random.default_rng(100 + step)
    for n_eval in (1, 63, 64, 65, 1000):
        W = (n_eval - 1) * step + 1 + (step - 1)   # the last stride incomplete unless step = 1
        P, Q = _rand_f32(rng, (W, 3), dev), _rand_f32(rng, (W, 4), dev)
        pe, qe = _sentinel_f32((n_eval + 3, 3), dev), _sentinel_f32((n_eval + 3, 4), dev)
        _ok(L.tohip_gather_waypoints(_p(P), _p(Q), n_eval, step, _p(pe), _p(qe), _s()), "gather_waypoints")
        torch.cuda.synchronize()
        _assert_bits(_bits(pe)[:n_eval], _bits(P)[::step][:n_eval], ("poses", n_eval))
        _assert_bits(_bits(qe)[:n_eval], _bits(Q)[::step][:n_eval], ("quats", n_eval))
        assert np.all(_bits(pe)[n_eval:] == NAN_BITS) and np.all(_bits(qe)[n_eval:] == NAN_BITS)
    assert L.tohip_gather_waypoints(_p(P), _p(Q), 1, 0, _p(pe), _p(qe), _s()) == EINVAL


def test_gather_waypoints_multi(dev):
    L = _L()
    rng = np.random.default_rng(7)
    for B, n_eval, step in ((1, 4, 3), (3, 4, 3), (3, 5, 2), (65535, 4, 3), (3, 6, 1)):
        W = (n_eval - 1) * step + 1   # (n_eval - 1) step = W - 1; W not a multiple of step unless step = 1
        P, Q = _rand_f32(rng, (B * W, 3), dev), _rand_f32(rng, (B * W, 4), dev)
        pe, qe = _sentinel_f32((B * n_eval + 2, 3), dev), _sentinel_f32((B * n_eval + 2, 4), dev)
        _ok(L.tohip_gather_waypoints_multi(_p(P), _p(Q), W, B, n_eval, step, _p(pe), _p(qe), _s()), "gather_waypoints_multi")
        torch.cuda.synchronize()
        wp = _bits(P).reshape(B, W, 3)[:, ::step][:, :n_eval].reshape(-1, 3)
        wq = _bits(Q).reshape(B, W, 4)[:, ::step][:, :n_eval].reshape(-1, 4)
        _assert_bits(_bits(pe)[:B * n_eval], wp, ("poses", B, step))
        _assert_bits(_bits(qe)[:B * n_eval], wq, ("quats", B, step))
        assert np.all(_bits(pe)[B * n_eval:] == NAN_BITS) and np.all(_bits(qe)[B * n_eval:] == NAN_BITS)
    assert L.tohip_gather_waypoints_multi(_p(P), _p(Q), 10, 65536, 4, 3, _p(pe), _p(qe), _s()) == EINVAL
    assert L.tohip_gather_waypoints_multi(_p(P), _p(Q), 10, 3, 4, 0, _p(pe), _p(qe), _s()) == EINVAL


def _gather_points_case(L, dev, rng, n, layout, capacity, count, idx_np, extra_rows):
    rows = rng.standard_normal((n, 3)).astype(np.float32)
    xyz = torch.from_numpy(np.ascontiguousarray(rows if layout == 0 else rows.T)).to(dev)
    idx = torch.from_numpy(idx_np.astype(np.int32)).to(dev)
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    out = _sentinel_f32((capacity + extra_rows, 3), dev)
    _ok(L.tohip_gather_points(_p(xyz), n, layout, _p(idx), _p(cnt), capacity, _p(out), _s()), "gather_points")
    torch.cuda.synchronize()
    m = min(count, capacity)
    ob = _bits(out)
    _assert_bits(ob[:m], rows[idx_np[:m]], ("rows", layout, capacity, count))
    assert np.all(ob[m:] == NAN_BITS), ("written past min(count, capacity)", layout, capacity, count,
                                        int(np.argmax(np.any(ob[m:] != NAN_BITS, axis=1))) + m)


@pytest.mark.parametrize("layout", [0, 1])
def test_gather_points(dev, layout):
    L = _L()
    rng = np.random.default_rng(11 + layout)
    n, cap = 1000, 300
    dup = np.repeat(rng.integers(0, n, cap // 3 + 1), 3)[:cap + 64]          # every index three times
    dup = np.concatenate([dup, rng.integers(0, n, cap + 64 - dup.size)])
    rnd = rng.integers(0, n, cap + 64)
    for idx_np in (dup, rnd):
        for count in (0, 1, cap - 1, cap):
            _gather_points_case(L, dev, rng, n, layout, cap, count, idx_np, extra_rows=64)
    # a grid-stride loop: more rows than 2048 blocks x 256 threads
    big = 2048 * 256 + 4097
    _gather_points_case(L, dev, rng, 5000, layout, big, big, rng.integers(0, 5000, big), extra_rows=8)


@pytest.mark.parametrize("layout", [0, 1])
def test_gather_points_stops_at_capacity(dev, layout):
    """A device count above `capacity` writes capacity rows: the rows from capacity on keep their sentinels."""
    L = _L()
    rng = np.random.default_rng(21 + layout)
    n, cap = 1000, 300
    _gather_points_case(L, dev, rng, n, layout, cap, cap + 17, rng.integers(0, n, cap + 64), extra_rows=64)


# ---- 2. the inverse permutation of a packed cloud ------------------------------------------------------------------------------

@pytest.mark.parametrize("sort", [True, False])
def test_inverse_permutation(dev, sort):
    from trajectory_optimization_amd import ops
    L = _L()
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 2049, 1_000_003):
        pts = (rng.random((n, 3)) * 20 - 10).astype(np.float32)
        cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=sort)
        inv = torch.full((n + 37,), -7, dtype=torch.int32, device=dev)
        _ok(L.tohip_inverse_permutation(_p(cloud.blob), n, _p(inv), _s()), "inverse_permutation")
        torch.cuda.synchronize()
        inv_h, perm = _bits(inv), _bits(cloud.perm)[:n]
        assert np.array_equal(np.sort(perm), np.arange(n))
        assert np.array_equal(inv_h[perm], np.arange(n, dtype=np.int32)), n
        assert np.array_equal(inv_h[:n], _bits(cloud.inv_perm)), n
        assert np.all(inv_h[n:] == -7), n


# ---- 3. one waypoint's occlusion bit row -------------------------------------------------------------------------------------

@pytest.mark.parametrize("sort", [True, False])
def test_occlusion_row(dev, sort):
    from trajectory_optimization_amd import ops
    L = _L()
    rng = np.random.default_rng(5 + sort)
    for n in (1, 31, 32, 33, 2047, 2048, 2049, 100_000):
        pts = (rng.random((n, 3)) * 20 - 10).astype(np.float32)
        cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=sort)
        npad, roww = cloud.npad, cloud.npad // 32
        inv = _bits(cloud.inv_perm)
        last = int(_bits(cloud.perm)[n - 1])   # the caller's index of the last sorted point
        some = max(1, n // 3)
        cases = [(np.zeros(0, np.int64), np.zeros(0, np.int64)),                              # nothing kept
                 (np.sort(rng.choice(n, some, replace=False)), np.zeros(0, np.int64)),        # kept, none visible
                 (np.arange(n), np.arange(n))]                                                # all kept, all visible
        k = np.sort(rng.choice(n, some, replace=False))
        cases.append((k, np.sort(rng.choice(k.size, max(1, k.size // 2), replace=False))))   # some of some
        k = np.union1d(rng.choice(n, some, replace=False), [last])
        hide = int(np.searchsorted(k, last))
        vis = np.setdiff1d(np.arange(k.size), [hide])
        cases.append((k, vis))                                   # the last sorted point kept and hidden: pad bits 0
        for kept, vis_pos in cases:
            want = _occ_row_ref(n, npad, inv, kept, vis_pos)
            kept_d = torch.from_numpy(np.concatenate([kept, np.zeros(n - kept.size, np.int64)]).astype(np.int32)).to(dev)
            vis_d = torch.from_numpy(np.concatenate([vis_pos, [0]]).astype(np.int32)).to(dev)
            kc = torch.tensor([kept.size], dtype=torch.int32, device=dev)
            vc = torch.tensor([vis_pos.size], dtype=torch.int32, device=dev)
            row = torch.full((roww + 4,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
            _ok(L.tohip_occlusion_row(n, _p(cloud.inv_perm), _p(kept_d), _p(kc), _p(vis_d), _p(vc), _p(row), _s()), "occlusion_row")
            rows = torch.full((roww,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
            voff = torch.tensor([0, vis_pos.size], dtype=torch.int32, device=dev)
            allv = torch.zeros(1, dtype=torch.int32, device=dev)
            _ok(L.tohip_occlusion_rows(n, _p(cloud.inv_perm), _p(kept_d), _p(kc), _p(vis_d), _p(voff), _p(allv), 1, _p(rows), _s()),
                "occlusion_rows")
            torch.cuda.synchronize()
            rh = _bits(row)
            assert np.array_equal(rh[:roww], want), (n, sort, kept.size, vis_pos.size)
            assert np.all(rh[roww:] == 0x5a5a5a5a), (n, kept.size)
            assert np.array_equal(_bits(rows), rh[:roww]), (n, kept.size)
        if n % 2048:   # the hidden-last case: pad bits 0
            assert not (want.view(np.uint32)[-1] >> np.uint32(31)) & 1


# ---- 4. Adam for one group -----------------------------------------------------------------------------------------------

B1, B2, AEPS = 0.9, 0.999, 1e-8


def _adam(L, p, g, m, v, lr, step, state=None, n=None):
    return L.tohip_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel() if n is None else n, lr, B1, B2, AEPS, step, _p(state), _s())


@pytest.mark.parametrize("n", [1, 3, 4, 255, 256, 257, 100_003])
def test_adam_step_equals_torch_adam(dev, n):
    from trajectory_optimization_amd import _lib
    L = _L()
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * float(10.0 ** ((i * 7) % 5 - 3)) for i in range(25)]
    lr = 0.05
    tp = torch.nn.Parameter(p0.clone().to(dev))
    opt = torch.optim.Adam([tp], lr=lr)
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ps, ms, vs = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)            # step = 0, state[3]
    pm, mm, vm = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)            # tohip_adam_step_multi
    state = torch.zeros(8, device=dev)
    for i, g in enumerate(grads):
        gd = g.to(dev)
        tp.grad = gd.clone()
        opt.step()
        _ok(_adam(L, p, gd, m, v, lr, i + 1), "adam_step")
        state[3] = float(i)
        _ok(_adam(L, ps, gd, ms, vs, lr, 0, state), "adam_step (state)")
        grp = _lib.AdamGroup(pm.data_ptr(), gd.data_ptr(), mm.data_ptr(), vm.data_ptr(), n, lr, B1, B2, AEPS, i + 1)
        _ok(L.tohip_adam_step_multi(grp, 1, _s()), "adam_step_multi")
        torch.cuda.synchronize()
    np.testing.assert_allclose(p.cpu().numpy(), tp.detach().cpu().numpy(), rtol=2e-6, atol=1e-6)
    for a, b in ((p, ps), (m, ms), (v, vs), (p, pm), (m, mm), (v, vm)):
        _assert_bits(_bits(a), _bits(b))


def test_adam_step_one_step_against_f64(dev):
    """One update from a known state and step index vs torch's update restated in f64: within 4 f32 ulps of each parameter."""
    L = _L()
    rng = np.random.default_rng(9)
    n, t, lr = 100_003, 7, 0.01
    p0 = (rng.random(n) + 0.5).astype(np.float32) * np.where(rng.random(n) < 0.5, -1, 1).astype(np.float32)
    m0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v0 = (rng.random(n) * 0.009 + 0.001).astype(np.float32)   # updates well under |p|: 4 ulps of p measure the update
    g = (rng.standard_normal(n) * 0.3).astype(np.float32)
    p, m, v = (torch.from_numpy(x.copy()).to(dev) for x in (p0, m0, v0))
    _ok(_adam(L, p, torch.from_numpy(g).to(dev), m, v, lr, t), "adam_step")
    torch.cuda.synchronize()
    b1, b2, eps = (float(np.float32(x)) for x in (B1, B2, AEPS))
    md = b1 * m0.astype(np.float64) + (1 - b1) * g.astype(np.float64)
    vd = b2 * v0.astype(np.float64) + (1 - b2) * g.astype(np.float64) ** 2
    denom = np.sqrt(vd) / np.sqrt(1 - b2 ** t) + eps
    want = p0.astype(np.float64) - (float(np.float32(lr)) / (1 - b1 ** t)) * (md / denom)
    ulp = np.spacing(np.abs(want.astype(np.float32)))
    err = np.abs(p.cpu().numpy().astype(np.float64) - want) / ulp
    assert err.max() <= 4.0, err.max()


def test_adam_step_stopped_and_size_limit(dev):
    L = _L()
    gen = torch.Generator().manual_seed(2)
    p, g, m, v = (torch.randn(257, generator=gen).to(dev) for _ in range(4))
    v.abs_()
    before = [_bits(x) for x in (p, m, v)]
    state = torch.zeros(8, device=dev)
    state[2] = 1.0   # early stop reached
    _ok(_adam(L, p, g, m, v, 0.1, 3, state), "adam_step (stopped)")
    _ok(_adam(L, p, g, m, v, 0.1, 0, state), "adam_step (stopped, step from state)")
    torch.cuda.synchronize()
    for b, x in zip(before, (p, m, v)):
        _assert_bits(_bits(x), b)
    # n beyond int32: refused like tohip_adam_step_multi does (real 8-element buffers; no kernel may run)
    p8, g8, m8, v8 = (torch.ones(8, device=dev) for _ in range(4))
    assert _adam(L, p8, g8, m8, v8, 0.1, 1, n=2 ** 31) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(p8, torch.ones(8, device=dev)) and torch.equal(m8, torch.ones(8, device=dev))


# ---- 5. the early-stop rule, bitwise against np.float32 ------------------------------------------------------------------------

def _early_stop_ref(state, mean_r, smooth, rth, sth):
    """The reference's rule (src/trajectory_optimization.py:100-124) in np.float32, on the 8-float state of the header."""
    s = state.copy()
    f = np.float32
    if s[2] == 0:
        if s[3] == 0:
            s[0], s[1] = f(mean_r), f(smooth)
        s[3] = s[3] + f(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            vg, sg = f(mean_r) / s[0], s[1] / f(smooth)
        s[4], s[5] = vg, sg
        if vg > f(rth) and sg > f(sth):
            s[2] = f(1)
    return s


def _run_early_stop(dev, seq, rth, sth, row_from_state):
    L = _L()
    state = torch.zeros(8, device=dev)
    ref = np.zeros(8, np.float32)
    n = len(seq)
    log = torch.zeros((n + 1, 8), device=dev)
    stops = []
    for i, (mean_r, smooth) in enumerate(seq):
        scal = torch.tensor([mean_r, 1.0, 0.0, 0.0], device=dev)
        if row_from_state:
            log[:, 3] = float("nan")   # only the state's row may be read
            log[int(ref[3]), 3] = smooth
            lt = log
        else:
            lt = torch.tensor([0.0, 0.0, 0.0, smooth, 0.0, 0.0, 0.0, 0.0], device=dev)
        _ok(L.tohip_early_stop(_p(scal), _p(lt), rth, sth, _p(state), row_from_state, _s()), "early_stop")
        torch.cuda.synchronize()
        ref = _early_stop_ref(ref, np.float32(mean_r), np.float32(smooth), rth, sth)
        _assert_bits(_bits(state), ref, ("call", i))
        stops.append(bool(ref[2]))
    return stops, ref


@pytest.mark.parametrize("row_from_state", [0, 1])
def test_early_stop_rule(dev, row_from_state):
    f = np.float32
    th = float(f(0.6) / f(0.5))   # the gain of the third call below, exactly
    seq = [(0.5, 3.0), (0.55, 2.9), (0.6, 2.8), (0.65, 2.7), (0.7, 2.6), (0.8, 2.5)]
    stops, st = _run_early_stop(dev, seq, th, 0.5, row_from_state)
    assert stops == [False, False, False, True, True, True]   # gain == rewards_th does not stop (strict); 0.65 / 0.5 does
    assert st[3] == 4
    # the smoothness gain holds it back: smooth loss grows, smooth0 / smooth falls under 0.9
    stops, _ = _run_early_stop(dev, [(0.5, 1.0), (0.9, 1.2), (0.95, 1.05)], 1.2, 0.9, row_from_state)
    assert stops == [False, False, True]
    # rewards_th < 1: the first call stops (gains 1 and 1)
    stops, st = _run_early_stop(dev, [(0.4, 2.0), (0.9, 1.0)], 0.99, 0.5, row_from_state)
    assert stops == [True, True] and st[3] == 1
    # smooth loss 0 at the first step: 0 / 0 = NaN never stops (as the reference's torch tensors); then 0 / x = 0
    stops, st = _run_early_stop(dev, [(0.5, 0.0), (0.9, 0.0), (0.9, 1.0)], 1.1, -1.0, row_from_state)
    assert stops == [False, False, True] and st[5] == 0


# ---- 6. the split step equals the fused tail -----------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [1, 3])
def test_step_tail_equals_its_pieces(dev, step):
    """tohip_traj_step_tail == rows_strided x2 + traj_regularizers(accumulate, state) + adam_step x2 (step 0, state) + early_stop
    (row_from_state): every output bitwise after every call, through the early stop (call 9) and after it."""
    L = _L()
    W, calls = 23, 15
    n_eval = (W - 1) // step + 1
    sw, lw, eps, lr_p, lr_q, rth, sth = 28.0, 0.05, 1e-6, 0.12, 0.05, 1.075, -1e30
    rng = np.random.default_rng(step)
    poses0_np, quats_np = synth.make_path(W, optical=True, jitter_seed=3)
    poses0 = torch.from_numpy(poses0_np).to(dev)
    pge = _rand_f32(rng, (n_eval, 3), dev) * 0.01
    qge = _rand_f32(rng, (n_eval, 4), dev) * 0.01

    def fresh():
        d = dict(poses=poses0.clone() + 0.01 * _rand_f32(np.random.default_rng(0), (W, 3), dev),
                 quats=torch.from_numpy(quats_np).to(dev).clone(), pg=_sentinel_f32((W, 3), dev), qg=_sentinel_f32((W, 4), dev),
                 state=torch.zeros(8, device=dev), log=torch.zeros((calls, 8), device=dev))
        for k in ("mp", "vp"):
            d[k] = torch.zeros((W, 3), device=dev)
        for k in ("mq", "vq"):
            d[k] = torch.zeros((W, 4), device=dev)
        return d

    A, B = fresh(), fresh()
    stopped_at = None
    for c in range(calls):
        scal = torch.tensor([0.5 * (1 + 0.01 * c), 1.7 - 0.01 * c, -0.1, 0.0], device=dev)
        _ok(L.tohip_traj_step_tail(_p(A["poses"]), _p(A["quats"]), _p(poses0), W, _p(pge), _p(qge), n_eval, step, _p(A["pg"]),
                                   _p(A["qg"]), _p(A["mp"]), _p(A["vp"]), _p(A["mq"]), _p(A["vq"]), sw, lw, eps, lr_p, lr_q, B1, B2, AEPS,
                                   rth, sth, _p(scal), _p(A["log"]), _p(A["state"]), _s()), "traj_step_tail")
        B["pg"].zero_()
        B["qg"].zero_()
        _ok(L.tohip_rows_strided(_p(pge), n_eval, 3, step, 1, _p(B["pg"]), _s()), "rows_strided")
        _ok(L.tohip_rows_strided(_p(qge), n_eval, 4, step, 1, _p(B["qg"]), _s()), "rows_strided")
        _ok(L.tohip_traj_regularizers(_p(B["poses"]), _p(poses0), W, sw, lw, eps, _p(scal), _p(B["log"]), _p(B["pg"]), 1, _p(B["state"]),
                                      None, _s()), "traj_regularizers")
        _ok(L.tohip_adam_step(_p(B["poses"]), _p(B["pg"]), _p(B["mp"]), _p(B["vp"]), W * 3, lr_p, B1, B2, AEPS, 0, _p(B["state"]), _s()),
            "adam_step")
        _ok(L.tohip_adam_step(_p(B["quats"]), _p(B["qg"]), _p(B["mq"]), _p(B["vq"]), W * 4, lr_q, B1, B2, AEPS, 0, _p(B["state"]), _s()),
            "adam_step")
        _ok(L.tohip_early_stop(_p(scal), _p(B["log"]), rth, sth, _p(B["state"]), 1, _s()), "early_stop")
        torch.cuda.synchronize()
        for k in ("poses", "quats", "pg", "qg", "mp", "vp", "mq", "vq", "log", "state"):
            _assert_bits(_bits(A[k]), _bits(B[k]), (k, "call", c + 1))
        if stopped_at is None and A["state"][2].item() != 0:
            stopped_at = c + 1
    assert stopped_at == 9
    assert A["state"][3].item() == 9 and not torch.equal(A["poses"], poses0)


# (W, step, n_eval): the smallest legal W, no interior angle to spare | the last row is evaluated | W no multiple of the step, the
# trailing rows 7..9 carry the regularisers only | one element more than a block's stride: every strided loop takes a second trip
TAIL_SHAPES = [(3, 1, 3), (9, 2, 5), (10, 3, 3), (257, 1, 257)]


@pytest.mark.parametrize("clearance", [False, True])
@pytest.mark.parametrize("W,step,n_eval", TAIL_SHAPES)
def test_team_tail_members_are_trajectory_tails(dev, W, step, n_eval, clearance):
    """The block the two tails share: tohip_team_step_tail with B = 3 against tohip_traj_step_tail_multi (_clearance) with n_traj = 3
    on copies of the same random inputs, the same scalars row for every member, thresholds out of reach, two consecutive steps:
    poses, quats, full gradients, all four moments and the loss log's columns 0..3 (5 with clearance) are equal to the bit.
    Column 4 is left out: the team's total is the team's by design."""
    L = _L()
    B, n_steps = 3, 2
    sw, lw, eps, lr_p, lr_q, th, clr_w = 28.0, 0.05, 1e-6, 0.12, 0.05, 1e9, 0.7
    rng = np.random.default_rng(1000 * W + step)
    poses0 = _rand_f32(rng, (B * W, 3), dev)
    clr_rows = _rand_f32(rng, (B * W, 3), dev) * 0.01 if clearance else None
    clr_terms = torch.from_numpy(rng.random(B * W)).to(dev) if clearance else None   # f64, (r - d)^2 >= 0
    start = dict(poses=poses0 + 0.05 * _rand_f32(rng, (B * W, 3), dev), quats=_rand_f32(rng, (B * W, 4), dev))

    def fresh():
        d = {k: v.clone() for k, v in start.items()}
        d.update(pg=_sentinel_f32((B * W, 3), dev), qg=_sentinel_f32((B * W, 4), dev), log=torch.zeros((B, n_steps, 8), device=dev))
        for k, cols in (("mp", 3), ("vp", 3), ("mq", 4), ("vq", 4)):
            d[k] = torch.zeros((B * W, cols), device=dev)
        return d

    def head(d, pge, qge):
        return (_p(d["poses"]), _p(d["quats"]), _p(poses0), W, B, _p(pge), _p(qge), n_eval, step, _p(d["pg"]), _p(d["qg"]), _p(d["mp"]),
                _p(d["vp"]), _p(d["mq"]), _p(d["vq"]), sw, lw, eps, lr_p, lr_q, B1, B2, AEPS, th, th)

    T, M = fresh(), fresh()
    sb = L.tohip_team_state_bytes(B, n_steps)
    team_state = torch.zeros(sb, dtype=torch.uint8, device=dev)
    terms64 = team_state[sb // 2:].view(torch.float64).view(n_steps + 1, B, 4)
    _ok(L.tohip_team_loss(_p(T["poses"]), _p(poses0), W, B, sw, lw, eps, None, 0.0, None, _p(torch.empty((B, 8), device=dev)), _p(terms64),
                          None, None, None, _s()), "team_loss")
    state = torch.zeros((B, 8), device=dev)
    for i in range(n_steps):
        pge, qge = _rand_f32(rng, (B * n_eval, 3), dev) * 0.01, _rand_f32(rng, (B * n_eval, 4), dev) * 0.01
        row = torch.tensor([0.5 + 0.01 * i, 1.7 - 0.01 * i, -0.1, 0.0], device=dev)
        rows = row.repeat(B, 1).contiguous()
        _ok(L.tohip_team_step_tail(*head(T, pge, qge), _p(row), _p(T["log"]), n_steps * 8, _p(team_state), sb, n_steps, i, clr_w,
                                   _p(clr_rows), _p(clr_terms), _s()), "team_step_tail")
        if clearance:
            _ok(L.tohip_traj_step_tail_clearance(*head(M, pge, qge), _p(rows), _p(M["log"]), n_steps * 8, _p(state), clr_w, _p(clr_rows),
                                                 _p(clr_terms), _s()), "traj_step_tail_clearance")
        else:
            _ok(L.tohip_traj_step_tail_multi(*head(M, pge, qge), _p(rows), _p(M["log"]), n_steps * 8, _p(state), _s()), "traj_step_tail_multi")
        torch.cuda.synchronize()
        for k in ("poses", "quats", "pg", "qg", "mp", "vp", "mq", "vq"):
            assert torch.equal(T[k], M[k]), (k, "step", i + 1)
        cols = [0, 1, 2, 3, 5] if clearance else [0, 1, 2, 3]
        assert torch.equal(T["log"][:, :, cols], M["log"][:, :, cols]), ("loss log", "step", i + 1)
    assert (state[:, 3] == n_steps).all() and (state[:, 2] == 0).all()   # both steps were taken, by every trajectory
    assert not torch.equal(T["poses"], start["poses"]) and bool((T["log"][:, n_steps - 1, 3] != 0).all())


@pytest.mark.parametrize("masked", [False, True])
def test_pose_opt_step_equals_its_pieces(dev, masked):
    """INTEGRATION.md's piecewise pose step: tohip_pose_forward_backward + tohip_adam_step (trans, lr_pose) + tohip_adam_step (quat,
    lr_quat) is, bit for bit, tohip_pose_opt_step over ten steps; loss_log[step - 1] = that step's scalars[1]."""
    from trajectory_optimization_amd import ops
    L = _L()
    pts = synth.make_cloud(30_000, seed=4)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev), sort=False)
    cam = ops.Camera(K, IW, IH)
    poses, quats = synth.make_path(3, optical=True, jitter_seed=4)
    mask = None
    if masked:
        mask = torch.from_numpy((np.random.default_rng(4).random(cloud.n) < 0.7).astype(np.float32)).to(dev)
    wsb = L.tohip_pose_workspace_bytes(cloud.n)
    lr_p, lr_q, steps = 0.05, 0.02, 10

    def fresh():
        d = dict(t=torch.from_numpy(poses[1].copy()).to(dev), q=torch.from_numpy(quats[1].copy()).to(dev),
                 obs=torch.empty(cloud.n, device=dev), sc=torch.zeros(4, device=dev), tg=torch.zeros(3, device=dev),
                 qg=torch.zeros(4, device=dev), mt=torch.zeros(3, device=dev), vt=torch.zeros(3, device=dev),
                 mq=torch.zeros(4, device=dev), vq=torch.zeros(4, device=dev), log=torch.zeros(steps, device=dev),
                 ws=torch.zeros(wsb, dtype=torch.uint8, device=dev))
        return d

    A, B = fresh(), fresh()
    for s in range(1, steps + 1):
        _ok(L.tohip_pose_opt_step(_p(cloud.blob), cloud.n, _p(A["t"]), _p(A["q"]), cam.ref(), _p(mask), _p(A["obs"]), _p(A["sc"]),
                                  _p(A["tg"]), _p(A["qg"]), _p(A["mt"]), _p(A["vt"]), _p(A["mq"]), _p(A["vq"]), lr_p, lr_q, B1, B2, AEPS, s,
                                  _p(A["log"]), _p(A["ws"]), wsb, _s()), "pose_opt_step")
        _ok(L.tohip_pose_forward_backward(_p(cloud.blob), cloud.n, _p(B["t"]), _p(B["q"]), cam.ref(), _p(mask), _p(B["obs"]), _p(B["sc"]),
                                          None, _p(B["tg"]), _p(B["qg"]), _p(B["ws"]), wsb, _s()), "pose_forward_backward")
        _ok(L.tohip_adam_step(_p(B["t"]), _p(B["tg"]), _p(B["mt"]), _p(B["vt"]), 3, lr_p, B1, B2, AEPS, s, None, _s()), "adam_step")
        _ok(L.tohip_adam_step(_p(B["q"]), _p(B["qg"]), _p(B["mq"]), _p(B["vq"]), 4, lr_q, B1, B2, AEPS, s, None, _s()), "adam_step")
        B["log"][s - 1] = B["sc"][1]
        torch.cuda.synchronize()
        for k in ("t", "q", "obs", "sc", "tg", "qg", "mt", "vt", "mq", "vq", "log"):
            _assert_bits(_bits(A[k]), _bits(B[k]), (k, "step", s))
    assert not np.array_equal(A["t"].cpu().numpy(), poses[1])   # (zero observations would leave the pose where it was)


# ---- 7. the fused reward + backward of several trajectories ---------------------------------------------------------------

LENS = [7, 19, 3]


def _paths():
    ps, qs = [], []
    for i, n in enumerate(LENS):
        p, q = synth.make_path(n, optical=True, jitter_seed=60 + i)
        p[:, 1] += 0.7 * i
        ps.append(p)
        qs.append(q)
    return ps, qs


def _reward_backward_case(dev, cloud, cam, P, Q, toff, gout, rig, flags, occ, prefilled):
    """-> per trajectory: (rewards, scalars, pg, qg) of tohip_traj_reward_backward_multi; asserts them against
    tohip_traj_reward_multi and the single-trajectory forward + tohip_traj_reward_backward."""
    from trajectory_optimization_amd import ops
    L = _L()
    Bn, W, n = len(LENS), P.shape[0], cloud.n
    C = rig.n_cams if rig is not None else 1
    ws = ops.TrajWorkspace(cloud, W * C, Bn)
    half = torch.empty((Bn, n), device=dev) if prefilled else None
    lo, _ = ops.traj_forward(cloud, P, Q, cam, ws, rig, flags=flags, occ=occ, rewards_half=half, traj_offsets=toff)
    rm = half.clone() if prefilled else _sentinel_f32((Bn, n), dev)
    rb = half.clone() if prefilled else _sentinel_f32((Bn, n), dev)
    sm, sb = _sentinel_f32((Bn, 4), dev), _sentinel_f32((Bn, 4), dev)
    _ok(L.tohip_traj_reward_multi(_p(cloud.blob), _p(lo), n, Bn, cam.eps, int(prefilled), _p(rm), _p(sm), _p(ws.buf), ws.bytes, _s()),
        "traj_reward_multi")
    pg, qg = _sentinel_f32((W, 3), dev), _sentinel_f32((W, 4), dev)
    from trajectory_optimization_amd.ops import _NULL_RIG
    _ok(L.tohip_traj_reward_backward_multi(_p(cloud.blob), n, W, Bn, cam.ref(), rig.ref() if rig is not None else _NULL_RIG, flags, _p(occ),
                                           _p(lo), cam.eps, int(prefilled), _p(rb), _p(sb), _p(gout), _p(pg), _p(qg), _p(ws.buf), ws.bytes,
                                           _s()), "traj_reward_backward_multi")
    torch.cuda.synchronize()
    _assert_bits(_bits(rb), _bits(rm), "rewards vs tohip_traj_reward_multi")
    _assert_bits(_bits(sb), _bits(sm), "scalars vs tohip_traj_reward_multi")
    o, out = 0, []
    for b, w in enumerate(LENS):
        ws1 = ops.TrajWorkspace(cloud, w * C)
        occ1 = occ[o * C:(o + w) * C].contiguous() if occ is not None else None
        h1 = torch.empty(n, device=dev) if prefilled else None
        lo1, _ = ops.traj_forward(cloud, P[o:o + w].contiguous(), Q[o:o + w].contiguous(), cam, ws1, rig, flags=flags, occ=occ1,
                                  rewards_half=h1)
        r1, s1, pg1, qg1 = ops.traj_reward_backward(cloud, w, cam, ws1, lo1, gout[b:b + 1], rewards=h1, prefilled=prefilled, rig=rig,
                                                    flags=flags, occ=occ1)
        torch.cuda.synchronize()
        what = (b, flags, rig is not None, occ is not None, prefilled)
        _assert_bits(_bits(lo[b, :n]), _bits(lo1[:n]), ("lo_sum",) + what)
        _assert_bits(_bits(rb[b]), _bits(r1), ("rewards",) + what)
        _assert_bits(_bits(sb[b]), _bits(s1), ("scalars",) + what)
        _assert_bits(_bits(pg[o:o + w]), _bits(pg1), ("poses_grad",) + what)
        _assert_bits(_bits(qg[o:o + w]), _bits(qg1), ("quats_grad",) + what)
        out.append((rb[b].cpu().numpy(), sb[b].cpu().numpy(), pg[o:o + w].cpu().numpy(), qg[o:o + w].cpu().numpy()))
        o += w
    return out


@pytest.mark.parametrize("n", [3000, 120_000])
def test_reward_backward_of_several_trajectories(dev, n):
    from oracle import oracle
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(n, seed=31)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    cam = ops.Camera(K, IW, IH)
    ps, qs = _paths()
    P, Q = torch.from_numpy(np.concatenate(ps)).to(dev), torch.from_numpy(np.concatenate(qs)).to(dev)
    toff = torch.tensor(np.concatenate([[0], np.cumsum(LENS)]), dtype=torch.int32, device=dev)
    gout = torch.tensor([1.0, 0.5, 2.0], device=dev)
    rq, rt = synth.camera_rig(2)
    rig2 = ops.CameraRig(rq, rt, dev)
    occ1 = ops.occlusion_bits(cloud, cloud.points, P, Q, cam, 1.0, 15.0)
    occ2 = occ1.repeat_interleave(2, dim=0).contiguous()   # virtual waypoint v = w C + c: the body's row for both cameras
    assert 0 < int((occ1 != -1).sum()) and cloud.n == n
    perm = _bits(cloud.perm)[:n]
    ref = {}
    for occ_on in (False, True):
        o = 0
        for b, w in enumerate(LENS):
            occ_np = None
            if occ_on:
                rows = _bits(occ1[o:o + w]).view(np.uint32)
                bits = ((rows[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w, -1)[:, :n]
                occ_np = np.zeros((w, n), np.float32)
                occ_np[:, perm] = bits
            f = oracle.traj_forward(pts, ps[b], qs[b], K, IW, IH, prec="f64", occ=occ_np)
            pgr, qgr = oracle.traj_backward(pts, ps[b], qs[b], K, IW, IH, f, gout=float(gout[b]), prec="f64")
            ref[occ_on, b] = (f, pgr, qgr)
            o += w
    for flags in (0, ops.DENSE):
        for rig in (None, rig2):
            for occ_on in (False, True):
                occ = (occ2 if rig is not None else occ1) if occ_on else None
                for prefilled in (0, 1):
                    out = _reward_backward_case(dev, cloud, cam, P, Q, toff, gout, rig, flags, occ, prefilled)
                    if rig is not None:
                        continue   # (the oracle has no rig; the rig's gradient is pinned by test_hip_traj.py's rig tests)
                    for b in range(len(LENS)):
                        f, pgr, qgr = ref[occ_on, b]
                        rew, sc, pg, qg = out[b]
                        np.testing.assert_allclose(rew, f["rewards"], rtol=2e-5, atol=2e-6)
                        assert abs(sc[1] - f["loss_vis"]) <= 3e-6 * f["loss_vis"]
                        assert rel_inf(pg, pgr) < 1e-5 and rel_inf(qg, qgr) < 1e-5, (b, flags, occ_on, prefilled)


def test_reward_backward_of_several_trajectories_past_the_block_cap(dev):
    """1 M points: more than the 128 reward blocks per trajectory the split caps at (524 288 points)."""
    from trajectory_optimization_amd import ops
    pts = synth.make_cloud(1_000_000, seed=32)
    cloud = ops.PackedCloud(torch.from_numpy(pts).to(dev))
    cam = ops.Camera(K, IW, IH)
    ps, qs = _paths()
    P, Q = torch.from_numpy(np.concatenate(ps)).to(dev), torch.from_numpy(np.concatenate(qs)).to(dev)
    toff = torch.tensor(np.concatenate([[0], np.cumsum(LENS)]), dtype=torch.int32, device=dev)
    gout = torch.tensor([1.0, 0.5, 2.0], device=dev)
    for prefilled in (0, 1):
        out = _reward_backward_case(dev, cloud, cam, P, Q, toff, gout, None, 0, None, prefilled)
        assert all(np.isfinite(o[2]).all() and np.abs(o[2]).max() > 0 for o in out)
