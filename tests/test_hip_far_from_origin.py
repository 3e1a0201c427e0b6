"""Every kernel far from the origin.

1. Exact translation invariance.  The inputs lie on a 2^-10 m grid within +-32 m and T = (8192, -8192, 4096): every translated
   coordinate is representable and every difference x - t, b - a, x - origin keeps its bits (tests/test_far_from_origin_cpu.py proves
   it for the fixtures and for the references).  The reference computes everything from y = x - t, so every output of the run at T
   must equal the run at the origin BIT FOR BIT — no tolerance.  What differs between the two runs is only what must not matter: the
   tile spheres (their centres fall between grid points at T), the prunes' slack and the culling decisions.
   Not invariant by definition, and so not in the bitwise list but in part 2:
   * the ingest voxel grid — trajectory_optimization_amd/csrc/ingest_kernels.hip:223 and :242-244: a point's cell is
     floorf(x * inv_leaf) of the ABSOLUTE coordinate (as the reference's VoxelGrid filter), and a voxel's centroid is a sequential
     float32 sum of absolute coordinates;
   * world-frame hidden-point removal, ops.hidden_pts_removal and ModelPose.forward(hpr=True) — hard_kernels.hip:640 (k_flip) and
     hull_kernels.hip:2374 (k_flip_seg): the spherical flip is about the world origin, which IS the viewpoint
     (/root/reference/src/model.py:112-115, tools.py:56-85);
   * PackedCloud's tile spheres (hard_kernels.hip:130, c = (min + max) / 2 of absolute coordinates): not an output; whatever they
     are, the culled results must equal the dense ones, which parts 2 and 3 assert.
2. Unsnapped offsets 1e3 and 1e5 (1e6 for the clearance queries): the float32 inputs are the definition; the clearance queries
   against their numpy brute forces bit for bit, culled against dense bit for bit, the models against the f64 oracle on the same
   float32 inputs under the project's own bars (tests/test_hip_conditioning.py); the voxel grid against oracle/ingest_oracle.py bit
   for bit and world-frame HPR against the Qhull oracle, index set for index set.
3. Degenerate bounding boxes for the Morton pack: an outlier that sends every other point into cell 0, a planar, a collinear and an
   all-but-one-identical cloud, the slab at millimetre and at kilometre scale."""
import numpy as np
import pytest
import torch

from test_far_from_origin_cpu import (COVMAP_ORIGIN, COVMAP_R, T, cloud as snapped_cloud, covmap_rows, path as snapped_path, queries,
                                      segments, shifted, snap, walled_scene)
from trajectory_optimization_amd import synth

pytestmark = pytest.mark.gpu
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
f32, f64 = np.float32, np.float64
N, N_BIG = 20_000, 300_000   # 79 tiles: more than one wave's group of spheres; 1 172 tiles: a wave's second group, shrunken radius


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(x):
    x = x.detach().contiguous().reshape(-1)
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64) if x.dtype == torch.float64 else x


def _how(x, y):
    if x.shape != y.shape or x.dtype != y.dtype:
        return f"{tuple(x.shape)} {x.dtype} against {tuple(y.shape)} {y.dtype}"
    n = int((_bits(x) != _bits(y)).sum())
    if not x.is_floating_point():
        return f"{n} of {x.numel()} entries differ"
    gap = (x.double() - y.double()).abs()
    return f"{n} of {x.numel()} entries differ, max |a - b| = {float(torch.nan_to_num(gap, nan=float('inf')).max()):.3e}"


def assert_same(a, b, what):
    """Two dicts of outputs, bit for bit (a NaN equals the same NaN, -0.0 does not equal +0.0); the message names the output."""
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), f"{what}: {k}: {_how(x, y)}"
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y), f"{what}: {k}"
        else:
            assert x == y, f"{what}: {k}: {x!r} against {y!r}"


def at(a, t):
    return np.asarray(a, f32) if t is None else shifted(a, t)


def _cam(ops, clip=(1.0, 5.0)):
    return ops.Camera(K, IW, IH, clip[0], clip[1])


def _prior_row(n):
    rng = np.random.default_rng(23)
    row = (rng.random(n) * 2.0).astype(f32)
    row[rng.random(n) < 0.3] = 0.0
    return row


# ================================================================================ 1. exact translation invariance

def test_packed_cloud_keeps_its_order(dev):
    from trajectory_optimization_amd import ops
    pts = snapped_cloud(N)
    a, b = (ops.PackedCloud(_t(at(pts, t), dev), sort=True) for t in (None, T))
    assert torch.equal(a.perm, b.perm), "perm"
    assert torch.equal(a.inv_perm, b.inv_perm), "inv_perm"
    n = a.npad
    for k in range(3):
        assert torch.equal(a.soa[k * n:k * n + a.n] + float(T[k]), b.soa[k * n:k * n + a.n]), f"soa row {k}"
    assert sorted(a.perm[:a.n].tolist()) == list(range(a.n))


TRAJ_MODES = ["dense", "culled", "rig3", "prior", "hpr", "zbuffer"]


def _traj_outputs(dev, mode, t, W=17):
    from trajectory_optimization_amd import ops
    pts, (p, q) = snapped_cloud(N), snapped_path(W)
    x = _t(at(pts, t), dev)
    cloud, cam = ops.PackedCloud(x), _cam(ops)
    ps, qs = _t(at(p, t), dev), _t(q, dev)
    rig = ops.CameraRig(*synth.camera_rig(3), dev) if mode == "rig3" else None
    flags = ops.DENSE if mode == "dense" else 0
    prior = ops.LogOddsPrior(cloud, _t(_prior_row(N), dev)) if mode == "prior" else None
    occ = ops.occlusion_bits(cloud, cloud.points, ps, qs, cam, 1.0, 15.0, mode) if mode in ("hpr", "zbuffer") else None
    V = W * (3 if rig is not None else 1)
    gout = torch.ones(1, dtype=torch.float32, device=dev)
    out = {}
    ws = ops.TrajWorkspace(cloud, V)
    lo, mm = ops.traj_forward(cloud, ps, qs, cam, ws, rig, flags=flags, occ=occ)
    out["forward lo_sum"], out["forward minmax"] = lo[:cloud.n].clone(), mm.clone()
    r, s, pg, qg = ops.traj_reward_backward(cloud, W, cam, ws, lo, gout, rig=rig, flags=flags, occ=occ, prior=prior)
    out.update({"rewards": r, "scalars": s, "poses_grad": pg, "quats_grad": qg})
    if prior is None:
        ws2 = ops.TrajWorkspace(cloud, V)
        r2, s2, pg2, qg2, lo2, mm2 = ops.traj_forward_backward(cloud, ps, qs, cam, ws2, gout, rig=rig, flags=flags, occ=occ)
        out.update({"one call rewards": r2, "one call scalars": s2, "one call poses_grad": pg2, "one call quats_grad": qg2,
                    "one call lo_sum": lo2[:cloud.n].clone(), "one call minmax": mm2})
    if occ is not None:
        out["occlusion rows"] = occ
    return out


@pytest.mark.parametrize("mode", TRAJ_MODES)
def test_traj_forward_and_backward(dev, mode):
    a, b = _traj_outputs(dev, mode, None), _traj_outputs(dev, mode, T)
    assert_same(a, b, f"traj {mode}")
    assert int((a["rewards"] > 0.5).sum()) > 100 and float(a["poses_grad"].abs().max()) > 0.0 and float(a["quats_grad"].abs().max()) > 0.0
    assert not bool(torch.isnan(a["rewards"]).any())
    if "occlusion rows" in a:   # the rows hide something and keep something
        assert 0 < int((a["forward lo_sum"] > 0).sum()) < N


@pytest.mark.parametrize("method", ["hpr", "zbuffer"])
def test_occlusion_bits(dev, method):
    from trajectory_optimization_amd import ops
    pts, (p, q) = snapped_cloud(N), snapped_path(9)
    rows = []
    for t in (None, T):
        cloud = ops.PackedCloud(_t(at(pts, t), dev))
        rows.append(ops.occlusion_bits(cloud, cloud.points, _t(at(p, t), dev), _t(q, dev), _cam(ops), 1.0, 15.0, method))
        seen = ops.unpack_occlusion_rows(cloud, rows[-1]).sum(dim=1)
    assert torch.equal(rows[0], rows[1]), f"occlusion bit rows ({method}): {_how(rows[0], rows[1])}"
    assert bool((seen > 0).all()) and bool((seen < N).all())


CLR = dict(clearance_radius=0.75, clearance_weight=2.0)


def _model_outputs(m, loss):
    loss.backward()
    out = {"loss": loss.detach(), "rewards": m.rewards.detach(), "poses.grad": m.poses.grad, "quats.grad": m.quats.grad}
    for k, v in m.loss.items():
        for j, e in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            out[f"loss[{k}]" + (f"[{j}]" if isinstance(v, (list, tuple)) else "")] = e.detach()
    return out


def _model_traj(dev, t, W=17, **kw):
    from trajectory_optimization_amd.model import ModelTraj
    pts, (p, q) = snapped_cloud(N), snapped_path(W)
    return ModelTraj(torch.from_numpy(at(pts, t)), torch.from_numpy(at(p, t)), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev,
                     **kw)


@pytest.mark.parametrize("vwd", [0.0, 2.5])
@pytest.mark.parametrize("mode", ["waypoints", "segments"])
def test_model_traj(dev, mode, vwd):
    outs = []
    for t in (None, T):
        m = _model_traj(dev, t, clearance_mode=mode, **CLR)
        spacing = float(np.linalg.norm(np.diff(snapped_path(17)[0].astype(f64), axis=0), axis=1).mean())
        assert (int(vwd / spacing) + 1 > 1) == (vwd > 0.0)   # forward's rule: every (int(vis_wps_dist / mean spacing) + 1)-th waypoint
        outs.append(_model_outputs(m, m(vis_wps_dist=vwd)))
    assert_same(outs[0], outs[1], f"ModelTraj {mode} vis_wps_dist={vwd}")
    a = outs[0]
    assert set(k for k in a if k.startswith("loss[")) == {"loss[vis]", "loss[l2]", "loss[length]", "loss[smooth]", "loss[clearance]"}
    assert float(a["loss[clearance]"]) > 0.0 and float(a["quats.grad"].abs().max()) > 0.0


@pytest.mark.parametrize("kind", ["prior", "zbuffer", "rig3"])
def test_model_traj_other_paths(dev, kind):
    """The separate-call step (a prior, occlusion rows) and a rig through the model."""
    kw = {"prior": dict(prior_log_odds=torch.from_numpy(_prior_row(N))), "zbuffer": dict(occlusion="zbuffer"),
          "rig3": dict(rig=synth.camera_rig(3))}[kind]
    outs = []
    for t in (None, T):
        m = _model_traj(dev, t, **{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()})
        outs.append(_model_outputs(m, m(vis_wps_dist=0.0)))
    assert_same(outs[0], outs[1], f"ModelTraj {kind}")
    assert float(outs[0]["poses.grad"].abs().max()) > 0.0


def test_team_of_two(dev):
    from trajectory_optimization_amd.model import ModelTraj, TeamTraj
    pts, (p, q) = snapped_cloud(N), snapped_path(17)
    side = f32([0.0, 1.5, 0.0])
    outs = []
    for t in (None, T):
        first = ModelTraj(torch.from_numpy(at(pts, t)), torch.from_numpy(at(p, t)), torch.from_numpy(q), torch.from_numpy(K), IW, IH,
                          device=dev, **CLR)
        second = ModelTraj.sharing_cloud_of(first, torch.from_numpy(at(snap(p + side), t)), torch.from_numpy(q), **CLR)
        team = TeamTraj([first, second])
        total = team(vis_wps_dist=0.0)
        total.backward()
        out = {"total": total.detach(), "rewards": team.rewards.detach()}
        for k, v in team.loss.items():
            for j, e in enumerate(v if isinstance(v, list) else [v]):
                out[f"loss[{k}][{j}]"] = e.detach()
        for j, m in enumerate((first, second)):
            out[f"member {j} poses.grad"], out[f"member {j} quats.grad"] = m.poses.grad, m.quats.grad
        outs.append(out)
    assert_same(outs[0], outs[1], "TeamTraj")
    a = outs[0]
    assert float(a["loss[clearance][0]"]) > 0.0 and float(a["loss[clearance][1]"]) > 0.0 and float(a["member 1 quats.grad"].abs().max()) > 0.0


@pytest.mark.parametrize("occlusion", [None, "hpr"])
def test_model_pose(dev, occlusion):
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelPose
    pts, (p, q) = snapped_cloud(N), snapped_path(9)
    outs = []
    for t in (None, T):
        m = ModelPose(torch.from_numpy(at(pts, t)), torch.from_numpy(at(p[4:5], t)), torch.from_numpy(q[4:5].copy()), torch.from_numpy(K),
                      IW, IH, device=dev, occlusion=occlusion)
        loss = m()
        loss.backward()
        outs.append({"loss": loss.detach(), "observations": m.observations.detach(), "trans.grad": m.trans.grad, "quat.grad": m.quat.grad})
        if occlusion is not None:   # the row the model builds for itself: the same call over its unsorted pack
            outs[-1]["occlusion row"] = ops.occlusion_bits(ops.PackedCloud(m.points, sort=False), m.points, m.trans.detach(), m.quat.detach(),
                                                           _cam(ops), 1.0, 15.0, occlusion)
    assert_same(outs[0], outs[1], f"ModelPose occlusion={occlusion}")
    assert float(outs[0]["observations"].sum()) > 1.0 and float(outs[0]["trans.grad"].abs().max()) > 0.0


def _clearance_outputs(dev, cloud, q, segs, walk, r, w=1.5):
    """Every output of the three queries: q (nq,3) positions, segs (E,2,3) unrelated segments, walk (W,3) one path."""
    from trajectory_optimization_amd import ops
    E = len(segs)
    qt, st, wt = _t(q, dev), _t(segs.reshape(-1, 3), dev), _t(walk, dev)
    out = {}
    g = torch.empty((len(q), 3), dtype=torch.float32, device=dev)
    terms = ops.clearance_terms(len(q), 1, "waypoints", dev)
    out["points d"], out["points idx"], out["points value"] = ops.clearance(cloud, qt, r, w, grad=g, want_value=True, terms=terms)
    out["points grad"], out["points terms"] = g, terms[:len(q)].clone()
    g2 = torch.empty((2 * E, 3), dtype=torch.float32, device=dev)
    out["segments d"], out["segments idx"], out["segments s"], out["segments value"] = ops.clearance_segments(cloud, st, r, w, n_traj=E, grad=g2,
                                                                                                          want_value=True)
    out["segments grad"] = g2
    g3 = torch.empty((len(walk), 3), dtype=torch.float32, device=dev)
    out["walk d"], out["walk idx"], out["walk s"], out["walk value"] = ops.clearance_segments(cloud, wt, r, w, grad=g3, want_value=True)
    out["walk grad"] = g3
    out["edges d"], out["edges idx"], out["edges s"] = ops.clearance_edges(cloud, st[0::2].contiguous(), st[1::2].contiguous(), r)
    return out


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("n", [N, N_BIG])
def test_clearance_queries(dev, n, sort):
    from trajectory_optimization_amd import ops
    pts = snapped_cloud(n, 5)
    r = 1.0 if n == N else 0.5
    q, segs, walk = queries(pts, 1), segments(pts, 2), snapped_path(9)[0]
    outs = []
    for t in (None, T):
        cloud = ops.PackedCloud(_t(at(pts, t), dev), sort=sort)
        outs.append(_clearance_outputs(dev, cloud, at(q, t), at(segs.reshape(-1, 3), t).reshape(-1, 2, 3), at(walk, t), r))
    assert_same(outs[0], outs[1], f"clearance n={n} sort={sort}")
    a = outs[0]
    for k in ("points", "segments", "edges", "walk"):
        idx = a[f"{k} idx"]
        assert int((idx >= 0).sum()) >= idx.numel() // 3, k
    assert int(a["points idx"][-1]) == -1 and int(a["segments idx"][-1]) == -1 and float(a["segments s"][-2]) == 0.0   # far; zero length
    assert torch.equal(a["edges idx"], a["segments idx"]) and torch.equal(_bits(a["edges d"]), _bits(a["segments d"]))
    assert float(a["points grad"].abs().max()) > 0.0 and float(a["walk grad"].abs().max()) > 0.0 and float(a["points d"][44:46].max()) == 0.0


def test_select_views(dev):
    from trajectory_optimization_amd import tools
    pts = snapped_cloud(N)
    cp, cq = synth.candidate_grid(np.linspace(-15, 15, 4), np.linspace(-15, 15, 4), 0.0, 2)
    cp = snap(cp)
    outs = []
    for t in (None, T):
        sel = tools.select_views(_t(at(pts, t), dev), torch.from_numpy(at(cp, t)), torch.from_numpy(cq), 4, intrins=torch.from_numpy(K),
                                 img_width=IW, img_height=IH, prior_log_odds=_t(_prior_row(N), dev))
        outs.append({"order": sel.order, "gain_fixed": sel.gain_fixed, "coverage_log_odds": sel.coverage_log_odds, "nnz": sel.nnz,
                     "rewards": sel.rewards, "absent": sel.absent})
    assert_same(outs[0], outs[1], "select_views")
    assert outs[0]["order"].numel() == 4 and int(outs[0]["gain_fixed"].min()) > 0 and outs[0]["nnz"] > 1000


@pytest.mark.parametrize("closed", [False, True])
def test_plan_tour(dev, closed):
    from trajectory_optimization_amd import tools
    pts, P, r = walled_scene()
    outs = []
    for t in (None, T):
        tour = tools.plan_tour(_t(at(pts, t), dev), torch.from_numpy(at(P, t)), clearance_radius=r, closed=closed)
        outs.append({"walk": tour.walk, "blocked": tour.blocked, "D": tour.D, "nxt": tour.nxt, "length_fixed": tour.length_fixed,
                     "order": tour.order, "unreachable": tour.unreachable, "edge_distance": tour.edge_distance, "moves": tour.moves})
    assert_same(outs[0], outs[1], f"plan_tour closed={closed}")
    a = outs[0]
    assert bool(a["blocked"].any()) and a["walk"].count(3) == 2 and a["unreachable"].tolist() == [False] * 6 + [True]


def test_coverage_map(dev):
    from trajectory_optimization_amd import ops
    pts, other, row = snapped_cloud(N), snapped_cloud(5_000, 8), covmap_rows(N)
    outs, centres = [], []
    for t in (None, T):
        cmap = ops.CoverageMap(at(COVMAP_ORIGIN, t), COVMAP_R, clamp_max=4.0, device=dev)
        x = _t(at(pts, t), dev)
        cmap.integrate(x, _t(row, dev), "max")
        cmap.integrate(x[::3].contiguous(), _t(row[::3], dev), "add")
        c, v, k = cmap.export()
        centres.append(c)
        outs.append({"export keys": k, "export values": v, "lookup other": cmap.lookup(_t(at(other, t), dev)), "lookup own": cmap.lookup(x),
                     "n_voxels": cmap.n_voxels, "skipped": cmap.skipped})
    assert_same(outs[0], outs[1], "CoverageMap")
    assert torch.equal(_bits(centres[0] + _t(T, dev)), _bits(centres[1])), f"export centres: {_how(centres[0] + _t(T, dev), centres[1])}"
    assert outs[0]["skipped"] == (0, 0) and 1000 < outs[0]["n_voxels"] < N and float(outs[0]["lookup other"].max()) > 0.0


def test_cull_transform_and_trajectory_clearance(dev):
    from trajectory_optimization_amd import ops, tools
    pts, (p, q) = snapped_cloud(N), snapped_path(9)
    outs = []
    for t in (None, T):
        x, ps, qs = _t(at(pts, t), dev), _t(at(p, t), dev), _t(q, dev)
        kept, kpts, counts, _ = ops.cull_waypoints(x, ps, qs, _cam(ops), 1.0, 15.0)
        out = {"cull counts": counts}
        for w, c in enumerate(counts):
            out[f"cull kept_idx[{w}]"], out[f"cull kept_pts[{w}]"] = kept[w, :c].clone(), kpts[w, :c].clone()
        for norm in (True, False):
            out[f"to_camera_frame_exact normalize={norm}"] = ops.to_camera_frame_exact(x, qs[3], ps[3], normalize=norm)
        out["to_camera_frame_exact transpose"] = ops.to_camera_frame_exact(x, qs[5], ps[5], transpose=True)
        d, idx = tools.trajectory_clearance(x, ps, 1.0)
        ds, ids, ss = tools.trajectory_clearance(x, ps, 1.0, segments=True)
        out.update({"trajectory_clearance d": d, "trajectory_clearance idx": idx, "trajectory_clearance segments d": ds,
                    "trajectory_clearance segments idx": ids, "trajectory_clearance segments s": ss})
        outs.append(out)
    assert_same(outs[0], outs[1], "cull / transform / trajectory_clearance")
    assert min(outs[0]["cull counts"]) > 0 and max(outs[0]["cull counts"]) < N and int((outs[0]["trajectory_clearance idx"] >= 0).sum()) >= 3


# ================================================================================ 2. unsnapped offsets

DIRECTION = np.array([1.0, -1.0, 0.5])


def offset(a, off):
    """The raw synthetic rows plus off (1, -1, 1/2), cast to float32: these float32 rows are the input's definition."""
    return (np.asarray(a, f64) + off * DIRECTION).astype(f32)


_brute = {}


def _clearance_case(n, off):
    """(pts, q, A, B, r, point / edge / segment brute force) at one offset, computed once.  Nothing is snapped; the two queries "on a
    cloud point" are rows of the OFFSET cloud, so d == 0 is met at every offset."""
    from test_hip_clearance import brute as brute_points
    from test_hip_clearance_segments import brute as brute_segments
    from test_hip_tour import brute_edges
    key = (n, off)
    if key not in _brute:
        raw = synth.make_cloud(n, seed=5)
        r = 1.0 if n == N else 0.5
        segs = segments(raw, 2, snapped=False)
        pts, q, A, B = offset(raw, off), offset(queries(raw, 1, snapped=False), off), offset(segs[:, 0], off), offset(segs[:, 1], off)
        q[44:46] = pts[[n // 3, n // 2]]
        ends = np.stack([A, B], axis=1).reshape(-1, 3)
        _brute[key] = (pts, q, A, B, r, brute_points(pts, q, r), brute_edges(pts, A, B, r), brute_segments(pts, ends, r, n_traj=len(A)))
    return _brute[key]


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("off", [1e3, 1e5, 1e6])
@pytest.mark.parametrize("n", [N, N_BIG])
def test_unsnapped_clearance_equals_brute_force(dev, n, off, sort):
    """1e6 (float32 spacing 0.06 m) is there because the 1e-5 amax slack terms turned out not to be what keeps these queries right:
    see DESIGN.md's parity section."""
    from trajectory_optimization_amd import ops
    pts, q, A, B, r, (d_ref, i_ref), (de_ref, ie_ref, se_ref), (ds_ref, is_ref, ss_ref, _) = _clearance_case(n, off)
    cloud = ops.PackedCloud(_t(pts, dev), sort=sort)
    d, idx = ops.clearance(cloud, _t(q, dev), r)
    a, b = _t(A, dev), _t(B, dev)
    seg = ops.clearance_segments(cloud, torch.stack([a, b], dim=1).reshape(-1, 3), r, n_traj=len(A))
    edge = ops.clearance_edges(cloud, a, b, r)
    what = f"n={n} offset={off:g} sort={sort}"
    assert np.array_equal(idx.cpu().numpy(), i_ref), f"{what}: points idx"
    assert np.array_equal(d.cpu().numpy().view(np.uint32), d_ref.view(np.uint32)), f"{what}: points d"
    for name, got in (("segments", seg), ("edges", edge)):
        assert np.array_equal(got[1].cpu().numpy(), ie_ref), f"{what}: {name} idx"
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), de_ref.view(np.uint32)), f"{what}: {name} d"
        assert np.array_equal(got[2].cpu().numpy().view(np.uint32), se_ref.view(np.uint32)), f"{what}: {name} s"
    # the segment query's own brute force (tests/test_hip_clearance_segments.py) states d and idx as brute_edges does and s in f64 with
    # another summation order: its home test's bound for s, 1e-6, holds here too
    assert np.array_equal(seg[1].cpu().numpy(), is_ref), f"{what}: segments idx (segment brute force)"
    assert np.array_equal(seg[0].cpu().numpy().view(np.uint32), ds_ref.view(np.uint32)), f"{what}: segments d (segment brute force)"
    assert np.abs(seg[2].cpu().numpy() - ss_ref).max() <= 1e-6, f"{what}: segments s (segment brute force)"
    assert int((i_ref >= 0).sum()) >= len(q) // 3 and int((ie_ref >= 0).sum()) >= len(A) // 3 and i_ref[-1] == -1 and ie_ref[-1] == -1
    assert float(d_ref[44:46].max()) == 0.0 and i_ref[44] <= n // 3 and i_ref[45] <= n // 2   # on a cloud point (or a copy of it in a lower row)


def _prune_edge_queries(pts, perm, r, tiles):
    """The queries a sphere prune is most likely to get wrong, for the given tiles of a pack (256 consecutive packed rows each): with c
    the tile's box centre as k_pack_cloud takes it and x* its farthest point from c (the one that sets the sphere's radius R), the
    positions t = x* + f r u, u = (x* - c) / R, for f just below 1, 0.9 and 0.5 — c, x* and t are collinear, so |t - c| = R + f r with
    nothing to spare but the prune's slack whenever x* is t's nearest point — and per position two segments: one that starts at t and
    leads away (nearest point beyond its first end) and one through t across u (nearest point beside its interior).
    -> (q (3k,3), A (6k,3), B (6k,3), target (3k,) the row of x*), float32 / int."""
    q, A, B, target = [], [], [], []
    for k in tiles:
        rows = perm[256 * k:256 * (k + 1)]
        rows = rows[rows >= 0]
        if len(rows) == 0:   # (a tile of pads only)
            continue
        x = pts[rows]
        c = (f32(0.5) * (x.min(axis=0) + x.max(axis=0))).astype(f64)
        dist = np.linalg.norm(x.astype(f64) - c, axis=1)
        j = int(np.argmax(dist))
        if not dist[j] > 0:
            continue
        u = (x[j].astype(f64) - c) / dist[j]
        w = np.cross(u, [0.0, 0.0, 1.0]) if abs(u[2]) < 0.9 else np.cross(u, [0.0, 1.0, 0.0])
        w /= np.linalg.norm(w)
        for frac in (1.0 - 1e-6, 0.9, 0.5):
            t = x[j].astype(f64) + frac * r * u
            q.append(t), target.append(int(rows[j]))
            A.extend([t, t - r * w]), B.extend([t + 2.0 * r * u, t + r * w])
    return np.asarray(q, f32), np.asarray(A, f32), np.asarray(B, f32), np.asarray(target)


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("off", [0.0, 1e3, 1e5, 1e6])
@pytest.mark.parametrize("n", [N, N_BIG])
def test_unsnapped_clearance_at_the_prunes_edge(dev, n, off, sort):
    """Random queries rarely meet a prune's edge: a prune 2 % too tight passes test_unsnapped_clearance_equals_brute_force.  These
    are aimed at it (every tile at 20 000 points, every 18th at 300 000), and the brute force decides what the answer is."""
    from test_hip_clearance import brute as brute_points
    from test_hip_tour import brute_edges
    from trajectory_optimization_amd import ops
    pts = offset(synth.make_cloud(n, seed=5), off)
    r = 1.0 if n == N else 0.5
    cloud = ops.PackedCloud(_t(pts, dev), sort=sort)
    tiles = range(cloud.npad // 256) if n == N else range(0, cloud.npad // 256, 18)
    q, A, B, target = _prune_edge_queries(pts, cloud.perm.cpu().numpy(), r, tiles)
    d_ref, i_ref = brute_points(pts, q, r)
    de_ref, ie_ref, se_ref = brute_edges(pts, A, B, r)
    d, idx = ops.clearance(cloud, _t(q, dev), r)
    a, b = _t(A, dev), _t(B, dev)
    seg = ops.clearance_segments(cloud, torch.stack([a, b], dim=1).reshape(-1, 3), r, n_traj=len(A))
    edge = ops.clearance_edges(cloud, a, b, r)
    what = f"n={n} offset={off:g} sort={sort}"
    hits, hits_seg = int((i_ref == target).sum()), int((ie_ref == np.repeat(target, 2)).sum())
    print(f"{what}: {len(q)} positions, x* is the answer of {hits} of them and of {hits_seg} of {len(A)} segments")
    assert np.array_equal(idx.cpu().numpy(), i_ref), f"{what}: points idx"
    assert np.array_equal(d.cpu().numpy().view(np.uint32), d_ref.view(np.uint32)), f"{what}: points d"
    for name, got in (("segments", seg), ("edges", edge)):
        assert np.array_equal(got[1].cpu().numpy(), ie_ref), f"{what}: {name} idx"
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), de_ref.view(np.uint32)), f"{what}: {name} d"
        assert np.array_equal(got[2].cpu().numpy().view(np.uint32), se_ref.view(np.uint32)), f"{what}: {name} s"
    # the aim holds: for some of them the tile's own farthest point is the answer, i.e. the prune had only its slack to spare
    assert hits >= 4 and hits_seg >= 4, what


@pytest.mark.parametrize("off", [1e3, 1e5])
def test_unsnapped_culled_equals_dense(dev, off):
    from trajectory_optimization_amd import ops
    p, q = synth.make_path(16, optical=True, jitter_seed=3)
    cloud, cam = ops.PackedCloud(_t(offset(synth.make_cloud(N, seed=3), off), dev)), _cam(ops)
    ps, qs, gout = _t(offset(p, off), dev), _t(q, dev), torch.ones(1, dtype=torch.float32, device=dev)
    names = ("rewards", "scalars", "poses_grad", "quats_grad", "lo_sum", "minmax")
    outs = [dict(zip(names, ops.traj_forward_backward(cloud, ps, qs, cam, ops.TrajWorkspace(cloud, 16), gout, flags=flags)))
            for flags in (0, ops.DENSE)]
    assert_same(outs[0], outs[1], f"culled against dense, offset {off:g}")
    assert int((outs[0]["rewards"] > 0.5).sum()) > 100 and not bool(torch.isnan(outs[0]["rewards"]).any())


GRAD_TOL = 1e-5   # tests/test_hip_conditioning.py's bar, under its condition


@pytest.mark.parametrize("off", [0.0, 1e3, 1e5])
def test_unsnapped_model_traj_against_the_f64_oracle(dev, off):
    """The project's own bars at an offset (0 is there for the side-by-side): rewards rtol 1e-5, loss['vis'] 5e-6 relative, gradients
    1e-5 of the largest row on every waypoint whose nearest point keeps MARGIN from both thresholds of the clipped log-odds.  The f32
    oracle's own distance from f64 goes into every message: what float32 arithmetic on x - t can give at that offset."""
    from oracle import oracle
    from test_hip_conditioning import MARGIN, _margins
    from trajectory_optimization_amd.model import ModelTraj
    W = 20
    pts = offset(synth.make_cloud(N, seed=3), off)
    p, q = synth.make_path(W, optical=True, jitter_seed=3)
    p = offset(p, off)
    m = ModelTraj(torch.from_numpy(pts), torch.from_numpy(p), torch.from_numpy(q), torch.from_numpy(K), IW, IH, device=dev)
    m(vis_wps_dist=0.0)
    m.loss["vis"].backward()
    f = oracle.traj_forward(pts, p, q, K, IW, IH, prec="f64")
    pg, qg = oracle.traj_backward(pts, p, q, K, IW, IH, f, prec="f64")
    f1 = oracle.traj_forward(pts, p, q, K, IW, IH, prec="f32")
    pg1, qg1 = oracle.traj_backward(pts, p, q, K, IW, IH, f1, prec="f32")
    rew = m.rewards.detach().cpu().numpy()
    rel = lambda a: float(np.abs(a.astype(f64) - f["rewards"]).max() / np.abs(f["rewards"]).max())
    dp, dq = np.abs(pg).max(), np.abs(qg).max()
    assert dp > 0 and dq > 0
    row = lambda g, ref, den: np.abs(np.asarray(g, f64) - ref).max(axis=1) / den
    ep, eq = row(m.poses.grad.cpu().numpy(), pg, dp), row(m.quats.grad.cpu().numpy(), qg, dq)
    ep1, eq1 = row(pg1, pg, dp), row(qg1, qg, dq)
    keep = _margins(pts, p, q, (1.0, 5.0)) > MARGIN
    vis, vis1 = abs(m.loss["vis"].item() - f["loss_vis"]) / f["loss_vis"], abs(f1["loss_vis"] - f["loss_vis"]) / f["loss_vis"]
    report = (f"offset {off:g}: distance from the f64 oracle, kernel | f32 oracle: rewards {rel(rew):.2e} | {rel(f1['rewards']):.2e}, "
              f"loss_vis {vis:.2e} | {vis1:.2e}, poses_grad {ep[keep].max():.2e} | {ep1[keep].max():.2e}, "
              f"quats_grad {eq[keep].max():.2e} | {eq1[keep].max():.2e}, {int((~keep).sum())} of {W} waypoints excluded")
    print(report)
    assert int((~keep).sum()) <= W // 20, report
    assert vis <= 5e-6, report
    np.testing.assert_allclose(rew, f["rewards"], rtol=1e-5, atol=0, err_msg=report)
    assert (ep[keep] < GRAD_TOL).all() and (eq[keep] < GRAD_TOL).all(), report


@pytest.mark.parametrize("off", [0.0, 1e3, 1e5])
def test_unsnapped_model_pose_against_the_f64_oracle(dev, off):
    """ModelPose's existing bars (tests/test_hip_pose_occlusion.py::test_values_against_the_oracle): the loss 1e-5 relative, the
    observations rtol 5e-5 (atol 1e-9), both gradients 1e-5 of their largest entry."""
    from conftest import rel_inf
    from oracle import oracle
    from trajectory_optimization_amd.model import ModelPose
    pts = offset(synth.make_cloud(N, seed=3), off)
    p, q = synth.make_path(9, optical=True, jitter_seed=3)
    t0, q0 = offset(p[4:5], off), np.ascontiguousarray(q[4:5])
    m = ModelPose(torch.from_numpy(pts), torch.from_numpy(t0), torch.from_numpy(q0), torch.from_numpy(K), IW, IH, device=dev)
    loss = m()
    loss.backward()
    obs, ref_loss = oracle.pose_forward(pts, t0, q0, K, IW, IH, prec="f64")
    tg, qg = oracle.pose_backward(pts, t0, q0, K, IW, IH, ref_loss, prec="f64")
    obs1, loss1 = oracle.pose_forward(pts, t0, q0, K, IW, IH, prec="f32")
    tg1, qg1 = oracle.pose_backward(pts, t0, q0, K, IW, IH, loss1, prec="f32")
    e = (abs(loss.item() - ref_loss) / ref_loss, rel_inf(m.trans.grad.cpu().numpy(), tg), rel_inf(m.quat.grad.cpu().numpy(), qg))
    e1 = (abs(loss1 - ref_loss) / ref_loss, rel_inf(tg1, tg), rel_inf(qg1, qg))
    report = (f"offset {off:g}: distance from the f64 oracle, kernel | f32 oracle: loss {e[0]:.2e} | {e1[0]:.2e}, trans grad {e[1]:.2e} | "
              f"{e1[1]:.2e}, quat grad {e[2]:.2e} | {e1[2]:.2e}")
    print(report)
    assert obs.sum() > 1.0
    assert e[0] <= 1e-5 and e[1] < 1e-5 and e[2] < 1e-5, report
    np.testing.assert_allclose(m.observations.detach().cpu().numpy(), obs, rtol=5e-5, atol=1e-9, err_msg=report)


@pytest.mark.parametrize("leaf", [0.5, (0.3, 0.7, 0.2)])
@pytest.mark.parametrize("off", [1e3, 1e5])
def test_unsnapped_voxel_grid_against_the_oracle(dev, off, leaf):
    """Not invariant by definition (the module docstring): the cell index and the centroid sum take the absolute coordinate.  So the
    check is the definition itself at the offset: oracle/ingest_oracle.py's float32 restatement, same voxels in the same order,
    centroids bit for bit — without a pass-through filter and with one on z around the offset slab.  (At 1e5 a float32 step is
    0.008 m, a twenty-fifth of the smallest leaf.  tests/test_hip_ingest_layouts.py holds the same at -5e3 m.)"""
    from test_hip_ingest_layouts import voxel_vs_oracle
    pts = offset(synth.make_cloud(N, seed=3), off)
    out = voxel_vs_oracle(dev, pts, leaf, None)
    assert 1000 < len(out) < N and np.isfinite(out).all()
    z0 = 0.5 * off
    cut = voxel_vs_oracle(dev, pts, leaf, 2, z0 - 1.0, z0 + 0.5)
    assert 100 < len(cut) < len(out) and bool(((cut[:, 2] >= z0 - 1.0) & (cut[:, 2] <= z0 + 0.5)).all())


@pytest.mark.parametrize("off", [1e3, 1e5])
def test_unsnapped_world_frame_hpr_against_qhull(dev, off):
    """Not invariant by definition (the module docstring): the viewpoint is the world origin, so a far cloud is a cloud seen from far
    away.  The check is the definition at the offset: the index set of scipy's Qhull on the oracle's flipped points
    (tests/test_hip_hpr.py's reference), and ModelPose.forward(hpr=True) with that mask against the f64 oracle under ModelPose's
    bars."""
    from conftest import rel_inf
    from oracle import oracle
    from trajectory_optimization_amd import ops
    from trajectory_optimization_amd.model import ModelPose
    pts = offset(synth.make_cloud(N, seed=3), off)
    vis_ref, mask_ref = oracle.hidden_pts_removal(pts)
    idx, mask = ops.hidden_pts_removal(_t(pts, dev))
    print(f"offset {off:g}: {len(vis_ref)} of {N} points visible from the world origin")
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), vis_ref), f"offset {off:g}: visible index set"
    assert np.array_equal(mask.cpu().numpy().astype(f32).reshape(-1), mask_ref), f"offset {off:g}: mask"
    assert 4 <= len(vis_ref) < N
    if off > 1e3:   # the 78 points visible from 1.5e5 m away carry 1e-14 of observation at this pose: the loss is 1 / eps and the f32
        return      # oracle's own gradient sits 4e-6 from f64 (measured on the CPU oracle alone) — no bar of ModelPose's applies
    p, q = synth.make_path(9, optical=True, jitter_seed=3)
    t0, q0 = offset(p[4:5], off), np.ascontiguousarray(q[4:5])
    m = ModelPose(torch.from_numpy(pts), torch.from_numpy(t0), torch.from_numpy(q0), torch.from_numpy(K), IW, IH, device=dev)
    loss = m(hpr=True)
    loss.backward()
    obs, ref_loss = oracle.pose_forward(pts, t0, q0, K, IW, IH, mask=mask_ref, prec="f64")
    tg, qg = oracle.pose_backward(pts, t0, q0, K, IW, IH, ref_loss, mask=mask_ref, prec="f64")
    e = (abs(loss.item() - ref_loss) / ref_loss, rel_inf(m.trans.grad.cpu().numpy(), tg), rel_inf(m.quat.grad.cpu().numpy(), qg))
    report = f"offset {off:g}: ModelPose(hpr=True) from the f64 oracle: loss {e[0]:.2e}, trans grad {e[1]:.2e}, quat grad {e[2]:.2e}"
    print(report)
    assert obs.sum() > 1.0
    assert e[0] <= 1e-5 and e[1] < 1e-5 and e[2] < 1e-5, report
    np.testing.assert_allclose(m.observations.detach().cpu().numpy(), obs, rtol=5e-5, atol=1e-9, err_msg=report)


# ================================================================================ 3. degenerate boxes for the Morton pack

def _degenerate(name):
    """-> (points (N,3) f32, scale: what r, the clip distances and the path are multiplied by)."""
    slab = synth.make_cloud(N, seed=3)
    rng = np.random.default_rng(29)
    if name == "outlier":      # the box's longest side is 1e6 m: a Morton cell is about 1 km, every other point falls into cell 0
        slab[N // 2] = (1e6, 1e6, 1e6)
        return slab, 1.0
    if name == "planar":
        slab[:, 2] = f32(0.375)
        return slab, 1.0
    if name == "collinear":
        s = rng.uniform(-20, 20, N)
        return np.stack([s, 0.25 * s + 0.5, np.full(N, 0.375)], axis=1).astype(f32), 1.0
    if name == "identical":    # all rows the same point but one
        pts = np.tile(f32([[3.0, 0.5, 0.25]]), (N, 1))
        pts[N // 3] = (4.0, -0.5, 0.0)
        return pts, 1.0
    scale = {"millimetres": 1e-3, "kilometres": 1e3}[name]
    return (slab * f32(scale)).astype(f32), scale


@pytest.mark.parametrize("name", ["outlier", "planar", "collinear", "identical", "millimetres", "kilometres"])
def test_degenerate_boxes(dev, name):
    from test_hip_clearance import brute as brute_points
    from test_hip_tour import brute_edges
    from trajectory_optimization_amd import ops
    pts, scale = _degenerate(name)
    x = _t(pts, dev)
    cloud = ops.PackedCloud(x, sort=True)
    # the pack: a permutation, and the SoA rows are the caller's rows in that order
    perm = cloud.perm[:N].long()
    assert sorted(perm.tolist()) == list(range(N)), "perm is not a permutation"
    assert bool((cloud.perm[N:] == -1).all()), "perm pads"
    for k in range(3):
        assert torch.equal(cloud.soa[k * cloud.npad:k * cloud.npad + N], x[perm, k]), f"soa row {k}"
    assert torch.equal(cloud.inv_perm.long()[perm], torch.arange(N, device=dev)), "inv_perm"
    # the queries: at cloud points, half a radius off them, in the bulk's box and far away; consecutive ones make the segments
    rng = np.random.default_rng(31)
    r = 1.0 * scale
    lo, hi = np.percentile(pts.astype(f64), [1, 99], axis=0)
    at_pts = pts[rng.integers(0, N, 8)].astype(f64)
    dirs = rng.standard_normal((8, 3))
    q = np.concatenate([at_pts[:2], at_pts + 0.5 * r * dirs / np.linalg.norm(dirs, axis=1, keepdims=True), rng.uniform(lo, hi, (6, 3)),
                        hi[None, :] + 50.0 * scale]).astype(f32)
    q = np.concatenate([q, q[-1:]])   # (the last segment has zero length, far away)
    d_ref, i_ref = brute_points(pts, q, r)
    de_ref, ie_ref, se_ref = brute_edges(pts, q[:-1], q[1:], r)
    d, idx = ops.clearance(cloud, _t(q, dev), r)
    ds, ids, ss = ops.clearance_segments(cloud, _t(q, dev), r)
    assert np.array_equal(idx.cpu().numpy(), i_ref), "points idx"
    assert np.array_equal(d.cpu().numpy().view(np.uint32), d_ref.view(np.uint32)), "points d"
    assert np.array_equal(ids.cpu().numpy(), ie_ref), "segments idx"
    assert np.array_equal(ds.cpu().numpy().view(np.uint32), de_ref.view(np.uint32)), "segments d"
    assert np.array_equal(ss.cpu().numpy().view(np.uint32), se_ref.view(np.uint32)), "segments s"
    assert int((i_ref >= 0).sum()) >= 8 and i_ref[-1] == -1 and int((ie_ref >= 0).sum()) >= 8
    assert not bool(torch.isnan(d).any()) and not bool(torch.isnan(ds).any()) and not bool(torch.isnan(ss).any())
    # culled equals dense; every waypoint sees some of the cloud, so nothing is NaN
    W = 16
    p, qs = synth.make_path(W, optical=True, jitter_seed=3, scale=(0.1 if name == "identical" else 1.0) * scale)
    cam = _cam(ops, (1.0 * scale, 5.0 * scale))
    ps, qt, gout = _t(p, dev), _t(qs, dev), torch.ones(1, dtype=torch.float32, device=dev)
    names = ("rewards", "scalars", "poses_grad", "quats_grad", "lo_sum", "minmax")
    outs = [dict(zip(names, ops.traj_forward_backward(cloud, ps, qt, cam, ops.TrajWorkspace(cloud, W), gout, flags=flags)))
            for flags in (0, ops.DENSE)]
    assert_same(outs[0], outs[1], f"{name}: culled against dense")
    for k in names:
        v = outs[0][k] if k != "lo_sum" else outs[0][k][:N]
        assert not bool(torch.isnan(v).any()), f"{name}: NaN in {k}"
    assert int((outs[0]["rewards"] > 0.5).sum()) >= 1
