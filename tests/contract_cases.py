"""One table of small cases for tests/test_hip_contracts.py: every op of the package once, at the smallest shapes that have a tail.

A case is a name, `inputs` (a dict of host arrays), `decoys` (the same keys, shapes and dtypes from another seed: different VALID
values, never garbage), `run(d) -> {name: output}` over the device copies `d` of the inputs — it builds whatever objects it needs
from them, grid -> field -> travel field -> lookups — and optionally `undefined`, {output: (index, the line that declares the region
unspecified)}, and `loose`, {output: (rtol, atol, the float atomic responsible and the file:line of the bar used)}.  Both are empty
for every case today: outputs whose documentation leaves a tail unspecified (the pads of a packed-order row, "first N valid",
ops.py:175; the rows past counts[w] of a cull, ops.py:3132) are returned cut to their defined part instead.

Shapes: clouds of 2049 + 37 points (two 2048-point tiles, the second almost empty, no multiple of 32 or 256) and of 1 point; 5
waypoints (no multiple of 4) and 1; grids (37, 5, 20), (13, 10, 7) (no multiple of the 4 x 4 x 2 brick or the 8^3 tile) and (1, 1, 1);
259 and 1 query rows; 17 x 9 depth images; 33 views; 3 team members; 3 travel fields; a cloud with exact duplicate rows for the hull.

Objects with host read-backs in the middle of their build (travel, components, covmap, hull) head cases of their own, so that the
side-stream run's ordering guarantee — which holds up to a case's first host synchronisation — covers the start of each build.

NOT_DRIVEN lists the stream-taking entry points no case calls, each with its reason; tests/test_hip_contracts.py asserts that it
equals what a recording proxy of the library finds, that it holds at most 20 names and none of the map layer."""
import ctypes

import numpy as np
import torch

import travel_cases as tc
from trajectory_optimization_amd import synth

f32 = np.float32
N = 2049 + 37
W5 = 5
K, IW, IH = synth.K_INTRINS, synth.IMG_WIDTH, synth.IMG_HEIGHT
ORIGIN, RES = tc.ORIGIN, tc.RES
GRID_A, GRID_B, GRID_1 = (37, 5, 20), (13, 10, 7), (1, 1, 1)
CLOUD_EXTENT = (24.0, 10.0, 4.0)   # denser than synth.make_cloud's default slab: every waypoint of the path sees some of 2086 points

NOT_DRIVEN = {
    "tohip_selftest_wave_reduce": "a self-test of the wave reduction, not an op (tests/test_hip_edges.py runs it)",
}

CASES = []


class Case:
    def __init__(self, name, make, run, undefined=None, loose=None):
        self.name, self._make, self.run = name, make, run
        self.undefined, self.loose = undefined or {}, loose or {}
        self._inputs = self._decoys = None

    @property
    def inputs(self):
        if self._inputs is None:
            self._inputs = self._make(0)
        return self._inputs

    @property
    def decoys(self):
        if self._decoys is None:
            self._decoys = self._make(1)
            assert self._decoys.keys() == self.inputs.keys()
            for k, v in self.inputs.items():
                w = self._decoys[k]
                assert v.shape == w.shape and v.dtype == w.dtype, k
                assert v.size == 0 or not np.array_equal(v, w, equal_nan=v.dtype.kind == "f"), f"{self.name}: decoy {k} equals the input"
        return self._decoys


def case(name, make, **kw):
    def deco(run):
        CASES.append(Case(name, make, run, **kw))
        return run
    return deco


# ---- helpers ---------------------------------------------------------------------------------------------------------------------

def _ops():
    from trajectory_optimization_amd import ops
    return ops


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


def _cam(clip=(1.0, 5.0)):
    return _ops().Camera(K, IW, IH, clip[0], clip[1])


def flat(out, prefix, obj):
    """Flatten tensors, numbers, lists / tuples / dicts and the tools' result objects into `out` under dotted names."""
    if obj is None:
        return out
    if torch.is_tensor(obj) or isinstance(obj, (int, float, bool, str, np.ndarray)):
        out[prefix] = obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            flat(out, f"{prefix}.{k}", v)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            flat(out, f"{prefix}[{i}]", v)
    else:
        names = [s for c in type(obj).__mro__ for s in getattr(c, "__slots__", ())]
        for k in names:
            if hasattr(obj, k):
                v = getattr(obj, k)
                if torch.is_tensor(v) or isinstance(v, (int, float, bool, list, tuple, np.ndarray)) or type(v).__name__ in _RESULTS:
                    flat(out, f"{prefix}.{k}", v)
    return out


_RESULTS = {"Tour", "Roadmap", "RoadmapRoutes", "PlannedPath", "RefinedPath", "ViewProposals", "ViewSelection", "VolumeSelection", "TravelMatrix",
            "FrontierAssignment", "FrontierClusters", "TravelPath", "RayHits", "DepthScan"}


def _yaw_quats(deg):
    h = np.deg2rad(np.asarray(deg, dtype=np.float64)) / 2.0
    return np.stack([synth.quat_mul(np.array([np.cos(a), 0.0, 0.0, np.sin(a)]), synth.Q_OPTICAL) for a in h]).astype(f32)


def cloud_path(seed, n=N, W=W5):
    """A cloud of n points and a path of W waypoints through it; the seed moves the points, the waypoints and their headings."""
    rng = np.random.default_rng(100 + seed)
    pts = synth.make_cloud(n, seed=10 + seed, extent=CLOUD_EXTENT)
    p, q = synth.make_path(W, optical=True, jitter_seed=3 + seed)
    p = (p + rng.uniform(-0.4, 0.4, p.shape)).astype(f32)
    return dict(points=pts, poses=p, quats=q.astype(f32))


def cloud_path_prior(seed, n=N, W=W5):
    d = cloud_path(seed, n, W)
    rng = np.random.default_rng(200 + seed)
    row = (rng.random(n) * 2.0).astype(f32)
    row[rng.random(n) < 0.3] = 0.0
    d["prior"] = row
    return d


def _traj_outputs(d, flags=0, prior=False):
    ops = _ops()
    cloud, cam = ops.PackedCloud(d["points"]), _cam()
    ps, qs = d["poses"], d["quats"]
    W = ps.shape[0]
    pr = ops.LogOddsPrior(cloud, d["prior"]) if prior else None
    gout = torch.ones(1, dtype=torch.float32, device=cloud.device)
    out = {}
    ws = ops.TrajWorkspace(cloud, W)
    lo, mm = ops.traj_forward(cloud, ps, qs, cam, ws, flags=flags)
    out["lo_sum"], out["minmax"] = lo[:cloud.n].clone(), mm
    r, s = ops.traj_reward(cloud, lo, cam, ws, prior=pr)
    out["reward.rewards"], out["reward.scalars"] = r, s
    pg, qg = ops.traj_backward(cloud, W, cam, ws, lo, scalars=s, gout=gout, flags=flags, prior=pr)
    out["backward.poses_grad"], out["backward.quats_grad"] = pg, qg
    r2, s2, pg2, qg2 = ops.traj_reward_backward(cloud, W, cam, ws, lo, gout, flags=flags, prior=pr)
    out.update({"rb.rewards": r2, "rb.scalars": s2, "rb.poses_grad": pg2, "rb.quats_grad": qg2})
    out["coverage"] = ops.traj_coverage(cloud, lo, pr, clamp_max=3.0)
    flat(out, "stats", {k: v for k, v in ops.traj_step_stats(cloud, ws).items() if k != "flagged_fraction"})
    if not prior:
        ws2 = ops.TrajWorkspace(cloud, W)
        r3, s3, pg3, qg3, lo3, mm3 = ops.traj_forward_backward(cloud, ps, qs, cam, ws2, gout, flags=flags)
        out.update({"fb.rewards": r3, "fb.scalars": s3, "fb.poses_grad": pg3, "fb.quats_grad": qg3, "fb.lo_sum": lo3[:cloud.n].clone(), "fb.minmax": mm3})
        half = torch.empty(cloud.n, dtype=torch.float32, device=cloud.device)
        ws3 = ops.TrajWorkspace(cloud, W)
        lo4, _ = ops.traj_forward(cloud, ps, qs, cam, ws3, flags=flags, rewards_half=half)
        r4, s4 = ops.traj_reward(cloud, lo4, cam, ws3, rewards=half, prefilled=True)
        out["prefilled.rewards"], out["prefilled.scalars"] = r4, s4
    return out


# ================================================================================ cloud and trajectory

@case("packed_cloud", lambda seed: {"points": synth.make_cloud(N, seed=20 + seed, extent=CLOUD_EXTENT)})
def _packed_cloud(d):
    ops = _ops()
    out = {}
    for sort in (True, False):
        c = ops.PackedCloud(d["points"], sort=sort)
        out[f"perm sort={sort}"], out[f"inv_perm sort={sort}"] = c.perm[:c.n].clone(), c.inv_perm.clone()
        for k in range(3):
            out[f"soa[{k}] sort={sort}"] = c.soa[k * c.npad:k * c.npad + c.n].clone()
        inv = torch.empty(c.n, dtype=torch.int32, device=c.device)
        _ok(_L().tohip_inverse_permutation(_p(c.blob), c.n, _p(inv), _s()), "inverse_permutation")
        out[f"inverse_permutation sort={sort}"] = inv
    return out


@case("packed_cloud_of_one_point", lambda seed: {"points": synth.make_cloud(1, seed=30 + seed, extent=CLOUD_EXTENT)})
def _packed_cloud_1(d):
    ops = _ops()
    c = ops.PackedCloud(d["points"])
    return {"perm": c.perm[:1].clone(), "inv_perm": c.inv_perm.clone(), "soa": torch.stack([c.soa[k * c.npad] for k in range(3)])}


@case("traj_plain", cloud_path)
def _traj_plain(d):
    return _traj_outputs(d)


@case("traj_dense", cloud_path)
def _traj_dense(d):
    return _traj_outputs(d, flags=_ops().DENSE)


@case("traj_prior", cloud_path_prior)
def _traj_prior(d):
    return _traj_outputs(d, prior=True)


@case("traj_one_waypoint_one_point", lambda seed: cloud_path(seed, n=1, W=1))
def _traj_1(d):
    ops = _ops()
    cloud, cam = ops.PackedCloud(d["points"]), _cam()
    gout = torch.ones(1, dtype=torch.float32, device=cloud.device)
    r, s, pg, qg, lo, mm = ops.traj_forward_backward(cloud, d["poses"], d["quats"], cam, ops.TrajWorkspace(cloud, 1), gout)
    return {"rewards": r, "scalars": s, "poses_grad": pg, "quats_grad": qg, "lo_sum": lo[:1].clone(), "minmax": mm}


@case("traj_single_trajectory_twins", cloud_path)
def _traj_twins(d):
    """The single-trajectory C entries ops.py does not wrap, through ctypes over buffers from torch.empty."""
    ops = _ops()
    from trajectory_optimization_amd.ops import _NULL_RIG
    L = _L()
    cloud, cam = ops.PackedCloud(d["points"]), _cam()
    dev, n, W = cloud.device, cloud.n, d["poses"].shape[0]
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
    wsb = L.tohip_traj_workspace_bytes(n, W)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    lo, mm, half = e(cloud.npad), e(W, 2), e(n)
    _ok(L.tohip_traj_forward(_p(cloud.blob), n, _p(d["poses"]), _p(d["quats"]), W, cam.ref(), _NULL_RIG, 0, None, _p(lo), _p(mm), _p(half),
                             _p(ws), wsb, _s()), "traj_forward")
    sc = e(4)
    _ok(L.tohip_traj_reward(_p(cloud.blob), _p(lo), n, cam.eps, 1, _p(half), _p(sc), _p(ws), wsb, _s()), "traj_reward")
    gout = torch.ones(1, dtype=torch.float32, device=dev)
    pg, qg = e(W, 3), e(W, 4)
    _ok(L.tohip_traj_backward(_p(cloud.blob), n, W, cam.ref(), _NULL_RIG, 0, None, _p(lo), None, _p(sc), _p(gout), _p(pg), _p(qg), _p(ws), wsb, _s()),
        "traj_backward")
    ws2 = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    lo2, mm2, r2, sc2, pg2, qg2 = e(cloud.npad), e(W, 2), e(n), e(4), e(W, 3), e(W, 4)
    _ok(L.tohip_traj_forward_backward(_p(cloud.blob), n, _p(d["poses"]), _p(d["quats"]), W, cam.ref(), _NULL_RIG, 0, None, _p(lo2), _p(mm2), _p(r2),
                                      _p(sc2), _p(gout), _p(pg2), _p(qg2), _p(ws2), wsb, _s()), "traj_forward_backward")
    # the fused reward + backward of several trajectories (here: one)
    ws3 = ops.TrajWorkspace(cloud, W, 1)
    toff = torch.zeros(2, dtype=torch.int32, device=dev)
    toff[1] = W
    lo3, _ = ops.traj_forward(cloud, d["poses"], d["quats"], cam, ws3, traj_offsets=toff)
    rb, sb, pg3, qg3 = e(1, n), e(1, 4), e(W, 3), e(W, 4)
    _ok(L.tohip_traj_reward_backward_multi(_p(cloud.blob), n, W, 1, cam.ref(), _NULL_RIG, 0, None, _p(lo3), cam.eps, 0, _p(rb), _p(sb), _p(gout),
                                           _p(pg3), _p(qg3), _p(ws3.buf), ws3.bytes, _s()), "traj_reward_backward_multi")
    return {"lo_sum": lo[:n].clone(), "minmax": mm, "rewards": half, "scalars": sc, "poses_grad": pg, "quats_grad": qg,
            "fb.lo_sum": lo2[:n].clone(), "fb.minmax": mm2, "fb.rewards": r2, "fb.scalars": sc2, "fb.poses_grad": pg2, "fb.quats_grad": qg2,
            "multi.rewards": rb, "multi.scalars": sb, "multi.poses_grad": pg3, "multi.quats_grad": qg3}


class _OneRankShard:
    """A shard of one rank that issues its (identity) collectives: WaypointShardStep's compacted all-reduce path without a process
    group."""
    kind, collective, compact, world_size, rank = "waypoints", True, True, 1, 0

    @staticmethod
    def bounds(n, rank=None):
        return 0, n

    @staticmethod
    def allreduce_sum(t):
        return t

    allreduce_max = allreduce_sum


class _OneRankPointShard(_OneRankShard):
    kind = "points"

    @staticmethod
    def point_bounds(n, rank=None):
        return 0, n


@case("point_shard_step", cloud_path)
def _pshard(d):
    ops = _ops()
    cloud, cam = ops.PackedCloud(d["points"]), _cam()
    W = d["poses"].shape[0]
    step = ops.PointShardStep(cloud, cloud.n, W, cam, ops.TrajWorkspace(cloud, W), _OneRankPointShard())
    r, s, pg, qg = step.step(d["poses"], d["quats"])
    return {"rewards": r.clone(), "scalars": s.clone(), "poses_grad": pg.clone(), "quats_grad": qg.clone()}


@case("waypoint_shard_step", cloud_path_prior)
def _wshard(d):
    ops = _ops()
    cloud, cam = ops.PackedCloud(d["points"]), _cam()
    W = d["poses"].shape[0]
    out = {}
    for name, prior in (("plain", None), ("prior", ops.LogOddsPrior(cloud, d["prior"]))):
        step = ops.WaypointShardStep(cloud, W, cam, ops.TrajWorkspace(cloud, W), _OneRankShard())
        r, s, pg, qg = step.step(d["poses"], d["quats"], prior=prior)
        out.update({f"{name}.rewards": r.clone(), f"{name}.scalars": s.clone(), f"{name}.poses_grad": pg.clone(), f"{name}.quats_grad": qg.clone()})
    return out


# ================================================================================ pose

def pose_inputs(seed):
    d = cloud_path(seed, W=3)
    rng = np.random.default_rng(300 + seed)
    d["mask"] = (rng.random(N) < 0.7).astype(f32)
    return d


@case("pose_calls", pose_inputs)
def _pose(d):
    ops = _ops()
    cloud, cam = ops.PackedCloud(d["points"], sort=False), _cam()
    ws, wsm = ops.PoseWorkspace(cloud), ops.PoseWorkspace(cloud, 3)
    t, q = d["poses"][1:2].contiguous(), d["quats"][1:2].contiguous()
    occ3 = ops.occlusion_bits(cloud, cloud.points, d["poses"], d["quats"], cam, 1.0, 15.0, "zbuffer")
    out = {"occ rows": occ3}
    one = torch.ones(1, dtype=torch.float32, device=cloud.device)
    for name, kw in (("plain", {}), ("mask", dict(mask=d["mask"])), ("bits", dict(occ=occ3[1:2].contiguous()))):
        obs, sc = ops.pose_forward(cloud, t, q, cam, ws, **kw)
        out[f"{name}.forward.obs"], out[f"{name}.forward.scalars"] = obs, sc
        tg, qg = ops.pose_backward(cloud, t, q, cam, ws, scalars=sc, gout=one, **kw)
        out[f"{name}.backward.tg"], out[f"{name}.backward.qg"] = tg, qg
        obs2, sc2, tg2, qg2 = ops.pose_forward_backward(cloud, t, q, cam, ws, **kw)
        out.update({f"{name}.fb.obs": obs2, f"{name}.fb.scalars": sc2, f"{name}.fb.tg": tg2.clone(), f"{name}.fb.qg": qg2.clone()})
    for name, kw in (("plain", {}), ("mask", dict(mask=d["mask"])), ("bits", dict(occ=occ3))):
        obs, sc, tg, qg = ops.pose_forward_backward_multi(cloud, d["poses"], d["quats"], cam, wsm, observations=True, **kw)
        out.update({f"{name}.multi.obs": obs, f"{name}.multi.scalars": sc, f"{name}.multi.tg": tg, f"{name}.multi.qg": qg})
    _, sc, _, _ = ops.pose_forward_backward_multi(cloud, d["poses"], d["quats"], cam, wsm, grad=False)
    out["multi.forward_only.scalars"] = sc
    return out


# ================================================================================ occlusion, culling and projection

@case("occlusion_hpr", cloud_path)
def _occ_hpr(d):
    ops = _ops()
    cloud = ops.PackedCloud(d["points"])
    return {"rows": ops.occlusion_bits(cloud, cloud.points, d["poses"], d["quats"], _cam(), 1.0, 15.0, "hpr")}


@case("occlusion_hpr_unsorted_cloud", cloud_path)
def _occ_hpr_unsorted(d):
    ops = _ops()
    cloud = ops.PackedCloud(d["points"], sort=False)
    other = d["points"].clone()   # not the cloud's own tensor: the scattered bit-by-bit path
    return {"rows": ops.occlusion_bits(cloud, other, d["poses"], d["quats"], _cam(), 1.0, 15.0, "hpr")}


@case("occlusion_zbuffer", cloud_path)
def _occ_zbuffer(d):
    ops = _ops()
    cloud = ops.PackedCloud(d["points"])
    return {"rows": ops.occlusion_bits(cloud, cloud.points, d["poses"], d["quats"], _cam(), 1.0, 15.0, "zbuffer")}


@case("occlusion_voxel_and_los_rows", cloud_path)
def _occ_voxel(d):
    ops = _ops()
    cloud = ops.PackedCloud(d["points"])
    grid = ops.OccupancyGrid.from_points(cloud, resolution=0.25)
    rows = ops.occlusion_bits(cloud, cloud.points, d["poses"], d["quats"], _cam(), 1.0, 15.0, "voxel", grid=grid)
    stats = torch.zeros(2, dtype=torch.int64, device=cloud.device)
    rows2 = ops.los_rows(cloud, d["poses"], d["quats"], _cam(), 1.0, 15.0, grid, skip=(1, 1), prune=False, stats=stats)
    # the C hosts' bit rows from kept / visible lists
    kept, _, counts, kcnt = ops.cull_waypoints(cloud.points, d["poses"][:1], d["quats"][:1], _cam(), 1.0, 15.0)
    vis = torch.arange(max(counts[0], 1), dtype=torch.int32, device=cloud.device)
    vc = torch.tensor([counts[0] // 2], dtype=torch.int32, device=cloud.device)
    row = torch.empty(cloud.npad // 32, dtype=torch.int32, device=cloud.device)
    _ok(_L().tohip_occlusion_row(cloud.n, _p(cloud.inv_perm), _p(kept[0]), _p(kcnt), _p(vis), _p(vc), _p(row), _s()), "occlusion_row")
    rows1 = torch.empty((1, cloud.npad // 32), dtype=torch.int32, device=cloud.device)
    voff = torch.tensor([0, counts[0] // 2], dtype=torch.int32, device=cloud.device)
    allv = torch.zeros(1, dtype=torch.int32, device=cloud.device)
    _ok(_L().tohip_occlusion_rows(cloud.n, _p(cloud.inv_perm), _p(kept[0]), _p(kcnt), _p(vis), _p(voff), _p(allv), 1, _p(rows1), _s()), "occlusion_rows")
    return {"voxel rows": rows, "los_rows unpruned": rows2, "los stats": stats, "occlusion_row": row, "occlusion_rows": rows1}


@case("cull_and_projection", cloud_path)
def _cull(d):
    ops = _ops()
    x, ps, qs, cam = d["points"], d["poses"], d["quats"], _cam()
    out = {}
    kept, kpts, counts, kcnt = ops.cull_waypoints(x, ps, qs, cam, 1.0, 15.0)
    out["cull counts"] = kcnt
    for w, c in enumerate(counts):
        out[f"cull kept_idx[{w}]"], out[f"cull kept_pts[{w}]"] = kept[w, :c].clone(), kpts[w, :c].clone()
    kept2, cat, counts2, kcnt2, offs = ops.cull_waypoints(x, ps, qs, cam, 1.0, 15.0, packed=True)
    out["packed counts"], out["packed pts"], out["packed offsets"] = kcnt2, cat.clone(), offs
    for w, c in enumerate(counts2):
        out[f"packed kept_idx[{w}]"] = kept2[w, :c].clone()
    cam_pts = ops.to_camera_frame_exact(x, qs[2], ps[2])
    out["to_camera_frame"] = cam_pts
    out["to_camera_frame unnormalised"] = ops.to_camera_frame_exact(x, qs[1], ps[1], normalize=False)
    t3 = ops.to_camera_frame_exact(x, qs[3], ps[3], transpose=True)
    out["to_camera_frame transposed"] = t3
    dm, fm, idx = ops.frustum_cull(t3, cam, 1.0, 15.0)
    out["frustum dist_mask"], out["frustum fov_mask"], out["frustum idx"] = dm, fm, idx.clone()
    g = torch.sin(torch.arange(3 * x.shape[0], dtype=torch.float32, device=x.device)).view(-1, 3)
    gx, gq, gt = ops.to_camera_frame_backward(x, qs[2], ps[2], g)
    out["to_camera_frame_backward points"], out["to_camera_frame_backward quat"], out["to_camera_frame_backward trans"] = gx, gq, gt
    dmask, fmask = ops.soft_masks(cam_pts, cam)
    out["soft dist"], out["soft fov"] = dmask, fmask
    out["soft_masks_backward"] = ops.soft_masks_backward(cam_pts, cam, grad_dist=g[:, 0].contiguous(), grad_fov=g[:, 1].contiguous())
    # the C hosts' gather of kept rows
    cap = x.shape[0]
    rows = torch.empty((cap, 3), dtype=torch.float32, device=x.device)
    _ok(_L().tohip_gather_points(_p(x), x.shape[0], 0, _p(kept[0]), _p(kcnt[:1]), cap, _p(rows), _s()), "gather_points")
    out["gather_points"] = rows[:counts[0]].clone()
    return out


# ================================================================================ hull

def hull_inputs(seed):
    base = synth.make_cloud(N - 200, seed=40 + seed, extent=(6.0, 6.0, 4.0)) + f32([0.0, 0.0, 6.0])   # off the origin: the viewpoint
    pts, _ = synth.with_duplicate_rows(base, np.arange(0, 600, 4), 1040 + seed)   # 150 + 25 copies
    pts = np.concatenate([pts, base[:N - len(pts)] * f32(1.01)]).astype(f32)
    assert pts.shape == (N, 3)
    return {"points": pts}


@case("hull_flip", hull_inputs)
def _flip(d):
    out, rad = _ops().spherical_flip(d["points"])
    return {"flipped": out, "radius": rad}


@case("hull_hidden_pts_removal", hull_inputs)
def _hpr(d):
    idx, mask = _ops().hidden_pts_removal(d["points"])
    return {"visible idx": idx.clone(), "mask": mask}


@case("hull_hidden_pts_removal_batched", hull_inputs)
def _hpr_batched(d):
    idx, voff, mask, status = _ops().hidden_pts_removal_batched(d["points"], [0, 1000, 1003, N])   # a segment of three rows: status 1
    return {"visible idx": idx.clone(), "visible offsets": voff, "mask": mask, "status": status}


@case("hull_vertices_with_origin", hull_inputs)
def _hull_vertices(d):
    ops = _ops()
    # (return_rounds is left out: the count is the tag of the read-back that found no candidate left, with a batch of rounds kept in
    # flight ahead of it — hull_kernels.hip:2208-2257 — so it varies with the host's timing, 12 or 14 here in plain repeated runs)
    a = ops.hull_vertices_with_origin(d["points"])
    b = ops.hull_vertices_with_origin(d["points"], with_origin=False)
    return {"with origin": a.clone(), "without": b.clone()}


# ================================================================================ render and ingest

def render_inputs(seed):
    rng = np.random.default_rng(500 + seed)
    v = np.stack([rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(0.5, 9.0, N)], axis=1).astype(f32)
    return {"verts": v}


@case("render_points", render_inputs)
def _render(d):
    ops = _ops()
    img, owner, owns = ops.render_points(d["verts"], K, 33, 47, want_owner=True)
    return {"image": img, "owner": owner, "owns": owns, "blend": ops.render_points_blend(d["verts"], K, 33, 47)}


def ingest_inputs(seed):
    rng = np.random.default_rng(600 + seed)
    msg = rng.uniform(-4, 4, (N, 5)).astype(f32)   # point_step 20: x y z and two more fields
    msg[rng.random(N) < 0.05, 1] = np.nan
    return {"msg": msg}


@case("ingest", ingest_inputs)
def _ingest(d):
    L = _L()
    msg = d["msg"]
    dev, n = msg.device, msg.shape[0]
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.tohip_ingest_workspace_bytes(n), dtype=torch.uint8, device=dev)
    _ok(L.tohip_pointcloud2_to_xyz(_p(msg), n, 20, 0, 4, 8, 7, 0, 1, _p(xyz), _p(cnt), _p(ws), ws.numel(), _s()), "pointcloud2_to_xyz")
    m = int(cnt.item())
    pts = xyz[:m].contiguous()
    vout = torch.empty((m, 3), dtype=torch.float32, device=dev)
    vcnt = torch.zeros(1, dtype=torch.int32, device=dev)
    vws = torch.empty(L.tohip_voxel_grid_workspace_bytes(m), dtype=torch.uint8, device=dev)
    _ok(L.tohip_voxel_grid(_p(pts), m, 0.5, 0.3, 0.7, 2, -3.0, 3.5, _p(vout), _p(vcnt), _p(vws), vws.numel(), _s()), "voxel_grid")
    nx, ny, nz = 13, 10, 7
    vox = torch.empty((nx, ny, nz), dtype=torch.float64, device=dev)
    _ok(L.tohip_pc_to_voxel(_p(pts), m, 3, 0.75, -4.0, 5.75, -4.0, 3.5, -2.0, 3.25, nx, ny, nz, _p(vox), _s()), "pc_to_voxel")
    return {"xyz": pts, "count": cnt, "voxel_grid": vout[:int(vcnt.item())].clone(), "voxel_grid count": vcnt, "pc_to_voxel": vox}


# ================================================================================ clearance

def clearance_inputs(seed):
    d = cloud_path(seed)
    rng = np.random.default_rng(700 + seed)
    q = rng.uniform([-12, -5, -2], [12, 5, 2], (259, 3)).astype(f32)
    q[7] = d["points"][N // 3]          # on a cloud point
    q[-1] = (500.0, 500.0, 500.0)       # far from everything
    d["queries"] = q
    return d


def _clearance_outputs(out, name, source, q, walk, r=1.0, w=1.5):
    ops = _ops()
    dev = q.device
    g = torch.empty((q.shape[0], 3), dtype=torch.float32, device=dev)
    terms = ops.clearance_terms(q.shape[0], 1, "waypoints", dev)
    out[f"{name}.points d"], out[f"{name}.points idx"], out[f"{name}.points value"] = ops.clearance(source, q, r, w, grad=g, want_value=True, terms=terms)
    out[f"{name}.points grad"], out[f"{name}.points terms"] = g, terms[:q.shape[0]].clone()
    d1, i1 = ops.clearance(source, q[:1].contiguous(), r)
    out[f"{name}.one point d"], out[f"{name}.one point idx"] = d1, i1
    E = q.shape[0] // 2
    g2 = torch.empty((2 * E, 3), dtype=torch.float32, device=dev)
    out[f"{name}.segments d"], out[f"{name}.segments idx"], out[f"{name}.segments s"], out[f"{name}.segments value"] = \
        ops.clearance_segments(source, q[:2 * E].contiguous(), r, w, n_traj=E, grad=g2, want_value=True)
    out[f"{name}.segments grad"] = g2
    g3 = torch.empty((walk.shape[0], 3), dtype=torch.float32, device=dev)
    out[f"{name}.walk d"], out[f"{name}.walk idx"], out[f"{name}.walk s"], out[f"{name}.walk value"] = \
        ops.clearance_segments(source, walk, r, w, grad=g3, want_value=True)
    out[f"{name}.walk grad"] = g3


@case("clearance_cloud", clearance_inputs)
def _clearance_cloud(d):
    ops = _ops()
    out = {}
    for sort in (True, False):
        cloud = ops.PackedCloud(d["points"], sort=sort)
        _clearance_outputs(out, f"sort={sort}", cloud, d["queries"], d["poses"])
        q = d["queries"]
        out[f"sort={sort}.edges d"], out[f"sort={sort}.edges idx"], out[f"sort={sort}.edges s"] = \
            ops.clearance_edges(cloud, q[0::2][:129].contiguous(), q[1::2][:129].contiguous(), 1.0)
    return out


# ================================================================================ the map layer

def _box(dims, origin=ORIGIN, r=RES):
    lo = np.asarray(origin, dtype=np.float64)
    return lo, lo + r * np.asarray(dims, dtype=np.float64)


def map_inputs(dims, fill=0.08, M=259, V=33):
    """A scan of `dims`: returns at the centres of a random share `fill` of the voxels (the same count for every seed), the sensor in a
    voxel left empty near the middle, query positions in and around the box (two out of range, one NaN), V views inside it."""
    def make(seed):
        rng = np.random.default_rng(800 + seed + dims[0])
        nvox = int(np.prod(dims))
        count = max(1, int(round(fill * nvox))) if nvox > 1 else 1
        mid = np.asarray(dims) // 2
        lin_mid = int((mid[2] * dims[1] + mid[1]) * dims[0] + mid[0])
        cand = np.setdiff1d(np.arange(nvox), [lin_mid]) if nvox > 1 else np.arange(1)
        lin = np.sort(rng.choice(cand, size=min(count, len(cand)), replace=False))
        ijk = np.stack([lin % dims[0], (lin // dims[0]) % dims[1], lin // (dims[0] * dims[1])], axis=1)
        lo, hi = _box(dims)
        pos = rng.uniform(lo - 3 * RES, hi + 3 * RES, (M, 3)).astype(f32)
        if M >= 4:
            pos[1] = (1.0e6, 0.0, 0.0)
            pos[2] = (np.nan, 0.0, 0.0)
            pos[3] = tc.centre(mid)
        views = rng.uniform(lo, hi, (V, 3)).astype(f32)
        returns = (tc.centre(ijk) + rng.uniform(-0.3, 0.3, (len(ijk), 3)) * RES).astype(f32)   # inside their voxels
        return {"returns": returns, "sensor": (tc.centre(mid) + f32(0.01 * (seed + 1))).astype(f32)[None, :], "positions": pos,
                "view_poses": views, "view_quats": _yaw_quats(rng.uniform(0, 360, V)),
                "ijk": rng.integers(-2, np.asarray(dims) + 2, (M, 3)).astype(np.int32)}
    return make


def _space_of(d, dims):
    """The three-state map of one scan: the rays sensor -> returns carve the free plane, the returns become occupied."""
    ops = _ops()
    dev = d["returns"].device
    space = ops.SpaceMap(ops.OccupancyGrid(ORIGIN, RES, dims, device=dev))
    skipped = space.integrate(d["sensor"], d["returns"], max_range=2.0)
    return space, skipped


def _occupancy_outputs(d, dims):
    ops = _ops()
    space, skipped = _space_of(d, dims)
    grid = space.occupied
    out = {"skipped": skipped, "insert again skipped": grid.insert(d["positions"]), "lookup": grid.lookup(d["ijk"]), "state": space.state(d["positions"]),
           "count": grid.count(), "free count": space.free.count()}
    out["export ijk"], out["export centres"] = grid.export()
    fr = space.frontier(1)
    out["frontier ijk"], out["frontier points"] = fr.ijk, fr.points
    out["unknown count"] = space.unknown().count()
    n = d["positions"].shape[0]
    flags = torch.empty(n, dtype=torch.uint8, device=grid.device)
    stats = torch.zeros(3, dtype=torch.int64, device=grid.device)
    plane = grid.empty_like()
    out["carve skipped"] = plane.carve(d["sensor"], d["positions"], max_range=0.5, stats=stats, flags=flags)
    # (stats[2], the atomics issued, is left out: an atomic OR is "issued only where a brick's word lacks one of the gathered bits",
    # include/trajopt_hip.h:1175-1178, so the count depends on which ray's wave reaches a shared word first; the plane does not)
    out["carve flags"], out["carve stats"], out["carve plane"] = flags, stats[:2].clone(), plane.buf[256:].clone()
    a, b = d["positions"], d["positions"].roll(1, 0).contiguous()
    out["line_of_sight"] = grid.line_of_sight(a, b, skip=(1, 1))
    out["cast voxel"], out["cast lam"] = grid.cast(a, b)
    return out


@case("occupancy_37_5_20", map_inputs(GRID_A))
def _occupancy_a(d):
    return _occupancy_outputs(d, GRID_A)


@case("occupancy_13_10_7", map_inputs(GRID_B))
def _occupancy_b(d):
    return _occupancy_outputs(d, GRID_B)


@case("occupancy_1_1_1", map_inputs(GRID_1, M=1, V=1))
def _occupancy_1(d):
    return _occupancy_outputs(d, GRID_1)


def _view_cam():
    return _ops().Camera(K, IW, IH, 0.2, 2.0)


@case("view_volume_and_select", map_inputs(GRID_A))
def _view_volume(d):
    ops = _ops()
    space, _ = _space_of(d, GRID_A)
    cam = _view_cam()
    P, Q = d["view_poses"], d["view_quats"]
    stats = torch.zeros(3, dtype=torch.int64, device=space.device)
    mark = space.free.empty_like()
    out = {"gains": ops.view_volume(space, P, Q, cam, 0.2, 2.0, mark=mark, stats=stats), "mark": mark.buf[256:].clone(), "stats": stats}
    out["gains every brick"] = ops.view_volume(space, P, Q, cam, 0.2, 2.0, window=False)
    out["gains one view"] = ops.view_volume(space, P[:1], Q[:1], cam, 0.2, 2.0)
    order, picked, revealed = ops.view_volume_select(space, P, Q, cam, 0.2, 2.0, 3)
    out["select order"], out["select gains"], out["select revealed"] = order, picked, revealed.buf[256:].clone()
    return out


@case("view_volume_travel_pick", map_inputs(GRID_A))
def _view_volume_travel(d):
    ops = _ops()
    space, _ = _space_of(d, GRID_A)
    field = ops.ClearanceField.build(space, 3 * RES)
    tf = ops.TravelField(field, tc.RADIUS, d["sensor"])
    cost = tf.cost(d["view_poses"])
    order, picked, revealed = ops.view_volume_select(space, d["view_poses"], d["view_quats"], _view_cam(), 0.2, 2.0, 3, travel_cost=cost, travel_m=2)
    return {"cost": cost, "order": order, "gains": picked, "revealed": revealed.buf[256:].clone()}


def scan_inputs(seed):
    d = map_inputs(GRID_A, V=3)(seed)
    return d


@case("depth_scan_17x9", scan_inputs)
def _depth_scan(d):
    ops = _ops()
    space, _ = _space_of(d, GRID_A)
    grid = space.occupied
    import raycast_cases as rc
    cam = ops.Camera(rc.camera(17, 9, integral=False), 17, 9, 0.1, 2.0)
    hit, pas = grid.empty_like(), grid.empty_like()
    stats = torch.zeros(3, dtype=torch.int64, device=grid.device)
    voxel, depth, flags, pts = ops.depth_scan(grid, d["view_poses"], d["view_quats"], cam, 0.1, 2.0, hit_plane=hit, pass_plane=pas, points=True, stats=stats)
    v1, d1, f1, _ = ops.depth_scan(grid, d["view_poses"][:1], d["view_quats"][:1], cam, 0.1, 2.0)
    # (stats[2], the plane atomics issued, is left out as carve's is: include/trajopt_hip.h:1395, issued only where the word lacks the bit)
    return {"voxel": voxel, "depth": depth, "flags": flags, "points": pts, "hit plane": hit.buf[256:].clone(), "pass plane": pas.buf[256:].clone(),
            "stats": stats[:2].clone(), "one view voxel": v1, "one view depth": d1, "one view flags": f1}


def _field_outputs(d, dims):
    ops = _ops()
    space, _ = _space_of(d, dims)
    out = {}
    for unknown in ("free", "obstacle"):
        field = ops.ClearanceField.build(space, 3 * RES, unknown=unknown)
        out[f"{unknown}.dense"] = field.dense()
        out[f"{unknown}.d2"], out[f"{unknown}.distance"] = field.lookup_positions(d["positions"]), field.distance(d["positions"])
        a, b = d["positions"], d["positions"].roll(1, 0).contiguous()
        out[f"{unknown}.segments d2"], out[f"{unknown}.segments vox"] = field.segments(a, b)
        out[f"{unknown}.edges d"], out[f"{unknown}.edges idx"], _ = field.edges(a, b, tc.RADIUS)
        nodes = field.free_nodes(tc.RADIUS, stride=2, space=space if unknown == "free" else None)
        out[f"{unknown}.nodes ijk"], out[f"{unknown}.nodes points"] = nodes.ijk, nodes.points
    return out


@case("clearance_field_37_5_20", map_inputs(GRID_A))
def _field_a(d):
    return _field_outputs(d, GRID_A)


@case("clearance_field_13_10_7", map_inputs(GRID_B))
def _field_b(d):
    return _field_outputs(d, GRID_B)


@case("clearance_field_1_1_1", map_inputs(GRID_1, M=1, V=1))
def _field_1(d):
    return _field_outputs(d, GRID_1)


def clearance_map_inputs(seed):
    d = map_inputs(GRID_B, fill=0.05)(seed)
    lo, hi = _box(GRID_B)
    rng = np.random.default_rng(900 + seed)
    d["walk"] = rng.uniform(lo, hi, (W5, 3)).astype(f32)
    return d


@case("clearance_from_the_map", clearance_map_inputs)
def _clearance_map(d):
    ops = _ops()
    space, _ = _space_of(d, GRID_B)
    out = {}
    for unknown in ("free", "obstacle"):
        _clearance_outputs(out, unknown, ops.MapObstacles(space, unknown=unknown), d["positions"], d["walk"], r=0.3)
    _clearance_outputs(out, "grid", ops.MapObstacles(space.occupied), d["positions"], d["walk"], r=0.3)
    return out


def travel_inputs(dims, S=4):
    base = map_inputs(dims, fill=0.04)

    def make(seed):
        d = base(seed)
        lo, hi = _box(dims)
        rng = np.random.default_rng(1000 + seed)
        src = rng.uniform(lo, hi, (S, 3)).astype(f32)
        src[0] = d["sensor"][0]
        if S > 2:
            src[-1] = (np.nan, 0.0, 0.0)
        d["sources"] = src
        d["goals"] = d["positions"][3:3 + W5].copy()
        return d
    return make


def _travel_field_of(d, dims):
    ops = _ops()
    space, _ = _space_of(d, dims)
    field = ops.ClearanceField.build(space, 3 * RES)
    return space, field


def _travel_outputs(d, dims):
    ops = _ops()
    space, field = _travel_field_of(d, dims)
    tf = ops.TravelField(field, tc.RADIUS, d["sources"], space=space, max_dist=40 * RES, rounds_per_check=3)
    out = {"seeded": tf.seeded, "rounds": tf.rounds, "dense": tf.dense(), "cost": tf.cost(d["positions"]), "distance": tf.distance(d["positions"])}
    flat(out, "paths", tf.paths(d["goals"]))
    tf.rebuild(d["sources"][:1])
    out["rebuilt seeded"], out["rebuilt dense"] = tf.seeded, tf.dense()
    return out


@case("travel_37_5_20", travel_inputs(GRID_A))
def _travel_a(d):
    return _travel_outputs(d, GRID_A)


@case("travel_13_10_7", travel_inputs(GRID_B))
def _travel_b(d):
    return _travel_outputs(d, GRID_B)


@case("travel_1_1_1", lambda seed: {k: v for k, v in travel_inputs(GRID_1, S=1)(seed).items()})
def _travel_1(d):
    ops = _ops()
    field = ops.ClearanceField(ops.OccupancyGrid(ORIGIN, RES, GRID_1, device=d["sources"].device), D=tc.D)
    tf = ops.TravelField(field, tc.RADIUS, d["sources"])
    return {"seeded": tf.seeded, "dense": tf.dense(), "cost": tf.cost(d["sources"])}


def _travel_batch_outputs(d, dims):
    ops = _ops()
    from trajectory_optimization_amd import tools
    space, field = _travel_field_of(d, dims)
    src = d["sources"][:3].contiguous()
    tfs = ops.TravelFields(field, tc.RADIUS, src, space=space, rounds_per_check=3)   # 3 fields, one per source
    out = {"seeded": tfs.seeded, "rounds": tfs.rounds, "dense": tfs.dense(), "cost": tfs.cost(d["positions"]), "distance": tfs.distance(d["positions"])}
    gf = torch.arange(d["goals"].shape[0], device=src.device) % 4 - 1    # -1, 0, 1, 2, -1
    flat(out, "paths", tfs.paths(d["goals"], gf))
    flat(out, "assign", tools.assign_frontiers(space, tfs))
    flat(out, "matrix", tools.travel_matrix(field, src, tc.RADIUS, space=space))
    return out


@case("travel_batch_37_5_20", travel_inputs(GRID_A))
def _travel_batch_a(d):
    return _travel_batch_outputs(d, GRID_A)


@case("travel_batch_13_10_7", travel_inputs(GRID_B))
def _travel_batch_b(d):
    return _travel_batch_outputs(d, GRID_B)


def _components_outputs(d, dims):
    ops = _ops()
    space, field = _travel_field_of(d, dims)
    out = {}
    for c in (6, 26):
        comp = ops.Components(space.free, connectivity=c, rounds_per_check=2)
        out.update({f"c{c}.n": comp.n, f"c{c}.rounds": comp.rounds, f"c{c}.labels": comp.labels.clone(), f"c{c}.roots": comp.roots.clone(),
                    f"c{c}.sizes": comp.sizes, f"c{c}.sums": comp.sums, f"c{c}.bbox": comp.bbox, f"c{c}.centroids": comp.centroids,
                    f"c{c}.at": comp.at(d["positions"])})
        if c == 26:
            tf = ops.TravelField(field, tc.RADIUS, d["sources"], space=space)
            out["min value"], out["min voxel"] = comp.min_over(tf)
    occ = ops.Components(space.occupied)
    out["occupied.n"], out["occupied.sizes"] = occ.n, occ.sizes
    return out


@case("components_37_5_20", travel_inputs(GRID_A))
def _components_a(d):
    return _components_outputs(d, GRID_A)


@case("components_13_10_7", travel_inputs(GRID_B))
def _components_b(d):
    return _components_outputs(d, GRID_B)


@case("components_1_1_1", map_inputs(GRID_1, M=1, V=1))
def _components_1(d):
    ops = _ops()
    grid = ops.OccupancyGrid(ORIGIN, RES, GRID_1, device=d["returns"].device)
    grid.insert(d["returns"])
    comp = ops.Components(grid)
    return {"n": comp.n, "labels": comp.labels.clone(), "sizes": comp.sizes, "at": comp.at(d["positions"])}


@case("frontier_clusters", travel_inputs(GRID_A))
def _frontier_clusters(d):
    from trajectory_optimization_amd import tools
    ops = _ops()
    space, field = _travel_field_of(d, GRID_A)
    tf = ops.TravelField(field, tc.RADIUS, d["sources"], space=space)
    return flat({}, "clusters", tools.frontier_clusters(space, travel=tf))


def _evidence_outputs(d, dims, shift):
    ops = _ops()
    dev = d["returns"].device
    em = ops.EvidenceMap(ORIGIN, RES, dims, device=dev)
    out = {"skipped": em.integrate(d["sensor"], d["returns"], max_range=2.0)}
    out["counts 1"] = em._counts.clone()
    em.integrate(d["sensor"], d["positions"])   # a second scan: other returns, misses where the first scan had hits
    out["counts 2"] = em._counts.clone()
    hit, pas = em.occupied.empty_like(), em.occupied.empty_like()
    hit.insert(d["positions"])
    pas.carve(d["sensor"], d["view_poses"])
    em.fold(hit, pas, clear=True)
    out["counts 3"], out["hit plane after a clearing fold"] = em._counts.clone(), hit.buf[256:].clone()
    out["dense"], out["occupied plane"], out["free plane"] = em.dense(), em.occupied.buf[256:].clone(), em.free.buf[256:].clone()
    out["log_odds values"], out["log_odds state"] = em.log_odds(d["positions"])
    # re-framing at a shift unaligned on every axis, and merging: all three map types
    moved = em.reframed(shift=shift)
    out["reframed dense"], out["reframed counts"] = moved.dense(), moved._counts.clone()
    out["reframed occupied"] = moved.occupied.buf[256:].clone()
    other = ops.EvidenceMap.from_space(_space_of(d, dims)[0])
    for mode in ("confident", "add"):
        m = em.reframed(shift=(0, 0, 0))
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        m.merge(moved, mode=mode, counts=counts)
        m.merge(other, mode=mode)
        out[f"merge {mode} dense"], out[f"merge {mode} counts"], out[f"merge {mode} last counts"] = m.dense(), counts, m._counts.clone()
    space = _space_of(d, dims)[0]
    sm = space.reframed(shift=shift)
    out["space reframed occupied"], out["space reframed free"] = sm.occupied.buf[256:].clone(), sm.free.buf[256:].clone()
    grown = space.occupied.reframed(centre=d["sensor"][0].tolist(), dims=tuple(n + 3 for n in dims))
    out["grid reframed by centre"] = grown.buf[256:].clone()
    n_new = torch.zeros(1, dtype=torch.int64, device=dev)
    space.occupied.merge(sm.occupied, counts=n_new)
    space.merge(sm)
    out["grid merge count"], out["space merged occupied"], out["space merged free"] = n_new, space.occupied.buf[256:].clone(), space.free.buf[256:].clone()
    return out


@case("evidence_and_reframe_37_5_20", map_inputs(GRID_A))
def _evidence_a(d):
    return _evidence_outputs(d, GRID_A, (3, -1, 1))


@case("evidence_and_reframe_13_10_7", map_inputs(GRID_B))
def _evidence_b(d):
    return _evidence_outputs(d, GRID_B, (-5, 2, -3))


def fold_inputs(seed):
    import reframe_cases as rfc
    d = {"positions": map_inputs(GRID_A)(seed)["positions"]}
    d["hit_words"] = rfc.plane_words(rfc.plane_bits(GRID_A, 0.05, seed=seed)).view(np.int32)
    d["pass_words"] = rfc.plane_words(rfc.plane_bits(GRID_A, 0.3, seed=seed + 10)).view(np.int32)
    return d


@case("evidence_fold_first", fold_inputs)
def _evidence_fold_first(d):
    """The fold as the first call that reads the inputs, with no host synchronisation before it (integrate's carve reads its skipped
    count back first): a fold misplaced on another stream has nothing to hide behind."""
    ops = _ops()
    em = ops.EvidenceMap(ORIGIN, RES, GRID_A, device=d["positions"].device)
    hit, pas = em.occupied.empty_like(), em.occupied.empty_like()
    hit.buf[256:].view(torch.int32).copy_(d["hit_words"])
    pas.buf[256:].view(torch.int32).copy_(d["pass_words"])
    em.fold(hit, pas, clear=True)
    out = {"counts": em._counts.clone(), "dense": em.dense(), "occupied plane": em.occupied.buf[256:].clone(), "free plane": em.free.buf[256:].clone(),
           "hit plane after the clearing fold": hit.buf[256:].clone()}
    out["values"], out["state"] = em.log_odds(d["positions"])
    return out


@case("evidence_1_1_1", map_inputs(GRID_1, M=1, V=1))
def _evidence_1(d):
    ops = _ops()
    em = ops.EvidenceMap(ORIGIN, RES, GRID_1, device=d["returns"].device)
    em.integrate(d["sensor"] + 1.0, d["returns"])
    v, s = em.log_odds(d["positions"])
    return {"dense": em.dense(), "values": v, "state": s, "reframed": em.reframed(shift=(1, 0, 0)).dense()}


# ================================================================================ planning

def planning_inputs(seed):
    d = cloud_path(seed)
    rng = np.random.default_rng(1100 + seed)
    d["nodes"] = rng.uniform([-11, -4, -1], [11, 4, 1], (W5 + 2, 3)).astype(f32)
    d["lattice"] = rng.uniform([-11, -4, -1], [11, 4, 1], (40, 3)).astype(f32)
    d["prior"] = (rng.random(N) * 2.0 * (rng.random(N) > 0.3)).astype(f32)
    return d


@case("tour", planning_inputs)
def _tour(d):
    from trajectory_optimization_amd import tools
    ops = _ops()
    cloud = ops.PackedCloud(d["points"])
    out = {}
    flat(out, "open", tools.plan_tour(cloud, d["nodes"], clearance_radius=0.6))
    flat(out, "closed", tools.plan_tour(cloud, d["nodes"], clearance_radius=0.6, closed=True))
    flat(out, "via", tools.plan_tour(cloud, d["nodes"], clearance_radius=0.6, via=d["lattice"], via_k=6))
    return out


@case("roadmap", planning_inputs)
def _roadmap(d):
    from trajectory_optimization_amd import tools
    ops = _ops()
    cloud = ops.PackedCloud(d["points"])
    out = {}
    nbr, length = ops.roadmap_knn(d["lattice"], k=5, max_edge=9.0)
    out["knn nbr"], out["knn length"] = nbr, length
    D, pred, sweeps = ops.roadmap_routes(nbr, length, nbr >= 0, [0, 7, 39], sweeps_per_check=2)
    out["routes D"], out["routes pred"], out["routes sweeps"] = D.clone(), pred.clone(), sweeps
    flat(out, "roadmap", tools.build_roadmap(cloud, d["lattice"], 0.5, k=6))
    flat(out, "path", tools.plan_path(cloud, d["nodes"][0], d["nodes"][1], d["lattice"], 0.1, k=8))
    return out


@case("path_refine", planning_inputs)
def _path_refine(d):
    from trajectory_optimization_amd import tools
    ops = _ops()
    cloud = ops.PackedCloud(d["points"])
    out = {}
    flat(out, "refined", tools.refine_path(cloud, d["lattice"][:W5 + 4], clearance_radius=0.4, spacing=0.75))
    flat(out, "with quats", tools.refine_path(cloud, d["poses"], quats=d["quats"], clearance_radius=0.4))
    return out


@case("view_proposal", planning_inputs)
def _propose(d):
    from trajectory_optimization_amd import tools
    ops = _ops()
    cloud = ops.PackedCloud(d["points"])
    out = {}
    w = (d["prior"] * 1000).to(torch.int32)
    hist = ops.view_histogram(cloud, d["lattice"], weights=w, sectors=16, min_dist=1.0, max_dist=5.0)
    out["hist"] = hist
    out["hist one position"] = ops.view_histogram(cloud, d["lattice"][:1].contiguous(), sectors=8, prune=False)
    out["heading"], out["score"] = ops.view_headings(hist, hw=1, n_per=3)
    flat(out, "proposals", tools.propose_views(cloud, d["lattice"], prior_log_odds=d["prior"], clearance_radius=0.3, K=torch.from_numpy(K), img_width=IW,
                                               img_height=IH))
    return out


def views_inputs(seed):
    d = planning_inputs(seed)
    rng = np.random.default_rng(1200 + seed)
    d["cand_poses"] = rng.uniform([-11, -4, -0.5], [11, 4, 0.5], (33, 3)).astype(f32)
    d["cand_quats"] = _yaw_quats(rng.uniform(0, 360, 33))
    return d


@case("view_set_and_select", views_inputs)
def _views(d):
    from trajectory_optimization_amd import tools
    ops = _ops()
    cloud, cam = ops.PackedCloud(d["points"]), _cam()
    prior = ops.LogOddsPrior(cloud, d["prior"])
    vs = ops.ViewSet(cloud, cam, 33, chunk=8)   # two appends in chunks of 8: the second one's last chunk holds one candidate
    vs.append(d["cand_poses"][:16], d["cand_quats"][:16])
    vs.append(d["cand_poses"][16:], d["cand_quats"][16:])
    out = {"header": vs.header().clone(), "absent": vs.absent, "offsets": vs.offsets.clone()}
    idx, val = vs.entries()
    out["idx"], out["val"] = idx.clone(), val.clone()
    out["row 0"], out["row 32"] = vs.row(0)[:cloud.n].clone(), vs.row(32)[:cloud.n].clone()
    order, gain, n_sel, S = ops.views_select(vs, 4, prior=prior)
    out["order"], out["gain"], out["n_selected"], out["S"] = order, gain, n_sel, S[:cloud.n].clone()
    sel = tools.select_views(cloud, d["cand_poses"], d["cand_quats"], 3, intrins=torch.from_numpy(K), img_width=IW, img_height=IH, occlusion="zbuffer")
    flat(out, "select_views", sel)
    return out


def team_inputs(seed):
    d = cloud_path(seed, W=3 * W5)
    rng = np.random.default_rng(1300 + seed)
    d["poses"] = (d["poses"] + np.repeat(f32([[0, 0, 0], [0, 1.5, 0], [0, -1.5, 0]]), W5, axis=0)).astype(f32)
    d["poses0"] = (d["poses"] + rng.uniform(-0.1, 0.1, d["poses"].shape)).astype(f32)
    d["scalars"] = f32([0.5 + 0.01 * seed, 1.7, -0.1, 0.0])
    d["clr_terms"] = rng.random(3 * W5)
    return d


@case("team_loss_and_member_gains", team_inputs)
def _team(d):
    ops = _ops()
    cloud, cam = ops.PackedCloud(d["points"]), _cam()
    out = {}
    terms, total, reg = ops.team_loss(d["poses"], d["poses0"], 3, 28.0, 0.05, 1e-6, d["scalars"])
    out["terms"], out["total"], out["reg"] = terms[:, [0, 1, 2, 3, 5]].clone(), total, reg
    terms, total, reg = ops.team_loss(d["poses"], d["poses0"], 3, 28.0, 0.05, 1e-6, d["scalars"], clearance_weight=0.7, clr_terms=d["clr_terms"])
    out["clearance terms"], out["clearance total"], out["clearance reg"] = terms[:, [0, 1, 2, 3, 5]].clone(), total, reg
    toff = (torch.arange(4, dtype=torch.int32, device=cloud.device) * W5).contiguous()
    ws = ops.TrajWorkspace(cloud, 3 * W5, 3)
    lo, _ = ops.traj_forward(cloud, d["poses"], d["quats"], cam, ws, traj_offsets=toff)
    gain, count = ops.team_member_gains(cloud, lo)
    out["member gains"], out["member counts"] = gain, count
    r, s = ops.traj_reward(cloud, lo, cam, ws)
    out["member rewards"], out["member scalars"] = r, s
    gout = torch.ones(3, dtype=torch.float32, device=cloud.device)
    pg, qg = ops.traj_backward(cloud, 3 * W5, cam, ws, lo, scalars=s, gout=gout, n_traj=3)
    out["member poses_grad"], out["member quats_grad"] = pg, qg
    return out


def covmap_inputs(seed):
    d = cloud_path(seed)
    rng = np.random.default_rng(1400 + seed)
    d["log_odds"] = (rng.random(N) * 3.0).astype(f32)
    d["other"] = synth.make_cloud(259, seed=1450 + seed, extent=CLOUD_EXTENT)
    d["other_log_odds"] = (rng.random(259) * 3.0).astype(f32)
    return d


@case("coverage_map", covmap_inputs)
def _covmap(d):
    ops = _ops()
    dev = d["points"].device
    cmap = ops.CoverageMap((-0.3, 0.2, 0.1), 0.5, clamp_max=4.0, capacity=16, device=dev)   # 16 slots: the first integrate forces a rehash
    cmap.integrate(d["points"], d["log_odds"], "max")
    cmap.integrate(d["points"][::3].contiguous(), d["log_odds"][::3].contiguous(), "add")
    other = ops.CoverageMap((-0.3, 0.2, 0.1), 0.5, clamp_max=4.0, device=dev)
    other.integrate(d["other"], d["other_log_odds"], "max")
    out = {"lookup before merge": cmap.lookup(d["other"])}
    cmap.merge(other, "add")
    c, v, k = cmap.export()
    out.update({"export centres": c, "export values": v, "export keys": k, "lookup": cmap.lookup(d["points"]), "lookup other": cmap.lookup(d["other"]),
                "n_voxels": cmap.n_voxels, "capacity": cmap.capacity})
    flat(out, "header", cmap.header())
    return out


# ================================================================================ optimiser steps

def _model_traj(d, **kw):
    from trajectory_optimization_amd.model import ModelTraj
    return ModelTraj(d["points"], d["poses"], d["quats"], torch.from_numpy(K), IW, IH, device=d["points"].device, **kw)


def _traj_result(out, name, m, res):
    out[f"{name}.poses"], out[f"{name}.quats"], out[f"{name}.rewards"] = m.poses.detach().clone(), m.quats.detach().clone(), m.rewards.detach().clone()
    out[f"{name}.losses"], out[f"{name}.steps"] = np.asarray(res.losses, dtype=np.float64), res.steps_taken
    flat(out, f"{name}.loss", {k: (v.detach().clone() if torch.is_tensor(v) else float(v)) for k, v in m.loss.items()})


def optimiser_inputs(seed):
    return cloud_path_prior(seed, W=2 * W5 + 1)


@case("optimise_trajectory_clearance", optimiser_inputs)
def _opt_traj(d):
    from trajectory_optimization_amd.optimizer import optimize_trajectory
    out = {}
    for mode in ("waypoints", "segments"):
        m = _model_traj(d, clearance_radius=0.75, clearance_weight=2.0, clearance_mode=mode)
        res = optimize_trajectory(m, n_opt_steps=3, lr_pose=0.05, lr_quat=0.02, rewards_th=1e9, vis_wps_dist=0.0)
        _traj_result(out, mode, m, res)
    return out


@case("optimise_trajectory_prior", optimiser_inputs)
def _opt_traj_prior(d):
    from trajectory_optimization_amd.optimizer import optimize_trajectory
    out = {}
    for mode in ("waypoints", "segments"):
        m = _model_traj(d, clearance_radius=0.75, clearance_weight=2.0, clearance_mode=mode, prior_log_odds=d["prior"])
        res = optimize_trajectory(m, n_opt_steps=3, lr_pose=0.05, lr_quat=0.02, rewards_th=1e9, vis_wps_dist=2.5)
        _traj_result(out, mode, m, res)
    return out


@case("optimise_trajectory_plain_strided", optimiser_inputs)
def _opt_traj_plain(d):
    from trajectory_optimization_amd.optimizer import optimize_trajectories, optimize_trajectory
    out = {}
    m = _model_traj(d)
    _traj_result(out, "strided", m, optimize_trajectory(m, n_opt_steps=3, lr_pose=0.05, lr_quat=0.02, rewards_th=1e9, vis_wps_dist=2.5))
    a, b = _model_traj(d), None
    from trajectory_optimization_amd.model import ModelTraj
    b = ModelTraj.sharing_cloud_of(a, d["poses"] + 0.25, d["quats"])
    for name, m, res in zip(("first", "second"), (a, b), optimize_trajectories([a, b], n_opt_steps=3, lr_pose=0.05, rewards_th=1e9, vis_wps_dist=0.0)):
        _traj_result(out, name, m, res)
    return out


@case("model_traj_forward_backward", optimiser_inputs)
def _model_fb(d):
    from trajectory_optimization_amd.optimizer import Adam
    out = {}
    clr = dict(clearance_radius=0.75, clearance_weight=2.0)
    for name, kw in (("clearance", clr), ("prior", dict(prior_log_odds=d["prior"])), ("prior and clearance", dict(prior_log_odds=d["prior"], **clr)),
                     ("zbuffer", dict(occlusion="zbuffer"))):
        m = _model_traj(d, **kw)
        opt = Adam([{"params": [m.poses], "lr": 0.05}, {"params": [m.quats], "lr": 0.02}])
        loss = m(vis_wps_dist=0.0)
        loss.backward()
        out[f"{name}.loss"], out[f"{name}.rewards"] = loss.detach().clone(), m.rewards.detach().clone()
        out[f"{name}.poses.grad"], out[f"{name}.quats.grad"] = m.poses.grad.clone(), m.quats.grad.clone()
        opt.step()   # one launch for both groups
        out[f"{name}.poses after Adam"], out[f"{name}.quats after Adam"] = m.poses.detach().clone(), m.quats.detach().clone()
        loss2 = m(vis_wps_dist=0.0)
        out[f"{name}.loss again"] = loss2.detach().clone()
    # a backward through the rewards first leaves ITS sums in the plan: the loss's own backward takes them again
    m = _model_traj(d)
    loss = m(vis_wps_dist=0.0)
    m.rewards.sum().backward(retain_graph=True)
    out["rewards first.poses.grad"] = m.poses.grad.clone()
    loss.backward()
    out["then loss.poses.grad"], out["then loss.quats.grad"] = m.poses.grad.clone(), m.quats.grad.clone()
    return out


@case("optimise_trajectory_occlusion", optimiser_inputs)
def _opt_traj_occlusion(d):
    """The separate-call step without a clearance term: forward | rows | reward + backward | the plain step tail."""
    from trajectory_optimization_amd.optimizer import optimize_trajectory
    out = {}
    m = _model_traj(d, occlusion="zbuffer")
    _traj_result(out, "zbuffer", m, optimize_trajectory(m, n_opt_steps=3, lr_pose=0.05, lr_quat=0.02, rewards_th=1e9, vis_wps_dist=0.0))
    return out


def pose_opt_inputs(seed):
    d = cloud_path(seed, W=3)
    return d


@case("optimise_pose", pose_opt_inputs)
def _opt_pose(d):
    from trajectory_optimization_amd.model import ModelPose
    from trajectory_optimization_amd.optimizer import optimize_pose, optimize_poses
    Kt = torch.from_numpy(K)
    dev = d["points"].device
    out = {}
    for name, kw in (("plain", {}), ("zbuffer", dict(occlusion="zbuffer"))):
        m = ModelPose(d["points"], d["poses"][1:2], d["quats"][1:2], Kt, IW, IH, device=dev, **kw)
        res = optimize_pose(m, n_opt_steps=3, lr_pose=0.05, lr_quat=0.02)
        out[f"{name}.trans"], out[f"{name}.quat"], out[f"{name}.losses"] = m.trans.detach().clone(), m.quat.detach().clone(), np.asarray(res.losses, dtype=np.float64)
    first = ModelPose(d["points"], d["poses"][0:1], d["quats"][0:1], Kt, IW, IH, device=dev)
    models = [first] + [ModelPose.sharing_cloud_of(first, d["poses"][i:i + 1], d["quats"][i:i + 1]) for i in (1, 2)]
    res = optimize_poses(models, n_opt_steps=3, lr_pose=0.05, lr_quat=0.02)
    for i, (m, r) in enumerate(zip(models, res)):
        out[f"multi[{i}].trans"], out[f"multi[{i}].quat"], out[f"multi[{i}].losses"] = m.trans.detach().clone(), m.quat.detach().clone(), np.asarray(r.losses, dtype=np.float64)
    m = ModelPose(d["points"], d["poses"][1:2], d["quats"][1:2], Kt, IW, IH, device=dev)
    loss = m()
    loss.backward()
    out["model.loss"], out["model.trans.grad"], out["model.quat.grad"] = loss.detach().clone(), m.trans.grad.clone(), m.quat.grad.clone()
    return out


def team_opt_inputs(seed):
    d = cloud_path(seed, W=2 * W5 + 1)
    d["poses_b"] = (d["poses"] + f32([0.0, 1.5, 0.0])).astype(f32)
    return d


@case("optimise_team_of_two", team_opt_inputs)
def _opt_team(d):
    from trajectory_optimization_amd.model import ModelTraj
    from trajectory_optimization_amd.optimizer import optimize_team
    a = _model_traj(d, clearance_radius=0.75, clearance_weight=2.0)
    b = ModelTraj.sharing_cloud_of(a, d["poses_b"], d["quats"], clearance_radius=0.75, clearance_weight=2.0)
    res = optimize_team([a, b], n_opt_steps=3, lr_pose=0.05, lr_quat=0.02, rewards_th=1e9, vis_wps_dist=0.0)
    out = {"losses": np.asarray(res.losses, dtype=np.float64), "steps": res.steps_taken}
    for name, m in (("a", a), ("b", b)):
        out[f"{name}.poses"], out[f"{name}.quats"] = m.poses.detach().clone(), m.quats.detach().clone()
    return out


# ================================================================================ the C hosts' pieces

def pieces_inputs(seed):
    rng = np.random.default_rng(1500 + seed)
    W, step = 2 * W5 + 1, 2
    n_eval = (W - 1) // step + 1
    p, q = synth.make_path(W, optical=True, jitter_seed=7 + seed)
    p = p + f32(0.125 * seed)
    return {"poses0": p.astype(f32), "poses": (p + rng.uniform(-0.05, 0.05, p.shape)).astype(f32), "quats": q.astype(f32),
            "pge": (rng.standard_normal((n_eval, 3)) * 0.01).astype(f32), "qge": (rng.standard_normal((n_eval, 4)) * 0.01).astype(f32),
            "scalars": f32([0.5 + 0.01 * seed, 1.7, -0.1, 0.0]), "params": rng.standard_normal(259).astype(f32),
            "grads": rng.standard_normal(259).astype(f32)}


@case("c_host_pieces", pieces_inputs)
def _pieces(d):
    L = _L()
    dev = d["poses"].device
    W, step = d["poses"].shape[0], 2
    n_eval = d["pge"].shape[0]
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)   # noqa: E731
    out = {}
    # gathers
    pe, qe = e(n_eval, 3), e(n_eval, 4)
    _ok(L.tohip_gather_waypoints(_p(d["poses"]), _p(d["quats"]), n_eval, step, _p(pe), _p(qe), _s()), "gather_waypoints")
    out["gather_waypoints poses"], out["gather_waypoints quats"] = pe, qe
    pe2, qe2 = e(n_eval, 3), e(n_eval, 4)
    _ok(L.tohip_gather_waypoints_multi(_p(d["poses"]), _p(d["quats"]), W, 1, n_eval, step, _p(pe2), _p(qe2), _s()), "gather_waypoints_multi")
    out["gather_waypoints_multi poses"], out["gather_waypoints_multi quats"] = pe2, qe2
    rows = e(n_eval, 3)
    _ok(L.tohip_rows_strided(_p(d["poses"]), n_eval, 3, step, 0, _p(rows), _s()), "rows_strided gather")
    scat = z(W, 4)
    _ok(L.tohip_rows_strided(_p(d["qge"]), n_eval, 4, step, 1, _p(scat), _s()), "rows_strided scatter")
    out["rows_strided gather"], out["rows_strided scatter"] = rows, scat
    # Adam for one group, twice, and the early stop
    p, m, v = d["params"].clone(), z(259), z(259)
    for t in (1, 2):
        _ok(L.tohip_adam_step(_p(p), _p(d["grads"]), _p(m), _p(v), 259, 0.05, 0.9, 0.999, 1e-8, t, None, _s()), "adam_step")
    out["adam p"], out["adam m"], out["adam v"] = p, m, v
    state = z(8)
    for mean_r, smooth in ((0.5, 3.0), (0.65, 2.7)):
        sc = torch.tensor([mean_r, 1.0, 0.0, 0.0], device=dev)
        lt = torch.tensor([0.0, 0.0, 0.0, smooth, 0.0, 0.0, 0.0, 0.0], device=dev)
        _ok(L.tohip_early_stop(_p(sc), _p(lt), 1.2, 0.5, _p(state), 0, _s()), "early_stop")
    out["early_stop state"] = state
    # the fused step tail of one trajectory, twice
    A = dict(poses=d["poses"].clone(), quats=d["quats"].clone(), pg=e(W, 3), qg=e(W, 4), state=z(8), log=z(4, 8), mp=z(W, 3), vp=z(W, 3), mq=z(W, 4),
             vq=z(W, 4))
    for _ in range(2):
        _ok(L.tohip_traj_step_tail(_p(A["poses"]), _p(A["quats"]), _p(d["poses0"]), W, _p(d["pge"]), _p(d["qge"]), n_eval, step, _p(A["pg"]), _p(A["qg"]),
                                   _p(A["mp"]), _p(A["vp"]), _p(A["mq"]), _p(A["vq"]), 28.0, 0.05, 1e-6, 0.12, 0.05, 0.9, 0.999, 1e-8, 1e9, 1e9,
                                   _p(d["scalars"]), _p(A["log"]), _p(A["state"]), _s()), "traj_step_tail")
    for k, t in A.items():
        out[f"step_tail {k}"] = t
    # the regularisers alone
    terms, g = z(8), e(W, 3)
    _ok(L.tohip_traj_regularizers(_p(d["poses"]), _p(d["poses0"]), W, 28.0, 0.05, 1e-6, _p(d["scalars"]), _p(terms), _p(g), 0, None, None, _s()),
        "traj_regularizers")
    out["regularizers terms"], out["regularizers grad"] = terms[:4].clone(), g
    return out
