"""Thin torch-tensor wrappers over the C ABI (include/trajopt_hip.h).

PyTorch here is plumbing only: device memory, streams and autograd bookkeeping.  Every numeric
step of the hot path runs in libtrajopt_hip.so; nothing in this module computes on the CPU and
nothing falls back to torch ops when the library is missing.
"""
import collections
import ctypes

import numpy as np

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


def _dev_f32(t, device):
    return torch.as_tensor(t, dtype=torch.float32, device=device).contiguous()


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on a HIP device (got {t.device}); the visibility path has no CPU fallback")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _float_or_nan(v, cast=float):
    """float(cast(v)), or NaN where v cannot be one (cast=np.float32: rounded as the library is handed it)."""
    try:
        return float(cast(v))
    except (TypeError, ValueError):
        return float("nan")


def _check_float_rows(t, name, wording, cols, rows=None, empty=True):
    """t must be a floating tensor of shape (rows, cols) — any number of rows for None, none at all only with `empty` — otherwise
    ValueError '<name> must be <wording>, got <its shape, or its type>'."""
    if (not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != 2 or t.shape[1] != cols or (rows is not None and t.shape[0] != rows)
            or not (empty or t.shape[0])):
        raise ValueError(f"{name} must be {wording}, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")


def _sections(header_bytes, sections):
    """Byte offsets of a buffer's sections, each rounded up to 256 bytes, behind a header of header_bytes ("header": 0; none for 0)
    -> {name: offset, ..., "total": bytes}.  sections: ((name, nbytes), ...)."""
    out, o = ({"header": 0} if header_bytes else {}), header_bytes
    for name, nbytes in sections:
        out[name] = o
        o += (nbytes + 255) // 256 * 256
    out["total"] = o
    return out


def _model_cloud(m, what):
    """m's packed cloud where m is a ModelTraj (ValueError for a sharded one); anything else is handed back as it is."""
    if hasattr(m, "_cloud") and hasattr(m, "_shard"):
        if m._shard.kind == "points" or m._shard.world_size > 1 or m._shard.collective:
            raise ValueError(f"{what}: a sharded model (WaypointShard / PointShard) is not supported")
        return m._cloud
    return m


class PackedCloud:
    """The cloud in the kernels' layout (x|y|z, padded); built once per CLOUD (it is constant over an optimisation run:
    /root/reference/src/model.py:80,174) and shared by every model over it — the reference builds a model per message pair over the
    same map (/root/reference/src/trajectory_optimization.py:129-136): `ModelTraj(cloud, ...)` / `ModelTraj(points, ..., cloud=other)`
    take a packed cloud as it is.  `points` keeps the caller's (N,3) f32 tensor (the models' `.points`)."""

    def __init__(self, points, sort=True):
        _require_cuda(points, "points")
        pts = points.detach().to(torch.float32).contiguous()
        if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
            raise ValueError(f"points must be (N,3) with N>0, got {tuple(pts.shape)}")
        L = _lib.lib()
        self.points, self.sorted = pts, bool(sort)
        self.n = pts.shape[0]
        self.npad = L.tohip_padded_points(self.n)
        self.device = pts.device
        self.blob = torch.empty(L.tohip_packed_cloud_bytes(self.n), dtype=torch.uint8, device=pts.device)
        wsb = L.tohip_pack_workspace_bytes(self.n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=pts.device)
        with torch.cuda.device(pts.device):
            check(L.tohip_pack_cloud(ptr(pts), self.n, int(bool(sort)), ptr(self.blob), ptr(ws), wsb, stream_ptr()),
                  "tohip_pack_cloud")
        # views into the blob (for tests / debugging): sorted x|y|z and the permutation to the caller's order
        self.soa = self.blob[:12 * self.npad].view(torch.float32)
        self.perm = self.blob[12 * self.npad:16 * self.npad].view(torch.int32)
        inv0 = 16 * self.npad + 16 * (self.npad // 256)
        self.inv_perm = self.blob[inv0:inv0 + 4 * self.n].view(torch.int32)  # caller's index -> sorted position


def _sorted_rows(cloud):
    """The cloud's points as (N,3) rows in the PACKED order (row s = the caller's row perm[s]); built on first use, kept with the cloud
    (12 bytes per point).  The occlusion refresh culls THESE rows: a waypoint's kept indices are then positions of the packed order,
    ascending — its bit row is written run by run instead of bit by scattered bit, and the hull pass's gather walks memory in order."""
    t = getattr(cloud, "_sorted_rows", None)
    if t is None:
        t = cloud.points[cloud.perm[:cloud.n].long()].contiguous() if cloud.sorted else cloud.points
        cloud._sorted_rows = t
    return t


class Camera:
    """Host-side camera constants (struct tohip_camera)."""

    def __init__(self, K, img_width, img_height, min_dist=1.0, max_dist=5.0, eps=1e-6):
        Kh = torch.as_tensor(K, dtype=torch.float32).detach().cpu().reshape(9).tolist()
        self.c = _lib.make_camera(Kh, img_width, img_height, min_dist, max_dist, eps)
        self.eps = float(eps)

    def ref(self):
        return ctypes.byref(self.c)


class CameraRig:
    """Multi-camera rig extrinsics on the device (struct tohip_rig)."""

    def __init__(self, rig_quats, rig_trans, device):
        self.q = _dev_f32(rig_quats, device)
        self.t = _dev_f32(rig_trans, device) if rig_trans is not None else torch.zeros_like(self.q[:, :3]).contiguous()
        self.n_cams = self.q.shape[0]
        self.c = _lib.Rig(self.n_cams, self.q.data_ptr(), self.t.data_ptr())

    def ref(self):
        return ctypes.byref(self.c)


_NULL_RIG = ctypes.POINTER(_lib.Rig)()


class TrajWorkspace:
    """Scratch + step state of the ModelTraj kernels.  Zero-filled once (the C ABI's contract); `generation` counts the
    forwards that used it — the backward of a step must find the state its own forward left (model.py checks)."""

    def __init__(self, cloud, n_virtual, n_traj=1):
        self.bytes = _lib.lib().tohip_traj_workspace_bytes_multi(cloud.n, n_virtual, n_traj)
        self.buf = torch.zeros(self.bytes, dtype=torch.uint8, device=cloud.device)
        self.n_virtual, self.n_traj = n_virtual, n_traj
        self.generation = 0


DENSE = _lib.CONSTANTS["TOHIP_TRAJ_DENSE"]


def _rig_ref(rig):
    return rig.ref() if rig is not None else _NULL_RIG


# The two launches the wrappers below share with WaypointShardStep.step (which hands in buffers allocated once); the caller has made
# the cloud's device current.  Here and in the wrappers a prior selects the _prior twin of an entry, which takes the same arguments
# and prior_buf after them.

def _forward(c, poses, quats, W, traj_offsets, B, cam, rig_ref, flags, occ, lo_sum, minmax, rewards_half, ws, stream):
    ws.generation += 1
    check(_lib.lib().tohip_traj_forward_multi(ptr(c.blob), c.n, ptr(poses), ptr(quats), W, ptr(traj_offsets), B, cam.ref(), rig_ref, flags,
                                              ptr(occ), ptr(lo_sum), ptr(minmax), ptr(rewards_half), ptr(ws.buf), ws.bytes, stream),
          "tohip_traj_forward_multi")


def _reward_backward(c, W, cam, rig_ref, flags, occ, lo_sum, prefilled, rewards, scalars, gout, pg, qg, ws, prior, stream):
    L = _lib.lib()
    args = (ptr(c.blob), c.n, W, cam.ref(), rig_ref, flags, ptr(occ), ptr(lo_sum), cam.eps, prefilled, ptr(rewards), ptr(scalars), ptr(gout),
            ptr(pg), ptr(qg), ptr(ws.buf), ws.bytes)
    if prior is None:
        check(L.tohip_traj_reward_backward(*args, stream), "tohip_traj_reward_backward")
    else:
        check(L.tohip_traj_reward_backward_prior(*args, ptr(prior.buf), stream), "tohip_traj_reward_backward_prior")


def traj_forward(cloud, poses, quats, cam, ws, rig=None, flags=0, occ=None, lo_sum=None, minmax=None, rewards_half=None,
                 traj_offsets=None):
    """-> (lo_sum[npad] in packed order (first N valid), minmax[V,2]) for the given waypoints (this rank's shard).
    Leaves the step's state in `ws` for traj_backward.  rewards_half: optional (N,) f32 tensor filled with 0.5 on the way
    (hand it to traj_reward as `rewards=` with prefilled=True).
    traj_offsets: several trajectories over one cloud in one pass — `poses` (W,3) / `quats` (W,4) hold their waypoints end to end,
    `traj_offsets` (B+1 int32 on the device) where each starts; lo_sum is then (B, npad) and ws = TrajWorkspace(cloud, V, B)."""
    W = poses.shape[0]
    C = rig.n_cams if rig is not None else 1
    B = traj_offsets.numel() - 1 if traj_offsets is not None else 1
    if lo_sum is None:   # one trajectory: (npad,); the trajectories of traj_offsets: (B, npad)
        lo_sum = torch.empty((B, cloud.npad) if traj_offsets is not None else cloud.npad, dtype=torch.float32, device=cloud.device)
    if minmax is None:
        minmax = torch.empty((W * C, 2), dtype=torch.float32, device=cloud.device)
    with torch.cuda.device(cloud.device):
        _forward(cloud, poses, quats, W, traj_offsets, B, cam, _rig_ref(rig), int(flags), occ, lo_sum, minmax, rewards_half, ws, stream_ptr())
    return lo_sum, minmax


def traj_reward(cloud, lo_sum, cam, ws, rewards=None, scalars=None, prefilled=False, prior=None):
    """-> (rewards[N], scalars[4] = mean, loss_vis, dloss/dreward, -).  prefilled: `rewards` holds 0.5 everywhere (traj_forward's
    rewards_half): only the others are stored.  A (B, npad) lo_sum (traj_forward with traj_offsets): rewards (B,N), scalars (B,4).
    prior: a LogOddsPrior over the cloud (one trajectory, not prefilled): rewards = sigmoid(lo_sum + prior)."""
    lead = tuple(lo_sum.shape[:-1])
    if rewards is None:
        rewards = torch.empty((*lead, cloud.n), dtype=torch.float32, device=cloud.device)
    if scalars is None:
        scalars = torch.empty((*lead, 4), dtype=torch.float32, device=cloud.device)  # all four written by the kernel
    L, args = _lib.lib(), (ptr(cloud.blob), ptr(lo_sum), cloud.n)
    rest = (cam.eps, int(bool(prefilled)), ptr(rewards), ptr(scalars), ptr(ws.buf), ws.bytes)
    with torch.cuda.device(cloud.device):
        if prior is None:
            check(L.tohip_traj_reward_multi(*args, lead[0] if lead else 1, *rest, stream_ptr()), "tohip_traj_reward_multi")
        else:
            check(L.tohip_traj_reward_prior(*args, *rest, ptr(prior.buf), stream_ptr()), "tohip_traj_reward_prior")
    return rewards, scalars


def traj_backward(cloud, n_wps, cam, ws, lo_sum, grad_rewards=None, scalars=None, gout=None, rig=None, flags=0, occ=None, n_traj=1,
                  prior=None):
    """Gradients of the step whose traj_forward last used `ws` (same cloud, n_wps, rig, flags, occ).
    lo_sum: the (all-reduced) log-odds vector in packed order, as returned by traj_forward.  n_traj: the number of trajectories of
    traj_forward's traj_offsets (gout: (B,) dL/d loss_vis per trajectory); the gradients are (n_wps,3), (n_wps,4) of all of them.
    prior: the LogOddsPrior the rewards were taken with (one trajectory): d reward / d lo_sum = r (1 - r) at lo_sum + prior."""
    pg = torch.empty((n_wps, 3), dtype=torch.float32, device=cloud.device)
    qg = torch.empty((n_wps, 4), dtype=torch.float32, device=cloud.device)
    L, args = _lib.lib(), (ptr(cloud.blob), cloud.n, n_wps)
    rest = (cam.ref(), _rig_ref(rig), int(flags), ptr(occ), ptr(lo_sum), ptr(grad_rewards), ptr(scalars), ptr(gout), ptr(pg), ptr(qg),
            ptr(ws.buf), ws.bytes)
    with torch.cuda.device(cloud.device):
        if prior is None:
            check(L.tohip_traj_backward_multi(*args, n_traj, *rest, stream_ptr()), "tohip_traj_backward_multi")
        else:
            check(L.tohip_traj_backward_prior(*args, *rest, ptr(prior.buf), stream_ptr()), "tohip_traj_backward_prior")
    return pg, qg


def traj_reward_backward(cloud, n_wps, cam, ws, lo_sum, gout, rewards=None, prefilled=False, rig=None, flags=0, occ=None, prior=None):
    """traj_reward + traj_backward of the fused visibility loss in two launches instead of three.
    -> (rewards[N], scalars[4], poses_grad (n_wps,3), quats_grad (n_wps,4)).  prior: as traj_reward's (not prefilled)."""
    if rewards is None:
        rewards = torch.empty(cloud.n, dtype=torch.float32, device=cloud.device)
    scalars = torch.empty(4, dtype=torch.float32, device=cloud.device)
    pg = torch.empty((n_wps, 3), dtype=torch.float32, device=cloud.device)
    qg = torch.empty((n_wps, 4), dtype=torch.float32, device=cloud.device)
    with torch.cuda.device(cloud.device):
        _reward_backward(cloud, n_wps, cam, _rig_ref(rig), int(flags), occ, lo_sum, int(bool(prefilled)), rewards, scalars, gout, pg, qg, ws,
                         prior, stream_ptr())
    return rewards, scalars, pg, qg


def traj_forward_backward(cloud, poses, quats, cam, ws, gout, rig=None, flags=0, occ=None, lo_sum=None, minmax=None, rewards=None,
                          traj_offsets=None):
    """The whole step of the fused visibility loss when no collective sits between forward and backward (tohip_traj_forward_backward,
    five launches).  -> (rewards[N], scalars[4], poses_grad (W,3), quats_grad (W,4), lo_sum[npad] packed order, minmax[V,2]).
    traj_offsets: B trajectories laid end to end (traj_forward's layout; gout: (B,) dL/d loss_vis each): rewards (B,N),
    scalars (B,4), lo_sum (B,npad)."""
    W = poses.shape[0]
    C = rig.n_cams if rig is not None else 1
    B = traj_offsets.numel() - 1 if traj_offsets is not None else 1
    lead = (B,) if traj_offsets is not None else ()   # the per-trajectory outputs' leading shape
    dev = cloud.device
    if lo_sum is None:
        lo_sum = torch.empty((*lead, cloud.npad), dtype=torch.float32, device=dev)
    if minmax is None:
        minmax = torch.empty((W * C, 2), dtype=torch.float32, device=dev)
    if rewards is None:
        rewards = torch.empty((*lead, cloud.n), dtype=torch.float32, device=dev)
    scalars = torch.empty((*lead, 4), dtype=torch.float32, device=dev)
    pg = torch.empty((W, 3), dtype=torch.float32, device=dev)
    qg = torch.empty((W, 4), dtype=torch.float32, device=dev)
    ws.generation += 1
    with torch.cuda.device(dev):
        check(_lib.lib().tohip_traj_forward_backward_multi(ptr(cloud.blob), cloud.n, ptr(poses), ptr(quats), W, ptr(traj_offsets), B, cam.ref(),
                                                           _rig_ref(rig), int(flags), ptr(occ), ptr(lo_sum), ptr(minmax), ptr(rewards),
                                                           ptr(scalars), ptr(gout), ptr(pg), ptr(qg), ptr(ws.buf), ws.bytes, stream_ptr()),
              "tohip_traj_forward_backward_multi")
    return rewards, scalars, pg, qg, lo_sum, minmax


class PointShardStep:
    """One point-sharded visibility step (tohip_traj_pshard_*; distributed.PointShard): this rank's part of the cloud, all the
    waypoints, two small collectives.  Buffers are allocated once; step(poses, quats) -> (rewards of this rank's points, scalars
    (4: mean reward of ALL points, loss_vis, d loss_vis / d reward, -), poses_grad (W,3), quats_grad (W,4)) — scalars and
    gradients identical on every rank (gradients for dL/d loss_vis = 1)."""

    def __init__(self, cloud, n_global, n_wps, cam, ws, shard, rig=None, flags=0):
        L = _lib.lib()
        self.cloud, self.n_global, self.n_wps, self.cam, self.ws, self.shard, self.rig, self.flags = cloud, int(n_global), int(n_wps), cam, ws, shard, rig, int(flags)
        dev = cloud.device
        C = rig.n_cams if rig is not None else 1
        V = n_wps * C
        f32 = dict(dtype=torch.float32, device=dev)
        self.lo_sum, self.minmax = torch.empty(cloud.npad, **f32), torch.empty((V, 2), **f32)
        self.rewards, self.scalars = torch.empty(cloud.n, **f32), torch.empty(4, **f32)
        self.pg, self.qg = torch.empty((n_wps, 3), **f32), torch.empty((n_wps, 4), **f32)
        self.partial = torch.empty(L.tohip_traj_pshard_partial_count(V), dtype=torch.float64, device=dev)
        words, n_words = ctypes.c_void_p(), ctypes.c_int64()
        check(L.tohip_traj_extrema_view(cloud.n, V, ptr(ws.buf), ws.bytes, ctypes.byref(words), ctypes.byref(n_words)), "tohip_traj_extrema_view")
        off = words.value - ws.buf.data_ptr()
        self.extrema = ws.buf[off:off + 4 * n_words.value].view(torch.int32)   # the workspace's own words: reduced in place
        self.rig_ref = _rig_ref(rig)

    def step(self, poses, quats, flags_extra=0):
        """flags_extra: TOHIP_TRAJ_STRIDE bits (the evaluated waypoints as every step-th row of poses / quats, read in place)."""
        L, c, ws = _lib.lib(), self.cloud, self.ws
        with torch.cuda.device(c.device):
            s = stream_ptr()
            check(L.tohip_traj_pshard_pass1(ptr(c.blob), c.n, self.n_global, ptr(poses), ptr(quats), self.n_wps, self.cam.ref(), self.rig_ref,
                                            self.flags | int(flags_extra), None, ptr(self.lo_sum), ptr(self.rewards), ptr(ws.buf), ws.bytes, s), "tohip_traj_pshard_pass1")
            ws.generation += 1
            self.shard.allreduce_max(self.extrema)      # collective 1: the waypoints' extrema over all points (16 B per virtual waypoint)
            check(L.tohip_traj_pshard_local(ptr(c.blob), c.n, self.n_global, self.n_wps, self.cam.ref(), self.rig_ref, self.flags, None,
                                            ptr(self.lo_sum), ptr(self.minmax), ptr(self.rewards), ptr(self.partial), ptr(ws.buf), ws.bytes, s),
                  "tohip_traj_pshard_local")
            self.shard.allreduce_sum(self.partial)      # collective 2: the sums everything after is linear in (40 doubles per virtual waypoint)
            check(L.tohip_traj_pshard_finish(c.n, self.n_global, self.n_wps, self.cam.ref(), self.rig_ref, ptr(self.partial), None,
                                             ptr(self.scalars), ptr(self.pg), ptr(self.qg), ptr(ws.buf), ws.bytes, s), "tohip_traj_pshard_finish")
        return self.rewards, self.scalars, self.pg, self.qg


class WaypointShardStep:
    """One waypoint-sharded visibility step (distributed.WaypointShard, or one process with every waypoint): this rank's range
    [lo, hi) = shard.bounds(n_wps) of the evaluated waypoints over the whole cloud, ONE all-reduce of the log-odds vector between
    forward and reward, ONE (n_wps, 7) all-reduce of the gradient rows.  Every rank issues both in that order, a rank that owns no
    waypoint included.  `ws` serves max(hi - lo, 1) waypoints.

    step() is the launch-only loop's step over buffers allocated once (as PointShardStep.step: gradients for dL/d loss_vis = 1);
    forward() / backward() are an autograd node's two halves, with fresh outputs per call."""

    def __init__(self, cloud, n_wps, cam, ws, shard, rig=None, flags=0):
        self.cloud, self.n_wps, self.cam, self.ws, self.shard, self.rig, self.flags = cloud, int(n_wps), cam, ws, shard, rig, int(flags)
        self.lo, self.hi = shard.bounds(self.n_wps)
        n_loc = max(self.hi - self.lo, 1)
        f32 = dict(dtype=torch.float32, device=cloud.device)
        self.lo_sum, self.minmax = torch.empty(cloud.npad, **f32), torch.empty((n_loc * (rig.n_cams if rig is not None else 1), 2), **f32)
        self.rewards, self.scalars = torch.empty(cloud.n, **f32), torch.zeros(4, **f32)
        self.pg_loc, self.qg_loc = torch.empty((n_loc, 3), **f32), torch.empty((n_loc, 4), **f32)
        self.g = torch.zeros((self.n_wps, 7), **f32)   # rows outside this rank's range stay zero
        self.pg, self.qg = torch.empty((self.n_wps, 3), **f32), torch.empty((self.n_wps, 4), **f32)
        self.gout = torch.ones(1, **f32)
        self.rig_ref = _rig_ref(rig)

    def step(self, poses, quats, flags_extra=0, occ=None, prior=None):
        """poses / quats: the whole trajectory, read in place; flags_extra: TOHIP_TRAJ_STRIDE bits (the evaluated waypoints are every
        s-th row, this rank's first at row lo * s).  occ: the occlusion rows of this rank's waypoints.  prior: a LogOddsPrior (the same
        on every rank; added after the all-reduce).  -> (rewards, scalars, poses_grad (n_wps,3), quats_grad (n_wps,4)), the same on
        every rank."""
        c, ws, n_loc = self.cloud, self.ws, self.hi - self.lo
        at = self.lo * (((int(flags_extra) >> 8) & 0xffff) + 1)
        with torch.cuda.device(c.device):
            s = stream_ptr()
            if n_loc:
                # (with a prior every reward is stored: no 1/2 prefill)
                _forward(c, poses[at:], quats[at:], n_loc, None, 1, self.cam, self.rig_ref, self.flags | int(flags_extra), occ, self.lo_sum,
                         self.minmax, self.rewards if prior is None else None, ws, s)
            else:
                self.lo_sum.zero_()
            allreduce_log_odds(self.shard, c, ws, self.lo_sum, local=n_loc > 0)
            if n_loc:
                # rewards, their mean and the loss scalars share the backward's first launch
                _reward_backward(c, n_loc, self.cam, self.rig_ref, self.flags, occ, self.lo_sum, int(prior is None), self.rewards, self.scalars,
                                 self.gout, self.pg_loc, self.qg_loc, ws, prior, s)
                self.g[self.lo:self.hi, :3], self.g[self.lo:self.hi, 3:] = self.pg_loc, self.qg_loc
            else:
                traj_reward(c, self.lo_sum, self.cam, ws, self.rewards, self.scalars, prior=prior)
            self.shard.allreduce_sum(self.g)
            self.pg.copy_(self.g[:, :3])
            self.qg.copy_(self.g[:, 3:])
            self.g.zero_()   # the other ranks' rows must be zero again before the next sum
        return self.rewards, self.scalars, self.pg, self.qg

    def forward(self, ps, qs, occ=None, prior=None):
        """ps / qs: this rank's evaluated waypoints (rows lo:hi, contiguous).  -> (lo_sum, rewards, scalars); the step's state stays
        in the workspace for backward(), which needs ws.generation as it is now.  prior: a LogOddsPrior, added to the all-reduced
        log-odds where the rewards are taken (every reward stored: no 1/2 prefill)."""
        c = self.cloud
        local = self.hi > self.lo
        half = torch.empty(c.n, dtype=torch.float32, device=c.device) if local and prior is None else None
        if local:
            lo_sum, _ = traj_forward(c, ps, qs, self.cam, self.ws, self.rig, flags=self.flags, occ=occ, rewards_half=half)
        else:
            lo_sum = torch.zeros(c.npad, dtype=torch.float32, device=c.device)
        allreduce_log_odds(self.shard, c, self.ws, lo_sum, local=local)
        rewards, scalars = traj_reward(c, lo_sum, self.cam, self.ws, rewards=half, prefilled=half is not None, prior=prior)
        return lo_sum, rewards, scalars

    def backward(self, ps, qs, occ, gen, lo_sum, upstream, prior=None, unit_sums=False):
        """-> the all-reduced gradient rows (n_wps,3), (n_wps,4) of the forward that left the workspace at generation `gen`.
        upstream: traj_backward's upstream keyword arguments, or None when no gradient reaches this rank's visibility term (the
        all-reduce is joined all the same).  If another forward has used the workspace since, that state is rebuilt first — same
        inputs, same bits.  prior: the forward's LogOddsPrior or None.  unit_sums (with the fused visibility loss's upstream): the
        sums are taken with unit dL/d reward and scaled once per waypoint (traj_reward_backward, the rewards taken again) — the
        arithmetic of the one-call step, whose bits a prior model without collective or occlusion rows keeps for a zero prior."""
        g = torch.zeros((self.n_wps, 7), dtype=torch.float32, device=lo_sum.device)
        if upstream is not None and self.hi > self.lo:
            if self.ws.generation != gen:
                traj_forward(self.cloud, ps, qs, self.cam, self.ws, self.rig, flags=self.flags, occ=occ)
            if unit_sums and "gout" in upstream:
                _, _, pg, qg = traj_reward_backward(self.cloud, ps.shape[0], self.cam, self.ws, lo_sum, upstream["gout"], rig=self.rig,
                                                    flags=self.flags, occ=occ, prior=prior)
            else:
                pg, qg = traj_backward(self.cloud, ps.shape[0], self.cam, self.ws, lo_sum, rig=self.rig, flags=self.flags, occ=occ,
                                       prior=prior, **upstream)
            g[self.lo:self.hi, :3], g[self.lo:self.hi, 3:] = pg, qg
        g = self.shard.allreduce_sum(g)
        return g[:, :3], g[:, 3:]


def allreduce_log_odds(shard, cloud, ws, lo_sum, local=True):
    """The one data-path collective of a waypoint-sharded step: the sum of the ranks' partial log-odds vectors, in
    place.  With shard.compact only the slots some rank's forward listed as candidates travel (tohip_traj_candidate_flags ...
    tohip_slots_pack): the vector is exactly zero elsewhere on every rank.  local=False: this rank ran no forward over `ws` (it
    holds no waypoint): its vector is zero and it lists nothing."""
    if not (shard.compact and shard.collective):
        return shard.allreduce_sum(lo_sum)
    L = _lib.lib()
    dev = cloud.device
    nslots = cloud.npad // 256
    flags = torch.zeros(nslots, dtype=torch.int32, device=dev)
    prefix = torch.empty(nslots + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if local:
            check(L.tohip_traj_candidate_flags(cloud.n, ws.n_virtual, ws.n_traj, ptr(ws.buf), ws.bytes, ptr(flags), stream_ptr()), "tohip_traj_candidate_flags")
        shard.allreduce_max(flags)
        check(L.tohip_slot_flags_prefix(ptr(flags), cloud.n, ptr(prefix), stream_ptr()), "tohip_slot_flags_prefix")
        count = int(prefix[nslots].item())   # the step's one host read: the union's size is the message's
        if count == 0:
            return lo_sum
        buf = getattr(ws, "_compact", None)
        if buf is None or buf.numel() < count * 256:
            buf = ws._compact = torch.empty(max(count * 256 * 2, 1 << 16), dtype=torch.float32, device=dev)
        check(L.tohip_slots_pack(ptr(flags), ptr(prefix), cloud.n, ptr(lo_sum), ptr(buf), count, 1, stream_ptr()), "tohip_slots_pack")
        shard.allreduce_sum(buf[:count * 256])
        check(L.tohip_slots_pack(ptr(flags), ptr(prefix), cloud.n, ptr(lo_sum), ptr(buf), count, 0, stream_ptr()), "tohip_slots_pack")
    return lo_sum


def check_clearance(radius, weight):
    """The clearance term's settings: radius > 0 and weight >= 0, both finite (ValueError otherwise)."""
    r, w = float(radius) if radius is not None else float("nan"), float(weight)
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError(f"clearance_weight must be a finite number >= 0, got {weight!r}")
    if w > 0.0 and not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"clearance_radius must be a finite number > 0 when clearance_weight > 0, got {radius!r}")
    return r, w


CLEARANCE_MODES = ("waypoints", "segments")
CLEARANCE_SEGMENTS = _lib.CONSTANTS["TOHIP_TRAJ_CLEARANCE_SEGMENTS"]   # the flag bit of tohip_traj_loss / tohip_traj_opt


def check_clearance_mode(mode):
    """The clearance term's mode: 'waypoints' (each waypoint's distance) or 'segments' (each segment's); ValueError otherwise."""
    if mode not in CLEARANCE_MODES:
        raise ValueError(f"clearance_mode must be one of {CLEARANCE_MODES}, got {mode!r}")
    return mode


def check_prior(prior, n, device=None, name="prior_log_odds"):
    """A log-odds prior for n points: an (n,) floating tensor, finite and >= 0 (on `device` when one is given) -> it as a contiguous
    float32 tensor; ValueError otherwise.  >= 0 is the model's own range (p is clipped at 1/2), where the integer reward sum is exact.
    name: what the messages call it (CoverageMap.integrate checks its row here)."""
    if not torch.is_tensor(prior) or not (prior.is_floating_point()):
        raise ValueError(f"{name} must be a floating-point tensor, got {type(prior).__name__}"
                         f"{'' if not torch.is_tensor(prior) else ' of ' + str(prior.dtype)}")
    if prior.dim() != 1 or prior.shape[0] != n:
        raise ValueError(f"{name} must have shape ({n},) (one entry per point), got {tuple(prior.shape)}")
    dev = torch.device(device) if device is not None else None
    if dev is not None and (prior.device.type != dev.type or (dev.index is not None and prior.device.index != dev.index)):
        raise ValueError(f"{name} lives on {prior.device}, {'the model' if name == 'prior_log_odds' else 'the map'} on {device}")
    p = prior.detach().to(torch.float32).contiguous()
    if not bool(torch.isfinite(p).all()):
        raise ValueError(f"{name} must be finite (NaN or inf found)")
    if not bool((p >= 0).all()):
        raise ValueError(f"{name} must be >= 0 (a negative entry found): the prior is log-odds of coverage, p >= 1/2")
    return p


class LogOddsPrior:
    """A per-point log-odds prior over a packed cloud, in the kernels' form (tohip_traj_prior_build: the prior and sigmoid(prior) in
    packed order, the fixed-point sums the reward starts from).  `values`: the (N,) f32 prior in the caller's order."""

    def __init__(self, cloud, values):
        L = _lib.lib()
        self.values = check_prior(values, cloud.n, cloud.device)
        self.bytes = L.tohip_traj_prior_bytes(cloud.n)
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=cloud.device)
        status = torch.empty(1, dtype=torch.int32, device=cloud.device)
        with torch.cuda.device(cloud.device):
            check(L.tohip_traj_prior_build(ptr(cloud.blob), cloud.n, ptr(self.values), ptr(self.buf), self.bytes, ptr(status), stream_ptr()),
                  "tohip_traj_prior_build")
        if int(status.item()) != 0:   # (check_prior has seen the values already: the kernel's own word, read once per prior)
            raise ValueError("prior_log_odds must be finite and >= 0")


def traj_coverage(cloud, lo_sum, prior=None, clamp_max=None):
    """The fused log-odds map (N,) f32 in the caller's order: prior + lo_sum (lo_sum in packed order as traj_forward writes it;
    prior a LogOddsPrior or None), clamped to clamp_max when one is given (OctoMap's upper clamping threshold, >= 0)."""
    c = float("inf") if clamp_max is None else float(clamp_max)
    if not c >= 0.0:
        raise ValueError(f"clamp_max must be a number >= 0 or None, got {clamp_max!r}")
    out = torch.empty(cloud.n, dtype=torch.float32, device=cloud.device)
    with torch.cuda.device(cloud.device):
        check(_lib.lib().tohip_traj_coverage(ptr(cloud.blob), cloud.n, ptr(lo_sum), ptr(prior.buf) if prior is not None else None, c,
                                             ptr(out), stream_ptr()), "tohip_traj_coverage")
    return out


COVMAP_MODES = {"max": _lib.CONSTANTS["TOHIP_COVMAP_MAX"], "add": _lib.CONSTANTS["TOHIP_COVMAP_ADD"]}
COVMAP_MIN_CAPACITY = 16
COVMAP_INDEX_LIMIT = 1 << 20          # voxel indices lie in [-2^20, 2^20) per axis


def covmap_layout(capacity):
    """Byte offsets of a coverage map's buffer (include/trajopt_hip.h, tohip_covmap_bytes): a 256-byte header, then `capacity` slots
    of 16 bytes (uint64 key | f32 value | uint32 pending)."""
    return {"header": 0, "slots": 256, "slot_bytes": 16, "total": 256 + 16 * int(capacity)}


def check_covmap(origin, resolution, clamp_max=None, capacity=None):
    """A coverage map's settings: origin 3 finite numbers, resolution a finite number > 0, clamp_max None or a number >= 0, capacity
    None or an integer >= 1 -> (origin (3,) float32 array, resolution and clamp_max as float32-exact floats, capacity rounded up to a
    power of two >= COVMAP_MIN_CAPACITY or None); ValueError otherwise."""
    try:
        o = np.asarray(origin.detach().cpu() if torch.is_tensor(origin) else origin, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        o = np.zeros(0, dtype=np.float32)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"origin must be 3 finite numbers, got {origin!r}")
    r = _float_or_nan(resolution, np.float32)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"resolution must be a finite number > 0, got {resolution!r}")
    c = float("inf") if clamp_max is None else _float_or_nan(clamp_max, np.float32)
    if not c >= 0.0:
        raise ValueError(f"clamp_max must be a number >= 0 or None, got {clamp_max!r}")
    if capacity is not None:
        if not _is_int(capacity) or not 1 <= capacity <= 1 << 32:
            raise ValueError(f"capacity must be None or an integer in [1, 2^32], got {capacity!r}")
        capacity = max(COVMAP_MIN_CAPACITY, 1 << (int(capacity) - 1).bit_length())
    return o, r, c, capacity


def covmap_points(points_or_cloud, device, what="CoverageMap"):
    """The rows a coverage map keys: (N,3) points, a PackedCloud (its caller-order points) or a ModelTraj (its cloud's) -> (N,3) f32
    contiguous on `device`; ValueError for a sharded model, another shape or another device."""
    m = _model_cloud(points_or_cloud, what)
    if isinstance(m, PackedCloud):
        m = m.points
    if not torch.is_tensor(m) or not m.is_floating_point() or m.dim() != 2 or m.shape[1] != 3:
        raise ValueError(f"{what}: points must be an (N,3) floating-point tensor, a PackedCloud or a ModelTraj, got "
                         f"{tuple(m.shape) if torch.is_tensor(m) else type(m).__name__}")
    dev = torch.device(device)
    if m.device.type != dev.type or (dev.index is not None and m.device.index != dev.index):
        raise ValueError(f"{what}: the points live on {m.device}, the map on {dev}")
    return m.detach().to(torch.float32).contiguous()


def check_covmap_rows(points_or_cloud, log_odds, device):
    """integrate's arguments: the points (covmap_points) and their (N,) log-odds row, finite and >= 0 (check_prior) -> (points, row)."""
    pts = covmap_points(points_or_cloud, device, "CoverageMap.integrate")
    return pts, check_prior(log_odds, pts.shape[0], device, name="log_odds")


def check_covmap_mode(mode):
    if mode not in COVMAP_MODES:
        raise ValueError(f"mode must be 'max' or 'add', got {mode!r}")
    return COVMAP_MODES[mode]


def check_covmap_merge(a, b):
    """Two maps that may be merged: same origin, same resolution, same device, not the same map (ValueError names what differs)."""
    if a is b:
        raise ValueError("CoverageMap.merge: a map cannot be merged into itself")
    if not np.array_equal(np.asarray(a.origin, dtype=np.float32), np.asarray(b.origin, dtype=np.float32)):
        raise ValueError(f"CoverageMap.merge: the maps' origins differ ({tuple(map(float, a.origin))} and {tuple(map(float, b.origin))})")
    if float(a.resolution) != float(b.resolution):
        raise ValueError(f"CoverageMap.merge: the maps' resolutions differ ({a.resolution} and {b.resolution})")
    if torch.device(a.device) != torch.device(b.device):
        raise ValueError(f"CoverageMap.merge: the maps live on {a.device} and {b.device}")


def resolve_prior(prior, points_or_cloud):
    """prior_log_odds as the models and select_views take it: a CoverageMap becomes its lookup over the points (a valid prior by
    construction: every value of a map is finite and >= 0); anything else is handed back as it is, for check_prior."""
    if isinstance(prior, CoverageMap):
        return prior.lookup(points_or_cloud)
    return prior


class CoverageMap:
    """A device-resident log-odds map keyed by voxel (covmap_kernels.hip): what has been seen, kept by POSITION, so that
    coverage computed over one cloud is the prior of any other.  A voxel is origin + [i, i + 1) x resolution per axis, i =
    floor((x - origin) / resolution) in float32; a point with a non-finite coordinate or an index outside [-2^20, 2^20) is skipped
    (read back as 0).  clamp_max: OctoMap's upper clamping threshold (None: none).  capacity: slots of the hash table to start with
    (rounded up to a power of two; it grows by itself, kept at most half full).  Everything observable — lookup, export, n_voxels,
    skipped — is bitwise the same in every run and under any permutation of the rows."""

    def __init__(self, origin=(0.0, 0.0, 0.0), resolution=0.1, clamp_max=None, capacity=None, device="cuda"):
        self.origin, self.resolution, clamp, capacity = check_covmap(origin, resolution, clamp_max, capacity)
        self.clamp_max = None if clamp_max is None else clamp
        self._clamp = clamp
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"a CoverageMap lives on a HIP device (got {self.device}); there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # runs of equal keys in consecutive rows are folded inside the wave before the table is touched (False: every row probes; the
        # same map either way).  On: 1.2-4 x faster on rows sorted by voxel, within 0.02 ms on unsorted ones (Measured)
        self.fold = True
        self.n_voxels = 0
        self.skipped = (0, 0)   # (points skipped for their position, rows skipped for their log-odds) over every integrate so far
        self.capacity, self.buf = 0, None
        self.buf = self._allocate(capacity if capacity is not None else 1 << 16)

    def _allocate(self, capacity):
        L = _lib.lib()
        nbytes = L.tohip_covmap_bytes(capacity)
        if nbytes == 0:
            raise ValueError(f"a coverage map of {capacity} slots is out of range")
        buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(L.tohip_covmap_init(ptr(buf), nbytes, capacity, (ctypes.c_float * 3)(*self.origin.tolist()), self.resolution, self._clamp,
                                      stream_ptr()), "tohip_covmap_init")
        self.capacity = capacity
        return buf

    def _sizes(self):
        return ptr(self.buf), self.buf.numel(), self.capacity

    def _grow(self, n_voxels):
        """A table that holds n_voxels at most half full, with the present contents (allocate, rehash)."""
        old = self._sizes()
        keep = self.buf
        self.buf = self._allocate(max(2 * self.capacity, 1 << (2 * int(n_voxels) - 1).bit_length()))
        h = (ctypes.c_int64 * 8)()
        with torch.cuda.device(self.device):
            check(_lib.lib().tohip_covmap_rehash(*self._sizes(), *old, h, stream_ptr()), "tohip_covmap_rehash")
        if int(h[0]) != self.n_voxels:   # (the call above returns an error on any status: this is the count itself)
            raise RuntimeError(f"CoverageMap: the grown table holds {int(h[0])} of {self.n_voxels} voxels")
        del keep

    def _call(self, call, n_new):
        """One integrate / merge: run it; when the table would end more than half full nothing was written — grow and run once more.
        n_new: the most voxels the call can add.  One synchronisation per run (the header)."""
        h = (ctypes.c_int64 * 8)()
        for attempt in range(2):
            with torch.cuda.device(self.device):
                rc = call(h)
            if rc != _lib.ENOSPC:
                break
            if attempt == 1:
                raise RuntimeError(f"CoverageMap: {int(h[3])} voxels do not fit {self.capacity} slots after growing")
            self._grow(int(h[3]) if not int(h[2]) & 2 else self.n_voxels + n_new)
        if rc == 0:   # (any other code: the header was not read, the count stands)
            self.n_voxels = int(h[0])
        return rc, h

    def integrate(self, points_or_cloud, log_odds, mode="max"):
        """Fold a log-odds row into the map: the observation of a voxel is the maximum over the rows that fall into it; then
        value = min(max(old, obs), clamp_max) (mode 'max': a fused row such as coverage_log_odds, which already holds the prior read
        from this map — integrating it twice changes nothing) or min(old + obs, clamp_max) ('add': an independent observation,
        fuse_log_odds' sum per voxel).  points_or_cloud: (N,3) points, a PackedCloud or a ModelTraj; log_odds: (N,) in the same
        order, finite and >= 0 (check_prior).  -> self."""
        m = check_covmap_mode(mode)
        pts, row = check_covmap_rows(points_or_cloud, log_odds, self.device)
        n = pts.shape[0]
        L = _lib.lib()
        rc, h = self._call(lambda h: L.tohip_covmap_integrate(*self._sizes(), ptr(pts), ptr(row), n, m, int(self.fold), h, stream_ptr()), n)
        check(rc, "tohip_covmap_integrate")
        self.skipped = (self.skipped[0] + int(h[4]), self.skipped[1] + int(h[5]))
        return self

    def lookup(self, points_or_cloud):
        """(N,) f32: the value of each point's voxel, 0.0 where the map holds none and for a skipped point — a valid prior_log_odds
        for that cloud.  One launch, nothing synchronises."""
        pts = covmap_points(points_or_cloud, self.device, "CoverageMap.lookup")
        out = torch.empty(pts.shape[0], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().tohip_covmap_lookup(*self._sizes(), ptr(pts), pts.shape[0], ptr(out), stream_ptr()), "tohip_covmap_lookup")
        return out

    def merge(self, other, mode="add"):
        """Every voxel of `other` (same origin and resolution) integrated as one observation: 'add' for an independent map (another
        robot's), 'max' for one that already contains this one.  -> self."""
        m = check_covmap_mode(mode)
        if not isinstance(other, CoverageMap):
            raise ValueError(f"CoverageMap.merge: a CoverageMap is needed, got {type(other).__name__}")
        check_covmap_merge(self, other)
        L = _lib.lib()
        rc, _ = self._call(lambda h: L.tohip_covmap_merge(*self._sizes(), *other._sizes(), m, h, stream_ptr()), other.n_voxels)
        check(rc, "tohip_covmap_merge")
        return self

    def export(self):
        """-> (centres (V,3) f32, values (V,) f32, keys (V,) int64) on the device, in ascending key order (x index highest)."""
        V = self.n_voxels
        keys = torch.empty(V, dtype=torch.int64, device=self.device)
        vals = torch.empty(V, dtype=torch.float32, device=self.device)
        ctr = torch.empty((V, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().tohip_covmap_export(*self._sizes(), V, ptr(keys), ptr(vals), ptr(ctr), stream_ptr()), "tohip_covmap_export")
        keys, order = torch.sort(keys)
        return ctr[order], vals[order], keys

    def header(self):
        """-> (words: 8 ints, geometry: origin x y z, resolution, clamp_max) as the device holds them; synchronises."""
        w, g = (ctypes.c_int64 * 8)(), (ctypes.c_float * 5)()
        with torch.cuda.device(self.device):
            check(_lib.lib().tohip_covmap_read_header(ptr(self.buf), w, g, stream_ptr()), "tohip_covmap_read_header")
        return list(w), list(g)


OCC_MAX_DIM = 2048        # voxels per axis of an occupancy grid
OCC_MAX_VOXELS = 1 << 31
LOS_MAX_SKIP = 8192
OCCLUSION_METHODS = (None, "hpr", "zbuffer", "voxel")


def check_occlusion(occlusion):
    """The models' and select_views' occlusion= value: None, 'hpr', 'zbuffer' or 'voxel'; ValueError otherwise."""
    if occlusion not in OCCLUSION_METHODS:
        raise ValueError(f"occlusion must be None, 'hpr' or 'zbuffer', or 'voxel', got {occlusion!r}")
    return occlusion


def check_los_skip(skip):
    """skip = (start_skip, end_skip): two integers in [0, LOS_MAX_SKIP] -> (int, int); ValueError otherwise."""
    try:
        s = tuple(skip)
    except TypeError:
        s = ()
    if len(s) != 2 or not all(_is_int(v) and 0 <= v <= LOS_MAX_SKIP for v in s):
        raise ValueError(f"skip must be two integers (start_skip, end_skip) in [0, {LOS_MAX_SKIP}], got {skip!r}")
    return int(s[0]), int(s[1])


def check_los(origin, resolution, dims, skip=(1, 1), a=None, b=None):
    """An occupancy grid's settings and a segment query's arguments, by name: origin 3 finite numbers, resolution a finite number > 0,
    dims three integers in [1, OCC_MAX_DIM] with at most 2^31 voxels, skip two integers in [0, LOS_MAX_SKIP], a and b (given
    together) floating tensors of one shape (R,3) on one device -> (origin (3,) float32 array, resolution as a float32-exact float,
    dims (nx, ny, nz), skip); ValueError otherwise.  Needs no GPU."""
    o, r, _, _ = check_covmap(origin, resolution)
    try:
        d = tuple(dims)
    except TypeError:
        d = ()
    if len(d) != 3 or not all(_is_int(v) and 1 <= v <= OCC_MAX_DIM for v in d):
        raise ValueError(f"dims must be three integers in [1, {OCC_MAX_DIM}], got {dims!r}")
    d = tuple(int(v) for v in d)
    if d[0] * d[1] * d[2] > OCC_MAX_VOXELS:
        raise ValueError(f"dims must hold at most 2^31 voxels, got {d} = {d[0] * d[1] * d[2]}")
    skip = check_los_skip(skip)
    if (a is None) != (b is None):
        raise ValueError("a and b must be given together")
    if a is not None:
        _check_float_rows(a, "a", "an (R,3) floating-point tensor", 3)
        _check_float_rows(b, "b", f"an (R,3) floating-point tensor with a's {a.shape[0]} rows", 3, rows=a.shape[0])
        if a.device != b.device:
            raise ValueError(f"a and b must live on one device, got {a.device} and {b.device}")
    return o, r, d, skip


def occupancy_extent(lo, hi, resolution, margin):
    """from_points' geometry from a cloud's f64 bounds -> (origin (3,) f32, dims): origin = r floor(lo / r) - margin r computed in
    f64 and cast to f32, dims = the voxels from there to hi plus the margin; ValueError names an extent the grid cannot hold."""
    r = _float_or_nan(resolution, np.float32)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"resolution must be a finite number > 0, got {resolution!r}")
    if not _is_int(margin) or not 0 <= margin <= OCC_MAX_DIM:
        raise ValueError(f"margin must be an integer in [0, {OCC_MAX_DIM}], got {margin!r}")
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("OccupancyGrid.from_points: the points have no finite bounding box")
    origin = (r * np.floor(lo / r) - margin * r).astype(np.float32)
    # (+ 2: the f32 origin and the f32 division may move a point on the far face by a voxel)
    ext = np.floor((hi - origin.astype(np.float64)) / r) + 2 + margin
    if (ext > OCC_MAX_DIM).any():
        raise ValueError(f"OccupancyGrid.from_points: an extent of {tuple(int(v) for v in ext)} voxels exceeds {OCC_MAX_DIM} per axis; "
                         "use a coarser resolution")
    dims = tuple(int(max(v, 1)) for v in ext)
    if dims[0] * dims[1] * dims[2] > OCC_MAX_VOXELS:
        raise ValueError(f"OccupancyGrid.from_points: {dims} holds more than 2^31 voxels; use a coarser resolution")
    return origin, dims


def _map_call(device, name, *args):
    """One call of the map layer's C entry `name` on `device`: the arguments, then the current stream; a failure raises by name."""
    with torch.cuda.device(device):
        check(getattr(_lib.lib(), name)(*args, stream_ptr()), name)


def _map_call0(device, name, *args):
    """_map_call for the entries with a reserved flags word behind the stream (0)."""
    with torch.cuda.device(device):
        check(getattr(_lib.lib(), name)(*args, stream_ptr(), 0), name)


class OccupancyGrid:
    """A dense occupancy bit grid on the device (occupancy_kernels.hip), filled from any number of clouds: voxel
    (i, j, k) is origin + [i, i+1) x [j, j+1) x [k, k+1) resolution, the index floor((x - origin) / resolution) in float32.  Around
    the grid lies an apron (indices -2048 .. 4095 per axis) in which everything is free; a position beyond it is out of range.
    Bits are only ever set: two inserts equal one insert of both clouds, in any row order."""

    def __init__(self, origin=(0.0, 0.0, 0.0), resolution=0.1, dims=(64, 64, 64), device="cuda"):
        self.origin, self.resolution, self.dims, _ = check_los(origin, resolution, dims)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"an OccupancyGrid lives on a HIP device (got {self.device}); there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        L = _lib.lib()
        self.geom = _lib.OccGeom((ctypes.c_float * 3)(*self.origin.tolist()), self.resolution, (ctypes.c_int32 * 3)(*self.dims))
        nbytes = L.tohip_occ_bytes(*self.dims)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.skipped = 0   # rows skipped over every insert so far
        _map_call(self.device, "tohip_occ_init", *self._sizes())

    @classmethod
    def from_points(cls, points_or_cloud, resolution=0.1, margin=2):
        """The grid around a cloud — (N,3) points, a PackedCloud or a ModelTraj — with `margin` free voxels on every side, the cloud
        inserted.  The origin is r floor(min / r) - margin r in f64, cast to f32.  One host read of the bounds."""
        m = _model_cloud(points_or_cloud, "OccupancyGrid.from_points")
        pts = m.points if isinstance(m, PackedCloud) else m
        if not torch.is_tensor(pts) or not pts.is_floating_point() or pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
            raise ValueError("OccupancyGrid.from_points: points must be an (N,3) floating-point tensor with N > 0, a PackedCloud or a "
                             f"ModelTraj, got {tuple(pts.shape) if torch.is_tensor(pts) else type(pts).__name__}")
        _require_cuda(pts, "points")
        p = pts.detach()
        fin = torch.where(torch.isfinite(p), p, torch.full_like(p, float("nan")))
        big = torch.finfo(p.dtype).max
        lo = torch.nan_to_num(fin, nan=big).amin(dim=0).double().cpu().numpy()
        hi = torch.nan_to_num(fin, nan=-big).amax(dim=0).double().cpu().numpy()
        if (lo > hi).any():
            raise ValueError("OccupancyGrid.from_points: the points have no finite bounding box")
        origin, dims = occupancy_extent(lo, hi, resolution, margin)
        g = cls(origin, resolution, dims, device=pts.device)
        g.insert(pts)
        return g

    def _sizes(self):
        return ptr(self.buf), self.buf.numel(), ctypes.byref(self.geom)

    def insert(self, points_or_cloud):
        """Set the voxel of every row; -> the number of rows skipped (a coordinate out of range or not finite, or a voxel outside
        dims).  One synchronisation (that count)."""
        pts = covmap_points(points_or_cloud, self.device, "OccupancyGrid.insert")
        skipped = ctypes.c_int64(0)
        _map_call(self.device, "tohip_occ_insert", *self._sizes(), ptr(pts), pts.shape[0], ctypes.byref(skipped))
        self.skipped += int(skipped.value)
        return int(skipped.value)

    def lookup(self, ijk):
        """(M,3) integer voxel indices -> (M,) uint8, 1 = occupied, 0 outside dims."""
        if not torch.is_tensor(ijk) or ijk.is_floating_point() or ijk.dtype == torch.bool or ijk.dim() != 2 or ijk.shape[1] != 3:
            raise ValueError(f"ijk must be an (M,3) integer tensor, got {tuple(ijk.shape) if torch.is_tensor(ijk) else type(ijk).__name__}")
        q = ijk.to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty(q.shape[0], dtype=torch.uint8, device=self.device)
        _map_call(self.device, "tohip_occ_lookup", *self._sizes(), ptr(q), q.shape[0], ptr(out))
        return out

    def dense(self):
        """The grid as a bool (nx, ny, nz) tensor, through lookup: for tests and small grids."""
        nx, ny, nz = self.dims
        ijk = torch.stack(torch.meshgrid(torch.arange(nx), torch.arange(ny), torch.arange(nz), indexing="ij"), dim=-1).reshape(-1, 3)
        return self.lookup(ijk.to(self.device)).view(nx, ny, nz).bool()

    def line_of_sight(self, a, b, skip=(1, 1), stats=None):
        """(R,) uint8 for the segments a[i] -> b[i] of world points: 1 clear, 0 blocked, 2 an endpoint out of range.  stats: a
        zero-filled (2,) int64 device tensor that receives (rays walked, voxels visited), or None."""
        _, _, _, (ss, es) = check_los(self.origin, self.resolution, self.dims, skip, a, b)
        a, b = covmap_points(a, self.device, "line_of_sight"), covmap_points(b, self.device, "line_of_sight")
        out = torch.empty(a.shape[0], dtype=torch.uint8, device=self.device)
        _map_call(self.device, "tohip_los_segments", *self._sizes(), ptr(a), ptr(b), a.shape[0], ss, es, ptr(out), ptr(stats))
        return out

    def cast(self, a, b, skip=(1, 0), stats=None):
        """Where does the segment a[i] -> b[i] stop?  -> (voxel (R,) int32, lam (R,) f32) (tohip_cast_segments, DESIGN.md 10 "Ray
        casts and depth scans"): the first voxel line_of_sight(a, b, skip) would call occupied as its linear index i + nx (j + ny k),
        -1 where the segment is clear, -2 where an endpoint is out of range; lam the parameter in [0, 1] at which the segment
        enters that voxel, 1 where clear, NaN where out of range.  With the default skip the end voxel itself is never tested.
        stats: a zero-filled (2,) int64 device tensor that receives (rays walked, voxels visited), or None."""
        _, _, _, (ss, es) = check_los(self.origin, self.resolution, self.dims, skip, a, b)
        a, b = covmap_points(a, self.device, "cast"), covmap_points(b, self.device, "cast")
        voxel = torch.empty(a.shape[0], dtype=torch.int32, device=self.device)
        lam = torch.empty(a.shape[0], dtype=torch.float32, device=self.device)
        _map_call(self.device, "tohip_cast_segments", *self._sizes(), ptr(a), ptr(b), a.shape[0], ss, es, ptr(voxel), ptr(lam), ptr(stats))
        return voxel, lam

    def empty_like(self):
        """An empty grid of this one's origin, resolution, dims and device: a free plane or a mask for it."""
        return OccupancyGrid(self.origin, self.resolution, self.dims, device=self.device)

    def reframed(self, shift=None, dims=None, centre=None):
        """This grid's content in another box of the same lattice -> a NEW grid (tohip_occ_transfer, DESIGN.md 10 "Re-framing and
        merging maps"); this one is untouched, and whatever holds it (a SpaceMap, a ClearanceField, ModelTraj(clearance_map=)) keeps
        it: such consumers are re-pointed or built anew after a re-frame.  Give exactly one of shift — three integers: new voxel v is
        old voxel v + shift, the new origin float32(float64(origin) + shift * float64(resolution)) — or centre, a world position
        whose voxel (the f32 index rule) becomes voxel dims // 2.  dims: the new box's (default: this one's).  What leaves the box is
        dropped, what enters it is empty.  The content moves by the voxel shift, not by re-inserting points.  One launch, nothing
        read back; `skipped` carries over."""
        s, d, origin = check_reframe(self, shift, dims, centre)
        out = OccupancyGrid(origin, self.resolution, d, device=self.device)
        _map_call(self.device, "tohip_occ_transfer", *self._sizes(), *out._sizes(), *s, XFER_MODES["copy"], None)
        out.skipped = self.skipped
        return out

    def _resample(self, src, affine, rule, mode, counts):
        keep, a, frac = _affine_arg(affine)
        _map_call0(self.device, "tohip_occ_resample", *src._sizes(), *self._sizes(), a, frac, RESAMPLE_OCC_RULES[rule], XFER_MODES[mode], ptr(counts))

    def transformed(self, pose, quat, origin=None, resolution=None, dims=None, like=None, rule="nearest", _plane_rule=None):
        """This grid's content under a rigid transform and, if asked, at a finer resolution -> a NEW grid (tohip_occ_resample, DESIGN.md
        10 "Resampling maps"); this one is only read.  pose (3,), quat (4,) wxyz: world_new = R(quat) world_old + pose, the pose of
        this grid's frame in the new one.  The new box: like= a map (its frame), or origin / resolution / dims (check_transform);
        by default the axis-aligned box around this box's transformed corners, its origin a multiple of the resolution.  rule
        'nearest': the bit of the voxel that holds the new voxel's centre — unbiased, and a wall one voxel thick may show pinholes;
        'cover': the OR over the 3 x 3 x 3 voxels around it — no set voxel is lost, walls stay shut and grow by up to a voxel.  One
        launch, nothing read back; `skipped` carries over."""
        frame, affine = check_transform(self, pose, quat, origin, resolution, dims, like, rule)
        out = OccupancyGrid(frame.origin, frame.resolution, frame.dims, device=self.device)
        out._resample(self, affine, _plane_rule or ("any" if rule == "cover" else "nearest"), "copy", None)
        out.skipped = self.skipped
        return out

    def merge(self, other, counts=None, pose=None, quat=None, rule="nearest", _plane_rule=None):
        """OR another grid into this one over the overlap of the two boxes, in place -> self; `other` is only read.  Without a pose
        the two share a lattice and the bits move by a voxel shift.  pose (3,), quat (4,) wxyz: the other grid's frame stands at
        world_self = R(quat) world_other + pose and is resampled (rule 'nearest' or 'cover', as transformed takes it; this grid
        must not be coarser than the other); an identity pose on this grid's lattice takes the shift path.  counts: a zero-filled
        (1,) int64 device tensor that receives += the bits that were not set before, or None.  One launch, nothing read back."""
        s, overlap, affine = check_merge_posed(self, other, None, pose, quat, rule)
        _check_counts(counts, 1, self.device)
        if affine is not None:
            self._resample(other, affine, _plane_rule or ("any" if rule == "cover" else "nearest"), "or", counts)
        elif overlap:
            _map_call(self.device, "tohip_occ_transfer", *other._sizes(), *self._sizes(), *s, XFER_MODES["or"], ptr(counts))
        return self

    def _coarsen(self, src, factor, offset, rule, mode, counts, veto=None):
        _map_call0(self.device, "tohip_occ_coarsen", *src._sizes(), ptr(veto.buf) if veto is not None else None, *self._sizes(), factor, *offset,
                   COARSEN_OCC_RULES[rule], XFER_MODES[mode], ptr(counts))

    def coarsened(self, factor=2, rule="any", anchor="origin", origin=None, dims=None, like=None, _veto=None):
        """This grid at `factor` times its voxel edge -> a NEW grid (tohip_occ_coarsen, DESIGN.md 10 "Coarsening maps"); this one is only
        read.  factor: an integer in [2, 8]; a coarse voxel's bit is the OR (rule 'any', the default: no set voxel is lost) or the AND
        (rule 'all': a voxel outside this grid counts 0) of its factor^3 children.  anchor 'origin': the coarse box starts at this
        grid's origin and holds ceil(n / factor) voxels an axis.  anchor 'world': the coarse lattice's planes lie at multiples of the
        coarse edge, so coarse grids of any sources on one fine lattice share a lattice and merge as they are.  origin / dims / like:
        another box (check_coarsen).  One launch, nothing read back; `skipped` carries over."""
        frame, o, rule = check_coarsen(self, factor, rule, anchor, origin, dims, like)
        out = OccupancyGrid(frame.origin, frame.resolution, frame.dims, device=self.device)
        out._coarsen(self, int(factor), o, rule, "copy", None, _veto)
        out.skipped = self.skipped
        return out

    def merge_fine(self, fine, rule="any", counts=None):
        """OR a FINER grid into this one, in place -> self; `fine` is only read.  The factor (2 .. 8) and the offset come from the two
        frames (check_merge_fine): this grid's resolution is a whole multiple of the other's and the origins lie a whole number of
        fine voxels apart.  Each of this grid's voxels takes the OR ('any') or AND ('all') of its children.  counts: a zero-filled
        (1,) int64 device tensor that receives += the bits that were not set before, or None.  One launch, nothing read back."""
        factor, o, rule = check_merge_fine(self, fine, None, rule)
        _check_counts(counts, 1, self.device)
        self._coarsen(fine, factor, o, rule, "or", counts)
        return self

    def carve(self, origins, points, max_range=None, stats=None, flags=None):
        """Treat this grid as a FREE PLANE (a set bit: "a ray passed through") and set the bit of every voxel the rays origins[i] ->
        points[i] cross, walked exactly as line_of_sight walks (tohip_occ_carve).  origins: (3,) / (1,3) for one origin
        shared by all rays, or (N,3).  A ray longer than max_range metres (None: no limit) is truncated to that length and carves all
        of it; any other ray is a hit and leaves its last voxel — the measured one — alone.  -> the number of rays skipped (an
        endpoint out of range or not finite); one synchronisation (that count).  stats: a zero-filled (3,) int64 device tensor that
        receives (rays walked, voxels visited, atomics issued); flags: an (N,) uint8 device tensor that receives 0 hit / 1 truncated
        / 2 skipped per ray.  Bits are only ever set: any split and order of the rays gives the same plane."""
        R = check_carve(origins, points, max_range, self.resolution)
        pts = covmap_points(points, self.device, "OccupancyGrid.carve")
        org = origins if torch.is_tensor(origins) else torch.as_tensor(np.asarray(origins, dtype=np.float32), device=self.device)
        org = covmap_points(org.reshape(-1, 3), self.device, "OccupancyGrid.carve")
        if flags is not None and (not torch.is_tensor(flags) or flags.dtype != torch.uint8 or flags.shape != (pts.shape[0],)
                                  or flags.device != self.device or not flags.is_contiguous()):
            raise ValueError(f"flags must be a contiguous ({pts.shape[0]},) uint8 tensor on {self.device}")
        skipped = ctypes.c_int64(0)
        _map_call(self.device, "tohip_occ_carve", *self._sizes(), ptr(org), 0 if org.shape[0] == 1 else 3, ptr(pts), pts.shape[0], R, ptr(flags),
                  ptr(stats), ctypes.byref(skipped))
        return int(skipped.value)

    def _count(self):
        """-> (the number of set bits, the workspace holding the blocks' offsets for export); the one synchronisation."""
        ws = torch.empty(_lib.lib().tohip_occ_export_workspace_bytes(*self.dims), dtype=torch.uint8, device=self.device)
        total = ctypes.c_int64(0)
        _map_call(self.device, "tohip_occ_count", *self._sizes(), ptr(ws), ws.numel(), ctypes.byref(total))
        return int(total.value), ws

    def count(self):
        """The number of set bits; synchronises."""
        return self._count()[0]

    def export(self):
        """The set bits listed -> (ijk (F,3) int32, centres (F,3) f32) on the device in ascending (word, bit) order — brick order, what
        a kernel gives without a sort; centre = origin + (i + 0.5) resolution per axis in f32.  One synchronisation (F)."""
        total, ws = self._count()
        ijk = torch.empty((total, 3), dtype=torch.int32, device=self.device)
        centres = torch.empty((total, 3), dtype=torch.float32, device=self.device)
        _map_call(self.device, "tohip_occ_export", *self._sizes(), ptr(ws), ws.numel(), total, total, ptr(ijk), ptr(centres))
        return ijk, centres


CARVE_MAX_RANGE = 6144 * 256   # of max_range in 1/256 voxel: the span of a grid and its apron


def check_carve(origins, points, max_range=None, resolution=0.1):
    """carve's arguments, by name: points an (N,3) floating tensor; origins a (3,) or (1,3) floating tensor or 3 numbers (one origin
    for all rays) or an (N,3) floating tensor on points' device; max_range None or a finite number of metres whose fixed-point form
    R = floor(float64(max_range) / float64(f32 resolution) * 256) lies in [1, 6144 * 256] -> R (0 for None); ValueError otherwise.
    Needs no GPU."""
    _check_float_rows(points, "points", "an (N,3) floating-point tensor", 3)
    n = points.shape[0]
    o = origins
    if not torch.is_tensor(o):
        try:
            o = torch.from_numpy(np.asarray(o, dtype=np.float32))
        except (TypeError, ValueError):
            o = None
    if o is None or not o.is_floating_point() or tuple(o.shape) not in ((3,), (1, 3), (n, 3)):
        raise ValueError("origins must be a (3,) or (1,3) floating-point tensor (one origin for all rays) or an (N,3) one with points' "
                         f"{n} rows, got {tuple(o.shape) if o is not None else type(origins).__name__}")
    if torch.is_tensor(origins) and origins.device != points.device:
        raise ValueError(f"origins and points must live on one device, got {origins.device} and {points.device}")
    if max_range is None:
        return 0
    m, r = _float_or_nan(max_range), float(np.float32(resolution))
    R = int(np.floor(m / r * 256.0)) if np.isfinite(m) and _is_real(max_range) else -1
    if not 1 <= R <= CARVE_MAX_RANGE:
        raise ValueError(f"max_range must be None or a finite number of metres between resolution / 256 and 6144 voxels ({6144 * r:g} m), "
                         f"got {max_range!r}")
    return R


def _is_real(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


class Frontier:
    """What SpaceMap.frontier returns: ijk (F,3) int32 voxel indices and points (F,3) f32 (their centres) on the device in brick
    order, grid (the mask as an OccupancyGrid: lookup, dense, export work on it) and n = F."""
    __slots__ = ("ijk", "points", "grid")

    def __init__(self, ijk, points, grid):
        self.ijk, self.points, self.grid = ijk, points, grid

    @property
    def n(self):
        return int(self.ijk.shape[0])


def _grid_difference(a, b):
    """Two OccupancyGrids' geometry compared -> None where origin, resolution, dims and device agree, else (what, a's, b's) of the first
    of these that differs."""
    for what, x, y in (("origin", tuple(map(float, a.origin)), tuple(map(float, b.origin))), ("resolution", a.resolution, b.resolution),
                       ("dims", a.dims, b.dims), ("device", a.device, b.device)):
        if x != y:
            return what, x, y
    return None


def _listed_plane(cls, like, name, head, tail):
    """An empty plane of `like`'s geometry, filled by the C entry `name` (head, the plane, tail) and listed -> cls(ijk, centres, plane)."""
    plane = like.empty_like()
    _map_call(like.device, name, *head, *plane._sizes(), *tail)
    return cls(*plane.export(), plane)


def check_space_planes(occupied, free):
    """A SpaceMap's two planes: OccupancyGrids of one origin, resolution, dims and device, not the same grid; ValueError names what
    differs."""
    for name, g in (("occupied", occupied), ("free", free)):
        if not isinstance(g, OccupancyGrid):
            raise ValueError(f"SpaceMap: {name} must be an ops.OccupancyGrid, got {type(g).__name__}")
    if free is occupied:
        raise ValueError("SpaceMap: free must not be the occupied grid itself")
    diff = _grid_difference(occupied, free)
    if diff:
        texts = {"origin": "the planes' origins differ ({} and {})", "resolution": "the planes' resolutions differ ({} and {})",
                 "dims": "the planes' dims differ ({} and {})", "device": "the planes live on {} and {}"}
        raise ValueError("SpaceMap: " + texts[diff[0]].format(*diff[1:]))


def check_min_unknown(min_unknown):
    if not _is_int(min_unknown) or not 1 <= min_unknown <= 6:
        raise ValueError(f"min_unknown must be an integer in [1, 6], got {min_unknown!r}")
    return int(min_unknown)


class SpaceMap:
    """The three-state map ("Free space and frontiers"): the caller's occupied grid — shared, not copied — and a free
    plane of the same geometry.  A voxel is occupied (2) where the occupied bit is set, else free (1) where a ray passed through, else
    unknown (0).  Bits are never cleared: this map has no moving obstacles (EvidenceMap, below, is the map that takes a voxel back
    and hands out the same planes); free space leaks through a wall sampled more sparsely than the voxel; the box's own boundary is
    not a frontier."""

    def __init__(self, occupied, free=None):
        if free is None:
            if not isinstance(occupied, OccupancyGrid):
                raise ValueError(f"SpaceMap: occupied must be an ops.OccupancyGrid, got {type(occupied).__name__}")
            free = occupied.empty_like()
        check_space_planes(occupied, free)
        self.occupied, self.free = occupied, free
        self.device = occupied.device

    def integrate(self, origin, points, max_range=None):
        """One scan: the rays origin -> points[i] carve the free plane, and the rows become occupied — except those beyond max_range:
        a truncated ray's far point is a direction, not a return, and is carved up to max_range but not inserted.  Which rows those
        are is carve's own integer rule, read from its per-ray flags (one carve launch, then one insert of the other rows).
        -> the number of rays skipped (an endpoint out of range)."""
        check_carve(origin, points, max_range, self.free.resolution)
        pts = covmap_points(points, self.device, "SpaceMap.integrate")
        flags = torch.empty(pts.shape[0], dtype=torch.uint8, device=self.device)
        skipped = self.free.carve(origin, pts, max_range, flags=flags)
        self.occupied.insert(pts if max_range is None else pts[flags != 1])
        return skipped

    def reframed(self, shift=None, dims=None, centre=None):
        """Both planes re-framed (OccupancyGrid.reframed) -> a NEW SpaceMap over two new grids; this map and its planes are untouched."""
        s, d, _ = check_reframe(self, shift, dims, centre)
        return SpaceMap(self.occupied.reframed(shift=s, dims=d), self.free.reframed(shift=s, dims=d))

    def transformed(self, pose, quat, origin=None, resolution=None, dims=None, like=None, rule="nearest"):
        """Both planes under a rigid transform (OccupancyGrid.transformed) -> a NEW SpaceMap over two new grids; this map is only
        read.  rule 'nearest': both planes take the bit under the new voxel's centre.  rule 'cover', for planning: occupied takes
        the OR of the 3 x 3 x 3 voxels around it and free their AND (outside the box counts as not free), so no occupied voxel is
        lost, nothing is called free that touches a voxel that is not, and the two planes stay disjoint."""
        frame, _ = check_transform(self, pose, quat, origin, resolution, dims, like, rule)
        cover = rule == "cover"
        return SpaceMap(self.occupied.transformed(pose, quat, like=frame, rule=rule, _plane_rule="any" if cover else None),
                        self.free.transformed(pose, quat, like=frame, rule=rule, _plane_rule="all" if cover else None))

    def merge(self, other, pose=None, quat=None, rule="nearest"):
        """OR both planes of another SpaceMap into this one's over the overlap, in place -> self: of the same lattice, or, with pose
        and quat (OccupancyGrid.merge), resampled — under rule 'cover' the occupied plane by ANY and the free plane by ALL."""
        check_merge_posed(self, other, None, pose, quat, rule)
        cover = rule == "cover"
        self.occupied.merge(other.occupied, pose=pose, quat=quat, rule=rule, _plane_rule="any" if cover else None)
        self.free.merge(other.free, pose=pose, quat=quat, rule=rule, _plane_rule="all" if cover else None)
        return self

    def coarsened(self, factor=2, rule="cover", anchor="origin", origin=None, dims=None, like=None):
        """Both planes at `factor` times the voxel edge (OccupancyGrid.coarsened) -> a NEW SpaceMap over two new grids; this map is
        only read.  rule 'cover', for planning: occupied takes the OR of its children and free their AND (outside the box counts as
        not free) — no occupied voxel is lost and a coarse voxel is free only where all it holds is free.  rule 'max', for display,
        occlusion and matching: occupied takes the OR, free the OR of the free children unless one of them is occupied — the unknown
        is passed over.  The planes stay disjoint under both."""
        frame, _, rule = check_coarsen(self, factor, rule, anchor, origin, dims, like)
        occupied = self.occupied.coarsened(factor, "any", like=frame)
        if rule == "cover":
            return SpaceMap(occupied, self.free.coarsened(factor, "all", like=frame))
        return SpaceMap(occupied, self.free.coarsened(factor, "any", like=frame, _veto=self.occupied))

    def merge_fine(self, fine, rule="cover"):
        """OR both planes of a FINER SpaceMap into this one's, in place -> self: the occupied plane by ANY; the free plane by ALL (rule
        'cover') or by ANY vetoed by the finer map's occupied plane ('max').  Factor and offset come from the two frames."""
        factor, o, rule = check_merge_fine(self, fine, None, rule)
        self.occupied._coarsen(fine.occupied, factor, o, "any", "or", None)
        if rule == "cover":
            self.free._coarsen(fine.free, factor, o, "all", "or", None)
        else:
            self.free._coarsen(fine.free, factor, o, "any", "or", None, fine.occupied)
        return self

    def state(self, positions):
        """(M,3) world positions -> (M,) uint8: 2 occupied, 1 free, 0 unknown, 3 beyond the apron, not finite or outside dims."""
        pos = covmap_points(positions, self.device, "SpaceMap.state")
        out = torch.empty(pos.shape[0], dtype=torch.uint8, device=self.device)
        _map_call(self.device, "tohip_occ_state", ptr(self.occupied.buf), *self.free._sizes(), ptr(pos), pos.shape[0], ptr(out))
        return out

    def frontier(self, min_unknown=1):
        """The free voxels with at least min_unknown (1 .. 6) unknown face neighbours inside dims -> Frontier (ijk, points, grid, n).
        One synchronisation (n)."""
        k = check_min_unknown(min_unknown)
        return _listed_plane(Frontier, self.free, "tohip_occ_frontier", (ptr(self.occupied.buf), ptr(self.free.buf)), (k,))

    def unknown(self):
        """The unknown voxels — inside dims, neither occupied nor free — as a new OccupancyGrid of this geometry (pad bits 0):
        unknown().export() lists them and their centres, unknown().count() is the unexplored volume in voxels."""
        plane = self.free.empty_like()
        _map_call(self.device, "tohip_occ_unknown", ptr(self.occupied.buf), ptr(self.free.buf), *plane._sizes())
        return plane


VIEW_VOLUME_MAX_VIEWS = 65535   # views per launch (the grid's second dimension); view_volume chunks by it


def check_view_volume(space, poses, quats, k=None, min_gain=1, claimed=None, mark=None):
    """The arguments of view_volume / view_volume_select, by name: space an ops.SpaceMap; poses (M,3) and quats (M,4) floating
    tensors with the same M >= 1 (with k given: M <= 65 535), finite; k None or an integer >= 1; min_gain an integer >= 1; claimed and mark None or
    ops.OccupancyGrids of the map's origin, resolution, dims and device, neither of them one of the map's planes; mark may be claimed
    itself only with M == 1 -> (M, k clipped to M or None, min_gain); ValueError otherwise.  Needs no GPU."""
    if not isinstance(space, SpaceMap):
        raise ValueError(f"space must be an ops.SpaceMap (or an ops.EvidenceMap's .space), got {type(space).__name__}")
    for name, t, w in (("poses", poses, 3), ("quats", quats, 4)):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError(f"{name} must be a floating-point tensor, got {type(t).__name__}{'' if not torch.is_tensor(t) else ' of ' + str(t.dtype)}")
        if t.dim() != 2 or t.shape[1] != w or t.shape[0] == 0:
            raise ValueError(f"{name} must have shape (M,{w}) with M >= 1, got {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{name} must be finite (NaN or inf found)")
    M = poses.shape[0]
    if quats.shape[0] != M:
        raise ValueError(f"poses holds {M} views, quats {quats.shape[0]}")
    if k is not None and (not _is_int(k) or k < 1):
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    if k is not None and M > VIEW_VOLUME_MAX_VIEWS:
        raise ValueError(f"poses holds {M} candidates, a selection (k given) takes at most {VIEW_VOLUME_MAX_VIEWS}")
    if not _is_int(min_gain) or min_gain < 1:
        raise ValueError(f"min_gain must be an integer >= 1 (a number of voxels), got {min_gain!r}")
    for name, g in (("claimed", claimed), ("mark", mark)):
        if g is None:
            continue
        if not isinstance(g, OccupancyGrid):
            raise ValueError(f"{name} must be an ops.OccupancyGrid or None, got {type(g).__name__}")
        if g is space.occupied or g is space.free:
            raise ValueError(f"{name} must not be one of the map's own planes")
        diff = _grid_difference(space.occupied, g)
        if diff:
            raise ValueError(f"{name}: its {diff[0]} differs from the map's ({diff[2]} and {diff[1]})")
    if mark is not None and mark is claimed and M > 1:
        raise ValueError(f"mark may be the claimed plane itself only for one view, got {M} views (two views' lanes would race on one word)")
    return M, (None if k is None else min(int(k), M)), int(min_gain)


def _view_rows(space, poses, quats):
    p = poses.detach().to(device=space.device, dtype=torch.float32).contiguous()
    q = quats.detach().to(device=space.device, dtype=torch.float32).contiguous()
    return p, q


def _view_volume_call(space, p, q, n, view_index, cam, min_dist, max_dist, claimed, mark, window, gains, stop, stats):
    _map_call(space.device, "tohip_view_volume", ptr(space.occupied.buf), ptr(space.free.buf), ptr(claimed.buf if claimed is not None else None),
              ptr(mark.buf if mark is not None else None), space.occupied.buf.numel(), ctypes.byref(space.occupied.geom), ptr(p), ptr(q), n,
              ptr(view_index), cam.ref(), float(min_dist), float(max_dist), int(bool(window)), ptr(gains), ptr(stop), ptr(stats))


def view_volume(space, poses, quats, cam, min_dist, max_dist, claimed=None, mark=None, window=True, stats=None):
    """The unknown volume each view would reveal (tohip_view_volume, DESIGN.md 10 "Unknown volume"): (M,) int64 on the device, entry
    w = the number of voxels of `space` in state 0 — and not set in `claimed` — whose centre cull_waypoints keeps for pose w with this
    camera and these limits and which line_of_sight(space.occupied, poses[w], centre, skip=(1, 0)) sees.  mark: an OccupancyGrid of
    the map's geometry that receives the revealed voxels of all M views (bits are only set).  window=False enumerates every brick (the
    same counts).  stats: a zero-filled (3,) int64 device tensor that receives (centres tested, rays walked, voxels visited).  One
    launch per 65 535 views, nothing read back."""
    M, _, _ = check_view_volume(space, poses, quats, claimed=claimed, mark=mark)
    p, q = _view_rows(space, poses, quats)
    gains = torch.empty(M, dtype=torch.int64, device=space.device)
    for w0 in range(0, M, VIEW_VOLUME_MAX_VIEWS):
        w1 = min(M, w0 + VIEW_VOLUME_MAX_VIEWS)
        _view_volume_call(space, p[w0:w1], q[w0:w1], w1 - w0, None, cam, min_dist, max_dist, claimed, mark, window, gains[w0:w1], None, stats)
    return gains


def view_volume_select(space, poses, quats, cam, min_dist, max_dist, k, min_gain=1, claimed=None, window=True, travel_cost=None,
                       travel_m=0):
    """Greedy selection by revealed volume, on the device: k rounds of (score every candidate against the plane of what is claimed so
    far, pick the largest gain — the lowest index on ties, stop where it is below min_gain — and set the winner's revealed voxels in
    that plane), 3 k launches and nothing read back; at most 65 535 candidates (one launch scores them all).  -> (order (k,) int32,
    -1 from the round that stopped; gains (k,) int64, the marginal gains; revealed: a new OccupancyGrid, the caller's `claimed` (not
    modified) plus what the chosen views reveal), all on the device.

    travel_cost (None: today's launches): an (M,) int64 device row of TravelField.cost codes, one per candidate, and travel_m an
    integer in [0, 2^31): the pick becomes tohip_view_volume_pick_travel — only candidates with cost >= 0 and gain >= min_gain can win,
    and gain 2^20 - travel_m cost decides."""
    M, k, min_gain = check_view_volume(space, poses, quats, k, min_gain, claimed)
    travel_cost = _check_travel_cost(travel_cost, travel_m, M, space.device)
    p, q = _view_rows(space, poses, quats)

    def score(view_index, claimed, mark, gains, stop):
        _view_volume_call(space, p, q, M, view_index, cam, min_dist, max_dist, claimed, mark, window, gains, stop, None)
    return _view_select(space, score, M, k, min_gain, claimed, travel_cost, travel_m)


def _check_travel_cost(travel_cost, travel_m, M, device):
    if travel_cost is None:
        return None
    if not torch.is_tensor(travel_cost) or travel_cost.dtype != torch.int64 or tuple(travel_cost.shape) != (M,):
        raise ValueError(f"travel_cost must be an ({M},) int64 tensor, got "
                         f"{(tuple(travel_cost.shape), travel_cost.dtype) if torch.is_tensor(travel_cost) else type(travel_cost).__name__}")
    if not _is_int(travel_m) or not 0 <= travel_m <= TRAVEL_MAX_LIMIT:
        raise ValueError(f"travel_m must be an integer in [0, 2^31), got {travel_m!r}")
    return travel_cost.to(device).contiguous()


def _view_select(space, score, M, k, min_gain, claimed, travel_cost, travel_m):
    """The greedy rounds of view_volume_select and view_information_select: score(view_index, claimed, mark, gains, stop) is the
    scoring launch over the M candidates.  -> (order, picked, revealed)."""
    dev = space.device
    revealed = space.free.empty_like()
    if claimed is not None:
        revealed.buf.copy_(claimed.buf)
    scores = torch.empty(M, dtype=torch.int64, device=dev)
    scratch = torch.empty(M, dtype=torch.int64, device=dev)
    taken = torch.zeros(M, dtype=torch.int32, device=dev)
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    order = torch.full((k,), -1, dtype=torch.int32, device=dev)
    picked = torch.zeros(k, dtype=torch.int64, device=dev)
    for j in range(k):
        score(None, revealed, None, scores, stop)
        if travel_cost is None:
            _map_call(dev, "tohip_view_volume_pick", ptr(scores), ptr(taken), M, min_gain, j, ptr(order), ptr(picked), ptr(stop))
        else:
            _map_call(dev, "tohip_view_volume_pick_travel", ptr(scores), ptr(travel_cost), int(travel_m), ptr(taken), M, min_gain, j, ptr(order),
                      ptr(picked), ptr(stop))
        # the mark step: the winner's number stays on the device, and one view may claim what it counts
        score(order[j:j + 1], revealed, revealed, scratch, stop)
    return order, picked, revealed


INFORMATION_MAX_WEIGHT = 65535   # a weight table's entries are unsigned 16-bit


def information_table(params, unit=0.05, unknown_bits=1.0, scale=4096):
    """The default weight table of an evidence map with the settings `params` = (hit, miss, lmin, lmax, threshold) -> (256,) uint16
    host tensor, indexed by L + 128: the binary entropy, in bits, that observation can still remove from a voxel at value L —
    H(sigma(unit L)) - H(sigma(unit c)), c the clamp its state moves towards (lmin where L <= threshold, lmax above), never below 0
    — times scale, rounded; entry 0 (never observed) = round(scale unknown_bits); entries outside [lmin, lmax] are 0.  So a voxel
    at a clamp weighs 0 and a finished map has information 0.  unit: the log-odds one step of L stands for.  Computed in f64."""
    _, _, lmin, lmax, threshold = params
    for name, v in (("unit", unit), ("unknown_bits", unknown_bits), ("scale", scale)):
        if not _is_real(v) or not np.isfinite(float(v)) or float(v) < 0.0 or (name == "unit" and float(v) == 0.0):
            raise ValueError(f"information_table: {name} must be a finite number {'> 0' if name == 'unit' else '>= 0'}, got {v!r}")

    def H(L):
        p = 1.0 / (1.0 + np.exp(-float(unit) * np.asarray(L, dtype=np.float64)))
        with np.errstate(divide="ignore", invalid="ignore"):
            h = -(p * np.log2(p) + (1.0 - p) * np.log2(1.0 - p))
        return np.where((p <= 0.0) | (p >= 1.0), 0.0, h)
    L = np.arange(int(lmin), int(lmax) + 1)
    c = np.where(L <= int(threshold), int(lmin), int(lmax))
    W = np.zeros(256, dtype=np.float64)
    W[L + 128] = np.round(float(scale) * np.maximum(0.0, H(L) - H(c)))
    W[0] = np.round(float(scale) * float(unknown_bits))
    if not W.max() <= INFORMATION_MAX_WEIGHT:
        raise ValueError(f"information_table: the weights do not fit 16 bits (the largest is {W.max():.0f}): scale = {scale!r}, "
                         f"unknown_bits = {unknown_bits!r}")
    return torch.from_numpy(W.astype(np.uint16))


def check_information_table(table, device=None):
    """A weight table, by name: 256 integers in [0, 65535] — a tensor, an array or a sequence of shape (256,), never floating point
    -> the table as 256 16-bit words on `device` (None: on the host).  A (256,) uint16 or int16 tensor already on `device` is used
    as it is: the bits are the weights, and nothing is read back.  ValueError otherwise."""
    if torch.is_tensor(table) and table.dtype in (torch.uint16, torch.int16):
        if tuple(table.shape) != (256,):
            raise ValueError(f"table must have shape (256,), got {tuple(table.shape)}")
        t = table.detach().contiguous().view(torch.int16)
        return t if device is None or t.device == torch.device(device) else t.to(device)
    if torch.is_tensor(table):
        if table.is_floating_point() or table.is_complex() or table.dtype == torch.bool:
            raise ValueError(f"table must hold integers, got {table.dtype}")
        a = table.detach().cpu().numpy()
    else:
        try:
            a = np.asarray(table)
        except Exception:
            a = None
        if a is None or a.dtype.kind not in "iu":
            raise ValueError(f"table must be 256 integers (a tensor or an array of an integer dtype), got {type(table).__name__}"
                             f"{'' if a is None else ' of ' + str(a.dtype)}")
    if a.shape != (256,):
        raise ValueError(f"table must have shape (256,), got {tuple(a.shape)}")
    if int(a.min()) < 0 or int(a.max()) > INFORMATION_MAX_WEIGHT:
        raise ValueError(f"table entries must lie in [0, {INFORMATION_MAX_WEIGHT}], got [{int(a.min())}, {int(a.max())}]")
    t = torch.from_numpy(a.astype(np.uint16).view(np.int16))
    return t if device is None else t.to(device)


def check_view_information(map, poses, quats, table=None, k=None, min_gain=1, claimed=None, mark=None, travel=False):
    """The arguments of view_information / view_information_select, by name: map an ops.EvidenceMap (a SpaceMap has no evidence
    bytes); table None (the map's default, information_table) or check_information_table's; poses, quats, k, claimed and mark as
    check_view_volume takes them; min_gain an integer >= 1, in table units; travel=True: the map must be small enough for the travel
    pick's gain 2^20 - m cost, 65535 x voxels x 2^20 < 2^63 -> (M, k clipped to M or None, min_gain); ValueError otherwise.
    Needs no GPU."""
    if not isinstance(map, EvidenceMap):
        raise ValueError(f"map must be an ops.EvidenceMap (a SpaceMap has no evidence bytes to weigh), got {type(map).__name__}")
    if table is not None:
        check_information_table(table)
    if not _is_int(min_gain) or min_gain < 1:
        raise ValueError(f"min_gain must be an integer >= 1 (in the table's units), got {min_gain!r}")
    n_voxels = int(map.dims[0]) * int(map.dims[1]) * int(map.dims[2])
    if travel and INFORMATION_MAX_WEIGHT * n_voxels * (1 << 20) >= 1 << 63:
        raise ValueError(f"travel: a map of {n_voxels} voxels is too large for a selection with travel= (the pick forms gain x 2^20, and "
                         f"{INFORMATION_MAX_WEIGHT} x {n_voxels} x 2^20 reaches 2^63); select on a window of the map (reframed) or without travel=")
    return check_view_volume(map.space, poses, quats, k, min_gain, claimed, mark)


def _information_plane(map, table, total=None):
    """(the table on the device, the candidate plane: a new OccupancyGrid) of an EvidenceMap under `table`; one launch.  total: a
    zero-filled int64 device tensor that receives the map's remaining information, or None."""
    t = check_information_table(information_table(map.params) if table is None else table, map.device)
    plane = map.occupied.empty_like()
    _map_call0(map.device, "tohip_evid_weight_plane", *map._sizes(), ptr(t), ptr(plane.buf), plane.buf.numel(), ptr(total))
    return t, plane


def _view_information_call(map, t, plane, p, q, n, view_index, cam, min_dist, max_dist, claimed, mark, window, gains, stop, stats):
    _map_call0(map.device, "tohip_view_information", ptr(map.occupied.buf), ptr(map.free.buf), ptr(claimed.buf if claimed is not None else None),
               ptr(mark.buf if mark is not None else None), map.occupied.buf.numel(), ctypes.byref(map.geom), ptr(map.buf), map.buf.numel(),
               ptr(t), ptr(plane.buf), ptr(p), ptr(q), n, ptr(view_index), cam.ref(), float(min_dist), float(max_dist), int(bool(window)),
               ptr(gains), ptr(stop), ptr(stats))


def view_information(map, poses, quats, cam, min_dist, max_dist, table=None, claimed=None, mark=None, window=True, stats=None):
    """The information each view would gain (tohip_view_information, DESIGN.md 10 "Information gain"): (M,) int64 on the device,
    entry w = the sum of table[L + 128] over the voxels of the EvidenceMap `map` with a positive weight — whatever their state, and
    not set in `claimed` — whose centre cull_waypoints keeps for pose w with this camera and these limits and which
    line_of_sight(map.occupied, poses[w], centre, skip=(1, 0)) sees: the target voxel is not tested, so a weakly occupied surface
    voxel counts.  table: None (information_table of the map's settings) or 256 integers in [0, 65535].  mark, window, stats: as
    view_volume takes them.  The candidate plane is built once per call (one launch); then one launch per 65 535 views, nothing
    read back."""
    M, _, _ = check_view_information(map, poses, quats, table, claimed=claimed, mark=mark)
    p, q = _view_rows(map.space, poses, quats)
    t, plane = _information_plane(map, table)
    gains = torch.empty(M, dtype=torch.int64, device=map.device)
    for w0 in range(0, M, VIEW_VOLUME_MAX_VIEWS):
        w1 = min(M, w0 + VIEW_VOLUME_MAX_VIEWS)
        _view_information_call(map, t, plane, p[w0:w1], q[w0:w1], w1 - w0, None, cam, min_dist, max_dist, claimed, mark, window, gains[w0:w1],
                               None, stats)
    return gains


def view_information_select(map, poses, quats, cam, min_dist, max_dist, k, table=None, min_gain=1, claimed=None, window=True,
                            travel_cost=None, travel_m=0):
    """Greedy selection by information gain, on the device: view_volume_select's rounds with view_information's gains — the
    candidate plane once, then 3 k launches, nothing read back; at most 65 535 candidates.  min_gain is in the table's units.
    -> (order (k,) int32, -1 from the round that stopped; gains (k,) int64, the marginal gains; revealed: a new OccupancyGrid, the
    caller's `claimed` (not modified) plus the voxels the chosen views inform), all on the device.  travel_cost, travel_m: as
    view_volume_select takes them; refused by name where 65535 x voxels x 2^20 could reach 2^63."""
    M, k, min_gain = check_view_information(map, poses, quats, table, k, min_gain, claimed, travel=travel_cost is not None)
    travel_cost = _check_travel_cost(travel_cost, travel_m, M, map.device)
    p, q = _view_rows(map.space, poses, quats)
    t, plane = _information_plane(map, table)

    def score(view_index, claimed, mark, gains, stop):
        _view_information_call(map, t, plane, p, q, M, view_index, cam, min_dist, max_dist, claimed, mark, window, gains, stop, None)
    return _view_select(map.space, score, M, k, min_gain, claimed, travel_cost, travel_m)


SCAN_MAX_SIDE = 8192   # pixels per side of a depth scan's image
SCAN_MAX_VIEWS = 65535  # views per launch (the grid's second dimension)


def check_depth_scan(grid, poses, quats, intrins, img_width, img_height, min_dist, max_dist, hit_plane=None, pass_plane=None):
    """depth_scan's arguments, by name: grid an ops.OccupancyGrid; poses (V,3) and quats (V,4) floating tensors with the same V in
    [1, 65 535], finite; intrins 9 finite numbers (fx 0 cx; 0 fy cy; 0 0 1) with fx, fy > 0; img_width and img_height integral
    numbers in [1, 8192] with V H W < 2^31; 0 <= min_dist < max_dist, both finite; hit_plane and pass_plane None or
    ops.OccupancyGrids of the grid's origin, resolution, dims and device, neither the grid itself nor each other
    -> (V, W, H); ValueError otherwise.  Needs no GPU."""
    if not isinstance(grid, OccupancyGrid):
        raise ValueError(f"grid must be an ops.OccupancyGrid, got {type(grid).__name__}")
    for name, t, w in (("poses", poses, 3), ("quats", quats, 4)):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError(f"{name} must be a floating-point tensor, got {type(t).__name__}{'' if not torch.is_tensor(t) else ' of ' + str(t.dtype)}")
        if t.dim() != 2 or t.shape[1] != w or t.shape[0] == 0:
            raise ValueError(f"{name} must have shape (V,{w}) with V >= 1, got {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{name} must be finite (NaN or inf found)")
    V = poses.shape[0]
    if quats.shape[0] != V:
        raise ValueError(f"poses holds {V} views, quats {quats.shape[0]}")
    if V > SCAN_MAX_VIEWS:
        raise ValueError(f"poses holds {V} views, a scan takes at most {SCAN_MAX_VIEWS}")
    try:
        K = np.asarray(torch.as_tensor(intrins, dtype=torch.float32).detach().cpu().numpy(), dtype=np.float32).reshape(-1)
    except (TypeError, ValueError, RuntimeError):
        K = np.zeros(0, dtype=np.float32)
    if K.shape != (9,) or not np.isfinite(K).all():
        raise ValueError(f"intrins must be 9 finite numbers (a 3 x 3 matrix), got {intrins!r}")
    if not (K[0] > 0 and K[4] > 0):
        raise ValueError(f"intrins must have fx > 0 and fy > 0, got fx = {K[0]:g}, fy = {K[4]:g}")
    if K[1] != 0 or K[3] != 0 or K[6] != 0 or K[7] != 0 or K[8] != 1:
        raise ValueError(f"intrins must be (fx 0 cx; 0 fy cy; 0 0 1): no skew and K[2][2] = 1, got {K.tolist()}")
    sides = []
    for name, v in (("img_width", img_width), ("img_height", img_height)):
        f = _float_or_nan(v, np.float32) if _is_real(v) else float("nan")
        if not (1 <= f <= SCAN_MAX_SIDE) or f != np.floor(f):
            raise ValueError(f"{name} must be an integral number in [1, {SCAN_MAX_SIDE}], got {v!r}")
        sides.append(int(f))
    W, H = sides
    if V * H * W >= 1 << 31:
        raise ValueError(f"img_width x img_height x views must stay below 2^31 pixels, got {W} x {H} x {V}")
    mn = _float_or_nan(min_dist, np.float32) if _is_real(min_dist) else float("nan")
    mx = _float_or_nan(max_dist, np.float32) if _is_real(max_dist) else float("nan")
    if not (np.isfinite(mn) and mn >= 0):
        raise ValueError(f"min_dist must be a finite number >= 0, got {min_dist!r}")
    if not (np.isfinite(mx) and mx > mn):
        raise ValueError(f"max_dist must be a finite number > min_dist = {mn:g}, got {max_dist!r}")
    for name, g in (("hit_plane", hit_plane), ("pass_plane", pass_plane)):
        if g is None:
            continue
        if not isinstance(g, OccupancyGrid):
            raise ValueError(f"{name} must be an ops.OccupancyGrid or None, got {type(g).__name__}")
        if g is grid:
            raise ValueError(f"{name} must not be the scanned grid itself")
        diff = _grid_difference(grid, g)
        if diff:
            raise ValueError(f"{name}: its {diff[0]} differs from the scanned grid's ({diff[2]} and {diff[1]})")
    if hit_plane is not None and pass_plane is hit_plane:
        raise ValueError("pass_plane must not be the hit plane itself")
    return V, W, H


def depth_scan(grid, poses, quats, cam, min_dist, max_dist, hit_plane=None, pass_plane=None, points=False, stats=None):
    """The depth image a sensor at each pose would return from `grid` (tohip_depth_scan, DESIGN.md 10 "Ray casts and depth scans")
    -> (voxel (V,H,W) int32, depth (V,H,W) f32, flags (V,H,W) uint8, points (V,H,W,3) f32 or None), on the device.  Per pixel the
    ray from the pose through the pixel to z-depth max_dist is cast with skip (1, 0): flags 0 a return (voxel: its linear index,
    depth = lam max_dist, points: the voxel's centre), 1 no return (voxel -1, depth +inf, points: the ray's far point), 2 skipped
    (the pose or the far point out of range: -2, NaN, NaN), 3 a hit nearer than min_dist (voxel and depth name it, points NaN).
    cam: an ops.Camera (its K and image size).  hit_plane / pass_plane: OccupancyGrids of the grid's geometry that receive the
    flag-0 hit voxels and the voxels the rays of flag 0 and 1 passed (bits are only set).  stats: a zero-filled (3,) int64 device
    tensor that receives (rays walked, voxels visited, plane atomics issued).  One launch, nothing read back."""
    V, W, H = check_depth_scan(grid, poses, quats, list(cam.c.K), cam.c.img_width, cam.c.img_height, min_dist, max_dist, hit_plane, pass_plane)
    p, q = _view_rows(grid, poses, quats)
    dev = grid.device
    voxel = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    flags = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    pts = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev) if points else None
    _map_call(dev, "tohip_depth_scan", *grid._sizes(), ptr(p), ptr(q), V, cam.ref(), float(min_dist), float(max_dist),
              ptr(hit_plane.buf if hit_plane is not None else None), ptr(pass_plane.buf if pass_plane is not None else None), ptr(voxel),
              ptr(depth), ptr(flags), ptr(pts), ptr(stats))
    return voxel, depth, flags, pts


FIELD_MAX_D = 254          # the largest truncation distance in voxels: D^2 < 65535, the sentinel
FIELD_SENTINEL = 65535     # "no obstacle within D voxels"
FIELD_UNKNOWN = ("free", "obstacle")


def field_need2(radius, resolution):
    """The squared gap in voxels that certifies `radius` metres at this resolution: ceil((float64(radius) / float64(f32 resolution) +
    1/64)^2), computed on the host ("Clearance field"; synth.field_need2 restates it)."""
    return int(np.ceil((float(radius) / float(np.float32(resolution)) + 1.0 / 64.0) ** 2))


def check_field(grid_or_space, max_dist=None, unknown="free", D=None, radius=None, stride=1, space=None):
    """A clearance field's settings and a query's, by name; needs no GPU.  grid_or_space: an OccupancyGrid or a SpaceMap (its occupied
    grid; its free plane is read only with unknown='obstacle', which needs a SpaceMap).  max_dist: a finite number of metres whose D
    = ceil(float64(max_dist) / float64(f32 resolution)) lies in [1, 254] — or D itself, an integer in that range, instead.  radius
    (None: not asked): a finite number > 0 whose need2 = field_need2(radius) is at most D^2 — a larger one this field cannot certify,
    and the error names the largest it can.  stride: an integer >= 1.  space (None: no filter): a SpaceMap of the grid's origin,
    resolution, dims and device.  -> (occupied grid, free plane or None, D, need2 or None); ValueError otherwise."""
    if isinstance(grid_or_space, SpaceMap):
        occupied, free = grid_or_space.occupied, grid_or_space.free
    elif isinstance(grid_or_space, OccupancyGrid):
        occupied, free = grid_or_space, None
    else:
        raise ValueError(f"ClearanceField: the map must be an ops.OccupancyGrid or an ops.SpaceMap, got {type(grid_or_space).__name__}")
    if unknown not in FIELD_UNKNOWN:
        raise ValueError(f"unknown must be 'free' or 'obstacle', got {unknown!r}")
    if unknown == "obstacle" and free is None:
        raise ValueError("unknown='obstacle' needs an ops.SpaceMap (the free plane tells unknown from free), got an OccupancyGrid")
    r = occupied.resolution
    if D is None:
        m = _float_or_nan(max_dist) if _is_real(max_dist) else float("nan")
        D = int(np.ceil(m / r)) if np.isfinite(m) and m > 0.0 and m / r <= FIELD_MAX_D + 1 else 0
        if not 1 <= D <= FIELD_MAX_D:
            raise ValueError(f"max_dist must be a finite number of metres > 0 and at most {FIELD_MAX_D} voxels ({FIELD_MAX_D * r:g} m at this "
                             f"resolution), got {max_dist!r}")
    elif not _is_int(D) or not 1 <= D <= FIELD_MAX_D:
        raise ValueError(f"D must be an integer number of voxels in [1, {FIELD_MAX_D}], got {D!r}")
    D = int(D)
    need2 = None
    if radius is not None:
        need2 = field_need2(check_tour_radius(radius), r)
        if need2 > D * D:
            raise ValueError(f"clearance_radius {radius!r} needs a squared gap of {need2} voxels, this field is truncated at D = {D} "
                             f"({D * D}): the largest radius it can certify is {(D - 1.0 / 64.0) * r:g} m; build it with a larger max_dist")
    if not _is_int(stride) or stride < 1:
        raise ValueError(f"stride must be an integer >= 1, got {stride!r}")
    if space is not None:
        if not isinstance(space, SpaceMap):
            raise ValueError(f"space must be an ops.SpaceMap or None, got {type(space).__name__}")
        diff = _grid_difference(space.occupied, occupied)
        if diff:
            raise ValueError("space: its {} differs from the field's ({} and {})".format(*diff))
    return occupied, (free if unknown == "obstacle" else None), D, need2


class FreeNodes(Frontier):
    """What ClearanceField.free_nodes returns: ijk (F,3) int32 and points (F,3) f32 (the voxel centres) on the device in brick order,
    grid (the node plane as an OccupancyGrid) and n = F — a Frontier's fields."""
    __slots__ = ()


class ClearanceField:
    """A conservative clearance field over an occupancy grid (field_kernels.hip, DESIGN.md 10 "Clearance field"): per voxel inside dims
    the squared gap, in voxels, to the nearest obstacle voxel — gap2(v, u) = sum over the axes of max(|v_a - u_a| - 1, 0)^2, the
    distance between the voxel cubes, never more than the true one — truncated at D voxels (65535 beyond).  Integers only: the same
    bits in every run.  It holds the buffers, the geometry, D and the obstacle rule, and reads the map's planes again on rebuild()."""

    def __init__(self, grid_or_space, max_dist=None, unknown="free", D=None):
        self.occupied, self.free, self.D, _ = check_field(grid_or_space, max_dist, unknown, D=D)
        self.unknown = unknown
        g = self.occupied
        self.origin, self.resolution, self.dims, self.device, self.geom = g.origin, g.resolution, g.dims, g.device, g.geom
        L = _lib.lib()
        self.buf = torch.empty(L.tohip_field_bytes(*self.dims), dtype=torch.uint8, device=self.device)
        self._ws = torch.empty(L.tohip_field_workspace_bytes(*self.dims), dtype=torch.uint8, device=self.device)
        self.rebuild()

    @classmethod
    def build(cls, grid_or_space, max_dist, unknown="free"):
        """The field of an OccupancyGrid or a SpaceMap, truncated at ceil(max_dist / resolution) voxels.  unknown='free': only
        occupied voxels are obstacles; 'obstacle' (a SpaceMap): the voxels no ray has passed through are too."""
        return cls(grid_or_space, max_dist, unknown)

    def _sizes(self):
        return ptr(self.buf), self.buf.numel(), ctypes.byref(self.geom)

    def rebuild(self):
        """Recompute the whole field from the same planes — after more inserts or carves — into the same buffers: three launches,
        nothing read back.  -> self."""
        _map_call(self.device, "tohip_field_build", ptr(self.occupied.buf), ptr(self.free.buf) if self.free is not None else None,
                  self.occupied.buf.numel(), ctypes.byref(self.geom), self.D, ptr(self.buf), self.buf.numel(), ptr(self._ws), self._ws.numel())
        return self

    def dense(self):
        """The field as an (nx, ny, nz) int32 tensor (a copy): for tests and small grids."""
        nx, ny, nz = self.dims
        return self.buf.view(torch.int16).view(nz, ny, nx).to(torch.int32).bitwise_and(0xFFFF).permute(2, 1, 0).contiguous()

    def _positions(self, p, want_d2, want_dist):
        pos = covmap_points(p, self.device, "ClearanceField")
        d2 = torch.empty(pos.shape[0], dtype=torch.int32, device=self.device) if want_d2 else None
        dist = torch.empty(pos.shape[0], dtype=torch.float32, device=self.device) if want_dist else None
        _map_call(self.device, "tohip_field_positions", *self._sizes(), ptr(pos), pos.shape[0], ptr(d2), ptr(dist))
        return d2, dist

    def lookup_positions(self, p):
        """(M,3) world positions -> (M,) int32: the squared gap of the position's voxel, 65535 where no obstacle lies within D voxels
        or the position is in range but outside dims, -1 out of range (beyond the apron, or not finite)."""
        return self._positions(p, True, False)[0]

    def distance(self, p):
        """(M,3) world positions -> (M,) f32 metres: sqrt(squared gap) resolution, a lower bound on the distance from anywhere in the
        position's voxel to anything in an obstacle voxel; +inf for 65535, NaN out of range."""
        return self._positions(p, False, True)[1]

    def _segments(self, a, b, need2=None):
        """One launch of tohip_field_segments over the legs a[e] -> b[e] -> (d2, vox), two (E,) int32 — or, with need2, the edge answer
        (d (E,) f32, idx (E,) int32)."""
        check_los(self.origin, self.resolution, self.dims, (0, 0), a, b)
        a, b = covmap_points(a, self.device, "ClearanceField"), covmap_points(b, self.device, "ClearanceField")
        x = torch.empty(a.shape[0], dtype=torch.int32 if need2 is None else torch.float32, device=self.device)
        y = torch.empty(a.shape[0], dtype=torch.int32, device=self.device)
        outs = (ptr(x), ptr(y), 0, None, None) if need2 is None else (None, None, need2, ptr(x), ptr(y))
        _map_call(self.device, "tohip_field_segments", *self._sizes(), ptr(a), ptr(b), a.shape[0], *outs)
        return x, y

    def segments(self, a, b):
        """The legs a[e] -> b[e], two (E,3) tensors of world points -> (d2 (E,) int32, vox (E,) int32): the smallest squared gap over
        the voxels the leg crosses — line_of_sight's exact walk, every voxel of it — and the linear index (k ny + j) nx + i of the
        first crossed voxel that holds it.  65535 / -1: no obstacle within D voxels of the leg; -1 / -1: an endpoint out of range."""
        return self._segments(a, b)

    def need2(self, radius):
        """The squared gap that certifies `radius` metres (field_need2); ValueError where it exceeds D^2, naming the largest radius
        this field can certify.  A leg is open iff its d2 >= need2."""
        return check_field(self.occupied, D=self.D, radius=radius)[3]

    def edges(self, a, b, radius):
        """The legs a[e] -> b[e] in the shape clearance_edges answers: (d (E,) f32, idx (E,) int32, s (E,) f32).  A leg the field
        certifies — every point of it at least `radius` from every obstacle voxel — is open: d +inf, idx -1.  Any other is blocked: d
        the gap in metres and idx the voxel's linear index; a leg with an endpoint out of range is never certified: d 0, idx -2.
        s is zeros.  One launch."""
        d, idx = self._segments(a, b, self.need2(radius))
        return d, idx, torch.zeros(d.shape[0], dtype=torch.float32, device=self.device)

    def free_nodes(self, radius, stride=1, space=None):
        """Free-space nodes from the map itself: the voxels whose whole cube keeps `radius` from every obstacle voxel (field >= need2),
        one in stride^3 (every index = stride // 2 modulo stride) and — with a SpaceMap of this geometry — known to be free.
        -> FreeNodes (ijk, points = the centres, grid, n) in brick order.  One synchronisation (n)."""
        _, _, _, need2 = check_field(self.occupied, D=self.D, radius=check_tour_radius(radius), stride=stride, space=space)
        occ, fre = (ptr(space.occupied.buf), ptr(space.free.buf)) if space is not None else (None, None)
        return _listed_plane(FreeNodes, self.occupied, "tohip_field_nodes", (ptr(self.buf), self.buf.numel(), occ, fre), (need2, int(stride)))


TRAVEL_SENTINEL = 0xFFFFFFFF          # a travel field's "unreachable"
TRAVEL_MAX_LIMIT = (1 << 31) - 1      # the largest cost a travel field stores, in 1/64 voxel edge
TRAVEL_MAX_ROUNDS_PER_CHECK = 65536
TRAVEL_MAX_ROWS = 1 << 20             # rows of one path that paths() sizes for without being told


def travel_limit(max_dist, resolution):
    """max_dist in metres (None: none) -> the largest cost kept, min(floor(float64(max_dist) / float64(f32 resolution) 64), 2^31 - 1)
    (synth.travel_limit restates it)."""
    if max_dist is None:
        return TRAVEL_MAX_LIMIT
    return int(min(np.floor(float(max_dist) / float(np.float32(resolution)) * 64.0), TRAVEL_MAX_LIMIT))


def _check_rows3(t, name, empty=False):
    if not torch.is_tensor(t) or not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor, got {type(t).__name__}{'' if not torch.is_tensor(t) else ' of ' + str(t.dtype)}")
    if t.dim() == 1 and t.shape[0] == 3:
        t = t.reshape(1, 3)
    if t.dim() != 2 or t.shape[1] != 3 or (t.shape[0] == 0 and not empty):
        raise ValueError(f"{name} must have shape ({'M' if empty else 'S'},3){'' if empty else ' with S >= 1'} (or (3,)), got {tuple(t.shape)}")
    return t


TRAVEL_KAPPA_NEUTRAL, TRAVEL_KAPPA_MAX = 16, 255   # a weight layer's factors: 16 is neutral, 255 costs about 15.9 times as much


def check_travel_lut(lut, what="lut"):
    """A weight table, by name; needs no GPU: a 1-D sequence, array or tensor of 1 .. 65536 integers in [16, 255] -> (n,) uint8 numpy;
    ValueError names the first offender."""
    a = lut.detach().cpu().numpy() if torch.is_tensor(lut) else np.asarray(lut)
    if a.ndim != 1 or not 1 <= a.shape[0] <= 65536 or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be a 1-D table of 1 .. 65536 integers, got shape {tuple(a.shape)} of {a.dtype}")
    bad = np.flatnonzero((a < TRAVEL_KAPPA_NEUTRAL) | (a > TRAVEL_KAPPA_MAX))
    if len(bad):
        raise ValueError(f"{what}[{int(bad[0])}] = {int(a[bad[0]])} is outside [{TRAVEL_KAPPA_NEUTRAL}, {TRAVEL_KAPPA_MAX}] (16 is neutral; "
                         "there are no discounts)")
    return a.astype(np.uint8)


def check_travel_unknown_add(unknown_add, space):
    """unknown_add of a weight layer, by name: an integer in [0, 255], and not 0 only with a space that says what is unknown."""
    if not _is_int(unknown_add) or not 0 <= unknown_add <= TRAVEL_KAPPA_MAX:
        raise ValueError(f"unknown_add must be an integer in [0, {TRAVEL_KAPPA_MAX}], got {unknown_add!r}")
    if unknown_add and space is None:
        raise ValueError("unknown_add needs space= (an ops.SpaceMap: what is unknown)")
    return int(unknown_add)


def _check_weights_field(field):
    if not isinstance(field, ClearanceField):
        raise ValueError(f"TravelWeights: field must be an ops.ClearanceField, got {type(field).__name__}")


def check_travel_dense(field, tensor):
    """A caller's weight layer, by name; needs no GPU for a host tensor's dtype and shape: an integer tensor (nx, ny, nz) of the
    field's dims on the field's device, every value in [16, 255] — the first offender is named."""
    _check_weights_field(field)
    if not torch.is_tensor(tensor) or tensor.is_floating_point() or tensor.is_complex() or tensor.dtype == torch.bool:
        raise ValueError(f"TravelWeights: the layer must be an integer tensor (dtype), got "
                         f"{tensor.dtype if torch.is_tensor(tensor) else type(tensor).__name__}")
    if tuple(tensor.shape) != tuple(field.dims):
        raise ValueError(f"TravelWeights: the layer must have the field's dims {tuple(field.dims)}, got {tuple(tensor.shape)}")
    bad = ((tensor < TRAVEL_KAPPA_NEUTRAL) | (tensor > TRAVEL_KAPPA_MAX)).nonzero()
    if bad.shape[0]:
        i, j, k = (int(v) for v in bad[0])
        raise ValueError(f"TravelWeights: kappa[{i}, {j}, {k}] = {int(tensor[i, j, k])} is outside [{TRAVEL_KAPPA_NEUTRAL}, "
                         f"{TRAVEL_KAPPA_MAX}] (16 is neutral; there are no discounts)")
    dev = torch.device(field.device)
    if tensor.device.type != dev.type or (dev.index is not None and tensor.device.index is not None and tensor.device.index != dev.index):
        raise ValueError(f"TravelWeights: the layer lives on device {tensor.device}, the field on {dev}")


class TravelWeights:
    """A weight layer for travel fields (travel_kernels.hip, DESIGN.md 10 "Weighted travel fields"): one uint8 factor kappa per voxel
    inside the clearance field's dims, 16 <= kappa <= 255, 16 neutral — the move m between v and u then costs (w_m (kappa[v] +
    kappa[u]) + 16) >> 5 instead of w_m.  It holds the byte volume (buf, x fastest) and the field's geometry.

    TravelWeights(field, lut=None, space=None, unknown_add=0) gathers kappa[v] = lut[min(field[v], len(lut) - 1)] on the device (the
    field's value is the squared gap in voxels; lut None: all 16) and, with space=, adds unknown_add at the voxels that are neither
    occupied nor known free, saturating at 255.  rebuild() re-reads the field (and the planes) after field.rebuild().
    TravelWeights.from_dense(field, tensor) holds a layer of the caller's own; set_dense(tensor) replaces it in place."""

    def __init__(self, field, lut=None, space=None, unknown_add=0):
        _check_weights_field(field)
        check_field(field.occupied, D=field.D, space=space)
        self.unknown_add = check_travel_unknown_add(unknown_add, space)
        table = check_travel_lut([TRAVEL_KAPPA_NEUTRAL] if lut is None else lut)
        self._over(field, space)
        self.lut = torch.from_numpy(table).to(self.device)
        self.rebuild()

    def _over(self, field, space):
        self.field, self.space = field, space
        self.origin, self.resolution, self.dims, self.device, self.geom = field.origin, field.resolution, field.dims, field.device, field.geom
        self.buf = torch.empty(_lib.lib().tohip_travel_weights_bytes(*self.dims), dtype=torch.uint8, device=self.device)

    @classmethod
    def from_dense(cls, field, tensor):
        """A layer of the caller's own: tensor (nx, ny, nz) on the field's device, uint8 or any integer dtype, every value in [16,
        255] — the first offender is named.  It is copied."""
        check_travel_dense(field, tensor)
        self = cls.__new__(cls)
        self.unknown_add, self.lut = 0, None
        self._over(field, None)
        return self.set_dense(tensor)

    def set_dense(self, tensor):
        """Replace the layer in place by `tensor` (from_dense's rules): the travel fields over it follow on their next rebuild().
        -> self."""
        check_travel_dense(self.field, tensor)
        self.lut = None
        self.buf.copy_(tensor.detach().to(torch.uint8).permute(2, 1, 0).reshape(-1))
        return self

    def rebuild(self):
        """Gather the layer again from the field (and the space's planes) — after field.rebuild().  One launch.  A layer from
        from_dense / set_dense has no table and stays as it is.  -> self."""
        if self.lut is None:
            return self
        occ, fre = (ptr(self.space.occupied.buf), ptr(self.space.free.buf)) if self.space is not None else (None, None)
        _map_call0(self.device, "tohip_travel_weights_build", ptr(self.field.buf), self.field.buf.numel(), occ, fre,
                   self.field.occupied.buf.numel(), ctypes.byref(self.geom), ptr(self.lut), self.lut.numel(), self.unknown_add, ptr(self.buf),
                   self.buf.numel())
        return self

    def dense(self):
        """The layer as an (nx, ny, nz) uint8 tensor (a copy)."""
        nx, ny, nz = self.dims
        return self.buf.view(nz, ny, nx).permute(2, 1, 0).contiguous()


def check_travel_weights(field, weights):
    """weights= of a travel field, by name; needs no GPU: None, or an ops.TravelWeights of the field's origin, resolution, dims and
    device.  -> weights."""
    if weights is None:
        return None
    if not isinstance(weights, TravelWeights):
        raise ValueError(f"weights must be an ops.TravelWeights or None, got {type(weights).__name__}")
    diff = _grid_difference(field, weights)
    if diff:
        raise ValueError(f"weights: the layer's {diff[0]} differs from the field's ({diff[2]} and {diff[1]})")
    return weights


def check_travel(field, radius, sources, space=None, max_dist=None, rounds_per_check=16, weights=None):
    """A travel field's arguments, by name; needs no GPU.  field: an ops.ClearanceField; radius: a finite number > 0 whose need2 =
    field_need2(radius) is at most the field's D^2 (check_field's rule and error); sources: a floating-point (S,3) tensor, S >= 1, or
    (3,) — rows that are not finite are allowed: they are ignored and reported; space: None or an ops.SpaceMap of the field's origin,
    resolution, dims and device; max_dist: None or a finite number of metres >= 0; rounds_per_check: an integer in [1, 65536]; weights:
    None or an ops.TravelWeights of the field's origin, resolution, dims and device.  -> (need2, limit, S); ValueError otherwise."""
    if not isinstance(field, ClearanceField):
        raise ValueError(f"TravelField: field must be an ops.ClearanceField, got {type(field).__name__}")
    _, _, _, need2 = check_field(field.occupied, D=field.D, radius=check_tour_radius(radius), space=space)
    src = _check_rows3(sources, "sources")
    if max_dist is not None:
        m = _float_or_nan(max_dist) if _is_real(max_dist) else float("nan")
        if not np.isfinite(m) or m < 0.0:
            raise ValueError(f"max_dist must be None or a finite number of metres >= 0, got {max_dist!r}")
    if not _is_int(rounds_per_check) or not 1 <= rounds_per_check <= TRAVEL_MAX_ROUNDS_PER_CHECK:
        raise ValueError(f"rounds_per_check must be an integer in [1, {TRAVEL_MAX_ROUNDS_PER_CHECK}], got {rounds_per_check!r}")
    check_travel_weights(field, weights)
    return need2, travel_limit(max_dist, field.resolution), src.shape[0]


class TravelField:
    """A travel field over a clearance field (travel_kernels.hip, DESIGN.md 10 "Travel field"): per voxel inside dims the length, in
    1/64 voxel edge, of the shortest 26-connected path from any of the sources through the voxels the field certifies for `radius`
    (and, with space=, that are known to be free), no corner cut — a navigation function from the robot's position.  Exact
    integers: the same bits in every run.  It holds the cost buffer and the worklist's workspace and reads the field (and the map's
    planes) again on rebuild().  seeded: (S,) uint8 on the device, 0 for a source that was ignored (not finite, out of range, outside
    dims or not traversable — there is no snapping); rounds: the worklist rounds the last build needed; limit: the largest cost
    kept.  weights (None: geometric length, today's calls): an ops.TravelWeights over the same field — the field then minimises
    the weighted length (DESIGN.md 10 "Weighted travel fields"), cost, distance and max_dist are in weighted units (never less than
    the geometric ones), and rebuild() reads the layer again."""

    def __init__(self, field, radius, sources, space=None, max_dist=None, rounds_per_check=16, weights=None):
        self.need2, self.limit, _ = check_travel(field, radius, sources, space, max_dist, rounds_per_check, weights)
        self._settings(field, radius, space, max_dist, rounds_per_check, weights)
        self.buf = torch.empty(_lib.lib().tohip_travel_bytes(*self.dims), dtype=torch.uint8, device=self.device)
        self._ws = None
        self.sources = self.seeded = None
        self.rounds = 0
        self.rebuild(sources)

    def _settings(self, field, radius, space, max_dist, rounds_per_check, weights=None):
        self.field, self.radius, self.space, self.max_dist, self.rounds_per_check = field, float(radius), space, max_dist, int(rounds_per_check)
        self.weights = weights
        self.origin, self.resolution, self.dims, self.device, self.geom = field.origin, field.resolution, field.dims, field.device, field.geom

    @classmethod
    def over(cls, buf, fields, sources, seeded):
        """An ops.TravelField over storage that exists: buf, one field's bytes (a slice of `fields`' buffer, an ops.TravelFields — no
        copy, no build), with the batch's settings, the sources that named the field and their seeded flags.  Its own rebuild() runs
        the single build into the slice."""
        self = cls.__new__(cls)
        self.need2, self.limit = fields.need2, fields.limit
        self._settings(fields.field, fields.radius, fields.space, fields.max_dist, fields.rounds_per_check, fields.weights)
        self.buf, self._ws, self.sources, self.seeded, self.rounds = buf, None, sources, seeded, fields.rounds
        return self

    def _set(self):
        """The arguments that name T: the field, the map's planes (or none), the planes' size, the geometry, need2."""
        occ, fre = (ptr(self.space.occupied.buf), ptr(self.space.free.buf)) if self.space is not None else (None, None)
        return (ptr(self.field.buf), self.field.buf.numel(), occ, fre, self.field.occupied.buf.numel(), ctypes.byref(self.geom), self.need2)

    def _layer(self):
        """The weighted entries' last arguments: the layer and its size."""
        w = check_travel_weights(self.field, self.weights)
        return ptr(w.buf), w.buf.numel()

    def rebuild(self, sources=None):
        """Recompute the whole field into the same buffers — after field.rebuild() (and weights.rebuild()), or from new sources
        (None: the last ones) when the robot has moved.  One synchronisation per rounds_per_check rounds.  -> self."""
        if sources is not None:
            check_travel(self.field, self.radius, sources, self.space, self.max_dist, self.rounds_per_check, self.weights)
            self.sources = _check_rows3(sources, "sources").detach().to(device=self.device, dtype=torch.float32).contiguous()
        S = self.sources.shape[0]
        if S == 0:
            raise ValueError("rebuild: this field of a batch had no source; give sources")
        if self._ws is None:   # (a field over a batch's slice needs none until it rebuilds alone)
            self._ws = torch.empty(_lib.lib().tohip_travel_workspace_bytes(*self.dims), dtype=torch.uint8, device=self.device)
        self.seeded = torch.empty(S, dtype=torch.uint8, device=self.device)
        rounds = ctypes.c_int64(0)
        if self.weights is None:
            _map_call(self.device, "tohip_travel_build", *self._set(), ptr(self.sources), S, self.limit, self.rounds_per_check, ptr(self.buf),
                      self.buf.numel(), ptr(self._ws), self._ws.numel(), ptr(self.seeded), ctypes.byref(rounds))
        else:   # the batch's weighted entry at n_fields = 1: every source names field 0
            zeros = torch.zeros(S, dtype=torch.int32, device=self.device)
            _map_call0(self.device, "tohip_travel_build_weighted", *self._set(), ptr(self.sources), ptr(zeros), S, 1, self.limit,
                       self.rounds_per_check, ptr(self.buf), self.buf.numel(), ptr(self._ws), self._ws.numel(), ptr(self.seeded),
                       ctypes.byref(rounds), *self._layer())
        self.rounds = int(rounds.value)
        return self

    def dense(self):
        """The field as an (nx, ny, nz) int64 tensor (a copy), -1 where unreachable: for tests and small grids."""
        nx, ny, nz = self.dims
        c = self.buf.view(torch.int32).view(nz, ny, nx).to(torch.int64).bitwise_and(0xFFFFFFFF)
        return torch.where(c == TRAVEL_SENTINEL, torch.full_like(c, -1), c).permute(2, 1, 0).contiguous()

    def _positions(self, p, want_cost, want_dist):
        pos = covmap_points(p, self.device, "TravelField")
        cost = torch.empty(pos.shape[0], dtype=torch.int64, device=self.device) if want_cost else None
        dist = torch.empty(pos.shape[0], dtype=torch.float32, device=self.device) if want_dist else None
        _map_call(self.device, "tohip_travel_positions", ptr(self.buf), self.buf.numel(), ctypes.byref(self.geom), ptr(pos), pos.shape[0],
                  ptr(cost), ptr(dist))
        return cost, dist

    def cost(self, positions):
        """(M,3) world positions -> (M,) int64: the cost of the position's voxel in 1/64 voxel edge, -1 unreachable, -2 out of range
        (beyond the apron, or not finite) or outside dims."""
        return self._positions(positions, True, False)[0]

    def distance(self, positions):
        """(M,3) world positions -> (M,) f32 metres travelled: cost / 64 resolution; +inf unreachable, NaN where cost() gives -2."""
        return self._positions(positions, False, True)[1]

    def reachable(self, positions):
        """(M,3) world positions -> (M,) bool: a path from a source to the position's voxel exists (within max_dist)."""
        return self.cost(positions) >= 0

    def paths(self, goals, max_rows=None):
        """One path per goal position -> a list of (L,3) f32 device tensors, the voxel centres from the source to the goal's voxel
        (L = 0: unreachable, out of range or outside dims); every leg joins two 26-neighbours and is one field.edges(a, b, radius)
        calls open.  max_rows (None: sized from the goals' costs) bounds the rows per path: ValueError names the goal and the rows
        it needs where a path does not fit.  One launch, one synchronisation.  Over a weighted field the paths are the weighted field's:
        every step costs at least its length, so the same row bound holds."""
        g = covmap_points(_check_rows3(goals, "goals", empty=True), self.device, "TravelField.paths")
        G = g.shape[0]
        if G == 0:
            return []
        if max_rows is None:
            # a path of cost c has at most c / 64 moves
            max_rows = min(max(int(self.cost(g).max().item()), 0) // 64 + 1, TRAVEL_MAX_ROWS)
        if not _is_int(max_rows) or max_rows < 1:
            raise ValueError(f"max_rows must be an integer >= 1 or None, got {max_rows!r}")
        rows = torch.empty((G, int(max_rows), 3), dtype=torch.float32, device=self.device)
        counts = torch.empty(G, dtype=torch.int64, device=self.device)
        if self.weights is None:
            _map_call(self.device, "tohip_travel_paths", ptr(self.buf), self.buf.numel(), *self._set(), ptr(g), G, int(max_rows), ptr(rows),
                      ptr(counts))
        else:
            zeros = torch.zeros(G, dtype=torch.int32, device=self.device)
            _map_call0(self.device, "tohip_travel_paths_weighted", ptr(self.buf), self.buf.numel(), *self._set(), 1, ptr(g), ptr(zeros), G,
                       int(max_rows), ptr(rows), ptr(counts), *self._layer())
        n = counts.cpu().tolist()
        for e, k in enumerate(n):
            if k < 0:
                raise ValueError(f"paths: goal {e} needs {-k} rows, max_rows is {int(max_rows)}")
        return [rows[e, :k].flip(0) for e, k in enumerate(n)]   # source -> goal


TRAVEL_MAX_FIELDS = _lib.CONSTANTS["TOHIP_TRAVEL_MAX_FIELDS"]
TRAVEL_MAX_ITEMS = (1 << 31) - 1      # (field, tile) items of a batch: n_fields times the 8 x 8 x 8-voxel tiles


def travel_tiles(dims):
    """The 8 x 8 x 8-voxel tiles of a grid of `dims`."""
    return int(np.prod([-(-int(d) // 8) for d in dims]))


def check_travel_batch(field, radius, sources, source_field=None, n_fields=None, space=None, max_dist=None, rounds_per_check=16, dims=None,
                       weights=None):
    """A batch of travel fields' arguments, by name; needs no GPU.  check_travel's rules, and: source_field: None (one field per
    source) or an integer tensor of shape (S,) — a row outside [0, n_fields) is allowed: its source is ignored and reported;
    n_fields: None (S without source_field, else the largest row + 1, at least 1) or an integer in [1, 256]; n_fields times the
    grid's tiles must fit 31 bits (dims: the grid's, None: the field's); weights: check_travel's, one layer for all fields.
    -> (need2, limit, S, n_fields); ValueError otherwise."""
    need2, limit, S = check_travel(field, radius, sources, space, max_dist, rounds_per_check, weights)
    if source_field is not None:
        if not torch.is_tensor(source_field) or source_field.is_floating_point() or source_field.dtype == torch.bool or \
                tuple(source_field.shape) != (S,):
            raise ValueError(f"source_field must be an integer tensor of shape ({S},), got "
                             f"{(tuple(source_field.shape), source_field.dtype) if torch.is_tensor(source_field) else type(source_field).__name__}")
    if n_fields is None:
        n_fields = S if source_field is None else max(int(source_field.max().item()) + 1, 1)
    if not _is_int(n_fields) or not 1 <= n_fields <= TRAVEL_MAX_FIELDS:
        raise ValueError(f"n_fields must be an integer in [1, {TRAVEL_MAX_FIELDS}], got {n_fields!r}")
    tiles = travel_tiles(field.dims if dims is None else dims)
    if n_fields * tiles > TRAVEL_MAX_ITEMS:
        raise ValueError(f"n_fields {n_fields} times the grid's {tiles} tiles of 8 x 8 x 8 voxels must fit 31 bits (a list entry packs "
                         f"field and tile), got {n_fields * tiles}")
    return need2, limit, S, int(n_fields)


class TravelFields:
    """B travel fields over one clearance field, built in the same worklist rounds (travel_kernels.hip, DESIGN.md 10 "Travel fields
    in batches"): field b is bit for bit the ops.TravelField of the sources that name b.  sources (S,3); source_field (S,) integers,
    the field each source seeds (None: one field per source, field i from source i) — a row outside [0, n_fields) is ignored and
    reported in seeded; n_fields: B (None: S, or the largest source_field + 1); one space, max_dist and limit for all fields.  It
    holds B cost volumes one after the other (4 B nx ny nz bytes) and the worklist's workspace.  n_fields, seeded (S,) uint8 on the
    device, rounds, limit as TravelField's.  fields[b] is an ops.TravelField over field b's slice: no copy, no build.  weights (None:
    none): one ops.TravelWeights that all fields share, as TravelField's; fields[b] carries it."""

    def __init__(self, field, radius, sources, source_field=None, n_fields=None, space=None, max_dist=None, rounds_per_check=16, weights=None):
        self.need2, self.limit, _, self.n_fields = check_travel_batch(field, radius, sources, source_field, n_fields, space, max_dist,
                                                                      rounds_per_check, weights=weights)
        TravelField._settings(self, field, radius, space, max_dist, rounds_per_check, weights)
        L = _lib.lib()
        self.buf = torch.empty(L.tohip_travel_batch_bytes(*self.dims, self.n_fields), dtype=torch.uint8, device=self.device)
        self._ws = torch.empty(L.tohip_travel_batch_workspace_bytes(*self.dims, self.n_fields), dtype=torch.uint8, device=self.device)
        self.sources = self.source_field = self.seeded = None
        self.rounds = 0
        self.rebuild(sources, source_field)

    _set = TravelField._set
    _layer = TravelField._layer

    def __len__(self):
        return self.n_fields

    def rebuild(self, sources=None, source_field=None):
        """Recompute every field into the same buffers — after field.rebuild(), or from new sources (None: the last ones; with new
        sources, source_field None means field i from source i again).  The number of fields stays.  -> self."""
        if sources is not None:
            _, _, S, _ = check_travel_batch(self.field, self.radius, sources, source_field, self.n_fields, self.space, self.max_dist,
                                            self.rounds_per_check, weights=self.weights)
            self.sources = _check_rows3(sources, "sources").detach().to(device=self.device, dtype=torch.float32).contiguous()
            self.source_field = (torch.arange(S, device=self.device) if source_field is None else source_field.detach().to(self.device)) \
                .clamp(-1, self.n_fields).to(torch.int32).contiguous()   # (any row out of range stays out of range)
        elif source_field is not None:
            raise ValueError("rebuild: source_field needs sources")
        S = self.sources.shape[0]
        self.seeded = torch.empty(S, dtype=torch.uint8, device=self.device)
        rounds = ctypes.c_int64(0)
        args = (*self._set(), ptr(self.sources), ptr(self.source_field), S, self.n_fields, self.limit, self.rounds_per_check, ptr(self.buf),
                self.buf.numel(), ptr(self._ws), self._ws.numel(), ptr(self.seeded), ctypes.byref(rounds))
        if self.weights is None:
            _map_call(self.device, "tohip_travel_build_batch", *args)
        else:
            _map_call0(self.device, "tohip_travel_build_weighted", *args, *self._layer())
        self.rounds = int(rounds.value)
        return self

    def __getitem__(self, b):
        if not _is_int(b) or not -self.n_fields <= b < self.n_fields:
            raise IndexError(f"field {b!r} of {self.n_fields}")
        b = int(b) % self.n_fields
        n = self.buf.numel() // self.n_fields
        mine = self.source_field == b
        return TravelField.over(self.buf[b * n:(b + 1) * n], self, self.sources[mine], self.seeded[mine])

    def dense(self):
        """The fields as a (B, nx, ny, nz) int64 tensor (a copy), -1 where unreachable: for tests and small grids."""
        nx, ny, nz = self.dims
        c = self.buf.view(torch.int32).view(self.n_fields, nz, ny, nx).to(torch.int64).bitwise_and(0xFFFFFFFF)
        return torch.where(c == TRAVEL_SENTINEL, torch.full_like(c, -1), c).permute(0, 3, 2, 1).contiguous()

    def _positions(self, p, want_cost, want_dist):
        pos = covmap_points(p, self.device, "TravelFields")
        shape = (self.n_fields, pos.shape[0])
        cost = torch.empty(shape, dtype=torch.int64, device=self.device) if want_cost else None
        dist = torch.empty(shape, dtype=torch.float32, device=self.device) if want_dist else None
        _map_call(self.device, "tohip_travel_positions_batch", ptr(self.buf), self.buf.numel(), ctypes.byref(self.geom), self.n_fields, ptr(pos),
                  pos.shape[0], ptr(cost), ptr(dist))
        return cost, dist

    def cost(self, positions):
        """(M,3) world positions -> (B,M) int64: row b is TravelField.cost in field b.  One launch."""
        return self._positions(positions, True, False)[0]

    def distance(self, positions):
        """(M,3) world positions -> (B,M) f32 metres: row b is TravelField.distance in field b.  One launch."""
        return self._positions(positions, False, True)[1]

    def reachable(self, positions):
        """(M,3) world positions -> (B,M) bool."""
        return self.cost(positions) >= 0

    def paths(self, goals, goal_field, max_rows=None):
        """One path per goal, walked in field goal_field[e] -> a list of (L,3) f32 device tensors, source -> goal, as
        TravelField.paths gives them; L = 0 also where goal_field[e] is outside [0, B).  One launch, one synchronisation."""
        g = covmap_points(_check_rows3(goals, "goals", empty=True), self.device, "TravelFields.paths")
        G = g.shape[0]
        gf = torch.as_tensor(goal_field, device=self.device)
        if tuple(gf.shape) != (G,) or (G > 0 and (gf.is_floating_point() or gf.dtype == torch.bool)):
            raise ValueError(f"goal_field must be ({G},) integers, got {tuple(gf.shape)} of {gf.dtype}")
        if G == 0:
            return []
        gf = gf.clamp(-1, self.n_fields).to(torch.int32).contiguous()
        if max_rows is None:
            # a path of cost c has at most c / 64 moves
            mine = self.cost(g).gather(0, gf.long().clamp(0, self.n_fields - 1)[None, :])
            max_rows = min(max(int(mine.max().item()), 0) // 64 + 1, TRAVEL_MAX_ROWS)
        if not _is_int(max_rows) or max_rows < 1:
            raise ValueError(f"max_rows must be an integer >= 1 or None, got {max_rows!r}")
        rows = torch.empty((G, int(max_rows), 3), dtype=torch.float32, device=self.device)
        counts = torch.empty(G, dtype=torch.int64, device=self.device)
        args = (ptr(self.buf), self.buf.numel(), *self._set(), self.n_fields, ptr(g), ptr(gf), G, int(max_rows), ptr(rows), ptr(counts))
        if self.weights is None:
            _map_call(self.device, "tohip_travel_paths_batch", *args)
        else:
            _map_call0(self.device, "tohip_travel_paths_weighted", *args, *self._layer())
        n = counts.cpu().tolist()
        for e, k in enumerate(n):
            if k < 0:
                raise ValueError(f"paths: goal {e} needs {-k} rows, max_rows is {int(max_rows)}")
        return [rows[e, :k].flip(0) for e, k in enumerate(n)]   # source -> goal


COMPONENT_CONNECTIVITIES = (6, 18, 26)
COMPONENT_SENTINEL = 0xFFFFFFFF       # a label volume's "clear voxel"
COMPONENT_MAX_ROUNDS_PER_CHECK = 1000


def check_components(grid, connectivity=26, rounds_per_check=16, values=None):
    """A component labelling's arguments, by name; needs no GPU.  grid: an ops.OccupancyGrid — any bit plane of that layout: an
    occupied grid, a free plane, Frontier.grid, SpaceMap.unknown(), EvidenceMap.occupied / .free, FreeNodes.grid; connectivity: 6, 18
    or 26; rounds_per_check: an integer in [1, 1000]; values (min_over's argument, None: not asked): an ops.TravelField of the grid's
    origin, resolution, dims and device, or a uint32-as-int32 / uint8 device tensor holding 4 nx ny nz bytes (one uint32 per voxel, x
    fastest, 0xFFFFFFFF = none).  -> (connectivity, rounds_per_check); ValueError otherwise."""
    if not isinstance(grid, OccupancyGrid):
        raise ValueError(f"Components: grid must be an ops.OccupancyGrid, got {type(grid).__name__}")
    if not _is_int(connectivity) or connectivity not in COMPONENT_CONNECTIVITIES:
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    if not _is_int(rounds_per_check) or not 1 <= rounds_per_check <= COMPONENT_MAX_ROUNDS_PER_CHECK:
        raise ValueError(f"rounds_per_check must be an integer in [1, {COMPONENT_MAX_ROUNDS_PER_CHECK}], got {rounds_per_check!r}")
    if values is not None:
        if isinstance(values, TravelField):
            diff = _grid_difference(grid, values)
            if diff:
                raise ValueError(f"values: the travel field's {diff[0]} differs from the grid's ({diff[2]} and {diff[1]})")
        else:
            nbytes = 4 * grid.dims[0] * grid.dims[1] * grid.dims[2]
            if not torch.is_tensor(values) or values.dtype not in (torch.int32, torch.uint8) or not values.is_contiguous() or \
                    values.numel() * values.element_size() != nbytes:
                raise ValueError(f"values must be an ops.TravelField or a contiguous int32 / uint8 tensor of {nbytes} bytes (one uint32 per "
                                 f"voxel), got {(tuple(values.shape), values.dtype) if torch.is_tensor(values) else type(values).__name__}")
            if values.device != grid.device:
                raise ValueError(f"values must live on the grid's device {grid.device}, got {values.device}")
    return int(connectivity), int(rounds_per_check)


class Components:
    """The connected components of a bit plane (components_kernels.hip, DESIGN.md 10 "Connected components"): two set voxels belong
    together iff a chain of adjacent set voxels joins them — adjacent: differing by at most 1 on every axis and on 1 (connectivity
    6), <= 2 (18) or <= 3 (26) axes; no corner-cut rule.  A component's root is its lowest linear index v = (k ny + j) nx + i, ids are
    0 .. n - 1 in ascending order of the root: a function of the plane and the connectivity alone, the same bits in every run.

    n: the number of components; labels: (nx ny nz,) int32 on the device holding uint32 bits, x fastest — the id of a set voxel,
    0xFFFFFFFF (-1 as int32) for a clear one; roots (n,) int32; sizes (n,) int64; sums (n,3) int64 of i, j, k; bbox (n,2,3) int32,
    minimum and maximum per axis; centroids (n,3) f32 = origin + (sum / size + 0.5) resolution, computed in float64 from the f32
    origin and resolution, then cast; rounds: the worklist rounds the last build needed.  roots is sized from a count of the plane's
    set bits (no component count exceeds it), so the build runs once: two synchronisations more than the worklist's own (that count,
    and n).  It reads the plane again on rebuild()."""

    def __init__(self, grid, connectivity=26, rounds_per_check=16):
        self.connectivity, self.rounds_per_check = check_components(grid, connectivity, rounds_per_check)
        self.grid = grid
        self.origin, self.resolution, self.dims, self.device, self.geom = grid.origin, grid.resolution, grid.dims, grid.device, grid.geom
        L = _lib.lib()
        self._buf = torch.empty(L.tohip_components_bytes(*self.dims), dtype=torch.uint8, device=self.device)
        self._ws = torch.empty(L.tohip_components_workspace_bytes(*self.dims), dtype=torch.uint8, device=self.device)
        self.labels = self._buf.view(torch.int32)
        self._roots = None
        self.n = self.rounds = 0
        self.rebuild()

    def _labels(self):
        return ptr(self._buf), self._buf.numel(), ctypes.byref(self.geom)

    def rebuild(self):
        """Label the plane again into the same buffers — after the grid has changed.  -> self."""
        dev = self.device
        capacity = self.grid.count()   # n never exceeds the set bits
        if self._roots is None or self._roots.numel() < capacity:
            self._roots = torch.empty(capacity, dtype=torch.int32, device=dev)
        n, rounds = ctypes.c_int64(0), ctypes.c_int64(0)
        _map_call(dev, "tohip_components_build", *self.grid._sizes(), self.connectivity, ptr(self._buf), self._buf.numel(), ptr(self._ws),
                  self._ws.numel(), self.rounds_per_check, ptr(self._roots), self._roots.numel(), ctypes.byref(n), ctypes.byref(rounds))
        self.n, self.rounds = int(n.value), int(rounds.value)
        C = self.n
        self.roots = self._roots[:C]
        self.sizes = torch.empty(C, dtype=torch.int64, device=dev)
        self.sums = torch.empty((C, 3), dtype=torch.int64, device=dev)
        self.bbox = torch.empty((C, 2, 3), dtype=torch.int32, device=dev)
        _map_call(dev, "tohip_components_stats", *self._labels(), C, ptr(self.sizes), ptr(self.sums), ptr(self.bbox))
        o = torch.from_numpy(np.asarray(self.origin, dtype=np.float32).astype(np.float64)).to(dev).reshape(1, 3)
        r = float(np.float32(self.resolution))
        self.centroids = (o + (self.sums.double() / self.sizes.double()[:, None] + 0.5) * r).float()
        return self

    def dense(self):
        """The ids as an (nx, ny, nz) int64 tensor (a copy), -1 where the voxel is clear: for tests and small grids."""
        nx, ny, nz = self.dims
        return self.labels.view(nz, ny, nx).to(torch.int64).permute(2, 1, 0).contiguous()

    def at(self, positions):
        """(M,3) world positions -> (M,) int64: the id of the position's voxel, -1 where it is clear, -2 out of range (beyond the
        apron, or not finite) or outside dims."""
        pos = covmap_points(positions, self.device, "Components.at")
        out = torch.empty(pos.shape[0], dtype=torch.int64, device=self.device)
        _map_call(self.device, "tohip_components_positions", *self._labels(), ptr(pos), pos.shape[0], ptr(out))
        return out

    def min_over(self, values):
        """The minimum of a value volume over each component -> (value (n,) int64, voxel (n,) int32): the smallest word over the
        component's voxels that is not 0xFFFFFFFF and the lowest linear index that attains it, -1 / -1 where there is none.  values: an
        ops.TravelField (its cost: how far is the nearest voxel of each component, and which is it — the weighted cost where the
        field has weights) or a tensor of one uint32 per voxel in the labels' layout."""
        check_components(self.grid, self.connectivity, self.rounds_per_check, values)
        buf = values.buf if isinstance(values, TravelField) else values
        value = torch.empty(self.n, dtype=torch.int64, device=self.device)
        voxel = torch.empty(self.n, dtype=torch.int32, device=self.device)
        _map_call(self.device, "tohip_components_min", *self._labels(), ptr(buf), buf.numel() * buf.element_size(), self.n, ptr(value), ptr(voxel))
        return value, voxel


EVID_UNKNOWN = -128        # an evidence value: never observed
EVID_DEFAULTS = dict(hit=17, miss=8, lmin=-40, lmax=70, threshold=0)


def check_evidence(origin, resolution, dims, hit=17, miss=8, lmin=-40, lmax=70, threshold=0, hit_plane=None, pass_plane=None, like=None,
                   own=()):
    """An evidence map's settings and a fold's planes, by name; needs no GPU.  origin, resolution, dims: an occupancy grid's
    (check_los).  hit and miss: integers in [1, 127]; lmin, lmax, threshold: integers with -127 <= lmin <= threshold < lmax <= 127.
    hit_plane and pass_plane (given together): two different ops.OccupancyGrids of the origin, resolution, dims and device of `like`
    (the map's occupied grid), neither of them one of `own` (the map's own planes).  -> (origin (3,) float32 array, resolution,
    dims, (hit, miss, lmin, lmax, threshold)); ValueError otherwise."""
    o, r, d, _ = check_los(origin, resolution, dims)
    for name, v in (("hit", hit), ("miss", miss)):
        if not _is_int(v) or not 1 <= v <= 127:
            raise ValueError(f"{name} must be an integer in [1, 127], got {v!r}")
    for name, v in (("lmin", lmin), ("lmax", lmax), ("threshold", threshold)):
        if not _is_int(v):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not -127 <= lmin <= threshold < lmax <= 127:
        raise ValueError(f"the clamps must satisfy -127 <= lmin <= threshold < lmax <= 127, got lmin = {lmin}, threshold = {threshold}, "
                         f"lmax = {lmax}")
    if (hit_plane is None) != (pass_plane is None):
        raise ValueError("hit_plane and pass_plane must be given together")
    if hit_plane is not None:
        for name, g in (("hit_plane", hit_plane), ("pass_plane", pass_plane)):
            if not isinstance(g, OccupancyGrid):
                raise ValueError(f"{name} must be an ops.OccupancyGrid, got {type(g).__name__}")
            if any(g is mine for mine in own):
                raise ValueError(f"{name} must not be one of the map's own planes")
            diff = _grid_difference(g, like) if like is not None else None
            if diff:
                raise ValueError("{}: its {} differs from the map's ({} and {})".format(name, *diff))
        if pass_plane is hit_plane:
            raise ValueError("pass_plane must not be the hit plane itself")
    return o, r, d, (int(hit), int(miss), int(lmin), int(lmax), int(threshold))


class EvidenceMap:
    """A hit/miss evidence map (evidence_kernels.hip, DESIGN.md 10 "Evidence map"): one signed 8-bit log-odds value per voxel of an
    occupancy grid's geometry, -128 = never observed, updated once per scan — + hit (up to lmax) where a return fell, otherwise - miss
    (down to lmin) where a ray passed — and the two planes derived from it: `occupied` (value > threshold) and `free` (observed and
    value <= threshold), ordinary OccupancyGrids that stay the same objects for the map's life, and `space`, a SpaceMap over them.
    line_of_sight, frontier, ClearanceField.build / rebuild, free_nodes and occlusion_grid= read them as they read any grid: a map
    that forgets what moved away.  Integers only: the same bytes in every run.  There is no decay without observation."""

    def __init__(self, origin=(0.0, 0.0, 0.0), resolution=0.1, dims=(64, 64, 64), hit=17, miss=8, lmin=-40, lmax=70, threshold=0, device="cuda"):
        _, _, _, self.params = check_evidence(origin, resolution, dims, hit, miss, lmin, lmax, threshold)
        self.occupied = OccupancyGrid(origin, resolution, dims, device=device)
        self.free = self.occupied.empty_like()
        self.space = SpaceMap(self.occupied, self.free)
        self._scan = SpaceMap(self.occupied.empty_like(), self.occupied.empty_like())   # one scan's hit and pass planes, empty between scans
        g = self.occupied
        self.origin, self.resolution, self.dims, self.device, self.geom = g.origin, g.resolution, g.dims, g.device, g.geom
        self.buf = torch.empty(_lib.lib().tohip_evid_bytes(*self.dims), dtype=torch.uint8, device=self.device)
        self._counts = torch.zeros(4, dtype=torch.int64, device=self.device)
        _map_call(self.device, "tohip_evid_init", *self._sizes())

    @classmethod
    def like(cls, grid, **params):
        """An empty map of an OccupancyGrid's origin, resolution, dims and device (the grid's bits are not read)."""
        if not isinstance(grid, OccupancyGrid):
            raise ValueError(f"EvidenceMap.like: grid must be an ops.OccupancyGrid, got {type(grid).__name__}")
        return cls(grid.origin, grid.resolution, grid.dims, device=grid.device, **params)

    @classmethod
    def from_space(cls, space, **params):
        """A map seeded from a SpaceMap, as settled as the clamps allow: its occupied voxels get lmax, its free ones lmin, the rest
        stay unknown (one fold of space.occupied / space.free with steps that reach the clamps, into an empty map; the SpaceMap is
        only read).  A later change of mind costs what the clamps say."""
        if not isinstance(space, SpaceMap):
            raise ValueError(f"EvidenceMap.from_space: space must be an ops.SpaceMap, got {type(space).__name__}")
        m = cls.like(space.occupied, **params)
        m._fold(space.occupied, space.free, False, steps=(127, 127))
        return m

    def _sizes(self):
        return ptr(self.buf), self.buf.numel(), ctypes.byref(self.geom)

    @property
    def threshold(self):
        return self.params[4]

    def _fold(self, hit_plane, pass_plane, clear, steps=None):
        hit, miss, lmin, lmax, threshold = self.params
        if steps is not None:
            hit, miss = steps
        self._counts.zero_()
        _map_call(self.device, "tohip_evid_fold", ptr(self.buf), self.buf.numel(), ptr(hit_plane.buf), ptr(pass_plane.buf), ptr(self.occupied.buf),
                  ptr(self.free.buf), self.occupied.buf.numel(), ctypes.byref(self.geom), hit, miss, lmin, lmax, threshold, int(bool(clear)),
                  ptr(self._counts))

    def fold(self, hit_plane, pass_plane, clear=False):
        """One scan given as planes of the caller's own: hit_plane (a set bit: a return fell in the voxel) and pass_plane (a ray
        passed through), two OccupancyGrids of the map's geometry.  A hit wins; a voxel moves once however many rays crossed it.
        clear=True empties both planes behind the fold (only the words that held a bit are written).  One launch, nothing read
        back; last_counts() tells what changed."""
        check_evidence(self.origin, self.resolution, self.dims, *self.params, hit_plane=hit_plane, pass_plane=pass_plane, like=self.occupied,
                       own=(self.occupied, self.free))
        self._fold(hit_plane, pass_plane, clear)

    def integrate(self, origin, points, max_range=None):
        """One scan: SpaceMap.integrate of the rays origin -> points[i] on the map's own two scratch planes — the carve, its per-ray
        flags, the insert of the rows whose ray was not truncated — then one fold, which also empties the scratch planes.
        -> the number of rays skipped (an endpoint out of range); that count is the one synchronisation."""
        skipped = self._scan.integrate(origin, points, max_range)
        self._fold(self._scan.occupied, self._scan.free, True)
        return skipped

    def _transfer(self, src, shift, mode, counts):
        _, _, lmin, lmax, threshold = self.params
        _map_call(self.device, "tohip_evid_transfer", *src._sizes(), *self._sizes(), ptr(self.occupied.buf), ptr(self.free.buf),
                  self.occupied.buf.numel(), *shift, XFER_MODES[mode], lmin, lmax, threshold, ptr(counts))

    def reframed(self, shift=None, dims=None, centre=None):
        """This map's values in another box of the same lattice -> a NEW EvidenceMap of the same parameters (tohip_evid_transfer,
        DESIGN.md 10 "Re-framing and merging maps"): a new buffer, both planes derived from it, empty scratch planes; shift, dims
        and centre as OccupancyGrid.reframed takes them.  This map is untouched, and consumers that hold it or its planes keep
        them: they are re-pointed or built anew.  One launch, nothing read back; the new map's last_counts() tells what it holds
        (known voxels, twice; occupied voxels; 0)."""
        s, d, origin = check_reframe(self, shift, dims, centre)
        hit, miss, lmin, lmax, threshold = self.params
        out = EvidenceMap(origin, self.resolution, d, hit, miss, lmin, lmax, threshold, device=self.device)
        out._transfer(self, s, "copy", out._counts)
        return out

    def _resample(self, src, affine, rule, mode, counts):
        _, _, lmin, lmax, threshold = self.params
        keep, a, frac = _affine_arg(affine)
        _map_call0(self.device, "tohip_evid_resample", *src._sizes(), *self._sizes(), ptr(self.occupied.buf), ptr(self.free.buf),
                   self.occupied.buf.numel(), a, frac, RESAMPLE_RULES[rule], XFER_MODES[mode], lmin, lmax, threshold, ptr(counts), None, 0)

    def transformed(self, pose, quat, origin=None, resolution=None, dims=None, like=None, rule="nearest"):
        """This map's values under a rigid transform and, if asked, at a finer resolution -> a NEW EvidenceMap of the same parameters
        (tohip_evid_resample, DESIGN.md 10 "Resampling maps"): a new buffer, both planes derived from it, empty scratch planes; this
        map is only read.  pose, quat and the new box as OccupancyGrid.transformed takes them.  rule 'nearest': the value of the
        voxel that holds the new voxel's centre — unbiased, the rule for fusing evidence; a wall one voxel thick may show pinholes.
        rule 'cover', for planning: the maximum over the 3 x 3 x 3 voxels around it under free < unknown < occupied — no occupied
        voxel is lost and nothing is free unless all it touches was free; walls and the unknown grow by up to a voxel.  One launch,
        nothing read back; the new map's last_counts() tells what it holds (known voxels, twice; occupied voxels; 0)."""
        frame, affine = check_transform(self, pose, quat, origin, resolution, dims, like, rule)
        hit, miss, lmin, lmax, threshold = self.params
        out = EvidenceMap(frame.origin, frame.resolution, frame.dims, hit, miss, lmin, lmax, threshold, device=self.device)
        out._resample(self, affine, rule, "copy", out._counts)
        return out

    def merge(self, other, mode="confident", counts=None, pose=None, quat=None, rule="nearest"):
        """Fuse another EvidenceMap of the same lattice into this one over the overlap of the two boxes, in place -> self; `other` is
        only read, both planes stay exact.  mode 'confident': per voxel the stronger belief wins (the larger |L|; at equal strength
        the positive, occupied one), the other's values clamped to this map's [lmin, lmax] first — a lattice join: commutative,
        associative and idempotent, so any merge order and any repetition give the same bytes.  mode 'add': independent evidence,
        clamp(L + L_other, lmin, lmax) where the other has observed the voxel — commutative, but a map merged twice is counted
        twice.  counts: a zero-filled (4,) int64 device tensor that receives += (values changed, voxels newly known, occupied
        voxels that appeared, that vanished), or None: last_counts() reports them.  pose (3,), quat (4,) wxyz: the other map's frame
        stands at world_self = R(quat) world_other + pose and its values are resampled (rule 'nearest', the unbiased one to fuse
        evidence with, or 'cover'; transformed says what each gives; this map must not be coarser than the other) before the same
        combine; an identity pose on this map's lattice takes the shift path.  One launch, nothing read back."""
        s, overlap, affine = check_merge_posed(self, other, mode, pose, quat, rule)
        _check_counts(counts, 4, self.device)
        if counts is None:
            counts = self._counts.zero_()
        if affine is not None:
            self._resample(other, affine, rule, mode, counts)
        elif overlap:
            self._transfer(other, s, mode, counts)
        return self

    def _coarsen(self, src, factor, offset, rule, mode, counts):
        _, _, lmin, lmax, threshold = self.params
        _map_call0(self.device, "tohip_evid_coarsen", *src._sizes(), *self._sizes(), ptr(self.occupied.buf), ptr(self.free.buf),
                   self.occupied.buf.numel(), factor, *offset, COARSEN_RULES[rule], XFER_MODES[mode], lmin, lmax, threshold, ptr(counts))

    def coarsened(self, factor=2, rule="cover", anchor="origin", origin=None, dims=None, like=None):
        """This map at `factor` times its voxel edge -> a NEW EvidenceMap of the same parameters (tohip_evid_coarsen, DESIGN.md 10
        "Coarsening maps"): a new buffer, both planes derived from it, empty scratch planes; this map is only read.  factor: an
        integer in [2, 8].  rule 'cover', for planning: the maximum of a coarse voxel's factor^3 children under free < unknown <
        occupied — the strongest occupied value if a child is occupied, else unknown if a child is unknown or lies outside this map,
        else the least free value: no occupied voxel is lost and nothing is free unless all it holds is free.  rule 'max', for
        display, occlusion and matching: the largest child as a number, unknown only where every child is — occupied if any child
        is, and optimistic about the unknown.  anchor, origin, dims, like: the coarse box, as OccupancyGrid.coarsened takes them.
        One launch, nothing read back; the new map's last_counts() tells what it holds (known voxels, twice; occupied voxels; 0)."""
        frame, o, rule = check_coarsen(self, factor, rule, anchor, origin, dims, like)
        hit, miss, lmin, lmax, threshold = self.params
        out = EvidenceMap(frame.origin, frame.resolution, frame.dims, hit, miss, lmin, lmax, threshold, device=self.device)
        out._coarsen(self, int(factor), o, rule, "copy", out._counts)
        return out

    def merge_fine(self, fine, mode="confident", rule="cover", counts=None):
        """Fuse a FINER EvidenceMap into this one, in place -> self; `fine` is only read, both planes stay exact.  The factor (2 .. 8)
        and the offset come from the two frames (check_merge_fine).  Each of this map's voxels reduces its children under `rule`
        (coarsened says what each gives; the threshold is this map's) and the result goes through merge's combine: mode 'confident'
        or 'add', counts as merge takes them.  One launch, nothing read back."""
        factor, o, rule = check_merge_fine(self, fine, mode, rule)
        _check_counts(counts, 4, self.device)
        if counts is None:
            counts = self._counts.zero_()
        self._coarsen(fine, factor, o, rule, mode, counts)
        return self

    def last_counts(self):
        """What the last fold changed -> (voxels updated, voxels newly known, occupied voxels that appeared, occupied voxels that
        vanished); synchronises.  A clearance field over the map needs a rebuild() when either of the last two is not zero."""
        return tuple(int(v) for v in self._counts.cpu().tolist())

    def log_odds(self, positions):
        """(M,3) world positions -> (values (M,) int8, state (M,) uint8): the voxel's value, -128 where it was never observed and
        where the position lies outside dims, beyond the apron or is not finite; state 0 unknown, 1 free, 2 occupied, 3 outside —
        SpaceMap.state's codes."""
        pos = covmap_points(positions, self.device, "EvidenceMap.log_odds")
        values = torch.empty(pos.shape[0], dtype=torch.int8, device=self.device)
        state = torch.empty(pos.shape[0], dtype=torch.uint8, device=self.device)
        _map_call(self.device, "tohip_evid_positions", *self._sizes(), self.threshold, ptr(pos), pos.shape[0], ptr(values), ptr(state))
        return values, state

    def uncertain(self, table=None):
        """The candidates of this map under a weight table (None: information_table of the map's settings) — the voxels inside dims
        whose weight table[L + 128] is positive, whatever their state — as a new OccupancyGrid of this geometry (pad bits 0):
        uncertain().export() lists them.  One launch (tohip_evid_weight_plane), nothing read back."""
        return _information_plane(self, table)[1]

    def information(self, table=None):
        """What is left to learn in this map -> a 0-d int64 device tensor: the sum of table[L + 128] over the voxels inside dims, in
        the table's units (the default table: 1/4096 bit); 0 for a map whose every voxel sits at a clamp.  One launch, nothing read
        back: int(m.information()) is the synchronisation."""
        total = torch.zeros((), dtype=torch.int64, device=self.device)
        _information_plane(self, table, total)
        return total

    def _bricks(self):
        nx, ny, nz = self.dims
        return (nx + 3) // 4, (ny + 3) // 4, (nz + 1) // 2

    def dense(self):
        """The values as an (nx, ny, nz) int8 tensor (a copy, out of brick order): for tests and small grids."""
        nx, ny, nz = self.dims
        nbx, nby, nbz = self._bricks()
        v = self.buf[256:].view(torch.int8).view(nbz, nby, nbx, 2, 4, 4).permute(2, 5, 1, 4, 0, 3).reshape(4 * nbx, 4 * nby, 2 * nbz)
        return v[:nx, :ny, :nz].contiguous()

    def load(self, values):
        """Replace the map's content by `values`, an (nx, ny, nz) integer tensor as dense() gives it — each -128 or in [lmin, lmax] —
        and derive both planes from it: for tests, small grids and a map saved earlier.  Plain tensor copies, no kernel of the
        library; the scratch planes and last_counts() are left as they are.  -> self."""
        _, _, lmin, lmax, threshold = self.params
        if (not torch.is_tensor(values) or values.is_floating_point() or values.dtype == torch.bool or tuple(values.shape) != tuple(self.dims)):
            raise ValueError(f"values must be an integer tensor of shape {tuple(self.dims)}, got "
                             f"{tuple(values.shape) if torch.is_tensor(values) else type(values).__name__}")
        v = values.to(device=self.device, dtype=torch.int64)
        if not bool(((v == EVID_UNKNOWN) | ((v >= lmin) & (v <= lmax))).all()):
            raise ValueError(f"values must each be -128 or lie in [lmin, lmax] = [{lmin}, {lmax}]")
        nx, ny, nz = self.dims
        nbx, nby, nbz = self._bricks()
        full = torch.full((4 * nbx, 4 * nby, 2 * nbz), EVID_UNKNOWN, dtype=torch.int64, device=self.device)
        full[:nx, :ny, :nz] = v
        bricks = full.view(nbx, 4, nby, 4, nbz, 2).permute(4, 2, 0, 5, 3, 1).reshape(-1, 4, 8)   # (word, byte of the plane word, bit)
        self.buf[256:] = bricks.reshape(-1).to(torch.int8).view(torch.uint8)
        weights = (1 << torch.arange(8, device=self.device, dtype=torch.int64))
        for plane, bits in ((self.occupied, bricks > threshold), (self.free, (bricks != EVID_UNKNOWN) & (bricks <= threshold))):
            plane.buf[256:] = (bits.to(torch.int64) * weights).sum(dim=2).to(torch.uint8).reshape(-1)
        return self


GROUND_MAX_HEADROOM = 64   # voxels
GROUND_MAX_STEP = 4        # voxels
GROUND_MAX_DROP = 2048     # voxels a snap may look down


def check_ground(map, headroom, step=1, unknown="free", H=None, max_drop=None):
    """A ground layer's settings and a snap's, by name; needs no GPU.  map: an OccupancyGrid, a SpaceMap or an EvidenceMap (its planes);
    headroom: a finite number of metres > 0 whose H = ceil(float64(headroom) / float64(f32 resolution)) lies in [1, 64] — or H itself,
    an integer in that range, instead; step: an integer number of voxels in [0, 4] with step + 1 <= H; unknown: 'free' or 'obstacle'
    (which needs a map with a free plane); max_drop (None: not asked): an integer number of voxels in [0, 2048].
    -> (occupied grid, free plane or None, H, step); ValueError otherwise."""
    if not isinstance(map, (OccupancyGrid, SpaceMap, EvidenceMap)):
        raise ValueError(f"GroundLayer: the map must be an ops.OccupancyGrid, an ops.SpaceMap or an ops.EvidenceMap, got {type(map).__name__}")
    occupied, free = (map, None) if isinstance(map, OccupancyGrid) else (map.occupied, map.free)
    if unknown not in FIELD_UNKNOWN:
        raise ValueError(f"unknown must be 'free' or 'obstacle', got {unknown!r}")
    if unknown == "obstacle" and free is None:
        raise ValueError("unknown='obstacle' needs an ops.SpaceMap or an ops.EvidenceMap (the free plane tells unknown from free), got an OccupancyGrid")
    r = occupied.resolution
    if H is None:
        m = _float_or_nan(headroom) if _is_real(headroom) else float("nan")
        H = int(np.ceil(m / r)) if np.isfinite(m) and m > 0.0 and m / r <= GROUND_MAX_HEADROOM + 1 else 0
        if not 1 <= H <= GROUND_MAX_HEADROOM:
            raise ValueError(f"headroom must be a finite number of metres > 0 and at most {GROUND_MAX_HEADROOM} voxels "
                             f"({GROUND_MAX_HEADROOM * r:g} m at this resolution), got {headroom!r}")
    elif not _is_int(H) or not 1 <= H <= GROUND_MAX_HEADROOM:
        raise ValueError(f"H must be an integer number of voxels in [1, {GROUND_MAX_HEADROOM}], got {H!r}")
    H = int(H)
    if not _is_int(step) or not 0 <= step <= GROUND_MAX_STEP:
        raise ValueError(f"step must be an integer number of voxels in [0, {GROUND_MAX_STEP}], got {step!r}")
    if step + 1 > H:
        raise ValueError(f"step {int(step)} needs a headroom of at least {int(step) + 1} voxels (the slab over a step must be clear), got H = {H}")
    if max_drop is not None and (not _is_int(max_drop) or not 0 <= max_drop <= GROUND_MAX_DROP):
        raise ValueError(f"max_drop must be an integer number of voxels in [0, {GROUND_MAX_DROP}], got {max_drop!r}")
    return occupied, (free if unknown == "obstacle" else None), H, int(step)


class GroundLayer:
    """The ground layer of a map (ground_kernels.hip, DESIGN.md 10 "Ground layer"): for a robot that DRIVES — headroom metres tall,
    climbing steps of `step` voxels — the planes that tell where it can stand and what is an obstacle for it.  support: occupied
    voxels with H clear voxels above; ground: the support voxels whose eight neighbour columns continue the surface within +-step
    levels or are walls; obstacles: what is occupied and not floor (the ground and what is stacked solid under it) — with
    unknown='obstacle' the unknown voxels too; drive: the standing voxel over every ground voxel and the `step` voxels above it.
    All four are ordinary OccupancyGrids of the map's geometry; space = SpaceMap(obstacles, drive) and field(max_dist), a
    ClearanceField over obstacles, go wherever a space and a field go: a TravelField over them covers exactly the places the robot's
    centre can be.  Integers only: the same bits in every run.  rebuild() follows the map."""

    def __init__(self, map, headroom=None, step=1, unknown="free", H=None):
        self.occupied, self.free, self.H, self.step = check_ground(map, headroom, step, unknown, H=H)
        self.map, self.unknown = map, unknown
        g = self.occupied
        self.origin, self.resolution, self.dims, self.device, self.geom = g.origin, g.resolution, g.dims, g.device, g.geom
        self.support, self.ground, self.obstacles, self.drive = (g.empty_like() for _ in range(4))
        self.space = SpaceMap(self.obstacles, self.drive)
        self.rebuild()

    def rebuild(self):
        """Recompute the four planes from the map as it is now — after more inserts, carves or folds — into the same buffers: three
        launches, nothing read back; fields and travel fields over the layer then rebuild as over any map.  -> self."""
        with torch.cuda.device(self.device):
            check(_lib.lib().tohip_ground_build(ptr(self.occupied.buf), ptr(self.free.buf) if self.free is not None else None,
                                                self.occupied.buf.numel(), ctypes.byref(self.geom), self.H, self.step,
                                                1 if self.free is not None else 0, ptr(self.support.buf), ptr(self.ground.buf),
                                                ptr(self.obstacles.buf), ptr(self.drive.buf), stream_ptr(), 0), "tohip_ground_build")
        return self

    def field(self, max_dist=None, D=None):
        """A ClearanceField over the layer's obstacles, truncated at max_dist metres (or D voxels): the floor the robot rolls on is
        no obstacle in it.  A new field each call; field.rebuild() follows layer.rebuild()."""
        return ClearanceField(self.obstacles, max_dist, D=D)

    def snap(self, positions, max_drop):
        """(M,3) world positions -> (standing (M,3) f32, drop (M,) int32): the centre of the standing voxel — a drive voxel right
        above a ground voxel — at or at most max_drop voxels below each position's voxel, and how many voxels below.  drop -1: none;
        -2: out of range (beyond the apron, or not finite) or outside dims; standing is NaN for both.  What turns a sensor-height
        pose into a travel source and a row of a path in the slab into a wheel position.  One launch."""
        check_ground(self.occupied, None, self.step, H=self.H, max_drop=max_drop)
        pos = covmap_points(_check_rows3(positions, "positions", empty=True), self.device, "GroundLayer.snap")
        standing = torch.empty((pos.shape[0], 3), dtype=torch.float32, device=self.device)
        drop = torch.empty(pos.shape[0], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().tohip_ground_snap(ptr(self.ground.buf), ptr(self.drive.buf), self.ground.buf.numel(), ctypes.byref(self.geom),
                                               ptr(pos), pos.shape[0], int(max_drop), ptr(standing), ptr(drop), stream_ptr(), 0),
                  "tohip_ground_snap")
        return standing, drop


SCAN_MAX_WINDOW = (16, 16, 4)     # voxels a search window reaches per axis
SCAN_MAX_ROTATIONS = 256
SCAN_MAX_POINTS = 1 << 22
SCAN_MAX_CANDIDATES = 1 << 22     # K S of a window search, B of explicit candidates


def _host_rows(v, cols, name, rows=None):
    """Host numbers -> a finite (rows, cols) float64 array: a list, a numpy array or a tensor (a device tensor is read back);
    a single row may come flat."""
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is not None and a.ndim == 1 and a.shape[0] == cols:
        a = a.reshape(1, cols)
    if a is None or a.ndim != 2 or a.shape[1] != cols or a.shape[0] == 0 or (rows is not None and a.shape[0] != rows) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be ({'B' if rows is None else rows},{cols}) finite numbers on the host, got "
                         f"{tuple(a.shape) if a is not None else type(v).__name__}")
    return a


def scan_rotations(quats, name="rotations"):
    """(K,4) quaternions wxyz on the host -> (K,3,3) f32: each normalised in f64, the matrix of p -> q p conj(q) in f64 — depth_scan's
    convention — rounded once to f32 (synth.scan_rotation)."""
    q = _host_rows(quats, 4, name)
    n = np.sqrt((q * q).sum(axis=1))
    if not (n > 0.0).all():
        raise ValueError(f"{name}: a quaternion of length 0")
    w, x, y, z = (q / n[:, None]).T
    R = np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                  2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                  2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)], axis=1)
    return R.astype(np.float32).reshape(-1, 3, 3)


def check_scan_match(map, floor=None, unknown_value=0, window=None, n_rotations=None):
    """A scan matcher's settings and a search's, by name; needs no GPU.  map: an ops.EvidenceMap (a SpaceMap goes through
    EvidenceMap.from_space); floor: None (no floor) or an integer in [-127, 0]; unknown_value: an integer in [-127, 0]; window (None:
    not asked): three integers (wx, wy, wz), 0 <= wx, wy <= 16, 0 <= wz <= 4; n_rotations (None: not asked): an integer K in [1, 256]
    with K (2wx+1)(2wy+1)(2wz+1) <= 2^22.  -> (floor as the library takes it, unknown_value, window or None); ValueError otherwise."""
    if not isinstance(map, EvidenceMap):
        raise ValueError(f"ScanMatcher: the map must be an ops.EvidenceMap (EvidenceMap.from_space takes a SpaceMap), got {type(map).__name__}")
    if floor is not None and (not _is_int(floor) or not -127 <= floor <= 0):
        raise ValueError(f"floor must be None or an integer in [-127, 0], got {floor!r}")
    if not _is_int(unknown_value) or not -127 <= unknown_value <= 0:
        raise ValueError(f"unknown_value must be an integer in [-127, 0], got {unknown_value!r}")
    if window is not None:
        try:
            w = tuple(window)
        except TypeError:
            w = ()
        if len(w) != 3 or not all(_is_int(c) and 0 <= c <= m for c, m in zip(w, SCAN_MAX_WINDOW)):
            raise ValueError(f"window must be three integers (wx, wy, wz) with 0 <= wx, wy <= 16 and 0 <= wz <= 4, got {window!r}")
        window = tuple(int(c) for c in w)
    if n_rotations is not None:
        S = (2 * window[0] + 1) * (2 * window[1] + 1) * (2 * window[2] + 1) if window is not None else 1
        if not _is_int(n_rotations) or not 1 <= n_rotations <= SCAN_MAX_ROTATIONS or n_rotations * S > SCAN_MAX_CANDIDATES:
            raise ValueError(f"the rotations must number 1 .. {SCAN_MAX_ROTATIONS} with K (2wx+1)(2wy+1)(2wz+1) <= 2^22, got K = {n_rotations!r}"
                             f"{'' if window is None else ' and a window of ' + str(S) + ' shifts'}")
    return (-127 if floor is None else int(floor)), int(unknown_value), window


class ScanMatcher:
    """Scan-to-map registration on an evidence map (scanmatch_kernels.hip, DESIGN.md 10 "Scan matching"): a scan of sensor-frame points
    is scored against the map's log-odds at candidate poses — the sum over the points of the value of the voxel each falls in, max(L,
    floor) where the voxel was observed and unknown_value elsewhere — and correlate() scores every pose of a window of integer voxel
    shifts around a prior, for a list of rotations, in one launch.  The matcher holds the SCORE TABLE, a second copy of the map's
    bytes with floor and unknown_value applied: refresh() re-prepares it after the map took another scan.  Integers only: the same
    scores in every run.  Points: (N,3) floating point on the map's device, 1 <= N <= 2^22; poses and quaternions: host numbers."""

    def __init__(self, map, floor=None, unknown_value=0):
        self.floor, self.unknown_value, _ = check_scan_match(map, floor, unknown_value)
        self.map = map
        self.origin, self.resolution, self.dims, self.device, self.geom = map.origin, map.resolution, map.dims, map.device, map.geom
        self.table = torch.empty(map.buf.numel(), dtype=torch.uint8, device=self.device)
        self.refresh()

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            check(getattr(_lib.lib(), name)(*args, stream_ptr(), 0), name)

    def refresh(self):
        """Prepare the table from the map as it is now: one launch, nothing read back; the level tables of levels() are dropped.
        -> self."""
        self._levels = None
        self._call("tohip_scan_prepare", *self.map._sizes(), self.floor, self.unknown_value, ptr(self.table), self.table.numel())
        return self

    def _points(self, points, what):
        pts = covmap_points(points, self.device, what)
        if not 1 <= pts.shape[0] <= SCAN_MAX_POINTS:
            raise ValueError(f"{what}: the scan must hold 1 .. 2^22 points, got {pts.shape[0]}")
        return pts

    def poses(self, poses, quats):
        """Host poses (B,3) (or one (3,) for all) and quaternions (B,4) -> the (B,12) f32 device tensor the kernels take: R row-major
        from scan_rotations, then t rounded to f32.  The copy to the device comes from pageable host memory: it waits for the current
        stream.  A caller that must not wait builds the tensor once and hands it to correlate / score as poses12=."""
        R = scan_rotations(quats, "quats")
        t = _host_rows(poses, 3, "poses")
        if t.shape[0] == 1 and R.shape[0] > 1:
            t = np.repeat(t, R.shape[0], axis=0)
        if t.shape[0] != R.shape[0]:
            raise ValueError(f"poses and quats must have as many rows, got {t.shape[0]} and {R.shape[0]}")
        rows = np.concatenate([R.reshape(-1, 9), t.astype(np.float32)], axis=1)
        return torch.from_numpy(np.ascontiguousarray(rows)).to(self.device)

    def _poses12(self, poses12, what):
        if (not torch.is_tensor(poses12) or poses12.dtype != torch.float32 or poses12.dim() != 2 or poses12.shape[1] != 12 or poses12.shape[0] == 0
                or poses12.device != self.device or not poses12.is_contiguous()):
            raise ValueError(f"{what}: poses12 must be a contiguous (B,12) float32 tensor on {self.device} (ScanMatcher.poses), got "
                             f"{(tuple(poses12.shape), poses12.dtype, str(poses12.device)) if torch.is_tensor(poses12) else type(poses12).__name__}")
        return poses12

    def correlate(self, points, pose, rotations, window, poses12=None):
        """Every pose of a search window: pose (3,), the prior translation; rotations (K,4) quaternions, the caller's list; window (wx,
        wy, wz) in voxels.  -> (scores (K, 2wz+1, 2wy+1, 2wx+1) int32, used (K,) int32) on the device: scores[k][dz+wz][dy+wy][dx+wx]
        is the score of rotation k with every point's voxel moved by (dx, dy, dz); used[k] the points in range under rotation k.  The
        table is read, not the map: refresh() after an integrate.  poses12: the (K,12) device tensor of poses() instead of pose and
        rotations, which are then not looked at.  Two clears and one launch, nothing read back; without poses12 the poses' copy to the
        device waits for the current stream first (poses())."""
        pts = self._points(points, "ScanMatcher.correlate")
        if poses12 is None:
            poses12 = self.poses(_host_rows(pose, 3, "pose", rows=1), rotations)
        else:
            poses12 = self._poses12(poses12, "ScanMatcher.correlate")
        K = poses12.shape[0]
        _, _, (wx, wy, wz) = check_scan_match(self.map, None, self.unknown_value, window, K)
        scores = torch.empty((K, 2 * wz + 1, 2 * wy + 1, 2 * wx + 1), dtype=torch.int32, device=self.device)
        used = torch.empty(K, dtype=torch.int32, device=self.device)
        self._call("tohip_scan_correlate", ptr(self.table), self.table.numel(), ctypes.byref(self.geom), self.unknown_value, ptr(pts),
                   pts.shape[0], ptr(poses12), K, wx, wy, wz, ptr(scores), scores.numel() * 4, ptr(used))
        return scores, used

    def score(self, points, poses, quats, shifts=None, poses12=None):
        """B explicit candidates, straight from the map's bytes (no table): poses (B,3) and quats (B,4) on the host, shifts None or
        (B,3) integers, voxels added to every point's voxel (a device int32 tensor is taken as it is).  -> (score, used, inside,
        known), each (B,) int32 on the device: the score; the points in range; those whose shifted voxel lies inside dims; those that
        met an observed voxel there.  What a particle filter weighs its particles by.  poses12: the (B,12) device tensor of poses()
        instead of poses and quats.  Four clears and one launch, nothing read back; without poses12, and with shifts from the host,
        the copies to the device wait for the current stream first (poses())."""
        pts = self._points(points, "ScanMatcher.score")
        if poses12 is None:
            poses12 = self.poses(poses, quats)
        else:
            poses12 = self._poses12(poses12, "ScanMatcher.score")
        B = poses12.shape[0]
        if not 1 <= B <= SCAN_MAX_CANDIDATES:
            raise ValueError(f"ScanMatcher.score: 1 .. 2^22 candidates, got {B}")
        if shifts is not None:
            if not torch.is_tensor(shifts):
                shifts = torch.from_numpy(np.ascontiguousarray(np.asarray(shifts, dtype=np.int64).astype(np.int32)))
            if shifts.is_floating_point() or tuple(shifts.shape) != (B, 3):
                raise ValueError(f"shifts must be ({B},3) integers, got {tuple(shifts.shape)} of {shifts.dtype}")
            shifts = shifts.to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty((4, B), dtype=torch.int32, device=self.device)
        self._call("tohip_scan_score", *self.map._sizes(), self.floor, self.unknown_value, ptr(pts), pts.shape[0], ptr(poses12),
                   ptr(shifts), B, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]))
        return out[0], out[1], out[2], out[3]

    def best(self, scores):
        """The best candidate of correlate's scores -> int32[8] on the device: flat index, k, dx, dy, dz, score, ties, 0 — the maximum
        of the key (score, then smaller dx^2 + dy^2 + dz^2, then lower flat index); ties: the candidates whose score equals the best.
        One launch of one block, nothing read back."""
        if (not torch.is_tensor(scores) or scores.dtype != torch.int32 or scores.dim() != 4 or not scores.is_contiguous()
                or scores.device != self.device or any(n % 2 == 0 for n in scores.shape[1:])):
            raise ValueError("scores must be the contiguous (K, 2wz+1, 2wy+1, 2wx+1) int32 tensor correlate returned")
        K, nzw, nyw, nxw = scores.shape
        window = (nxw // 2, nyw // 2, nzw // 2)
        check_scan_match(self.map, None, self.unknown_value, window, K)
        best = torch.empty(8, dtype=torch.int32, device=self.device)
        self._call("tohip_scan_best", ptr(scores), K, *window, ptr(best))
        return best

    # ---- relocalisation: exact branch and bound over wide windows (scansearch_kernels.hip, DESIGN.md 10 "Relocalisation")

    def levels(self, H):
        """The level tables T_1 .. T_H of the score table -> an (H, table bytes) uint8 tensor, row h - 1 the sliding maximum of the
        table over 2^h x 2^h voxels in x and y (check_scan_search: 0 <= H <= 6; H = 0: no rows).  Built once — H launches — and kept;
        refresh() drops them, a larger H builds them anew.  H + 1 copies of the table in all: 7.3 MB each for a 405 x 405 x 45 room."""
        check_scan_search(self.map, levels=H)
        if self._levels is None or self._levels.shape[0] < H:
            lv = torch.empty((H, self.table.numel()), dtype=torch.uint8, device=self.device)
            if H > 0:
                self._call("tohip_reloc_levels", ptr(self.table), self.table.numel(), ctypes.byref(self.geom), self.unknown_value, H, ptr(lv),
                           lv.numel())
            self._levels = lv
        return self._levels[:H]

    def _workspace(self, capacity):
        return torch.empty(_lib.lib().tohip_reloc_workspace_bytes(capacity), dtype=torch.uint8, device=self.device)

    def bound(self, points, nodes, level, pose=None, rotations=None, poses12=None):
        """The bounds of explicit nodes of one level: nodes (M,4) integers (k, sx, sy, sz), any order, 1 <= M <= 2^22 (a device int32
        tensor is taken as it is); pose and rotations, or poses12, as correlate takes them.  -> (bounds (M,) int32, used (K,) int32) on
        the device: bounds[i] = the sum over the points in range under rotation k of B_level(voxel + (sx, sy, sz)) - 128 used[k], an
        upper bound of the score of every candidate (k, dx in [sx, sx + 2^level), dy in [sy, sy + 2^level), dz = sz) and at level 0
        the score itself; INT32_MIN for a k outside [0, K).  Nothing read back."""
        pts = self._points(points, "ScanMatcher.bound")
        _, level, _, _ = check_scan_search(self.map, levels=level)
        if poses12 is None:
            poses12 = self.poses(_host_rows(pose, 3, "pose", rows=1), rotations)
        else:
            poses12 = self._poses12(poses12, "ScanMatcher.bound")
        K = poses12.shape[0]
        check_scan_search(self.map, n_rotations=K)
        if not torch.is_tensor(nodes):
            nodes = torch.from_numpy(np.ascontiguousarray(np.asarray(nodes, dtype=np.int64).astype(np.int32)))
        if nodes.is_floating_point() or nodes.dim() != 2 or nodes.shape[1] != 4 or not 1 <= nodes.shape[0] <= SCAN_MAX_CANDIDATES:
            raise ValueError(f"nodes must be (M,4) integers (k, sx, sy, sz) with 1 <= M <= 2^22, got {tuple(nodes.shape)} of {nodes.dtype}")
        nodes = nodes.to(device=self.device, dtype=torch.int32).contiguous()
        M = nodes.shape[0]
        table = self.table if level == 0 else self.levels(level)[level - 1]
        bounds = torch.empty(M, dtype=torch.int32, device=self.device)
        used = torch.empty(K, dtype=torch.int32, device=self.device)
        work = self._workspace(M)
        self._call("tohip_reloc_bounds", ptr(table), table.numel(), ctypes.byref(self.geom), self.unknown_value, level, ptr(pts), pts.shape[0],
                   ptr(poses12), K, ptr(nodes), M, ptr(bounds), ptr(used), ptr(work), work.numel())
        return bounds, used

    def search(self, points, pose, rotations, window, levels=None, capacity=1 << 22, poses12=None):
        """The best candidate of a WIDE window, exactly: window (wx, wy, wz) with 0 <= wx, wy <= 2048, 0 <= wz <= 4, K <= 256
        rotations; levels H in [0, 6] (None: scan_search_levels(window)).  Branch and bound over the level tables: equal to best(
        correlate(...)) where correlate's window reaches, bit for bit.  -> the record, (18,) int64 on the device: flat index ((k
        (2wz+1) + dz+wz)(2wy+1) + dy+wy)(2wx+1) + dx+wx, k, dx, dy, dz, score, ties, status, incumbent, evaluated, H, nodes[0 .. H].
        A level of more than `capacity` nodes stops the search: status = count << 3 | (level + 1) and flat index -1 (scan_search_status
        names it).  About 5 H + 4 launches, enqueued at once; nothing read back."""
        pts = self._points(points, "ScanMatcher.search")
        if poses12 is None:
            poses12 = self.poses(_host_rows(pose, 3, "pose", rows=1), rotations)
        else:
            poses12 = self._poses12(poses12, "ScanMatcher.search")
        K = poses12.shape[0]
        (wx, wy, wz), H, capacity, _ = check_scan_search(self.map, window, levels, capacity, K)
        lv = self.levels(H)
        record = torch.empty(SCAN_SEARCH_RECORD, dtype=torch.int64, device=self.device)
        work = self._workspace(capacity)
        self._call("tohip_reloc_search", ptr(self.table), self.table.numel(), ptr(lv) if H > 0 else ptr(None), lv.numel(), ctypes.byref(self.geom),
                   self.unknown_value, H, ptr(pts), pts.shape[0], ptr(poses12), K, wx, wy, wz, capacity, ptr(record), ptr(work), work.numel())
        return record

    # ---- fine registration: damped Gauss-Newton on the trilinear table (scanreg_kernels.hip, DESIGN.md 10 "Scan registration")

    def normal(self, points, poses=None, quats=None, poses12=None, state=None):
        """The integer normal equations of B poses (1 <= B <= 256) -> records (B, 32) int64 on the device: per pose the upper triangle
        of H = sum J J^T (21, row-major), sum J e (6), sum e^2, used, inside (all eight corners inside dims), 0, 0 — J and e of each
        point by the definitions of DESIGN.md 10 "Scan registration", on the trilinear interpolation of the TABLE (refresh() after
        an integrate).  A pose whose translation is out of range has an all-zero record.  poses (B,3) and quats (B,4) on the host, or
        poses12, the (B,12) device tensor of poses().  state: a register() state; the poses it has frozen are not evaluated (their
        records stay zero).  One clear and one launch, nothing read back."""
        pts = self._points(points, "ScanMatcher.normal")
        poses12 = self.poses(poses, quats) if poses12 is None else self._poses12(poses12, "ScanMatcher.normal")
        B = poses12.shape[0]
        check_scan_register(self.map, n_poses=B)
        if state is not None:
            state = self._state(state, B, "ScanMatcher.normal")
        records = torch.empty((B, SCAN_REGISTER_RECORD), dtype=torch.int64, device=self.device)
        self._call("tohip_scanreg_normal", ptr(self.table), self.table.numel(), ctypes.byref(self.geom), self.unknown_value, ptr(pts),
                   pts.shape[0], ptr(poses12), B, ptr(state), ptr(records))
        return records

    def _state(self, state, B, what):
        if (not torch.is_tensor(state) or state.dtype != torch.int64 or tuple(state.shape) != (B, SCAN_REGISTER_STATE) or state.device != self.device
                or not state.is_contiguous()):
            raise ValueError(f"{what}: state must be a contiguous ({B},{SCAN_REGISTER_STATE}) int64 tensor on {self.device} (scan_register_start), got "
                             f"{(tuple(state.shape), state.dtype, str(state.device)) if torch.is_tensor(state) else type(state).__name__}")
        return state

    def step(self, records, state, poses12, dof="xyzrpw", tol_t=None, tol_r=None):
        """One Gauss-Newton step of every pose, in place: records (B,32) int64 at the trial poses, state (B,64) int64 and poses12
        (B,12) f32, which receives the next trial poses.  What register() calls after each normal(); one launch, nothing read back."""
        B = state.shape[0] if torch.is_tensor(state) and state.dim() == 2 else 0
        _, mask, tol_t, tol_r = check_scan_register(self.map, None, dof, tol_t, tol_r, B)
        state, poses12 = self._state(state, B, "ScanMatcher.step"), self._poses12(poses12, "ScanMatcher.step")
        if (not torch.is_tensor(records) or records.dtype != torch.int64 or tuple(records.shape) != (B, SCAN_REGISTER_RECORD)
                or records.device != self.device or not records.is_contiguous() or poses12.shape[0] != B):
            raise ValueError(f"ScanMatcher.step: records must be the contiguous ({B},{SCAN_REGISTER_RECORD}) int64 tensor normal() returned and "
                             f"poses12 ({B},12)")
        self._call("tohip_scanreg_step", ptr(records), ptr(state), B, float(np.float32(self.resolution)), mask, tol_t, tol_r, ptr(poses12))
        return state

    def register(self, points, poses=None, quats=None, iterations=30, dof="xyzrpw", tol_t=None, tol_r=None, state=None, poses12=None):
        """Refine B poses (1 <= B <= 256) of one scan: `iterations` (1 .. 256) rounds of normal() and step() — Levenberg-Marquardt on
        the integer normal equations, each pose with its own lambda, frozen once it has converged, stalled, met a degenerate system
        or lost every point.  -> the device state (B, 64) int64 (f64 words by their bits; scan_register_fields names them).  dof: a
        string over 'x y z r p w' (translation, roll, pitch, yaw about the world's axes) or a 6-bit mask; tol_t in voxels (None:
        1/256), tol_r in radians (None: 1e-4).  The start: poses (B,3) and quats (B,4) on the host — one copy to the device, which
        waits for the current stream — or state and poses12, the device tensors of scan_register_start (they are not modified).  Every
        pose of a batch is bitwise its own single run.  The table is read, not the map: refresh() after an integrate.  Per iteration
        one clear and two launches, all enqueued at once; nothing is read back."""
        pts = self._points(points, "ScanMatcher.register")
        if state is None:
            R = scan_rotations(quats, "quats")
            t = _host_rows(poses, 3, "poses")
            if t.shape[0] == 1 and R.shape[0] > 1:
                t = np.repeat(t, R.shape[0], axis=0)
            if t.shape[0] != R.shape[0]:
                raise ValueError(f"poses and quats must have as many rows, got {t.shape[0]} and {R.shape[0]}")
            iterations, mask, tol_t, tol_r = check_scan_register(self.map, iterations, dof, tol_t, tol_r, t.shape[0])
            st, p12 = scan_register_start(t, _host_rows(quats, 4, "quats"))
            state, poses12 = torch.from_numpy(st).to(self.device), torch.from_numpy(p12).to(self.device)
        else:
            B = state.shape[0] if torch.is_tensor(state) and state.dim() == 2 else 0
            iterations, mask, tol_t, tol_r = check_scan_register(self.map, iterations, dof, tol_t, tol_r, B)
            state = self._state(state, B, "ScanMatcher.register").clone()
            poses12 = self._poses12(poses12, "ScanMatcher.register").clone()
            if poses12.shape[0] != B:
                raise ValueError(f"ScanMatcher.register: state and poses12 must have as many rows, got {B} and {poses12.shape[0]}")
        B = state.shape[0]
        records = torch.empty((B, SCAN_REGISTER_RECORD), dtype=torch.int64, device=self.device)
        r = float(np.float32(self.resolution))
        for _ in range(iterations):
            self._call("tohip_scanreg_normal", ptr(self.table), self.table.numel(), ctypes.byref(self.geom), self.unknown_value, ptr(pts),
                       pts.shape[0], ptr(poses12), B, ptr(state), ptr(records))
            self._call("tohip_scanreg_step", ptr(records), ptr(state), B, r, mask, tol_t, tol_r, ptr(poses12))
        return state


SCAN_REGISTER_RECORD = _lib.CONSTANTS["TOHIP_SCANREG_RECORD"]   # int64 words of a pose's record
SCAN_REGISTER_STATE = _lib.CONSTANTS["TOHIP_SCANREG_STATE"]     # 8-byte words of a pose's state
SCAN_REGISTER_MAX_ITERATIONS = 256
SCAN_REGISTER_LAMBDA0 = 2.0 ** -10
SCAN_REGISTER_TOL_T, SCAN_REGISTER_TOL_R = 1.0 / 256.0, 1.0e-4   # voxels, radians
SCAN_REGISTER_STATUS = ("RUNNING", "CONVERGED", "STALLED", "DEGENERATE", "EMPTY")
SCAN_REGISTER_DOF = "xyzrpw"
# the state's words: t (3), q (4), lambda, the last step (6), status, iterations, accepted, trial t (3), trial q (4), the record (32)
SCAN_REGISTER_FIELDS = dict(t=0, q=3, lam=7, delta=8, status=14, iterations=15, accepted=16, trial_t=17, trial_q=20, record=24)


def scan_dof_mask(dof):
    """A string over 'x y z r p w' (each at most once, one at least) or a mask in [1, 63] -> the 6-bit mask: bit i frees degree of
    freedom i of (x, y, z, roll, pitch, yaw)."""
    if isinstance(dof, str):
        if not dof or len(set(dof)) != len(dof) or any(c not in SCAN_REGISTER_DOF for c in dof):
            raise ValueError(f"dof must name each of 'x y z r p w' at most once and one at least, got {dof!r}")
        return sum(1 << SCAN_REGISTER_DOF.index(c) for c in dof)
    if _is_int(dof) and 1 <= dof <= 63:
        return int(dof)
    raise ValueError(f"dof must be a string over 'xyzrpw' or a mask in [1, 63], got {dof!r}")


def check_scan_register(map, iterations=None, dof="xyzrpw", tol_t=None, tol_r=None, n_poses=None):
    """A registration's settings, by name; needs no GPU.  map: an ops.EvidenceMap; iterations (None: not asked): an integer in [1,
    256]; dof: scan_dof_mask's; tol_t (None: 1/256) in voxels and tol_r (None: 1e-4) in radians: finite and >= 0; n_poses (None: not
    asked): an integer in [1, 256].  -> (iterations, mask, tol_t, tol_r); ValueError otherwise."""
    if not isinstance(map, EvidenceMap):
        raise ValueError(f"ScanMatcher: the map must be an ops.EvidenceMap (EvidenceMap.from_space takes a SpaceMap), got {type(map).__name__}")
    if iterations is not None and (not _is_int(iterations) or not 1 <= iterations <= SCAN_REGISTER_MAX_ITERATIONS):
        raise ValueError(f"iterations must be an integer in [1, {SCAN_REGISTER_MAX_ITERATIONS}], got {iterations!r}")
    mask = scan_dof_mask(dof)
    tols = []
    for name, v, default in (("tol_t", tol_t, SCAN_REGISTER_TOL_T), ("tol_r", tol_r, SCAN_REGISTER_TOL_R)):
        f = default if v is None else _float_or_nan(v)
        if not (np.isfinite(f) and f >= 0.0):
            raise ValueError(f"{name} must be None or a finite number >= 0, got {v!r}")
        tols.append(f)
    if n_poses is not None and (not _is_int(n_poses) or not 1 <= n_poses <= SCAN_MAX_ROTATIONS):
        raise ValueError(f"the poses must number 1 .. {SCAN_MAX_ROTATIONS}, got {n_poses!r}")
    return (None if iterations is None else int(iterations)), mask, tols[0], tols[1]


def scan_register_start(poses, quats):
    """The start of a registration on the host: poses (B,3) and quats (B,4) f64 -> (state (B,64) int64, poses12 (B,12) f32): current
    and trial pose = the start (the quaternion as given, not normalised), lambda = 2^-10, the rest 0; poses12: R of the quaternion with
    s = 2 / (q . q), in the step kernel's operation order, and t, each rounded once to f32 (synth.scan_register_init_ref)."""
    t, q = np.asarray(poses, dtype=np.float64).reshape(-1, 3), np.asarray(quats, dtype=np.float64).reshape(-1, 4)
    F = SCAN_REGISTER_FIELDS
    st = np.zeros((len(t), SCAN_REGISTER_STATE), dtype=np.float64)
    st[:, F["t"]:F["t"] + 3] = st[:, F["trial_t"]:F["trial_t"] + 3] = t
    st[:, F["q"]:F["q"] + 4] = st[:, F["trial_q"]:F["trial_q"] + 4] = q
    st[:, F["lam"]] = SCAN_REGISTER_LAMBDA0
    w, x, y, z = q.T
    s = 2.0 / (((w * w + x * x) + y * y) + z * z)
    R = np.stack([1.0 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y),
                  s * (x * y + w * z), 1.0 - s * (x * x + z * z), s * (y * z - w * x),
                  s * (x * z - w * y), s * (y * z + w * x), 1.0 - s * (x * x + y * y)], axis=1)
    return st.view(np.int64), np.ascontiguousarray(np.concatenate([R, t], axis=1).astype(np.float32))


# ---- pose-graph optimisation: Levenberg-Marquardt over scan poses (posegraph_kernels.hip, DESIGN.md 10 "Pose graph")

POSE_GRAPH_EDGE = _lib.CONSTANTS["TOHIP_POSEGRAPH_EDGE"]          # f64 words of an edge's record
POSE_GRAPH_SCALARS = _lib.CONSTANTS["TOHIP_POSEGRAPH_SCALARS"]    # words of the optimiser's scalars
POSE_GRAPH_MAX_ITERATIONS = _lib.CONSTANTS["TOHIP_POSEGRAPH_MAX_ITERATIONS"]
POSE_GRAPH_MAX_CG = _lib.CONSTANTS["TOHIP_POSEGRAPH_MAX_CG"]
POSE_GRAPH_MAX_NODES = POSE_GRAPH_MAX_EDGES = 1 << 22
POSE_GRAPH_STATUS = ("RUNNING", "CONVERGED", "STALLED", "DEGENERATE", "NONFINITE")
# the workspace's regions in tohip_posegraph_layout's order, and the scalars' words
POSE_GRAPH_REGIONS = ("scalars", "poses", "x", "edges", "nodes", "ldl", "r", "z", "p", "ap", "cost_partials", "rz_partials", "pap_partials",
                      "small_flags", "pivot_flags", "trial_cost", "total")
POSE_GRAPH_FIELDS = dict(lam=0, cost=1, initial_cost=2, status=3, iterations=4, accepted=5, cg_iterations=6, current=7, rz=8, rz0=9, cg_stop=10,
                         have=11)
# an edge record's words: e (6), s, w, rho, 0, Ja^T W Ja (21), Jb^T W Jb (21), Ja^T W Jb (36), Ja^T W e (6), Jb^T W e (6)
POSE_GRAPH_RECORD = dict(e=0, s=6, w=7, rho=8, haa=10, hbb=31, hab=52, ga=88, gb=94)
assert len(POSE_GRAPH_REGIONS) == _lib.CONSTANTS["TOHIP_POSEGRAPH_REGIONS"]
_TRIU6 = tuple((i, j) for i in range(6) for j in range(i, 6))


def pose_graph_layout(n_nodes, n_edges):
    """{region: its offset in the workspace, in 8-byte words}, 'total' the workspace's size: tohip_posegraph_layout's answer."""
    off = (ctypes.c_int64 * len(POSE_GRAPH_REGIONS))()
    check(_lib.lib().tohip_posegraph_layout(int(n_nodes), int(n_edges), off, 0), "tohip_posegraph_layout")
    return dict(zip(POSE_GRAPH_REGIONS, (int(v) for v in off)))


def pose_graph_incidence(ab, n_nodes):
    """Edges (E,2), a = -1 an absolute edge -> (row_ptr (n+1,) int32, incident int32): node i's entries incident[row_ptr[i]:row_ptr[i+1]]
    are 2 edge + side (0: the node is the edge's a, 1: its b) in ascending edge index — the order of every sum over a node's edges."""
    node = np.asarray(ab, dtype=np.int64).reshape(-1)
    code = np.arange(len(node), dtype=np.int64)
    keep = node >= 0
    node, code = node[keep], code[keep]
    order = np.argsort(node, kind="stable")
    row_ptr = np.zeros(int(n_nodes) + 1, dtype=np.int64)
    np.add.at(row_ptr, node + 1, 1)
    return np.cumsum(row_ptr).astype(np.int32), code[order].astype(np.int32)


def pose_graph_information(information, n_edges, name="information"):
    """(E,6,6) symmetric matrices, or (E,21) upper triangles row-major (one of either for E edges alike) -> (E,21) f64.  The order is
    (x, y, z, roll, pitch, yaw), metres and radians.  A non-finite entry, an asymmetric matrix or a negative diagonal entry is
    refused, by edge."""
    try:
        a = np.asarray(information.detach().cpu().numpy() if torch.is_tensor(information) else information, dtype=np.float64)
    except (TypeError, ValueError):
        a = np.zeros(0)
    if a.shape in ((6, 6), (21,)):
        a = np.broadcast_to(a, (n_edges,) + a.shape)
    if a.shape == (n_edges, 6, 6):
        if not np.array_equal(a, a.transpose(0, 2, 1)):
            k = int(np.flatnonzero((a != a.transpose(0, 2, 1)).any(axis=(1, 2)))[0])
            raise ValueError(f"{name}: the matrix of edge {k} is not symmetric")
        a = np.stack([a[:, i, j] for i, j in _TRIU6], axis=1)
    if a.shape != (n_edges, 21):
        raise ValueError(f"{name} must be ({n_edges},6,6), ({n_edges},21), or one (6,6) or (21,) for all, got {a.shape}")
    diag = a[:, [n for n, (i, j) in enumerate(_TRIU6) if i == j]]
    bad = ~np.isfinite(a).all(axis=1) | (diag < 0.0).any(axis=1)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{name}: edge {k} has a non-finite entry or a negative diagonal entry: {a[k].tolist()}")
    return np.ascontiguousarray(a)


def check_pose_graph(n_nodes, ab, fixed=()):
    """A graph's structure, by name; needs no GPU.  n_nodes in [1, 2^22]; ab (E,2) integers with 1 <= E <= 2^22, b in [0, n), a in [0, n)
    or -1 (an absolute edge), a != b; fixed: node indices in [0, n).  Every connected component must hold a fixed node or an
    absolute edge (union-find on the host), otherwise the optimum is not unique and ValueError names a node of the floating
    component.  -> (ab (E,2) int32, fixed as a sorted int64 array)."""
    if not _is_int(n_nodes) or not 1 <= n_nodes <= POSE_GRAPH_MAX_NODES:
        raise ValueError(f"the nodes must number 1 .. 2^22, got {n_nodes!r}")
    n = int(n_nodes)
    e = np.asarray(ab)
    if e.ndim != 2 or e.shape[1] != 2 or e.dtype.kind not in "iu" or not 1 <= e.shape[0] <= POSE_GRAPH_MAX_EDGES:
        raise ValueError(f"the edges must be an (E,2) integer array with 1 <= E <= 2^22, got {e.shape} {e.dtype}")
    e = e.astype(np.int64)
    bad = (e[:, 1] < 0) | (e[:, 1] >= n) | (e[:, 0] < -1) | (e[:, 0] >= n)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"edge {k} = ({e[k, 0]}, {e[k, 1]}): an index out of range for {n} nodes (a = -1 alone marks an absolute edge)")
    if (e[:, 0] == e[:, 1]).any():
        k = int(np.flatnonzero(e[:, 0] == e[:, 1])[0])
        raise ValueError(f"edge {k} = ({e[k, 0]}, {e[k, 1]}): a and b must differ")
    f = np.unique(np.asarray(list(fixed) if not isinstance(fixed, np.ndarray) else fixed, dtype=np.int64).reshape(-1))
    if len(f) and (f[0] < 0 or f[-1] >= n):
        raise ValueError(f"fixed: node {int(f[0] if f[0] < 0 else f[-1])} out of range for {n} nodes")
    rel = e[e[:, 0] >= 0]
    try:                                       # the components: scipy's where it is installed, union-find otherwise; `root` labels them
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        root = connected_components(coo_matrix((np.ones(len(rel), dtype=np.int8), (rel[:, 0], rel[:, 1])), shape=(n, n)), directed=False)[1]
        root = root.astype(np.int64)
    except ImportError:
        parent = np.arange(n, dtype=np.int64)

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i
        for a, b in rel:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        root = np.asarray([find(i) for i in range(n)], dtype=np.int64)
    anchored = np.zeros(n, dtype=bool)
    anchored[root[f]] = True
    anchored[root[e[e[:, 0] < 0, 1]]] = True
    loose = ~anchored[root]
    if loose.any():
        i = int(np.flatnonzero(loose)[0])
        raise ValueError(f"node {i} belongs to a floating component ({int((root == root[i]).sum())} nodes): it holds no fixed node and no "
                         "absolute edge, so its poses are not determined")
    return e.astype(np.int32), f


def check_pose_graph_buffers(outputs, inputs):
    """No output may share a byte with an input or with another output, by address ranges: {name: tensor} each; ValueError names
    the pair that overlaps."""
    seen = [(name, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for name, t in inputs.items()]
    for name, t in outputs.items():
        lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        for other, a, b in seen:
            if lo < b and a < hi:
                raise ValueError(f"the output `{name}` aliases `{other}`: an output may share no byte with an input or with another output")
        seen.append((name, lo, hi))


def check_pose_graph_options(iterations=None, cg_iterations=None, cg_tol=1e-8, robust=None, tol_t=1e-5, tol_r=1e-6, n_nodes=1):
    """An optimisation's settings, by name; needs no GPU -> (iterations, cg_iterations, cg_tol, robust_c, tol_t, tol_r): iterations
    (None: not asked) in [1, 256]; cg_iterations None (min(6 n, 1000)) or in [1, 4096]; robust None (-> 0.0, the plain cost) or a finite
    c > 0; cg_tol, tol_t, tol_r finite and >= 0."""
    if iterations is not None and (not _is_int(iterations) or not 1 <= iterations <= POSE_GRAPH_MAX_ITERATIONS):
        raise ValueError(f"iterations must be an integer in [1, {POSE_GRAPH_MAX_ITERATIONS}], got {iterations!r}")
    if cg_iterations is None:
        cg_iterations = min(6 * int(n_nodes), 1000)
    if not _is_int(cg_iterations) or not 1 <= cg_iterations <= POSE_GRAPH_MAX_CG:
        raise ValueError(f"cg_iterations must be None or an integer in [1, {POSE_GRAPH_MAX_CG}], got {cg_iterations!r}")
    out = []
    for name, v in (("cg_tol", cg_tol), ("tol_t", tol_t), ("tol_r", tol_r)):
        f = _float_or_nan(v)
        if not (np.isfinite(f) and f >= 0.0):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
        out.append(f)
    c = 0.0 if robust is None else _float_or_nan(robust)
    if robust is not None and not (np.isfinite(c) and c > 0.0):
        raise ValueError(f"robust must be None or a finite number > 0, got {robust!r}")
    return (None if iterations is None else int(iterations)), int(cg_iterations), out[0], c, out[1], out[2]


class PoseGraphProblem:
    """One graph ON THE DEVICE and its workspace: the stages of the optimiser, each enqueued on the current stream with nothing read
    back.  nodes (N,7) f64 (t, q wxyz), ab (E,2) int32, meas (E,7) f64, omega (E,21) f64, row_ptr (N+1,), incident and free_mask (N,)
    int32: contiguous tensors of one device, as PoseGraph.upload makes them.  They are read, never written."""
    NAMES = ("nodes", "ab", "meas", "omega", "row_ptr", "incident", "free_mask")

    def __init__(self, nodes, ab, meas, omega, row_ptr, incident, free_mask):
        t = dict(zip(self.NAMES, (nodes, ab, meas, omega, row_ptr, incident, free_mask)))
        n, e = (nodes.shape[0], ab.shape[0]) if torch.is_tensor(nodes) and torch.is_tensor(ab) and nodes.dim() == 2 and ab.dim() == 2 else (0, 0)
        if not (1 <= n <= POSE_GRAPH_MAX_NODES and 1 <= e <= POSE_GRAPH_MAX_EDGES):
            raise ValueError(f"PoseGraphProblem: 1 .. 2^22 nodes and edges, got {n} and {e}")
        want = dict(nodes=((n, 7), torch.float64), ab=((e, 2), torch.int32), meas=((e, 7), torch.float64), omega=((e, 21), torch.float64),
                    row_ptr=((n + 1,), torch.int32), free_mask=((n,), torch.int32))
        for name, v in t.items():
            ok = torch.is_tensor(v) and v.is_contiguous() and v.device == nodes.device
            if name == "incident":
                ok = ok and v.dtype == torch.int32 and v.dim() == 1 and e <= v.shape[0] <= 2 * e
            else:
                ok = ok and tuple(v.shape) == want[name][0] and v.dtype == want[name][1]
            if not ok:
                raise ValueError(f"PoseGraphProblem: {name} must be a contiguous {want.get(name, (('E .. 2E',), torch.int32))} tensor on {nodes.device}, got "
                                 f"{(tuple(v.shape), v.dtype, str(v.device)) if torch.is_tensor(v) else type(v).__name__}")
        self.tensors, self.n, self.e, self.device = t, n, e, nodes.device
        self.off = pose_graph_layout(n, e)
        assert self.off["total"] * 8 == _lib.lib().tohip_posegraph_workspace_bytes(n, e, 0)
        self.work = torch.empty(self.off["total"], dtype=torch.float64, device=self.device)
        check_pose_graph_buffers({"workspace": self.work}, t)

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            check(getattr(_lib.lib(), name)(*args, stream_ptr(), 0), name)

    def _graph(self):
        t = self.tensors
        return (ptr(t["ab"]), ptr(t["meas"]), ptr(t["omega"]), ptr(t["row_ptr"]), ptr(t["incident"]), ptr(t["free_mask"]), self.n, self.e,
                t["incident"].shape[0])

    def _work(self):
        return ptr(self.work), self.work.numel() * 8

    def start(self):
        """The current poses = nodes, the pending step 0, lambda = 2^-10 -> self.  One launch."""
        self._call("tohip_posegraph_start", ptr(self.tensors["nodes"]), self.n, self.e, *self._work())
        return self

    def linearize(self, robust_c=0.0):
        """The edge records at the trial poses, into the edge buffer that is not current -> self.  One launch."""
        self._call("tohip_posegraph_linearize", *self._graph(), float(robust_c), *self._work())
        return self

    def gather(self):
        """Each node's diagonal block and gradient from the trial records, and the trial cost -> self.  One launch."""
        self._call("tohip_posegraph_gather", *self._graph(), *self._work())
        return self

    def step(self, cg_iterations, cg_tol=1e-8, tol_t=1e-5, tol_r=1e-6):
        """Accept or reject the trial, adapt lambda, and solve the next damped step -> self.  1 + 2 cg_iterations launches."""
        self._call("tohip_posegraph_step", *self._graph(), int(cg_iterations), float(cg_tol), float(tol_t), float(tol_r), *self._work())
        return self

    def optimize(self, iterations, cg_iterations, cg_tol=1e-8, robust_c=0.0, tol_t=1e-5, tol_r=1e-6):
        """`iterations` rounds of linearize, gather and step, enqueued in one call -> self."""
        self._call("tohip_posegraph_optimize", *self._graph(), int(iterations), int(cg_iterations), float(cg_tol), float(robust_c), float(tol_t),
                   float(tol_r), *self._work())
        return self

    def result(self, out=None):
        """-> (16 + 7 N + 2 E,) f64 on the device: the scalars (POSE_GRAPH_FIELDS), the current poses, chi^2 and the weight of every
        edge at them.  out: a tensor to fill; it may be no input and not the workspace."""
        if out is None:
            out = torch.empty(POSE_GRAPH_SCALARS + 7 * self.n + 2 * self.e, dtype=torch.float64, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != torch.float64 or out.numel() != POSE_GRAPH_SCALARS + 7 * self.n + 2 * self.e
              or out.device != self.device or not out.is_contiguous()):
            raise ValueError(f"PoseGraphProblem.result: out must be a contiguous ({POSE_GRAPH_SCALARS + 7 * self.n + 2 * self.e},) float64 tensor on "
                             f"{self.device}")
        check_pose_graph_buffers({"out": out}, dict(self.tensors, workspace=self.work))
        self._call("tohip_posegraph_result", self.n, self.e, *self._work(), ptr(out))
        return out

    def region(self, name):
        """A view of one region of the workspace (f64 words; the flags and the integers among the scalars are int64 by their bits)."""
        i = POSE_GRAPH_REGIONS.index(name)
        return self.work[self.off[name]:self.off[POSE_GRAPH_REGIONS[i + 1]]]


class PoseGraphResult:
    """What PoseGraph.optimize returns, numpy on the host: poses (N,3) and quats (N,4) wxyz, normalised once on the host; cost and
    initial_cost, sum rho(s) at the result and at the start; iterations run, steps accepted and cg_iterations in total; status, a name
    of POSE_GRAPH_STATUS (RUNNING: the iterations ran out); lam, the last lambda; chi2 (E,), s_k = e^T Omega e of every edge at the
    result, and weights (E,), its IRLS weight (1 without robust=): a wrong closure shows as a large chi2 and a small weight."""
    __slots__ = ("poses", "quats", "cost", "initial_cost", "iterations", "accepted", "cg_iterations", "status", "lam", "chi2", "weights")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def pose_graph_result(out, n_nodes, n_edges):
    """The packed result ON THE HOST ((16 + 7 N + 2 E,) f64, PoseGraphProblem.result read back) -> PoseGraphResult."""
    out = np.ascontiguousarray(np.asarray(out, dtype=np.float64).reshape(-1))
    S, I, F = out[:POSE_GRAPH_SCALARS], out[:POSE_GRAPH_SCALARS].view(np.int64), POSE_GRAPH_FIELDS
    nodes = out[POSE_GRAPH_SCALARS:POSE_GRAPH_SCALARS + 7 * n_nodes].reshape(n_nodes, 7)
    rest = out[POSE_GRAPH_SCALARS + 7 * n_nodes:]
    q = nodes[:, 3:7]
    return PoseGraphResult(poses=nodes[:, :3].copy(), quats=q / np.sqrt((q * q).sum(axis=1, keepdims=True)), cost=float(S[F["cost"]]),
                           initial_cost=float(S[F["initial_cost"]]), iterations=int(I[F["iterations"]]), accepted=int(I[F["accepted"]]),
                           cg_iterations=int(I[F["cg_iterations"]]), status=POSE_GRAPH_STATUS[int(I[F["status"]])], lam=float(S[F["lam"]]),
                           chi2=rest[:n_edges].copy(), weights=rest[n_edges:2 * n_edges].copy())


def _quat_product(p, q):
    """The Hamilton product of (…,4) wxyz arrays."""
    pw, px, py, pz = np.moveaxis(np.asarray(p, dtype=np.float64), -1, 0)
    qw, qx, qy, qz = np.moveaxis(np.asarray(q, dtype=np.float64), -1, 0)
    return np.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], axis=-1)


class PoseGraph:
    """A pose graph built on the host and optimised on the device ("Pose graph").  poses (N,3) metres and quats (N,4)
    wxyz (any length but 0, either sign), the nodes; fixed: the indices of nodes that do not move.  Edges are appended with
    add_edges, add_absolute and add_registration; their ORDER is part of the definition of every sum, so the same edges in the same
    order give the same bits, however many calls appended them.  Building needs no GPU; linearize, gradient, cg, residuals and
    optimize upload the graph (one copy) and run on `device`."""

    def __init__(self, poses, quats, fixed=(), device="cuda"):
        self.t = _host_rows(poses, 3, "poses")
        self.q = _host_rows(quats, 4, "quats", rows=self.t.shape[0])
        if not ((self.q * self.q).sum(axis=1) > 0.0).all():
            raise ValueError("quats: a quaternion of length 0")
        if not 1 <= len(self.t) <= POSE_GRAPH_MAX_NODES:
            raise ValueError(f"the nodes must number 1 .. 2^22, got {len(self.t)}")
        self.fixed = np.unique(np.asarray(list(fixed), dtype=np.int64).reshape(-1))
        if len(self.fixed) and (self.fixed[0] < 0 or self.fixed[-1] >= len(self.t)):
            raise ValueError(f"fixed: node {int(self.fixed[0] if self.fixed[0] < 0 else self.fixed[-1])} out of range for {len(self.t)} nodes")
        self.device = torch.device(device)
        self.ab = np.zeros((0, 2), dtype=np.int32)
        self.meas = np.zeros((0, 7), dtype=np.float64)
        self.omega = np.zeros((0, 21), dtype=np.float64)

    n_nodes = property(lambda self: len(self.t))
    n_edges = property(lambda self: len(self.ab))

    def add_edges(self, a, b, t, q, information):
        """Append E relative edges: a, b (E,) node indices (a = -1: an absolute edge), the measured d_t = R_a^T (t_b - t_a) (E,3) and d_q
        = conj(q_a) (x) q_b (E,4) wxyz (any length but 0), and the information matrices (pose_graph_information) -> self."""
        a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
        if a.ndim != 1 or a.shape != b.shape or a.dtype.kind not in "iu" or b.dtype.kind not in "iu" or len(a) == 0:
            raise ValueError(f"a and b must be integer arrays of one length >= 1, got {a.shape} {a.dtype} and {b.shape} {b.dtype}")
        n, e0 = self.n_nodes, self.n_edges
        for bad, why in (((a < -1) | (a >= n) | (b < 0) | (b >= n), f"an index out of range for {n} nodes (a = -1 alone marks an absolute edge)"),
                         (a == b, "a and b must differ")):
            if bad.any():
                k = int(np.flatnonzero(bad)[0])
                raise ValueError(f"edge {e0 + k} = ({int(a[k])}, {int(b[k])}): {why}")
        zt, zq = _host_rows(t, 3, "t", rows=len(a)), _host_rows(q, 4, "q", rows=len(a))
        if not ((zq * zq).sum(axis=1) > 0.0).all():
            raise ValueError("q: a quaternion of length 0")
        om = pose_graph_information(information, len(a))
        if e0 + len(a) > POSE_GRAPH_MAX_EDGES:
            raise ValueError(f"the edges must number at most 2^22, got {e0 + len(a)}")
        self.ab = np.concatenate([self.ab, np.stack([a, b], axis=1).astype(np.int32)])
        self.meas = np.concatenate([self.meas, np.concatenate([zt, zq], axis=1)])
        self.omega = np.concatenate([self.omega, om])
        return self

    def add_absolute(self, b, t, q, information):
        """Append absolute edges: node b measured in the world at (t, q): e_t = t_b - t, e_r the Gibbs vector of q_b (x) conj(q) -> self."""
        b = np.atleast_1d(np.asarray(b))
        return self.add_edges(np.full(b.shape, -1, dtype=np.int64), b, t, q, information)

    def add_registration(self, b, reg):
        """Append register_scan's answer for node b as an absolute edge: the measurement reg.pose and reg.quat, the information
        reg.information / sigma^2 with sigma^2 = reg.cost / (reg.used - n_dof), n_dof the degrees of freedom the registration moved
        (the non-zero diagonal entries of reg.information) — the inverse of reg.covariance on them, with no change of frame: the edge's
        parameterisation is the registration's.  A DEGENERATE or EMPTY registration, and one with no residual degrees of freedom or
        no cost, is refused."""
        if reg.status in ("DEGENERATE", "EMPTY"):
            raise ValueError(f"add_registration: the registration of node {b} is {reg.status}: it measured nothing")
        A = np.asarray(reg.information, dtype=np.float64)
        n_dof = int((np.diag(A) != 0.0).sum())
        if not (reg.used > n_dof and reg.cost > 0.0 and np.isfinite(reg.cost)):
            raise ValueError(f"add_registration: node {b}: sigma^2 = cost / (used - n_dof) needs used > n_dof and a cost > 0, got used = {reg.used}, "
                             f"n_dof = {n_dof}, cost = {reg.cost}")
        sigma2 = float(reg.cost) / (int(reg.used) - n_dof)
        return self.add_absolute([int(b)], reg.pose, reg.quat, A / sigma2)

    def relative(self, a, b):
        """The relative pose of node b seen from node a at the CURRENT nodes, in an edge's convention -> (d_t (3,), d_q (4,) wxyz,
        normalised): what add_edges takes as a measurement, so that consecutive registered poses become odometry edges."""
        qa = self.q[a] / np.sqrt((self.q[a] * self.q[a]).sum())
        w, x, y, z = qa
        R = np.asarray([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                        [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                        [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])
        dq = _quat_product(qa * np.asarray([1.0, -1.0, -1.0, -1.0]), self.q[b])
        return R.T @ (self.t[b] - self.t[a]), dq / np.sqrt((dq * dq).sum())

    def check(self):
        """check_pose_graph on this graph -> self."""
        check_pose_graph(self.n_nodes, self.ab, self.fixed)
        return self

    def free_mask(self, dof="xyzrpw"):
        m = np.full(self.n_nodes, scan_dof_mask(dof), dtype=np.int32)
        m[self.fixed] = 0
        return m

    def arrays(self, dof="xyzrpw"):
        """The seven host arrays a PoseGraphProblem takes, by PoseGraphProblem.NAMES."""
        self.check()
        row_ptr, incident = pose_graph_incidence(self.ab, self.n_nodes)
        return dict(nodes=np.ascontiguousarray(np.concatenate([self.t, self.q], axis=1)), ab=self.ab, meas=self.meas, omega=self.omega, row_ptr=row_ptr,
                    incident=incident, free_mask=self.free_mask(dof))

    def upload(self, dof="xyzrpw"):
        """-> PoseGraphProblem: the arrays packed into one host buffer, ONE copy to the device, and views of it."""
        arrays = self.arrays(dof)
        at, spans = 0, {}
        for name, a in arrays.items():
            spans[name] = (at, a.nbytes)
            at += -(-a.nbytes // 8) * 8
        host = np.zeros(at, dtype=np.uint8)
        for name, a in arrays.items():
            host[spans[name][0]:spans[name][0] + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        dev = torch.from_numpy(host).to(self.device)
        views = {name: dev[spans[name][0]:spans[name][0] + a.nbytes].view(torch.float64 if a.dtype == np.float64 else torch.int32).view(a.shape)
                 for name, a in arrays.items()}
        return PoseGraphProblem(**views)

    # ---- the stages, one at a time: each starts from the graph's own nodes and reads its answer back

    def linearize(self, dof="xyzrpw", robust=None):
        """The edge records (E,100) f64 at the nodes (POSE_GRAPH_RECORD names the words), numpy."""
        c = check_pose_graph_options(robust=robust)[3]
        p = self.upload(dof).start().linearize(c)
        return p.region("edges").view(2, self.n_edges, POSE_GRAPH_EDGE)[1].cpu().numpy()   # (nothing is current yet: the trial buffer is 1)

    def residuals(self):
        """-> (e (E,6), chi2 (E,)) at the nodes: each edge's residual and e^T Omega e."""
        rec = self.linearize()
        return rec[:, :6].copy(), rec[:, POSE_GRAPH_RECORD["s"]].copy()

    def gradient(self, dof="xyzrpw", robust=None):
        """-> (D (N,21), the upper triangle of each node's diagonal block of H; g (N,6); the cost), numpy, at the nodes."""
        c = check_pose_graph_options(robust=robust)[3]
        p = self.upload(dof).start().linearize(c).gather()
        node = p.region("nodes").view(2, self.n_nodes, 27)[1].cpu().numpy()
        return node[:, :21].copy(), node[:, 21:].copy(), float(p.region("trial_cost").cpu().numpy()[0])

    def cg(self, cg_iterations=None, cg_tol=1e-8, dof="xyzrpw", robust=None, tol_t=1e-5, tol_r=1e-6):
        """The first damped solve (lambda = 2^-10) at the nodes -> dict(x (N,6), iterations, status, small): one linearize, gather and
        step."""
        _, cg_iterations, cg_tol, c, tol_t, tol_r = check_pose_graph_options(None, cg_iterations, cg_tol, robust, tol_t, tol_r, self.n_nodes)
        p = self.upload(dof).start().linearize(c).gather().step(cg_iterations, cg_tol, tol_t, tol_r)
        S = p.region("scalars").cpu().numpy()[POSE_GRAPH_SCALARS:2 * POSE_GRAPH_SCALARS].view(np.int64)
        return dict(x=p.region("x").view(self.n_nodes, 6).cpu().numpy(), iterations=int(S[POSE_GRAPH_FIELDS["cg_iterations"]]),
                    status=POSE_GRAPH_STATUS[int(S[POSE_GRAPH_FIELDS["status"]])],
                    small=bool((p.region("small_flags").cpu().numpy().view(np.int64) != 0).all()))

    def optimize(self, iterations=30, cg_iterations=None, cg_tol=1e-8, dof="xyzrpw", robust=None, tol_t=1e-5, tol_r=1e-6):
        """Levenberg-Marquardt from the nodes -> PoseGraphResult.  iterations: 1 .. 256 outer iterations, each one linearisation, one
        gather and one damped solve by block-Jacobi conjugate gradients of at most cg_iterations (None: min(6 N, 1000), a default,
        not a measurement) steps, stopped at r.z <= cg_tol^2 (r.z)_0.  dof: the degrees of freedom that move, register_scan's
        ('xyw' for a planar robot).  robust: None, or Geman-McClure's c (in units of sqrt(chi^2)): an edge with s >> c^2 loses its
        say.  CONVERGED: an accepted step within tol_t metres and tol_r radians on every node.  One upload, launches only, one
        read-back.  The graph's own nodes are not modified."""
        iterations, cg_iterations, cg_tol, c, tol_t, tol_r = check_pose_graph_options(iterations, cg_iterations, cg_tol, robust, tol_t, tol_r,
                                                                                     self.n_nodes)
        p = self.upload(dof).start().optimize(iterations, cg_iterations, cg_tol, c, tol_t, tol_r)
        return pose_graph_result(p.result().cpu().numpy(), self.n_nodes, self.n_edges)


SCAN_SEARCH_MAX_WINDOW = (2048, 2048, 4)
SCAN_SEARCH_MAX_LEVELS = 6
SCAN_SEARCH_MAX_CAPACITY = 1 << 24
SCAN_SEARCH_RECORD = 18


def scan_search_levels(window):
    """The default number of levels of a search: the smallest H <= 6 with ceil((2wx+1) / 2^H) ceil((2wy+1) / 2^H) <= 256."""
    wx, wy = int(window[0]), int(window[1])
    for H in range(SCAN_SEARCH_MAX_LEVELS + 1):
        if -(-(2 * wx + 1) // (1 << H)) * -(-(2 * wy + 1) // (1 << H)) <= 256:
            return H
    return SCAN_SEARCH_MAX_LEVELS


def scan_search_window(voxel, dims):
    """The window centred on the prior's voxel, clamped into dims, that reaches every voxel of dims: wx = max(i_x, nx - 1 - i_x), wy
    likewise, wz = 0."""
    i = [min(max(int(v), 0), int(d) - 1) for v, d in zip(voxel, dims)]
    return (max(i[0], int(dims[0]) - 1 - i[0]), max(i[1], int(dims[1]) - 1 - i[1]), 0)


def scan_search_status(status):
    """A record's status word -> None where the search ran to its end, else (level, count): the level that would have held `count`
    nodes, more than the capacity."""
    status = int(status)
    return None if status == 0 else ((status & 7) - 1, status >> 3)


def check_scan_search(map, window=None, levels=None, capacity=None, n_rotations=None):
    """A wide-window search's settings, by name; needs no GPU.  map: an ops.EvidenceMap; window (None: not asked): three integers (wx,
    wy, wz), 0 <= wx, wy <= 2048, 0 <= wz <= 4; levels: None (with a window: scan_search_levels(window)) or an integer in [0, 6];
    capacity (None: not asked): an integer in [1, 2^24], the nodes a level may hold; n_rotations (None: not asked): an integer in
    [1, 256].  -> (window, levels, capacity, n_rotations); ValueError otherwise."""
    if not isinstance(map, EvidenceMap):
        raise ValueError(f"ScanMatcher: the map must be an ops.EvidenceMap (EvidenceMap.from_space takes a SpaceMap), got {type(map).__name__}")
    if window is not None:
        try:
            w = tuple(window)
        except TypeError:
            w = ()
        if len(w) != 3 or not all(_is_int(c) and 0 <= c <= m for c, m in zip(w, SCAN_SEARCH_MAX_WINDOW)):
            raise ValueError(f"window must be three integers (wx, wy, wz) with 0 <= wx, wy <= 2048 and 0 <= wz <= 4, got {window!r}")
        window = tuple(int(c) for c in w)
    if levels is None:
        levels = scan_search_levels(window) if window is not None else None
    elif not _is_int(levels) or not 0 <= levels <= SCAN_SEARCH_MAX_LEVELS:
        raise ValueError(f"levels must be None or an integer in [0, {SCAN_SEARCH_MAX_LEVELS}], got {levels!r}")
    if capacity is not None and (not _is_int(capacity) or not 1 <= capacity <= SCAN_SEARCH_MAX_CAPACITY):
        raise ValueError(f"capacity must be an integer in [1, 2^24] nodes a level, got {capacity!r}")
    if n_rotations is not None and (not _is_int(n_rotations) or not 1 <= n_rotations <= SCAN_MAX_ROTATIONS):
        raise ValueError(f"the rotations must number 1 .. {SCAN_MAX_ROTATIONS}, got K = {n_rotations!r}")
    return window, (None if levels is None else int(levels)), (None if capacity is None else int(capacity)), n_rotations


XFER_MAX_SHIFT = 4096      # of a voxel shift per axis (tohip_occ_transfer / tohip_evid_transfer)
XFER_MODES = {"copy": 0, "or": 1, "add": 1, "confident": 2}
LATTICE_TOLERANCE = 1.0 / 256.0   # the layer's fixed-point unit, in voxels


def _map_frame(m, name):
    """The object that carries a map's origin, resolution, dims and device: the map itself, or a SpaceMap's occupied plane."""
    if isinstance(m, SpaceMap):
        return m.occupied
    if isinstance(m, (OccupancyGrid, EvidenceMap)):
        return m
    raise ValueError(f"{name} must be an ops.OccupancyGrid, SpaceMap or EvidenceMap, got {type(m).__name__}")


def _check_counts(counts, n, device):
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int64 or tuple(counts.shape) != (n,)
                               or counts.device != device or not counts.is_contiguous()):
        raise ValueError(f"counts must be None or a contiguous ({n},) int64 tensor on {device}")


def lattice_offset(a, b):
    """Two maps' frames on one lattice -> the integer voxel offset (kx, ky, kz) of b's origin from a's: b's voxel v is a's voxel v +
    k.  One lattice iff the f32 resolutions are equal and per axis (float64(o_b) - float64(o_a)) / float64(r) lies within 1/256 of
    an integer (the layer's fixed-point unit); ValueError names the axis and both origins otherwise.  Needs no GPU."""
    fa, fb = _map_frame(a, "a"), _map_frame(b, "b")
    ra, rb = np.float32(fa.resolution), np.float32(fb.resolution)
    if ra != rb:
        raise ValueError(f"the maps are not on one lattice: their resolutions differ ({float(ra)!r} and {float(rb)!r})")
    oa, ob = np.asarray(fa.origin, dtype=np.float64), np.asarray(fb.origin, dtype=np.float64)
    d = (ob - oa) / float(ra)
    k = np.rint(d)
    for axis in range(3):
        if not abs(d[axis] - k[axis]) <= LATTICE_TOLERANCE:
            raise ValueError(f"the maps are not on one lattice: along {'xyz'[axis]} the origins {tuple(oa.tolist())} and {tuple(ob.tolist())} "
                             f"lie {d[axis]:.6g} voxels apart, not within 1/256 of an integer")
    return tuple(int(v) for v in k)


def reframed_origin(origin, resolution, shift):
    """The origin of a box moved by `shift` voxels: float32(float64(origin) + shift * float64(f32 resolution)), the way
    occupancy_extent forms origins."""
    o = np.asarray(origin, dtype=np.float32).astype(np.float64)
    return (o + np.asarray(shift, dtype=np.float64) * float(np.float32(resolution))).astype(np.float32)


def position_voxel(frame, position, name="position"):
    """The voxel of a world position in a map's frame by the f32 index rule (g = (p - origin) / r in f32, in range iff -2048 <= g <
    4096, voxel = floor(g * 256) >> 8) -> (i, j, k), which may lie outside dims; ValueError for a position that is not three finite
    numbers or lies beyond the apron."""
    try:
        p = np.asarray(position.detach().cpu() if torch.is_tensor(position) else position, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        p = np.zeros(0, dtype=np.float32)
    if p.shape != (3,) or not np.isfinite(p).all():
        raise ValueError(f"{name} must be three finite numbers, got {position!r}")
    with np.errstate(all="ignore"):
        g = ((p - np.asarray(frame.origin, dtype=np.float32)).astype(np.float32) / np.float32(frame.resolution)).astype(np.float32)
    if not ((g >= np.float32(-2048)) & (g < np.float32(4096))).all():
        raise ValueError(f"{name} {tuple(p.tolist())} lies beyond the map's apron (voxel indices -2048 .. 4095)")
    return tuple(int(v) >> 8 for v in np.floor(g * np.float32(256)).astype(np.int64))


def check_reframe(map, shift=None, dims=None, centre=None):
    """reframed's arguments, by name; needs no GPU.  map: an OccupancyGrid, SpaceMap or EvidenceMap.  Exactly one of shift — three
    integers in [-4096, 4096]: new voxel v is old voxel v + shift — and centre — a world position, three finite numbers within the
    apron, whose voxel becomes voxel dims // 2 of the new box.  dims: the new box's (check_los's rule), default the map's own.
    -> (shift, dims, the new origin as a (3,) float32 array); ValueError otherwise."""
    f = _map_frame(map, "map")
    d = f.dims if dims is None else check_los(f.origin, f.resolution, dims)[2]
    if (shift is None) == (centre is None):
        raise ValueError("give exactly one of shift and centre")
    if centre is not None:
        s = tuple(c - n // 2 for c, n in zip(position_voxel(f, centre, "centre"), d))
    else:
        try:
            s = tuple(shift)
        except TypeError:
            s = ()
        if len(s) != 3 or not all(_is_int(v) for v in s):
            raise ValueError(f"shift must be three integers, got {shift!r}")
        s = tuple(int(v) for v in s)
    if not all(-XFER_MAX_SHIFT <= v <= XFER_MAX_SHIFT for v in s):
        raise ValueError(f"the shift must lie in [-{XFER_MAX_SHIFT}, {XFER_MAX_SHIFT}] voxels per axis, got {s}")
    origin = reframed_origin(f.origin, f.resolution, s)
    if not np.isfinite(origin).all():
        raise ValueError(f"the re-framed origin {tuple(origin.tolist())} is not finite")
    return s, d, origin


def check_merge(a, b, mode=None):
    """merge's arguments, by name; needs no GPU.  a (written) and b (read): two different maps of one kind — OccupancyGrid, SpaceMap or
    EvidenceMap — on one device and one lattice (lattice_offset); mode: None for planes, 'confident' or 'add' for evidence.
    -> (shift, overlap): a's voxel v takes b's voxel v + shift; overlap False where the two boxes share no voxel (nothing to do)."""
    fa = _map_frame(a, "a")
    _map_frame(b, "other")
    if type(a) is not type(b):
        raise ValueError(f"a {type(a).__name__} merges with its own kind, got {type(b).__name__}")
    if a is b:
        raise ValueError("a map cannot be merged into itself")
    fb = _map_frame(b, "other")
    if fa.device != fb.device:
        raise ValueError(f"the maps must live on one device, got {fa.device} and {fb.device}")
    if isinstance(a, EvidenceMap):
        if mode not in ("confident", "add"):
            raise ValueError(f"mode must be 'confident' or 'add', got {mode!r}")
    elif mode is not None:
        raise ValueError(f"mode applies to evidence maps only, got {mode!r} for a {type(a).__name__}")
    k = lattice_offset(a, b)
    s = tuple(-v for v in k)   # a's voxel v is b's voxel v - k
    overlap = all(-na < v < nb for v, na, nb in zip(s, fa.dims, fb.dims))   # some v in [0, na) with v + s in [0, nb)
    return s, overlap


MERGE_MAX_DIM = 2048        # of a merged or transformed map's box per axis
MERGE_MAX_VOXELS = 1 << 31
RESAMPLE_FRAC_BITS = 20     # fraction bits of the integer affine map (tohip_occ_resample / tohip_evid_resample)
RESAMPLE_MAX_OFFSET = 1 << 20   # voxels of the source between the two origins
RESAMPLE_MIN_RATIO = 0.125  # of r_dst / r_src
RESAMPLE_RULES = {"nearest": 0, "cover": 1}
RESAMPLE_OCC_RULES = {"nearest": 0, "any": 1, "all": 2}


class MapFrame(collections.namedtuple("MapFrame", "origin resolution dims")):
    """A box of voxels without a buffer — origin (3,), resolution, dims — where only the geometry of a map is needed (resample_affine,
    transformed_box); every map class carries the same three attributes."""
    __slots__ = ()


def _frame_of(m, name):
    f = m.occupied if isinstance(m, SpaceMap) else m
    if not all(hasattr(f, k) for k in ("origin", "resolution", "dims")):
        raise ValueError(f"{name} must be a map or carry origin, resolution and dims, got {type(m).__name__}")
    return f


def quat_matrix(quat, name="quat"):
    """One quaternion wxyz on the host -> the (3,3) float64 matrix of p -> q p conj(q), q normalised in f64: scan_rotations' matrix
    before its rounding to f32."""
    q = _host_rows(quat, 4, name, rows=1)[0]
    n = np.sqrt((q * q).sum())
    if not n > 0.0:
        raise ValueError(f"{name}: a quaternion of length 0")
    w, x, y, z = q / n
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def resample_affine(src_frame, dst_frame, pose, quat):
    """The twelve integers the resample entries take ("Resampling maps") -> (12,) int64: M (3 x 3, row major) = rint(A
    2^19), then T = rint(b 2^20), in f64, with world_dst = R(quat) world_src + pose — the pose of the source map's frame in the
    destination's, quaternions wxyz as ScanMatch.world reads them — A = (r_d / r_s) R^T and b = (R^T (o_d - pose) - o_s) / r_s: the
    centre of dst voxel d lies at A (d + 1/2) + b in source voxels.  The frames are maps or MapFrames (f32 origins and resolutions,
    read as float64).  ValueError where |b| exceeds 2^20 voxels, where r_d > r_s (1 + 1e-6) — coarsening is a reduction, not a
    resampling — or r_d < r_s / 8.  Needs no GPU."""
    fs, fd = _frame_of(src_frame, "src_frame"), _frame_of(dst_frame, "dst_frame")
    rs, rd = float(np.float32(fs.resolution)), float(np.float32(fd.resolution))
    if not (rs > 0.0 and rd > 0.0 and np.isfinite(rs) and np.isfinite(rd)):
        raise ValueError(f"the resolutions must be finite and > 0, got {rs!r} and {rd!r}")
    if rd > rs * (1.0 + 1e-6):
        raise ValueError(f"the destination's resolution {rd:g} is coarser than the source's {rs:g}: coarsening is a reduction, not a resampling "
                         "(coarsened() / tools.coarsen_map reduce by a whole factor)")
    if rd < rs * RESAMPLE_MIN_RATIO * (1.0 - 1e-6):
        raise ValueError(f"the destination's resolution {rd:g} is finer than an eighth of the source's {rs:g}")
    R = quat_matrix(quat)
    t = _host_rows(pose, 3, "pose", rows=1)[0]
    o_s = np.asarray(fs.origin, dtype=np.float32).astype(np.float64)
    o_d = np.asarray(fd.origin, dtype=np.float32).astype(np.float64)
    A = (rd / rs) * R.T
    b = (R.T @ (o_d - t) - o_s) / rs
    if not (np.abs(b) <= RESAMPLE_MAX_OFFSET).all():
        raise ValueError(f"the destination's origin lies {tuple(b.tolist())} source voxels from the source's: beyond 2^20")
    return np.concatenate([np.rint(A * float(1 << (RESAMPLE_FRAC_BITS - 1))).reshape(9), np.rint(b * float(1 << RESAMPLE_FRAC_BITS))]).astype(np.int64)


def transformed_box(frame, pose, quat, resolution=None, anchor=None):
    """The axis-aligned box around the eight corners of a map's box taken by world_dst = R(quat) world_src + pose, at `resolution`
    (default: the map's), on the lattice through `anchor` (default: the world's origin) -> (k, dims): the box starts k voxels (three
    integers) from the anchor — snapped down, a corner within 1/256 voxel above a lattice plane counting as on it — and holds dims
    voxels, at least one per axis.  Host arithmetic in f64; needs no GPU."""
    f = _frame_of(frame, "frame")
    r_s = float(np.float32(f.resolution))
    r = r_s if resolution is None else float(np.float32(resolution))
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"resolution must be a finite number > 0, got {resolution!r}")
    R, t = quat_matrix(quat), _host_rows(pose, 3, "pose", rows=1)[0]
    o = np.asarray(f.origin, dtype=np.float32).astype(np.float64)
    ext = r_s * np.asarray(f.dims, dtype=np.float64)
    corners = np.array([[o[0] + cx * ext[0], o[1] + cy * ext[1], o[2] + cz * ext[2]] for cx in (0, 1) for cy in (0, 1) for cz in (0, 1)])
    w = corners @ R.T + t
    a = np.zeros(3) if anchor is None else np.asarray(anchor, dtype=np.float32).astype(np.float64)
    k = np.floor((w.min(axis=0) - a) / r + LATTICE_TOLERANCE)
    n = np.maximum(np.ceil((w.max(axis=0) - a) / r - k - LATTICE_TOLERANCE), 1.0)
    if not (np.isfinite(k).all() and np.isfinite(n).all() and (np.abs(k) < 2.0 ** 40).all() and (n < 2.0 ** 40).all()):
        raise ValueError("the transformed box is not finite")
    return tuple(int(v) for v in k), tuple(int(v) for v in n)


def check_transform(map, pose, quat, origin=None, resolution=None, dims=None, like=None, rule="nearest"):
    """transformed's arguments, by name; needs no GPU.  map: an OccupancyGrid, SpaceMap or EvidenceMap; pose (3,), quat (4,) wxyz:
    world_dst = R(quat) world_src + pose; rule 'nearest' or 'cover'.  The new box: like= a map (its origin, resolution and dims; then
    none of the other three may be given), or origin / resolution / dims, each defaulting — the resolution to the map's, the origin
    to transformed_box's (a multiple of the resolution), dims to what reaches the far corners of the transformed box from the
    origin.  Refused beyond MERGE_MAX_DIM per axis or MERGE_MAX_VOXELS.  -> (MapFrame of the new box, the (12,) int64 affine map);
    ValueError otherwise."""
    f = _map_frame(map, "map")
    if rule not in RESAMPLE_RULES:
        raise ValueError(f"rule must be 'nearest' or 'cover', got {rule!r}")
    if like is not None:
        if origin is not None or resolution is not None or dims is not None:
            raise ValueError("like= brings origin, resolution and dims: give none of them with it")
        fl = _frame_of(like, "like")
        origin, resolution, dims = fl.origin, fl.resolution, fl.dims
    r = f.resolution if resolution is None else resolution
    k, n = transformed_box(f, pose, quat, r)
    r64 = float(np.float32(r))
    if origin is None:
        origin = (np.asarray(k, dtype=np.float64) * r64).astype(np.float32)
    elif dims is None:
        o64 = np.asarray(origin, dtype=np.float32).astype(np.float64).reshape(-1)
        if o64.shape != (3,) or not np.isfinite(o64).all():
            raise ValueError(f"origin must be three finite numbers, got {origin!r}")
        far = np.ceil((np.asarray(k, dtype=np.float64) + np.asarray(n, dtype=np.float64)) - o64 / r64 - LATTICE_TOLERANCE)
        n = tuple(int(max(v, 1.0)) for v in far)
    if dims is None:
        dims = n
        if max(dims) > MERGE_MAX_DIM or dims[0] * dims[1] * dims[2] > MERGE_MAX_VOXELS:
            raise ValueError(f"the transformed box of {dims} voxels exceeds {MERGE_MAX_DIM} per axis or 2^31 voxels: give origin= and dims=, "
                             "or a coarser map")
    o, r, d, _ = check_los(origin, r, dims)
    frame = MapFrame(o, r, d)
    return frame, resample_affine(f, frame, pose, quat)


def check_merge_posed(a, b, mode=None, pose=None, quat=None, rule="nearest"):
    """A merge of b, whose frame stands at (pose, quat) in a's — world_a = R(quat) world_b + pose — into a; needs no GPU.  The kinds,
    devices and mode as check_merge.  -> (shift, overlap, None) where the pose is the identity (pose 0, quat (w, 0, 0, 0)) and b sits
    on a's lattice: the integer path, check_merge's answer; otherwise (None, True, the (12,) int64 affine map) for the resample
    entries, which refuse an `a` coarser than b."""
    if (pose is None) != (quat is None):
        raise ValueError("pose and quat must be given together")
    if rule not in RESAMPLE_RULES:
        raise ValueError(f"rule must be 'nearest' or 'cover', got {rule!r}")
    if pose is None:
        return (*check_merge(a, b, mode), None)
    t, q = _host_rows(pose, 3, "pose", rows=1)[0], _host_rows(quat, 4, "quat", rows=1)[0]
    if not t.any() and not q[1:].any() and q[0] != 0.0:
        try:
            return (*check_merge(a, b, mode), None)
        except ValueError as e:
            if "not on one lattice" not in str(e):
                raise
    fa, fb = _map_frame(a, "a"), _map_frame(b, "other")
    if type(a) is not type(b):
        raise ValueError(f"a {type(a).__name__} merges with its own kind, got {type(b).__name__}")
    if a is b:
        raise ValueError("a map cannot be merged into itself")
    if fa.device != fb.device:
        raise ValueError(f"the maps must live on one device, got {fa.device} and {fb.device}")
    if isinstance(a, EvidenceMap):
        if mode not in ("confident", "add"):
            raise ValueError(f"mode must be 'confident' or 'add', got {mode!r}")
    elif mode is not None:
        raise ValueError(f"mode applies to evidence maps only, got {mode!r} for a {type(a).__name__}")
    return None, True, resample_affine(fb, fa, t, q)


COARSEN_MAX_FACTOR = 8      # of tohip_occ_coarsen / tohip_evid_coarsen, the same on all axes
COARSEN_MAX_OFFSET = 1 << 20   # source voxels between the two origins
COARSEN_RULES = {"cover": 0, "max": 1}
COARSEN_OCC_RULES = {"any": 0, "all": 1}
COARSEN_ANCHORS = ("origin", "world")


def _coarsen_factor(factor):
    if not _is_int(factor) or not 2 <= factor <= COARSEN_MAX_FACTOR:
        raise ValueError(f"factor must be an integer in [2, {COARSEN_MAX_FACTOR}], got {factor!r}")
    return int(factor)


def _coarsen_rule(map, rule):
    """The rule by name for the map's kind (None: the kind's default): planes 'any' / 'all', three-state and evidence maps 'cover' / 'max'."""
    names = COARSEN_OCC_RULES if isinstance(map, OccupancyGrid) else COARSEN_RULES
    if rule is None:
        return next(iter(names))
    if rule not in names:
        raise ValueError(f"rule must be {' or '.join(repr(n) for n in names)} for a {type(map).__name__}, got {rule!r}")
    return rule


def coarsen_offset(src_frame, dst_frame, factor):
    """A fine and a coarse frame -> the integer offset (ox, oy, oz) the coarsen entries take ("Coarsening maps"): the
    children of dst voxel d are the source voxels factor d + o + e, e in [0, factor)^3, so o is the coarse origin's place in source
    voxels.  The frames are maps or MapFrames (f32 origins and resolutions, read as float64).  ValueError unless factor is an integer
    in [2, 8], r_d = factor r_s within 1e-6 relative, the origins lie a whole number of source voxels apart within 1/256 voxel
    (lattice_offset's rule) and at most 2^20 of them.  Needs no GPU."""
    f = _coarsen_factor(factor)
    fs, fd = _frame_of(src_frame, "src_frame"), _frame_of(dst_frame, "dst_frame")
    rs, rd = float(np.float32(fs.resolution)), float(np.float32(fd.resolution))
    if not (rs > 0.0 and rd > 0.0 and np.isfinite(rs) and np.isfinite(rd)):
        raise ValueError(f"the resolutions must be finite and > 0, got {rs!r} and {rd!r}")
    if not abs(rd - f * rs) <= 1e-6 * f * rs:
        raise ValueError(f"the coarse resolution {rd:g} is not {f} times the fine one {rs:g}")
    o_s = np.asarray(fs.origin, dtype=np.float32).astype(np.float64)
    o_d = np.asarray(fd.origin, dtype=np.float32).astype(np.float64)
    d = (o_d - o_s) / rs
    k = np.rint(d)
    for axis in range(3):
        if not abs(d[axis] - k[axis]) <= LATTICE_TOLERANCE:
            raise ValueError(f"the coarse box is not on the fine lattice: along {'xyz'[axis]} the origins {tuple(o_s.tolist())} and "
                             f"{tuple(o_d.tolist())} lie {d[axis]:.6g} fine voxels apart, not within 1/256 of an integer")
    if not (np.abs(k) <= COARSEN_MAX_OFFSET).all():
        raise ValueError(f"the coarse origin lies {tuple(k.tolist())} fine voxels from the fine one: beyond 2^20")
    return tuple(int(v) for v in k)


def check_coarsen(map, factor=2, rule=None, anchor="origin", origin=None, dims=None, like=None):
    """coarsened's arguments, by name; needs no GPU.  map: an OccupancyGrid, SpaceMap or EvidenceMap; factor: an integer in [2, 8];
    rule: 'any' or 'all' for an OccupancyGrid, 'cover' or 'max' for the other two (None: the first).  The coarse box has resolution
    float32(factor r) and: like= a map or MapFrame (its origin, resolution and dims; none of the other three with it); or origin=
    (three finite numbers a whole number of fine voxels from the map's origin) and / or dims=; by default what `anchor` says —
    'origin': o = 0, the map's origin, dims ceil(n / factor); 'world': the coarse lattice's planes at multiples of factor r, o_a =
    -(round(origin_a / r) mod factor), refused where the map's origin is not within 1/256 voxel of a multiple of r.  dims defaults to
    ceil((n - o) / factor), at least 1.  Refused beyond MERGE_MAX_DIM per axis or MERGE_MAX_VOXELS.  -> (MapFrame of the coarse box,
    the offset (ox, oy, oz), the rule's name); ValueError otherwise."""
    fr = _map_frame(map, "map")
    f = _coarsen_factor(factor)
    rule = _coarsen_rule(map, rule)
    if anchor not in COARSEN_ANCHORS:
        raise ValueError(f"anchor must be 'origin' or 'world', got {anchor!r}")
    rs = float(np.float32(fr.resolution))
    rd = float(np.float32(f * rs))
    if like is not None:
        if origin is not None or dims is not None:
            raise ValueError("like= brings origin and dims: give neither with it")
        fl = _frame_of(like, "like")
        o = coarsen_offset(fr, fl, f)
        frame = MapFrame(*check_los(fl.origin, fl.resolution, fl.dims)[:3])
        return frame, o, rule
    if origin is None:
        if anchor == "origin":
            o = (0, 0, 0)
        else:
            q = np.asarray(fr.origin, dtype=np.float32).astype(np.float64) / rs
            k = np.rint(q)
            if not (np.abs(q - k) <= LATTICE_TOLERANCE).all():
                raise ValueError(f"anchor='world' needs the map's origin {tuple(fr.origin.tolist())} within 1/256 voxel of a multiple of its "
                                 f"resolution {rs:g}: it lies at {tuple(q.tolist())} voxels")
            o = tuple(-(int(v) % f) for v in k)
        origin = reframed_origin(fr.origin, rs, o)
    else:
        try:
            o32 = np.asarray(origin, dtype=np.float32).reshape(-1)
        except (TypeError, ValueError):
            o32 = np.zeros(0, dtype=np.float32)
        if o32.shape != (3,) or not np.isfinite(o32).all():
            raise ValueError(f"origin must be three finite numbers, got {origin!r}")
        o = coarsen_offset(fr, MapFrame(o32, rd, (1, 1, 1)), f)
        origin = o32
    if dims is None:
        dims = tuple(max(-((o_a - n) // f), 1) for n, o_a in zip(fr.dims, o))   # ceil((n - o) / f)
        if max(dims) > MERGE_MAX_DIM or dims[0] * dims[1] * dims[2] > MERGE_MAX_VOXELS:
            raise ValueError(f"the coarse box of {dims} voxels exceeds {MERGE_MAX_DIM} per axis or 2^31 voxels: give dims=")
    og, rg, dg, _ = check_los(origin, rd, dims)
    return MapFrame(og, rg, dg), o, rule


def check_merge_fine(coarse, fine, mode=None, rule=None):
    """merge_fine's arguments, by name; needs no GPU.  coarse (written) and fine (read): two different maps of one kind on one device,
    the coarse one's resolution 2 .. 8 times the fine one's (within 1e-6 relative) and the origins a whole number of fine voxels
    apart (coarsen_offset); mode: None for planes, 'confident' or 'add' for evidence; rule as check_coarsen.
    -> (factor, offset, the rule's name); ValueError otherwise."""
    fc, ff = _map_frame(coarse, "coarse"), _map_frame(fine, "fine")
    if type(coarse) is not type(fine):
        raise ValueError(f"a {type(coarse).__name__} merges with its own kind, got {type(fine).__name__}")
    if coarse is fine:
        raise ValueError("a map cannot be merged into itself")
    if fc.device != ff.device:
        raise ValueError(f"the maps must live on one device, got {fc.device} and {ff.device}")
    if isinstance(coarse, EvidenceMap):
        if mode not in ("confident", "add"):
            raise ValueError(f"mode must be 'confident' or 'add', got {mode!r}")
    elif mode is not None:
        raise ValueError(f"mode applies to evidence maps only, got {mode!r} for a {type(coarse).__name__}")
    rule = _coarsen_rule(coarse, rule)
    ratio = float(np.float32(fc.resolution)) / float(np.float32(ff.resolution))
    f = int(round(ratio)) if np.isfinite(ratio) else 0
    if not 2 <= f <= COARSEN_MAX_FACTOR:
        raise ValueError(f"merge_fine takes a map 2 to {COARSEN_MAX_FACTOR} times finer than this one: the resolutions {fc.resolution:g} and "
                         f"{ff.resolution:g} stand {ratio:g} to 1")
    return f, coarsen_offset(ff, fc, f), rule


def _affine_arg(affine):
    """The (12,) int64 affine map as the resample entries take it: a host array (kept alive by the caller) and frac_bits."""
    a = np.ascontiguousarray(affine, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), RESAMPLE_FRAC_BITS


def check_occlusion_grid(grid, cloud):
    """occlusion_bits(method='voxel')'s grid: an OccupancyGrid on the cloud's device; ValueError otherwise."""
    if not isinstance(grid, OccupancyGrid):
        raise ValueError(f"method='voxel' needs grid= an OccupancyGrid, got {type(grid).__name__}")
    if grid.device != cloud.device:
        raise ValueError(f"the grid lives on {grid.device}, the cloud on {cloud.device}")
    return grid


def los_rows(cloud, poses, quats, cam, min_dist, max_dist, grid, skip=(1, 1), prune=True, rows=None, stats=None):
    """The 'voxel' occlusion bit rows (tohip_los_rows): (W, npad/32) int32, bit i = packed position i, 1 iff cull_waypoints keeps the
    point for waypoint w and the ray from poses[w] to it is not blocked in `grid`.  One launch per 65 535 waypoints, nothing read
    back.  prune=False tests every point (the same bits)."""
    check_occlusion_grid(grid, cloud)
    ss, es = check_los_skip(skip)
    dev, W = cloud.device, poses.shape[0]
    p = poses.detach().to(device=dev, dtype=torch.float32).contiguous()
    q = quats.detach().to(device=dev, dtype=torch.float32).contiguous()
    if rows is None:
        rows = torch.empty((W, cloud.npad // 32), dtype=torch.int32, device=dev)
    for w0 in range(0, W, 65535):
        w1 = min(W, w0 + 65535)
        _map_call(dev, "tohip_los_rows", *grid._sizes(), ptr(cloud.blob), cloud.n, ptr(p[w0:w1]), ptr(q[w0:w1]), w1 - w0, cam.ref(),
                  float(min_dist), float(max_dist), ss, es, int(bool(prune)), ptr(rows[w0:w1]), ptr(stats))
    return rows


def team_loss(poses, poses0, n_members, smoothness_weight, traj_length_weight, eps, scalars, clearance_weight=0.0, clr_terms=None):
    """tohip_team_loss: criterion's terms of every member (poses / poses0: the members' (B W, 3) rows end to end) behind the team's
    `scalars` -> (member_terms (B, 8): [0] vis [1] l2 [2] length [3] smooth [5] clearance; total (1): the team total; reg (B W, 3): the
    regularisers' gradient rows).  clr_terms: the clearance query's per-waypoint terms of all B W waypoints (float64), or None."""
    dev, W = poses.device, poses.shape[0] // n_members
    terms = torch.empty((n_members, 8), dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.float32, device=dev)
    reg = torch.empty((n_members * W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().tohip_team_loss(ptr(poses), ptr(poses0), W, n_members, float(smoothness_weight), float(traj_length_weight), float(eps),
                                         ptr(scalars), float(clearance_weight), ptr(clr_terms), ptr(terms), None, ptr(total), ptr(reg), None,
                                         stream_ptr()), "tohip_team_loss")
    return terms, total, reg


VIEWS_MAX_CHUNK = _lib.CONSTANTS["TOHIP_VIEWS_MAX_CHUNK"]
VIEWS_MAX_CANDIDATES = _lib.CONSTANTS["TOHIP_VIEWS_MAX_CANDIDATES"]
VIEWS_CHUNK_BYTES = 1 << 30    # the dense (chunk, npad) f32 rows a ViewSet compacts at a time: 256 candidates at 1 M points


def check_views(cand_poses, cand_quats, k, min_gain=0.0, chunk=None):
    """The arguments of a view selection: cand_poses (M,3) and cand_quats (M,4) floating tensors with the same M in
    [1, VIEWS_MAX_CANDIDATES], finite; 1 <= k (an int); min_gain a finite number >= 0; chunk None or an int in [1, VIEWS_MAX_CHUNK]
    -> (M, k clipped to M, min_gain); ValueError otherwise."""
    for name, t, w in (("cand_poses", cand_poses, 3), ("cand_quats", cand_quats, 4)):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError(f"{name} must be a floating-point tensor, got {type(t).__name__}"
                             f"{'' if not torch.is_tensor(t) else ' of ' + str(t.dtype)}")
        if t.dim() != 2 or t.shape[1] != w or t.shape[0] == 0:
            raise ValueError(f"{name} must have shape (M,{w}) with M >= 1, got {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{name} must be finite (NaN or inf found)")
    M = cand_poses.shape[0]
    if cand_quats.shape[0] != M:
        raise ValueError(f"cand_poses holds {M} candidates, cand_quats {cand_quats.shape[0]}")
    if M > VIEWS_MAX_CANDIDATES:
        raise ValueError(f"at most {VIEWS_MAX_CANDIDATES} candidate views, got {M}")
    if not _is_int(k) or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    g = _float_or_nan(min_gain)
    if not (np.isfinite(g) and g >= 0.0):
        raise ValueError(f"min_gain must be a finite number >= 0, got {min_gain!r}")
    if chunk is not None and (not _is_int(chunk) or not 1 <= chunk <= VIEWS_MAX_CHUNK):
        raise ValueError(f"chunk must be None or an integer in [1, {VIEWS_MAX_CHUNK}], got {chunk!r}")
    return M, min(int(k), M), g


def views_layout(npad, n_candidates, nnz_capacity):
    """Byte offsets of a view set's sections (include/trajopt_hip.h, tohip_views_bytes): every section aligned to 256 bytes."""
    M, nseg = n_candidates, (npad + 8191) // 8192
    return _sections(256, (("offsets", 8 * (M + 1)), ("absent", 4 * M), ("gain", 8 * M), ("chosen", 4 * M),
                           ("segments", 4 * VIEWS_MAX_CHUNK * nseg), ("idx", 4 * nnz_capacity), ("val", 4 * nnz_capacity)))


class ViewSet:
    """M candidate views over one packed cloud as sparse log-odds rows (tohip_views_append): per candidate the (packed index,
    log-odds) pairs of the row traj_forward gives it as a trajectory of its own with one body waypoint, ascending, zeros and pads
    left out.  Owns the CSR buffers; `append` runs the forward in chunks of `chunk` candidates (default: as many as keep the dense
    chunk, chunk x npad x 4 bytes, within VIEWS_CHUNK_BYTES; at most VIEWS_MAX_CHUNK) and compacts each.  nnz_capacity: entries the
    buffers hold (default 1 % of M x N); a set that outgrows it stores nothing more and says so in `status()`."""

    def __init__(self, cloud, cam, n_candidates, rig=None, flags=0, nnz_capacity=None, chunk=None):
        L = _lib.lib()
        self.cloud, self.cam, self.rig, self.flags = cloud, cam, rig, int(flags)
        self.n_candidates = int(n_candidates)
        self.capacity = int(nnz_capacity) if nnz_capacity is not None else max(4096, self.n_candidates * cloud.n // 100)
        self.chunk = int(chunk) if chunk is not None else max(1, min(VIEWS_MAX_CHUNK, VIEWS_CHUNK_BYTES // (4 * cloud.npad)))
        self.bytes = L.tohip_views_bytes(cloud.n, self.n_candidates, self.capacity)
        if self.bytes == 0 or not 1 <= self.chunk <= VIEWS_MAX_CHUNK:
            raise ValueError(f"a view set of {n_candidates} candidates x {self.capacity} entries in chunks of {self.chunk} is out of range")
        self.layout = views_layout(cloud.npad, self.n_candidates, self.capacity)
        assert self.layout["total"] == self.bytes
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=cloud.device)
        self.buf[:256].zero_()   # the header: an empty set until the first append
        self.appended = 0
        self._ws, self._dense = {}, None

    def _sizes(self):
        return ptr(self.buf), self.bytes, self.cloud.n, self.n_candidates, self.capacity

    def _section(self, name, count, dtype):
        o = self.layout[name]
        return self.buf[o:o + count * torch.empty(0, dtype=dtype).element_size()].view(dtype)

    def append(self, poses, quats, occ=None):
        """The next candidates: poses (n,3), quats (n,4) wxyz on the cloud's device; occ: their occlusion bit rows (n C, npad/32), one
        per virtual waypoint, or None.  Launches only."""
        c, C = self.cloud, self.rig.n_cams if self.rig is not None else 1
        n = poses.shape[0]
        if self.appended + n > self.n_candidates:
            raise ValueError(f"the view set holds {self.n_candidates} candidates: {self.appended} appended, {n} more given")
        if self._dense is None:
            self._dense = torch.empty((self.chunk, c.npad), dtype=torch.float32, device=c.device)
        L = _lib.lib()
        for w0 in range(0, n, self.chunk):
            t = min(self.chunk, n - w0)
            ws = self._ws.get(t)
            if ws is None:   # a workspace per chunk size: its layout depends on the number of trajectories
                ws = self._ws[t] = (TrajWorkspace(c, t * C, t), torch.arange(t + 1, dtype=torch.int32, device=c.device))
            ps, qs = poses[w0:w0 + t].contiguous(), quats[w0:w0 + t].contiguous()
            rows = occ[w0 * C:(w0 + t) * C].contiguous() if occ is not None else None
            lo = self._dense[:t]
            traj_forward(c, ps, qs, self.cam, ws[0], self.rig, flags=self.flags, occ=rows, lo_sum=lo, traj_offsets=ws[1])
            with torch.cuda.device(c.device):
                check(L.tohip_views_append(*self._sizes(), ptr(lo), self.appended, t, None, stream_ptr()), "tohip_views_append")
            self.appended += t

    def header(self):
        """The header's first five words on the device: entries stored, entries needed, status, candidates appended, stopped."""
        return self.buf[:40].view(torch.int64)

    def status(self):
        """-> (entries stored, entries needed by everything appended, fits) — one device-to-host read."""
        h = self.header().cpu()
        if int(h[2]) & 2:
            raise RuntimeError("the view set's chunks were not appended in order")
        return int(h[0]), int(h[1]), int(h[2]) == 0

    @property
    def nnz(self):
        return self.status()[0]

    @property
    def absent(self):
        """(M,) bool on the device: the candidates whose row is NaN (a view that sees nothing at all); never chosen."""
        return self._section("absent", self.n_candidates, torch.int32)[:self.appended] != 0

    @property
    def offsets(self):
        return self._section("offsets", self.n_candidates + 1, torch.int64)[:self.appended + 1]

    def entries(self):
        """-> (idx int32, val f32) views of the stored entries (the first nnz of the capacity), candidate after candidate."""
        nnz = self.nnz
        return self._section("idx", self.capacity, torch.int32)[:nnz], self._section("val", self.capacity, torch.float32)[:nnz]

    def row(self, c):
        """Candidate c's list scattered back to a dense (npad,) f32 row in packed order (zeros where nothing is stored, pads
        included; NaN at every point of an absent candidate)."""
        if not 0 <= int(c) < self.appended:
            raise IndexError(f"candidate {c} of {self.appended}")
        row = torch.empty(self.cloud.npad, dtype=torch.float32, device=self.cloud.device)
        with torch.cuda.device(self.cloud.device):
            check(_lib.lib().tohip_views_row(*self._sizes(), int(c), ptr(row), stream_ptr()), "tohip_views_row")
        return row


def views_select(viewset, k, prior=None, min_gain=0.0):
    """tohip_views_select: k greedy rounds over a complete ViewSet -> (order (k,) int32, gain_fixed (k,) int64, n_selected (1,) int32,
    S (npad,) f32 in packed order), all on the device, nothing synchronised; the first n_selected entries of order / gain_fixed count.
    prior: a LogOddsPrior over the set's cloud or None."""
    if viewset.appended != viewset.n_candidates:
        raise ValueError(f"the view set holds {viewset.appended} of its {viewset.n_candidates} candidates: append the rest first")
    c = viewset.cloud
    k = int(k)
    order = torch.zeros(k, dtype=torch.int32, device=c.device)
    gain = torch.zeros(k, dtype=torch.int64, device=c.device)
    n_sel = torch.empty(1, dtype=torch.int32, device=c.device)
    S = torch.empty(c.npad, dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        check(_lib.lib().tohip_views_select(*viewset._sizes(), ptr(prior.buf) if prior is not None else None, k, float(min_gain), ptr(S),
                                            ptr(order), ptr(gain), ptr(n_sel), stream_ptr()), "tohip_views_select")
    return order, gain, n_sel, S


def team_member_gains(cloud, lo_members, prior=None):
    """tohip_team_member_gains over the (B, npad) per-member log-odds rows traj_forward leaves with traj_offsets -> (gain (B,) f64:
    the team's mean reward minus the team's without member b; count (B,) int64: the points with lo_b > 0), on the host.  Integer
    sums on the device: the same bits every run."""
    L = _lib.lib()
    B = lo_members.shape[0]
    nbytes = L.tohip_team_member_gains_bytes(B)
    sums = torch.empty(nbytes // 8, dtype=torch.int64, device=cloud.device)
    with torch.cuda.device(cloud.device):
        check(L.tohip_team_member_gains(ptr(cloud.blob), cloud.n, ptr(lo_members), B, ptr(prior.buf) if prior is not None else None, ptr(sums),
                                        nbytes, stream_ptr()), "tohip_team_member_gains")
    h = sums.cpu()
    shift = 47 - (cloud.n - 1).bit_length()   # the reward kernel's fixed point: 2^shift per unit, N 2^shift <= 2^47
    gain = (h[0] - h[1:1 + B]).to(torch.float64) / float(2 ** shift) / cloud.n
    return gain, h[1 + B:1 + 2 * B].clone()


CLEARANCE_MAP_MAX_VOXELS = 64   # of radius / resolution: a waypoint's window is at most 131^3 voxels
CLEARANCE_PREFILLED = _lib.CONSTANTS["TOHIP_TRAJ_CLEARANCE_PREFILLED"]


class MapObstacles:
    """The clearance term's obstacles taken from a map (clearance_map_kernels.hip, DESIGN.md 10 "Clearance from the map"): accepted
    by clearance, clearance_segments and clearance_rows where they take a PackedCloud.  map: an OccupancyGrid, a SpaceMap or an
    EvidenceMap; unknown 'free': the occupied voxels are the obstacles; 'obstacle' (a SpaceMap or an EvidenceMap: the free plane
    tells unknown from free): the never-seen voxels as well — check_field's rule, ValueError otherwise.  Holds the map's two planes
    — the objects, not copies: every query reads the buffers as they are then — and idx is a voxel's linear index (z ny + y) nx + x."""
    __slots__ = ("map", "unknown", "occupied", "free")

    def __init__(self, map, unknown="free"):
        if not isinstance(map, (OccupancyGrid, SpaceMap, EvidenceMap)):
            raise ValueError(f"clearance_map must be an ops.OccupancyGrid, an ops.SpaceMap or an ops.EvidenceMap, got {type(map).__name__}")
        self.map, self.unknown = map, unknown
        self.occupied, self.free, _, _ = check_field(map.space if isinstance(map, EvidenceMap) else map, D=1, unknown=unknown)

    def same_as(self, other):
        """The same map objects read under the same rule (what a batched or a team run demands of its members)."""
        return (isinstance(other, MapObstacles) and other.occupied is self.occupied and other.free is self.free and
                other.unknown == self.unknown)

    def check_radius(self, radius):
        voxels = float(np.float32(radius)) / float(np.float32(self.occupied.resolution))
        if not voxels <= CLEARANCE_MAP_MAX_VOXELS:
            raise ValueError(f"clearance_radius {radius!r} is {voxels:g} voxels of this map; the map query takes at most "
                             f"{CLEARANCE_MAP_MAX_VOXELS} ({CLEARANCE_MAP_MAX_VOXELS * self.occupied.resolution:g} m at this resolution)")


def _clearance_source(source, radius, device):
    """What names a clearance query's obstacles to the C ABI -> (the entry points' infix, their leading arguments): a PackedCloud's
    blob and size, or a MapObstacles' planes and geometry (its radius cap and its device are checked here)."""
    if not isinstance(source, MapObstacles):
        return "", (source.blob.data_ptr(), source.n)
    source.check_radius(radius)
    g = source.occupied
    if g.device != device:
        raise ValueError(f"the clearance map lives on {g.device}, the positions on {device}")
    return "_map", (ptr(g.buf), ptr(source.free.buf) if source.free is not None else None, g.buf.numel(), ctypes.byref(g.geom))


def clearance(cloud, positions, radius, weight=0.0, grad=None, accumulate=False, want_value=False, terms=None):
    """tohip_clearance: each position's nearest cloud point within `radius` -> (d (n,) f32, +inf when none; idx (n,) int32 caller rows,
    -1 when none[, value: 0-d f32 = weight x sum (radius - d)^2]).  grad (n, 3) f32, optional: the term's gradient rows, overwritten
    (accumulate=False) or added to.  terms (optional): a float64 tensor of n entries that receives the per-position (radius - d)^2.
    cloud: a PackedCloud, or a MapObstacles (tohip_clearance_map: the nearest obstacle voxel's centre, idx its linear index)."""
    _require_cuda(positions, "positions")
    q = positions.detach().to(torch.float32).contiguous()
    if q.dim() != 2 or q.shape[1] != 3 or q.shape[0] == 0:
        raise ValueError(f"positions must be (n,3) with n>0, got {tuple(q.shape)}")
    r, w = check_clearance(radius, weight)
    L = _lib.lib()
    n, dev = q.shape[0], q.device
    d = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    value = torch.empty((), dtype=torch.float32, device=dev) if want_value else None
    wsb = L.tohip_clearance_workspace_bytes(n)
    if terms is None:
        terms = torch.empty(wsb // 8, dtype=torch.float64, device=dev)
    if grad is not None and not (grad.is_contiguous() and grad.dtype == torch.float32 and tuple(grad.shape) == (n, 3)):
        raise ValueError("grad must be a contiguous (n,3) float32 tensor")
    infix, source = _clearance_source(cloud, r, dev)
    name = f"tohip_clearance{infix}"
    with torch.cuda.device(dev):
        check(getattr(L, name)(*source, ptr(q), n, r, w, ptr(d), ptr(idx), ptr(value), ptr(grad), int(bool(accumulate)), ptr(terms),
                               terms.numel() * 8, stream_ptr()), name)
    return (d, idx, value) if want_value else (d, idx)


def clearance_segments(cloud, poses, radius, weight=0.0, n_traj=1, grad=None, want_value=False, terms=None):
    """tohip_clearance_segments: the nearest cloud point within `radius` of every segment between consecutive waypoints of each of the
    n_traj equal-length trajectories laid end to end in `poses` (n_traj W, 3), W >= 2 -> (d (n_traj (W-1),) f32, +inf when none; idx
    int32 caller rows, -1 when none; s f32: where along the segment the closest point lies, 0 = its first end[, value (n_traj,) f32 =
    weight x sum (radius - d)^2 per trajectory]).  grad (n_traj W, 3) f32, optional: the term's per-waypoint gradient rows,
    overwritten.  terms (optional): a float64 tensor of tohip_clearance_segments_workspace_bytes / 8 entries; its first n_traj W
    receive the per-waypoint terms ((radius - d)^2 of the segment a waypoint starts, 0 for a trajectory's last)."""
    _require_cuda(poses, "poses")
    q = poses.detach().to(torch.float32).contiguous()
    B = int(n_traj)
    if q.dim() != 2 or q.shape[1] != 3 or B < 1 or q.shape[0] % B or q.shape[0] // B < 2:
        raise ValueError(f"poses must be (n_traj W, 3) with W >= 2, got {tuple(q.shape)} for n_traj={n_traj}")
    r, w = check_clearance(radius, weight)
    L = _lib.lib()
    n, dev = q.shape[0], q.device
    W = n // B
    d = torch.empty(n - B, dtype=torch.float32, device=dev)
    idx = torch.empty(n - B, dtype=torch.int32, device=dev)
    s = torch.empty(n - B, dtype=torch.float32, device=dev)
    value = torch.empty(B, dtype=torch.float32, device=dev) if want_value else None
    if terms is None:
        terms = clearance_terms(W, B, "segments", dev)
    if grad is not None and not (grad.is_contiguous() and grad.dtype == torch.float32 and tuple(grad.shape) == (n, 3)):
        raise ValueError("grad must be a contiguous (n_traj W, 3) float32 tensor")
    infix, source = _clearance_source(cloud, r, dev)
    name = f"tohip_clearance{infix}_segments"
    with torch.cuda.device(dev):
        check(getattr(L, name)(*source, ptr(q), W, B, r, w, ptr(d), ptr(idx), ptr(s), ptr(value), ptr(grad), ptr(terms), terms.numel() * 8,
                               stream_ptr()), name)
    return (d, idx, s, value) if want_value else (d, idx, s)


def clearance_edges(cloud, a, b, radius):
    """tohip_clearance_edges: the nearest cloud point within `radius` of each of the E unrelated segments a[e] -> b[e] (two (E,3)
    tensors on the cloud's device) -> (d (E,) f32, +inf when none; idx (E,) int32 caller rows, -1 when none; s (E,) f32) — the bits
    clearance_segments gives for the same two ends.  One wave per edge, one launch."""
    _require_cuda(a, "a")
    _require_cuda(b, "b")
    a = a.detach().to(torch.float32).contiguous()
    b = b.detach().to(torch.float32).contiguous()
    if a.dim() != 2 or a.shape[1] != 3 or a.shape[0] == 0 or b.shape != a.shape:
        raise ValueError(f"a and b must both be (E,3) with E > 0, got {tuple(a.shape)} and {tuple(b.shape)}")
    r = check_tour_radius(radius)
    E, dev = a.shape[0], a.device
    d = torch.empty(E, dtype=torch.float32, device=dev)
    idx = torch.empty(E, dtype=torch.int32, device=dev)
    s = torch.empty(E, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().tohip_clearance_edges(cloud.blob.data_ptr(), cloud.n, ptr(a), ptr(b), E, r, ptr(d), ptr(idx), ptr(s), stream_ptr()),
              "tohip_clearance_edges")
    return d, idx, s


TOUR_MAX_NODES = _lib.CONSTANTS["TOHIP_TOUR_MAX_NODES"]
TOUR_UNIT = 2.0 ** -20   # metres per unit of a tour's integer lengths


def check_tour_radius(radius):
    """A clearance radius that is given: a finite number > 0 (ValueError otherwise)."""
    r = _float_or_nan(radius)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"clearance_radius must be a finite number > 0, got {radius!r}")
    return r


def check_tour(poses, quats=None, clearance_radius=None, closed=False, max_moves=None):
    """The arguments of a tour: poses (n,3) a floating tensor with 2 <= n <= TOUR_MAX_NODES, quats None or (n,4), clearance_radius
    None or a finite number > 0, max_moves None (4 n) or an integer >= 0 -> (n, radius or None, max_moves); ValueError otherwise."""
    _check_float_rows(poses, "poses", "a floating-point tensor of shape (n,3)", 3)
    n = poses.shape[0]
    if n < 2:
        raise ValueError(f"poses must hold n >= 2 nodes (the start and at least one view), got {n}")
    if n > TOUR_MAX_NODES:
        raise ValueError(f"poses must hold at most {TOUR_MAX_NODES} nodes, got n = {n}")
    if quats is not None:
        _check_float_rows(quats, "quats", f"None or a floating-point tensor of shape ({n},4)", 4, n)
    r = check_tour_radius(clearance_radius) if clearance_radius is not None else None
    if not isinstance(closed, (bool, np.bool_)):
        raise ValueError(f"closed must be True or False, got {closed!r}")
    if max_moves is None:
        max_moves = 4 * n
    elif not _is_int(max_moves) or max_moves < 0:
        raise ValueError(f"max_moves must be None or an integer >= 0, got {max_moves!r}")
    return n, r, int(max_moves)


def tour_layout(n):
    """Byte offsets of a tour buffer's sections (include/trajopt_hip.h, tohip_tour_bytes): every section aligned to 256 bytes."""
    return _sections(256, (("order", 4 * n), ("unreachable", n), ("D", 8 * n * n), ("nxt", 4 * n * n)))


def tour_edge_ends(n, device):
    """(i, j): the ends of the n (n - 1) / 2 edges in the order of their indices (the upper triangle, row-major)."""
    ij = torch.triu_indices(n, n, offset=1, device=device)
    return ij[0], ij[1]


def _tour_plan(nodes, edge_idx, closed, max_moves, via, via_D=None):
    """tour_plan (via=False) and tour_plan_via (via=True) behind their signatures: the checks, the buffer, the launch -> (buf, via_flag
    or None)."""
    _require_cuda(nodes, "nodes")
    n = nodes.shape[0]
    L = _lib.lib()
    nbytes = L.tohip_tour_bytes(n)
    if nbytes == 0 or tuple(nodes.shape) != (n, 3) or nodes.dtype != torch.float32 or not nodes.is_contiguous():
        raise ValueError(f"nodes must be a contiguous (n,3) float32 tensor with 2 <= n <= {TOUR_MAX_NODES}, got {tuple(nodes.shape)}")
    if edge_idx is not None and not (edge_idx.dtype == torch.int32 and edge_idx.is_contiguous() and edge_idx.numel() == n * (n - 1) // 2
                                     and edge_idx.device == nodes.device):
        raise ValueError(f"edge_idx must be {n * (n - 1) // 2} contiguous int32 on the nodes' device")
    if via and not (torch.is_tensor(via_D) and via_D.dtype == torch.int64 and via_D.dim() == 2 and via_D.shape[0] >= n and via_D.shape[1] >= n
                    and via_D.stride(1) == 1 and via_D.stride(0) >= via_D.shape[1] and via_D.device == nodes.device):
        raise ValueError(f"via_D must be an int64 tensor of at least ({n},{n}) with unit column stride on the nodes' device")
    assert nbytes == tour_layout(n)["total"]
    buf = torch.empty(nbytes, dtype=torch.uint8, device=nodes.device)
    closed, max_moves = int(bool(closed)), int(4 * n if max_moves is None else max_moves)
    with torch.cuda.device(nodes.device):
        if not via:
            check(L.tohip_tour_plan(ptr(nodes), n, ptr(edge_idx), closed, max_moves, ptr(buf), nbytes, stream_ptr()), "tohip_tour_plan")
            return buf, None
        flag = torch.empty((n, n), dtype=torch.uint8, device=nodes.device)
        check(L.tohip_tour_plan_via(ptr(nodes), n, ptr(edge_idx), ptr(via_D), via_D.stride(0), closed, max_moves, ptr(buf), nbytes, ptr(flag),
                                    stream_ptr()), "tohip_tour_plan_via")
    return buf, flag


def tour_plan(nodes, edge_idx=None, closed=False, max_moves=None):
    """tohip_tour_plan over nodes (n,3) f32 on the device and the edge stage's idx (n (n - 1) / 2 int32) or None -> the tour buffer
    (uint8, tour_layout(n)) on the device; launches only."""
    return _tour_plan(nodes, edge_idx, closed, max_moves, False)[0]


ROADMAP_MAX_NODES = _lib.CONSTANTS["TOHIP_ROADMAP_MAX_NODES"]
ROADMAP_MAX_K = _lib.CONSTANTS["TOHIP_ROADMAP_MAX_K"]
ROADMAP_MAX_SOURCES = _lib.CONSTANTS["TOHIP_ROADMAP_MAX_SOURCES"]
ROADMAP_INF = 1 << 62       # a route length where no route exists
ROADMAP_MAX_LEN = 1 << 40   # the longest edge that can be open, in units of 2^-20 m


def check_roadmap_options(k=12, clearance_radius=None, max_edge=None):
    """k an integer in 1..ROADMAP_MAX_K, clearance_radius None or a finite number > 0, max_edge None or a number >= 0 (NaN refused)
    -> (k, radius or None, max_edge as a float, +inf for None); ValueError otherwise."""
    if not _is_int(k) or not 1 <= k <= ROADMAP_MAX_K:
        raise ValueError(f"k must be an integer in 1..{ROADMAP_MAX_K}, got {k!r}")
    r = check_tour_radius(clearance_radius) if clearance_radius is not None else None
    me = float("inf") if max_edge is None else _float_or_nan(max_edge)
    if not me >= 0.0:
        raise ValueError(f"max_edge must be None or a number >= 0, got {max_edge!r}")
    return int(k), r, me


def check_roadmap(nodes, k=12, clearance_radius=None, max_edge=None, sources=None, sweeps_per_check=8):
    """The arguments of a roadmap: nodes (M,3) a floating tensor with 2 <= M <= ROADMAP_MAX_NODES, k an integer in 1..ROADMAP_MAX_K,
    clearance_radius None or a finite number > 0, max_edge None or a number >= 0 (NaN refused), sources None or 1..ROADMAP_MAX_SOURCES
    integer node indices in [0, M) (a list, an array or a tensor), sweeps_per_check an integer >= 1 -> (M, k, radius or None,
    max_edge as a float (+inf for None), sources as a list or None); ValueError otherwise.  Nothing is launched."""
    _check_float_rows(nodes, "nodes", "a floating-point tensor of shape (M,3)", 3)
    M = nodes.shape[0]
    if M < 2 or M > ROADMAP_MAX_NODES:
        raise ValueError(f"nodes must hold 2 <= M <= {ROADMAP_MAX_NODES} nodes, got M = {M}")
    k, r, me = check_roadmap_options(k, clearance_radius, max_edge)
    if not _is_int(sweeps_per_check) or sweeps_per_check < 1:
        raise ValueError(f"sweeps_per_check must be an integer >= 1, got {sweeps_per_check!r}")
    src = None
    if sources is not None:
        a = sources.detach().cpu().numpy() if torch.is_tensor(sources) else np.asarray(sources)
        if a.ndim != 1 or a.size < 1 or a.size > ROADMAP_MAX_SOURCES or a.dtype.kind not in "iu":
            raise ValueError(f"sources must be 1..{ROADMAP_MAX_SOURCES} integer node indices in one dimension, got "
                             f"shape {a.shape} of {a.dtype}")
        if (a < 0).any() or (a >= M).any():
            raise ValueError(f"sources must lie in [0, {M}), got {a.min()}..{a.max()}")
        src = [int(v) for v in a]
    return M, int(k), r, me, src


def roadmap_knn(nodes, k=12, max_edge=None):
    """tohip_roadmap_knn over nodes (M,3) f32 on the device -> (nbr (M,k) int32, length_fixed (M,k) int64): each node's k nearest
    others by the exact f64 key (d2, j), ties to the lower j, -1 where no candidate fills a slot.  One launch."""
    M, k, _, me, _ = check_roadmap(nodes, k, None, max_edge)
    _require_cuda(nodes, "nodes")
    if nodes.dtype != torch.float32 or not nodes.is_contiguous():
        raise ValueError("nodes must be a contiguous float32 tensor")
    nbr = torch.empty((M, k), dtype=torch.int32, device=nodes.device)
    length = torch.empty((M, k), dtype=torch.int64, device=nodes.device)
    with torch.cuda.device(nodes.device):
        check(_lib.lib().tohip_roadmap_knn(ptr(nodes), M, k, me, ptr(nbr), ptr(length), stream_ptr()), "tohip_roadmap_knn")
    return nbr, length


def roadmap_routes_layout(M, S):
    """Byte offsets of a routes buffer's sections (include/trajopt_hip.h, tohip_roadmap_routes_bytes)."""
    return _sections(0, (("D", 8 * M * S), ("pred", 4 * M * S), ("changed", 256)))


def roadmap_routes(nbr, length_fixed, open_, sources, sweeps_per_check=8):
    """Shortest routes from `sources` over the open slots of a roadmap -> (D (S,M) int64, pred (S,M) int32, sweeps).  The batch loop
    around tohip_roadmap_relax: sweeps_per_check sweeps per call, one 4-byte read-back per batch, until a sweep lowered nothing; then
    tohip_roadmap_pred.  M sweeps always suffice: a table still moving after them raises the library's 'did not converge' error."""
    _require_cuda(nbr, "nbr")
    dev = nbr.device
    if nbr.dim() != 2 or nbr.dtype != torch.int32 or not nbr.is_contiguous():
        raise ValueError(f"nbr must be a contiguous (M,k) int32 tensor, got {tuple(nbr.shape)} of {nbr.dtype}")
    M, k = nbr.shape
    if not (length_fixed.dtype == torch.int64 and length_fixed.is_contiguous() and tuple(length_fixed.shape) == (M, k)
            and length_fixed.device == dev):
        raise ValueError(f"length_fixed must be a contiguous ({M},{k}) int64 tensor on the nodes' device")
    if open_.dtype == torch.bool:
        open_ = open_.view(torch.uint8)
    if not (open_.dtype == torch.uint8 and open_.is_contiguous() and tuple(open_.shape) == (M, k) and open_.device == dev):
        raise ValueError(f"open must be a contiguous ({M},{k}) bool or uint8 tensor on the nodes' device")
    if not 1 <= k <= ROADMAP_MAX_K or not 2 <= M <= ROADMAP_MAX_NODES:
        raise ValueError(f"a roadmap holds 2 <= M <= {ROADMAP_MAX_NODES} nodes and 1 <= k <= {ROADMAP_MAX_K} slots, got ({M},{k})")
    _, _, _, _, src = check_roadmap(torch.empty((M, 3)), k, None, None, sources, sweeps_per_check)
    if src is None:
        raise ValueError("sources must be given")
    S, per = len(src), int(sweeps_per_check)
    L = _lib.lib()
    lay = roadmap_routes_layout(M, S)
    assert L.tohip_roadmap_routes_bytes(M, S) == lay["total"]
    buf = torch.empty(lay["total"], dtype=torch.uint8, device=dev)
    D = buf[:8 * M * S].view(torch.int64).view(S, M)
    pred = buf[lay["pred"]:lay["pred"] + 4 * M * S].view(torch.int32).view(S, M)
    changed = buf[lay["changed"]:lay["changed"] + 4].view(torch.int32)
    src_t = torch.tensor(src, dtype=torch.int32, device=dev)
    sweeps = 0
    with torch.cuda.device(dev):
        while True:
            if sweeps >= M:
                check(_lib.ENOTCONV, "roadmap_routes")
            n = min(per, M - sweeps)
            check(L.tohip_roadmap_relax(ptr(nbr), ptr(length_fixed), ptr(open_), M, k, ptr(src_t), S, ptr(D), n, ptr(changed),
                                        int(sweeps == 0), stream_ptr()), "tohip_roadmap_relax")
            last = int(changed.item())   # the batch's one read-back
            sweeps += n if last == n else last + 1   # (the sweeps that mattered: up to the first that lowered nothing)
            if last < n:
                break
        check(L.tohip_roadmap_pred(ptr(nbr), ptr(length_fixed), ptr(open_), M, k, ptr(src_t), S, ptr(D), ptr(pred), stream_ptr()),
              "tohip_roadmap_pred")
    return D, pred, sweeps


def tour_plan_via(nodes, edge_idx, via_D, closed=False, max_moves=None):
    """tohip_tour_plan_via: tour_plan whose initial legs are min(direct, via_D[i][j]) — via_D (n or more rows, n or more columns)
    int64 on the device, row i the roadmap's routes from tour node i -> (the tour buffer, via_flag (n,n) uint8); launches only."""
    return _tour_plan(nodes, edge_idx, closed, max_moves, True, via_D)


PATH_MAX_NODES = _lib.CONSTANTS["TOHIP_PATH_MAX_NODES"]
PATH_MAX_ROWS = _lib.CONSTANTS["TOHIP_PATH_MAX_ROWS"]


def check_path(path, quats=None, keep=None, window=None, spacing=None, max_rows=None):
    """The arguments of a path refinement: path (L,3) a floating tensor with 2 <= L <= PATH_MAX_NODES, quats None or (L,4) floating,
    keep None or (L,) bool / uint8, window None (L - 1) or an integer in 1..L-1, spacing None or a finite number > 0, max_rows None
    (PATH_MAX_ROWS) or an integer in 1..PATH_MAX_ROWS -> (L, window, spacing as a float or None, max_rows); ValueError otherwise.
    Nothing is launched."""
    _check_float_rows(path, "path", "a floating-point tensor of shape (L,3)", 3)
    L = path.shape[0]
    if L < 2 or L > PATH_MAX_NODES:
        raise ValueError(f"path must hold 2 <= L <= {PATH_MAX_NODES} nodes, got L = {L}")
    if quats is not None:
        _check_float_rows(quats, "quats", f"None or a floating-point tensor of shape ({L},4)", 4, L)
    if keep is not None and (not torch.is_tensor(keep) or keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (L,)):
        raise ValueError(f"keep must be None or a bool / uint8 tensor of shape ({L},), got "
                         f"{(tuple(keep.shape), keep.dtype) if torch.is_tensor(keep) else type(keep).__name__}")
    if window is None:
        window = L - 1
    elif not _is_int(window) or not 1 <= window <= L - 1:
        raise ValueError(f"window must be None or an integer in 1..{L - 1}, got {window!r}")
    h = None
    if spacing is not None:
        h = _float_or_nan(spacing)
        with np.errstate(over="ignore"):
            hf = float(np.float32(h))   # what the library is handed
        if not (np.isfinite(hf) and hf > 0.0):
            raise ValueError(f"spacing must be None or a finite number > 0 (as a float32), got {spacing!r}")
    if max_rows is None:
        max_rows = PATH_MAX_ROWS
    elif not _is_int(max_rows) or not 1 <= max_rows <= PATH_MAX_ROWS:
        raise ValueError(f"max_rows must be None or an integer in 1..{PATH_MAX_ROWS}, got {max_rows!r}")
    return L, int(window), h, int(max_rows)


def path_layout(L, max_rows):
    """Byte offsets of a refined path's buffer (include/trajopt_hip.h, tohip_path_bytes): every section aligned to 256 bytes."""
    return _sections(256, (("D", 8 * L), ("pred", 4 * L), ("corner", 4 * L), ("out_poses", 12 * max_rows), ("out_quats", 16 * max_rows),
                           ("row_node", 4 * max_rows)))


def path_refine(P, quats, keep, open_band, window=None, spacing=None, max_rows=None):
    """tohip_path_refine over P (L,3) f32 contiguous on the device, quats (L,4) f32 or None, keep (L,) bool / uint8 or None and
    open_band (L,W) bool / uint8, all on P's device -> the buffer (uint8, path_layout(L, max_rows)) on the device; one launch.  The
    header's status word is the caller's to read."""
    L, W, h, max_rows = check_path(P, quats, keep, window, spacing, max_rows)
    _require_cuda(P, "P")
    dev = P.device
    if P.dtype != torch.float32 or not P.is_contiguous():
        raise ValueError("P must be a contiguous float32 tensor")
    if quats is not None and not (quats.dtype == torch.float32 and quats.is_contiguous() and quats.device == dev):
        raise ValueError("quats must be a contiguous float32 tensor on P's device")
    if keep is not None:
        keep = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
        if not (keep.is_contiguous() and keep.device == dev):
            raise ValueError("keep must be contiguous on P's device")
    if torch.is_tensor(open_band) and open_band.dtype == torch.bool:
        open_band = open_band.view(torch.uint8)
    if not (torch.is_tensor(open_band) and open_band.dtype == torch.uint8 and open_band.is_contiguous() and tuple(open_band.shape) == (L, W)
            and open_band.device == dev):
        raise ValueError(f"open_band must be a contiguous ({L},{W}) bool or uint8 tensor on P's device")
    lib = _lib.lib()
    lay = path_layout(L, max_rows)
    assert lib.tohip_path_bytes(L, max_rows) == lay["total"]
    buf = torch.empty(lay["total"], dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.tohip_path_refine(ptr(P), ptr(quats), ptr(keep), L, W, ptr(open_band), 0.0 if h is None else h, max_rows, ptr(buf),
                                    lay["total"], stream_ptr()), "tohip_path_refine")
    return buf


VIEW_MAX_POSITIONS = _lib.CONSTANTS["TOHIP_VIEW_MAX_POSITIONS"]
VIEW_SECTORS = (8, 16, 32, 64, 128)
VIEW_MAX_PER_POSITION = _lib.CONSTANTS["TOHIP_VIEW_MAX_PER_POSITION"]
VIEW_MAX_WEIGHT = 32768         # a point's largest weight: 65 536 points of a block x 32 768 < 2^32
VIEW_MIN_DIST = float(np.float32(1e-3))


def check_propose(n_points, positions, open=None, weights=None, sectors=32, min_dist=1.0, max_dist=5.0, tan_v=1.0, hw=0, n_per=2, sep=None,
                  min_score=0):
    """The arguments of a view proposal over a cloud of n_points: positions (M,3) a floating tensor, 1 <= M <= VIEW_MAX_POSITIONS (a
    coordinate that is not finite is allowed: that position counts nothing); open None or (M,) bool / uint8; weights None or (n_points,)
    int32, each in [0, VIEW_MAX_WEIGHT]; sectors one of VIEW_SECTORS; 1e-3 <= min_dist < max_dist and tan_v >= 0, finite as float32;
    hw an integer >= 0 with 2 hw + 1 <= sectors; n_per an integer in 1..VIEW_MAX_PER_POSITION; sep None (2 hw) or an integer in
    0..sectors; min_score an integer >= 0 -> (M, sectors, min_dist, max_dist, tan_v, hw, n_per, sep, min_score); ValueError otherwise.
    Nothing is launched (the weights' range is read where they live)."""
    _check_float_rows(positions, "positions", "a floating-point tensor of shape (M,3)", 3)
    M = positions.shape[0]
    if M < 1 or M > VIEW_MAX_POSITIONS:
        raise ValueError(f"positions must hold 1 <= M <= {VIEW_MAX_POSITIONS} rows, got M = {M}")
    if open is not None and (not torch.is_tensor(open) or open.dtype not in (torch.bool, torch.uint8) or tuple(open.shape) != (M,)):
        raise ValueError(f"open must be None or a bool / uint8 tensor of shape ({M},), got "
                         f"{(tuple(open.shape), open.dtype) if torch.is_tensor(open) else type(open).__name__}")
    if weights is not None:
        if not torch.is_tensor(weights) or weights.dtype != torch.int32 or tuple(weights.shape) != (n_points,):
            raise ValueError(f"weights must be None or an int32 tensor of shape ({n_points},) (one entry per point), got "
                             f"{(tuple(weights.shape), weights.dtype) if torch.is_tensor(weights) else type(weights).__name__}")
        if n_points and (int(weights.min()) < 0 or int(weights.max()) > VIEW_MAX_WEIGHT):
            raise ValueError(f"weights must lie in [0, {VIEW_MAX_WEIGHT}], got {int(weights.min())}..{int(weights.max())}")
    if not _is_int(sectors) or sectors not in VIEW_SECTORS:
        raise ValueError(f"sectors must be one of {VIEW_SECTORS}, got {sectors!r}")
    vals = []
    for name, v in (("min_dist", min_dist), ("max_dist", max_dist), ("tan_v", tan_v)):
        with np.errstate(over="ignore"):
            f = float(np.float32(_float_or_nan(v)))   # what the library is handed
        if not np.isfinite(f):
            raise ValueError(f"{name} must be a finite number (as a float32), got {v!r}")
        vals.append(f)
    mn, mx, tv = vals
    if not (mn >= VIEW_MIN_DIST and mn < mx):
        raise ValueError(f"min_dist and max_dist must satisfy 1e-3 <= min_dist < max_dist, got {min_dist!r} and {max_dist!r}")
    if not tv >= 0.0:
        raise ValueError(f"tan_v must be >= 0, got {tan_v!r}")
    if not _is_int(hw) or hw < 0 or 2 * hw + 1 > sectors:
        raise ValueError(f"hw must be an integer >= 0 with 2 hw + 1 <= sectors = {sectors}, got {hw!r}")
    if not _is_int(n_per) or not 1 <= n_per <= VIEW_MAX_PER_POSITION:
        raise ValueError(f"n_per must be an integer in 1..{VIEW_MAX_PER_POSITION}, got {n_per!r}")
    if sep is None:
        sep = 2 * hw
    elif not _is_int(sep) or not 0 <= sep <= sectors:
        raise ValueError(f"sep must be None or an integer in 0..{sectors}, got {sep!r}")
    if not _is_int(min_score) or min_score < 0 or min_score >= 1 << 63:
        raise ValueError(f"min_score must be an integer >= 0, got {min_score!r}")
    return M, int(sectors), mn, mx, tv, int(hw), int(n_per), int(sep), int(min_score)


def view_histogram(cloud, positions, open=None, weights=None, sectors=32, min_dist=1.0, max_dist=5.0, tan_v=1.0, prune=True):
    """tohip_view_histogram over a PackedCloud (sorted or not): positions (M,3) f32 contiguous, open (M,) bool / uint8 or None (every
    position open) and weights (N,) int32 in the CALLER's row order or None (every point weighs 1), all on the cloud's device -> hist
    (M, sectors) int64: per position and bearing sector the summed weights of the points inside the range shell and the vertical
    field of view (propose_kernels.hip).  prune=False tests every tile against every position (the same bits; for timing).  One
    memset and one launch."""
    M, S, mn, mx, tv, _, _, _, _ = check_propose(cloud.n, positions, open, weights, sectors, min_dist, max_dist, tan_v)
    _require_cuda(positions, "positions")
    dev = cloud.device
    if positions.dtype != torch.float32 or not positions.is_contiguous() or positions.device != dev:
        raise ValueError("positions must be a contiguous float32 tensor on the cloud's device")
    if open is None:
        open = torch.ones(M, dtype=torch.uint8, device=dev)
    open = open.view(torch.uint8) if open.dtype == torch.bool else open
    if not (open.is_contiguous() and open.device == dev):
        raise ValueError("open must be contiguous on the cloud's device")
    if weights is not None and not (weights.is_contiguous() and weights.device == dev):
        raise ValueError("weights must be contiguous on the cloud's device")
    from .synth import propose_tables   # (numpy only)
    table = np.ascontiguousarray(propose_tables(S)[0].reshape(-1))
    table_c = (ctypes.c_float * max(1, table.size))(*table.tolist())
    hist = torch.empty((M, S), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().tohip_view_histogram(ptr(cloud.blob), cloud.n, ptr(positions), ptr(open), M, ptr(weights), S, table_c, mn, mx, tv,
                                              int(bool(prune)), ptr(hist), stream_ptr()), "tohip_view_histogram")
    return hist


def view_headings(hist, hw=0, n_per=2, sep=None, min_score=0):
    """tohip_view_headings over hist (M,S) int64 contiguous on the device -> (heading (M,n_per) int32, score (M,n_per) int64): per
    position the n_per best headings by the circular window sum over |j| <= hw, ties to the lowest heading, each suppressing the
    headings within sep (default 2 hw: disjoint windows) of it; -1 / 0 where fewer reach max(min_score, 1).  One launch."""
    if not torch.is_tensor(hist) or hist.dtype != torch.int64 or hist.dim() != 2 or not hist.is_contiguous():
        raise ValueError(f"hist must be a contiguous (M,S) int64 tensor, got "
                         f"{(tuple(hist.shape), hist.dtype) if torch.is_tensor(hist) else type(hist).__name__}")
    M, S = hist.shape
    _, S, _, _, _, hw, n_per, sep, min_score = check_propose(0, torch.empty((M, 3)), sectors=S, hw=hw, n_per=n_per, sep=sep, min_score=min_score)
    _require_cuda(hist, "hist")
    heading = torch.empty((M, n_per), dtype=torch.int32, device=hist.device)
    score = torch.empty((M, n_per), dtype=torch.int64, device=hist.device)
    with torch.cuda.device(hist.device):
        check(_lib.lib().tohip_view_headings(ptr(hist), M, S, hw, n_per, sep, min_score, ptr(heading), ptr(score), stream_ptr()),
              "tohip_view_headings")
    return heading, score


def clearance_terms(n_wps, n_traj, mode, device):
    """The float64 buffer the clearance query of `mode` fills for n_traj trajectories of n_wps waypoints: the per-waypoint terms lead
    it in either mode (what the step tails, the regularisers' kernel and the team calls read)."""
    L = _lib.lib()
    nbytes = (L.tohip_clearance_segments_workspace_bytes(n_wps, n_traj) if mode == "segments" else
              L.tohip_clearance_workspace_bytes(n_wps * n_traj))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def clearance_rows(cloud, poses, radius, weight, mode, n_traj, grad, terms):
    """The clearance term of `mode` for n_traj trajectories laid end to end: its per-waypoint gradient rows into `grad` and terms into
    `terms` (clearance_terms) — one launch for 'waypoints', two for 'segments'.  cloud: a PackedCloud or a MapObstacles."""
    if mode == "segments":
        clearance_segments(cloud, poses, radius, weight, n_traj=n_traj, grad=grad, terms=terms)
    else:
        clearance(cloud, poses, radius, weight, grad=grad, terms=terms)


def clearance_scratch_views(scratch, n_rows):
    """The two parts of a plan's clearance scratch (tohip_traj_clearance[_segments]_scratch_bytes, a uint8 tensor) as clearance_rows
    takes them -> (grad (n_rows, 3) f32 at offset 0, terms: the float64 rest from the 256-aligned end of the rows — the
    per-waypoint terms, then in 'segments' mode the per-segment parts): a caller that fills them sets CLEARANCE_PREFILLED."""
    off = (12 * n_rows + 255) // 256 * 256
    return scratch[:12 * n_rows].view(torch.float32).view(n_rows, 3), scratch[off:].view(torch.float64)


def traj_step_stats(cloud, ws):
    """What the last forward over `ws` found -> dict(flagged_pairs, candidate_slots, slots, virtual_waypoints, flagged_fraction,
    evaluated_pairs: those the last culled pass 1 evaluated)."""
    st = torch.zeros(5, dtype=torch.int64, device=cloud.device)
    with torch.cuda.device(cloud.device):
        check(_lib.lib().tohip_traj_step_stats(cloud.n, ws.n_virtual, ws.n_traj, ptr(ws.buf), ws.bytes, ptr(st), stream_ptr()), "tohip_traj_step_stats")
    f, c, s, v, e = (int(x) for x in st.cpu())
    return dict(flagged_pairs=f, candidate_slots=c, slots=s, virtual_waypoints=v, flagged_fraction=f / max(1, s * v), evaluated_pairs=e)


class PoseWorkspace:
    """Scratch of the ModelPose kernels.  The default is the single-pose calls' size; n_poses > 1, or multi=True, sizes it for the
    multi-pose calls (pose_forward_backward_multi) over up to n_poses poses — which serves the single-pose calls too."""

    def __init__(self, cloud, n_poses=1, multi=False):
        L = _lib.lib()
        if int(n_poses) < 1:
            raise ValueError(f"n_poses must be at least 1, got {n_poses}")
        self.n_poses, self.multi = int(n_poses), bool(multi) or int(n_poses) > 1
        self.bytes = L.tohip_pose_workspace_bytes_multi(cloud.n, self.n_poses) if self.multi else L.tohip_pose_workspace_bytes(cloud.n)
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=cloud.device)


def _occ_row(cloud, occ, rows=1, mask=None):
    """An occlusion bit row argument of the pose calls: (rows, npad/32) or (npad/32,) int32 words on the cloud's device (what
    occlusion_bits returns).  A float mask besides it is an error (the C ABI's TOHIP_EINVAL)."""
    if mask is not None:
        raise ValueError("give a float mask or occlusion bit rows, not both")
    words = cloud.npad // 32
    if occ.dtype != torch.int32 or not occ.is_contiguous() or occ.device != cloud.device or occ.numel() != rows * words:
        raise ValueError(f"occ must be a contiguous int32 tensor of {rows} x {words} words on {cloud.device} (ops.occlusion_bits' rows)")
    return occ


class PosePlan:
    """The pose visibility calls over one cloud, camera and workspace, with everything constant converted once (ModelPose's loop is
    host-bound): ModelPose's autograd nodes and the pose_* wrappers below go through it.  Each call takes a float mask or, in its
    place, occlusion bit rows `occ` (the _bits twin then runs).  Nothing is checked here: the wrappers check their arguments."""

    def __init__(self, cloud, cam, ws):
        self.L = _lib.lib()
        self.blob, self.n = cloud.blob.data_ptr(), cloud.n
        self.cam = cam.ref()
        self.ws, self.wsb = ws.buf.data_ptr(), ws.bytes
        self.dev_index = _lib.device_index(cloud.device)
        self.f32 = dict(dtype=torch.float32, device=cloud.device)

    def forward(self, t, q, mask, occ, obs, scalars):
        fn, m = (self.L.tohip_pose_forward_bits, occ) if occ is not None else (self.L.tohip_pose_forward, mask)
        rc = _lib.on_device(self.dev_index, fn, self.blob, self.n, t.data_ptr(), q.data_ptr(), self.cam,
                            m.data_ptr() if m is not None else None, obs.data_ptr(), scalars.data_ptr(), self.ws, self.wsb)
        if rc:
            check(rc, fn.__name__)

    def forward_backward(self, t, q, mask, occ, obs, scalars, grads, gout=None):
        """grads: 8 floats, d loss / d trans at [0:3] and d loss / d quat at [4:8] (times gout when one is given)."""
        fn, m = (self.L.tohip_pose_forward_backward_bits, occ) if occ is not None else (self.L.tohip_pose_forward_backward, mask)
        gp = grads.data_ptr()
        rc = _lib.on_device(self.dev_index, fn, self.blob, self.n, t.data_ptr(), q.data_ptr(), self.cam, m.data_ptr() if m is not None else None,
                            obs.data_ptr(), scalars.data_ptr(), gout.data_ptr() if gout is not None else None, gp, gp + 16, self.ws, self.wsb)
        if rc:
            check(rc, fn.__name__)

    def backward(self, t, q, mask, occ, grad_obs=None, scalars=None, gout=None):
        """-> fresh (trans_grad (1,3), quat_grad (1,4))."""
        fn, m = (self.L.tohip_pose_backward_bits, occ) if occ is not None else (self.L.tohip_pose_backward, mask)
        tg, qg = torch.empty((1, 3), **self.f32), torch.empty((1, 4), **self.f32)
        rc = _lib.on_device(self.dev_index, fn, self.blob, self.n, t.data_ptr(), q.data_ptr(), self.cam, m.data_ptr() if m is not None else None,
                            ptr(grad_obs), ptr(scalars), ptr(gout), tg.data_ptr(), qg.data_ptr(), self.ws, self.wsb)
        if rc:
            check(rc, fn.__name__)
        return tg, qg

    def forward_backward_multi(self, t, q, B, mask, occ, obs, scalars, tg, qg):
        fn, m = (self.L.tohip_pose_forward_backward_multi_bits, occ) if occ is not None else (self.L.tohip_pose_forward_backward_multi, mask)
        rc = _lib.on_device(self.dev_index, fn, self.blob, self.n, t.data_ptr(), q.data_ptr(), B, self.cam, ptr(m), ptr(obs), ptr(scalars),
                            None, ptr(tg), ptr(qg), self.ws, self.wsb)
        if rc:
            check(rc, fn.__name__)


def pose_forward(cloud, trans, quat, cam, ws, mask=None, occ=None):
    """occ: the pose's occlusion bit row (1, npad/32) instead of a float mask (tohip_pose_forward_bits)."""
    obs = torch.empty(cloud.n, dtype=torch.float32, device=cloud.device)
    scalars = torch.zeros(4, dtype=torch.float32, device=cloud.device)
    PosePlan(cloud, cam, ws).forward(trans, quat, mask, occ if occ is None else _occ_row(cloud, occ, mask=mask), obs, scalars)
    return obs, scalars


def pose_forward_backward(cloud, trans, quat, cam, ws, mask=None, gout=None, occ=None):
    """ModelPose.forward and the backward of its fused loss in ONE pass over the cloud (tohip_pose_forward_backward).
    -> (observations (N,), scalars (4: sum, loss, -, -), trans_grad (1,3), quat_grad (1,4)); gradients are gout x d loss / d (.).
    occ: the pose's occlusion bit row instead of a float mask (tohip_pose_forward_backward_bits)."""
    f32 = dict(dtype=torch.float32, device=cloud.device)
    obs, scalars, grads = torch.empty(cloud.n, **f32), torch.empty(4, **f32), torch.empty(8, **f32)
    PosePlan(cloud, cam, ws).forward_backward(trans, quat, mask, occ if occ is None else _occ_row(cloud, occ, mask=mask), obs, scalars, grads,
                                              gout)
    return obs, scalars, grads[0:3].view(1, 3), grads[4:8].view(1, 4)


def pose_forward_backward_multi(cloud, trans, quat, cam, ws, mask=None, observations=False, grad=True, occ=None):
    """B poses of one camera over one cloud in one pass (tohip_pose_forward_backward_multi): trans (B,3), quat (B,4) contiguous f32,
    ws a PoseWorkspace(cloud, n_poses >= B).  Each pose's results are bitwise those of pose_forward_backward (grad) or pose_forward.
    -> (observations (B,N) or None, scalars (B,4: sum, loss, -, -), trans_grad (B,3) or None, quat_grad (B,4) or None);
    grad=False runs the forward-only pass (scoring candidate views).  occ: (B, npad/32) int32, each pose's own occlusion bit row
    (ops.occlusion_bits of the B poses; tohip_pose_forward_backward_multi_bits) instead of one float mask for all."""
    dev = cloud.device
    B = trans.shape[0] if trans.dim() == 2 else 0
    if B == 0 or tuple(trans.shape) != (B, 3) or tuple(quat.shape) != (B, 4):
        raise ValueError(f"trans / quat must be (B,3) / (B,4) with B > 0, got {tuple(trans.shape)} / {tuple(quat.shape)}")
    for name, t in (("trans", trans), ("quat", quat), ("mask", mask)):   # the kernels read raw f32 rows on the cloud's device
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous float32 tensor on {dev}")
    if mask is not None and tuple(mask.shape) != (cloud.n,):
        raise ValueError(f"mask must have {cloud.n} entries, got {tuple(mask.shape)}")
    if occ is not None:
        _occ_row(cloud, occ, B, mask=mask)
    if not ws.multi or ws.n_poses < B:
        raise ValueError(f"ws must be a PoseWorkspace(cloud, n_poses >= {B}) sized for the multi-pose calls (multi=True)")
    f32 = dict(dtype=torch.float32, device=dev)
    obs = torch.empty((B, cloud.n), **f32) if observations else None
    scalars = torch.empty((B, 4), **f32)
    tg = torch.empty((B, 3), **f32) if grad else None
    qg = torch.empty((B, 4), **f32) if grad else None
    PosePlan(cloud, cam, ws).forward_backward_multi(trans, quat, B, mask, occ, obs, scalars, tg, qg)
    return obs, scalars, tg, qg


def pose_backward(cloud, trans, quat, cam, ws, mask=None, grad_obs=None, scalars=None, gout=None, occ=None):
    """occ: the pose's occlusion bit row instead of a float mask (tohip_pose_backward_bits)."""
    return PosePlan(cloud, cam, ws).backward(trans, quat, mask, occ if occ is None else _occ_row(cloud, occ, mask=mask), grad_obs, scalars, gout)


def unpack_occlusion_rows(cloud, rows):
    """(W, npad/32) occlusion bit rows -> (W, N) float32 masks of zeros and ones in the CALLER'S point order (1 = not occluded): what
    the float-mask calls take for the same weights.  For tests and inspection (plain torch ops)."""
    r = rows.reshape(-1, cloud.npad // 32)
    bits = (r[:, :, None] >> torch.arange(32, dtype=torch.int32, device=r.device)) & 1
    packed = bits.reshape(r.shape[0], -1)[:, :cloud.n].to(torch.float32)
    return packed[:, cloud.inv_perm.long()].contiguous()


HPR_BATCH_POINTS = 32_000_000  # points per batched hull pass (workspace ~0.12 KB per point)


OCCLUSION_CULL_BYTES = 4 << 30  # budget for the cull stage's worst-case buffers (16 B per point and waypoint): waypoints are chunked


def occlusion_bits(cloud, points, poses, quats, cam, min_dist, max_dist, method="hpr", grid=None, skip=(1, 1)):
    """(W, npad/32) int32 occlusion bit rows for the given waypoints: the hard per-camera pipeline of
    /root/reference/src/pc_processor.py:158-187 (exact transform -> hard frustum cull -> HPR from the camera
    centre, or the z-buffer splat for method="zbuffer") turned into the bit layout the kernels read.
    The waypoints go through in chunks sized by OCCLUSION_CULL_BYTES (the cull stage sizes its outputs for the worst case).
    method="voxel": the same cull, then a line-of-sight walk from the camera to each kept point through `grid` (an OccupancyGrid;
    `skip`: see los_rows) — the cloud's own packed points, one launch, no host synchronisation."""
    if method == "voxel":
        return los_rows(cloud, poses, quats, cam, min_dist, max_dist, grid, skip)
    dev = cloud.device
    W = poses.shape[0]
    rows = torch.empty((W, cloud.npad // 32), dtype=torch.int32, device=dev)
    chunk = max(1, min(W, OCCLUSION_CULL_BYTES // (16 * max(cloud.n, 1))))
    for w0 in range(0, W, chunk):
        w1 = min(W, w0 + chunk)
        _occlusion_rows_chunk(cloud, points, poses[w0:w1].contiguous(), quats[w0:w1].contiguous(), cam, min_dist, max_dist, method,
                              rows[w0:w1])
    return rows


_SCRATCH = {}


def _scratch(device, tag, nbytes):
    """A grow-only byte buffer per (device, STREAM, purpose): the occlusion rows are rebuilt again and again over buffers of GBs
    whose sizes vary a little from call to call — allocating them anew every time cost more than the kernels (12 of 34 ms per
    rebuild at 1 M points x 128 waypoints).  Keyed by the current stream: two models rebuilding their masks on two streams do not
    share a buffer (on ONE stream the calls are ordered, and a buffer's content is dead when the call that filled it returns its
    rows).  A buffer that is outgrown is handed to the caching allocator with its stream recorded, so that work still queued on it
    finishes first.  release_scratch() gives the memory back."""
    stream = torch.cuda.current_stream(device)
    key = (str(device), stream.cuda_stream, tag)
    t = _SCRATCH.get(key)
    if t is None or t.numel() < nbytes:
        old = _SCRATCH.pop(key, None)
        if old is not None:
            old.record_stream(stream)
        t = _SCRATCH[key] = torch.empty(int(nbytes * 1.1) + 256, dtype=torch.uint8, device=device)
    return t


def release_scratch():
    _SCRATCH.clear()


def _occlusion_rows_chunk(cloud, points, poses, quats, cam, min_dist, max_dist, method, rows):
    L = _lib.lib()
    dev = cloud.device
    W = poses.shape[0]
    n = cloud.n
    # transform -> cull -> gather for all waypoints of the chunk in three launches (one host read: the counts size the hull pass);
    # for the hull pass the kept clouds are written end to end at once (r06: 128 device copies, 0.83 of a refresh's 11.1 ms, until then)
    packed = method != "zbuffer" and W <= 65535
    # ... and culled in the packed cloud's order (same points, same arithmetic per point; a hull is a property of the SET, and among
    # exact duplicates the lowest row is reported in either order: the packing sort is stable): kept indices = packed positions
    in_packed_order = packed and points.data_ptr() == cloud.points.data_ptr() and tuple(points.shape) == tuple(cloud.points.shape) and points.is_contiguous()
    if packed:
        kept_all, cat, counts, kcnt_all, seg_off_dev = cull_waypoints(_sorted_rows(cloud) if in_packed_order else points, poses, quats, cam, min_dist,
                                                                      max_dist, normalize=True, scratch=True, packed=True)
    else:
        kept_all, pts_all, counts, kcnt_all = cull_waypoints(points, poses, quats, cam, min_dist, max_dist, normalize=True, scratch=True)
    if method == "zbuffer":
        # every waypoint's z-buffer in the same three launches (chunks of as many z-buffers as 2 GB hold); visible[w, j] = 1 when
        # kept point j of waypoint w owns a pixel
        K9 = (ctypes.c_float * 9)(*[cam.c.K[i] for i in range(9)])
        width, height = int(cam.c.img_width), int(cam.c.img_height)
        wsb = L.tohip_zbuffer_batched_workspace_bytes(width, height, W)
        zws = _scratch(dev, "zbuf", wsb)
        visible = _scratch(dev, "zvis", 4 * W * max(n, 1))[:4 * W * max(n, 1)].view(torch.float32)
        seg_off = torch.arange(W, dtype=torch.int64, device=dev) * max(n, 1)
        with torch.cuda.device(dev):
            check(L.tohip_zbuffer_visible_batched(ptr(pts_all), max(n, 1), ptr(kcnt_all), W, K9, width, height, 0.03, float(min_dist), float(max_dist),
                                                  ptr(visible), ptr(zws), wsb, stream_ptr()), "tohip_zbuffer_visible_batched")
    else:
        # one batched hull pass over the waypoints' culled clouds laid end to end (several when they exceed HPR_BATCH_POINTS)
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        tot = int(offs[-1])
        visible = _scratch(dev, "hvis", 4 * max(tot, 1))[:4 * max(tot, 1)].view(torch.float32)
        if not packed:
            cat = _scratch(dev, "hcat", 12 * max(tot, 1))[:12 * max(tot, 1)].view(torch.float32).view(-1, 3)
            for w in range(W):   # (device-to-device copies of each waypoint's kept rows: no host round trip)
                if counts[w]:
                    cat[int(offs[w]):int(offs[w + 1])].copy_(pts_all[w, :counts[w]])
        w0 = 0
        while w0 < W:
            w1 = w0 + 1
            while w1 < W and offs[w1 + 1] - offs[w0] <= HPR_BATCH_POINTS:
                w1 += 1
            lo, hi = int(offs[w0]), int(offs[w1])
            if hi > lo:
                status = _hpr_batched_mask(cat[lo:hi], [int(o) - lo for o in offs[w0:w1 + 1]], visible[lo:hi])
                st_h = status.cpu().numpy()   # (one host read for both checks)
                if (st_h == 3).any():
                    raise ValueError("Points cannot contain NaN")  # scipy's error in the reference's pipeline
                if ((st_h == 2) & (np.asarray(counts[w0:w1]) >= 4)).any():
                    raise _lib.HipError("occlusion_bits: a waypoint's culled cloud is flat (no 3-D hull; Qhull raises QH6154)")
            w0 = w1
        seg_off = seg_off_dev[:W] if packed else torch.from_numpy(offs[:W].copy()).to(dev)
    for w0 in range(0, W, 65535):
        w1 = min(W, w0 + 65535)
        with torch.cuda.device(dev):
            check(L.tohip_occlusion_rows_masked(n, None if in_packed_order else ptr(cloud.inv_perm), ptr(kept_all[w0:w1]), ptr(kcnt_all[w0:w1]), ptr(visible),
                                                ptr(seg_off[w0:w1]), 4, w1 - w0, ptr(rows[w0:w1]), stream_ptr()), "tohip_occlusion_rows_masked")


def _hpr_batched_mask(points, seg_offsets, mask_out):
    """tohip_hidden_pts_removal_batched for its mask only (mask_out: n_total f32, 1 = visible), over cached scratch -> status (B,) int32."""
    n, dev = points.shape[0], points.device
    B = len(seg_offsets) - 1
    idx = _scratch(dev, "hidx", 4 * max(n, 1))[:4 * max(n, 1)].view(torch.int32)
    voff = torch.empty(B + 1, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    _hpr_batched(points, seg_offsets, 2.0, idx, voff, mask_out, status, scratch=True)
    return status


def cull_waypoints(points, poses, quats, cam, min_dist, max_dist, normalize=True, scratch=False, packed=False):
    """Exact transform + hard frustum cull of `points` (N,3) for W poses at once (tohip_cull_waypoints).
    -> (kept_idx (W,N) int32, kept_pts (W,N,3) f32 camera frame, counts list[int], counts on the device (W,) int32): pose
    w's kept points are the first counts[w] rows of kept_idx[w] / kept_pts[w], in input order.  One host synchronisation
    (the counts).  scratch: the two worst-case sized outputs live in cached buffers (valid until the next such call).
    packed (tohip_cull_waypoints_packed; W <= 65535): kept_pts is (sum(counts), 3) instead — the poses' kept points end to end,
    pose w's in rows [offs[w], offs[w+1]) — and a fifth value, offs (W+1,) int64 on the device, is returned."""
    _require_cuda(points, "points")
    pts = points.detach().to(torch.float32).contiguous()
    dev, n, W = pts.device, pts.shape[0], poses.shape[0]
    p_in, q_in = poses.detach().to(torch.float32).contiguous(), quats.detach().to(torch.float32).contiguous()
    if packed and W > 65535:
        raise ValueError("cull_waypoints(packed=True) takes at most 65535 poses per call")
    if scratch:
        kept_all = _scratch(dev, "kept", 4 * W * max(n, 1))[:4 * W * max(n, 1)].view(torch.int32).view(W, max(n, 1))
        pts_all = _scratch(dev, "kpts", 12 * W * max(n, 1))[:12 * W * max(n, 1)].view(torch.float32).view(W, max(n, 1), 3)
    else:
        kept_all = torch.empty((W, max(n, 1)), dtype=torch.int32, device=dev)
        pts_all = torch.empty((W, max(n, 1), 3), dtype=torch.float32, device=dev)
    kcnt_all = torch.zeros(W, dtype=torch.int32, device=dev)
    L = _lib.lib()
    if packed:
        seg_off = torch.empty(W + 1, dtype=torch.int64, device=dev)
        wsb = L.tohip_cull_waypoints_workspace_bytes(n, W)
        fws = _scratch(dev, "cullws", wsb) if scratch else torch.empty(wsb, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(L.tohip_cull_waypoints_packed(ptr(pts), n, ptr(p_in), ptr(q_in), W, int(bool(normalize)), cam.ref(), float(min_dist),
                                                float(max_dist), ptr(kept_all), ptr(pts_all), ptr(kcnt_all), ptr(seg_off), ptr(fws), wsb,
                                                stream_ptr()), "tohip_cull_waypoints_packed")
        counts = kcnt_all.cpu().tolist()
        return kept_all, pts_all.view(-1, 3)[:sum(counts)], counts, kcnt_all, seg_off
    for w0 in range(0, W, 65535):  # grid.y limit
        w1 = min(W, w0 + 65535)
        wsb = L.tohip_cull_waypoints_workspace_bytes(n, w1 - w0)
        fws = _scratch(dev, "cullws", wsb) if scratch else torch.empty(wsb, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(L.tohip_cull_waypoints(ptr(pts), n, ptr(p_in[w0:w1]), ptr(q_in[w0:w1]), w1 - w0, int(bool(normalize)), cam.ref(),
                                         float(min_dist), float(max_dist), ptr(kept_all[w0:w1]), ptr(pts_all[w0:w1]),
                                         ptr(kcnt_all[w0:w1]), ptr(fws), wsb, stream_ptr()), "tohip_cull_waypoints")
    return kept_all, pts_all, kcnt_all.cpu().tolist(), kcnt_all


def to_camera_frame_exact(points, quat, trans, normalize=True, transpose=False):
    """Reference-exact f32 transform; (N,3) -> (N,3), or (3,N) when `transpose`."""
    _require_cuda(points, "points")
    pts = points.detach().to(torch.float32).contiguous()
    n = pts.shape[0]
    q = _dev_f32(quat, pts.device).reshape(4)
    t = _dev_f32(trans, pts.device).reshape(3)
    out = torch.empty((3, n) if transpose else (n, 3), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        check(_lib.lib().tohip_to_camera_frame(ptr(pts), n, ptr(q), ptr(t), int(normalize), int(transpose), ptr(out),
                                               stream_ptr()), "tohip_to_camera_frame")
    return out


def soft_masks(cam_points, cam, want_dist=True, want_fov=True):
    _require_cuda(cam_points, "points")
    pts = cam_points.detach().to(torch.float32).contiguous()
    n = pts.shape[0]
    d = torch.empty(n, dtype=torch.float32, device=pts.device) if want_dist else None
    f = torch.empty(n, dtype=torch.float32, device=pts.device) if want_fov else None
    with torch.cuda.device(pts.device):
        check(_lib.lib().tohip_soft_masks(ptr(pts), n, cam.ref(), ptr(d), ptr(f), stream_ptr()), "tohip_soft_masks")
    return d, f


def soft_masks_backward(cam_points, cam, grad_dist=None, grad_fov=None):
    """dL/d cam_points (N,3) for upstream gradients of get_dist_mask and / or the soft get_fov_mask."""
    pts = cam_points.detach().to(torch.float32).contiguous()
    n = pts.shape[0]
    out = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    gd = grad_dist.to(torch.float32).contiguous() if grad_dist is not None else None
    gf = grad_fov.to(torch.float32).contiguous() if grad_fov is not None else None
    with torch.cuda.device(pts.device):
        check(_lib.lib().tohip_soft_masks_backward(ptr(pts), n, cam.ref(), ptr(gd), ptr(gf), ptr(out), stream_ptr()),
              "tohip_soft_masks_backward")
    return out


def to_camera_frame_backward(points, quat, trans, grad_out, want_points_grad=True):
    """-> (dL/d points (N,3) or None, dL/d quat (4,) raw quaternion, dL/d trans (3,))"""
    pts = points.detach().to(torch.float32).contiguous()
    n, dev = pts.shape[0], pts.device
    q = _dev_f32(quat, dev).reshape(4)
    t = _dev_f32(trans, dev).reshape(3)
    g = grad_out.to(torch.float32).contiguous()
    gx = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_points_grad else None
    gq = torch.empty(4, dtype=torch.float32, device=dev)
    gt = torch.empty(3, dtype=torch.float32, device=dev)
    L = _lib.lib()
    wsb = L.tohip_pose_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.tohip_to_camera_frame_backward(ptr(pts), n, ptr(q), ptr(t), ptr(g), ptr(gx), ptr(gq), ptr(gt), ptr(ws), wsb, stream_ptr()),
              "tohip_to_camera_frame_backward")
    return gx, gq, gt


def frustum_cull(cam_3xN, cam, min_dist, max_dist, want_indices=True):
    """-> (dist_mask bool[N], fov_mask bool[N], kept_idx int32[M] ascending)"""
    _require_cuda(cam_3xN, "points")
    pts = cam_3xN.detach().to(torch.float32).contiguous()
    n = pts.shape[1]
    dev = pts.device
    dm = torch.empty(n, dtype=torch.uint8, device=dev)
    fm = torch.empty(n, dtype=torch.uint8, device=dev)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    wsb = _lib.lib().tohip_frustum_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().tohip_frustum_cull(ptr(pts), n, cam.ref(), float(min_dist), float(max_dist), ptr(dm), ptr(fm),
                                            ptr(idx) if want_indices else None, ptr(cnt), ptr(ws), wsb, stream_ptr()),
              "tohip_frustum_cull")
    m = int(cnt.item()) if want_indices else 0
    return dm.bool(), fm.bool(), idx[:m]


def spherical_flip(points, param=2):
    _require_cuda(points, "points")
    pts = points.detach().to(torch.float32).contiguous()
    n = pts.shape[0]
    out = torch.empty_like(pts)
    rad = torch.empty(1, dtype=torch.float32, device=pts.device)
    ws = torch.empty(_lib.CONSTANTS["TOHIP_FLIP_WORKSPACE_BYTES"], dtype=torch.uint8, device=pts.device)
    with torch.cuda.device(pts.device):
        check(_lib.lib().tohip_spherical_flip(ptr(pts), n, float(param), ptr(out), ptr(rad), ptr(ws), ws.numel(), stream_ptr()),
              "tohip_spherical_flip")
    return out, rad


def _with_hull_workspace(wsb, dev, call, scratch=False):
    """Run call(ws) over a hull workspace of the recommended wsb bytes — a fresh tensor, or (scratch) the cached _scratch buffer of at
    least that many (call passes ws.numel() as its size); a cloud whose hull needs more faces than that holds (TOHIP_ENOSPC: most of
    its points are hull vertices) is retried with 4x the bytes — every extra byte goes to faces."""
    for _ in range(4):
        ws = _scratch(dev, "hull", wsb) if scratch else torch.empty(wsb, dtype=torch.uint8, device=dev)
        try:
            return call(ws)
        except _lib.HipError as e:
            if e.code != _lib.ENOSPC:
                raise
            del ws
            wsb *= 4
    raise _lib.HipError("hull workspace: still out of face capacity at 64x the recommended size")


def hidden_pts_removal(points, param=2):
    """-> (visible_idx int32[V] ascending, mask f32[N])"""
    _require_cuda(points, "points")
    pts = points.detach().to(torch.float32).contiguous()
    n = pts.shape[0]
    dev = pts.device
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    mask = torch.empty(n, dtype=torch.float32, device=dev)
    def call(ws):
        with torch.cuda.device(dev):
            check(_lib.lib().tohip_hidden_pts_removal(ptr(pts), n, float(param), ptr(idx), ptr(cnt), ptr(mask), ptr(ws), ws.numel(),
                                                      stream_ptr()), "tohip_hidden_pts_removal")
    _with_hull_workspace(_lib.lib().tohip_hpr_workspace_bytes(n), dev, call)
    return idx[:int(cnt.item())], mask


def _hpr_batched(points, seg_offsets, param, idx, voff, mask, status, scratch=False):
    """tohip_hidden_pts_removal_batched of the segments `seg_offsets` (B+1 host ints) of `points` into the given outputs, with the hull
    workspace's retry rule (scratch: over the cached buffer)."""
    L, dev, B = _lib.lib(), points.device, len(seg_offsets) - 1
    c_offs = (ctypes.c_int64 * (B + 1))(*[int(o) for o in seg_offsets])

    def call(ws):
        with torch.cuda.device(dev):
            check(L.tohip_hidden_pts_removal_batched(ptr(points), c_offs, B, float(param), ptr(idx), ptr(voff), ptr(mask), ptr(status), ptr(ws),
                                                     ws.numel(), stream_ptr()), "tohip_hidden_pts_removal_batched")
    _with_hull_workspace(L.tohip_hpr_batched_workspace_bytes(points.shape[0], B), dev, call, scratch)


def hidden_pts_removal_batched(points, seg_offsets, param=2):
    """HPR of several independent clouds in one pass (one viewpoint = the origin of each): `points` (n_total,3)
    holds the segments end to end, `seg_offsets` (B+1 ints, host) their row ranges.
    -> (visible_idx int32 (rows of `points`, ascending), seg_visible_offsets int64 (B+1, host), mask f32[n_total],
        status int32[B] (0 ok, 1 fewer than 4 points, 2 flat, 3 NaN coordinates))"""
    _require_cuda(points, "points")
    pts = points.detach().to(torch.float32).contiguous()
    n, dev = pts.shape[0], pts.device
    offs = [int(o) for o in seg_offsets]
    B = len(offs) - 1
    if B < 1 or offs[0] != 0 or offs[-1] != n:
        raise ValueError("seg_offsets must run from 0 to len(points)")
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    voff = torch.empty(B + 1, dtype=torch.int32, device=dev)
    mask = torch.empty(n, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    _hpr_batched(pts, offs, param, idx, voff, mask, status)
    voff_h = voff.cpu().to(torch.int64)
    return idx[:int(voff_h[-1])], voff_h, mask, status


def hull_vertices_with_origin(points, with_origin=True, return_rounds=False):
    """Ascending hull-vertex indices of points (n,3) [+ the origin as index n] (tools.py:56-64)."""
    _require_cuda(points, "points")
    pts = points.detach().to(torch.float32).contiguous()
    n = pts.shape[0]
    dev = pts.device
    idx = torch.empty(n + 1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    rounds = ctypes.c_int32(0)
    def call(ws):
        with torch.cuda.device(dev):
            check(_lib.lib().tohip_convex_hull_vertices(ptr(pts), n, int(with_origin), ptr(idx), ptr(cnt),
                                                        ctypes.byref(rounds), ptr(ws), ws.numel(), stream_ptr()),
                  "tohip_convex_hull_vertices")
    _with_hull_workspace(_lib.lib().tohip_hpr_workspace_bytes(n), dev, call)
    out = idx[:int(cnt.item())]
    return (out, rounds.value) if return_rounds else out


def render_points(verts, K, height, width, radius=0.03, znear=1.0, zfar=10.0, background=1.0, want_owner=False):
    """-> (image (H,W,3) f32, owner (H,W) int32 or None, owns_pixel (n,) bool)"""
    _require_cuda(verts, "verts")
    v = verts.detach().to(torch.float32).contiguous()
    n = v.shape[0]
    dev = v.device
    H, W = int(height), int(width)
    Kh = torch.as_tensor(K, dtype=torch.float32).detach().cpu()[:3, :3].reshape(9).tolist()
    Kc = (ctypes.c_float * 9)(*Kh)
    img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    owner = torch.empty((H, W), dtype=torch.int32, device=dev) if want_owner else None
    owns = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    wsb = _lib.lib().tohip_render_workspace_bytes(W, H)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().tohip_render_points(ptr(v), n, Kc, W, H, float(radius), float(znear), float(zfar), float(background),
                                             ptr(img), ptr(owner), ptr(owns), ptr(ws), wsb, stream_ptr()), "tohip_render_points")
    return img, owner, owns[:n].bool()


def render_points_blend(verts, K, height, width, radius=0.03, znear=1.0, zfar=10.0, gamma=0.1, background=1.0):
    """-> image (H,W,3) f32: the depth-weighted blend of every disc over each pixel (render_kernels.hip; `gamma` = pulsar's softness)."""
    _require_cuda(verts, "verts")
    v = verts.detach().to(torch.float32).contiguous()
    dev = v.device
    H, W = int(height), int(width)
    Kh = torch.as_tensor(K, dtype=torch.float32).detach().cpu()[:3, :3].reshape(9).tolist()
    Kc = (ctypes.c_float * 9)(*Kh)
    img = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    wsb = _lib.lib().tohip_render_blend_workspace_bytes(W, H)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().tohip_render_points_blend(ptr(v), v.shape[0], Kc, W, H, float(radius), float(znear), float(zfar), float(gamma),
                                                   float(background), ptr(img), ptr(ws), wsb, stream_ptr()), "tohip_render_points_blend")
    return img


def selftest_wave_reduce(mat64xk):
    k = mat64xk.shape[1]
    dev = mat64xk.device
    s, mn, mx = (torch.empty(k, dtype=torch.float32, device=dev) for _ in range(3))
    with torch.cuda.device(dev):
        check(_lib.lib().tohip_selftest_wave_reduce(ptr(mat64xk.contiguous()), k, ptr(s), ptr(mn), ptr(mx), stream_ptr()),
              "tohip_selftest_wave_reduce")
    return s, mn, mx


# ---- the particle filter: Monte Carlo localisation on the evidence map (particle_kernels.hip, DESIGN.md 10 "Particle filter") -------
MCL_MAX_N = 1 << 20
MCL_TURN = 16384                   # heading units a turn
MCL_CLAMP = (1 << 24) - 1          # |X|, |Y|, |Z| of a state, 1/256 voxel
MCL_MAX_SIGMA = 65536.0            # state units: sigma_q8 = round(256 sigma) <= 2^24
MCL_RECORD = _lib.CONSTANTS["TOHIP_MCL_RECORD"]
MCL_RECORD_FIELDS = ("s1", "s2", "sum_x", "sum_y", "sum_z", "sum_cos", "sum_sin", "best", "best_score", "best_known", "best_used", "verdict",
                     "n_eff_bits", "max_log_weight", "n", "zero")
_MCL_TABLES = {}


def particle_tables():
    """The filter's three tables as the one int32 array the kernels take (TOHIP_MCL_TABLE_WORDS), built once on the host in f64 and
    rounded once: TRIG[h] = round(32768 cos), round(32768 sin) of 2 pi h / 16384 at words 2 h, 2 h + 1; GAUSS[i] = round(4096
    Phi^-1((i + 0.5) / 1025)), i = 0 .. 1024, at TOHIP_MCL_GAUSS_WORD; EXP2[j] = round(2^20 2^(-j / 256)), j = 0 .. 255, at
    TOHIP_MCL_EXP2_WORD (synth.mcl_table_words_ref restates them)."""
    if "words" not in _MCL_TABLES:
        from statistics import NormalDist
        C = _lib.CONSTANTS
        words = np.zeros(C["TOHIP_MCL_TABLE_WORDS"], dtype=np.int32)
        a = 2.0 * np.pi * np.arange(MCL_TURN, dtype=np.float64) / MCL_TURN
        words[0:2 * MCL_TURN:2], words[1:2 * MCL_TURN:2] = np.rint(32768.0 * np.cos(a)), np.rint(32768.0 * np.sin(a))
        nd = NormalDist()
        words[C["TOHIP_MCL_GAUSS_WORD"]:C["TOHIP_MCL_GAUSS_WORD"] + 1025] = [round(4096.0 * nd.inv_cdf((i + 0.5) / 1025.0)) for i in range(1025)]
        words[C["TOHIP_MCL_EXP2_WORD"]:C["TOHIP_MCL_EXP2_WORD"] + 256] = np.rint(2.0 ** 20 * 2.0 ** (-np.arange(256, dtype=np.float64) / 256.0))
        _MCL_TABLES["words"] = words
    return _MCL_TABLES["words"]


def _mcl_four(v, name, scale):
    """Four host numbers (x, y, z, heading) -> four f64 in state units: `scale` = (per position unit, per heading unit)."""
    a = _host_rows(v, 4, name, rows=1)[0]
    return np.array([a[0] * scale[0], a[1] * scale[0], a[2] * scale[0], a[3] * scale[1]], dtype=np.float64)


def check_particles(map_or_matcher, n=1, seed=0, beta_q=256, floor=None, unknown_value=0, sigma=None, delta=None, ratio=None, attitude=None,
                    units="metric"):
    """A particle filter's settings and a step's arguments, by name; needs no GPU.  map_or_matcher: an ops.EvidenceMap, or an
    ops.ScanMatcher (floor and unknown_value are then the matcher's and must be left at their defaults); n: an integer in [1, 2^20];
    seed: an integer in [0, 2^64); beta_q: an integer in [1, 65536], Q16 halvings of weight per score unit; floor, unknown_value:
    check_scan_match's.  sigma (None: not asked): four numbers >= 0 (x, y, z, heading), at most 65536 state units each; delta (None:
    not asked): four numbers, at most 2^24 - 1 state units each in size; units 'metric' (metres and radians) or 'state' (1/256 voxel
    and 1/16384 turn); ratio (None: not asked): a number in [0, 1]; attitude (None: the identity): nine finite numbers, a (3,3)
    rotation.  -> dict(map, floor, unknown_value, n, seed, beta_q, sigma_q8, delta, ratio, attitude): sigma_q8 four ints round(256
    sigma), delta four ints, attitude a (9,) f32 array or None; ValueError otherwise."""
    if isinstance(map_or_matcher, ScanMatcher):
        if floor is not None or not (_is_int(unknown_value) and unknown_value == 0):
            raise ValueError(f"ParticleFilter: floor and unknown_value belong to the ScanMatcher that was given (floor {map_or_matcher.floor}, "
                             f"unknown_value {map_or_matcher.unknown_value}); leave them at their defaults, got {floor!r} and {unknown_value!r}")
        map, fl, unk = map_or_matcher.map, map_or_matcher.floor, map_or_matcher.unknown_value
    else:
        map = map_or_matcher
        if not isinstance(map, EvidenceMap):
            raise ValueError("ParticleFilter: the map must be an ops.EvidenceMap or an ops.ScanMatcher (EvidenceMap.from_space takes a SpaceMap), "
                             f"got {type(map).__name__}")
        fl, unk, _ = check_scan_match(map, floor, unknown_value)
    if not _is_int(n) or not 1 <= n <= MCL_MAX_N:
        raise ValueError(f"n must be an integer in [1, 2^20] particles, got {n!r}")
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    if not _is_int(beta_q) or not 1 <= beta_q <= 65536:
        raise ValueError(f"beta_q must be an integer in [1, 65536] (Q16 halvings per score unit), got {beta_q!r}")
    if units not in ("metric", "state"):
        raise ValueError(f"units must be 'metric' (metres, radians) or 'state' (1/256 voxel, 1/16384 turn), got {units!r}")
    scale = (256.0 / float(map.resolution), MCL_TURN / (2.0 * np.pi)) if units == "metric" else (1.0, 1.0)
    sigma_q8 = None
    if sigma is not None:
        s = _mcl_four(sigma, "sigma", scale)
        if (s < 0.0).any() or (s > MCL_MAX_SIGMA).any():
            raise ValueError(f"sigma must be four numbers >= 0 (x, y, z, heading) of at most 65536 state units, got {s.tolist()} state units")
        sigma_q8 = [int(v) for v in np.rint(256.0 * s)]
    if delta is not None:
        d = np.rint(_mcl_four(delta, "delta", scale))
        if (np.abs(d) > MCL_CLAMP).any():
            raise ValueError(f"delta must be four numbers (x, y, z, heading) of at most 2^24 - 1 state units in size, got {d.tolist()} state units")
        delta = [int(v) for v in d]
    if ratio is not None:
        try:
            ratio = float(ratio)
        except (TypeError, ValueError):
            ratio = float("nan")
        if not 0.0 <= ratio <= 1.0:
            raise ValueError(f"ratio must be a number in [0, 1] (resample where n_eff < ratio n), got {ratio!r}")
    if attitude is not None:
        try:
            a = np.asarray(attitude.detach().cpu().numpy() if torch.is_tensor(attitude) else attitude, dtype=np.float64)
        except (TypeError, ValueError):
            a = np.zeros(0)
        if a.shape not in ((3, 3), (9,)) or not np.isfinite(a).all():
            raise ValueError(f"attitude must be nine finite numbers, a (3,3) rotation, got {a.shape if a.size else type(attitude).__name__}")
        attitude = a.reshape(9).astype(np.float32)
    return dict(map=map, floor=fl, unknown_value=unk, n=int(n), seed=int(seed), beta_q=int(beta_q), sigma_q8=sigma_q8, delta=delta, ratio=ratio,
                attitude=attitude)


ParticleEstimate = collections.namedtuple("ParticleEstimate", "pose yaw quat best_pose best_yaw best_index best_score known used n_eff resampled "
                                                              "state record")
ParticleEstimate.__doc__ = """ParticleFilter.estimate(): pose (3,) f64, the weighted mean position in the world (origin + resolution
(sum w X / S1) / 256); yaw, the weighted mean heading in radians (atan2 of sum w sin, sum w cos); quat (4,) wxyz of that heading;
best_pose, best_yaw, best_index, best_score: the particle with the largest weight (the lowest index among equals) and scan matching's
score of the last scan there; known, used: of its points, those that met an observed voxel and those in range; n_eff =
S1^2 / S2; resampled: the last verdict; state (4,) f64, the mean in state units; record: the device record's 16 integers
(MCL_RECORD_FIELDS)."""


class ParticleFilter:
    """Monte Carlo localisation on an evidence map (particle_kernels.hip, DESIGN.md 10 "Particle filter"): n pose hypotheses carried
    from scan to scan.  predict() moves them by odometry plus noise, weigh() multiplies each weight by 2^(score beta_q / 65536) with
    scan matching's score of the scan at the particle's pose, resample() draws a new generation where the weights have collapsed,
    estimate() reads the answer.  The state lives on the device — .state (n,4) int32: x, y, z in 1/256 voxel from the map's origin
    and a heading in 1/16384 turn about world z; .log_weight (n,) int64 in 1/65536 halvings — noise comes from Philox4x32-10 keyed by
    `seed`, and every step is integer arithmetic: the same bits in every run, and synth.mcl_*_ref's bit for bit.  Only estimate()
    reads anything back.  Roll and pitch are the caller's (`attitude`); the map's bytes are read as they are at each weigh() (no
    refresh() is needed after an integrate)."""

    def __init__(self, map_or_matcher, n, seed=0, beta_q=256, floor=None, unknown_value=0):
        c = check_particles(map_or_matcher, n, seed, beta_q, floor, unknown_value)
        self.map, self.floor, self.unknown_value, self.n, self.seed, self.beta_q = (c[k] for k in ("map", "floor", "unknown_value", "n", "seed",
                                                                                                    "beta_q"))
        m = self.map
        self.origin, self.resolution, self.dims, self.device, self.geom = m.origin, m.resolution, m.dims, m.device, m.geom
        self.step = 0
        self.ratio = 0.5
        dev, n = self.device, self.n
        self.tables = torch.from_numpy(particle_tables()).to(dev)
        self._states = [torch.empty((n, 4), dtype=torch.int32, device=dev) for _ in range(2)]
        self.log_weight = torch.empty(n, dtype=torch.int64, device=dev)
        self._weights = torch.empty(n, dtype=torch.int64, device=dev)
        self._cumulative = torch.empty(n, dtype=torch.int64, device=dev)
        self.ancestors = torch.empty(n, dtype=torch.int32, device=dev)
        self.record = torch.empty(MCL_RECORD, dtype=torch.int64, device=dev)
        self.scores = torch.empty((3, n), dtype=torch.int32, device=dev)   # score, used, known of the last weigh()
        self._workspace = torch.empty(_lib.CONSTANTS["TOHIP_MCL_WORKSPACE_BYTES"], dtype=torch.uint8, device=dev)
        self._seeded = self._weighed = False

    @property
    def state(self):
        return self._states[0]

    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            check(fn(*args, stream_ptr(), 0), fn.__name__)

    def _key(self):
        return self.seed & 0xFFFFFFFF, self.seed >> 32, self.step

    def _tables(self):
        return ptr(self.tables), self.tables.numel() * 4

    @staticmethod
    def _four(v):
        return (ctypes.c_int32 * 4)(*v)

    def _attitude(self, attitude):
        a = check_particles(self.map, attitude=attitude)["attitude"]
        return None if a is None else (ctypes.c_float * 9)(*a.tolist())

    def _need(self, what, seeded=True, weighed=False):
        if seeded and not self._seeded:
            raise ValueError(f"ParticleFilter.{what}: seed the filter first (seed_gaussian or seed_positions)")
        if weighed and not self._weighed:
            raise ValueError(f"ParticleFilter.{what}: weigh a scan first (weigh)")

    def state_units(self, pose, yaw):
        """A world position (3,) and a heading in radians -> the four state integers (f64, rounded once)."""
        p = np.rint(256.0 * (_host_rows(pose, 3, "pose", rows=1)[0] - np.asarray(self.origin, dtype=np.float64)) / float(self.resolution))
        if (np.abs(p) > MCL_CLAMP).any():
            raise ValueError(f"pose lies beyond 2^24 - 1 state units of the map's origin: {p.tolist()}")
        return [int(v) for v in p] + [int(round(MCL_TURN * float(yaw) / (2.0 * np.pi))) % MCL_TURN]

    def seed_gaussian(self, pose, yaw, sigma_xyz, sigma_yaw, units="metric"):
        """Particles around a prior: pose (3,) in the world and yaw in radians (units='state': four state integers as `pose`, yaw
        None), sigma_xyz one number or three and sigma_yaw, in metres and radians or in state units.  Every log-weight 0.  One
        launch, nothing read back.  -> self."""
        sx = np.broadcast_to(np.asarray(sigma_xyz, dtype=np.float64).reshape(-1), (3,))
        c = check_particles(self.map, sigma=[sx[0], sx[1], sx[2], sigma_yaw], units=units)
        if units == "state":
            prior = [int(v) for v in _host_rows(pose, 4, "pose", rows=1)[0]]
            if any(abs(v) > MCL_CLAMP for v in prior[:3]):
                raise ValueError(f"pose lies beyond 2^24 - 1 state units of the map's origin: {prior}")
            prior[3] %= MCL_TURN
        else:
            prior = self.state_units(pose, yaw)
        self._call(_lib.lib().tohip_mcl_seed_gaussian, ptr(self.state), ptr(self.log_weight), self.n, *self._tables(), self._four(prior),
                   self._four(c["sigma_q8"]), *self._key())
        self._seeded, self._weighed = True, False
        return self

    def seed_positions(self, positions, jitter=True):
        """A global start: particle i takes row (word0 mod M) of positions (M,3), floating point on the map's device — m.free.export(),
        a field's free_nodes, known-free voxel centres — lands uniformly inside that row's voxel (jitter=False: at its centre) and
        takes a uniform heading.  Every log-weight 0.  One launch, nothing read back.  -> self."""
        if isinstance(positions, tuple) and len(positions) == 2:   # (ijk, centres): what OccupancyGrid.export() returns
            positions = positions[1]
        pts = covmap_points(positions, self.device, "ParticleFilter.seed_positions")
        if not 1 <= pts.shape[0] < 1 << 31:
            raise ValueError(f"ParticleFilter.seed_positions: 1 .. 2^31 - 1 positions, got {pts.shape[0]}")
        self._call(_lib.lib().tohip_mcl_seed_positions, ptr(self.state), ptr(self.log_weight), self.n, ctypes.byref(self.geom), ptr(pts), pts.shape[0],
                   1 if jitter else 0, *self._key())
        self._seeded, self._weighed = True, False
        return self

    def predict(self, delta, sigma, units="metric"):
        """The motion update: delta = (dx, dy, dz, dyaw), the odometry in the BODY frame, and sigma, four standard deviations of the
        noise each particle adds to it; metres and radians, or state units.  The step counter advances first: every predict draws
        fresh noise.  One launch, nothing read back.  -> self."""
        self._need("predict")
        c = check_particles(self.map, sigma=sigma, delta=delta, units=units)
        self.step = (self.step + 1) & 0xFFFFFFFF
        self._call(_lib.lib().tohip_mcl_predict, ptr(self.state), self.n, *self._tables(), self._four(c["delta"]), self._four(c["sigma_q8"]), *self._key())
        return self

    def poses12(self, attitude=None):
        """-> (n,12) f32 on the device: scan matching's pose of every particle, R = Rz(heading) A row-major, then t — what
        ScanMatcher.score and correlate take as poses12=.  attitude: A, a (3,3) rotation (an IMU's roll and pitch); None: the
        identity.  One launch."""
        self._need("poses12")
        out = torch.empty((self.n, 12), dtype=torch.float32, device=self.device)
        self._call(_lib.lib().tohip_mcl_poses, ptr(self.state), self.n, *self._tables(), ctypes.byref(self.geom), self._attitude(attitude), ptr(out))
        return out

    def weigh(self, points, attitude=None, ratio=None):
        """The measurement update with one scan, points (P,3) in the SENSOR frame on the map's device, 1 <= P <= 2^22: every
        particle's log-weight gains beta_q times scan matching's score of the scan at its pose; then the largest is subtracted, the
        weights and their sums are formed and the record is written, with the verdict n_eff < ratio n; ratio None: self.ratio, what the
        last weigh() or resample() was given (0.5 at first), otherwise it becomes self.ratio.  .scores holds (score, used,
        known) per particle.  At most three clears and four launches, nothing read back.  -> self."""
        self._need("weigh")
        if ratio is not None:
            self.ratio = check_particles(self.map, ratio=ratio)["ratio"]
        pts = covmap_points(points, self.device, "ParticleFilter.weigh")
        if not 1 <= pts.shape[0] <= SCAN_MAX_POINTS:
            raise ValueError(f"ParticleFilter.weigh: the scan must hold 1 .. 2^22 points, got {pts.shape[0]}")
        sc = self.scores
        self._call(_lib.lib().tohip_mcl_weigh, *self.map._sizes(), self.floor, self.unknown_value, ptr(pts), pts.shape[0], ptr(self.state), self.n,
                   *self._tables(), self._attitude(attitude), ptr(sc[0]), ptr(sc[1]), ptr(sc[2]))
        return self._weights_call(sc)

    def _weights_call(self, sc=None):
        none = ctypes.c_void_p(0)
        self._call(_lib.lib().tohip_mcl_weights, ptr(self.state), ptr(self.log_weight), self.n, *self._tables(),
                   *((ptr(sc[0]), ptr(sc[1]), ptr(sc[2])) if sc is not None else (none, none, none)), self.beta_q, self.ratio * self.n,
                   ptr(self._weights), ptr(self.record), ptr(self._workspace), self._workspace.numel())
        self._best_row = self.state.index_select(0, self.record[7:8])   # (a device gather: the state moves on, the record does not)
        self._weighed = True
        return self

    def normalise(self, ratio=None):
        """The weights, their sums and the record from .log_weight as it stands, with no scan: after the caller wrote log-weights
        of its own; ratio as in weigh().  Three launches.  -> self."""
        self._need("normalise")
        if ratio is not None:
            self.ratio = check_particles(self.map, ratio=ratio)["ratio"]
        return self._weights_call(None)

    def weights(self):
        """-> (n,) int64 on the device: the integer weights of the last weigh(), at most 2^20 each (the largest is exactly 2^20)."""
        self._need("weights", weighed=True)
        return self._weights

    def resample(self, ratio=0.5):
        """Systematic resampling, decided on the device: where n_eff = S1^2 / S2 < ratio n, generation j descends from the least i
        with C_i > (j S1 + r) div n and every log-weight becomes 0; otherwise nothing changes.  .ancestors (n,) int32 names each
        particle's parent (the identity where nothing changed).  The state is double-buffered: .state is the new tensor.  Four
        launches, nothing read back.  -> self."""
        self._need("resample", weighed=True)
        self.ratio = check_particles(self.map, ratio=ratio)["ratio"]
        self._call(_lib.lib().tohip_mcl_resample_systematic, ptr(self._states[0]), ptr(self._states[1]), ptr(self.log_weight), self.n, ptr(self._weights),
                   ptr(self.record), self.ratio * self.n, ptr(self._cumulative), ptr(self.ancestors), ptr(self._workspace),
                   self._workspace.numel(), *self._key())
        self._states.reverse()
        return self

    def estimate(self):
        """The answer after a weigh(): one read-back — the record and the best particle's row — -> ParticleEstimate.  The means are
        formed on the host in f64 from the record's integer sums; they describe the weights of the last weigh(), also after a
        resample() (whose equal weights would say the same up to its sampling)."""
        self._need("estimate", weighed=True)
        return _particle_estimate(self, torch.cat([self.record, self._best_row.reshape(-1).to(torch.int64)]).cpu().numpy())

    def spread(self):
        """-> (std (3,) f64 tensor, metres; circular std of the heading, radians, a 0-d f64 tensor) on the device: the weighted
        spread of the particles as they are now, by torch ops in f64 from .log_weight and .state.  No bit promise: the reductions'
        order is torch's."""
        self._need("spread")
        w = torch.exp2(self.log_weight.to(torch.float64) / 65536.0)
        w = w / w.sum()
        x = self.state[:, :3].to(torch.float64) * (float(self.resolution) / 256.0)
        mean = (w[:, None] * x).sum(dim=0)
        std = torch.sqrt((w[:, None] * (x - mean) ** 2).sum(dim=0))
        a = self.state[:, 3].to(torch.float64) * (2.0 * np.pi / MCL_TURN)
        R = torch.sqrt((w * torch.cos(a)).sum() ** 2 + (w * torch.sin(a)).sum() ** 2).clamp(1e-300, 1.0)
        return std, torch.sqrt(-2.0 * torch.log(R))


def _particle_estimate(pf, host):
    rec = dict(zip(MCL_RECORD_FIELDS, (int(v) for v in host[:MCL_RECORD])))
    row = [int(v) for v in host[MCL_RECORD:MCL_RECORD + 4]]
    o, r = np.asarray(pf.origin, dtype=np.float64), float(pf.resolution)
    mean = np.array([rec["sum_x"], rec["sum_y"], rec["sum_z"]], dtype=np.float64) / float(rec["s1"])
    yaw = float(np.arctan2(float(rec["sum_sin"]), float(rec["sum_cos"])))
    return ParticleEstimate(pose=o + r * mean / 256.0, yaw=yaw, quat=np.array([np.cos(0.5 * yaw), 0.0, 0.0, np.sin(0.5 * yaw)]),
                            best_pose=o + r * np.asarray(row[:3], dtype=np.float64) / 256.0, best_yaw=2.0 * np.pi * row[3] / MCL_TURN,
                            best_index=rec["best"], best_score=rec["best_score"], known=rec["best_known"], used=rec["best_used"],
                            n_eff=float(rec["s1"]) * float(rec["s1"]) / float(rec["s2"]), resampled=bool(rec["verdict"]),
                            state=np.append(mean, (yaw % (2.0 * np.pi)) * MCL_TURN / (2.0 * np.pi)), record=np.asarray(host[:MCL_RECORD]))
