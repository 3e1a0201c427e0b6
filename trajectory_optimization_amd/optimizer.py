"""Device-resident optimisation loops.

`optimize_trajectory` is the reference's TrajOpt.run (/root/reference/src/trajectory_optimization.py:100-127):
Adam over (poses, quats) with two learning rates, the criterion of ModelTraj, and the early stop on visibility
and smoothness gains — but every step is a fixed sequence of kernel launches through the C ABI (visibility
forward/backward, regularisers + their analytic gradient, Adam, the early-stop rule), with no host
synchronisation until the run ends: the stop flag lives on the device and turns the remaining updates into no-ops.

The classes in model.py + torch.optim.Adam remain the drop-in path; this module is the launch-only fast path.
"""
import ctypes

import torch

from . import _lib, ops
from ._lib import check, ptr, stream_ptr


LAST_OUTPUTS = _lib.CONSTANTS["TOHIP_TRAJ_OPT_LAST_OUTPUTS"]


class TrajOptResult:
    def __init__(self, steps_taken, stopped, losses, vis_gain, smooth_gain):
        self.steps_taken, self.stopped, self.losses = steps_taken, stopped, losses
        self.visibility_gain, self.smoothness_gain = vis_gain, smooth_gain


class _OptRun:
    """One device-resident optimisation run as the library sees it (struct tohip_traj_opt): B equal-length trajectories over one
    packed cloud, every per-step vector allocated once; step(i) is ONE library call — five launches (tohip_traj_opt_step)."""

    def __init__(self, models, n_opt_steps, lr_pose, lr_quat, rewards_th, smoothness_th, vis_wps_dist, betas, adam_eps):
        L = _lib.lib()
        m0 = models[0]
        self.models, self.B, self.dev, self.n_steps = models, len(models), m0.device, max(int(n_opt_steps), 1)
        self.dev_index = _lib.device_index(self.dev)
        B, dev = self.B, self.dev
        cloud, rig = m0._cloud, m0._rig
        W = self.W = m0.poses.shape[0]
        step_w = m0._wps_step(vis_wps_dist)
        n_eval = self.n_eval = (W + step_w - 1) // step_w
        C = rig.n_cams if rig else 1
        f32 = dict(dtype=torch.float32, device=dev)
        if B == 1:   # the Parameters themselves are updated in place
            self.poses, self.quats, self.poses0 = m0.poses.data, m0.quats.data, m0.poses0.contiguous()
        else:
            self.poses = torch.cat([m.poses.data for m in models]).contiguous()
            self.quats = torch.cat([m.quats.data for m in models]).contiguous()
            self.poses0 = torch.cat([m.poses0 for m in models]).contiguous()
        if not (self.poses.is_contiguous() and self.quats.is_contiguous() and self.poses.dtype == torch.float32 and self.quats.dtype == torch.float32):
            raise RuntimeError("optimize_trajectory: poses / quats must be contiguous float32 tensors")
        self.toff = (torch.arange(B + 1, dtype=torch.int32) * n_eval).to(dev) if B > 1 else None
        self.ws = m0._workspace(n_eval) if B == 1 else ops.TrajWorkspace(cloud, B * n_eval * C, B)
        self.pg, self.qg = torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 4), **f32)
        self.lo_sum = torch.empty((B, cloud.npad), **f32)
        self.minmax = torch.empty((B * n_eval * C, 2), **f32)
        self.rewards, self.scalars = torch.empty((B, cloud.n), **f32), torch.zeros((B, 4), **f32)
        self.loss_log = torch.zeros((B, self.n_steps, 8), **f32)
        self.state_log = torch.zeros((B, self.n_steps + 1, 8), **f32)
        self.moments = [torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 4), **f32), torch.zeros((B * W, 4), **f32)]
        nbytes = L.tohip_traj_opt_scratch_bytes(W, B)
        self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        c = _lib.TrajOpt()
        # TOHIP_TRAJ_OPT_LAST_OUTPUTS: the rewards (and the log-odds vector) are materialised by the run's last step only — what the
        # reference publishes after its loop (trajectory_optimization.py:147-157); every step computes them all the same
        c.packed, c.n_points, c.n_wps, c.wps_step, c.flags, c.n_traj, c.n_steps = cloud.blob.data_ptr(), cloud.n, W, step_w, int(m0._flags) | LAST_OUTPUTS, B, self.n_steps
        c.traj_offsets = self.toff.data_ptr() if self.toff is not None else None
        c.cam = m0._cam.c
        if rig is not None:
            c.rig = rig.c
        c.poses, c.quats, c.poses0 = self.poses.data_ptr(), self.quats.data_ptr(), self.poses0.data_ptr()
        c.smoothness_weight, c.traj_length_weight = float(m0.smoothness_weight), float(m0.traj_length_weight)
        c.lr_pose, c.lr_quat, c.beta1, c.beta2, c.adam_eps = float(lr_pose), float(lr_quat), float(betas[0]), float(betas[1]), float(adam_eps)
        c.rewards_th, c.smoothness_th = float(rewards_th), float(smoothness_th)
        c.exp_avg_p, c.exp_avg_sq_p, c.exp_avg_q, c.exp_avg_sq_q = (t.data_ptr() for t in self.moments)
        c.poses_grad, c.quats_grad = self.pg.data_ptr(), self.qg.data_ptr()
        c.poses_grad_eval = c.quats_grad_eval = None
        c.lo_sum, c.minmax, c.rewards, c.scalars = self.lo_sum.data_ptr(), self.minmax.data_ptr(), self.rewards.data_ptr(), self.scalars.data_ptr()
        c.loss_log, c.state_log = self.loss_log.data_ptr(), self.state_log.data_ptr()
        c.workspace, c.workspace_bytes = self.ws.buf.data_ptr(), self.ws.bytes
        c.scratch, c.scratch_bytes = self.scratch.data_ptr(), nbytes
        self.clearance = m0._clearance_on
        if self.clearance:   # the clearance term: one launch more per step, first (its rows join the regularisers')
            if m0.clearance_mode == "segments":   # the swept term: the segment query and its per-waypoint combine, two launches
                c.flags |= ops.CLEARANCE_SEGMENTS
                cb = L.tohip_traj_clearance_segments_scratch_bytes(W, B)
            else:
                cb = L.tohip_traj_clearance_scratch_bytes(W, B)
            self.clr_scratch = torch.empty(cb, dtype=torch.uint8, device=dev)
            c.clearance_radius, c.clearance_weight = float(m0.clearance_radius), float(m0.clearance_weight)
            c.clearance_scratch, c.clearance_scratch_bytes = self.clr_scratch.data_ptr(), cb
        self.clr_fill = None
        if self.clearance and m0._clr_map is not None:   # the map's term: every step fills the scratch first, the library launches no query
            c.flags |= ops.CLEARANCE_PREFILLED
            self.clr_fill = (m0._clr_map, self.poses, m0.clearance_radius, m0.clearance_weight, m0.clearance_mode, B,
                             *ops.clearance_scratch_views(self.clr_scratch, B * W))
        self.c, self.ref, self.fn = c, ctypes.byref(c), L.tohip_traj_opt_step

    def run(self, n):
        if n != self.n_steps:   # a run cut short has no "last step" to leave the rewards: every step writes them
            self.c.flags &= ~LAST_OUTPUTS
        _lib.on_device(self.dev_index, self._steps, n)
        for m in self.models:   # the Parameters (or their copies) were written through raw pointers
            torch.autograd.graph.increment_version(m.poses)
            torch.autograd.graph.increment_version(m.quats)

    def _steps(self, n, stream):
        for i in range(n):
            if self.clr_fill is not None:
                ops.clearance_rows(*self.clr_fill)
            rc = self.fn(self.ref, i, stream)
            if rc:
                check(rc, "tohip_traj_opt_step")
            self.ws.generation += 1

    def results(self, n):
        """The run's only host synchronisation: the final state rows and the loss logs."""
        st = self.state_log[:, n].cpu()
        lt = self.loss_log.cpu()
        out = []
        for b, m in enumerate(self.models):
            if self.B > 1:
                m.poses.data.copy_(self.poses[b * self.W:(b + 1) * self.W])
                m.quats.data.copy_(self.quats[b * self.W:(b + 1) * self.W])
            steps = int(st[b, 3].item())
            if steps > 0:   # (a trajectory that was never stepped keeps what it had)
                row = lt[b, steps - 1]
                m.rewards = self.rewards[b]
                m.loss = {"vis": row[0], "l2": row[1], "length": row[2], "smooth": row[3]}
                if self.clearance:
                    m.loss["clearance"] = row[5]
            out.append(TrajOptResult(steps, bool(st[b, 2].item() != 0), lt[b, :steps, 4].tolist(), float(st[b, 4]), float(st[b, 5])))
        return out


@torch.no_grad()
def optimize_trajectory(model, n_opt_steps=10, lr_pose=0.1, lr_quat=0.0, rewards_th=1.2, smoothness_th=0.9,
                        vis_wps_dist=0.5, betas=(0.9, 0.999), adam_eps=1e-8):
    """Runs up to n_opt_steps on `model` (a ModelTraj) in place; returns a TrajOptResult (one host sync, at the end).
    model.poses / model.quats hold the optimised trajectory, model.rewards the last rewards, model.loss the last terms.

    A step is ONE library call and FIVE launches (tohip_traj_opt_step): the waypoint selection is a stride of the first launch's
    reads, the regularisers and Adam's constants are one block more of the THIRD launch (the sparse kernel's: nothing launched
    before it may read them), the parameter update and the early-stop bookkeeping are the tail of the last launch's blocks.  A waypoint-sharded or occlusion-aware model has a collective or a hull
    pass inside the step, and a model with a log-odds prior (prior_log_odds) a reward of its own: they go through the separate calls
    (forward | all-reduce | reward + backward | step tail).
    (A HIP-graph replay of the step was measured slower than issuing its launches — a replay costs 10-16 us of host time by
    itself, five launches 17 us, and the GPU side is the same — so there is no graph variant.)"""
    if n_opt_steps <= 0:   # nothing to run: the model keeps its rewards and loss terms
        return TrajOptResult(0, False, [], 0.0, 0.0)
    if model._needs_split_step():
        return _optimize_trajectory_split(model, n_opt_steps, lr_pose, lr_quat, rewards_th, smoothness_th, vis_wps_dist, betas, adam_eps)
    run = _OptRun([model], n_opt_steps, lr_pose, lr_quat, rewards_th, smoothness_th, vis_wps_dist, betas, adam_eps)
    run.run(n_opt_steps)
    return run.results(n_opt_steps)[0]


class _TailRun:
    """One run of the separate-calls path as its two users see it (_optimize_trajectory_split: one model; optimize_team: B members):
    equal-length trajectories laid end to end, every per-step buffer allocated once, and per step the caller's visibility step
    over the evaluated waypoints (`st`: what its step() leaves in st.pg / st.qg / st.scalars is what the tail reads), the clearance
    query when the term is on, the caller's tail entry — launches only.  `tail_args`: the arguments every tail entry starts with
    (tohip_traj_step_tail_multi / _clearance, tohip_team_step_tail), `clr_args`: the three the clearance term adds."""

    def __init__(self, models, st, n_opt_steps, lr_pose, lr_quat, rewards_th, smoothness_th, vis_wps_dist, betas, adam_eps, what):
        L = _lib.lib()
        m0 = models[0]
        self.models, self.B, self.dev, self.n, self.clr_source = models, len(models), m0.device, int(n_opt_steps), m0._clearance_source
        B, n, dev = self.B, self.n, self.dev
        W = self.W = m0.poses.shape[0]
        step_w = self.step_w = m0._wps_step(vis_wps_dist)
        n_eval = self.n_eval = (W + step_w - 1) // step_w
        f32 = dict(dtype=torch.float32, device=dev)
        if B == 1:   # the Parameters themselves are updated in place
            self.poses, self.quats, self.poses0 = m0.poses.data, m0.quats.data, m0.poses0.contiguous()
        else:
            self.poses = torch.cat([m.poses.data for m in models]).contiguous()
            self.quats = torch.cat([m.quats.data for m in models]).contiguous()
            self.poses0 = torch.cat([m.poses0 for m in models]).contiguous()
        poses, quats = self.poses, self.quats
        if not (poses.is_contiguous() and quats.is_contiguous() and poses.dtype == torch.float32 and quats.dtype == torch.float32):
            raise RuntimeError(f"{what}: poses / quats must be contiguous float32 tensors")
        # the evaluated waypoints are every step_w-th row of the Parameters, read in place (TOHIP_TRAJ_STRIDE in the flags: no gather);
        # over a concatenation that lands on each member's rows only when W is a multiple of the step: a gather otherwise
        self.strided = B == 1 or W % step_w == 0
        self.stride = ((step_w - 1) & 0xffff) << 8 if self.strided else 0
        self.src = (poses, quats) if self.strided else (torch.empty((B * n_eval, 3), **f32), torch.empty((B * n_eval, 4), **f32))
        self.pg, self.qg = torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 4), **f32)
        self.moments = [torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 3), **f32), torch.zeros((B * W, 4), **f32), torch.zeros((B * W, 4), **f32)]
        self.loss_log = torch.zeros((B, n + 1, 8), **f32)   # (a stopped trajectory's later steps rewrite the row after its last)
        self.clr, self.clr_args = m0._clearance_on, (0.0, None, None)
        if self.clr:   # the clearance query of all B W waypoints: its gradient rows and per-waypoint terms, consumed by the tail
            self.clr_rows = torch.empty((B * W, 3), **f32)
            self.clr_terms = ops.clearance_terms(W, B, m0.clearance_mode, dev)
            self.clr_args = (float(m0.clearance_weight), ptr(self.clr_rows), ptr(self.clr_terms))
        self.st, self.weights = st, (float(m0.smoothness_weight), float(m0.traj_length_weight), float(m0.eps))
        self.tail_args = (ptr(poses), ptr(quats), ptr(self.poses0), W, B, ptr(st.pg), ptr(st.qg), n_eval, step_w, ptr(self.pg), ptr(self.qg),
                          *(ptr(t) for t in self.moments), *self.weights, float(lr_pose), float(lr_quat), betas[0], betas[1], adam_eps,
                          float(rewards_th), float(smoothness_th), ptr(st.scalars), ptr(self.loss_log), (n + 1) * 8)

    def run(self, vis_step, tail, what):
        """n steps: vis_step(poses_src, quats_src, flags_extra) is the caller's visibility step, tail(i) its tail entry's return code."""
        L, m0 = _lib.lib(), self.models[0]
        with torch.cuda.device(self.dev):
            for i in range(self.n):
                if not self.strided:
                    check(L.tohip_gather_waypoints_multi(ptr(self.poses), ptr(self.quats), self.W, self.B, self.n_eval, self.step_w,
                                                         ptr(self.src[0]), ptr(self.src[1]), stream_ptr()), "tohip_gather_waypoints_multi")
                vis_step(*self.src, self.stride)
                if self.clr:
                    ops.clearance_rows(self.clr_source, self.poses, m0.clearance_radius, m0.clearance_weight, m0.clearance_mode, self.B,
                                       self.clr_rows, self.clr_terms)
                check(tail(i), what)

    def finish(self, steps):
        """Every model's Parameters, rewards (one tensor, shared) and loss terms after `steps` steps -> the loss logs on the host."""
        lt = self.loss_log.cpu()
        rewards = self.st.rewards.clone()   # (the step's buffer is the next run's)
        for b, m in enumerate(self.models):
            if self.B > 1:
                m.poses.data.copy_(self.poses[b * self.W:(b + 1) * self.W])
                m.quats.data.copy_(self.quats[b * self.W:(b + 1) * self.W])
            torch.autograd.graph.increment_version(m.poses)
            torch.autograd.graph.increment_version(m.quats)
            row = lt[b, max(steps, 1) - 1]
            m.rewards = rewards
            m.loss = {"vis": row[0], "l2": row[1], "length": row[2], "smooth": row[3]}
            if self.clr:
                m.loss["clearance"] = row[5]
        return lt


@torch.no_grad()
def _optimize_trajectory_split(model, n_opt_steps, lr_pose, lr_quat, rewards_th, smoothness_th, vis_wps_dist, betas, adam_eps):
    """optimize_trajectory with a collective (a sharded model) or a hull pass (occlusion rows) inside the step: per step the model's
    visibility step (ops.WaypointShardStep or ops.PointShardStep: gradients identical on every rank) and the replicated O(W)
    remainder in one launch — scatter, regularisers, both Adam updates, early stop — so every rank takes the same step."""
    L = _lib.lib()
    W = model.poses.shape[0]
    step_w = model._wps_step(vis_wps_dist)
    n_eval = (W + step_w - 1) // step_w
    points = model._shard.kind == "points"
    st = model._point_step(n_eval) if points else model._waypoint_step(n_eval)
    run = _TailRun([model], st, n_opt_steps, lr_pose, lr_quat, rewards_th, smoothness_th, vis_wps_dist, betas, adam_eps, "optimize_trajectory")
    state = torch.zeros(8, dtype=torch.float32, device=model.device)
    def vis_step(p, q, stride):   # (PointShard refuses occlusion and a prior)
        kw = {} if points else dict(occ=model._own_occlusion_rows(st, p, q, step_w), prior=model._prior)
        st.step(p, q, flags_extra=stride, **kw)
    tail, rest = (L.tohip_traj_step_tail_clearance, run.clr_args) if run.clr else (L.tohip_traj_step_tail_multi, ())
    run.run(vis_step, lambda i: tail(*run.tail_args, ptr(state), *rest, stream_ptr()), "step tail")
    stt = state.cpu()  # the run's only host synchronisation
    steps = int(stt[3].item())
    lt = run.finish(steps)
    if points:
        model._mean_reward = st.scalars[0].clone()
    return TrajOptResult(steps, bool(stt[2].item() != 0), lt[0, :max(steps, 1), 4].tolist(), float(stt[4]), float(stt[5]))


def _check_same_setup(models, vis_wps_dist, what):
    """What a run over several ModelTraj at once demands of them — built on the same points with the same camera, rig, mode, eps,
    weights and clearance settings, equal numbers of waypoints and the same waypoint step, no sharding, no occlusion rows — or a
    ValueError that names what differs.  Host checks only (equal tensors are compared where the objects differ)."""
    m0 = models[0]
    cloud, cam, rig = m0._cloud, m0._cam, m0._rig
    W = m0.poses.shape[0]
    step_w = m0._wps_step(vis_wps_dist)
    for m in models:
        if m._shard.world_size > 1:
            raise ValueError(f"{what}: a sharded model (WaypointShard / PointShard) is not supported")
        if m._occlusion is not None:
            raise ValueError(f"{what}: a model with occlusion rows (occlusion=) is not supported")
        if m.poses.shape[0] != W:
            raise ValueError(f"{what}: the models must have equal numbers of waypoints ({m.poses.shape[0]} and {W})")
        if m._wps_step(vis_wps_dist) != step_w:
            raise ValueError(f"{what}: the models must share the waypoint step ({m._wps_step(vis_wps_dist)} and {step_w} at "
                             f"vis_wps_dist={vis_wps_dist})")
        if m._cloud.n != cloud.n or (m is not m0 and m.points.data_ptr() != m0.points.data_ptr() and not torch.equal(m.points, m0.points)):
            raise ValueError(f"{what}: the models must be built on the same points")
        if (m._flags != m0._flags or (m._rig is None) != (rig is None) or bytes(m._cam.c) != bytes(cam.c) or
                m.smoothness_weight != m0.smoothness_weight or m.traj_length_weight != m0.traj_length_weight or
                m._clearance_on != m0._clearance_on or
                (m0._clearance_on and (m.clearance_radius != m0.clearance_radius or m.clearance_weight != m0.clearance_weight or
                                       m.clearance_mode != m0.clearance_mode))):
            raise ValueError(f"{what}: the models must share the camera, rig, mode, weights and clearance settings")
        if m0._clearance_on and ((m._clr_map is None) != (m0._clr_map is None) or (m0._clr_map is not None and not m0._clr_map.same_as(m._clr_map))):
            raise ValueError(f"{what}: the models must share the clearance settings: one clearance_map (the same map objects) and the "
                             "same clearance_unknown")
        if m is not m0 and (m.device != m0.device or float(m.eps) != float(m0.eps)):
            raise ValueError(f"{what}: the models must live on one device and share eps")
        if m is not m0 and rig is not None and (m._rig.n_cams != rig.n_cams or not torch.equal(m._rig.q, rig.q) or not torch.equal(m._rig.t, rig.t)):
            raise ValueError(f"{what}: the models must share the camera rig (extrinsics differ)")


@torch.no_grad()
def optimize_trajectories(models, n_opt_steps=10, lr_pose=0.1, lr_quat=0.0, rewards_th=1.2, smoothness_th=0.9,
                          vis_wps_dist=0.5, betas=(0.9, 0.999), adam_eps=1e-8):
    """`optimize_trajectory` for several candidate trajectories over the SAME cloud at once: every step is one
    set of launches for all of them — their evaluated waypoints go through the visibility kernels as one batch of virtual
    waypoints, each trajectory keeps its own log-odds vector, rewards, loss terms, Adam moments and early-stop state (a
    trajectory that has stopped stays put while the others go on).  Each model ends up exactly — bit for bit — where its own
    `optimize_trajectory` run would have put it.  Models: ModelTraj built on the same points with the same camera, rig and
    mode, equal numbers of waypoints and the same waypoint step; no sharding, no occlusion, no prior_log_odds.  -> [TrajOptResult]."""
    if any(m._prior is not None for m in models):
        raise ValueError("optimize_trajectories: a model with a log-odds prior (prior_log_odds) is not supported; run "
                         "optimize_trajectory on it")
    _check_same_setup(models, vis_wps_dist, "optimize_trajectories")
    if n_opt_steps <= 0:   # nothing to run: the models keep their rewards and loss terms
        return [TrajOptResult(0, False, [], 0.0, 0.0) for _ in models]
    run = _OptRun(list(models), n_opt_steps, lr_pose, lr_quat, rewards_th, smoothness_th, vis_wps_dist, betas, adam_eps)
    run.run(n_opt_steps)
    return run.results(n_opt_steps)


class TeamOptResult:
    """optimize_team's result: steps_taken and stopped (the team's), losses (the TEAM total of every step taken), visibility_gain (the
    team's mean reward over its first), smoothness_gains (per member) and member_losses (per member, the last step's own terms:
    l2, length, smooth[, clearance]); loss_log: a (B, steps_taken, 8) float32 array, every member's row of every step taken
    ([0] vis [1] l2 [2] length [3] smooth [4] the team total [5] clearance), or None when nothing ran; poses_grad (B, W, 3) /
    quats_grad (B, W, 4): the full gradients of the last step launched (device tensors), or None."""

    def __init__(self, steps_taken, stopped, losses, vis_gain, smooth_gains, member_losses, loss_log=None, poses_grad=None, quats_grad=None):
        self.poses_grad, self.quats_grad = poses_grad, quats_grad
        self.steps_taken, self.stopped, self.losses = steps_taken, stopped, losses
        self.visibility_gain, self.smoothness_gains, self.member_losses, self.loss_log = vis_gain, smooth_gains, member_losses, loss_log


def check_team(models, vis_wps_dist, what):
    """A team's members (team coverage): what _check_same_setup demands, no point-sharded member, and at most one
    log-odds prior — the first model's; the others have none or the same tensor.  -> the team's ops.LogOddsPrior or None."""
    models = list(models)
    if not models:
        raise ValueError(f"{what}: no models")
    for m in models:
        if m._shard.kind == "points":
            raise ValueError(f"{what}: a sharded model (WaypointShard / PointShard) is not supported")
    _check_same_setup(models, vis_wps_dist, what)
    prior = models[0]._prior
    for m in models[1:]:
        q = m._prior
        if q is None or q is prior:
            continue
        if prior is None or not (q.values.data_ptr() == prior.values.data_ptr() or torch.equal(q.values, prior.values)):
            raise ValueError(f"{what}: the team has ONE log-odds prior, the first model's: the other members must have none or the same "
                             "tensor (two different priors given)")
    return prior


@torch.no_grad()
def optimize_team(models, n_opt_steps=10, lr_pose=0.1, lr_quat=0.0, rewards_th=1.2, smoothness_th=0.9, vis_wps_dist=0.5,
                  betas=(0.9, 0.999), adam_eps=1e-8):
    """Several robots over ONE map, optimised in the same steps and rewarded ONCE for a point whichever of them sees it (DESIGN.md
    10, team coverage).  The team's log-odds are one sum over all members' evaluated waypoints, rewards = sigmoid(that + prior); a
    member's visibility gradient takes r (1 - r) from the team's reward; regularisers, clearance, Adam and its moments stay per
    member; the early stop is the team's (visibility gain of the team's mean reward, every member's smooth gain).  Launches only, one
    host synchronisation at the end.  Members: as optimize_trajectories', and at most one prior (the first model's).  Every model
    ends with poses / quats updated in place, model.loss = its own terms and the team's vis, model.rewards = the team's rewards (one
    tensor, shared).  A team of one is optimize_trajectory on the separate-calls path, bit for bit.  -> TeamOptResult."""
    models = list(models)
    prior = check_team(models, vis_wps_dist, "optimize_team")
    B, m0 = len(models), models[0]
    if n_opt_steps <= 0:   # nothing to run: the models keep their rewards and loss terms
        return TeamOptResult(0, False, [], 0.0, [0.0] * B, [])
    L = _lib.lib()
    n = int(n_opt_steps)
    W = m0.poses.shape[0]
    step_w = m0._wps_step(vis_wps_dist)
    # the team's visibility step: the members' evaluated waypoints as ONE trajectory of B n_eval rows through the separate calls
    st = m0._waypoint_step(B * ((W + step_w - 1) // step_w))
    run = _TailRun(models, st, n, lr_pose, lr_quat, rewards_th, smoothness_th, vis_wps_dist, betas, adam_eps, "optimize_team")
    sb = L.tohip_team_state_bytes(B, n)
    team_state = torch.zeros(sb, dtype=torch.uint8, device=m0.device)
    state = team_state[:sb // 2].view(torch.float32).view(n + 1, B, 8)
    terms64 = team_state[sb // 2:].view(torch.float64).view(n + 1, B, 4)
    member_terms = torch.empty((B, 8), dtype=torch.float32, device=m0.device)
    with torch.cuda.device(m0.device):
        # every member's terms at the start: row 0 of the state's terms (a step's blocks read the others' from the row before)
        check(L.tohip_team_loss(ptr(run.poses), ptr(run.poses0), W, B, *run.weights, None, 0.0, None, ptr(member_terms), ptr(terms64), None,
                                None, None, stream_ptr()), "tohip_team_loss")
    run.run(lambda p, q, stride: st.step(p, q, flags_extra=stride, prior=prior),
            lambda i: L.tohip_team_step_tail(*run.tail_args, ptr(team_state), sb, n, i, *run.clr_args, stream_ptr()), "tohip_team_step_tail")
    stt = state[n].cpu()   # the run's only host synchronisation
    steps = int(stt[0, 3].item())
    lt = run.finish(steps)
    member_losses = [{k: float(v) for k, v in m.loss.items() if k != "vis"} for m in models]
    return TeamOptResult(steps, bool(stt[0, 2].item() != 0), lt[0, :max(steps, 1), 4].tolist(), float(stt[0, 4]),
                         [float(x) for x in stt[:, 5]], member_losses, lt[:, :steps].numpy(), run.pg.view(B, W, 3), run.qg.view(B, W, 4))


class PoseOptResult:
    def __init__(self, losses):
        self.losses = losses


def _refresh_age(age, every):
    """The fixed refresh schedule of occlusion rows: a row is rebuilt on every `every`-th forward — when there is none (age None)
    or the cached one has served `every` forwards — and reused in between.  -> the row's age after this forward: 1 when this
    forward rebuilds it.  The models' row caches and the launch-only loops below all step it."""
    return 1 if age is None or age >= every else age + 1


def _occlusion_schedule(model, hpr, what):
    """The occlusion refresh period of a ModelPose run (0: no per-pose rows); hpr=True with occlusion= is refused as in forward()."""
    if model._occlusion is None:
        return 0
    if hpr:
        raise ValueError(f"{what}: hpr=True (the reference's world-frame mask) and occlusion= (each pose's own) exclude each other")
    return model.occlusion_refresh_every


@torch.no_grad()
def optimize_pose(model, n_opt_steps=100, lr_pose=0.1, lr_quat=0.1, hpr=False, betas=(0.9, 0.999), adam_eps=1e-8):
    """The reference's PoseOpt loop (/root/reference/src/pose_optimization.py:93-97,124-141): n_opt_steps of
    `loss = model(hpr); loss.backward(); Adam(trans @ lr_pose, quat @ lr_quat).step()` on a ModelPose, in place, as
    launches only — two per step (tohip_pose_opt_step: ONE pass over the cloud for observations, loss and gradient sums, then a
    one-block finish with both Adam updates and the loss log) — with one host synchronisation when the run ends.  model.trans / model.quat hold the optimised pose (the
    reference normalises the quaternion only when publishing, :102), model.observations the last observations.
    A model with occlusion= gets its row rebuilt from the pose on the device before steps 1, k + 1, 2k + 1, ... (k =
    model.occlusion_refresh_every: the schedule of a fresh model's forwards); the steps in between are launches only, and each
    refresh adds the hull pass's own host synchronisation.  The model's row cache is left as n_opt_steps forwards would leave it
    (the last row, the steps since it was built, the rebuilds counted in occlusion_rebuilds)."""
    L = _lib.lib()
    dev = model.device
    cloud, cam, ws = model._cloud, model._cam, model._ws
    f32 = dict(dtype=torch.float32, device=dev)
    every = _occlusion_schedule(model, hpr, "optimize_pose")
    mask = None
    if hpr:
        model(hpr=True)  # builds (and caches) the world-frame occlusion mask of model.py:114
        mask = model._occlusion_mask
    obs, scalars = torch.empty(cloud.n, **f32), torch.zeros(4, **f32)
    tg, qg = torch.empty((1, 3), **f32), torch.empty((1, 4), **f32)
    mt, vt = torch.zeros(3, **f32), torch.zeros(3, **f32)
    mq, vq = torch.zeros(4, **f32), torch.zeros(4, **f32)
    losses = torch.empty(max(n_opt_steps, 1), **f32)
    trans, quat = model.trans.data, model.quat.data
    fn = L.tohip_pose_opt_step_bits if every else L.tohip_pose_opt_step
    rest = (obs.data_ptr(), scalars.data_ptr(), tg.data_ptr(), qg.data_ptr(), mt.data_ptr(), vt.data_ptr(), mq.data_ptr(), vq.data_ptr(),
            float(lr_pose), float(lr_quat), float(betas[0]), float(betas[1]), float(adam_eps))
    args = (cloud.blob.data_ptr(), cloud.n, trans.data_ptr(), quat.data_ptr(), cam.ref(), mask.data_ptr() if mask is not None else None) + rest

    def steps(stream):
        """-> (the last occlusion row, its age, rows built): what the model's cache adopts."""
        args_i, row, age, rebuilds = args, None, None, 0
        for i in range(n_opt_steps):
            if every:
                age = _refresh_age(age, every)
                if age == 1:   # the pose's occlusion row from the pose the device holds now (queued after the last step)
                    row, rebuilds = model._build_occlusion_rows(trans, quat), rebuilds + 1
                    args_i = args[:5] + (row.data_ptr(),) + rest
            # one pass over the cloud (observations, their sum, the gradient sums) and its one-block finish (loss, gradient, both
            # Adam updates, the loss log): two launches per step
            rc = fn(*args_i, i + 1, losses.data_ptr(), ws.buf.data_ptr(), ws.bytes, stream)
            if rc:
                check(rc, "tohip_pose_opt_step_bits" if every else "tohip_pose_opt_step")
        return row, age, rebuilds

    row, age, rebuilds = _lib.on_device(_lib.device_index(dev), steps)
    torch.autograd.graph.increment_version(model.trans)
    torch.autograd.graph.increment_version(model.quat)
    model.observations = obs
    if every and n_opt_steps > 0:   # the cache holds the last row and its age: the next forward continues the schedule
        model._adopt_occlusion_row(row, age, rebuilds)
    return PoseOptResult(losses[:n_opt_steps].cpu().tolist())  # the run's only host synchronisation


@torch.no_grad()
def optimize_poses(models, n_opt_steps=100, lr_pose=0.1, lr_quat=0.1, hpr=False, betas=(0.9, 0.999), adam_eps=1e-8):
    """`optimize_pose` for several poses of ONE camera over the SAME cloud at once (many starts; scoring candidate views): every
    step is one library call and two launches for all of them (tohip_pose_opt_step_multi) — one pass over the cloud evaluates a
    tile of poses on the points it holds, then one finish block per pose runs its loss, gradient and both Adam updates.  Each model
    ends up bit for bit where its own `optimize_pose` run would have put it (trans, quat, losses, observations).  Models: ModelPose
    on the same points with the same camera (K, image size, clip limits), eps, device and occlusion settings.  -> [PoseOptResult].
    With occlusion= every pose has its own row: all B are rebuilt in ONE batched hull pass (ops.occlusion_bits) on optimize_pose's
    schedule, and the pass reads pose b's row for pose b (tohip_pose_opt.occlusion_bits).
    Each model.observations is row b of one (B, N) tensor: any one of them keeps all B x N floats alive (clone a row to keep it
    alone)."""
    models = list(models)
    if not models:
        raise ValueError("optimize_poses: no models")
    m0 = models[0]
    for m in models[1:]:
        if m.device != m0.device or float(m.eps) != float(m0.eps):
            raise ValueError("optimize_poses: the models must live on one device and share eps")
        if bytes(m._cam.c) != bytes(m0._cam.c):
            raise ValueError("optimize_poses: the models must share the camera (K, image size, clip limits)")
        if (m._occlusion != m0._occlusion or tuple(m._occlusion_limits) != tuple(m0._occlusion_limits) or
                m.occlusion_refresh_every != m0.occlusion_refresh_every):
            raise ValueError("optimize_poses: the models must share occlusion, occlusion_limits and occlusion_refresh_every")
        if m._occlusion_grid is not m0._occlusion_grid:
            raise ValueError("optimize_poses: the models must share one occlusion_grid (ModelPose.sharing_cloud_of hands it on)")
        # what the kernels read is the packed cloud: the same object, or one of equal size over equal rows (the shapes are compared
        # first — a model on a slice of the same tensor shares its data pointer)
        c, c0 = m._cloud, m0._cloud
        if c is not c0 and (c.n != c0.n or tuple(c.points.shape) != tuple(c0.points.shape) or not torch.equal(c.points, c0.points)):
            raise ValueError("optimize_poses: the models must be built on the same points")
    every = _occlusion_schedule(m0, hpr, "optimize_poses")
    if n_opt_steps <= 0:   # nothing to run: the models keep what they have
        return []
    if len(models) == 1:   # the single-pose pass carries no tile of accumulators: its own path
        return [optimize_pose(m0, n_opt_steps, lr_pose, lr_quat, hpr, betas, adam_eps)]
    L = _lib.lib()
    dev, cloud, B = m0.device, m0._cloud, len(models)
    f32 = dict(dtype=torch.float32, device=dev)
    mask = m0._hpr_mask() if hpr else None   # pose independent: built once for the batch
    trans = torch.cat([m.trans.data for m in models]).contiguous()
    quat = torch.cat([m.quat.data for m in models]).contiguous()
    obs, scalars = torch.empty((B, cloud.n), **f32), torch.zeros((B, 4), **f32)
    tg, qg = torch.empty((B, 3), **f32), torch.empty((B, 4), **f32)
    moments = [torch.zeros((B, 3), **f32), torch.zeros((B, 3), **f32), torch.zeros((B, 4), **f32), torch.zeros((B, 4), **f32)]
    losses = torch.empty((B, n_opt_steps), **f32)
    ws = ops.PoseWorkspace(cloud, B)
    c = _lib.PoseOpt()
    c.packed, c.n_points, c.n_poses, c.n_steps = cloud.blob.data_ptr(), cloud.n, B, n_opt_steps
    c.cam = m0._cam.c
    c.occlusion_mask = mask.data_ptr() if mask is not None else None
    c.occlusion_bits = None
    c.trans, c.quat = trans.data_ptr(), quat.data_ptr()
    c.lr_pose, c.lr_quat, c.beta1, c.beta2, c.adam_eps = float(lr_pose), float(lr_quat), float(betas[0]), float(betas[1]), float(adam_eps)
    c.exp_avg_t, c.exp_avg_sq_t, c.exp_avg_q, c.exp_avg_sq_q = (t.data_ptr() for t in moments)
    c.scalars, c.trans_grad, c.quat_grad, c.loss_log = scalars.data_ptr(), tg.data_ptr(), qg.data_ptr(), losses.data_ptr()
    c.workspace, c.workspace_bytes = ws.buf.data_ptr(), ws.bytes
    ref, fn = ctypes.byref(c), L.tohip_pose_opt_step_multi

    def steps(stream):
        rows, age, rebuilds = None, None, 0
        for i in range(n_opt_steps):
            if every:
                age = _refresh_age(age, every)
                if age == 1:   # every pose's row, from the poses the device holds now, in one batched pass
                    rows, rebuilds = m0._build_occlusion_rows(trans, quat), rebuilds + 1
                    c.occlusion_bits = rows.data_ptr()
            # the observations are what the last step leaves (optimize_pose writes them every step; the bits are the same)
            rc = fn(ref, i + 1, obs.data_ptr() if i + 1 == n_opt_steps else None, stream)
            if rc:
                check(rc, "tohip_pose_opt_step_multi")
        for b, m in enumerate(models):
            m.trans.data.copy_(trans[b:b + 1])
            m.quat.data.copy_(quat[b:b + 1])
            torch.autograd.graph.increment_version(m.trans)
            torch.autograd.graph.increment_version(m.quat)
            m.observations = obs[b]
            if every:   # each model's cache holds its own last row and its age (optimize_pose's bookkeeping)
                m._adopt_occlusion_row(rows[b:b + 1].clone(), age, rebuilds)

    _lib.on_device(_lib.device_index(dev), steps)
    lt = losses.cpu()   # the run's only host synchronisation
    return [PoseOptResult(lt[b].tolist()) for b in range(B)]


def _adam_update(L, entries, arr):
    """One launch for all the listed (group, param, state, grad) entries (at most ADAM_MAX_GROUPS per launch)."""
    k = 0
    dev = None
    for group, p, st, g in entries:
        e = arr[k]
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        e.n = p.numel()
        e.lr, (e.beta1, e.beta2), e.eps, e.step = group["lr"], group["betas"], group["eps"], int(st["step"])
        k += 1
        if dev is not None and p.device != dev:
            raise RuntimeError("one optimizer step over parameters of several devices is not supported")
        dev = p.device
    rc = _lib.on_device(dev.index, L.tohip_adam_step_multi, arr, k)   # (a tensor's device always has its index)
    if rc:
        check(rc, "tohip_adam_step_multi")
    for _, q, _, _ in entries:   # the kernel wrote through raw pointers: autograd's in-place guards must still see an update
        torch.autograd.graph.increment_version(q)


def _steppable(p, g):
    return p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.dtype == torch.float32 and g.is_contiguous() and not g.is_sparse


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam for the models' Parameters (defaults of the reference's loops: betas (0.9, 0.999), eps 1e-8, no
    weight decay, no amsgrad) with ONE kernel launch for all parameters (tohip_adam_step_multi) instead of the dozen small foreach
    kernels per group — the drop-in loop is launch-bound.  Same constructor (parameter groups with their own `lr`), so
    `ExponentialLR` and friends work unchanged:

        optimizer = Adam([{'params': [model.poses], 'lr': 0.1}, {'params': [model.quats], 'lr': 0.02}])
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._arr = (_lib.AdamGroup * _lib.ADAM_MAX_GROUPS)()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries = []
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not g.is_contiguous():
                    g = g.contiguous()
                if not _steppable(p, g):
                    raise RuntimeError("trajectory_optimization_amd.optimizer.Adam steps contiguous float32 HIP tensors only")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                entries.append((group, p, st, g))
        L = _lib.lib()
        for i in range(0, len(entries), _lib.ADAM_MAX_GROUPS):
            _adam_update(L, entries[i:i + _lib.ADAM_MAX_GROUPS], self._arr)
        return loss


# ---- torch.optim.Adam itself, for the models' Parameters ----------------------------------------------------------------------
# The reference builds `torch.optim.Adam([{'params': [model.poses], 'lr': lr_pose}, {'params': [model.quats], 'lr': lr_quat}])`
# (/root/reference/src/trajectory_optimization.py:91-94).  Its step() is ~14 foreach launches and 0.13-0.15 ms of host time for
# these two small tensors — longer than everything else in the loop together.  OPT-IN (r06; until r05 the hooks were installed
# process-wide when the first model was built — a drop-in must not change global torch state on its own): after
#     accelerate_torch_adam(opt)            # this optimizer instance only (Optimizer.register_step_pre_hook / _post_hook), or
#     accelerate_torch_adam(True)           # every torch.optim.Adam of the process (the global hook registry), or
#     ModelTraj(..., fast_adam=True)        # = accelerate_torch_adam(True), said where the model is built
# a step pre-hook updates the Parameters that belong to a model of this package (tagged at construction) with the one-launch
# kernel, on torch's own state entries (`step`, `exp_avg`, `exp_avg_sq`: state_dict(), schedulers and a later switch back all keep
# working), and hides their gradients from torch's step for its duration; every other parameter, and every optimizer configuration
# other than plain Adam (amsgrad, weight decay, maximize, capturable, fused, differentiable, a closure) is left to torch.
# Nothing is registered anywhere until one of the three is called.

_ACCEL = {"on": False, "installed": False}


def accelerate_torch_adam(enable=True):
    """enable = a torch.optim.Adam INSTANCE: take over the update of tagged Parameters inside that optimizer's step() (hooks on the
    instance; returns it).  enable = True / False: the same for every torch.optim.Adam of the process, on / off (the process-wide
    hooks are registered on the first True and do nothing while off).  Off and nowhere registered by default."""
    if isinstance(enable, torch.optim.Optimizer):
        opt = enable
        if not opt.__dict__.get("_tohip_accel"):
            opt.register_step_pre_hook(_adam_pre_hook_instance)
            opt.register_step_post_hook(_adam_post_hook)
            opt.__dict__["_tohip_accel"] = True
        return opt
    _ACCEL["on"] = bool(enable)
    if enable:
        _install_hooks()
    return None


def torch_adam_accelerated():
    """-> (process-wide switch on?, process-wide hooks registered?)"""
    return _ACCEL["on"], _ACCEL["installed"]


def tag_parameter(p):
    """Mark a Parameter as one whose plain-Adam update MAY be taken over once the user asks for it (the models call this for
    poses / quats / trans / quat).  Registers nothing."""
    p._tohip_param = True
    return p


def _install_hooks():
    if not _ACCEL["installed"]:
        from torch.optim.optimizer import register_optimizer_step_pre_hook, register_optimizer_step_post_hook
        register_optimizer_step_pre_hook(_adam_pre_hook)
        register_optimizer_step_post_hook(_adam_post_hook)
        _ACCEL["installed"] = True


def _plain_adam_group(g):
    return not (g.get("amsgrad", False) or g.get("weight_decay", 0) != 0 or g.get("maximize", False) or g.get("capturable", False) or
                g.get("differentiable", False) or g.get("fused", False) or g.get("decoupled_weight_decay", False) or
                not isinstance(g["lr"], float))


def _restore_stash(opt):
    stash = opt.__dict__.pop("_tohip_adam_stash", None)
    if stash:
        for _, p, _, g in stash:
            if p.grad is None:
                p.grad = g


def _adam_pre_hook_instance(opt, args, kwargs):
    return _adam_pre_hook(opt, args, kwargs, force=True)


def _adam_pre_hook(opt, args, kwargs, force=False):
    _restore_stash(opt)   # a step() that raised between the two hooks left the gradients hidden: put them back first
    if (not force and (not _ACCEL["on"] or opt.__dict__.get("_tohip_accel"))) or type(opt) is not torch.optim.Adam or (len(args) > 1 and args[1] is not None) or kwargs.get("closure") is not None:   # args[0] is the optimizer
        return None
    entries = []
    for group in opt.param_groups:
        plain = None
        for p in group["params"]:
            g = p.grad
            if g is None or not getattr(p, "_tohip_param", False):
                continue
            if plain is None:
                plain = _plain_adam_group(group)
            if not plain or not _steppable(p, g):
                continue
            st = opt.state[p]
            if len(st) == 0:   # what torch.optim.Adam._init_group creates (step on the host: neither capturable nor fused)
                st["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif st["step"].is_cuda or not st["exp_avg"].is_contiguous():
                continue
            entries.append((group, p, st, g))
    if not entries:
        return None
    arr = opt.__dict__.get("_tohip_adam_arr")
    if arr is None:
        arr = opt.__dict__["_tohip_adam_arr"] = (_lib.AdamGroup * _lib.ADAM_MAX_GROUPS)()
    L = _lib.lib()
    with torch.no_grad():
        for _, _, st, _ in entries:
            st["step"] += 1
        for i in range(0, len(entries), _lib.ADAM_MAX_GROUPS):
            _adam_update(L, entries[i:i + _lib.ADAM_MAX_GROUPS], arr)
    for _, p, _, _ in entries:
        p.grad = None    # torch's step skips parameters without a gradient; the post-hook puts it back
    opt.__dict__["_tohip_adam_stash"] = entries
    return None


def _adam_post_hook(opt, args, kwargs):
    _restore_stash(opt)
    return None
