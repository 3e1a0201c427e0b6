"""Drop-in ModelPose / ModelTraj (the reference's /root/reference/src/model.py) on MI355X.

Same class names, constructor arguments, attributes and forward()/criterion() semantics as the reference,
so its optimiser loops (/root/reference/src/trajectory_optimization.py:83-127,
/root/reference/src/pose_optimization.py:82-136) run unchanged: Adam over model.poses / model.quats (or
model.trans / model.quat), loss.backward(), reads of model.rewards, model.loss[...], model.observations.

What differs is inside: the visibility / reward forward and its analytic backward run as hand-written
gfx950 kernels behind the C ABI of include/trajopt_hip.h (see ops.py); the O(W) regularisers of
criterion() stay in torch.  There is no CPU fallback: constructing a model on a
non-HIP device raises.
"""
import ctypes
from copy import deepcopy
from time import time

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check, ptr, stream_ptr
from .optimizer import _refresh_age, accelerate_torch_adam, check_team, tag_parameter
from .tools import hidden_pts_removal


# ------------------------------------------------------------------------------ helper functions

class _DistMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, cam):
        ctx.cam = cam
        ctx.save_for_backward(points)
        return ops.soft_masks(points, cam, want_dist=True, want_fov=False)[0]

    @staticmethod
    def backward(ctx, g):
        (points,) = ctx.saved_tensors
        return ops.soft_masks_backward(points, ctx.cam, grad_dist=g).to(points.dtype), None


class _FovMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, cam):
        ctx.cam = cam
        ctx.save_for_backward(points)
        return ops.soft_masks(points, cam, want_dist=False, want_fov=True)[1]

    @staticmethod
    def backward(ctx, g):
        (points,) = ctx.saved_tensors
        return ops.soft_masks_backward(points, ctx.cam, grad_fov=g).to(points.dtype), None


class _ToCameraFrame(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, quat, trans):
        ctx.save_for_backward(verts, quat, trans)
        return ops.to_camera_frame_exact(verts, quat, trans, normalize=True)

    @staticmethod
    def backward(ctx, g):
        verts, quat, trans = ctx.saved_tensors
        gx, gq, gt = ops.to_camera_frame_backward(verts, quat, trans, g, want_points_grad=ctx.needs_input_grad[0])
        return (gx.to(verts.dtype) if gx is not None else None, gq.reshape(quat.shape).to(quat.dtype),
                gt.reshape(trans.shape).to(trans.dtype))


def get_dist_mask(points, min_dist=1.0, max_dist=5.0):
    """/root/reference/src/model.py:13-24.  HIP kernels forward and backward: differentiable w.r.t. `points` like the
    reference's torch ops."""
    assert isinstance(points, torch.Tensor)
    assert points.size()[1] == 3
    cam = ops.Camera(torch.eye(3), 1.0, 1.0, min_dist, max_dist)
    return _DistMask.apply(points, cam)


def get_fov_mask(points, img_height, img_width, intrins, eps=1e-6, binary=False):
    """/root/reference/src/model.py:27-47 (note the reference's positional order: height, then width).  The soft mask is
    differentiable w.r.t. `points`; a gradient w.r.t. the intrinsics is not provided and asking for one raises."""
    assert isinstance(points, torch.Tensor)
    assert points.size()[1] == 3
    assert isinstance(intrins, torch.Tensor)
    assert intrins.size() == torch.Size([3, 3])
    if intrins.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("get_fov_mask: no gradient w.r.t. the camera intrinsics (pass intrins.detach())")
    cam = ops.Camera(intrins, img_width, img_height, 1.0, 5.0, eps)
    if binary:
        pts3 = points.detach().to(torch.float32).t().contiguous()
        return ops.frustum_cull(pts3, cam, float("-inf"), float("inf"), want_indices=False)[1]
    return _FovMask.apply(points, cam)


def to_camera_frame(verts, quat, trans):
    """/root/reference/src/model.py:50-57, bit-identical f32 arithmetic; differentiable w.r.t. all three arguments (the
    quaternion gradient goes through F.normalize, as in the reference)."""
    assert verts.dim() == trans.dim()
    assert quat.size() == torch.Size([1, 4])
    return _ToCameraFrame.apply(verts, quat, trans)


def length_calc(traj):
    """/root/reference/src/model.py:135-139 (vectorised: one norm over the W-1 segments)."""
    if len(traj) < 2:
        return 0.0
    return torch.linalg.norm(traj[1:] - traj[:-1], dim=1).sum()


def mean_angle_calc(traj_wps, eps=1e-6):
    """/root/reference/src/model.py:142-155 (vectorised over the interior waypoints)."""
    traj_wps = torch.as_tensor(traj_wps)
    n_wps = len(traj_wps)
    if n_wps < 3:
        # the reference divides a python float 0.0 by (N_wps - 2): ZeroDivisionError for 2 waypoints
        return 0.0 / (n_wps - 2)
    ab = traj_wps[:-2] - traj_wps[1:-1]
    ac = traj_wps[2:] - traj_wps[1:-1]
    cosang = (ab * ac).sum(dim=1) / (torch.linalg.norm(ab, dim=1) * torch.linalg.norm(ac, dim=1) + eps)
    return torch.arccos(cosang).sum() / (n_wps - 2)


# ------------------------------------------------------------------------------ autograd bridges

class _PoseObservations(torch.autograd.Function):
    @staticmethod
    def forward(ctx, trans, quat, model, mask, occ):
        t = trans.detach().contiguous()
        q = quat.detach().contiguous()
        plan = model._plan
        obs = torch.empty(plan.n, **plan.f32)
        plan.forward(t, q, mask, occ, obs, torch.empty(4, **plan.f32))
        ctx.model, ctx.mask, ctx.occ = model, mask, occ
        ctx.save_for_backward(t, q)
        return obs

    @staticmethod
    def backward(ctx, grad_obs):
        t, q = ctx.saved_tensors
        tg, qg = ctx.model._plan.backward(t, q, ctx.mask, ctx.occ, grad_obs.contiguous())
        return tg, qg, None, None, None


class _PoseLoss(torch.autograd.Function):
    """ModelPose.forward in one autograd node: (trans, quat) -> (loss, observations).  The pass over the cloud that writes the
    observations also takes the gradient sums of the fused loss (they do not depend on its value; tohip_pose_forward_backward), so
    `loss.backward()` is a multiplication of seven numbers; a loss built on model.observations goes through the general
    dL/d observations pass.  mask: a float mask (the reference's world-frame HPR) or None; occ: the pose's occlusion bit row or None."""

    @staticmethod
    def forward(ctx, trans, quat, model, mask, occ):
        if not (trans.is_contiguous() and quat.is_contiguous() and trans.dtype == torch.float32 and quat.dtype == torch.float32):
            raise RuntimeError("ModelPose: trans / quat must be contiguous float32 tensors")
        plan = model._plan
        obs = torch.empty(plan.n, **plan.f32)
        scalars = torch.empty(4, **plan.f32)
        want_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        if want_grad:
            grads = torch.empty(8, **plan.f32)   # d loss / d trans [0:3], d loss / d quat [4:8]
            plan.forward_backward(trans, quat, mask, occ, obs, scalars, grads)
        else:
            grads = None
            plan.forward(trans, quat, mask, occ, obs, scalars)
        ctx.model, ctx.mask, ctx.occ, ctx.grads = model, mask, occ, grads
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(trans, quat, scalars)   # by reference: an in-place edit before backward() raises, as for torch's ops
        loss = scalars[1]
        if model.fast_backward:
            loss = loss.as_subclass(_Loss)
        return loss, obs, scalars

    @staticmethod
    def backward(ctx, g_loss, g_obs, _g_scalars):
        t, q, scalars = ctx.saved_tensors
        if g_loss is None and g_obs is None:
            return None, None, None, None, None
        if g_obs is None:
            g = g_loss.to(torch.float32) * ctx.grads
            return g[0:3].reshape(1, 3), g[4:8].reshape(1, 4), None, None, None
        g = g_obs.to(torch.float32)
        if g_loss is not None:
            g = g - g_loss.to(torch.float32) * scalars[1] * scalars[1]  # d loss / d observation_n = -loss^2
        tg, qg = ctx.model._plan.backward(t, q, ctx.mask, ctx.occ, g.contiguous())
        return tg, qg, None, None, None


class _TrajRewards(torch.autograd.Function):
    """rewards(poses, quats) for the evaluated waypoints (ops.WaypointShardStep: with a process group the waypoints are sharded
    over the ranks; the only data-path collective is the all-reduce of the log-odds vector)."""

    @staticmethod
    def forward(ctx, poses, quats, model):
        p, q = poses.detach().contiguous(), quats.detach().contiguous()
        st = model._waypoint_step(p.shape[0])
        ps, qs = p[st.lo:st.hi].clone(), q[st.lo:st.hi].clone()  # own copies: the step's inputs, whatever happens to the Parameters
        # occlusion masks are piecewise constant in the poses: computed per forward, not differentiated
        occ = model._own_occlusion_rows(st, p, q)
        lo_sum, rewards, _ = st.forward(ps, qs, occ, prior=model._prior)
        ctx.step, ctx.occ, ctx.gen, ctx.prior = st, occ, st.ws.generation, model._prior
        ctx.save_for_backward(ps, qs, lo_sum)
        return rewards

    @staticmethod
    def backward(ctx, grad_rewards):
        ps, qs, lo_sum = ctx.saved_tensors
        st = ctx.step
        upstream = dict(grad_rewards=grad_rewards.to(torch.float32).contiguous()) if st.hi > st.lo else None
        pg, qg = st.backward(ps, qs, ctx.occ, ctx.gen, lo_sum, upstream, prior=ctx.prior)
        return pg.contiguous(), qg.contiguous(), None


def _regularizers(model, p_all, scalars, clr_terms=None):
    """criterion()'s terms on the device after the visibility step that left `scalars` -> (terms[8]: vis, l2, length, smooth, total,
    ...; reg_sum (W,3): the gradient of the regularisers' sum; reg_terms (3,W,3): the gradient of each).  clr_terms (W float64, the
    clearance query's per-waypoint terms): terms[5] = clearance, and the total is the five-term sum rounded once, as on every path."""
    W, dev = p_all.shape[0], p_all.device
    terms = torch.empty(8, dtype=torch.float32, device=dev)
    reg_sum = torch.empty((W, 3), dtype=torch.float32, device=dev)
    reg_terms = torch.empty((3, W, 3), dtype=torch.float32, device=dev)
    args = (ptr(p_all), ptr(model.poses0), W, float(model.smoothness_weight), float(model.traj_length_weight), float(model.eps),
            ptr(scalars), ptr(terms), ptr(reg_sum), 0, None, ptr(reg_terms))
    L = _lib.lib()
    fn, extra = ((L.tohip_traj_regularizers, ()) if clr_terms is None else
                 (L.tohip_traj_regularizers_clearance, (float(model.clearance_weight), ptr(clr_terms))))
    with torch.cuda.device(dev):
        check(fn(*args, *extra, stream_ptr()), fn.__name__)
    return terms, reg_sum, reg_terms


def _assemble_grads(step_w, W, pg_e, qg_e, g_loss, g_terms, reg_sum, reg_terms, clr_rows=None, g_clr=None):
    """(W,3) / (W,4) gradients: the evaluated rows pg_e, qg_e (every step_w-th waypoint; None when the visibility term carries no
    gradient) plus the regularisers' share.  g_terms = (g_l2, g_length, g_smooth): upstream gradients of the single entries of
    model.loss, or all None.  clr_rows: the clearance term's gradient rows (None: the term is off), g_clr the upstream gradient of
    its entry.  dL/d loss alone: vis + g_loss (regularisers + clearance), the order of the one-call step (tohip_traj_opt_step)."""
    if clr_rows is not None and g_clr is None and all(g is None for g in g_terms):
        reg_sum, clr_rows = reg_sum + clr_rows, None
    grads = torch.zeros((W, 7), dtype=torch.float32, device=reg_sum.device)
    if pg_e is not None:
        rows = slice(0, (pg_e.shape[0] - 1) * step_w + 1, step_w)
        grads[rows, :3], grads[rows, 3:] = pg_e, qg_e
    pg_all, qg_all = grads[:, :3], grads[:, 3:]
    if all(g is None for g in g_terms):
        if g_loss is not None:
            pg_all = pg_all + g_loss * reg_sum
    else:
        for k, g in enumerate(g_terms):
            c = g_loss if g is None else (g.to(torch.float32) if g_loss is None else g_loss + g.to(torch.float32))
            if c is not None:
                pg_all = pg_all + c * reg_terms[k]
    if clr_rows is not None:
        c = g_loss if g_clr is None else (g_clr.to(torch.float32) if g_loss is None else g_loss + g_clr.to(torch.float32))
        if c is not None:
            pg_all = pg_all + c * clr_rows
    return pg_all.contiguous(), qg_all.contiguous()


class _Clearance(torch.autograd.Function):
    """The clearance term of the op-by-op criterion: poses (W,3) -> weight x sum (r - d)^2 (clearance_kernels.hip; its analytic
    gradient rows are taken by the same launch)."""

    @staticmethod
    def forward(ctx, poses, model):
        rows = torch.empty((poses.shape[0], 3), dtype=torch.float32, device=poses.device)
        if model.clearance_mode == "segments":
            value = ops.clearance_segments(model._clearance_source, poses.detach(), model.clearance_radius, model.clearance_weight, grad=rows,
                                           want_value=True)[3].reshape(())
        else:
            _, _, value = ops.clearance(model._clearance_source, poses.detach(), model.clearance_radius, model.clearance_weight, grad=rows,
                                        want_value=True)
        ctx.save_for_backward(rows)
        return value

    @staticmethod
    def backward(ctx, g):
        rows, = ctx.saved_tensors
        return (g.to(torch.float32) * rows).contiguous(), None


def _vis_upstream(g_loss, g_vis, g_rewards, scalars):
    """Keyword arguments of ops.traj_backward for the upstream gradients of (loss, loss['vis'], rewards); None: no gradient."""
    c_vis = g_vis if g_loss is None else (g_loss if g_vis is None else g_loss + g_vis)  # the visibility term enters the total with weight 1
    if c_vis is None and g_rewards is None:
        return None
    if g_rewards is None:
        return dict(scalars=scalars, gout=c_vis.reshape(1).contiguous())  # fused visibility loss, read on the device
    g = g_rewards.to(torch.float32)
    if c_vis is not None:
        g = g + c_vis * scalars[2]  # d loss_vis / d reward_n = -vis^2 / N
    return dict(grad_rewards=g.contiguous())


def _f32(g):
    return None if g is None else g.to(torch.float32)


class _TrajLoss(torch.autograd.Function):
    """ModelTraj.forward in one autograd node: (poses, quats) -> (loss, rewards, vis, l2, length, smooth), for a sharded and / or
    occlusion-aware model (the plain single-GPU model goes through _TrajLossPlan below: one library call per direction).

    The model's visibility step, then criterion's regularisers with their analytic gradients — instead of the ~60 small torch
    kernels and as many autograd nodes the op-by-op criterion costs.  Every output stays differentiable, as in the reference.

    Waypoint placement (ops.WaypointShardStep: visibility forward, [all-reduce], reward): `loss.backward()` takes the fused
    visibility-loss path; a loss built on model.rewards or on single entries of model.loss back-propagates through the general
    dL/d rewards path and the per-term regulariser gradients.

    Point placement (ops.PointShardStep: this rank's part of the cloud, every waypoint, two small collectives inside the
    forward): the forward has the gradient of the visibility loss in hand when it returns (the sums are taken with unit upstream
    gradient), so the backward issues no kernel and no collective: it scales.  Loss, loss terms and gradients are identical on
    every rank; `rewards` are this rank's rows.  A loss built on model.rewards would need the other ranks' upstream gradients per
    point: not supported (raises)."""

    @staticmethod
    def forward(ctx, poses, quats, model, step_w):
        W = poses.shape[0]
        n_eval = (W + step_w - 1) // step_w
        if model._shard.kind == "points":
            if not (poses.is_contiguous() and quats.is_contiguous() and poses.dtype == torch.float32 and quats.dtype == torch.float32):
                raise RuntimeError("ModelTraj: poses / quats must be contiguous float32 tensors")
            p_all = poses.detach()
            st = model._point_step(n_eval)
            rewards, scalars, pg_e, qg_e = st.step(p_all, quats.detach(), flags_extra=((step_w - 1) & 0xffff) << 8)   # every step_w-th waypoint, read in place
            model._mean_reward = scalars[0].clone()   # of ALL points, identical on every rank (model.mean_reward)
            rewards, saved = rewards.clone(), (pg_e.clone(), qg_e.clone())   # the step's buffers are the next step's
        else:
            p_all, q_all = poses.detach().contiguous(), quats.detach().contiguous()
            st = model._waypoint_step(n_eval)
            p_eval = p_all[::step_w].contiguous() if step_w > 1 else p_all
            q_eval = q_all[::step_w].contiguous() if step_w > 1 else q_all
            ps, qs = p_eval[st.lo:st.hi].clone(), q_eval[st.lo:st.hi].clone()  # own copies: the step's inputs, whatever happens to the Parameters
            occ = model._own_occlusion_rows(st, p_eval, q_eval)
            lo_sum, rewards, scalars = st.forward(ps, qs, occ, prior=model._prior)
            ctx.occ, ctx.gen, ctx.prior = occ, st.ws.generation, model._prior
            # a prior model that would take the one-call plan without its prior keeps the plan's gradient arithmetic (unit sums
            # scaled once per waypoint): a zero prior changes no bit
            ctx.unit_sums = not model._needs_split_step(prior=False)
            saved = (ps, qs, lo_sum, scalars)
        clr_rows = clr_terms = None
        if model._clearance_on:   # every rank: all W waypoints, the whole cloud
            clr_rows = torch.empty((W, 3), dtype=torch.float32, device=p_all.device)
            clr_terms = ops.clearance_terms(W, 1, model.clearance_mode, p_all.device)
            ops.clearance_rows(model._clearance_source, p_all, model.clearance_radius, model.clearance_weight, model.clearance_mode, 1, clr_rows, clr_terms)
        terms, reg_sum, reg_terms = _regularizers(model, p_all, scalars, clr_terms)
        ctx.step, ctx.step_w, ctx.W = st, step_w, W
        ctx.set_materialize_grads(False)
        vis, l2, length, smooth, total, clr = terms[:6].unbind()   # (clr: [5], written when the clearance term is on)
        ctx.has_clr = clr_rows is not None
        ctx.save_for_backward(reg_sum, reg_terms, *((clr_rows,) if ctx.has_clr else ()), *saved)
        return total, rewards, vis, l2, length, smooth, clr

    @staticmethod
    def backward(ctx, g_loss, g_rewards, g_vis, g_l2, g_length, g_smooth, g_clr):
        st = ctx.step
        reg_sum, reg_terms, *saved = ctx.saved_tensors
        clr_rows = saved.pop(0) if ctx.has_clr else None
        g_loss, g_vis = _f32(g_loss), _f32(g_vis)
        if isinstance(st, ops.PointShardStep):
            if g_rewards is not None:
                raise NotImplementedError("ModelTraj(shard=PointShard()): the rewards are rank-local; a loss built on model.rewards is not "
                                          "supported with point sharding (use WaypointShard, or model.loss / the returned loss)")
            c_vis = g_vis if g_loss is None else (g_loss if g_vis is None else g_loss + g_vis)
            pg_e, qg_e = (None, None) if c_vis is None else (c_vis * saved[0], c_vis * saved[1])
        else:
            ps, qs, lo_sum, scalars = saved
            upstream = _vis_upstream(g_loss, g_vis, g_rewards, scalars) if st.hi > st.lo else None
            pg_e, qg_e = st.backward(ps, qs, ctx.occ, ctx.gen, lo_sum, upstream, prior=ctx.prior, unit_sums=ctx.unit_sums)
        pg, qg = _assemble_grads(ctx.step_w, ctx.W, pg_e, qg_e, g_loss, (g_l2, g_length, g_smooth), reg_sum, reg_terms, clr_rows, g_clr)
        return pg, qg, None, None


class _LossPlan:
    """A ModelTraj as the library sees it (struct tohip_traj_loss): built once per (model, waypoint step), it owns the step's
    workspace and scratch vectors, so that model() and loss.backward() are one library call each with five pointers."""

    def __init__(self, model, step_w):
        L = _lib.lib()
        dev, cloud, rig = model.device, model._cloud, model._rig
        W = model.poses.shape[0]
        C = rig.n_cams if rig is not None else 1
        self.n, self.W, self.step_w = cloud.n, W, step_w
        self.n_eval = (W + step_w - 1) // step_w
        self.ws = model._workspace(self.n_eval)
        nbytes = L.tohip_traj_loss_scratch_bytes(cloud.n, W, step_w, C)
        self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        off = (ctypes.c_int64 * 8)()
        check(L.tohip_traj_loss_scratch_layout(cloud.n, W, step_w, C, off), "tohip_traj_loss_scratch_layout")

        def view(i, count, shape):
            return self.scratch[off[i]:off[i] + 4 * count].view(torch.float32).view(shape)
        self.poses_e, self.quats_e = view(0, 3 * self.n_eval, (self.n_eval, 3)), view(1, 4 * self.n_eval, (self.n_eval, 4))
        self.lo_sum, self.scalars = view(2, cloud.npad, (cloud.npad,)), view(4, 4, (4,))
        self.reg_sum = view(7, 3 * W, (W, 3))
        self.reg_terms = torch.empty((3, W, 3), dtype=torch.float32, device=dev)
        self.poses0 = model.poses0.contiguous()
        c = _lib.TrajLoss()
        c.packed, c.n_points, c.n_wps, c.wps_step, c.flags = cloud.blob.data_ptr(), cloud.n, W, step_w, int(model._flags)
        c.cam = model._cam.c
        if rig is not None:
            c.rig = rig.c
        c.poses0 = self.poses0.data_ptr()
        c.smoothness_weight, c.traj_length_weight = float(model.smoothness_weight), float(model.traj_length_weight)
        c.workspace, c.workspace_bytes = self.ws.buf.data_ptr(), self.ws.bytes
        c.scratch, c.scratch_bytes = self.scratch.data_ptr(), nbytes
        c.reg_terms = self.reg_terms.data_ptr()
        self.clr_rows = self.clr_fill = None
        if model._clearance_on:   # the clearance term: its gradient rows (W,3) lead the plan's clearance scratch
            if model.clearance_mode == "segments":   # the swept term: the flag bit and the larger scratch (rows and terms where they were)
                c.flags |= ops.CLEARANCE_SEGMENTS
                cb = L.tohip_traj_clearance_segments_scratch_bytes(W, 1)
            else:
                cb = L.tohip_traj_clearance_scratch_bytes(W, 1)
            self.clr_scratch = torch.empty(cb, dtype=torch.uint8, device=dev)
            self.clr_rows = self.clr_scratch[:12 * W].view(torch.float32).view(W, 3)
            c.clearance_radius, c.clearance_weight = float(model.clearance_radius), float(model.clearance_weight)
            c.clearance_scratch, c.clearance_scratch_bytes = self.clr_scratch.data_ptr(), cb
            if model._clr_map is not None:   # the map's term: forward() fills the scratch itself, the library launches no query
                c.flags |= ops.CLEARANCE_PREFILLED
                self.clr_fill = ops.clearance_scratch_views(self.clr_scratch, W)
        self.c, self.ref = c, ctypes.byref(c)
        self.model = model
        self.fwd, self.bwd, self.refresh = L.tohip_traj_loss_forward, L.tohip_traj_loss_backward, L.tohip_traj_loss_refresh
        self.sums_stale = False   # True: a general backward (tohip_traj_backward) has overwritten the unit-gradient pair sums
        self.dev_index = _lib.device_index(dev)
        self.dev = dev
        self.f32 = dict(dtype=torch.float32, device=dev)
        self.one = torch.ones((), **self.f32)   # dL/d loss of a plain loss.backward()

    def forward(self, poses, quats, rewards, terms):
        self.ws.generation += 1
        self.sums_stale = False
        if self.clr_fill is not None:   # the map as it is now: its rows and terms for these poses, on the stream of the call below
            m = self.model
            ops.clearance_rows(m._clr_map, poses, m.clearance_radius, m.clearance_weight, m.clearance_mode, 1, *self.clr_fill)
        rc = _lib.on_device(self.dev_index, self.fwd, self.ref, poses.data_ptr(), quats.data_ptr(), rewards.data_ptr(), terms.data_ptr())
        if rc:
            check(rc, "tohip_traj_loss_forward")
        return self.ws.generation

    def rebuild(self, poses, quats, versions):
        """The state of an earlier step, after another forward has used the workspace: possible while its inputs are unchanged."""
        if poses._version != versions[0] or quats._version != versions[1]:
            raise RuntimeError("ModelTraj: backward() of a loss whose model has been evaluated again AND whose poses / quats have been "
                               "modified by an inplace operation since: the step's state is gone (call backward() before the next "
                               "model(), or before optimizer.step())")
        return self.forward(poses, quats, torch.empty(self.n, **self.f32), torch.empty(8, **self.f32))

    def backward(self, gout, pg, qg):
        if self.sums_stale:
            # a backward through model.rewards / single loss terms of this step ran before: it left ITS sums (scaled by its
            # upstream gradient) where this one expects the unit-gradient ones — take them again (same pairs, same bits)
            rc = _lib.on_device(self.dev_index, self.refresh, self.ref)
            if rc:
                check(rc, "tohip_traj_loss_refresh")
            self.sums_stale = False
        rc = _lib.on_device(self.dev_index, self.bwd, self.ref, gout.data_ptr(), pg.data_ptr(), qg.data_ptr())
        if rc:
            check(rc, "tohip_traj_loss_backward")


class _FastBackward:
    """What `loss.backward()` needs when `loss` is exactly what model() returned and nothing else is asked for: the plan, the
    Parameters and their versions.  torch's autograd engine hands a HIP graph to a worker thread and waits for it (40-80 us per
    call for these two small tensors); this does what that thread would do — one library call, gradients accumulated into
    .grad — on the calling thread.  Anything beyond the plain call goes through the engine."""
    __slots__ = ("plan", "gen", "node", "params", "versions", "done")

    def __init__(self, plan, gen, node, params):
        self.plan, self.gen, self.node, self.params, self.done = plan, gen, node, params, False
        self.versions = (params[0]._version, params[1]._version)

    def usable(self, loss):
        p, q = self.params
        # (hooks registered on the Parameters' AccumulateGrad NODES — DDP does that — cannot be seen from Python: set
        # model.fast_backward = False under such wrappers)
        return (loss.grad_fn is self.node and loss._backward_hooks is None and not loss.retains_grad and
                p.requires_grad and q.requires_grad and p._backward_hooks is None and q._backward_hooks is None and
                getattr(p, "_post_accumulate_grad_hooks", None) is None and getattr(q, "_post_accumulate_grad_hooks", None) is None and
                (p.grad is None or _plain_grad(p)) and (q.grad is None or _plain_grad(q)) and not torch.is_anomaly_enabled())

    def compute(self):
        """-> the two gradients for dL/d loss = 1 (ModelTraj)."""
        plan = self.plan
        p, q = self.params
        if plan.ws.generation != self.gen:   # model() ran again since: rebuild this step's state
            self.gen = plan.rebuild(p, q, self.versions)
        pg, qg = torch.empty((plan.W, 3), **plan.f32), torch.empty((plan.W, 4), **plan.f32)
        plan.backward(plan.one, pg, qg)
        return pg, qg

    def run(self, retain_graph):
        if self.done:
            raise RuntimeError("Trying to backward through the graph a second time (or directly access saved tensors after they have "
                               "already been freed). Specify retain_graph=True if you need to backward through the graph a second time.")
        p, q = self.params
        pg, qg = self.compute()
        with torch.no_grad():
            if p.grad is None:
                p.grad = pg
            else:
                p.grad.add_(pg)
            if q.grad is None:
                q.grad = qg
            else:
                q.grad.add_(qg)
        if not retain_graph:
            self.done = True


class _FastBackwardPose(_FastBackward):
    """The same for ModelPose: the forward's pass has taken the gradient of the fused loss already.  The short cut is only taken
    while the Parameters are what the forward saw (else torch's engine raises its in-place error, as it would for torch's ops)."""
    __slots__ = ("grads",)

    def __init__(self, plan, node, params, grads):
        super().__init__(plan, 0, node, params)
        self.grads = grads

    def usable(self, loss):
        p, q = self.params
        return self.grads is not None and p._version == self.versions[0] and q._version == self.versions[1] and super().usable(loss)

    def compute(self):
        g = self.grads
        return g[0:3].reshape(1, 3).clone(), g[4:8].reshape(1, 4).clone()


def _plain_grad(p):
    g = p.grad
    return g.dtype == torch.float32 and g.device == p.device and g.shape == p.shape and not g.requires_grad and not g.is_sparse


class _Loss(torch.Tensor):
    """The 0-d loss ModelTraj.forward returns: an ordinary tensor (same storage, same autograd node) whose plain
    `.backward()` skips the autograd engine's thread hand-off (_FastBackward); every other use is torch's."""
    __torch_function__ = torch._C._disabled_torch_function_impl

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        fast = self.__dict__.get("_tohip_fast")
        if fast is not None and gradient is None and inputs is None and not create_graph and fast.usable(self):
            return fast.run(retain_graph)
        return super().backward(gradient, retain_graph, create_graph, inputs)


class _TrajLossPlan(torch.autograd.Function):
    """ModelTraj.forward of a single-GPU model without occlusion rows: (poses, quats) -> (loss, rewards, vis, l2, length, smooth)
    with ONE library call in each direction (tohip_traj_loss_forward / _backward over the model's _LossPlan) and no torch kernel
    besides: the reference's `zero_grad(); loss = model(); loss.backward(); step()` loop is bound by the host on this chip.
    The backward reads the state its forward left in the plan's workspace (records, flags, regulariser gradients), not the
    Parameters: editing them in place after model() — optimizer.step() — does not disturb it.  A backward that arrives after
    ANOTHER forward of the same model re-runs its own forward first (same inputs, same bits), which needs the inputs unchanged.
    Upstream gradients other than dL/d loss (model.rewards, single entries of model.loss) take the general kernels."""

    @staticmethod
    def forward(ctx, poses, quats, plan):
        if not (poses.is_contiguous() and quats.is_contiguous() and poses.dtype == torch.float32 and quats.dtype == torch.float32):
            raise RuntimeError("ModelTraj: poses / quats must be contiguous float32 tensors")
        rewards = torch.empty(plan.n, **plan.f32)
        terms = torch.empty(8, **plan.f32)
        ctx.gen = plan.forward(poses, quats, rewards, terms)
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        ctx.inputs, ctx.versions = (poses, quats), (poses._version, quats._version)
        ctx.save_for_backward(plan.one)   # nothing of it is needed: a second backward() without retain_graph raises like torch's ops
        vis, l2, length, smooth, total, clr = terms[:6].unbind()   # (clr: [5], written when the clearance term is on)
        if plan.model.fast_backward:
            total = total.as_subclass(_Loss)   # made here: an alias made outside would be one more autograd node
        return total, rewards, vis, l2, length, smooth, clr

    @staticmethod
    def backward(ctx, g_loss, g_rewards, g_vis, g_l2, g_length, g_smooth, g_clr):
        plan = ctx.plan
        ctx.saved_tensors
        if plan.ws.generation != ctx.gen:   # model() ran again since: rebuild this step's state (rewards / loss terms to spare vectors)
            ctx.gen = plan.rebuild(ctx.inputs[0], ctx.inputs[1], ctx.versions)
        if g_rewards is None and g_vis is None and g_l2 is None and g_length is None and g_smooth is None and g_clr is None:
            if g_loss is None:
                return None, None, None
            if g_loss.dtype != torch.float32 or g_loss.device != plan.dev:
                g_loss = g_loss.to(**plan.f32)
            pg, qg = torch.empty((plan.W, 3), **plan.f32), torch.empty((plan.W, 4), **plan.f32)
            plan.backward(g_loss, pg, qg)
            return pg, qg, None
        m = plan.model
        g_loss = _f32(g_loss)
        pg = qg = None
        kw = _vis_upstream(g_loss, _f32(g_vis), g_rewards, plan.scalars)
        if kw is not None:
            pg, qg = ops.traj_backward(m._cloud, plan.n_eval, m._cam, plan.ws, plan.lo_sum, rig=m._rig, flags=m._flags, **kw)
            plan.sums_stale = True   # the pair sums in the workspace are now scaled by THIS upstream gradient
        pg_all, qg_all = _assemble_grads(plan.step_w, plan.W, pg, qg, g_loss, (g_l2, g_length, g_smooth), plan.reg_sum, plan.reg_terms,
                                         plan.clr_rows, g_clr)
        return pg_all, qg_all, None


# ------------------------------------------------------------------------------ models

def _adopt_cloud(points, cloud, device, sort, model_cls):
    """The packed cloud a model's constructor adopts: `points` may be an ops.PackedCloud, or `cloud=` names one (or a model of
    `model_cls` whose cloud to share), packed with sort=`sort` on `device`.  -> (the cloud, its points), or (None, points) when there
    is none to adopt."""
    if isinstance(points, ops.PackedCloud):
        cloud, points = points, None
    if isinstance(cloud, model_cls):
        cloud = cloud._cloud
    if cloud is None:
        return None, points
    if not isinstance(cloud, ops.PackedCloud) or cloud.sorted != sort:
        order = "Morton order (sort=True)" if sort else "the caller's order (sort=False)"
        raise ValueError(f"cloud= must be an ops.PackedCloud in {order} or a {model_cls.__name__}")
    if cloud.device != torch.device(device.type, _lib.device_index(device)):
        raise ValueError(f"the packed cloud lives on {cloud.device}, the model on {device}")
    if points is not None and not (torch.is_tensor(points) and points.data_ptr() == cloud.points.data_ptr() and
                                   tuple(points.shape) == tuple(cloud.points.shape) and points.stride() == cloud.points.stride()):
        # a different tensor object: it must hold the packed cloud's rows (an equal-sized OTHER cloud would silently be replaced by
        # cloud.points otherwise); the comparison is one pass over the rows, paid only by callers who hand both
        pt = torch.as_tensor(points, dtype=torch.float32)
        if tuple(pt.shape) != tuple(cloud.points.shape) or not torch.equal(pt.to(cloud.points.device), cloud.points):
            raise ValueError("cloud= does not hold these points")
    return cloud, cloud.points


def _occlusion_grid(occlusion, grid, voxel, cloud):
    """The occupancy grid of a model with occlusion='voxel': `grid` (an ops.OccupancyGrid on the cloud's device: the map so far, walls
    of earlier clouds included) or, for None, one built here from the cloud's own points at resolution `voxel`.  None for every other
    method, which takes no grid."""
    if occlusion != "voxel":
        if grid is not None:
            raise ValueError(f"occlusion_grid needs occlusion='voxel', got occlusion={occlusion!r}")
        return None
    return ops.OccupancyGrid.from_points(cloud, resolution=voxel) if grid is None else ops.check_occlusion_grid(grid, cloud)


class ModelPose(nn.Module):
    """Single camera pose optimisation model (/root/reference/src/model.py:65-127).

    Extra keyword arguments (absent from the reference): `occlusion='hpr'|'zbuffer'` hides from the pose the points its own camera
    does not see — ModelTraj's per-waypoint rows for this one pose: the cloud in the camera frame (normalised quaternion), the hard
    frustum cull with `occlusion_limits`, then HPR from the camera centre (or the z-buffer splat), as in
    /root/reference/src/pc_processor.py:158-187; observations[n] = dist_mask * fov_mask * bit[n].  The row carries no gradient and is
    rebuilt on every `occlusion_refresh_every`-th forward (ModelTraj's policy).  forward(hpr=True) keeps the reference's world-frame
    HPR from the world origin (model.py:112-115) and cannot be combined with `occlusion`.
    `occlusion='voxel'` walks an occupancy grid from the camera to each kept point instead (ops.OccupancyGrid: `occlusion_grid=`, the
    map so far, or a grid of the model's own points at `occlusion_voxel` metres, built on construction).
    """

    def __init__(self,
                 points: torch.tensor,   # the cloud, (N, 3), world frame
                 trans0: torch.tensor,   # initial camera position, shape (1, 3)
                 q0: torch.tensor,       # initial camera orientation, shape (1, 4), scalar part first
                 intrins: torch.tensor,  # pinhole matrix K, shape (3, 3)
                 img_width, img_height,
                 min_dist=1.0, max_dist=5.0,
                 device=torch.device('cuda:0'), *, cloud=None, fast_adam=False, occlusion=None, occlusion_limits=(1.0, 15.0),
                 occlusion_refresh_every=1, occlusion_grid=None, occlusion_voxel=0.1):
        super().__init__()
        assert trans0.size() == torch.Size([1, 3])
        assert q0.size() == torch.Size([1, 4])
        assert intrins.size() == torch.Size([3, 3])

        self.device = torch.device(device)
        # One packed cloud for several poses (many starts of one camera, optimizer.optimize_poses).  The pose path keeps the caller's
        # order, so only an unsorted cloud (sort=False) will do: another order would change the sums.
        cloud, points = _adopt_cloud(points, cloud, self.device, False, ModelPose)
        # the reference keeps the caller's dtype (model.py:80) and then fails in get_fov_mask's matmul
        # for anything but float32; float32 is the contract here
        self.points = points if cloud is not None else torch.as_tensor(points, dtype=torch.float32).to(self.device)
        self.rewards = None
        self.observations = None
        self.lo_sum = 0.0

        trans = torch.as_tensor(trans0, dtype=torch.float32).to(self.device)
        self.trans = nn.Parameter(trans)
        quat = torch.as_tensor(q0, dtype=torch.float32).to(self.device)
        self.quat = nn.Parameter(quat)

        self.K = torch.as_tensor(intrins, dtype=torch.float32).to(self.device)
        self.img_width, self.img_height = float(img_width), float(img_height)
        self.eps = 1e-6
        self.pc_clip_limits = [min_dist, max_dist]  # near / far range of the distance mask, metres

        self.to(self.device)
        # nothing culls here: the caller's order, masks and observations in place
        self._cloud = cloud if cloud is not None else ops.PackedCloud(self.points, sort=False)
        self._cam = ops.Camera(self.K, self.img_width, self.img_height, min_dist, max_dist, self.eps)
        self._ws = ops.PoseWorkspace(self._cloud)
        self._occlusion_mask, self._occlusion_key = None, None
        self._occlusion, self._occlusion_limits = ops.check_occlusion(occlusion), occlusion_limits
        self._occlusion_grid, self._occlusion_voxel = _occlusion_grid(occlusion, occlusion_grid, occlusion_voxel, self._cloud), occlusion_voxel
        # The pose's occlusion row is piecewise constant in the pose and carries no gradient; building it (a hard cull and a convex
        # hull, or a z-buffer) costs many plain steps.  Rebuilt on the first forward and on every occlusion_refresh_every-th one after
        # (k = 1: every forward), reused in between; refresh_occlusion() forces a rebuild at the next forward.
        self.occlusion_refresh_every = max(1, int(occlusion_refresh_every))
        self._occ_cache = None    # (row (1, npad/32) int32, forwards since it was built)
        self.occlusion_rebuilds = 0   # full rebuilds: bookkeeping for tools and tests
        self.fused_loss = True  # forward() as one autograd node; False (or an overridden criterion): observations node + torch ops
        self.fast_backward = True   # a plain `loss.backward()` on what forward() returned runs on the calling thread
        self._plan = ops.PosePlan(self._cloud, self._cam, self._ws)
        for p in (self.trans, self.quat):
            tag_parameter(p)   # torch.optim.Adam.step() MAY update them with one launch — once the caller opts in:
        if fast_adam:          # fast_adam=True here, optimizer.accelerate_torch_adam(True) or accelerate_torch_adam(opt) (nothing is hooked otherwise)
            accelerate_torch_adam(True)

    @classmethod
    def sharing_cloud_of(cls, other, trans0, q0, **kw):
        """A model of another start over `other`'s cloud: same packed cloud (not packed again), camera and device; keyword
        arguments as the constructor's."""
        kw.setdefault("device", other.device)
        kw.setdefault("min_dist", other.pc_clip_limits[0])
        kw.setdefault("max_dist", other.pc_clip_limits[1])
        kw.setdefault("occlusion", other._occlusion)
        kw.setdefault("occlusion_limits", other._occlusion_limits)
        kw.setdefault("occlusion_refresh_every", other.occlusion_refresh_every)
        if kw["occlusion"] == "voxel":   # (the same grid object, not one more built from the same points)
            kw.setdefault("occlusion_grid", other._occlusion_grid)
            kw.setdefault("occlusion_voxel", other._occlusion_voxel)
        return cls(other._cloud, trans0, q0, other.K, other.img_width, other.img_height, **kw)

    def refresh_occlusion(self):
        """The next forward rebuilds the occlusion row whatever occlusion_refresh_every says."""
        self._occ_cache = None

    def _occlusion_row(self):
        """The pose's occlusion bit row for this forward: rebuilt from the current pose on every occlusion_refresh_every-th call,
        reused otherwise."""
        c = self._occ_cache
        age = _refresh_age(c[1] if c is not None else None, self.occlusion_refresh_every)
        if age == 1:
            row = self._build_occlusion_rows(self.trans.detach().contiguous(), self.quat.detach().contiguous())
            self.occlusion_rebuilds += 1
        else:
            row = c[0]
        self._occ_cache = (row, age)
        return row

    def _adopt_occlusion_row(self, row, age, rebuilds):
        """What a launch-only loop (optimizer.optimize_pose / optimize_poses) leaves in the cache: its last row, the number of steps
        that used it, and its rebuilds counted — so the model's next forwards continue the loop's schedule as if its steps had been
        forwards of the model."""
        self._occ_cache = (row, age)
        self.occlusion_rebuilds += rebuilds

    def _build_occlusion_rows(self, trans, quat):
        """(B, npad/32) occlusion bit rows of B poses of this camera over this cloud, in one batched pass (B = 1 for the model's own)."""
        return ops.occlusion_bits(self._cloud, self.points, trans, quat, self._cam, self._occlusion_limits[0], self._occlusion_limits[1],
                                  self._occlusion, grid=self._occlusion_grid)

    def _hpr_mask(self):
        """HPR of the WORLD-frame cloud seen from the world origin (model.py:114): pose independent, so it is computed once per
        cloud and cached; a replaced or edited cloud gets a new mask."""
        key = (self.points.data_ptr(), self.points._version, tuple(self.points.shape))
        if self._occlusion_mask is None or self._occlusion_key != key:
            self._occlusion_mask = hidden_pts_removal(self.points.detach(), device=self.device)[1].contiguous()
            self._occlusion_key = key
        return self._occlusion_mask

    def forward(self, debug=False, hpr=False):
        t0 = time()
        if hpr and self._occlusion is not None:
            raise ValueError("hpr=True (the reference's world-frame mask) and occlusion= (the pose's own) exclude each other")
        mask = self._hpr_mask() if hpr else None
        occ = self._occlusion_row() if self._occlusion is not None else None
        fused = self.fused_loss and type(self).criterion is ModelPose.criterion
        if fused:
            loss, self.observations, scalars = _PoseLoss.apply(self.trans, self.quat, self, mask, occ)
            if type(loss) is _Loss and loss.requires_grad:
                loss.__dict__["_tohip_fast"] = _FastBackwardPose(self._plan, loss.grad_fn, (self.trans, self.quat), loss.grad_fn.grads)
        else:
            self.observations = _PoseObservations.apply(self.trans, self.quat, self, mask, occ)
        if debug:
            torch.cuda.synchronize(self.device)
            print(f'Visibility estimation took: {1000 * (time() - t0)} msec')
            print(f'Point cloud size {self.points.size()}')
        if not fused:
            loss = self.criterion(self.observations)
        return loss

    def criterion(self, observations):
        # the more (softly) observed points, the smaller the loss: reciprocal of their sum (/root/reference/src/model.py:124-127)
        loss = 1. / (torch.sum(observations) + self.eps)
        return loss


class _NoShard:
    """Single-process placement: every waypoint is local, no collective (distributed.WaypointShard's surface)."""
    kind, world_size, rank, collective, compact = "waypoints", 1, 0, False, False

    @staticmethod
    def bounds(n, rank=None):
        return 0, n

    @staticmethod
    def allreduce_sum(t):
        return t

    allreduce_max = allreduce_sum


class ModelTraj(nn.Module):
    """Trajectory optimisation model (/root/reference/src/model.py:158-260).

    Extra keyword arguments (absent from the reference): `rig=(quats (C,4), trans (C,3))` evaluates a rigid
    multi-camera rig at every waypoint; `shard=` a trajectory_optimization_amd.distributed.WaypointShard
    placing the waypoints over the ranks of a process group (one process per GPU, RCCL); `dense=True`
    evaluates every (point, waypoint) pair instead of skipping the pairs that provably contribute nothing;
    `occlusion='hpr'|'zbuffer'` makes the reward occlusion-aware per waypoint — the reference's TODO
    (/root/reference/src/tools.py:61-62, /root/reference/src/model.py:210): each waypoint's camera-frame cloud goes
    through the hard pipeline of /root/reference/src/pc_processor.py:171-178 (frustum cull with `occlusion_limits`,
    then HPR from the camera centre) and the points it hides get p = 0 for that waypoint; `occlusion='voxel'` keeps the cull and
    walks an occupancy grid from the camera to each kept point instead (ops.OccupancyGrid: `occlusion_grid=`, the map so far — walls
    of earlier clouds included — or a grid of the model's own points at `occlusion_voxel` metres, built on construction);
    `prior_log_odds=` an (N,) tensor of what is already known of the map (OctoMap's accumulated log-odds, >= 0, in the caller's point
    order): rewards become sigmoid(lo_sum + prior) — see the prior_log_odds property and coverage_log_odds().  An ops.CoverageMap is
    accepted in its place: the prior is its lookup over this cloud (commit_coverage folds a plan back into it).
    `clearance_map=` an ops.OccupancyGrid, SpaceMap or EvidenceMap: the clearance term keeps the path off the map's occupied voxels
    (`clearance_unknown='obstacle'`: and its never-seen ones) instead of off `points`; the map is read as it is at every step.
    """

    def __init__(self,
                 points: torch.tensor,     # the cloud, (N, 3), world frame
                 wps_poses: torch.tensor,  # waypoint positions, (W, 3), one row per waypoint
                 wps_quats: torch.tensor,  # waypoint orientations, (W, 4), scalar part first
                 intrins: torch.tensor,    # pinhole matrix K, shape (3, 3)
                 img_width, img_height,
                 min_dist=1.0, max_dist=5.0,
                 smoothness_weight=14.0, traj_length_weight=0.02,
                 device=torch.device('cuda'),
                 *, rig=None, shard=None, dense=False, occlusion=None, occlusion_limits=(1.0, 15.0), occlusion_refresh_every=1,
                 occlusion_refresh_tol=None, occlusion_check_every=5, n_points_global=None, cloud=None, fast_adam=False,
                 clearance_radius=None, clearance_weight=0.0, prior_log_odds=None, clearance_mode='waypoints', occlusion_grid=None,
                 occlusion_voxel=0.1, clearance_map=None, clearance_unknown='free'):
        super().__init__()
        # the clearance term (clearance_kernels.hip): weight x sum over ALL waypoints of (r - d)^2, d = the distance to the nearest
        # cloud point within r — it keeps the path off the cloud; weight 0 (the default): off, the reference's criterion as it is.
        # clearance_mode 'segments': d = the distance from each SEGMENT between consecutive waypoints to its nearest point, so the
        # straight line driven between two waypoints stays off the cloud as well
        self._clr_points_shard = shard is not None and shard.kind == "points"
        self._clr = (None, 0.0)
        self._clr_mode = "waypoints"
        self.set_clearance(clearance_radius, clearance_weight, clearance_mode)
        # clearance_map= an ops.OccupancyGrid, SpaceMap or EvidenceMap: the term's obstacles are the map's voxels (their centres), read
        # at every step as the map is then, instead of this model's cloud; clearance_unknown='obstacle': never-seen voxels repel too
        self._clr_map = None
        self.set_clearance_map(clearance_map, clearance_unknown)
        assert wps_poses.dim() == wps_quats.dim()
        assert wps_poses.size()[1] == 3
        assert wps_quats.size()[1] == 4

        self.device = torch.device(device)
        self._n_global = None
        # One packed cloud for many models: the reference builds a model per (cloud, path) message pair over the same map
        # (/root/reference/src/trajectory_optimization.py:129-136); packing — bounding box, Morton sort, tile bounds — costs several
        # optimiser steps and 20 B/point.
        cloud, points = _adopt_cloud(points, cloud, self.device, True, ModelTraj)
        if cloud is not None:
            if shard is not None and shard.kind == "points":
                raise ValueError("a shared packed cloud holds the whole cloud: not available with PointShard")
            self.points = points
        elif shard is not None and shard.kind == "points":
            # point sharding: this rank keeps its own rows of the cloud (the whole cloud is handed in, or — n_points_global — the
            # rows already); model.rewards are those rows' rewards
            pts = torch.as_tensor(points, dtype=torch.float32)
            if n_points_global is None:
                self._n_global = int(pts.shape[0])
                lo_p, hi_p = shard.point_bounds(self._n_global)
                pts = pts[lo_p:hi_p]
            else:
                self._n_global = int(n_points_global)
            if occlusion is not None:
                raise ValueError("occlusion-aware rewards need the whole cloud on every rank: not available with PointShard")
            self.points = pts.contiguous().to(self.device)
        else:
            self.points = torch.as_tensor(points, dtype=torch.float32).to(self.device)
        self.rewards = None
        self._mean_reward = None
        self.observations = None
        self.lo_sum = 0.0  # attribute kept for the reference's surface (its accumulated log-odds); the kernels hold theirs in packed order

        self.poses0 = torch.as_tensor(wps_poses, dtype=torch.float32).to(self.device)  # the trajectory as given: criterion measures against it
        self.quats0 = torch.as_tensor(wps_quats, dtype=torch.float32).to(self.device)

        self.poses = nn.Parameter(deepcopy(self.poses0))
        self.quats = nn.Parameter(deepcopy(self.quats0))

        self.K = torch.as_tensor(intrins, dtype=torch.float32).to(self.device)
        self.img_width, self.img_height = float(img_width), float(img_height)
        self.eps = 1e-6
        self.pc_clip_limits = [min_dist, max_dist]  # near / far range of the distance mask, metres

        self.loss = {'vis': float('inf'),
                     'length': float('inf'),
                     'l2': float('inf'),
                     'smooth': float('inf')}
        self.smoothness_weight = smoothness_weight
        self.traj_length_weight = traj_length_weight

        self.to(self.device)
        self._cloud = cloud if cloud is not None else ops.PackedCloud(self.points)
        self._cam = ops.Camera(self.K, self.img_width, self.img_height, min_dist, max_dist, self.eps)
        self._rig = ops.CameraRig(rig[0], rig[1], self.device) if rig is not None else None
        self._shard = shard if shard is not None else _NoShard()
        self._flags = ops.DENSE if dense else 0  # dense: evaluate every pair (results are bitwise the same)
        self._occlusion, self._occlusion_limits = ops.check_occlusion(occlusion), occlusion_limits
        self._occlusion_grid, self._occlusion_voxel = _occlusion_grid(occlusion, occlusion_grid, occlusion_voxel, self._cloud), occlusion_voxel
        self._prior = None   # ops.LogOddsPrior (the property below)
        self.prior_log_odds = prior_log_odds
        # The occlusion masks are piecewise constant in the poses (a point is hidden from a waypoint or it is not) and carry no
        # gradient; building them — a hard cull and a convex hull (or a z-buffer) per waypoint — costs hundreds of plain steps.
        # occlusion_refresh_every = k: they are rebuilt on every k-th forward of the model (k = 1: every forward, the bits of a
        # model without the policy) and reused in between; refresh_occlusion() forces a rebuild at the next forward.
        # occlusion_refresh_tol = metres, or (metres, radians): the MOTION-triggered policy — every occlusion_check_every-th
        # forward looks (one small device-to-host read) whether a waypoint has moved or turned by more than that since ITS rows were
        # built; if one has, the rows of every waypoint beyond half the tolerance are rebuilt (one batched pass for them) and the
        # others kept: a waypoint that has converged stops paying.  occlusion_refresh_every stays the cap on a row's age.
        self.occlusion_refresh_every = max(1, int(occlusion_refresh_every))
        self._occ_cache = None   # (rows, shape key, forwards since the last FULL rebuild)
        self._occ_built = None   # the body poses each waypoint's rows were built for: (positions, normalised quaternions)
        self.occlusion_refresh_tol = occlusion_refresh_tol   # (property: a scalar becomes (metres, radians); setting it later restarts the policy)
        self.occlusion_check_every = max(1, int(occlusion_check_every))
        self.occlusion_rebuilds = [0, 0]   # (full rebuilds, waypoints rebuilt by the motion policy): bookkeeping for tools and tests
        self._ws_cache = {}
        self._plan_obj, self._plan_key = None, None
        self._wps_step_cache = {}
        self._length0 = None
        # forward() as ONE autograd node (visibility + criterion on the device); False: rewards node + the op-by-op
        # torch criterion below (always used when a subclass overrides criterion, or for fewer than 3 waypoints)
        self.fused_loss = True
        # a plain `loss.backward()` on what forward() returned runs on the calling thread (_FastBackward); False: always torch's engine
        self.fast_backward = True
        for p in (self.poses, self.quats):
            tag_parameter(p)   # torch.optim.Adam.step() MAY update them with one launch — once the caller opts in:
        if fast_adam:          # fast_adam=True here, optimizer.accelerate_torch_adam(True) or accelerate_torch_adam(opt) (nothing is hooked otherwise)
            accelerate_torch_adam(True)

    def set_clearance(self, radius, weight, mode=None):
        """The clearance term's settings (checked together: radius > 0 when weight > 0, both finite, mode 'waypoints' or 'segments' —
        None keeps the current one; ValueError otherwise).  Weight 0 switches the term off.  The next forward / optimiser run uses
        them."""
        r, w = ops.check_clearance(radius, weight)
        mode = ops.check_clearance_mode(self._clr_mode if mode is None else mode)
        if w > 0.0 and self._clr_points_shard:
            raise ValueError("the clearance term needs the whole cloud on every rank: not available with PointShard")
        self._clr, self._clr_mode = (r if w > 0.0 else radius, w), mode

    def set_clearance_map(self, map, unknown='free'):
        """The map whose voxels the clearance term keeps the path off (an ops.OccupancyGrid, SpaceMap or EvidenceMap; unknown 'free'
        or 'obstacle': ops.MapObstacles' rule, ValueError otherwise), or None: the model's own cloud again.  The model keeps the map
        object and reads its buffers at every step: an insert or an integrate between two steps is seen by the next one."""
        self._clr_map = ops.MapObstacles(map, unknown) if map is not None else None

    @property
    def clearance_map(self):
        return self._clr_map.map if self._clr_map is not None else None

    @property
    def _clearance_source(self):
        """What the clearance queries search: the map's obstacles when there is a clearance_map, the packed cloud otherwise."""
        return self._clr_map if self._clr_map is not None else self._cloud

    @property
    def clearance_mode(self):
        return self._clr_mode

    @clearance_mode.setter
    def clearance_mode(self, mode):
        self.set_clearance(self._clr[0], self._clr[1], mode)

    @property
    def clearance_radius(self):
        return self._clr[0]

    @clearance_radius.setter
    def clearance_radius(self, radius):
        self.set_clearance(radius, self._clr[1])

    @property
    def clearance_weight(self):
        return self._clr[1]

    @clearance_weight.setter
    def clearance_weight(self, weight):
        self.set_clearance(self._clr[0], weight)

    @property
    def _clearance_on(self):
        return self._clr[1] > 0.0

    @property
    def prior_log_odds(self):
        """The per-point log-odds prior (N,) f32 in the caller's order, or None.  Rewards are sigmoid(lo_sum + prior): lo_sum the sum
        over the evaluated waypoints as without it, the prior added last (a zero prior gives the bits of the model without one).
        Setting it checks the value (finite, >= 0, one entry per point, on the model's device: ValueError otherwise) and the next
        forward / optimiser run uses it; None returns the model to the path without a prior.  A prior model goes through the
        separate visibility calls (as an occlusion-aware one); not available with PointShard or optimize_trajectories."""
        return self._prior.values if self._prior is not None else None

    @prior_log_odds.setter
    def prior_log_odds(self, prior):
        if prior is None:
            self._prior = None
            return
        if self._shard.kind == "points":
            raise ValueError("prior_log_odds needs the whole cloud on every rank: not available with PointShard")
        # (a CoverageMap: its lookup over this cloud; checks the result: ops.check_prior)
        self._prior = ops.LogOddsPrior(self._cloud, ops.resolve_prior(prior, self._cloud))

    @torch.no_grad()
    def coverage_log_odds(self, upto=None, clamp_max=None, vis_wps_dist=0.5):
        """The fused log-odds map (N,) f32 in the caller's order: prior + lo_sum, lo_sum from the model's evaluated waypoints (every
        wps_step-th, as forward(vis_wps_dist) selects them) with index < upto (all when None) at their current poses, with their
        current occlusion rows when the model has them.  clamp_max: OctoMap's upper clamping threshold (>= 0; None: none).  Forward
        only.  This is the next plan's prior_log_odds: the coverage of the path flown so far, or of another robot's plan."""
        if self._shard.kind == "points":
            raise ValueError("coverage_log_odds needs the whole cloud: not available with PointShard")
        W = self.poses.shape[0]
        upto = W if upto is None else int(upto)
        if not 0 <= upto <= W:
            raise ValueError(f"upto must be in [0, {W}], got {upto}")
        step_w = self._wps_step(vis_wps_dist)
        ps = self.poses.detach()[0:upto:step_w].contiguous()
        qs = self.quats.detach()[0:upto:step_w].contiguous()
        cloud = self._cloud
        if ps.shape[0] > 0:
            occ = self._build_occlusion_rows(ps, qs) if self._occlusion is not None else None
            lo_sum, _ = ops.traj_forward(cloud, ps, qs, self._cam, self._workspace(ps.shape[0]), self._rig, flags=self._flags, occ=occ)
        else:
            lo_sum = torch.zeros(cloud.npad, dtype=torch.float32, device=cloud.device)
        return ops.traj_coverage(cloud, lo_sum, self._prior, clamp_max)

    def commit_coverage(self, coverage_map, upto=None, vis_wps_dist=0.5):
        """Fold what this plan has seen into an ops.CoverageMap: coverage_log_odds(upto, the map's clamp_max, vis_wps_dist) integrated
        over this model's points with mode 'max' (the row holds the prior, which a model built with prior_log_odds=map read from that
        map).  Any later cloud reads it back: ModelTraj(other_points, ..., prior_log_odds=coverage_map).  -> the map."""
        if self._shard.kind == "points" or self._shard.world_size > 1 or self._shard.collective:
            raise ValueError("commit_coverage: a sharded model (WaypointShard / PointShard) is not supported")
        return coverage_map.integrate(self, self.coverage_log_odds(upto, clamp_max=coverage_map.clamp_max, vis_wps_dist=vis_wps_dist), mode="max")

    @classmethod
    def sharing_cloud_of(cls, other, wps_poses, wps_quats, **kw):
        """A model of another trajectory over `other`'s cloud: same packed cloud (not packed again), camera and device; keyword
        arguments as the constructor's (weights, rig, dense, ...)."""
        kw.setdefault("device", other.device)
        kw.setdefault("min_dist", other.pc_clip_limits[0])
        kw.setdefault("max_dist", other.pc_clip_limits[1])
        if kw.get("occlusion") == "voxel" and other._occlusion_grid is not None:   # (the same grid object, not one more of the same points)
            kw.setdefault("occlusion_grid", other._occlusion_grid)
            kw.setdefault("occlusion_voxel", other._occlusion_voxel)
        if other._clr_map is not None and "clearance_map" not in kw:   # (the same map objects: what a batched or a team run demands)
            kw["clearance_map"] = other._clr_map.map
            kw.setdefault("clearance_unknown", other._clr_map.unknown)
        return cls(other._cloud, wps_poses, wps_quats, other.K, other.img_width, other.img_height, **kw)

    @property
    def mean_reward(self):
        """mean(rewards) over the WHOLE cloud after the last forward, as a 0-d tensor — what the reference's early-stop rule reads
        (`torch.mean(model.rewards) / reward0`, /root/reference/src/trajectory_optimization.py:119-122).  With point sharding
        model.rewards holds this rank's rows only and torch.mean of it differs from rank to rank: a loop that stops on it would
        leave the ranks at different steps, and the ones that go on would wait for ever in the next forward's collectives.  This is
        the replicated value (the all-reduced reward sum over the global point count); without point sharding it is
        torch.mean(model.rewards)."""
        if self._n_global is not None:
            return self._mean_reward
        return torch.mean(self.rewards.detach()) if self.rewards is not None else None

    def refresh_occlusion(self):
        """The next forward rebuilds the occlusion masks whatever occlusion_refresh_every says."""
        self._occ_cache = None

    @property
    def occlusion_refresh_tol(self):
        return self._occ_tol

    @occlusion_refresh_tol.setter
    def occlusion_refresh_tol(self, tol):
        """None, metres, or (metres, radians).  Public like occlusion_refresh_every: changing it after a forward drops the cached rows,
        so the next forward is a full rebuild that records the poses the motion policy compares against."""
        if tol is not None and not isinstance(tol, (tuple, list)):
            tol = (float(tol), 0.35 * float(tol))   # (1 rad turns a point 3 m away by 3 m)
        self._occ_tol = tuple(float(x) for x in tol) if tol is not None else None
        self._occ_cache, self._occ_built = None, None

    def _occlusion_rows(self, ps, qs):
        """Occlusion bit rows of the given body waypoints, one row per virtual waypoint v = w*C + c (with a rig: the cameras'
        own poses t_v = t_w + R(q_w) l_c, q_v = q_w/|q_w| (x) q_c — the composition the kernels apply).  Rebuilt as a whole on
        every occlusion_refresh_every-th call; with occlusion_refresh_tol set, in between, the rows of the waypoints that have
        moved (see the constructor); reused otherwise."""
        key = (tuple(ps.shape), tuple(qs.shape))
        c = self._occ_cache
        kept = c is not None and c[1] == key and (self.occlusion_refresh_tol is None or self._occ_built is not None)
        age = _refresh_age(c[2] if kept else None, self.occlusion_refresh_every)
        if age == 1:
            rows = self._build_occlusion_rows(ps, qs)
            self._occ_cache = (rows, key, 1)
            self.occlusion_rebuilds[0] += 1
            if self.occlusion_refresh_tol is not None:
                self._occ_built = (ps.clone(), torch.nn.functional.normalize(qs, dim=1))
            return rows
        rows = c[0]
        if self.occlusion_refresh_tol is not None and c[2] % self.occlusion_check_every == 0:
            tol_p, tol_q = self.occlusion_refresh_tol
            bp, bq = self._occ_built
            qn = torch.nn.functional.normalize(qs, dim=1)
            dist = (ps - bp).norm(dim=1)
            ang = 2.0 * torch.arccos((qn * bq).sum(dim=1).abs().clamp(max=1.0))   # the rotation between the two orientations
            if bool(((dist > tol_p) | (ang > tol_q)).any()):   # (the policy's host read)
                idx = ((dist > 0.5 * tol_p) | (ang > 0.5 * tol_q)).nonzero().flatten()
                C = self._rig.n_cams if self._rig is not None else 1
                new = self._build_occlusion_rows(ps[idx].contiguous(), qs[idx].contiguous())
                vidx = (idx[:, None] * C + torch.arange(C, device=idx.device)[None, :]).flatten()
                rows = rows.clone()   # (a step whose backward is still to come holds the old rows)
                rows[vidx] = new
                bp[idx], bq[idx] = ps[idx], qn[idx]
                self.occlusion_rebuilds[1] += int(idx.numel())
        self._occ_cache = (rows, key, age)
        return rows

    def _own_occlusion_rows(self, st, poses, quats, step_w=1):
        """The occlusion rows of the waypoints the waypoint-placed step `st` owns — rows lo .. hi-1 of the evaluated waypoints, which
        are every step_w-th row of poses / quats — or None: no occlusion, or no waypoint on this rank."""
        if self._occlusion is None or st.hi <= st.lo:
            return None
        own = slice(st.lo * step_w, (st.hi - 1) * step_w + 1, step_w)
        return self._occlusion_rows(poses[own].contiguous(), quats[own].contiguous())

    def _build_occlusion_rows(self, ps, qs):
        if self._rig is not None:
            qn = qs / qs.norm(dim=1, keepdim=True).clamp_min(1e-12)
            qc, lc = self._rig.q, self._rig.t
            aw, ax, ay, az = qn[:, None, :].unbind(-1)
            bw, bx, by, bz = qc[None, :, :].unbind(-1)
            vq = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                              aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1).reshape(-1, 4)
            w, x, y, z = qn.unbind(-1)
            R = torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                             2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                             2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1).reshape(-1, 3, 3)
            vt = (ps[:, None, :] + torch.einsum("wij,cj->wci", R, lc)).reshape(-1, 3)
            ps, qs = vt.contiguous(), vq.contiguous()
        return ops.occlusion_bits(self._cloud, self.points, ps, qs, self._cam, self._occlusion_limits[0],
                                  self._occlusion_limits[1], self._occlusion, grid=self._occlusion_grid)

    def _needs_split_step(self, prior=True):
        """Whether the visibility step goes through the separate calls (ops.WaypointShardStep / PointShardStep) instead of the
        one-call library step: point sharding, a collective, occlusion rows or (prior=True) a log-odds prior."""
        return (self._shard.kind == "points" or self._shard.collective or self._occlusion is not None or
                (prior and self._prior is not None))

    def _workspace(self, n_local_wps):
        v = n_local_wps * (self._rig.n_cams if self._rig is not None else 1)
        ws = self._ws_cache.get(v)
        if ws is None:
            ws = self._ws_cache[v] = ops.TrajWorkspace(self._cloud, v)
        return ws

    def _point_step(self, n_eval):
        """The point-sharded step's buffers (ops.PointShardStep) for n_eval evaluated waypoints."""
        st = self._ws_cache.get(("points", n_eval))
        if st is None:
            st = self._ws_cache[("points", n_eval)] = ops.PointShardStep(self._cloud, self._n_global, n_eval, self._cam, self._workspace(n_eval),
                                                                         self._shard, rig=self._rig, flags=self._flags)
        return st

    def _waypoint_step(self, n_eval):
        """The waypoint-placed step (ops.WaypointShardStep) for n_eval evaluated waypoints."""
        st = self._ws_cache.get(("waypoints", n_eval))
        if st is None:
            lo, hi = self._shard.bounds(n_eval)
            st = self._ws_cache[("waypoints", n_eval)] = ops.WaypointShardStep(self._cloud, n_eval, self._cam, self._workspace(max(hi - lo, 1)),
                                                                               self._shard, rig=self._rig, flags=self._flags)
        return st

    def _plan(self, step_w):
        """The library-side description of this model for the one-call forward / backward (rebuilt when something it froze
        has changed: the weights of criterion, the mode, the initial trajectory, the number of waypoints)."""
        key = (step_w, float(self.smoothness_weight), float(self.traj_length_weight), self._flags, self.poses0.data_ptr(),
               self.poses.shape[0], self._clearance_on, self.clearance_radius, self.clearance_weight, self.clearance_mode, self._clr_map)
        if self._plan_key != key:
            self._plan_obj, self._plan_key = _LossPlan(self, step_w), key
        return self._plan_obj

    def _wps_step(self, vis_wps_dist):
        # based on the mean waypoint distance of the INITIAL trajectory (model.py:214-215); constant per
        # model, so the host sync the reference pays on every forward happens once
        step = self._wps_step_cache.get(vis_wps_dist)
        if step is None:
            mean_wps_dist = (self.poses0[1:, :] - self.poses0[:-1, :]).norm(dim=1).mean()
            step = int(vis_wps_dist / mean_wps_dist) + 1
            self._wps_step_cache[vis_wps_dist] = step
        return step

    def forward(self,
                vis_wps_dist=0.5,  # metres between the waypoints whose visibility is evaluated (every wps_step-th one)
                debug=False):
        """/root/reference/src/model.py:200-242: soft visibility of every point from every wps_step-th waypoint, normalised per
        waypoint, clipped, turned into log-odds and summed over the waypoints; rewards = sigmoid of the sum; returns criterion()."""
        t0 = time()
        N_wps = len(self.poses)
        wps_step = self._wps_step(vis_wps_dist)
        points = self._shard.kind == "points"
        fused = N_wps >= 3 and type(self).criterion is ModelTraj.criterion
        if points and not fused:
            raise NotImplementedError("ModelTraj(shard=PointShard()) supports the reference's criterion on >= 3 waypoints")
        if fused and (self.fused_loss or points):
            if self._needs_split_step():
                loss, self.rewards, vis, l2, length, smooth, clr = _TrajLoss.apply(self.poses, self.quats, self, wps_step)
            else:
                plan = self._plan(wps_step)
                loss, self.rewards, vis, l2, length, smooth, clr = _TrajLossPlan.apply(self.poses, self.quats, plan)
                if type(loss) is _Loss and loss.requires_grad:
                    loss.__dict__["_tohip_fast"] = _FastBackward(plan, plan.ws.generation, loss.grad_fn, (self.poses, self.quats))
            self.loss = {'vis': vis, 'length': length, 'l2': l2, 'smooth': smooth}
            if self._clearance_on:
                self.loss['clearance'] = clr
            if debug:
                torch.cuda.synchronize(self.device)
                print(f'Trajectory evaluation took {1000 * (time() - t0)} msec')
            return loss
        if wps_step == 1:
            poses_eval, quats_eval = self.poses, self.quats
        else:
            idx = torch.arange(0, N_wps, wps_step, device=self.device)
            poses_eval, quats_eval = self.poses.index_select(0, idx), self.quats.index_select(0, idx)
        self.rewards = _TrajRewards.apply(poses_eval, quats_eval, self)  # total trajectory observations
        if debug:
            torch.cuda.synchronize(self.device)
            print(f'Trajectory evaluation took {1000 * (time() - t0)} msec')
        loss = self.criterion(self.rewards)
        return loss

    def criterion(self, rewards):
        # the four terms of /root/reference/src/model.py:244-260, op by op (the fused node computes the same on the device)
        # visibility: reciprocal of the mean reward
        self.loss['vis'] = 1. / (torch.mean(rewards) + self.eps)

        # the first waypoint should stay where the trajectory started
        self.loss['l2'] = torch.linalg.norm(self.poses[0] - self.poses0[0])

        # straighter is better: weight over the mean interior angle of the polyline
        self.loss['smooth'] = self.smoothness_weight / (mean_angle_calc(self.poses, self.eps) + self.eps)

        # the path should keep its initial length
        if self._length0 is None:
            self._length0 = length_calc(self.poses0)
        self.loss['length'] = self.traj_length_weight * torch.abs(length_calc(self.poses) - self._length0)

        total = self.loss['vis'] + self.loss['l2'] + self.loss['length'] + self.loss['smooth']
        if self._clearance_on:
            # keep the waypoints (clearance_mode 'segments': the segments between them) off the cloud — the term's query and gradient rows
            self.loss['clearance'] = _Clearance.apply(self.poses, self)
            total = total + self.loss['clearance']
        return total


# ------------------------------------------------------------------------------ team coverage

class _TeamLoss(torch.autograd.Function):
    """TeamTraj.forward in one autograd node: (every member's poses, every member's quats) -> (team total, rewards, member terms).
    The visibility step is a plain trajectory's over the members' evaluated waypoints laid end to end (the separate calls a prior
    model takes, n_traj = 1); criterion's terms of all members and their gradient rows are one launch (tohip_team_loss).  The total,
    the rewards and vis are differentiable; the member terms (B, 8) are not.  `loss.backward()` takes the fused visibility loss's
    unit sums (the arithmetic of the optimiser's step); any other upstream takes the kernels a ModelTraj on the same rows takes for it
    (with a prior the unit sums for loss['vis'] as well, the general dL/d rewards path otherwise)."""

    @staticmethod
    def forward(ctx, team, step_w, *params):
        B, m0 = team.B, team.models[0]
        P, Q = [p.detach() for p in params[:B]], [q.detach() for q in params[B:]]
        W = P[0].shape[0]
        n_eval = (W + step_w - 1) // step_w
        p_all = torch.cat(P).contiguous()
        ps, qs = torch.cat([p[::step_w] for p in P]).contiguous(), torch.cat([q[::step_w] for q in Q]).contiguous()   # E: own copies
        st = m0._waypoint_step(B * n_eval)
        lo_sum, rewards, scalars = st.forward(ps, qs, None, prior=team._prior)
        clr_rows = clr_terms = None
        if m0._clearance_on:
            clr_rows = torch.empty((B * W, 3), dtype=torch.float32, device=p_all.device)
            clr_terms = ops.clearance_terms(W, B, m0.clearance_mode, p_all.device)
            ops.clearance_rows(m0._clearance_source, p_all, m0.clearance_radius, m0.clearance_weight, m0.clearance_mode, B, clr_rows, clr_terms)
        terms, total, reg = ops.team_loss(p_all, team._poses0, B, m0.smoothness_weight, m0.traj_length_weight, m0.eps, scalars,
                                          m0.clearance_weight, clr_terms)
        ctx.team, ctx.step, ctx.gen, ctx.step_w, ctx.W, ctx.n_eval, ctx.has_clr = team, st, st.ws.generation, step_w, W, n_eval, clr_rows is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(terms)
        ctx.save_for_backward(ps, qs, lo_sum, scalars, reg, *((clr_rows,) if ctx.has_clr else ()))
        return total.reshape(()), rewards, scalars[1].clone(), terms

    @staticmethod
    def backward(ctx, g_loss, g_rewards, g_vis, _g_terms):
        team, st, W, n_eval = ctx.team, ctx.step, ctx.W, ctx.n_eval
        B, m0 = team.B, team.models[0]
        ps, qs, lo_sum, scalars, reg, *rest = ctx.saved_tensors
        clr_rows = rest[0] if ctx.has_clr else None
        g_loss = _f32(g_loss)
        upstream = _vis_upstream(g_loss, _f32(g_vis), g_rewards, scalars)
        pg = qg = None
        if upstream is not None:   # unit sums scaled once per waypoint for loss.backward(), and for loss['vis'] where a prior model takes them
            pg, qg = st.backward(ps, qs, None, ctx.gen, lo_sum, upstream, prior=team._prior,
                                 unit_sums=team._prior is not None or g_vis is None)
        grads_p, grads_q = [], []
        for b in range(B):
            e, w = slice(b * n_eval, (b + 1) * n_eval), slice(b * W, (b + 1) * W)
            gp, gq = _assemble_grads(ctx.step_w, W, pg[e] if pg is not None else None, qg[e] if qg is not None else None, g_loss,
                                     (None, None, None), reg[w], None, clr_rows[w] if clr_rows is not None else None, None)
            grads_p.append(gp)
            grads_q.append(gq)
        return (None, None, *grads_p, *grads_q)


class TeamTraj(nn.Module):
    """Several ModelTraj over ONE map as one model (team coverage): its parameters are the members' poses / quats, its
    reward is the team's — sigmoid(one log-odds sum over every member's evaluated waypoints + the prior) — so a point counts once
    whichever robot sees it, and the members divide the scene.  forward() returns the team total: 1 / (mean reward + eps) once, plus
    every member's own l2, length, smooth (and clearance).  Members: as optimizer.optimize_team's (same points, camera, rig, mode, eps,
    weights, waypoint count and step; no sharding, no occlusion; at most one prior, the first model's).  optimizer.optimize_team is
    the launch-only loop over the same arithmetic."""

    def __init__(self, models):
        super().__init__()
        models = list(models)
        self._prior = check_team(models, 0.5, "TeamTraj")
        self.models = nn.ModuleList(models)
        self.B = len(models)
        self._poses0 = torch.cat([m.poses0 for m in models]).contiguous()
        self._checked = {0.5}
        self.rewards = None
        self.loss = {"vis": float("inf")}

    def _step(self, vis_wps_dist):
        if vis_wps_dist not in self._checked:   # (the members' waypoint steps may differ at another distance)
            check_team(self.models, vis_wps_dist, "TeamTraj")
            self._checked.add(vis_wps_dist)
        return self.models[0]._wps_step(vis_wps_dist)

    def forward(self, vis_wps_dist=0.5):
        step_w = self._step(vis_wps_dist)
        total, self.rewards, vis, terms = _TeamLoss.apply(self, step_w, *[m.poses for m in self.models], *[m.quats for m in self.models])
        self.loss = {"vis": vis, "l2": list(terms[:, 1].unbind()), "length": list(terms[:, 2].unbind()),
                     "smooth": list(terms[:, 3].unbind())}
        if self.models[0]._clearance_on:
            self.loss["clearance"] = list(terms[:, 5].unbind())
        return total

    def mean_reward(self):
        """mean(rewards) of the team after the last forward (0-d tensor), or None before it."""
        return torch.mean(self.rewards.detach()) if self.rewards is not None else None

    def _evaluated(self, step_w):
        ps = torch.cat([m.poses.detach()[::step_w] for m in self.models]).contiguous()
        qs = torch.cat([m.quats.detach()[::step_w] for m in self.models]).contiguous()
        return ps, qs

    @torch.no_grad()
    def coverage_log_odds(self, clamp_max=None, vis_wps_dist=0.5):
        """The team's fused log-odds map (N,) f32 in the caller's order: prior + the one sum over every member's evaluated waypoints at
        their current poses — the next plan's prior_log_odds.  clamp_max: OctoMap's upper clamping threshold (>= 0; None: none)."""
        m0 = self.models[0]
        ps, qs = self._evaluated(self._step(vis_wps_dist))
        lo_sum, _ = ops.traj_forward(m0._cloud, ps, qs, m0._cam, m0._workspace(ps.shape[0]), m0._rig, flags=m0._flags)
        return ops.traj_coverage(m0._cloud, lo_sum, self._prior, clamp_max)

    def commit_coverage(self, coverage_map, vis_wps_dist=0.5):
        """ModelTraj.commit_coverage for the team: its coverage_log_odds (the map's clamp_max) integrated over the shared cloud with
        mode 'max'.  -> the map."""
        return coverage_map.integrate(self.models[0], self.coverage_log_odds(clamp_max=coverage_map.clamp_max, vis_wps_dist=vis_wps_dist),
                                      mode="max")

    @torch.no_grad()
    def member_gains(self, vis_wps_dist=0.5):
        """What each member adds, at the current poses -> (gain (B,) float64: the team's mean reward minus the mean reward of the team
        without member b; count (B,) int64: the points member b sees at all, log-odds > 0), on the host.  One forward that keeps a
        log-odds row per member, one pass over those rows (tohip_team_member_gains).  A member that sees nothing at all (far from the
        cloud: its row is NaN, as the reference's rewards are for such a waypoint) counts as absent: gain 0 and count 0 exactly, and
        the others' gains are those of the team without it.  At most 16 members."""
        if self.B > _lib.CONSTANTS["TOHIP_TEAM_MAX_GAINS"]:   # the pass keeps one accumulator pair per member in registers
            raise ValueError(f"TeamTraj.member_gains: at most 16 members ({self.B} given)")
        m0 = self.models[0]
        ps, qs = self._evaluated(self._step(vis_wps_dist))
        n_eval, C = ps.shape[0] // self.B, (m0._rig.n_cams if m0._rig is not None else 1)
        ws = m0._ws_cache.get(("team", self.B, n_eval))
        if ws is None:
            ws = m0._ws_cache[("team", self.B, n_eval)] = ops.TrajWorkspace(m0._cloud, self.B * n_eval * C, self.B)
        toff = (torch.arange(self.B + 1, dtype=torch.int32) * n_eval).to(m0.device)
        lo, _ = ops.traj_forward(m0._cloud, ps, qs, m0._cam, ws, m0._rig, flags=m0._flags, traj_offsets=toff)
        return ops.team_member_gains(m0._cloud, lo, self._prior)
