"""Drop-in geometry helpers of the reference's /root/reference/src/tools.py:38-187,320-325 on MI355X:
hidden-point removal (spherical flip + convex hull), the hard frustum cull, camera intrinsics, and the
per-camera hard-visibility pipeline of /root/reference/src/pc_processor.py:158-187.

All index sets are bit-exact with the reference's CPU path (tests/test_hip_hard.py).  No CPU fallback.
"""
import math
import types

import numpy as np
import torch

from . import ops


def load_intrinsics(device=torch.device('cuda')):
    """/root/reference/src/tools.py:320-325 -> (K, width, height)."""
    width, height = 1232., 1616.
    K = torch.tensor([[758.03967, 0., 621.46572],
                      [0., 761.62359, 756.86402],
                      [0., 0., 1.]], dtype=torch.float32).to(device)
    return K, width, height


def sphericalFlip(points, device, param):
    """/root/reference/src/tools.py:38-53."""
    return ops.spherical_flip(torch.as_tensor(points).to(device), param)[0]


def convexHull(points, device):
    """/root/reference/src/tools.py:56-64: hull of `points` plus the origin appended as the last row.
    Returns an object with `.vertices` (ascending int32 indices, as scipy reports them in 3-D)."""
    pts = torch.as_tensor(points, dtype=torch.float32).to(device)
    idx = ops.hull_vertices_with_origin(pts)
    return types.SimpleNamespace(vertices=idx)


def hidden_pts_removal(pts: torch.Tensor, device, R_param: int = 2, duplicate_rows: str = "lowest"):
    """/root/reference/src/tools.py:67-85 -> (pts_visible (V,3), visibleMask (N,) float32 of 0/1).
    Keeps the reference's quirk: the LAST hull vertex is dropped whether or not it is the origin.

    duplicate_rows — what to do when a VISIBLE point has exact copies (identical xyz rows) elsewhere in the cloud.  The visible set
    is the same either way (count and coordinates); what differs is which of the identical rows carries the index / mask bit:
      "lowest" (default)  the copy with the lowest row index, whatever the build's schedule.  Qhull (the reference, tools.py:79)
                          reports whichever copy its insertion history met first — the first copy in ~70 % of the cases, a later one
                          otherwise — which a parallel build cannot reproduce;
      "error"             raise ValueError if that situation occurs: for callers that need Qhull's exact row indices and would
                          rather de-duplicate (a VoxelGrid-filtered cloud has no duplicates) than get a different, equally valid row."""
    if duplicate_rows not in ("lowest", "error"):
        raise ValueError('duplicate_rows must be "lowest" or "error"')
    pts = torch.as_tensor(pts).to(device)
    idx, mask = ops.hidden_pts_removal(pts, R_param)
    if duplicate_rows == "error" and idx.numel():
        _, inverse, counts = torch.unique(pts.to(torch.float32), dim=0, return_inverse=True, return_counts=True)
        dup = counts[inverse[idx.long()]] > 1
        if bool(dup.any()):
            rows = idx[dup][:8].tolist()
            raise ValueError(f"{int(dup.sum())} visible point(s) have exact duplicate rows in the cloud (e.g. rows {rows}): their indices follow the "
                             "lowest-row rule here and Qhull's insertion history in the reference; de-duplicate the cloud or pass duplicate_rows='lowest'")
    pts_visible = pts[idx.long(), :]
    return pts_visible, mask


def get_cam_frustum_pts(points, img_height, img_width, intrins, min_dist=1.0, max_dist=10.0):
    """/root/reference/src/tools.py:176-187. `points` is (3,N) in the camera frame.
    -> (points_kept (M,3), dist_mask bool (N,), fov_mask bool (N,))"""
    intr = torch.as_tensor(intrins, dtype=torch.float32)[:3, :3]
    cam = ops.Camera(intr, img_width, img_height, 1.0, 5.0)
    dist_mask, fov_mask, idx = ops.frustum_cull(points, cam, min_dist, max_dist)
    kept = points[:, idx.long()].T
    return kept, dist_mask, fov_mask


def render_pc_image(verts, K, height, width, R=None, T=None, device=torch.device('cuda'), gamma=1.0e-1, znear=1.0,
                    zfar=10.0):
    """/root/reference/src/tools.py:122-173: image (height, width, 3) of a camera-frame cloud (N,3): spheres of
    0.03 m, nearest point per pixel, white background, colours = coordinates min-max normalised over the whole
    tensor.  The reference delegates to pytorch3d's pulsar renderer, which cannot be pinned offline; this is the build's
    statement of that configuration (render_kernels.hip): every disc over a pixel weighted by its falloff and
    exp(normalised depth / gamma) — `gamma` is pulsar's blending softness, 1e-5 = the nearest point alone .. 1 = everything
    shines through; `gamma=None` gives the nearest-depth splat itself.
    R, T (pytorch3d row-vector convention X_cam = X R + T) default to the identity like the reference's."""
    v = torch.as_tensor(verts, dtype=torch.float32).to(device)
    if R is not None or T is not None:
        Rm = torch.eye(3, device=v.device) if R is None else torch.as_tensor(R, dtype=torch.float32).to(v.device).reshape(3, 3)
        Tv = torch.zeros(3, device=v.device) if T is None else torch.as_tensor(T, dtype=torch.float32).to(v.device).reshape(3)
        v = v @ Rm + Tv
    if gamma is None:
        return ops.render_points(v, K, int(height), int(width), radius=0.03, znear=znear, zfar=zfar, background=1.0)[0]
    return ops.render_points_blend(v, K, int(height), int(width), radius=0.03, znear=znear, zfar=zfar, gamma=float(gamma), background=1.0)


def zbuffer_visible_points(verts, K, height, width, znear=1.0, zfar=10.0, radius=0.03):
    """Indices of the camera-frame points that win at least one pixel of the splat: the z-buffer counterpart of
    hidden_pts_removal (resolution dependent, approximate)."""
    _, _, owns = ops.render_points(torch.as_tensor(verts), K, int(height), int(width), radius, znear, zfar)
    return torch.nonzero(owns).squeeze(1).to(torch.int32)


def denormalize(x, eps=1e-6):
    """/root/reference/src/tools.py:190-196: scale an image to 0..1 between its 2nd and 98th percentiles (for display).
    Accepts a numpy array or a tensor; returns the same kind."""
    if torch.is_tensor(x):
        flat = x.detach().to(torch.float32).flatten()
        hi, lo = torch.quantile(flat, 0.98), torch.quantile(flat, 0.02)
        return ((x - lo) / torch.clamp(hi - lo, min=eps)).clamp(0, 1)
    import numpy as np
    x_max, x_min = np.percentile(x, 98), np.percentile(x, 2)
    return ((x - x_min) / np.max([(x_max - x_min), eps])).clip(0, 1)


def ego_to_cam(points, trans, quat):
    """/root/reference/src/pc_processor.py:63-70: (N,3) ego-frame points -> (3,N) camera frame; the
    quaternion is NOT normalised there, and is not here."""
    return ops.to_camera_frame_exact(points, quat, trans, normalize=False, transpose=True)


def visible_points_from_camera(points, trans, quat, intrins, img_height, img_width, min_dist=1.0, max_dist=15.0):
    """The per-camera hard visibility pipeline of /root/reference/src/pc_processor.py:158-187 without the
    ROS glue: transform -> hard frustum cull -> HPR from the camera centre.
    -> dict(cam_points (3,N), kept_idx, kept_points (M,3), visible_idx (into kept), visible_points (V,3))"""
    cam_pts = ego_to_cam(points, trans, quat)
    intr = torch.as_tensor(intrins, dtype=torch.float32)[:3, :3]
    cam = ops.Camera(intr, img_width, img_height, 1.0, 5.0)
    _, _, kept_idx = ops.frustum_cull(cam_pts, cam, min_dist, max_dist)
    kept = cam_pts[:, kept_idx.long()].T.contiguous()
    if kept.shape[0] >= 4:
        vis_idx, _ = ops.hidden_pts_removal(kept, 2)
    else:
        vis_idx = torch.empty(0, dtype=torch.int32, device=kept.device)
    return dict(cam_points=cam_pts, kept_idx=kept_idx, kept_points=kept, visible_idx=vis_idx,
                visible_points=kept[vis_idx.long()])


def visible_points_from_cameras(points, trans, quats, intrins, img_height, img_width, min_dist=1.0, max_dist=15.0):
    """visible_points_from_camera for C cameras at once (the reference repeats the pipeline per camera topic,
    /root/reference/src/pc_processor.py:57-59,158-187): per camera transform -> hard cull, then ONE batched hull pass
    for all cameras.  trans (C,3), quats (C,4) wxyz.  -> list of dicts as visible_points_from_camera returns."""
    pts = torch.as_tensor(points, dtype=torch.float32)
    dev = pts.device
    trans = torch.as_tensor(trans, dtype=torch.float32).reshape(-1, 3).to(dev).contiguous()
    quats = torch.as_tensor(quats, dtype=torch.float32).reshape(-1, 4).to(dev).contiguous()
    intr = torch.as_tensor(intrins, dtype=torch.float32)[:3, :3]
    cam = ops.Camera(intr, img_width, img_height, 1.0, 5.0)
    C, n = trans.shape[0], pts.shape[0]
    # transform + hard cull of every camera in one batched call (quaternions NOT normalised: ego_to_cam_torch)
    kept_idx, kept_pts, counts, _ = ops.cull_waypoints(pts, trans, quats, cam, min_dist, max_dist, normalize=False)
    out = []
    for c in range(C):
        m = counts[c]
        out.append(dict(cam_points=ego_to_cam(pts, trans[c], quats[c]), kept_idx=kept_idx[c, :m], kept_points=kept_pts[c, :m]))
    offs = [0]
    for r in out:
        offs.append(offs[-1] + r["kept_points"].shape[0])
    idx, voff, _, status = ops.hidden_pts_removal_batched(torch.cat([r["kept_points"] for r in out]), offs, 2)
    for c, r in enumerate(out):
        if int(status[c]) == 3:
            raise ValueError("Points cannot contain NaN")
        if int(status[c]) == 2:
            raise RuntimeError(f"camera {c}: the culled cloud is flat, no 3-D hull (Qhull raises QH6154)")
        # fewer than 4 kept points: no hull and nothing hidden-point removal could say -> empty, as the single-camera call
        r["visible_idx"] = (idx[int(voff[c]):int(voff[c + 1])] - offs[c]).contiguous()
        r["visible_points"] = r["kept_points"][r["visible_idx"].long()]
    return out


def xy_yaw_gradient(poses_grad, quats, quats_grad):
    """(dL/dx, dL/dy, dL/dyaw) per waypoint from the gradients the models produce (`model.poses.grad`, `model.quats.grad`):
    the planar parametrisation of a ground robot's waypoint.  Yaw turns the waypoint about the world z axis,
    q(yaw) = r_z(yaw) (x) q, so dq/dyaw = 1/2 (0,0,0,1) (x) q = 1/2 (-z, -y, x, w) for q = (w, x, y, z) and
    dL/dyaw = <dL/dq, dq/dyaw>.  `quats` are the models' raw quaternions (they are normalised inside the kernels; the
    gradient w.r.t. the raw quaternion is what autograd returns).  -> (W, 3) tensor."""
    q = torch.as_tensor(quats).detach()
    gq = torch.as_tensor(quats_grad).detach()
    gp = torch.as_tensor(poses_grad).detach()
    w, x, y, z = q.unbind(-1)
    dq = 0.5 * torch.stack([-z, -y, x, w], dim=-1)
    return torch.cat([gp[..., :2], (gq * dq).sum(-1, keepdim=True)], dim=-1)


def trajectory_clearance(points_or_packed_cloud, poses, radius, segments=False, unknown='free'):
    """How far each waypoint is from the cloud: (d, idx) on the device — d (W,) f32 the distance to the nearest point within
    `radius` (+inf when none), idx (W,) int32 that point's row in the caller's order (-1 when none; ties go to the lowest row).
    segments=True: how far each of the W - 1 straight segments between consecutive waypoints is from it: (d, idx, s), s (W-1,) f32
    where along the segment its closest point lies (0 = the segment's first waypoint, 1 = its second).
    The queries behind ModelTraj's clearance term (clearance_kernels.hip); `points_or_packed_cloud`: (N,3) points on the device, an
    ops.PackedCloud (sorted or not) or a ModelTraj (its cloud) — or a MAP, an ops.OccupancyGrid, SpaceMap or EvidenceMap: how far each
    waypoint (segment) is from the centre of the nearest occupied voxel — with unknown='obstacle' (not a bare grid) of the nearest
    occupied or never-seen one — and idx that voxel's linear index (z ny + y) nx + x (clearance_map_kernels.hip)."""
    cloud = points_or_packed_cloud
    if isinstance(cloud, (ops.OccupancyGrid, ops.SpaceMap, ops.EvidenceMap)):
        cloud = ops.MapObstacles(cloud, unknown)
        device = cloud.occupied.device
    else:
        if hasattr(cloud, "_cloud") and isinstance(cloud._cloud, ops.PackedCloud):
            cloud = cloud._cloud
        if not isinstance(cloud, ops.PackedCloud):
            cloud = ops.PackedCloud(torch.as_tensor(cloud, dtype=torch.float32))
        device = cloud.device
    poses = torch.as_tensor(poses, dtype=torch.float32)
    if poses.device != device:
        poses = poses.to(device)
    return ops.clearance_segments(cloud, poses, radius) if segments else ops.clearance(cloud, poses, radius)


def fuse_log_odds(*maps, clamp_max=None):
    """OctoMap's fusion of independent log-odds maps of one cloud (ModelTraj.coverage_log_odds of two robots' plans, or a map and a
    new plan's): their sum, clamped to clamp_max (its upper threshold; None: none) -> (N,) f32, a valid prior_log_odds when each map
    is one.  Maps of the same cloud in the same point order."""
    if not maps:
        raise ValueError("fuse_log_odds: no map given")
    out = torch.as_tensor(maps[0], dtype=torch.float32).clone()
    for m in maps[1:]:
        m = torch.as_tensor(m, dtype=torch.float32, device=out.device)
        if m.shape != out.shape:
            raise ValueError(f"fuse_log_odds: maps of {tuple(out.shape)} and {tuple(m.shape)} points")
        out += m
    if clamp_max is not None:
        out.clamp_(max=float(clamp_max))
    return out


def coverage_map(origin=(0.0, 0.0, 0.0), resolution=0.1, clamp_max=None, capacity=None, device=torch.device('cuda')):
    """An empty ops.CoverageMap: the voxel-keyed log-odds map that carries coverage from one cloud to the next.
    resolution: the voxel edge in metres — by default the leaf of the reference's VoxelGrid filter
    (/root/reference/launch/voxels_filtering.launch, voxel_grid_filter's default), so a filtered cloud has about one point per voxel.
    clamp_max: OctoMap's upper clamping threshold (None: none).  model.commit_coverage(map) writes, prior_log_odds=map reads."""
    return ops.CoverageMap(origin, resolution, clamp_max=clamp_max, capacity=capacity, device=device)


def occupancy_grid(points_or_cloud=None, resolution=0.1, margin=2, origin=None, dims=None, device=torch.device('cuda')):
    """An ops.OccupancyGrid: the dense occupancy bit grid the 'voxel' occlusion method and line_of_sight walk.  With
    points — (N,3) on the device, a PackedCloud or a ModelTraj — the grid around them with `margin` free voxels on every side, the
    points inserted; with origin and dims instead, an empty grid of that box.  grid.insert(more_points) adds any later cloud: a wall
    scanned two messages ago keeps occluding."""
    if points_or_cloud is not None:
        if origin is not None or dims is not None:
            raise ValueError("occupancy_grid: give points (the box is theirs) or origin and dims, not both")
        return ops.OccupancyGrid.from_points(points_or_cloud, resolution=resolution, margin=margin)
    if origin is None or dims is None:
        raise ValueError("occupancy_grid: without points both origin and dims are needed")
    return ops.OccupancyGrid(origin, resolution, dims, device=device)


def line_of_sight(grid, a, b, skip=(1, 1)):
    """Is b[i] visible from a[i]?  a, b (R,3) world points on the grid's device -> (R,) uint8: 1 clear, 0 blocked, 2 when an endpoint
    lies beyond the grid's apron (or is not finite).  An exact integer voxel walk (ops.OccupancyGrid): the same bits in every run.
    skip = (start_skip, end_skip): voxels within start_skip - 1 (Chebyshev) of a's voxel and within end_skip of b's are not tested
    — the default leaves out a's own voxel and the 3 x 3 x 3 block around b, so a surface point is not hidden by its own patch; a wall
    seen at a grazing angle still hides its far parts."""
    if not isinstance(grid, ops.OccupancyGrid):
        raise ValueError(f"line_of_sight: grid must be an ops.OccupancyGrid, got {type(grid).__name__}")
    return grid.line_of_sight(a, b, skip)


def space_map(grid, free=None):
    """An ops.SpaceMap over an occupancy grid: the grid stays the caller's — what it holds is occupied — and a free
    plane is added.  space.integrate(origin, points, max_range) takes a scan: its rows become occupied and its rays carve free space;
    what neither has touched stays unknown."""
    return ops.SpaceMap(grid, free)


def frontier_points(space, min_unknown=1):
    """The centres (F,3) f32 of the frontier voxels — free, with at least min_unknown unknown face neighbours: where the map ends.  A
    cloud every planning call accepts: propose_views(frontier_points(space), ...), select_views(..., occlusion='voxel',
    occlusion_grid=space.occupied)."""
    if not isinstance(space, ops.SpaceMap):
        raise ValueError(f"frontier_points: space must be an ops.SpaceMap, got {type(space).__name__}")
    return space.frontier(min_unknown).points


def known_free(space, positions):
    """(M,3) positions -> (M,) bool: the voxel is known to be free (a ray passed through it and nothing was measured in it).  The
    filter for roadmap_lattice nodes and propose_views positions: a node in a never-scanned room does not pass."""
    if not isinstance(space, ops.SpaceMap):
        raise ValueError(f"known_free: space must be an ops.SpaceMap, got {type(space).__name__}")
    return space.state(positions) == 1


def clearance_field(grid_or_space, max_dist, unknown='free'):
    """An ops.ClearanceField over an occupancy grid or a space map ("Clearance field"): per voxel a conservative
    distance to the nearest obstacle voxel, up to max_dist metres, in integers — so every collision check can ask the MAP, which
    outlives a message, instead of the current cloud.  unknown='free': only occupied voxels are obstacles; 'obstacle' (needs a
    SpaceMap): so is every voxel no ray has passed through, and a leg through a never-scanned room is blocked.  edge_clearance,
    build_roadmap, plan_path, plan_tour and refine_path take the field where they take a cloud; field.rebuild() follows later
    inserts and carves."""
    return ops.ClearanceField.build(grid_or_space, max_dist, unknown)


def free_nodes(field, radius, stride=1, space=None):
    """Free-space nodes from the map itself instead of a hand-chosen lattice: the voxels of `field` that keep `radius` from every
    obstacle, one in stride^3, and with space= (an ops.SpaceMap) only those known to be free -> ops.FreeNodes; its .points (F,3) are
    the via nodes of build_roadmap / plan_path / plan_tour and the positions of propose_views."""
    if not isinstance(field, ops.ClearanceField):
        raise ValueError(f"free_nodes: field must be an ops.ClearanceField, got {type(field).__name__}")
    return field.free_nodes(radius, stride, space)


def travel_field(field, start, radius, space=None, max_dist=None, weights=None):
    """Can the robot get there, and how far is it?  An ops.TravelField ("Travel field"): from `start` — (3,) or (S,3)
    positions, the robot's — the length of the shortest path to every voxel of the map, through voxels whose whole cube the clearance
    field certifies for `radius` metres and, with space= (an ops.SpaceMap), that are known to be free; 26-connected, no corner cut.
    tf.reachable(positions), tf.distance(positions) (metres), tf.cost(positions) and tf.paths(goals) ask it; travel_path(tf, goal)
    gives one path; select_views_volume(..., travel=tf, travel_weight=w) prices the trip to each candidate.  max_dist (metres)
    truncates the field.  A start that is not traversable is ignored (tf.seeded): nothing is then reachable.  tf.rebuild(start)
    follows field.rebuild() or a robot that has moved.  weights (an ops.TravelWeights, travel_weights' result; None: geometric
    length): the field minimises the weighted length instead — routes keep off walls and out of the unknown — and every cost,
    distance and max_dist is then in weighted units; tf.weights tells a consumer what it holds."""
    if not isinstance(field, ops.ClearanceField):
        raise ValueError(f"travel_field: field must be an ops.ClearanceField, got {type(field).__name__}")
    return ops.TravelField(field, radius, start, space=space, max_dist=max_dist, weights=weights)


def travel_weights(field, radius, soft_radius, gain=4.0, space=None, unknown_add=0, lut=None):
    """A cost layer so that routes keep off walls: an ops.TravelWeights ("Weighted travel fields") for
    travel_field(s)(..., weights=).  Each voxel gets a factor kappa in [16, 255] (16: neutral) from the clearance field's gap g
    around it: kappa = 16 + 16 gain max(0, (soft_radius - g) / (soft_radius - radius))^2, rounded — neutral at and beyond soft_radius,
    1 + gain times as dear at `radius`, where the traversable set ends.  The table is computed on the host in float64
    (synth.travel_weights_lut restates it) and gathered on the device in one launch; lut= (1-D integers in [16, 255], indexed by the
    field's squared gap in voxels, the last entry for everything beyond) replaces it.  space= with unknown_add (0 .. 255) adds that
    much at every voxel that is neither occupied nor known free, saturating at 255: a dash through the unknown stops costing what
    a walk through the scanned room costs.  weights.rebuild() follows field.rebuild()."""
    if not isinstance(field, ops.ClearanceField):
        raise ValueError(f"travel_weights: field must be an ops.ClearanceField, got {type(field).__name__}")
    if lut is None:
        r = ops.check_tour_radius(radius)
        soft = ops._float_or_nan(soft_radius) if ops._is_real(soft_radius) else float("nan")
        if not np.isfinite(soft) or soft <= r:
            raise ValueError(f"travel_weights: soft_radius must be a finite number of metres > radius ({radius!r}), got {soft_radius!r}")
        gn = ops._float_or_nan(gain) if ops._is_real(gain) else float("nan")
        if not np.isfinite(gn) or gn < 0.0:
            raise ValueError(f"travel_weights: gain must be a finite number >= 0, got {gain!r}")
        d2 = np.arange(field.D * field.D + 1, dtype=np.float64)
        t = np.maximum(0.0, (soft - np.sqrt(d2) * float(np.float32(field.resolution))) / (soft - r))
        lut = np.clip(np.rint(16.0 + 16.0 * gn * t * t), ops.TRAVEL_KAPPA_NEUTRAL, ops.TRAVEL_KAPPA_MAX).astype(np.uint8)
    return ops.TravelWeights(field, lut=lut, space=space, unknown_add=unknown_add)


def ground_layer(map, headroom, step=1, unknown='free'):
    """For a robot that drives: an ops.GroundLayer ("Ground layer") over an ops.OccupancyGrid, ops.SpaceMap or
    ops.EvidenceMap.  headroom: the robot's height in metres; step: the riser it climbs, in voxels (0 .. 4); unknown='obstacle'
    (needs a free plane): unseen space neither carries nor lets pass.  layer.ground is where it can stand, layer.obstacles what it
    must keep its radius from — the floor it rolls on is not among them — and layer.drive the slab its centre rides in.
    layer.field(max_dist) and layer.space go wherever a clearance field and a space map go: travel_field(s), travel_matrix,
    travel_path, free_nodes, plan_path, plan_tour(travel=True), refine_path, assign_frontiers, frontier_clusters(travel=),
    select_views_volume(travel=).  layer.rebuild() follows the map."""
    return ops.GroundLayer(map, headroom, step, unknown)


def ground_travel(layer, start, radius, max_dist=None, max_drop=None, field=None, weights=None):
    """Can the robot DRIVE there, and how far is it?  The ops.TravelField of a ground layer: over layer.field(...) and layer.space,
    from `start` — (3,) or (S,3) poses at any height above the floor, a sensor's for instance — snapped to the standing voxel at or
    at most max_drop voxels below (None: the layer's headroom H; a start with nothing to stand on is ignored, tf.seeded).  radius:
    the robot's, in metres; max_dist (metres) truncates the travel field; field: a ClearanceField from layer.field(...) to reuse
    (None: one is built, truncated one voxel beyond what `radius` needs).  Every voxel with a cost is a place the robot's centre can
    be: over ramps and steps of at most layer.step voxels, never across a ledge or a pit, under a table only where it fits.
    tf.sources holds the snapped starts; layer.snap(path, max_drop) brings a path's rows down to the wheels.  weights: an
    ops.TravelWeights of the layer's geometry (over `field`, or over another layer.field(...)), as travel_field's — a slope penalty, a
    keep-out zone."""
    if not isinstance(layer, ops.GroundLayer):
        raise ValueError(f"ground_travel: layer must be an ops.GroundLayer, got {type(layer).__name__}")
    if field is None:
        need = int(np.ceil(np.sqrt(ops.field_need2(ops.check_tour_radius(radius), layer.resolution))))
        field = layer.field(D=min(need + 1, ops.FIELD_MAX_D))
    elif not isinstance(field, ops.ClearanceField) or field.occupied is not layer.obstacles:
        raise ValueError("ground_travel: field must be an ops.ClearanceField from layer.field(...)")
    standing, _ = layer.snap(ops._check_rows3(start, "start"), layer.H if max_drop is None else max_drop)
    return ops.TravelField(field, radius, standing, space=layer.space, max_dist=max_dist, weights=weights)


def yaw_candidates(quat, half_range, n):
    """n headings about the world's z axis, centred on `quat` (wxyz) -> (n,4) float64 on the host: n odd, the yaw offsets evenly spaced
    over [-half_range, +half_range] radians (0 for n = 1), each composed in f64 as yaw(a) * quat.  The middle row is `quat` itself,
    normalised: its offset is exactly 0."""
    q = ops._host_rows(quat, 4, "quat", rows=1)[0]
    if not ops._is_int(n) or n < 1 or n % 2 == 0 or n > ops.SCAN_MAX_ROTATIONS:
        raise ValueError(f"yaw_candidates: n must be an odd integer in [1, {ops.SCAN_MAX_ROTATIONS}], got {n!r}")
    h = ops._float_or_nan(half_range)
    if not (np.isfinite(h) and 0.0 <= h <= math.pi):
        raise ValueError(f"yaw_candidates: half_range must be a finite angle in [0, pi] radians, got {half_range!r}")
    q = q / np.sqrt((q * q).sum())
    m = n // 2
    w, x, y, z = q
    out = np.tile(q, (n, 1))
    for i in range(n):
        if i != m:
            c, s = math.cos(0.5 * h * (i - m) / m), math.sin(0.5 * h * (i - m) / m)
            out[i] = (c * w - s * z, c * x - s * y, c * y + s * x, c * z + s * w)   # (c, 0, 0, s) * q
    return out


def scan_refine(volume, at):
    """The sub-voxel offset (dx, dy, dz) of one rotation's window volume (2wz+1, 2wy+1, 2wx+1) around its best cell at = (dzi, dyi,
    dxi) -> (3,) float64 in voxels: per axis the vertex 0.5 (s- - s+) / (s+ - 2 s0 + s-) of the parabola through the best score and
    its two neighbours along that axis, only where both neighbours lie inside the window and the second difference is negative,
    clamped to +-0.5 voxel; 0 otherwise.  Host arithmetic in f64."""
    v = np.asarray(volume, dtype=np.float64)
    at = tuple(int(c) for c in at)
    out = np.zeros(3, dtype=np.float64)
    for axis in range(3):       # of the volume: 0 is z, 1 is y, 2 is x
        i = at[axis]
        if i < 1 or i > v.shape[axis] - 2:
            continue
        lo, hi = list(at), list(at)
        lo[axis], hi[axis] = i - 1, i + 1
        s0, sm, sp = v[at], v[tuple(lo)], v[tuple(hi)]
        dd = sp - 2.0 * s0 + sm
        if dd < 0.0:
            out[2 - axis] = min(0.5, max(-0.5, 0.5 * (sm - sp) / dd))
    return out


def _scan_matcher(what, map_or_matcher, floor, unknown_value):
    if isinstance(map_or_matcher, ops.ScanMatcher):
        if floor is not None or not (ops._is_int(unknown_value) and unknown_value == 0):
            raise ValueError(f"{what}: floor and unknown_value belong to the ScanMatcher that was given (floor {map_or_matcher.floor}, "
                             f"unknown_value {map_or_matcher.unknown_value}); leave them at their defaults, got {floor!r} and {unknown_value!r}")
        return map_or_matcher
    if isinstance(map_or_matcher, ops.SpaceMap):
        raise ValueError(f"{what}: a SpaceMap holds no log-odds: give ops.EvidenceMap.from_space(space)")
    return ops.ScanMatcher(map_or_matcher, floor, unknown_value)


def match_scan(map_or_matcher, points, pose, quat, window=(8, 8, 2), yaw=None, rotations=None, floor=None, unknown_value=0, refine=True):
    """Where was the sensor when it took this scan?  Correlative scan matching on an ops.EvidenceMap ("Scan matching"):
    `points` (N,3), the scan in the SENSOR frame, is scored against the map at the prior `pose` (3,) / `quat` (4,) wxyz moved by every
    integer voxel shift of `window` = (wx, wy, wz) and turned to every candidate rotation, and the best is returned -> ScanMatch.
    The rotations are the caller's list: yaw=(half_range_rad, n) asks for yaw_candidates(quat, half_range, n); rotations=(K,4)
    gives the list itself; neither: the prior's rotation alone.  map_or_matcher: the map — floor and unknown_value then shape the
    score: max(L, floor) where observed, unknown_value elsewhere — or an ops.ScanMatcher to reuse over several scans of one map
    (refresh() it after an integrate; floor and unknown_value are then the matcher's and must be left at their defaults).  refine: fit a parabola per axis through the best score and its neighbours for a sub-voxel
    translation, pose_refined.  Translation is found to one voxel (or to the parabola), rotation to the list's spacing; there is no
    covariance.  One read-back: the best candidate's eight integers and its counters (and, with refine, its rotation's window);
    before it one copy of the K poses to the device, which waits for the current stream."""
    matcher = _scan_matcher("match_scan", map_or_matcher, floor, unknown_value)
    prior = ops._host_rows(quat, 4, "quat", rows=1)
    if yaw is not None and rotations is not None:
        raise ValueError("match_scan: give yaw or rotations, not both")
    if yaw is not None:
        try:
            half_range, n = yaw
        except (TypeError, ValueError):
            raise ValueError(f"match_scan: yaw must be (half_range_rad, n), got {yaw!r}") from None
        quats = yaw_candidates(prior, half_range, n)
    else:
        quats = ops._host_rows(prior if rotations is None else rotations, 4, "rotations")
    t = ops._host_rows(pose, 3, "pose", rows=1)
    poses12 = matcher.poses(t, quats)
    scores, used = matcher.correlate(points, t, quats, window, poses12=poses12)
    best = matcher.best(scores)
    k = best[1:2].long()
    counters = matcher.score(points, None, None, shifts=best[2:5].reshape(1, 3), poses12=poses12.index_select(0, k))
    parts = [best, torch.cat(counters), used.index_select(0, k)]
    if refine:
        parts.append(scores.index_select(0, k).reshape(-1))
    host = torch.cat(parts).cpu().numpy()   # the one read-back
    flat, kk, dx, dy, dz, score, ties = (int(v) for v in host[:7])
    if int(host[8]) != score:
        raise RuntimeError(f"match_scan: the window's best score {score} and the winner's own {int(host[8])} differ: the matcher's table is "
                           "stale — refresh() it after the map took a scan")
    r = np.float32(matcher.resolution)
    shift = np.asarray((dx, dy, dz), dtype=np.float32)
    found = (t[0].astype(np.float32) + (shift * r).astype(np.float32)).astype(np.float32)
    refined = found.astype(np.float64)
    if refine:
        volume = host[13:].reshape(scores.shape[1:])
        w = tuple(n // 2 for n in scores.shape[1:])
        refined = refined + scan_refine(volume, (dz + w[0], dy + w[1], dx + w[2])) * float(r)
    return ScanMatch(pose=found, quat=quats[kk].copy(), shift=(dx, dy, dz), rotation=kk, score=score, used=int(host[12]), known=int(host[11]),
                     ties=ties, scores=scores, pose_refined=refined)


def relocalise_scan(map_or_matcher, points, pose, quat, window=None, yaw=None, rotations=None, levels=None, floor=None, unknown_value=0,
                    refine=True, capacity=1 << 22):
    """Where in this map am I?  match_scan's question over a WIDE window ("Relocalisation"): the exact best candidate of
    |dx| <= wx, |dy| <= wy (up to 2048 voxels each), |dz| <= wz <= 4 and the caller's rotations, found by branch and bound over
    sliding-maximum copies of the score table instead of scoring every candidate — the same winner, tie rule and `ties` as the
    exhaustive search, bit for bit.  window=None: centred on the prior, reaching every voxel of dims in x and y (wz = 0).  levels: None
    (the smallest H <= 6 that leaves at most 256 top-level blocks a rotation and z shift) or H in [0, 6].  yaw, rotations, floor,
    unknown_value, refine and map_or_matcher as match_scan takes them.  -> ScanMatch with, beyond match_scan's fields, levels,
    nodes (the nodes of each level 0 .. H before the drop), evaluated (all bounds computed), candidates (K S) and incumbent; scores
    is the (3,3,3) int32 score neighbourhood [dz][dy][dx] of the winner, which the parabola is fitted through.  A level of more
    than `capacity` nodes raises RuntimeError.  On a map with little structure nothing is pruned and the search costs more than
    scoring every candidate.  WHEN TO CALL WHICH (measured, DESIGN.md 10 "Relocalisation": a 405 x 405 x 45 room, 100 k points, 41 headings): at
    window (10, 10, 2) this search and match_scan cost the same, 3.1 against 3.2 ms; at (64, 64, 1) it takes 3.3 ms where scoring
    every candidate takes 475 ms.  So inside match_scan's reach (16, 16, 4) match_scan remains the right call — it also returns the
    whole score volume — and every window beyond it is this function's.  One read-back; before it one
    copy of the K poses to the device, which waits for the current stream."""
    matcher = _scan_matcher("relocalise_scan", map_or_matcher, floor, unknown_value)
    prior = ops._host_rows(quat, 4, "quat", rows=1)
    if yaw is not None and rotations is not None:
        raise ValueError("relocalise_scan: give yaw or rotations, not both")
    if yaw is not None:
        try:
            half_range, n = yaw
        except (TypeError, ValueError):
            raise ValueError(f"relocalise_scan: yaw must be (half_range_rad, n), got {yaw!r}") from None
        quats = yaw_candidates(prior, half_range, n)
    else:
        quats = ops._host_rows(prior if rotations is None else rotations, 4, "rotations")
    t = ops._host_rows(pose, 3, "pose", rows=1)
    if window is None:
        g = (t[0].astype(np.float32) - np.asarray(matcher.origin, dtype=np.float32)) / np.float32(matcher.resolution)   # (the map's rule, in f32)
        voxel = np.floor(np.clip(g, -2048.0, 4095.0)).astype(np.int64)
        window = ops.scan_search_window(voxel, matcher.dims)
    poses12 = matcher.poses(t, quats)
    record = matcher.search(points, t, quats, window, levels=levels, capacity=capacity, poses12=poses12)
    k = record[1:2].clamp(0, len(quats) - 1)
    shift = record[2:5].to(torch.int32)
    counters = matcher.score(points, None, None, shifts=shift.reshape(1, 3), poses12=poses12.index_select(0, k))
    i = torch.arange(27, dtype=torch.int32, device=matcher.device)   # the winner's 3 x 3 x 3 neighbourhood, built on the device
    offs = torch.stack([torch.zeros_like(i), i % 3 - 1, torch.div(i, 3, rounding_mode="floor") % 3 - 1, torch.div(i, 9, rounding_mode="floor") - 1], dim=1)
    nodes = torch.cat([k.to(torch.int32), shift]).reshape(1, 4) + offs
    around, used = matcher.bound(points, nodes, 0, poses12=poses12)
    host = torch.cat([record, torch.cat(counters).long(), used.index_select(0, k).long(), around.long()]).cpu().numpy()   # the one read-back
    rec = host[:ops.SCAN_SEARCH_RECORD]
    H = int(rec[10])
    wx, wy, wz = (int(c) for c in window)
    stopped = ops.scan_search_status(rec[7])
    if stopped is not None:
        raise RuntimeError(f"relocalise_scan: level {stopped[0]} of the search would hold {stopped[1]} nodes, more than the capacity of "
                           f"{capacity}: give a narrower window, more levels (levels={H} now), fewer rotations or a larger capacity")
    flat, kk, dx, dy, dz, score, ties = (int(v) for v in rec[:7])
    if int(host[ops.SCAN_SEARCH_RECORD]) != score:
        raise RuntimeError(f"relocalise_scan: the search's best score {score} and the winner's own {int(host[ops.SCAN_SEARCH_RECORD])} differ: "
                           "the matcher's table is stale — refresh() it after the map took a scan")
    r = np.float32(matcher.resolution)
    found = (t[0].astype(np.float32) + (np.asarray((dx, dy, dz), dtype=np.float32) * r).astype(np.float32)).astype(np.float32)
    refined = found.astype(np.float64)
    if refine:
        refined = refined + scan_refine(host[-27:].reshape(3, 3, 3), (1, 1, 1)) * float(r)
    return ScanMatch(pose=found, quat=quats[kk].copy(), shift=(dx, dy, dz), rotation=kk, score=score, used=int(host[ops.SCAN_SEARCH_RECORD + 4]),
                     known=int(host[ops.SCAN_SEARCH_RECORD + 3]), ties=ties, scores=around.reshape(3, 3, 3), pose_refined=refined, levels=H,
                     nodes=tuple(int(v) for v in rec[11:12 + H]), evaluated=int(rec[9]), candidates=len(quats) * (2 * wx + 1) * (2 * wy + 1) * (2 * wz + 1),
                     incumbent=int(rec[8]))


def scan_registrations(state, resolution, dof="xyzrpw"):
    """A registration state (B,64) int64 ON THE HOST -> [ScanRegistration] in numpy: the pose, the quaternion normalised once, the
    cost and counters of the record at the result, the information matrix A = S H S and the covariance sigma^2 A^-1 over the free
    degrees of freedom, both in metres and radians."""
    mask = ops.scan_dof_mask(dof)
    free = np.asarray([(mask >> i) & 1 for i in range(6)], dtype=bool)
    r = float(np.float32(resolution))
    state = np.ascontiguousarray(np.asarray(state, dtype=np.int64).reshape(-1, ops.SCAN_REGISTER_STATE))
    floats = state.view(np.float64)
    F = ops.SCAN_REGISTER_FIELDS
    scale = np.asarray([1.0 / (256.0 * r)] * 3 + [4.0] * 3)   # 1/256 byte per voxel -> byte per metre; 4 byte per radian -> byte per radian
    iu = np.triu_indices(6)
    out = []
    for I, D in zip(state, floats):
        rec = I[F["record"]:F["record"] + ops.SCAN_REGISTER_RECORD]
        H = np.zeros((6, 6))
        H[iu] = rec[:21].astype(np.float64)
        H = H + np.triu(H, 1).T
        A = H * scale[:, None] * scale[None, :]
        A[~free] = 0.0
        A[:, ~free] = 0.0
        used, n_dof = int(rec[28]), int(free.sum())
        cost = float(int(rec[27])) / 4096.0 ** 2
        cov = np.zeros((6, 6))
        if used > n_dof:
            sub = A[np.ix_(free, free)]
            if np.isfinite(sub).all() and np.linalg.matrix_rank(sub) == n_dof:
                cov[np.ix_(free, free)] = cost / (used - n_dof) * np.linalg.inv(sub)
        q = D[F["q"]:F["q"] + 4].copy()
        out.append(ScanRegistration(pose=D[F["t"]:F["t"] + 3].copy(), quat=q / np.sqrt((q * q).sum()), cost=cost,
                                    rms=math.sqrt(cost / used) if used else 0.0, used=used, inside=int(rec[29]), iterations=int(I[F["iterations"]]),
                                    accepted=int(I[F["accepted"]]), status=ops.SCAN_REGISTER_STATUS[int(I[F["status"]])], information=A,
                                    covariance=cov, lam=float(D[F["lam"]])))
    return out


def register_scan(map_or_matcher, points, pose, quat, iterations=30, dof="xyzrpw", tol_t=None, tol_r=None, floor=None, unknown_value=0):
    """The last link of match -> REGISTER -> integrate ("Scan registration"): refine a pose that match_scan or
    relocalise_scan found to one voxel and one step of a yaw list into a sub-voxel translation and a continuous rotation, by damped
    Gauss-Newton steps on the trilinear interpolation of the map's score table.  points (N,3), the scan in the SENSOR frame; pose (3,)
    and quat (4,) wxyz, or B of each (at most 256): a batch is refined in the same launches, and each pose of it is bitwise its own
    single run.  dof: the degrees of freedom that move, a string over 'x y z r p w' (roll, pitch, yaw: rotations about the world's x,
    y, z through the sensor's position) or a 6-bit mask; a planar robot passes 'xyw'.  iterations: 1 .. 256 rounds, each pose frozen
    as soon as its status leaves RUNNING: CONVERGED (an accepted step within tol_t voxels — None: 1/256 — and tol_r radians — None:
    1e-4), STALLED (lambda passed 2^30: no step lowers the cost, the usual end at a kink of the field), DEGENERATE (a pivot of the
    damped system is not positive: a direction the scan does not constrain — lock it with dof) or EMPTY (no point in range).
    map_or_matcher, floor and unknown_value as match_scan takes them.  -> ScanRegistration for one pose, a list of them for a batch.

    THE COVARIANCE is sigma^2 A^-1 over the free degrees of freedom, A the Gauss-Newton normal matrix at the result and sigma^2 =
    cost / (used - n_dof): the Gauss-Newton approximation on a piecewise-trilinear field whose residual target is the byte 255.  It
    tells WHICH DIRECTIONS the scan constrains and how they compare — a corridor's axis comes out orders of magnitude looser than its
    width, or DEGENERATE — it is not a calibrated uncertainty: the residuals are neither independent nor Gaussian, and the map's own
    error is not in it.  The basin is about one voxel (that is what match_scan is for); there is no robust loss.

    One copy of the poses to the device, which waits for the current stream, then launches only; one read-back, of the state, at
    the end."""
    matcher = _scan_matcher("register_scan", map_or_matcher, floor, unknown_value)
    q = ops._host_rows(quat, 4, "quat")
    t = ops._host_rows(pose, 3, "pose")
    single = t.shape[0] == 1 and q.shape[0] == 1 and np.ndim(pose) <= 1 and np.ndim(quat) <= 1
    state = matcher.register(points, t, q, iterations=iterations, dof=dof, tol_t=tol_t, tol_r=tol_r)
    out = scan_registrations(state.cpu().numpy(), matcher.resolution, dof)   # the one read-back
    return out[0] if single else out


PoseGraph, PoseGraphResult = ops.PoseGraph, ops.PoseGraphResult


def optimize_pose_graph(poses, quats, a, b, t, q, information, fixed=(0,), registrations=None, device=torch.device('cuda'), **kw):
    """The back end behind match -> register -> integrate ("Pose graph"): spread the corrections that loop closures and
    registrations measure back over a trajectory.  poses (N,3) and quats (N,4) wxyz, the scan poses as they were integrated (any
    quaternion length, either sign); a, b (E,) node indices, t (E,3) and q (E,4) the measured relative poses R_a^T (t_b - t_a) and
    conj(q_a) (x) q_b — odometry between consecutive scans (PoseGraph.relative of two registered poses), closures from
    relocalise_scan — a = -1 for a measurement of node b in the world; information (E,6,6) or (E,21) over (x, y, z, roll, pitch, yaw)
    in metres and radians, rotations about the edge's own axes through the node's position: for an absolute edge exactly
    register_scan's parameterisation, so registrations={node: ScanRegistration} appends each with its information / sigma^2 and no
    change of frame.  fixed: the nodes that do not move (the first by default); every connected component needs a fixed node or an
    absolute edge, and ValueError names a node of one that floats.  Keywords are PoseGraph.optimize's: iterations=30,
    cg_iterations=None (min(6 N, 1000)), cg_tol=1e-8, dof='xyzrpw' ('xyw': a planar robot), robust=None or Geman-McClure's c — a
    relocaliser in a building with two similar corridors WILL close a loop wrongly some day, and with robust= such an edge ends with
    a weight near 0 and a large chi2 in the result, which is how to find it —, tol_t=1e-5, tol_r=1e-6.  -> PoseGraphResult: poses,
    quats (normalised), cost, initial_cost, iterations, accepted, cg_iterations, status (CONVERGED, STALLED, DEGENERATE, NONFINITE;
    RUNNING: the iterations ran out), lam, chi2 (E,) and weights (E,).

    WHAT IT IS NOT.  The solve is block-Jacobi conjugate gradients: it needs on the order of the graph's diameter in iterations, and a
    long chain with one closure is its worst case.  There are no marginal covariances.  The rotation residual is the Gibbs vector 2
    tan(theta / 2): it grows faster than the angle beyond about 60 degrees and is undefined at 180.  Geman-McClure needs a sensible
    start: from a start where the good edges are as wrong as the bad, it keeps whichever it meets.  Edges join poses only: there are
    no landmarks.  Every sum runs in one stated order: two runs, and the numpy restatement, give the same bits.

    One upload, then launches only; one read-back, of the result, at the end."""
    g = ops.PoseGraph(poses, quats, fixed=fixed, device=device)
    if a is not None and len(np.atleast_1d(a)):
        g.add_edges(a, b, t, q, information)
    for node, reg in (registrations or {}).items():
        g.add_registration(node, reg)
    return g.optimize(**kw)


def score_scans(map_or_matcher, points, poses, quats, shifts=None, floor=None, unknown_value=0):
    """How well does the scan fit the map at each of these poses?  B explicit candidates — poses (B,3), quats (B,4) wxyz, shifts None
    or (B,3) voxels — -> (score, used, inside, known), each (B,) int32 on the device (ops.ScanMatcher.score): the weights a particle
    filter needs, read from the map's bytes themselves.  One launch, nothing read back."""
    return _scan_matcher("score_scans", map_or_matcher, floor, unknown_value).score(points, poses, quats, shifts)


def label_components(grid_or_plane, connectivity=26):
    """Which voxels belong together?  An ops.Components ("Connected components") of a bit plane: an ops.OccupancyGrid
    (an occupied grid, a free plane, space.unknown(), an evidence map's .occupied / .free) or anything that carries one as .grid
    (space.frontier(), field.free_nodes()).  connectivity 6, 18 or 26.  comp.n, comp.sizes, comp.centroids, comp.bbox describe the
    components, comp.at(positions) names the one a position lies in, comp.min_over(travel_field) the nearest voxel of each."""
    grid = grid_or_plane.grid if isinstance(grid_or_plane, ops.Frontier) else grid_or_plane
    if not isinstance(grid, ops.OccupancyGrid):
        raise ValueError(f"label_components: the plane must be an ops.OccupancyGrid or carry one as .grid, got {type(grid_or_plane).__name__}")
    return ops.Components(grid, connectivity)


def evidence_map(grid_or_points, resolution=0.1, **params):
    """An ops.EvidenceMap ("Evidence map"): per voxel an integer log-odds value that every scan moves — up where a
    return fell, down where a ray passed — and the occupied and free planes derived from it, so a person who walked through the
    first scan, a door that was shut or one spurious return leave the map again after a few contradicting scans.  From an
    ops.OccupancyGrid: an empty map of its box; from an ops.SpaceMap: seeded with what it holds (occupied at lmax, free at lmin);
    from points — (N,3) on the device, a PackedCloud or a ModelTraj — an empty map of the box around them at `resolution`.
    params: hit, miss, lmin, lmax, threshold (integers; ops.check_evidence).  m.integrate(origin, points, max_range) takes a scan;
    m.occupied, m.free and m.space go wherever an OccupancyGrid or a SpaceMap goes."""
    if isinstance(grid_or_points, ops.SpaceMap):
        return ops.EvidenceMap.from_space(grid_or_points, **params)
    if isinstance(grid_or_points, ops.OccupancyGrid):
        return ops.EvidenceMap.like(grid_or_points, **params)
    return ops.EvidenceMap.like(ops.OccupancyGrid.from_points(grid_or_points, resolution=resolution), **params)


MERGE_MAX_DIM, MERGE_MAX_VOXELS = ops.MERGE_MAX_DIM, ops.MERGE_MAX_VOXELS   # of a merged or transformed map's box: per axis, in all


def reframe_map(map, shift=None, dims=None, centre=None):
    """A map's content in another box of its lattice -> a NEW map of the same kind ("Re-framing and merging maps"): an
    ops.OccupancyGrid, ops.SpaceMap or ops.EvidenceMap (values, both planes, the parameters).  Give exactly one of shift — three
    integers: new voxel v is old voxel v + shift — or centre, a world position whose voxel becomes the new box's middle voxel dims //
    2; dims: the new box's (default: the old one's): grow, crop or move.  What leaves the box is dropped, what enters it is empty
    (unknown).  The old map is untouched; a ClearanceField, TravelField, Components or ModelTraj(clearance_map=) built over it keeps
    it and is built anew over the new one.  The move is a whole number of voxels and copies bits and bytes; transform_map is the call
    that rotates, shifts by a fraction of a voxel or refines the resolution."""
    ops.check_reframe(map, shift, dims, centre)
    return map.reframed(shift=shift, dims=dims, centre=centre)


def follow_map(map, position, margin):
    """Keep a map's box around a moving robot: -> `map` itself while position's voxel lies at least `margin` voxels from every side
    of the box — host arithmetic only, nothing is launched — otherwise map.reframed(centre=position), a new map of the same dims with
    that voxel in the middle.  margin: an integer, or three (one per axis: a sensor's range along the axes the robot travels, little
    along the others), each >= 0 and satisfied by the middle voxel itself (margin <= (n - 1) // 2).  A frontier needs unknown space
    inside the box, so the margin should exceed the sensor's range.  Call it every step: `m = follow_map(m, p, margin)`."""
    f = ops._map_frame(map, "map")
    limits = tuple((n - 1) // 2 for n in f.dims)
    try:
        ms = (margin,) * 3 if ops._is_int(margin) else tuple(margin)
    except TypeError:
        ms = ()
    if len(ms) != 3 or not all(ops._is_int(m) and 0 <= m <= lim for m, lim in zip(ms, limits)):
        raise ValueError(f"margin must be an integer or three integers, each in [0, (n - 1) // 2] of its axis — at most {limits} for dims "
                         f"{tuple(f.dims)} — got {margin!r}")
    v = ops.position_voxel(f, position)
    if all(m <= c <= n - 1 - m for c, n, m in zip(v, f.dims, ms)):
        return map
    return map.reframed(centre=position)


def transform_map(map, pose, quat, origin=None, resolution=None, dims=None, like=None, rule="nearest"):
    """A map under a rigid transform and, if asked, at a finer resolution -> a NEW map of the same kind and parameters (DESIGN.md 10,
    "Resampling maps"): an ops.OccupancyGrid, ops.SpaceMap or ops.EvidenceMap; the old one is only read.  pose (3,), quat (4,) wxyz:
    world_new = R(quat) world_old + pose — the pose of the old map's frame in the new one, what align_maps and register_scan return,
    or a pose-graph correction.  The new box: like= a map whose frame to take, or origin / resolution / dims; by default the
    axis-aligned box around the old box's transformed corners at the old resolution, its origin a multiple of it (ValueError beyond
    2048 voxels an axis or 2^31 voxels).  rule 'nearest': each new voxel takes the old voxel that holds its centre — unbiased, the
    rule for evidence that will be fused; a wall one voxel thick may show pinholes after a rotation.  rule 'cover', for planning: the
    maximum over the 3 x 3 x 3 old voxels around it under free < unknown < occupied (planes: OR for occupied, AND for free) — no
    occupied voxel is lost, nothing is free unless all it touches was free, a ray cannot slip through a wall; walls and the unknown
    grow by up to a voxel.  Not a coarsening: a resolution coarser than the map's is refused (coarsen_map reduces by a whole
    factor), one finer than an eighth of it too.
    A ClearanceField, TravelField or Components over the old map is built anew over the new one."""
    ops.check_transform(map, pose, quat, origin, resolution, dims, like, rule)
    return map.transformed(pose, quat, origin=origin, resolution=resolution, dims=dims, like=like, rule=rule)


def coarsen_map(map, factor=2, rule=None, anchor="origin", origin=None, dims=None, like=None):
    """A map at `factor` times its voxel edge -> a NEW map of the same kind and parameters ("Coarsening maps"): an
    ops.OccupancyGrid, ops.SpaceMap or ops.EvidenceMap; the old one is only read.  factor: an integer in [2, 8]; each coarse voxel
    reduces its factor^3 children.  rule, for a SpaceMap or an EvidenceMap: 'cover' (the default), for planning — occupied if a child
    is occupied, else unknown if a child is unknown or lies outside the map, else free: no occupied voxel is lost, nothing is free
    unless all it holds is free, so clearance_field, travel_field and line of sight over the coarse map err on the safe side; or
    'max', for display, occlusion and matching — the largest child, optimistic about the unknown.  For an OccupancyGrid: 'any' (the
    default) or 'all'.  anchor 'origin': the coarse box starts at the map's origin; 'world': the coarse lattice's planes lie at
    multiples of the coarse edge, so coarse maps of any sources on one fine lattice share a lattice and merge_maps takes them as they
    are.  origin / dims / like: another box on the fine lattice (ops.check_coarsen).  A ClearanceField, TravelField or Components is
    built anew over the coarse map."""
    _, _, rule = ops.check_coarsen(map, factor, rule, anchor, origin, dims, like)
    return map.coarsened(factor, rule=rule, anchor=anchor, origin=origin, dims=dims, like=like)


def map_pyramid(map, levels, rule=None):
    """A map at several scales -> [map, level 1, ..., level `levels`]: each level is the one before it at factor 2 with
    anchor='origin' (coarsen_map), so level l equals coarsen_map(map, 2 ** l) bit for bit where that factor is allowed — the rules'
    reductions are associative.  levels: an integer >= 0; rule as coarsen_map (None: the kind's default, 'cover' or 'any')."""
    ops._map_frame(map, "map")
    if not ops._is_int(levels) or levels < 0:
        raise ValueError(f"levels must be an integer >= 0, got {levels!r}")
    out = [map]
    for _ in range(int(levels)):
        out.append(coarsen_map(out[-1], 2, rule=rule))
    return out


def merge_maps(maps, mode=None, poses=None, quats=None, rule="nearest"):
    """Fuse a team's maps into one -> a NEW map over the union of their boxes; the inputs are only read.  maps: two or more
    ops.OccupancyGrids, ops.SpaceMaps or ops.EvidenceMaps (one kind) on one device.  Without poses they share one lattice — equal
    resolutions, origins a whole number of voxels apart (ops.lattice_offset; ValueError names the axis otherwise).  poses (n,3) and
    quats (n,4) wxyz place map i's frame in map 0's — world_0 = R(quats[i]) world_i + poses[i], what align_maps(maps[0], maps[i], ...)
    returns; row 0 is the identity — and the union is taken over the transformed boxes on map 0's lattice; a map whose pose is the
    identity and which sits on that lattice moves by a voxel shift, every other one is resampled under `rule` ('nearest', unbiased,
    or 'cover', conservative: transform_map says what each gives) and must not be finer than map 0.  The first map is re-framed
    into the union box — which keeps its parameters — and the others are merged into it: planes by OR; evidence by mode 'confident'
    (the default: per voxel the stronger belief wins; any order and any repetition give the same map) or 'add' (independent evidence
    summed and clamped; a map given twice counts twice).  ValueError if the union exceeds 2048 voxels on an axis or 2^31 voxels."""
    maps = list(maps)
    if len(maps) < 2:
        raise ValueError(f"merge_maps: at least two maps are needed, got {len(maps)}")
    if (poses is None) != (quats is None):
        raise ValueError("merge_maps: poses and quats must be given together")
    first = maps[0]
    evidence = isinstance(first, ops.EvidenceMap)
    mode = ("confident" if mode is None else mode) if evidence else mode
    frames = [ops._map_frame(m, "map") for m in maps]
    if poses is None:
        placed = [(None, None)] * len(maps)
    else:
        t, q = ops._host_rows(poses, 3, "poses"), ops._host_rows(quats, 4, "quats")
        if len(t) != len(maps) or len(q) != len(maps):
            raise ValueError(f"merge_maps: {len(maps)} maps need as many poses and quats, got {len(t)} and {len(q)}")
        if t[0].any() or q[0][1:].any() or q[0][0] == 0.0:
            raise ValueError("merge_maps: the poses place each map in map 0's frame: row 0 must be the identity (pose 0, quat (1, 0, 0, 0))")
        placed = list(zip(t, q))
    boxes = [((0, 0, 0), frames[0].dims)]
    for m, f, (pose, quat) in list(zip(maps, frames, placed))[1:]:
        affine = None
        if m is not first:   # (the first map again: merged into the new map like any other)
            s, _, affine = ops.check_merge_posed(first, m, mode, pose, quat, rule)
        if affine is None:
            boxes.append((ops.lattice_offset(first, m), f.dims))
        else:
            boxes.append(ops.transformed_box(f, pose, quat, frames[0].resolution, anchor=frames[0].origin))
    lo = tuple(min(k[a] for k, _ in boxes) for a in range(3))
    hi = tuple(max(k[a] + n[a] for k, n in boxes) for a in range(3))
    dims = tuple(h - l for l, h in zip(lo, hi))
    if max(dims) > MERGE_MAX_DIM or dims[0] * dims[1] * dims[2] > MERGE_MAX_VOXELS:
        raise ValueError(f"merge_maps: the union box of {dims} voxels exceeds {MERGE_MAX_DIM} per axis or 2^31 voxels")
    out = first.reframed(shift=lo, dims=dims)
    for m, (pose, quat) in list(zip(maps, placed))[1:]:
        kw = {} if pose is None else dict(pose=pose, quat=quat, rule=rule)
        out.merge(m, mode, **kw) if evidence else out.merge(m, **kw)
    return out


def align_maps(target, source, pose, quat, window=None, yaw=None, iterations=30, dof="xyzrpw"):
    """Where does one map's frame stand in another's?  -> ScanRegistration whose .pose, .quat satisfy world_target = R(quat)
    world_source + pose and go straight into merge_maps(poses=, quats=) and transform_map.  Host composition of what exists: the
    centres of `source`'s occupied voxels (export(), in the source's frame) are the scan; relocalise_scan finds the best integer
    shift within `window` (None: all of the target's x and y) and heading of yaw=(half_range_rad, n) around the prior (pose, quat),
    register_scan refines it below a voxel over `dof` in `iterations` rounds.  target: an ops.EvidenceMap or an ops.ScanMatcher over
    one; source: an ops.OccupancyGrid, SpaceMap or EvidenceMap.  The answer is as good as the two maps' overlap: the matchers' own
    limits (one voxel and one step of the yaw list before the refinement, a basin of about a voxel for it) apply, and two rooms that
    look alike align as happily as one room seen twice."""
    matcher = _scan_matcher("align_maps", target, None, 0)
    ops._map_frame(source, "source")
    plane = source if isinstance(source, ops.OccupancyGrid) else source.occupied
    _, centres = plane.export()
    if centres.shape[0] == 0:
        raise ValueError("align_maps: the source map has no occupied voxel")
    found = relocalise_scan(matcher, centres, pose, quat, window=window, yaw=yaw)
    return register_scan(matcher, centres, found.pose, found.quat, iterations=iterations, dof=dof)


class _Result:
    """What the result classes share: the keyword constructor; each names its fields in its own __slots__."""
    __slots__ = ()

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class ScanMatch(_Result):
    """What match_scan returns: pose (3,) f32 — fl(prior + fl(shift r)) per axis — and quat (4,) f64, the winning candidate; shift (dx,
    dy, dz) in voxels and rotation, its row of the list; score; used (the points in range under that rotation), known (those that met
    an observed voxel), ties (the candidates that share the best score: 1 for a unique answer); scores (K, 2wz+1, 2wy+1, 2wx+1) int32
    on the device; pose_refined (3,) f64, the pose moved by the parabola's sub-voxel offset (equal to pose with refine=False);
    world(points) takes sensor-frame points to the world at the matched pose.  From relocalise_scan: scores is the (3,3,3) score
    neighbourhood [dz][dy][dx] of the winner, and levels (H), nodes (the nodes of each level 0 .. H before the drop), evaluated (all
    bounds computed), candidates (K S, what an exhaustive search would score) and incumbent are set as well."""
    __slots__ = ("pose", "quat", "shift", "rotation", "score", "used", "known", "ties", "scores", "pose_refined", "levels", "nodes", "evaluated",
                 "candidates", "incumbent")

    def world(self, points, refined=False):
        """(N,3) sensor-frame points on a device -> (N,3) f32 world points at the matched (or refined) pose: torch ops, rounded as torch
        rounds them — the scores' own arithmetic is not promised."""
        R = torch.from_numpy(ops.scan_rotations(self.quat, "quat")[0]).to(points.device)
        t = torch.as_tensor(np.asarray(self.pose_refined if refined else self.pose, dtype=np.float32), device=points.device)
        return points.to(torch.float32) @ R.T + t


class ScanRegistration(_Result):
    """What register_scan returns: pose (3,) f64 in metres and quat (4,) f64 wxyz, normalised on the host; cost, the sum of squared
    residuals 255 - M in byte^2 at the result, and rms = sqrt(cost / used) in bytes; used (the points in range) and inside (those whose
    eight corners all lie inside dims); iterations run and steps accepted; status, a name of ops.SCAN_REGISTER_STATUS; lam, the last
    lambda; information (6,6) f64, A = J^T J at the result over (x, y, z in metres; roll, pitch, yaw in radians), and covariance (6,6)
    f64 = cost / (used - n_dof) A^-1 over the free degrees of freedom — rows and columns of a locked one are zero, and all of it where
    used <= n_dof or A is singular.  See register_scan for what the covariance is and is not.  world(points) takes sensor-frame points
    to the world at the registered pose."""
    __slots__ = ("pose", "quat", "cost", "rms", "used", "inside", "iterations", "accepted", "status", "lam", "information", "covariance")

    def world(self, points):
        """(N,3) sensor-frame points on a device -> (N,3) f32 world points at the registered pose: torch ops, rounded as torch rounds."""
        R = torch.from_numpy(ops.scan_rotations(self.quat, "quat")[0]).to(points.device)
        t = torch.as_tensor(np.asarray(self.pose, dtype=np.float32), device=points.device)
        return points.to(torch.float32) @ R.T + t


class ViewSelection(_Result):
    """What select_views returns: order (n_selected,) int64 and gains (n_selected,) f64 on the host (gain j = what view order[j] added
    to the mean reward when it was chosen), poses / quats (the chosen rows in selection order), rewards (N,) and mean_reward of the
    chosen views together (with the prior), coverage_log_odds (N,) in the caller's order (prior + the chosen views' log-odds: the next
    plan's prior), nnz (entries the candidates' sparse rows hold), absent (M,) bool (the candidates that see nothing at all),
    gain_fixed (n_selected,) int64 (the integer sums behind `gains`) and log_odds (npad,) the chosen views' summed log-odds in the
    packed order."""
    __slots__ = ("order", "gains", "gain_fixed", "poses", "quats", "rewards", "mean_reward", "coverage_log_odds", "nnz", "absent", "log_odds")

    @property
    def n_selected(self):
        return int(self.order.shape[0])


def _views_setup(model_or_cloud, prior_log_odds, occlusion, kw, occlusion_grid=None, occlusion_voxel=0.1):
    """select_views' first argument resolved -> dict(cloud, cam, rig, flags, prior, occlusion, limits, grid, voxel); cloud / prior
    may still be what the caller gave (points / a tensor): they are packed after every check has passed (and, for
    occlusion='voxel' without a grid, the grid built from the packed cloud's points)."""
    m = model_or_cloud
    if ops._model_cloud(m, "select_views") is not m:   # a ModelTraj: its own settings, nothing to override
        if kw:
            raise ValueError(f"select_views: {sorted(kw)} belong to the call with points; a ModelTraj brings its own camera and rig")
        if occlusion is not None and occlusion != m._occlusion:
            raise ValueError(f"select_views: occlusion={occlusion!r} given, the model has {m._occlusion!r}")
        own_grid = getattr(m, "_occlusion_grid", None)
        if occlusion_grid is not None and occlusion_grid is not own_grid:
            raise ValueError("select_views: occlusion_grid given, the model brings its own (occlusion_grid= of its constructor)")
        prior = m._prior if prior_log_odds is None else ops.resolve_prior(prior_log_odds, m._cloud)
        return dict(cloud=m._cloud, cam=m._cam, rig=m._rig, flags=m._flags, prior=prior, occlusion=m._occlusion,
                    limits=m._occlusion_limits, grid=own_grid, voxel=getattr(m, "_occlusion_voxel", 0.1))
    ops.check_occlusion(occlusion)
    if occlusion_grid is not None and (occlusion != "voxel" or not isinstance(occlusion_grid, ops.OccupancyGrid)):
        raise ValueError(f"select_views: occlusion_grid must be an ops.OccupancyGrid and needs occlusion='voxel', got "
                         f"{type(occlusion_grid).__name__} with occlusion={occlusion!r}")
    allowed = {"intrins", "img_width", "img_height", "min_dist", "max_dist", "rig", "dense", "occlusion_limits"}
    if set(kw) - allowed:
        raise ValueError(f"select_views: unknown keyword(s) {sorted(set(kw) - allowed)}")
    missing = [k for k in ("intrins", "img_width", "img_height") if k not in kw]
    if missing:
        raise ValueError(f"select_views: with points or a PackedCloud the camera is needed: {missing} missing")
    if isinstance(m, ops.PackedCloud):
        if not m.sorted:
            raise ValueError("select_views: the PackedCloud must be in Morton order (sort=True), as ModelTraj's")
        n = m.n
    else:
        if not torch.is_tensor(m) or m.dim() != 2 or m.shape[1] != 3 or m.shape[0] == 0:
            raise ValueError(f"select_views: points must be an (N,3) tensor with N > 0, a PackedCloud or a ModelTraj, got "
                             f"{tuple(m.shape) if torch.is_tensor(m) else type(m).__name__}")
        n = m.shape[0]
    if prior_log_odds is not None:
        prior_log_odds = ops.resolve_prior(prior_log_odds, m)   # (a CoverageMap: its lookup over these points)
        ops.check_prior(prior_log_odds, n)
    cam = ops.Camera(kw["intrins"], kw["img_width"], kw["img_height"], kw.get("min_dist", 1.0), kw.get("max_dist", 5.0))
    return dict(cloud=m, cam=cam, rig=kw.get("rig"), flags=ops.DENSE if kw.get("dense") else 0, prior=prior_log_odds, occlusion=occlusion,
                limits=kw.get("occlusion_limits", (1.0, 15.0)), grid=occlusion_grid, voxel=occlusion_voxel)


def select_views(model_or_cloud, cand_poses, cand_quats, k, prior_log_odds=None, min_gain=0.0, occlusion=None, clamp_max=None, chunk=None,
                 occlusion_grid=None, occlusion_voxel=0.1, **camera):
    """Greedy view selection: out of the M candidate views cand_poses (M,3) / cand_quats (M,4) wxyz, choose up to k
    that together cover the most, against what prior_log_odds (N,) — or an ops.CoverageMap, looked up over the cloud — already holds.  Round after round the view that adds the most to
    the mean reward sigmoid(S + prior) is chosen (S: the log-odds of the views chosen so far; ties go to the lowest index) until k
    are chosen, none is left, the best adds nothing or adds less than min_gain to the mean reward.  The objective is monotone
    submodular: the greedy choice is within (1 - 1/e) of the best set of that size.

    model_or_cloud: a ModelTraj — its cloud, camera, rig, dense mode, prior and occlusion setting score the candidates exactly as
    that model rewards them (prior_log_odds overrides its prior) — or (N,3) points / an ops.PackedCloud with the keywords intrins,
    img_width, img_height[, min_dist, max_dist, rig=(quats, trans), dense, occlusion_limits] as the models take them.
    occlusion='hpr'|'zbuffer'|'voxel': every candidate's occlusion rows are built chunk by chunk (ops.occlusion_bits); 'voxel' walks
    occlusion_grid (an ops.OccupancyGrid: the map so far), or a grid of the cloud's own points at occlusion_voxel metres.  clamp_max: OctoMap's
    upper clamping threshold for coverage_log_odds.  chunk: candidates per forward (None: ops.ViewSet's default).
    -> ViewSelection.  One host synchronisation at the end (the hull pass's own with occlusion; one more run when the candidates'
    rows outgrow the first capacity guess, 1 % of M x N)."""
    cfg = _views_setup(model_or_cloud, prior_log_odds, occlusion, camera, occlusion_grid, occlusion_voxel)
    M, k, min_gain = ops.check_views(cand_poses, cand_quats, k, min_gain, chunk)
    if clamp_max is not None and not float(clamp_max) >= 0.0:
        raise ValueError(f"clamp_max must be a number >= 0 or None, got {clamp_max!r}")
    cloud = cfg["cloud"]
    if not isinstance(cloud, ops.PackedCloud):
        cloud = ops.PackedCloud(torch.as_tensor(cloud, dtype=torch.float32))
    dev = cloud.device
    prior = cfg["prior"]
    if prior is not None and not isinstance(prior, ops.LogOddsPrior):
        prior = ops.LogOddsPrior(cloud, prior)   # (checks it: ops.check_prior)
    rig = cfg["rig"]
    if rig is not None and not isinstance(rig, ops.CameraRig):
        rig = ops.CameraRig(rig[0], rig[1], dev)
    ps = cand_poses.detach().to(device=dev, dtype=torch.float32).contiguous()
    qs = cand_quats.detach().to(device=dev, dtype=torch.float32).contiguous()
    occ_of = None
    if cfg["occlusion"] is not None:
        from .model import ModelTraj, _occlusion_grid   # (model imports this module)
        cfg["grid"] = _occlusion_grid(cfg["occlusion"], cfg["grid"], cfg["voxel"], cloud)
        shim = types.SimpleNamespace(_rig=rig, _cloud=cloud, points=cloud.points, _cam=cfg["cam"], _occlusion_limits=cfg["limits"],
                                     _occlusion=cfg["occlusion"], _occlusion_grid=cfg["grid"])
        occ_of = lambda p, q: ModelTraj._build_occlusion_rows(shim, p, q)
    capacity = None
    for attempt in range(2):
        vs = ops.ViewSet(cloud, cfg["cam"], M, rig=rig, flags=cfg["flags"], nnz_capacity=capacity, chunk=chunk)
        for w0 in range(0, M, vs.chunk):
            p, q = ps[w0:w0 + vs.chunk], qs[w0:w0 + vs.chunk]
            vs.append(p, q, occ_of(p, q) if occ_of is not None else None)
        order, gain, n_sel, S = ops.views_select(vs, k, prior, min_gain)
        ws = ops.TrajWorkspace(cloud, 1)
        rewards, scalars = ops.traj_reward(cloud, S, cfg["cam"], ws, prior=prior)
        coverage = ops.traj_coverage(cloud, S, prior, clamp_max)
        absent = vs.absent
        # the one synchronisation: everything small in one copy
        h = torch.cat([vs.header(), n_sel.long(), order.long(), gain]).cpu()
        if int(h[2]) & 2:
            raise RuntimeError("select_views: the view set's chunks were not appended in order")
        if int(h[2]) == 0:
            break
        if attempt == 1:
            raise RuntimeError(f"select_views: the candidates' rows need {int(h[1])} entries, more than the reported {capacity}")
        capacity = int(h[1])
    n = int(h[5])
    sel = h[6:6 + n].clone()
    gfix = h[6 + k:6 + k + n].clone()
    shift = 47 - (cloud.n - 1).bit_length()   # the reward kernel's fixed point
    idx = sel.to(dev)
    return ViewSelection(order=sel, gain_fixed=gfix, gains=gfix.to(torch.float64) / float(2 ** shift) / cloud.n, poses=ps[idx], quats=qs[idx],
                         rewards=rewards, mean_reward=float(scalars[0]), coverage_log_odds=coverage, nnz=int(h[0]), absent=absent.cpu(),
                         log_odds=S)


class VolumeSelection(_Result):
    """What select_views_volume returns: order (n_selected,) int64 and gains (n_selected,) int64 on the host (gain j = the unknown
    voxels view order[j] added when it was chosen: a marginal gain), poses / quats (the chosen rows in selection order, on the
    device), revealed (an ops.OccupancyGrid: the caller's `claimed` plus every voxel the chosen views reveal — the next round's or the
    next robot's `claimed`) and total = sum(gains), the popcount the selection added to it.  travel: (n_selected,) f32 on the device,
    the metres from the travel field's sources to each chosen view — None where the selection was made without a travel field."""
    __slots__ = ("order", "gains", "poses", "quats", "revealed", "total", "travel")

    @property
    def n_selected(self):
        return int(self.order.shape[0])


def _volume_setup(what, space_or_evidence_map, camera):
    """view_volume's and select_views_volume's map and camera keywords -> (ops.SpaceMap, ops.Camera, min_dist, max_dist)."""
    space = space_or_evidence_map.space if isinstance(space_or_evidence_map, ops.EvidenceMap) else space_or_evidence_map
    if not isinstance(space, ops.SpaceMap):
        raise ValueError(f"{what}: the map must be an ops.SpaceMap or an ops.EvidenceMap, got {type(space_or_evidence_map).__name__}")
    allowed = {"intrins", "img_width", "img_height", "min_dist", "max_dist"}
    if set(camera) - allowed:
        raise ValueError(f"{what}: unknown keyword(s) {sorted(set(camera) - allowed)}")
    missing = [k for k in ("intrins", "img_width", "img_height") if k not in camera]
    if missing:
        raise ValueError(f"{what}: the camera is needed: {missing} missing")
    mn, mx = camera.get("min_dist", 1.0), camera.get("max_dist", 5.0)
    return space, ops.Camera(camera["intrins"], camera["img_width"], camera["img_height"], mn, mx), mn, mx


def view_volume(space_or_evidence_map, poses, quats, claimed=None, **camera):
    """How much unknown space would a camera see from here?  (M,) int64 on the device: per view poses[w] (M,3) / quats[w] (M,4) wxyz
    the number of UNKNOWN voxels of the map — neither occupied nor free, and not set in `claimed` (an ops.OccupancyGrid of the map's
    geometry, or None) — whose centre lies inside the camera frustum and the depth limits and is in line of sight of the camera
    through the occupied voxels ("Unknown volume").  Unknown voxels do not block: the rule is optimistic.  Keywords:
    intrins, img_width, img_height[, min_dist = 1, max_dist = 5], as select_views takes them with points.  An ops.EvidenceMap is
    used through its .space.  Exact integers: the same counts in every run."""
    space, cam, mn, mx = _volume_setup("view_volume", space_or_evidence_map, camera)
    return ops.view_volume(space, poses, quats, cam, mn, mx, claimed=claimed)


def select_views_volume(space_or_evidence_map, cand_poses, cand_quats, k, min_gain=1, claimed=None, travel=None, travel_weight=0.0,
                        **camera):
    """Greedy next-best-view selection by revealed volume ("Unknown volume"): out of the M candidates cand_poses (M,3) /
    cand_quats (M,4) wxyz, M <= 65 535 — propose_views' prop.poses, prop.quats go in as they are — choose up to k that together
    reveal the most unknown voxels of the map.  Round after round every candidate not yet taken is scored by view_volume against the voxels claimed
    so far, the largest gain wins (ties go to the lowest index), and the winner's voxels are claimed; selection stops after k views,
    when none is left, or when the best gain is below min_gain (an integer number of voxels >= 1).  claimed: an ops.OccupancyGrid of
    the map's geometry holding what earlier rounds or other robots will already see (not modified), or None.

    The objective is the coverage of a set — the number of distinct voxels revealed — which is monotone submodular: the greedy
    choice is within (1 - 1/e) of the best set of that size.  Everything runs on the device, 3 k launches and one host
    synchronisation at the end.  Keywords: the camera, as view_volume takes it.  -> VolumeSelection.

    travel (an ops.TravelField of the map's geometry, travel_field's result; None: none) prices the trip: a candidate whose position
    the robot cannot reach is never chosen, and every round's winner maximises gain - travel_weight x metres travelled
    (travel_weight >= 0, in revealed voxels per metre; 0: reachability alone).  The stop rule stays the gain's.  With a weighted
    field (travel_field(..., weights=)) the trip's price is the weighted cost."""
    space, cam, mn, mx = _volume_setup("select_views_volume", space_or_evidence_map, camera)
    cost, m = None, 0
    if travel is not None:
        m = _travel_weight_fixed("select_views_volume", travel, travel_weight)
        ops.check_view_volume(space, cand_poses, cand_quats, k, min_gain, claimed)
        cost = travel.cost(cand_poses.detach().to(device=space.device, dtype=torch.float32).contiguous())
    elif travel_weight != 0.0:
        raise ValueError("select_views_volume: travel_weight needs travel= (an ops.TravelField)")
    order, gains, revealed = ops.view_volume_select(space, cand_poses, cand_quats, cam, mn, mx, k, min_gain, claimed, travel_cost=cost,
                                                    travel_m=m)
    return VolumeSelection(**_selection_fields(space.device, cand_poses, cand_quats, order, gains, revealed, travel))


def _travel_weight_fixed(what, travel, travel_weight):
    """travel= and travel_weight= of a selection -> the weight's fixed-point form m (gain 2^20 - m cost decides)."""
    if not isinstance(travel, ops.TravelField):
        raise ValueError(f"{what}: travel must be an ops.TravelField or None, got {type(travel).__name__}")
    w = float(travel_weight) if isinstance(travel_weight, (int, float)) and not isinstance(travel_weight, bool) else float("nan")
    if not (w >= 0.0) or w == float("inf"):
        raise ValueError(f"{what}: travel_weight must be a finite number >= 0, got {travel_weight!r}")
    m = int(round(w * float(travel.resolution) * (1 << 20) / 64.0))
    if m >= 1 << 31:
        raise ValueError(f"{what}: travel_weight {travel_weight!r} is too large at this resolution (its fixed-point form "
                         f"{m} must stay below 2^31)")
    return m


def _selection_fields(device, cand_poses, cand_quats, order, gains, revealed, travel):
    """A device selection (order, gains, revealed) -> the fields VolumeSelection and InformationSelection share; the one
    synchronisation."""
    h = torch.cat([order.long(), gains]).cpu()
    kk = order.shape[0]
    n = int((h[:kk] >= 0).sum())
    sel, g = h[:n].clone(), h[kk:kk + n].clone()
    idx = sel.to(device)
    ps = cand_poses.detach().to(device=device, dtype=torch.float32)
    qs = cand_quats.detach().to(device=device, dtype=torch.float32)
    return dict(order=sel, gains=g, poses=ps[idx], quats=qs[idx], revealed=revealed, total=int(g.sum()),
                travel=travel.distance(ps[idx].contiguous()) if travel is not None else None)


def information_table(map, unit=0.05, unknown_bits=1.0, scale=4096):
    """The default weight table of an ops.EvidenceMap -> (256,) uint16 on the host, indexed by the evidence byte read as unsigned,
    L + 128: the entropy that observation can still remove from a voxel, round(scale max(0, H(sigma(unit L)) - H(sigma(unit c))))
    with H the binary entropy in bits and c the clamp the voxel's state moves towards (lmin where L <= threshold, lmax above);
    entry 0, a voxel never observed, weighs round(scale unknown_bits).  A voxel at a clamp weighs 0: a finished map has information
    0.  unit = 0.05 is the log-odds per step of the map's default hit = 17 / miss = 8 (0.85 / 0.4).  Any (256,) table of the caller's
    own goes wherever table= goes — "only weakly occupied voxels" is a table that is 0 up to the threshold."""
    if not isinstance(map, ops.EvidenceMap):
        raise ValueError(f"information_table: the map must be an ops.EvidenceMap, got {type(map).__name__}")
    return ops.information_table(map.params, unit, unknown_bits, scale)


class InformationSelection(_Result):
    """What select_views_information returns: VolumeSelection's fields with gains in the table's units — order (n_selected,) int64
    and gains (n_selected,) int64 on the host (gain j = the weights view order[j] added when it was chosen), poses / quats (the
    chosen rows in selection order, on the device), revealed (an ops.OccupancyGrid: the caller's `claimed` plus every voxel the chosen
    views inform — the next robot's `claimed`), total = sum(gains), travel ((n_selected,) f32 metres, or None) — and table, the
    (256,) weights the selection used, on the host."""
    __slots__ = ("order", "gains", "poses", "quats", "revealed", "total", "travel", "table")

    @property
    def n_selected(self):
        return int(self.order.shape[0])


def _information_setup(what, evidence_map, camera, table):
    """view_information's and select_views_information's map, camera keywords and table -> (ops.Camera, min_dist, max_dist, table)."""
    if not isinstance(evidence_map, ops.EvidenceMap):
        raise ValueError(f"{what}: the map must be an ops.EvidenceMap (a SpaceMap has no evidence bytes to weigh), got "
                         f"{type(evidence_map).__name__}")
    _, cam, mn, mx = _volume_setup(what, evidence_map, camera)
    return cam, mn, mx, information_table(evidence_map) if table is None else table


def view_information(evidence_map, poses, quats, table=None, claimed=None, **camera):
    """How much is left to learn about what a camera would see from here?  (M,) int64 on the device: per view poses[w] (M,3) /
    quats[w] (M,4) wxyz the sum of the weights table[L + 128] of the voxels of the ops.EvidenceMap — of any state, with a positive
    weight and not set in `claimed` — whose centre lies inside the camera frustum and the depth limits and is in line of sight of
    the camera through the occupied voxels ("Information gain").  table: None (information_table(evidence_map)) or
    256 integers in [0, 65535].  A voxel seen once keeps most of its weight, a weakly occupied surface attracts a view, and a
    voxel at a clamp weighs nothing.  Unknown voxels do not block.  Keywords: the camera, as view_volume takes it.  The map is read
    when the call is made: an integrate between two calls is seen.  Exact integers: the same gains in every run."""
    cam, mn, mx, table = _information_setup("view_information", evidence_map, camera, table)
    return ops.view_information(evidence_map, poses, quats, cam, mn, mx, table=table, claimed=claimed)


def select_views_information(evidence_map, cand_poses, cand_quats, k, min_gain=1, table=None, claimed=None, travel=None, travel_weight=0.0,
                             **camera):
    """select_views_volume with view_information's objective ("Information gain"): out of the M <= 65 535 candidates
    choose up to k that together inform the largest weight of the ops.EvidenceMap's voxels.  Round after round every candidate
    not yet taken is scored against the voxels claimed so far, the largest gain wins (ties go to the lowest index), and the
    winner's voxels are claimed; selection stops after k views, when none is left, or when the best gain is below min_gain (an
    integer >= 1 in the table's units).  A weighted coverage: monotone submodular, so greedy is within (1 - 1/e) of the best set.
    The candidate plane is rebuilt on every call (one launch, then 3 k), one host synchronisation at the end.  travel, travel_weight:
    as select_views_volume takes them, travel_weight in table units per metre; refused by name on a map so large that
    65535 x voxels x 2^20 could reach 2^63.  -> InformationSelection."""
    what = "select_views_information"
    cam, mn, mx, table = _information_setup(what, evidence_map, camera, table)
    cost, m = None, 0
    if travel is not None:
        m = _travel_weight_fixed(what, travel, travel_weight)
        ops.check_view_information(evidence_map, cand_poses, cand_quats, table, k, min_gain, claimed, travel=True)
        cost = travel.cost(cand_poses.detach().to(device=evidence_map.device, dtype=torch.float32).contiguous())
    elif travel_weight != 0.0:
        raise ValueError(f"{what}: travel_weight needs travel= (an ops.TravelField)")
    order, gains, revealed = ops.view_information_select(evidence_map, cand_poses, cand_quats, cam, mn, mx, k, table, min_gain, claimed,
                                                         travel_cost=cost, travel_m=m)
    host = ops.check_information_table(table).cpu().view(torch.uint16)
    return InformationSelection(table=host, **_selection_fields(evidence_map.device, cand_poses, cand_quats, order, gains, revealed, travel))


class RayHits(_Result):
    """What cast_rays returns, on the device: voxel (R,) int32 (the hit's linear index i + nx (j + ny k), -1 clear, -2 an endpoint
    out of range), ijk (R,3) int32 (the hit voxel, (-1, -1, -1) without one), lam (R,) f32 (where along a -> b the ray enters it, 1
    clear, NaN out of range) and points (R,3) f32 (the hit voxel's centre by export()'s rule, b where clear, NaN out of range)."""
    __slots__ = ("voxel", "ijk", "lam", "points")


def _scanned_grid(what, grid_or_map):
    """The occupancy grid a cast walks: an ops.OccupancyGrid, or the occupied plane of an ops.SpaceMap / ops.EvidenceMap."""
    g = grid_or_map.occupied if isinstance(grid_or_map, (ops.SpaceMap, ops.EvidenceMap)) else grid_or_map
    if not isinstance(g, ops.OccupancyGrid):
        raise ValueError(f"{what}: the map must be an ops.OccupancyGrid, an ops.SpaceMap or an ops.EvidenceMap, got {type(grid_or_map).__name__}")
    return g


def _voxel_rows(grid, voxel):
    """Linear voxel indices (any shape; negative: no voxel) -> (ijk (..., 3) int32, -1 where there is none; centres (..., 3) f32 by
    export()'s rule fl(origin + fl(fl(i + 0.5) r)), NaN where there is none)."""
    nx, ny, _ = grid.dims
    has = (voxel >= 0).unsqueeze(-1)
    v = voxel.clamp(min=0)
    ijk = torch.stack([v % nx, (v // nx) % ny, v // (nx * ny)], dim=-1)
    o = torch.from_numpy(np.asarray(grid.origin, dtype=np.float32)).to(voxel.device)
    r = torch.tensor(grid.resolution, dtype=torch.float32, device=voxel.device)
    centres = o + (ijk.to(torch.float32) + 0.5) * r
    return torch.where(has, ijk, torch.full_like(ijk, -1)), torch.where(has, centres, torch.full_like(centres, float("nan")))


def cast_rays(grid_or_map, a, b, skip=(1, 0)):
    """Where does each segment a[i] -> b[i] stop in the map?  a, b (R,3) world points on the map's device -> RayHits (DESIGN.md 10,
    "Ray casts and depth scans").  The walk and the tests are line_of_sight's: a ray is clear here exactly where line_of_sight(a, b,
    skip) says 1.  With the default skip (1, 0) a's own voxel and b's voxel are not tested.  grid_or_map: an ops.OccupancyGrid, or
    an ops.SpaceMap / ops.EvidenceMap (its occupied plane).  Hits are reported at voxel granularity."""
    grid = _scanned_grid("cast_rays", grid_or_map)
    voxel, lam = grid.cast(a, b, skip)
    ijk, centres = _voxel_rows(grid, voxel)
    far = b.detach().to(device=grid.device, dtype=torch.float32)
    points = torch.where((voxel == -1).unsqueeze(-1), far, centres)
    return RayHits(voxel=voxel, ijk=ijk, lam=lam, points=points)


class DepthScan(_Result):
    """What depth_scan returns, on the device, each image indexed [view][row][column]: depth (V,H,W) f32 (the z-depth at which the
    ray enters the hit voxel, +inf without a return, NaN where skipped), voxel (V,H,W) int32 (the hit's linear index, -1, -2),
    flags (V,H,W) uint8 (0 a return, 1 no return within max_dist, 2 skipped: the pose or the far point out of range, 3 blocked
    nearer than min_dist), points (V,H,W,3) f32 or None (flag 0: the hit voxel's centre, flag 1: the far point, else NaN), grid (the
    scanned ops.OccupancyGrid).  far and visible() are computed when asked for."""
    __slots__ = ("depth", "voxel", "flags", "points", "grid", "_rays", "_far")

    @property
    def far(self):
        """(V,H,W,3) f32: every pixel's far point B at z-depth max_dist, with the kernel's own operations in its order (the pixel
        directions and the normalised quaternions come from the host, V x 4 and W + H numbers: one synchronisation)."""
        if self._far is None:
            poses, quats, K, D = self._rays
            f32 = np.float32
            V, H, W = self.depth.shape
            dev = self.depth.device
            q = quats.detach().cpu().numpy().astype(f32)
            ss = q[:, 0] * q[:, 0]
            for a in (1, 2, 3):
                ss = ss + q[:, a] * q[:, a]
            nn = np.maximum(np.sqrt(ss), f32(1e-12)).astype(f32)
            q = torch.from_numpy((q / nn[:, None]).astype(f32)).to(dev)
            bx = torch.from_numpy((((np.arange(W).astype(f32) - K[2]) / K[0]).astype(f32) * D).astype(f32)).to(dev).view(1, 1, W)
            by = torch.from_numpy((((np.arange(H).astype(f32) - K[5]) / K[4]).astype(f32) * D).astype(f32)).to(dev).view(1, H, 1)
            bz = torch.full((1, 1, 1), float(D), dtype=torch.float32, device=dev)
            bw = torch.zeros((1, 1, 1), dtype=torch.float32, device=dev)
            aw, ax, ay, az = (q[:, i].view(V, 1, 1) for i in range(4))
            cw, cx, cy, cz = aw, -ax, -ay, -az
            ow = aw * bw - ax * bx - ay * by - az * bz
            ox = aw * bx + ax * bw + ay * bz - az * by
            oy = aw * by - ax * bz + ay * bw + az * bx
            oz = aw * bz + ax * by - ay * bx + az * bw
            r = (ow * cx + ox * cw + oy * cz - oz * cy, ow * cy - ox * cz + oy * cw + oz * cx, ow * cz + ox * cy - oy * cx + oz * cw)
            t = poses.detach().to(device=dev, dtype=torch.float32)
            self._far = torch.stack([(r[a] + t[:, a].view(V, 1, 1)).expand(V, H, W) for a in range(3)], dim=-1).contiguous()
        return self._far

    def visible(self):
        """The visible surface of the map as a cloud -> (ijk (F,3) int32, centres (F,3) f32): the hit voxels of the flag-0 pixels,
        each once, in brick order — a hit plane of the scan's own, listed by export().  The cloud to give ModelTraj, propose_views or
        select_views as "points".  One synchronisation (F)."""
        g = self.grid
        plane = g.empty_like()
        v = torch.unique(self.voxel[self.flags == 0].long())
        nx, ny, _ = g.dims
        x, y, z = v % nx, (v // nx) % ny, v // (nx * ny)
        nbx, nby = (nx + 3) // 4, (ny + 3) // 4
        word = ((z >> 1) * nby + (y >> 2)) * nbx + (x >> 2)
        bit = (x & 3) | ((y & 3) << 2) | ((z & 1) << 4)
        # distinct voxels are distinct bits: per byte of the plane their sum is their OR
        acc = torch.zeros(plane.buf.numel() - 256, dtype=torch.int32, device=g.device)
        acc.index_add_(0, word * 4 + (bit >> 3), (1 << (bit & 7)).to(torch.int32))
        plane.buf[256:] = acc.to(torch.uint8)
        return plane.export()


def depth_scan(grid_or_map, poses, quats, into=None, points=False, **camera):
    """What would a depth sensor at these poses return?  Per view poses[w] (V,3) / quats[w] (V,4) wxyz and per pixel, the ray through
    the pixel is cast through the map's occupied voxels up to z-depth max_dist ("Ray casts and depth scans")
    -> DepthScan.  grid_or_map: an ops.OccupancyGrid, or an ops.SpaceMap / ops.EvidenceMap (its occupied plane): a ground-truth grid
    makes this a simulated sensor, the robot's own map the measurement it expects.  Keywords: intrins, img_width, img_height[,
    min_dist = 1, max_dist = 5], as view_volume takes them; intrins must be (fx 0 cx; 0 fy cy; 0 0 1).

    into: a DIFFERENT map of the scanned grid's geometry that receives the scan — an ops.SpaceMap has its occupied plane marked with
    the hit voxels and its free plane with the voxels the rays passed, directly by the kernel; an ops.EvidenceMap has its scratch
    planes marked and then takes one fold: one call is one scan, however many views.  points=True also returns the per-pixel
    points.  Hits are reported at voxel granularity (voxel centres); there is no beam divergence and no noise."""
    grid = _scanned_grid("depth_scan", grid_or_map)
    allowed = {"intrins", "img_width", "img_height", "min_dist", "max_dist"}
    if set(camera) - allowed:
        raise ValueError(f"depth_scan: unknown keyword(s) {sorted(set(camera) - allowed)}")
    missing = [k for k in ("intrins", "img_width", "img_height") if k not in camera]
    if missing:
        raise ValueError(f"depth_scan: the camera is needed: {missing} missing")
    mn, mx = camera.get("min_dist", 1.0), camera.get("max_dist", 5.0)
    hit = free = None
    if into is not None:
        if not isinstance(into, (ops.SpaceMap, ops.EvidenceMap)):
            raise ValueError(f"depth_scan: into must be an ops.SpaceMap or an ops.EvidenceMap, got {type(into).__name__}")
        target = into._scan if isinstance(into, ops.EvidenceMap) else into
        hit, free = target.occupied, target.free
        if into is grid_or_map or any(p is grid for p in (into.occupied, into.free, hit, free)):
            raise ValueError("depth_scan: into must be a different map from the one that is scanned")
    ops.check_depth_scan(grid, poses, quats, camera["intrins"], camera["img_width"], camera["img_height"], mn, mx, hit, free)
    cam = ops.Camera(camera["intrins"], camera["img_width"], camera["img_height"], mn, mx)
    voxel, depth, flags, pts = ops.depth_scan(grid, poses, quats, cam, mn, mx, hit, free, points)
    if isinstance(into, ops.EvidenceMap):
        into._fold(hit, free, True)
    K = np.asarray(list(cam.c.K), dtype=np.float32)
    return DepthScan(depth=depth, voxel=voxel, flags=flags, points=pts, grid=grid, _rays=(poses, quats, K, np.float32(mx)), _far=None)


def _clearance_cloud(points_or_cloud_or_model, what, field=False):
    """The packed cloud behind a clearance query's first argument: a ModelTraj (its cloud), an ops.PackedCloud (sorted or not) or
    (N,3) points (packed here) — checked, nothing launched: -> (cloud or None, points or None).  field=True: an ops.ClearanceField
    is accepted too and comes back in the cloud's place (leg_query asks it)."""
    c = ops._model_cloud(points_or_cloud_or_model, what)
    if isinstance(c, ops.PackedCloud) or (field and isinstance(c, ops.ClearanceField)):
        return c, None
    if not torch.is_tensor(c) or c.dim() != 2 or c.shape[1] != 3 or c.shape[0] == 0:
        raise ValueError(f"{what}: points must be an (N,3) tensor with N > 0, a PackedCloud or a ModelTraj, got "
                         f"{tuple(c.shape) if torch.is_tensor(c) else type(c).__name__}")
    return None, c


def leg_query(cloud_or_field, a, b, radius, stage="edges"):
    """(d, idx, s) of the legs a[e] -> b[e], (E,3) f32 contiguous on the source's device — the one query behind edge_clearance,
    build_roadmap, plan_path, plan_tour and refine_path.  A PackedCloud: the swept clearance query through one of its two stages
    ('edges': tohip_clearance_edges; 'segments': tohip_clearance_segments over two-waypoint paths — the same bits).  An
    ops.ClearanceField: field.edges (idx -1 iff the field certifies the leg)."""
    if isinstance(cloud_or_field, ops.ClearanceField):
        return cloud_or_field.edges(a, b, radius)
    if stage == "edges":
        return ops.clearance_edges(cloud_or_field, a, b, radius)
    return ops.clearance_segments(cloud_or_field, torch.stack([a, b], dim=1).reshape(-1, 3), radius, n_traj=a.shape[0])


def edge_clearance(points_or_cloud_or_model, a, b, radius):
    """How far each straight segment a[e] -> b[e] is from the cloud: (d, idx, s) on the device, (E,) each — trajectory_clearance's
    segment query (segments=True) for E unrelated segments: d f32 the distance to the nearest point within `radius` (+inf when
    none), idx int32 that point's row in the caller's order (-1 when none, or an end that is not finite), s f32 where along the
    segment its closest point lies.  The same bits as the query over the two-waypoint path a[e], b[e].
    With an ops.ClearanceField in the cloud's place the map answers (ClearanceField.edges): idx -1 iff the field certifies that the
    leg keeps `radius` from every obstacle voxel, else d the gap in metres and idx the voxel's linear index (-2: out of range)."""
    cloud, pts = _clearance_cloud(points_or_cloud_or_model, "edge_clearance", field=True)
    a, b = torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    if a.dim() != 2 or a.shape[1] != 3 or a.shape[0] == 0 or b.shape != a.shape:
        raise ValueError(f"edge_clearance: a and b must both be (E,3) with E > 0, got {tuple(a.shape)} and {tuple(b.shape)}")
    r = ops.check_tour_radius(radius)
    if cloud is None:
        cloud = ops.PackedCloud(pts.to(torch.float32))
    return leg_query(cloud, a.to(cloud.device), b.to(cloud.device), r)


class Tour(_Result):
    """What plan_tour returns.  order (m,) int64 on the host: the reachable nodes in visiting order, order[0] == 0; unreachable (n,)
    bool; walk: the list of node indices actually travelled — the order with the nodes a leg passes through inserted (and the way
    back to node 0 when closed); poses / quats: the walk's rows on the device (a pass-through node keeps its own quaternion; quats is
    None when none were given), ready for ModelTraj.sharing_cloud_of; length / nn_length: the walk's length and the nearest-neighbour
    start's, metres in f64 from the integer sums length_fixed / nn_length_fixed (units of 2^-20 m); moves, converged: the 2-opt
    moves made and whether no improving move is left; blocked (n,n) bool on the host: the pairs whose straight leg comes within the
    clearance radius of the cloud; edge_distance (n,n) f32 on the device: that leg's distance to the cloud, +inf where it keeps the
    radius (and on the diagonal); D (n,n) int64 / nxt (n,n) int32 on the host: the shortest open route between every two nodes and
    its first step.
    With via= (a free-space roadmap behind the legs; None otherwise): roadmap: the Roadmap over [poses; via]; via_flag (n,n) bool on
    the host: the legs that run over the roadmap because that is shorter than the straight leg (or the straight leg is blocked);
    walk_nodes: the walk as indices into [poses; via], every such leg expanded into the roadmap's nodes — poses / quats then follow
    walk_nodes (a free-space node takes the quaternion of the view its leg leads to), walk keeps listing tour nodes only.
    With travel=True: via_flag marks the legs that run over the map's travel field, poses / quats hold those legs expanded into the
    route's voxel centres (they take the quaternion of the view they lead to); roadmap and walk_nodes stay None."""
    __slots__ = ("order", "unreachable", "walk", "poses", "quats", "length", "nn_length", "length_fixed", "nn_length_fixed", "moves",
                 "converged", "blocked", "edge_distance", "D", "nxt", "roadmap", "via_flag", "walk_nodes")


def tour_edge_stage(cloud, n_edges):
    """Which of the two edge stages answers n_edges segments over `cloud` sooner — the same bits either way.  'segments': one 16-wave
    block per edge (tohip_clearance_segments over two-waypoint paths), about 25 ns per edge whatever the cloud; 'edges': one wave per
    edge (tohip_clearance_edges), 4 to 13 ns per edge behind a floor of one wave's walk over all tile spheres, 64 at a time.  Measured
    crossings (tools/time_tour.py --sweep): about 1 100 edges on the bundled cloud (159 tiles), about 5 600 at 1 M
    points (4 096 tiles)."""
    return "edges" if n_edges >= 1024 + 64 * -(-cloud.npad // 16384) else "segments"


def tour_edge_query(cloud, nodes, radius, stage=None):
    """(d, idx, s) of every edge i < j of `nodes` (n,3) in edge-index order (the upper triangle, row-major) through one of the two
    edge stages (stage=None: tour_edge_stage's choice)."""
    i, j = ops.tour_edge_ends(nodes.shape[0], nodes.device)
    a, b = nodes[i], nodes[j]
    if isinstance(cloud, ops.ClearanceField):
        return leg_query(cloud, a.contiguous(), b.contiguous(), radius)
    return leg_query(cloud, a, b, radius, stage or tour_edge_stage(cloud, a.shape[0]))


def plan_tour(points_or_cloud_or_model, poses, quats=None, clearance_radius=None, closed=False, max_moves=None, via=None, via_k=12,
              via_max_edge=None, travel=False, space=None, weights=None):
    """A short visiting order through view poses whose every straight leg keeps clearance_radius from the cloud.
    poses (n,3), 2 <= n <= 256: row 0 is where the tour starts (the robot), the others are the views (select_views' sel.poses);
    quats (n,4) or None.  Every pair of nodes is put to the swept clearance query (edge_clearance); the pairs it finds nothing near
    are the open legs.  Shortest open routes between all nodes (Floyd-Warshall), a nearest-neighbour order from node 0 over them and
    best-improvement 2-opt (at most max_moves moves, default 4 n; 0: the nearest-neighbour order) run on the device in integer
    arithmetic — lengths in units of 2^-20 m — so every run gives the same tour.  Where the direct leg is blocked the walk passes
    through other nodes; nodes no open route reaches are reported in `unreachable` and left out.  closed=True: the tour returns to
    node 0.  clearance_radius=None: no query, every leg is open.
    points_or_cloud_or_model: (N,3) points on the device, an ops.PackedCloud (sorted or not) or a ModelTraj (its cloud).
    via (F,3), optional: free-space nodes (synth.roadmap_lattice, say), n + F <= 16 384; clearance_radius is then required.  A
    roadmap (build_roadmap, k = via_k, max_edge = via_max_edge) over [poses; via] gives every pair of tour nodes its shortest
    collision-checked route, and a leg takes it wherever that beats the straight leg: a view behind a wall is reached through the
    doorway.  A via node that coincides with a pose is left out (its row is made non-finite: the index of every other node stays).
    travel=True (the first argument must then be an ops.ClearanceField, clearance_radius is required and via= must be None): the
    map itself stands behind the legs.  travel_matrix over the n tour nodes (space=: an ops.SpaceMap, known-free voxels only) gives
    every pair its route length along the travel field's metric, converted to the tour's unit (synth.tour_travel_units) and handed
    to the same planner as via_D; a leg takes the map route wherever that beats the open straight leg (via_flag).  Such a leg u ->
    v is walked as pose u, the voxel centres of fields.paths(pose v, field u), pose v; the first and the last hop stay inside the
    end voxels' certified cubes, every other hop joins two 26-neighbours, so every hop is a leg field.edges calls open, and the rows
    go into refine_path(field, ...) as any tour's do.  A path's rows take the quaternion of the view they lead to; walk_nodes and
    roadmap stay None.  No lattice, no node limit: the map of any size is the roadmap.  weights (an ops.TravelWeights, needs
    travel=True): the matrix is the weighted one, so a map route is priced by its weighted cost against the straight leg's length.
    -> Tour.  Launches only, then one copy to the host (with via: one read-back per batch of route sweeps before it; with travel:
    the build's read-backs before it and one for the paths after it)."""
    if not isinstance(travel, (bool, np.bool_)):
        raise ValueError(f"plan_tour: travel must be True or False, got {travel!r}")
    if travel:
        if not isinstance(points_or_cloud_or_model, ops.ClearanceField):
            raise ValueError(f"plan_tour: travel=True needs an ops.ClearanceField as the first argument, got {type(points_or_cloud_or_model).__name__}")
        if via is not None:
            raise ValueError("plan_tour: travel=True and via= exclude each other (the map is the roadmap)")
        if clearance_radius is None:
            raise ValueError("plan_tour: travel=True needs a clearance_radius (a finite number > 0), got None")
    elif space is not None:
        raise ValueError("plan_tour: space= needs travel=True")
    if weights is not None and not travel:
        raise ValueError("plan_tour: weights= needs travel=True")
    cloud, pts = _clearance_cloud(points_or_cloud_or_model, "plan_tour", field=True)
    n, r, max_moves = ops.check_tour(poses, quats, clearance_radius, closed, max_moves)
    if via is not None:
        _check_via(via, n)
        if r is None:
            raise ValueError("plan_tour: via needs a clearance_radius (a finite number > 0), got None")
        k, _, _ = ops.check_roadmap_options(via_k, r, via_max_edge)
    cloud = _device_cloud(cloud, pts, "plan_tour", pack=r is not None, radius=r)
    dev = cloud.device if cloud is not None else pts.device
    nodes = allnodes = poses.detach().to(device=dev, dtype=torch.float32).contiguous()
    qs = quats.detach().to(device=dev, dtype=torch.float32).contiguous() if quats is not None else None
    rm = None
    if via is not None:   # the roadmap over [poses; via] and the routes from every tour node
        allnodes = _join_nodes(nodes, via.detach().to(device=dev, dtype=torch.float32))
        rm = _build_roadmap(cloud, allnodes, r, k, via_max_edge)
        routes = rm.routes(list(range(n)))
    E, M = n * (n - 1) // 2, allnodes.shape[0]
    d, idx, _ = tour_edge_query(cloud, nodes, r) if r is not None else (None, None, None)
    dist = _symmetric(n, ops.tour_edge_ends(n, dev), d, float("inf"), torch.float32)
    tail = [idx.view(torch.uint8)] if idx is not None else []
    tm = None
    if travel:   # the map's route lengths between the tour nodes, in the tour's unit
        tm = travel_matrix(cloud, nodes, r, space=space, weights=weights)
        scale = float(np.float32(cloud.resolution)) * 16384.0   # (synth.tour_travel_units: one rounded f64 product, half to even)
        via_D = torch.where(tm.cost < 0, torch.full_like(tm.cost, ops.ROADMAP_INF), torch.round(tm.cost.clamp(min=0).double() * scale).long())
        buf, flag = ops.tour_plan_via(nodes, idx, via_D.contiguous(), closed, max_moves)
        tail += [flag.reshape(-1)]
    elif rm is None:
        buf = ops.tour_plan(nodes, idx, closed, max_moves)
    else:
        buf, flag = ops.tour_plan_via(nodes, idx, routes.D, closed, max_moves)
        tail += [routes.pred.reshape(-1).view(torch.uint8), flag.reshape(-1)]
    # the one synchronisation: the tour buffer, the edges' answers and (with via) the routes' predecessors and the flags in one copy
    h = torch.cat([buf] + tail).cpu()
    hdr, order, unreachable, D, nxt = _unpack_tour(h, n)
    o = ops.tour_layout(n)["total"]
    hit = h[o:o + 4 * E].view(torch.int32) != -1 if idx is not None else None
    blocked = _symmetric(n, ops.tour_edge_ends(n, "cpu"), hit, False, torch.bool)
    from .synth import tour_walk   # (numpy only)
    walk = tour_walk(order.tolist(), nxt.numpy(), closed)
    via_flag, walk_nodes, q_of = None, None, walk   # q_of: the tour node whose quaternion each row of the walk takes
    if rm is not None:   # every leg that runs over the roadmap expanded into its nodes
        o += 4 * E
        pred = h[o:o + 4 * n * M].view(torch.int32).reshape(n, M).numpy()
        o += 4 * n * M
        via_flag = h[o:o + n * n].reshape(n, n) != 0
        walk_nodes, q_of = [walk[0]], [walk[0]]
        for u, v in zip(walk, walk[1:]):
            hop = rm.walk(routes, u, pred[u], v)[1:] if via_flag[u, v] else [v]
            walk_nodes += hop
            q_of += [x if x < n else v for x in hop]
    w = torch.as_tensor(walk if walk_nodes is None else walk_nodes, dtype=torch.int64, device=dev)
    walk_poses = allnodes[w]
    if tm is not None:   # every leg that runs over the map expanded into its voxel centres
        via_flag = h[o + 4 * E:o + 4 * E + n * n].reshape(n, n) != 0
        legs = [(u, v) for u, v in zip(walk, walk[1:]) if via_flag[u, v]]
        paths = iter(tm.fields.paths(nodes[[v for _, v in legs]], torch.as_tensor([u for u, _ in legs], dtype=torch.int32))) if legs else None
        rows, q_of = [nodes[walk[0]][None]], [walk[0]]
        for u, v in zip(walk, walk[1:]):
            if via_flag[u, v]:
                hop = next(paths)
                rows.append(hop)
                q_of += [v] * hop.shape[0]
            rows.append(nodes[v][None])
            q_of.append(v)
        walk_poses = torch.cat(rows)
    return Tour(order=order, unreachable=unreachable, walk=walk, poses=walk_poses,
                quats=qs[torch.as_tensor(q_of, dtype=torch.int64, device=dev)] if qs is not None else None,
                length=int(hdr[3]) * ops.TOUR_UNIT, nn_length=int(hdr[4]) * ops.TOUR_UNIT, length_fixed=int(hdr[3]),
                nn_length_fixed=int(hdr[4]), moves=int(hdr[1]), converged=bool(hdr[2]), blocked=blocked, edge_distance=dist, D=D, nxt=nxt,
                roadmap=rm, via_flag=via_flag, walk_nodes=walk_nodes)


def _symmetric(n, ends, values, fill, dtype):
    """The symmetric (n,n) matrix of per-edge values: values[e] at (i[e], j[e]) and (j[e], i[e]) for ends = (i, j), `fill` elsewhere
    (and everywhere for values None), on the ends' device."""
    i, j = ends
    out = torch.full((n, n), fill, dtype=dtype, device=i.device)
    if values is not None:
        out[i, j] = values
        out[j, i] = values
    return out


def _unpack_tour(h, n):
    """A host copy h of a tour buffer (ops.tour_layout(n); anything may follow it) -> (hdr: the first 8 int64 of the header, order (m,)
    int64, unreachable (n,) bool, D (n,n) int64, nxt (n,n) int32)."""
    lay = ops.tour_layout(n)
    hdr = h[:64].view(torch.int64)
    order = h[lay["order"]:lay["order"] + 4 * n].view(torch.int32)[:int(hdr[0])].to(torch.int64)
    unreachable = h[lay["unreachable"]:lay["unreachable"] + n] != 0
    D = h[lay["D"]:lay["D"] + 8 * n * n].view(torch.int64).reshape(n, n).clone()
    nxt = h[lay["nxt"]:lay["nxt"] + 4 * n * n].view(torch.int32).reshape(n, n).clone()
    return hdr, order, unreachable, D, nxt


class RoadmapRoutes(_Result):
    """What Roadmap.routes returns: sources (the list asked for), D (S,M) int64 and pred (S,M) int32 on the device — the shortest
    route length from each source to every node over the open edges (2^62 where none exists) and, for each node, the lowest
    neighbour a shortest route arrives from (-1 for the source and the unreachable) — and sweeps, the relaxation sweeps it took."""
    __slots__ = ("sources", "D", "pred", "sweeps")


class Roadmap(_Result):
    """What build_roadmap returns, device tensors unless noted: nodes (M,3) f32; nbr (M,k) int32: each node's k nearest others (-1:
    none); length_fixed (M,k) int64: those edges' lengths in units of 2^-20 m; open (M,k) bool: the edges that keep the clearance
    radius; edge_distance (M,k) f32: a blocked edge's distance to the cloud, +inf where open (and in an empty slot); isolated (M,)
    bool: the nodes no open edge touches; n_open (an int): the open edges, each unordered pair counted once."""
    __slots__ = ("nodes", "nbr", "length_fixed", "open", "edge_distance", "isolated", "n_open", "_edges")

    def host_edges(self):
        """(u, v, L) on the host: both directions of every open slot (synth.roadmap_edges), copied once — what a walk falls back
        on when coincident nodes tie its predecessors in a circle."""
        if getattr(self, "_edges", None) is None:
            from .synth import roadmap_edges   # (numpy only)
            self._edges = roadmap_edges(self.nbr.cpu().numpy(), self.length_fixed.cpu().numpy(), self.open.cpu().numpy())
        return self._edges

    def walk(self, routes, row, pred_row, dst):
        """routes.sources[row], ..., dst: along pred_row (that row of routes.pred on the host), or over the tight edges where
        zero-length edges between coincident nodes close the predecessors into a circle; None when dst is not reached."""
        from .synth import roadmap_walk   # (numpy only)
        return roadmap_walk(pred_row, routes.sources[row], dst, tight=lambda: (routes.D[row].cpu().numpy(), self.host_edges()))

    def routes(self, sources, sweeps_per_check=8):
        """Shortest routes from up to 256 source nodes to every node -> RoadmapRoutes."""
        _, _, _, _, src = ops.check_roadmap(self.nodes, self.nbr.shape[1], None, None, sources, sweeps_per_check)
        if src is None:
            raise ValueError("sources must be given")
        D, pred, sweeps = ops.roadmap_routes(self.nbr, self.length_fixed, self.open, src, sweeps_per_check)
        return RoadmapRoutes(sources=src, D=D, pred=pred, sweeps=sweeps)

    def route(self, src, dst):
        """The shortest open route between two nodes -> (walk: the node indices src, ..., dst; length_fixed; length in metres), or
        None when there is none.  One routes() call and one copy to the host."""
        M = self.nodes.shape[0]
        for name, v in (("src", src), ("dst", dst)):
            if isinstance(v, bool) or not hasattr(v, "__index__") or not 0 <= v < M:
                raise ValueError(f"{name} must be a node index in [0, {M}), got {v!r}")
        r = self.routes([int(src)])
        h = torch.cat([r.D[0, dst].reshape(1).view(torch.int32), r.pred[0]]).cpu()
        walk = self.walk(r, 0, h[2:].numpy(), dst)
        if walk is None:
            return None
        fixed = int(h[:2].view(torch.int64))
        return walk, fixed, fixed * ops.TOUR_UNIT


def _device_cloud(cloud, pts, what, pack=True, radius=None):
    """The packed cloud of a _clearance_cloud pair: the points are packed here, which is the first GPU call (pack=False: only
    checked to be on the device, and None comes back for them).  A ClearanceField comes back as it is, once it can certify `radius`
    (ValueError otherwise, before anything is launched)."""
    if isinstance(cloud, ops.ClearanceField) and radius is not None:
        cloud.need2(radius)
    if cloud is None:
        if not pts.is_cuda:
            raise ValueError(f"{what}: points must live on a HIP device, got {pts.device}")
        if pack:
            cloud = ops.PackedCloud(pts.to(torch.float32))
    return cloud


def _build_roadmap(cloud, nodes, r, k, max_edge):
    """build_roadmap behind its checks: nodes (M,3) f32 contiguous on the cloud's device."""
    M = nodes.shape[0]
    nbr, length = ops.roadmap_knn(nodes, k, max_edge)
    # the edge stage: the filled slots, each asked from the lower index
    i = torch.arange(M, device=nodes.device, dtype=torch.int64)[:, None].expand(M, k).reshape(-1)
    slot = torch.nonzero(nbr.reshape(-1) >= 0).reshape(-1)
    i, j = i[slot], nbr.reshape(-1)[slot].to(torch.int64)
    lo, hi = torch.minimum(i, j), torch.maximum(i, j)
    opened = torch.zeros(M * k, dtype=torch.bool, device=nodes.device)
    dist = torch.full((M * k,), float("inf"), dtype=torch.float32, device=nodes.device)
    if slot.numel():
        d, idx, _ = leg_query(cloud, nodes[lo], nodes[hi], r)
        free = (idx == -1) & (length.reshape(-1)[slot] <= ops.ROADMAP_MAX_LEN)
        opened[slot] = free
        dist[slot] = d
        lo, hi = lo[free], hi[free]
    opened, dist = opened.view(M, k), dist.view(M, k)
    touched = torch.zeros(M, dtype=torch.bool, device=nodes.device)
    touched[lo] = True
    touched[hi] = True
    pairs = lo * M + hi
    n_open = int(torch.unique(pairs).numel())
    return Roadmap(nodes=nodes, nbr=nbr, length_fixed=length, open=opened, edge_distance=dist, isolated=~touched, n_open=n_open,
                   _edges=None)


def build_roadmap(points_or_cloud_or_model, nodes, clearance_radius, k=12, max_edge=None):
    """A roadmap over caller-supplied free-space nodes: nodes (M,3), 2 <= M <= 16 384 (synth.roadmap_lattice makes a
    lattice); every node is joined to its k <= 32 nearest others (no further than max_edge when that is given) by the exact f64 key
    (d2, j), ties to the lower index, and an edge is open when the swept clearance query (edge_clearance, asked from the lower index)
    finds no cloud point within clearance_radius of it.  The graph is undirected: a pair is an edge when either list names it open.
    Lengths are integers in units of 2^-20 m, so routes over it are the same bits in every run.  -> Roadmap."""
    cloud, pts = _clearance_cloud(points_or_cloud_or_model, "build_roadmap", field=True)
    if clearance_radius is None:
        ops.check_tour_radius(clearance_radius)   # (raises: a roadmap needs one)
    _, k, r, me, _ = ops.check_roadmap(nodes, k, clearance_radius, max_edge)
    cloud = _device_cloud(cloud, pts, "build_roadmap", radius=r)
    q = nodes.detach().to(device=cloud.device, dtype=torch.float32).contiguous()
    return _build_roadmap(cloud, q, r, k, max_edge)


class PlannedPath(_Result):
    """What plan_path returns: poses (L,3) f32 on the device: start, the free-space nodes of the route, goal — every leg keeps the
    clearance radius; length in metres (f64 from the integer length_fixed, units of 2^-20 m); walk: the route as indices into
    [start; goal; via]; roadmap: the Roadmap it ran over."""
    __slots__ = ("poses", "length", "length_fixed", "walk", "roadmap")


def _point3(p, name, device):
    t = torch.as_tensor(p, dtype=torch.float32).detach()
    if t.numel() != 3:
        raise ValueError(f"{name} must hold 3 coordinates, got shape {tuple(t.shape)}")
    return t.reshape(1, 3).to(device)


def _check_via(via, n, what="via"):
    ops._check_float_rows(via, what, "a floating-point tensor of shape (F,3) with F > 0", 3, empty=False)
    if n + via.shape[0] > ops.ROADMAP_MAX_NODES:
        raise ValueError(f"{what}: the roadmap holds at most {ops.ROADMAP_MAX_NODES} nodes, got {n} + {via.shape[0]}")


def _join_nodes(head, via):
    """[head; via] with the via rows that coincide with a head row made non-finite: such a node has no edge, and no zero-length
    edge ties it to its twin."""
    twin = (via[:, None, :] == head[None, :, :]).all(dim=2).any(dim=1)
    return torch.cat([head, torch.where(twin[:, None], torch.full_like(via, float("nan")), via)]).contiguous()


def plan_path(points_or_cloud_or_model, start, goal, via, clearance_radius, k=12, max_edge=None):
    """A path from start to goal that keeps clearance_radius from the cloud, over the free-space nodes `via` (F,3): the shortest
    route of the roadmap over [start; goal; via] (build_roadmap).  -> PlannedPath, whose poses are an initial path for
    ModelTraj.sharing_cloud_of(..., clearance_mode='segments'); ValueError when no route exists."""
    cloud, pts = _clearance_cloud(points_or_cloud_or_model, "plan_path", field=True)
    _check_via(via, 2)
    if clearance_radius is None:
        ops.check_tour_radius(clearance_radius)   # (raises: a path needs one)
    k, r, _ = ops.check_roadmap_options(k, clearance_radius, max_edge)
    ends = torch.cat([_point3(start, "start", "cpu"), _point3(goal, "goal", "cpu")])
    cloud = _device_cloud(cloud, pts, "plan_path", radius=r)
    dev = cloud.device
    nodes = _join_nodes(ends.to(dev), via.detach().to(device=dev, dtype=torch.float32))
    rm = _build_roadmap(cloud, nodes, r, k, max_edge)
    got = rm.route(0, 1)
    if got is None:
        raise ValueError(f"plan_path: no route from start to goal keeps {r} m from the cloud over these {via.shape[0]} via nodes")
    walk, fixed, length = got
    return PlannedPath(poses=nodes[torch.as_tensor(walk, dtype=torch.int64, device=dev)], length=length, length_fixed=fixed, walk=walk,
                       roadmap=rm)


def travel_fields(field, starts, radius, space=None, max_dist=None, weights=None):
    """One travel field per start, all built in the same worklist rounds: an ops.TravelFields ("Travel fields in
    batches") over `starts` (S,3), S <= 256 — a team's robots, a tour's views.  fields[b] is the ops.TravelField of start b (no
    copy), fields.cost(positions) / .distance / .reachable answer (S,M) at once, fields.paths(goals, goal_field) walks each goal in
    the field it names.  Field b is bit for bit travel_field(field, starts[b], ...).  weights: one ops.TravelWeights for all fields, as
    travel_field's."""
    if not isinstance(field, ops.ClearanceField):
        raise ValueError(f"travel_fields: field must be an ops.ClearanceField, got {type(field).__name__}")
    return ops.TravelFields(field, radius, ops._check_rows3(starts, "starts"), space=space, max_dist=max_dist, weights=weights)


class TravelMatrix(_Result):
    """What travel_matrix returns: cost (M,M) int64 on the device, cost[i][j] the cost in 1/64 voxel edge, in the field seeded at
    position i, of position j's voxel (-1: unreachable — a whole row where i was not seeded — and -2 in the columns out of range or
    outside dims); distance (M,M) f32 metres (+inf / NaN); seeded (M,) uint8; fields: the ops.TravelFields behind it."""
    __slots__ = ("cost", "distance", "seeded", "fields")


def travel_matrix(field, positions, radius, space=None, max_dist=None, weights=None):
    """The map distance between every two of `positions` (M,3), M <= 256: what the robot must travel, not the straight line.
    -> TravelMatrix.  One batched build, one lookup launch.  Symmetric wherever both rows are seeded: an allowed move is allowed
    both ways at the same weight.  weights (travel_field's): the weighted cost of every pair, still symmetric — a step's cost is
    symmetric in its two voxels."""
    fields = travel_fields(field, positions, radius, space, max_dist, weights)
    cost, distance = fields._positions(fields.sources, True, True)
    return TravelMatrix(cost=cost, distance=distance, seeded=fields.seeded, fields=fields)


class FrontierAssignment(_Result):
    """What assign_frontiers returns, all on the device.  clusters: frontier_clusters(...) without travel (K rows: descending size,
    then ascending id); cost_fixed (R,K) int64: robot r's cost, in 1/64 voxel edge, to cluster k's nearest voxel (-1 unreachable);
    cost (R,K) f64 metres (inf); approach (R,K,3) f32 that voxel's centre (NaN where unreachable); goal (R,) int64: the row of
    clusters robot r is sent to, -1 for none; goal_position (R,3) f32 = approach[r, goal[r]] (NaN) and goal_cost (R,) f64 metres
    (inf); robot_of_cluster (K,) int64, -1 where the cluster went to nobody."""
    __slots__ = ("clusters", "cost_fixed", "cost", "approach", "goal", "goal_position", "goal_cost", "robot_of_cluster")


ASSIGN_MAX_ROBOTS = 64
ASSIGN_MAX_CLUSTERS = 4096


def assign_frontiers(space_or_evidence_map, fields, min_unknown=1, min_size=1, connectivity=26, min_cost=0.0):
    """Which robot goes to which opening ("Travel fields in batches").  fields: an ops.TravelFields of the map's
    geometry with one field per robot, R <= 64.  Every frontier cluster (frontier_clusters: min_unknown, min_size, connectivity; at
    most 4096 of them) is priced from every robot by its nearest voxel — Components.min_over on fields[r], R launches with no read-
    back between them — and tohip_assign_greedy hands them out: among the pairs (robot, cluster) with a cost >= min_cost (metres;
    just above 0 keeps a robot from being sent to the opening it stands in) the cheapest goes first, ties to the lower robot, then
    the lower cluster row, and no robot or cluster is taken twice.  Greedy, not optimal; cluster size plays no part.  The same
    answer in every run.  Over weighted fields (travel_fields(..., weights=)) the price is the weighted cost.
    -> FrontierAssignment."""
    if not isinstance(fields, ops.TravelFields):
        raise ValueError(f"assign_frontiers: fields must be an ops.TravelFields, got {type(fields).__name__}")
    R = fields.n_fields
    if R > ASSIGN_MAX_ROBOTS:
        raise ValueError(f"assign_frontiers: fields must hold at most {ASSIGN_MAX_ROBOTS} fields (one per robot), got {R}")
    m = ops._float_or_nan(min_cost) if ops._is_real(min_cost) else float("nan")
    if not np.isfinite(m) or m < 0.0:
        raise ValueError(f"assign_frontiers: min_cost must be a finite number of metres >= 0, got {min_cost!r}")
    clusters = frontier_clusters(space_or_evidence_map, min_unknown, min_size, connectivity)
    comp, dev = clusters.components, clusters.ids.device
    diff = ops._grid_difference(comp.grid, fields)
    if diff:
        raise ValueError(f"assign_frontiers: the travel fields' {diff[0]} differs from the map's ({diff[2]} and {diff[1]})")
    K = clusters.n
    if K > ASSIGN_MAX_CLUSTERS:
        raise ValueError(f"assign_frontiers: {K} clusters, at most {ASSIGN_MAX_CLUSTERS} can be assigned; raise min_size (now {min_size})")
    from .synth import assign_min_cost_fixed   # (numpy only)
    priced = [comp.min_over(fields[b]) for b in range(R)]
    cost_fixed = torch.stack([v[clusters.ids] for v, _ in priced]).contiguous() if K else torch.empty((R, 0), dtype=torch.int64, device=dev)
    voxel = torch.stack([x[clusters.ids].long() for _, x in priced]) if K else torch.empty((R, 0), dtype=torch.int64, device=dev)
    reachable = cost_fixed >= 0
    nx, ny, _ = comp.dims
    v = voxel.clamp(min=0)
    ijk = torch.stack([v % nx, (v // nx) % ny, v // (nx * ny)], dim=-1)
    o = torch.from_numpy(np.asarray(comp.origin, dtype=np.float32)).to(dev)
    r32 = float(np.float32(comp.resolution))
    approach = o + (ijk.float() + 0.5) * r32   # a voxel's centre as the map computes it, in f32
    approach = torch.where(reachable[..., None], approach, torch.full_like(approach, float("nan")))
    cost = torch.where(reachable, cost_fixed.double() / 64.0 * r32, torch.full_like(cost_fixed, float("inf"), dtype=torch.float64))
    col_of_row = torch.full((R,), -1, dtype=torch.int32, device=dev)
    row_of_col = torch.full((K,), -1, dtype=torch.int32, device=dev)
    if K:
        ops._map_call(dev, "tohip_assign_greedy", ops.ptr(cost_fixed), R, K, K, assign_min_cost_fixed(m, comp.resolution), ops.ptr(col_of_row),
                      ops.ptr(row_of_col))
    goal = col_of_row.long()
    has = goal >= 0
    pick = goal.clamp(min=0)
    if K:
        rows = torch.arange(R, device=dev)
        goal_position = torch.where(has[:, None], approach[rows, pick], torch.full((R, 3), float("nan"), device=dev))
        goal_cost = torch.where(has, cost[rows, pick], torch.full((R,), float("inf"), dtype=torch.float64, device=dev))
    else:
        goal_position = torch.full((R, 3), float("nan"), device=dev)
        goal_cost = torch.full((R,), float("inf"), dtype=torch.float64, device=dev)
    return FrontierAssignment(clusters=clusters, cost_fixed=cost_fixed, cost=cost, approach=approach, goal=goal, goal_position=goal_position,
                              goal_cost=goal_cost, robot_of_cluster=row_of_col.long())


class TravelPath(_Result):
    """What travel_path returns: poses (L,3) f32 on the device, the voxel centres from the travel field's source to the goal's voxel
    (L = 0 where it is not reachable) — they go as they are into refine_path(field, path.poses, clearance_radius=radius), which
    shortcuts the 26-connected staircase; length: metres along the field's metric (inf where not reachable); cost: the integer
    behind it, in 1/64 voxel edge (-1 unreachable, -2 out of range or outside dims); reachable: bool.  Over a weighted field
    (tf.weights) cost is the weighted cost the field minimises and length the GEOMETRIC metres summed over the rows' moves (64, 91
    or 111 per move, then the same conversion): never more than cost / 64 resolution, and equal to it at kappa = 16 everywhere."""
    __slots__ = ("poses", "length", "cost", "reachable")


def travel_path(tf, goal):
    """The shortest path of the travel field `tf` (travel_field's result) to `goal` (3,) -> TravelPath.  One synchronisation."""
    if not isinstance(tf, ops.TravelField):
        raise ValueError(f"travel_path: tf must be an ops.TravelField, got {type(tf).__name__}")
    g = _point3(goal, "goal", tf.device).reshape(1, 3)
    cost = int(tf.cost(g).item())
    poses = tf.paths(g)[0] if cost >= 0 else torch.empty((0, 3), dtype=torch.float32, device=tf.device)
    length = float(tf.distance(g).item())
    if tf.weights is not None and cost >= 0:   # the geometric length of the rows: the field's unit, unweighted
        axes = ((poses[1:] - poses[:-1]).abs() > 0.5 * float(tf.resolution)).sum(dim=1)
        units = int(torch.tensor([0, 64, 91, 111], device=tf.device)[axes].sum().item())
        length = float(np.float32(np.float32(units) * np.float32(0.015625)) * np.float32(tf.resolution))
    return TravelPath(poses=poses, length=length, cost=cost, reachable=cost >= 0)


class FrontierClusters(_Result):
    """What frontier_clusters returns, one row per cluster kept, all on the device: ids (K,) int64 (the component's id in
    .components), sizes (K,) int64 voxels, centroids (K,3) f32, bbox (K,2,3) int32, cost (K,) f64 metres along the travel field's
    metric to the cluster's nearest voxel (inf: unreachable, or no travel field), approach (K,3) f32 the centre of that voxel (NaN
    where unreachable), reachable (K,) bool; frontier: the ops.Frontier clustered; components: the ops.Components of its plane."""
    __slots__ = ("ids", "sizes", "centroids", "bbox", "cost", "approach", "reachable", "frontier", "components")

    @property
    def n(self):
        return int(self.ids.shape[0])


def frontier_clusters(space_or_evidence_map, min_unknown=1, min_size=1, connectivity=26, travel=None):
    """The openings of the map ("Connected components"): the frontier voxels — free, with at least min_unknown unknown
    face neighbours — grouped into connected clusters, those smaller than min_size voxels dropped: a stray ray through a gap makes a
    one-voxel frontier, a doorway into an unscanned hall a large one.  -> FrontierClusters.

    travel (an ops.TravelField of the map's geometry; None: none) prices each cluster by its nearest voxel: rows are ordered
    reachable first, by ascending cost, then descending size, then ascending id — row 0 is the nearest reachable opening, and
    approach[reachable] goes unchanged into travel_path(travel, goal), propose_views(..., positions=...) and select_views_volume as
    candidate positions.  Without travel the rows go by descending size, then ascending id.  The order is made on the device by
    stable integer sorts.

    The cost is taken over the cluster's own voxels, so it needs a travel field in which frontier voxels are traversable: the
    pairing clearance_field(space, ..., unknown='free') with travel_field(..., space=space).  With unknown='obstacle' every frontier
    voxel touches an obstacle, none is traversable and every cluster reports unreachable.  With a weighted field the cost is the
    weighted one."""
    space = space_or_evidence_map.space if isinstance(space_or_evidence_map, ops.EvidenceMap) else space_or_evidence_map
    if not isinstance(space, ops.SpaceMap):
        raise ValueError(f"frontier_clusters: the map must be an ops.SpaceMap or an ops.EvidenceMap, got {type(space_or_evidence_map).__name__}")
    if not ops._is_int(min_size) or min_size < 1:
        raise ValueError(f"frontier_clusters: min_size must be an integer >= 1, got {min_size!r}")
    if travel is not None and not isinstance(travel, ops.TravelField):
        raise ValueError(f"frontier_clusters: travel must be an ops.TravelField or None, got {type(travel).__name__}")
    ops.check_components(space.free, connectivity, values=travel)
    front = space.frontier(min_unknown)
    comp = ops.Components(front.grid, connectivity)
    dev = space.device
    ids = torch.nonzero(comp.sizes >= int(min_size)).reshape(-1)             # ascending id
    ids = ids[torch.sort(comp.sizes[ids], stable=True, descending=True)[1]]  # ... then descending size
    K = ids.shape[0]
    if travel is None:
        value = torch.full((K,), -1, dtype=torch.int64, device=dev)
        voxel = torch.full((K,), -1, dtype=torch.int64, device=dev)
    else:
        value, voxel = comp.min_over(travel)
        key = torch.where(value < 0, torch.full_like(value, torch.iinfo(torch.int64).max), value)
        ids = ids[torch.sort(key[ids], stable=True)[1]]                      # ... then ascending cost, the unreachable last
        value, voxel = value[ids], voxel[ids].long()
    reachable = value >= 0
    nx, ny, _ = comp.dims
    v = voxel.clamp(min=0)
    ijk = torch.stack([v % nx, (v // nx) % ny, v // (nx * ny)], dim=1)
    o = torch.from_numpy(np.asarray(comp.origin, dtype=np.float32)).to(dev)
    approach = o + (ijk.float() + 0.5) * float(np.float32(comp.resolution))  # a voxel's centre as the map computes it, in f32
    approach = torch.where(reachable[:, None], approach, torch.full_like(approach, float("nan")))
    cost = torch.where(reachable, value.double() / 64.0 * float(np.float32(comp.resolution)), torch.full((K,), float("inf"), dtype=torch.float64, device=dev))
    return FrontierClusters(ids=ids, sizes=comp.sizes[ids], centroids=comp.centroids[ids], bbox=comp.bbox[ids], cost=cost, approach=approach,
                            reachable=reachable, frontier=front, components=comp)


class RefinedPath(_Result):
    """What refine_path returns.  poses (R,3) f32 and quats (R,4) f32 (None when no quaternions came in) on the device, ready for
    ModelTraj.sharing_cloud_of; row_node (R,) int32 on the host: the input row a corner row came from, -1 at an interpolated row;
    corners (m + 1,) int64 on the host: the input rows the refined path turns at, 0 first and L - 1 last; length / input_length in
    metres (f64 from the integer sums length_fixed / input_length_fixed, units of 2^-20 m); leg_blocked (L - 1,) bool on the host:
    the input legs the swept clearance query finds within the radius (reported, not acted on); n_open: the open chords that skip
    at least one node; open_band (L,W) uint8 on the device: the chord stage's answers as the search read them."""
    __slots__ = ("poses", "quats", "row_node", "corners", "length", "length_fixed", "input_length", "input_length_fixed", "leg_blocked",
                 "n_open", "open_band")


def _path_chord_band(cloud, P, kept, W, r):
    """open_band (L,W) uint8 on the device: 1 where the swept clearance query finds nothing within r of the chord (i, i + off + 1).
    Only the admissible slots are asked — no kept node strictly between the ends — gathered on the device."""
    L, dev = P.shape[0], P.device
    idx = torch.arange(L, device=dev, dtype=torch.int64)
    last = torch.cummax(torch.where(kept, idx, torch.full_like(idx, -1)), dim=0).values   # the largest kept node <= i
    i = idx[:, None].expand(L, W)
    j = i + torch.arange(1, W + 1, device=dev, dtype=torch.int64)[None, :]
    ask = j < L
    ask &= last[(j - 1).clamp(max=L - 1)] <= i
    slot = torch.nonzero(ask.reshape(-1)).reshape(-1)
    band = torch.zeros(L * W, dtype=torch.uint8, device=dev)
    _, hit, _ = leg_query(cloud, P[i.reshape(-1)[slot]], P[j.reshape(-1)[slot]], r)   # (the input legs are always asked)
    band[slot] = (hit == -1).to(torch.uint8)
    return band.view(L, W)


def refine_path(points_or_cloud_or_model, path, quats=None, clearance_radius=None, spacing=None, keep=None, window=None, max_rows=None):
    """Turn a planned walk into a trajectory: shortcut it under the same clearance radius, so that it runs at any
    angle instead of along a roadmap's directions, and resample it at `spacing` metres with orientations turning evenly between
    the views.  path: (L,3) poses with 2 <= L <= 1024, a Tour (its poses, quats and keep = the walk rows that are tour nodes) or a
    PlannedPath (its poses); quats / keep given here take precedence.  keep (L,) bool: the rows the result must pass through (the
    first and the last always are); window: the most rows a shortcut may span (default L - 1).  Every pair of rows at most
    `window` apart with no kept row between them is put to the swept clearance query (edge_clearance); the shortest route over
    the open chords and the input legs is found on the device in integer arithmetic — lengths in units of 2^-20 m, ties to the
    lowest predecessor — so every run gives the same path.  Each leg between two corners is then cut into equal pieces no longer
    than `spacing` (None: corners only); a row's quaternion is the normalised linear blend of the two kept rows around it by arc
    length.  -> RefinedPath; ValueError when a coordinate (or a kept row's quaternion) is not finite or more than max_rows
    (default 4 096) rows are needed.  Launches only, then one copy to the host."""
    cloud, pts = _clearance_cloud(points_or_cloud_or_model, "refine_path", field=True)
    if isinstance(path, Tour):
        if keep is None:   # (without via every row of the walk is a tour node)
            n = path.D.shape[0]
            keep = torch.tensor([v < n for v in (path.walk_nodes if path.walk_nodes is not None else path.walk)], dtype=torch.bool)
        quats = path.quats if quats is None else quats
        path = path.poses
    elif isinstance(path, PlannedPath):
        path = path.poses
    L, W, h, max_rows = ops.check_path(path, quats, keep, window, spacing, max_rows)
    r = ops.check_tour_radius(clearance_radius)
    cloud = _device_cloud(cloud, pts, "refine_path", radius=r)
    dev = cloud.device
    P = path.detach().to(device=dev, dtype=torch.float32).contiguous()
    qs = quats.detach().to(device=dev, dtype=torch.float32).contiguous() if quats is not None else None
    kept = torch.zeros(L, dtype=torch.bool, device=dev) if keep is None else keep.to(dev) != 0
    kept[0] = kept[L - 1] = True
    band = _path_chord_band(cloud, P, kept, W, r)
    buf = ops.path_refine(P, qs, kept, band, W, h, max_rows)
    lay = ops.path_layout(L, max_rows)
    # the one synchronisation: the header, the corners, row_node and the input legs' answers in one copy
    h_ = torch.cat([buf[:256], buf[lay["corner"]:lay["corner"] + 4 * L], buf[lay["row_node"]:lay["row_node"] + 4 * max_rows],
                    band[:L - 1, 0].contiguous()]).cpu()
    hdr = h_[:256].view(torch.int64)
    m, R, status = int(hdr[0]), int(hdr[1]), int(hdr[4])
    if status & 1:
        raise ValueError("refine_path: path holds a coordinate that is not finite, or a kept row's quaternion is zero or not finite")
    if status & 2:
        raise ValueError(f"refine_path: the refined path needs {R} rows, max_rows = {max_rows}")
    o = 256
    corners = h_[o:o + 4 * L].view(torch.int32)[:m + 1].to(torch.int64)
    o += 4 * L
    row_node = h_[o:o + 4 * R].view(torch.int32).clone()
    o += 4 * max_rows
    leg_blocked = h_[o:o + L - 1] == 0
    poses = buf[lay["out_poses"]:lay["out_poses"] + 12 * R].view(torch.float32).view(R, 3).clone()
    out_q = buf[lay["out_quats"]:lay["out_quats"] + 16 * R].view(torch.float32).view(R, 4).clone() if qs is not None else None
    return RefinedPath(poses=poses, quats=out_q, row_node=row_node, corners=corners, length=int(hdr[2]) * ops.TOUR_UNIT,
                       length_fixed=int(hdr[2]), input_length=int(hdr[3]) * ops.TOUR_UNIT, input_length_fixed=int(hdr[3]),
                       leg_blocked=leg_blocked, n_open=int(hdr[5]), open_band=band)


class ViewProposals(_Result):
    """What propose_views returns, ranked by what is left to see.  poses (V,3) f32 and quats (V,4) f32 wxyz on the device — they feed
    select_views(..., prop.poses, prop.quats, k) as they are; score (V,) int64: the summed weights inside the proposal's window
    of sectors; position_index (V,) int64 and heading (V,) int32: the position row and the sector the view looks along; all in rank
    order: score descending, then position, then heading.  hist (M,S) int64, open (M,) bool and weights (N,) int32 or None (no
    prior: every point weighs 1) are what the ranking was computed from, on the device; sectors, hw, tan_v, min_dist, max_dist: the
    settings behind them."""
    __slots__ = ("poses", "quats", "score", "position_index", "heading", "hist", "open", "weights", "sectors", "hw", "tan_v", "min_dist",
                 "max_dist")

    @property
    def n_views(self):
        return int(self.score.shape[0])


def _propose_camera(m, prior_log_odds, given):
    """propose_views' camera and prior: a ModelTraj brings its own (the keywords must stay None), points need K, img_width, img_height
    -> (prior or None, min_dist, max_dist, K as nine host floats, img_width, img_height)."""
    names = ("min_dist", "max_dist", "K", "img_width", "img_height")
    if hasattr(m, "_cloud") and hasattr(m, "_shard"):
        extra = [k for k in names if given[k] is not None]
        if extra:
            raise ValueError(f"propose_views: {extra} belong to the call with points; a ModelTraj brings its own camera and distances")
        prior = m.prior_log_odds if prior_log_odds is None else prior_log_odds
        return prior, m.pc_clip_limits[0], m.pc_clip_limits[1], [float(v) for v in m._cam.c.K], m.img_width, m.img_height
    missing = [k for k in ("K", "img_width", "img_height") if given[k] is None]
    if missing:
        raise ValueError(f"propose_views: with points or a PackedCloud the camera is needed: {missing} missing")
    K = torch.as_tensor(given["K"], dtype=torch.float32).detach().cpu().reshape(-1).tolist()
    if len(K) != 9:
        raise ValueError(f"propose_views: K must hold 3 x 3 intrinsics, got {len(K)} values")
    return (prior_log_odds, 1.0 if given["min_dist"] is None else given["min_dist"], 5.0 if given["max_dist"] is None else given["max_dist"],
            K, given["img_width"], given["img_height"])


def propose_views(points_or_cloud_or_model, positions, n_per_position=2, sectors=32, prior_log_odds=None, clearance_radius=None,
                  max_views=None, min_score=0, min_dist=None, max_dist=None, K=None, img_width=None, img_height=None):
    """Candidate views for select_views, ranked by what is left to see: where can a level camera stand among
    `positions` (M,3) — a lattice from synth.roadmap_lattice, say — and which way should it look from there?

    A position is open when its coordinates are finite and, with clearance_radius, trajectory_clearance finds no cloud point nearer
    than it.  From every open position one pass over the cloud sorts the points whose RANGE lies in [min_dist, max_dist] and whose
    elevation lies inside the vertical field of view, tan_v = (img_height / 2) / fy, into `sectors` bearing sectors about +z, each
    point weighing rint(32768 (1 - sigmoid(prior))) — what the prior has not covered yet; without a prior every point weighs 1.
    prior_log_odds: (N,) log-odds or an ops.CoverageMap (looked up over the cloud).  A heading's score is the sum over the sectors the
    horizontal field of view spans, hw = floor(atan((img_width / 2) / fx) / (2 pi / sectors)) on either side; each position
    proposes its n_per_position <= 8 best headings with disjoint windows and a score >= max(min_score, 1).  The view at heading h
    looks along the centre of sector h: r_z((h + 1/2) 2 pi / sectors) (x) Q_OPTICAL, synth.candidate_grid's convention.

    This is a pre-filter and a heuristic by design: the gate is on range, not on camera depth, nothing is occluded, there is no
    rig and no soft mask.  select_views does the exact scoring on the few hundred views that come out.  Everything is integer
    after the f32 gates, so every run gives the same ranking: by (score descending, position, heading), cut to max_views.

    First argument: a ModelTraj (its cloud, camera, distances and prior; prior_log_odds overrides the prior), (N,3) points or an
    ops.PackedCloud (sorted or not) with K, img_width, img_height[, min_dist = 1, max_dist = 5].  -> ViewProposals."""
    m = points_or_cloud_or_model
    cloud, pts = _clearance_cloud(m, "propose_views")
    given = dict(min_dist=min_dist, max_dist=max_dist, K=K, img_width=img_width, img_height=img_height)
    prior, mn, mx, Kh, iw, ih = _propose_camera(m, prior_log_odds, given)
    iw, ih, fx, fy = (ops._float_or_nan(v) for v in (iw, ih, Kh[0], Kh[4]))
    if not all(math.isfinite(v) and v > 0.0 for v in (iw, ih, fx, fy)):
        raise ValueError(f"propose_views: img_width, img_height and the focal lengths K[0][0], K[1][1] must be finite numbers > 0, got "
                         f"{img_width!r}, {img_height!r}, {Kh[0]!r}, {Kh[4]!r}")
    if sectors not in ops.VIEW_SECTORS:
        raise ValueError(f"sectors must be one of {ops.VIEW_SECTORS}, got {sectors!r}")
    hw = int(math.floor(math.atan((iw / 2.0) / fx) / (2.0 * math.pi / sectors)))
    tan_v = (ih / 2.0) / fy
    n = cloud.n if cloud is not None else pts.shape[0]
    M, S, mn, mx, tan_v, hw, n_per, sep, min_score = ops.check_propose(n, positions, None, None, sectors, mn, mx, tan_v, hw, n_per_position,
                                                                       None, min_score)
    if max_views is not None and (isinstance(max_views, bool) or not isinstance(max_views, int) or max_views < 1):
        raise ValueError(f"max_views must be None or an integer >= 1, got {max_views!r}")
    r = ops.check_tour_radius(clearance_radius) if clearance_radius is not None else None
    if prior is not None and not isinstance(prior, ops.CoverageMap):
        ops.check_prior(prior, n)
    cloud = _device_cloud(cloud, pts, "propose_views")
    dev = cloud.device
    P = positions.detach().to(device=dev, dtype=torch.float32).contiguous()
    weights = None
    if prior is not None:
        prior = ops.check_prior(ops.resolve_prior(prior, cloud), n, dev)
        weights = torch.round(32768.0 * (1.0 - torch.sigmoid(prior))).to(torch.int32)   # f32; round = rint (half to even)
    is_open = torch.isfinite(P).all(dim=1)
    if r is not None:
        d, _ = trajectory_clearance(cloud, P, r)
        is_open &= d >= r
    hist = ops.view_histogram(cloud, P, is_open, weights, S, mn, mx, tan_v)
    heading, score = ops.view_headings(hist, hw, n_per, sep, min_score)
    # the ranking: one unique int64 key per proposal, so no tie is left to the sort — the rank of the score among the distinct
    # scores (descending), then the position, then the heading
    slot = torch.nonzero(heading.reshape(-1) >= 0).reshape(-1)
    h, s = heading.reshape(-1)[slot].to(torch.int64), score.reshape(-1)[slot]
    p = slot // n_per
    distinct, rank = torch.unique(s, sorted=True, return_inverse=True)
    key = ((distinct.numel() - 1 - rank) * ops.VIEW_MAX_POSITIONS + p) * 128 + h
    order = torch.sort(key).indices
    if max_views is not None:
        order = order[:max_views]
    h, s, p = h[order], s[order], p[order]
    from .synth import propose_tables   # (numpy only)
    qtable = torch.from_numpy(propose_tables(S)[1]).to(dev)
    return ViewProposals(poses=P[p], quats=qtable[h], score=s, position_index=p, heading=h.to(torch.int32), hist=hist, open=is_open,
                         weights=weights, sectors=S, hw=hw, tan_v=tan_v, min_dist=mn, max_dist=mx)


def particle_filter(map_or_matcher, n=4096, seed=0, beta_q=256, floor=None, unknown_value=0):
    """Where is the robot, scan after scan?  An ops.ParticleFilter ("Particle filter") on an ops.EvidenceMap — or on an
    ops.ScanMatcher, whose floor and unknown_value it takes: n pose hypotheses on the device that predict() moves by odometry,
    weigh() judges by scan matching's score, resample() renews and estimate() reads.  pf.seed_gaussian(pose, yaw, sigma_xyz,
    sigma_yaw) starts from a prior, pf.seed_positions(m.free.export()) from everywhere the map knows to be free.  beta_q: how sharply
    a score unit halves a weight, in 1/65536 (256: a weight halves per 256 score units)."""
    if isinstance(map_or_matcher, ops.SpaceMap):
        raise ValueError("particle_filter: a SpaceMap holds no log-odds: give ops.EvidenceMap.from_space(space)")
    return ops.ParticleFilter(map_or_matcher, n, seed, beta_q, floor, unknown_value)


def localise_particles(map_or_matcher, scans, deltas, pose, yaw, sigma_xyz, sigma_yaw, motion_sigma, n=4096, seed=0, beta_q=256, ratio=0.5,
                       floor=None, unknown_value=0, attitudes=None, units="metric", filter=None):
    """Track a robot over a sequence: scans, K tensors (P_k,3) in the SENSOR frame, and deltas (K,4), the odometry (dx, dy, dz, dyaw)
    in the body frame that led to each.  The filter is seeded around (pose, yaw) with (sigma_xyz, sigma_yaw) — or `filter`, an
    ops.ParticleFilter already seeded, is carried on — and runs predict(delta_k, motion_sigma) -> weigh(scan_k) -> resample(ratio)
    per scan.  attitudes: None or K (3,3) rotations, the roll and pitch at each scan.  units: of deltas and sigmas, 'metric' or
    'state'.  -> (estimates, filter): K ops.ParticleEstimate, each of the weights before that step's resample.  One read-back per
    scan (the estimate); deltas and attitudes are host numbers."""
    d = ops._host_rows(deltas, 4, "deltas")
    scans = list(scans)
    if len(scans) != d.shape[0] or (attitudes is not None and len(attitudes) != len(scans)):
        raise ValueError(f"localise_particles: as many scans, deltas and attitudes, got {len(scans)}, {d.shape[0]}"
                         f"{'' if attitudes is None else ', ' + str(len(attitudes))}")
    pf = filter
    if pf is None:
        pf = particle_filter(map_or_matcher, n, seed, beta_q, floor, unknown_value).seed_gaussian(pose, yaw, sigma_xyz, sigma_yaw, units=units)
    elif not isinstance(pf, ops.ParticleFilter):
        raise ValueError(f"localise_particles: filter must be an ops.ParticleFilter, got {type(pf).__name__}")
    estimates = []
    for k, pts in enumerate(scans):
        pf.predict(d[k], motion_sigma, units=units)
        pf.weigh(pts, None if attitudes is None else attitudes[k], ratio=ratio)
        estimates.append(pf.estimate())
        pf.resample(ratio)
    return estimates, pf
