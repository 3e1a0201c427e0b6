/*
 * trajopt_hip.h — C ABI of libtrajopt_hip.so: the MI355X (gfx950) implementation of the
 * differentiable point-cloud visibility + coverage-reward path of ctu-vras/trajectory_optimization.
 *
 * The reference has no FFI/plugin seam; its boundary is the Python object API of src/model.py and
 * src/tools.py.  Each entry point below therefore names the reference code it replaces (file:line,
 * relative to the reference checkout).  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host.  The suffix is load-bearing: the Python binding
 *     (trajectory_optimization_amd/_lib.py) is read from this file, and it types a parameter named *_host as a pointer to its
 *     pointee (or to the struct it names) and every other pointer as an opaque address — a new HOST pointer must be named *_host,
 *     and every declaration here must be one that reader knows (fixed-width scalars, int, size_t, float, double, pointers to them,
 *     the structs below);
 *   - the caller allocates every input, output and workspace buffer, and no DEVICE memory is ever allocated or freed by the
 *     library.  Nothing a call computes is kept for a later call.  The two things the library does keep, both HOST-side
 *     scratch that never changes a result:
 *       * the hull builds (tohip_convex_hull_vertices, tohip_hidden_pts_removal and its _batched form: the calls that read
 *         counters back and therefore synchronise): two
 *         pinned read-back buffers (~2 KB each) and two events per (calling thread, device), created at the first such call
 *         of the thread on that device and released when the thread ends;
 *       * tohip_profile_enable(1): a pool of timing events per process, grown on demand while profiling is on, released by
 *         tohip_profile_enable(0) after tohip_profile_read;
 *     and the process-wide switches tohip_profile_enable / tohip_profile_clock themselves.  Everything else is stateless:
 *     two threads may call any entry point concurrently on different streams with different workspaces;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); kernels are only enqueued,
 *     no entry point synchronises unless its comment says so;
 *   - return value: 0 = ok, >0 = a hipError_t from a launch, <0 = an argument error (TOHIP_E*);
 *     nothing throws, nothing calls exit();
 *   - quaternions are (w,x,y,z) like the reference's models (model.py:69,162);
 *   - float = IEEE binary32 everywhere; indices are int32; counts int64.
 */
#ifndef TRAJOPT_HIP_H
#define TRAJOPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (still 15) + tohip_mcl_seed_gaussian / tohip_mcl_seed_positions / tohip_mcl_predict / tohip_mcl_poses / tohip_mcl_weigh /
 * tohip_mcl_weights / tohip_mcl_resample_systematic and the TOHIP_MCL_* constants (a particle filter on the evidence map: pose hypotheses seeded,
 * moved, weighed by scan matching's score and resampled on the device, in integers): new symbols only.
 * (still 15) + tohip_evid_weight_plane / tohip_view_information (information gain: a view scored by a weight per voxel that depends on
 * its evidence byte, summed over the voxels it sees, and the map's remaining information): new symbols only.
 * (still 15) + tohip_travel_weights_bytes / tohip_travel_weights_build / tohip_travel_build_weighted / tohip_travel_paths_weighted (weighted
 * travel fields: a per-voxel cost factor so routes keep off walls and out of the unknown): new symbols only.
 * (still 15) + tohip_occ_coarsen / tohip_evid_coarsen and the TOHIP_COARSEN_* constants (coarsening maps: f x f x f voxels of one box reduced
 * to one voxel of a coarser box under a conservative or an optimistic rule, written or combined as the transfers do): new symbols only.
 * (still 15) + tohip_occ_resample / tohip_evid_resample and the TOHIP_RESAMPLE_* constants (resampling maps: voxel content of one box read
 * in another under a rigid transform and a change of resolution, by an integer affine map the host quantises once): new symbols only.
 * (still 15) + tohip_posegraph_workspace_bytes / tohip_posegraph_layout / tohip_posegraph_start / tohip_posegraph_linearize /
 * tohip_posegraph_gather / tohip_posegraph_step / tohip_posegraph_optimize / tohip_posegraph_result and the TOHIP_POSEGRAPH_* constants
 * (pose-graph optimisation: Levenberg-Marquardt over scan poses, each step by block-Jacobi conjugate gradients): new symbols only.
 * (still 15) + tohip_scanreg_normal / tohip_scanreg_step and TOHIP_SCANREG_RECORD / TOHIP_SCANREG_STATE (fine scan registration: integer
 * normal equations of a scan on the trilinear score table, and a damped Gauss-Newton step per pose): new symbols only.
 * (still 15) + tohip_reloc_levels / tohip_reloc_bounds / tohip_reloc_workspace_bytes / tohip_reloc_search (relocalisation: exact
 * branch-and-bound scan matching over wide windows, on sliding-maximum copies of the score table): new symbols only.
 * (still 15) + tohip_scan_prepare / tohip_scan_score / tohip_scan_correlate / tohip_scan_best (scan-to-map registration: a scan scored
 * against the evidence map at every pose of a search window, and the best of them): new symbols only.
 * (still 15) + tohip_ground_build / tohip_ground_snap (the ground layer: where a robot that drives can stand, what is an obstacle for it
 * and the slab its centre rides in, as planes the field and travel entry points take unchanged): new symbols only.
 * (still 15) + tohip_travel_batch_bytes / tohip_travel_batch_workspace_bytes / tohip_travel_build_batch / tohip_travel_positions_batch /
 * tohip_travel_paths_batch / tohip_assign_greedy and TOHIP_TRAVEL_MAX_FIELDS (many travel fields built in the same worklist rounds, their
 * lookups and paths in one launch each, and a deterministic greedy assignment of rows to columns): new symbols only.
 * (still 15) + tohip_occ_transfer / tohip_evid_transfer (re-framing and merging maps: voxel content moved from one box into another at
 * an integer voxel shift, written or combined): new symbols only.
 * (still 15) + tohip_components_bytes / tohip_components_workspace_bytes / tohip_components_build / tohip_components_stats /
 * tohip_components_min / tohip_components_positions (connected components of a bit plane: a label volume, per-component size, sums,
 * box, and the minimum of a value volume over each component): new symbols only.
 * (still 15) + tohip_travel_bytes / tohip_travel_workspace_bytes / tohip_travel_build / tohip_travel_positions / tohip_travel_paths /
 * tohip_view_volume_pick_travel (a travel field: reachable space and path cost over the clearance field, and a view pick that prices
 * the trip): new symbols only.
 * (still 15) + tohip_cast_segments / tohip_depth_scan (where a ray through the map stops: first hits of segments and the depth image a
 * sensor at a pose would return): new symbols only.
 * (still 15) + tohip_occ_unknown / tohip_view_volume / tohip_view_volume_pick (the unknown volume a view would reveal, and the greedy
 * choice of views by it): new symbols only.
 * (still 15) + tohip_clearance_map / tohip_clearance_map_segments and the flag bit TOHIP_TRAJ_CLEARANCE_PREFILLED (the clearance term
 * asked of the map: the obstacles are an occupancy grid's voxels): new symbols and one flag bit that was refused before — no struct
 * and no existing signature changes.
 * (still 15) + tohip_evid_bytes / tohip_evid_init / tohip_evid_fold / tohip_evid_positions (a hit/miss evidence map: integer log-odds
 * per voxel, the occupied and free planes derived from it): new symbols only.
 * (still 15) + tohip_field_bytes / tohip_field_workspace_bytes / tohip_field_build / tohip_field_positions / tohip_field_segments /
 * tohip_field_nodes (a conservative clearance field over the occupancy grid): new symbols only.
 * (still 15) + tohip_occ_carve / tohip_occ_state / tohip_occ_frontier / tohip_occ_export_workspace_bytes / tohip_occ_count /
 * tohip_occ_export (free-space carving, the three-state map, frontiers and the ordered listing of a grid): new symbols only.
 * (still 15) + tohip_occ_bytes / tohip_occ_init / tohip_occ_insert / tohip_occ_lookup / tohip_los_segments / tohip_los_rows (an
 * occupancy bit grid and exact line-of-sight walks: the 'voxel' occlusion rows): new symbols only.
 * (still 15) + tohip_view_histogram / tohip_view_headings (propose candidate views: per-position bearing histograms of what is left to
 * see, and the best headings of each): new symbols only.
 * (still 15) + tohip_path_bytes / tohip_path_refine (refine a planned walk: any-angle shortcuts and even waypoint spacing): new symbols
 * only.
 * (still 15) + tohip_roadmap_knn / tohip_roadmap_routes_bytes / tohip_roadmap_relax / tohip_roadmap_pred / tohip_tour_plan_via (a
 * free-space roadmap: routes where no straight leg is open): new symbols only.
 * (still 15) + tohip_clearance_edges / tohip_tour_bytes / tohip_tour_plan (a collision-checked tour through chosen views): new symbols
 * only.
 * (still 15) + tohip_clearance_segments / tohip_clearance_segments_workspace_bytes / tohip_traj_clearance_segments_scratch_bytes and
 * the flag bit TOHIP_TRAJ_CLEARANCE_SEGMENTS (the swept clearance term: the hinge on each segment's distance): new symbols and one
 * flag bit that was refused before — no struct and no existing signature changes.
 * (still 15) + tohip_covmap_bytes / tohip_covmap_init / tohip_covmap_integrate / tohip_covmap_lookup / tohip_covmap_merge /
 * tohip_covmap_rehash / tohip_covmap_export / tohip_covmap_read_header (the voxel-keyed log-odds map): new symbols only.
 * (still 15) + tohip_views_bytes / tohip_views_append / tohip_views_select / tohip_views_row (greedy view selection): new symbols only.
 * (still 15) + tohip_team_step_tail / tohip_team_loss / tohip_team_member_gains / tohip_team_state_bytes /
 * tohip_team_member_gains_bytes (team coverage): new symbols only — no struct and no existing signature changes, so a caller built
 * against the earlier header of 15 works unchanged and the number stays.
 * (still 15) + tohip_traj_prior_bytes / tohip_traj_prior_build / tohip_traj_reward_prior / tohip_traj_reward_backward_prior /
 * tohip_traj_backward_prior / tohip_traj_coverage (a per-point log-odds prior): new symbols only.
 * 15: + tohip_clearance / tohip_clearance_workspace_bytes / tohip_traj_clearance_scratch_bytes / tohip_traj_step_tail_clearance /
 * tohip_traj_regularizers_clearance (the clearance term); tohip_traj_loss and tohip_traj_opt gain clearance_radius,
 * clearance_weight, clearance_scratch(_bytes) at their ends (zero = off).
 * 14: + tohip_pose_forward_bits / _backward_bits / _forward_backward_bits / _opt_step_bits / _forward_backward_multi_bits (per-pose
 * occlusion bit rows); tohip_pose_opt gains occlusion_bits at its end.
 * 13: + tohip_pose_workspace_bytes_multi / tohip_pose_forward_backward_multi / tohip_pose_opt_step_multi (several poses of one
 * camera over one cloud per pass).
 * 12 (r05): + tohip_render_points_blend / tohip_render_blend_workspace_bytes; + TOHIP_TRAJ_OPT_LAST_OUTPUTS; tohip_voxel_grid reports
 * PCL's "leaf size too small" case as *out_count = -1.  (11: r04) */
#define TOHIP_ABI_VERSION 15

#define TOHIP_OK 0
#define TOHIP_EINVAL (-1)   /* bad size / null pointer */
#define TOHIP_ENOSPC (-2)   /* caller-provided workspace or output capacity too small */
#define TOHIP_ENOTCONV (-3) /* an iteration did not converge within its limit: the hull's rounds, a roadmap's relaxation sweeps */
#define TOHIP_ENAN (-4)     /* hull input holds a NaN (a zero-norm point flips to NaN, tools.py:49-52): scipy raises ValueError */

/* Points are processed in tiles of this many; packed clouds are padded to a multiple of it. */
#define TOHIP_POINT_TILE 2048

/* Camera model shared by all waypoints: load_intrinsics (tools.py:320-325) + the constants the
 * models keep (model.py:91-94,186-189).  Passed by pointer in HOST memory. */
typedef struct tohip_camera {
    float K[9];      /* row-major 3x3 intrinsics */
    float img_width; /* 1232. */
    float img_height;/* 1616. */
    float min_dist;  /* pc_clip_limits[0]  (1.0) */
    float max_dist;  /* pc_clip_limits[1]  (5.0) */
    float eps;       /* 1e-6 */
} tohip_camera;

/* Optional multi-camera rig (BASELINE.json config 5; the reference has no fusion code — each
 * (camera, waypoint) pair is a virtual waypoint with its own min/max normalisation, all log-odds
 * summed).  rig_quats: (C,4) unit wxyz rotating camera->body; rig_trans: (C,3) lever arms in the body
 * frame.  n_cams = 0 or NULL pointers mean "one camera at the body frame". */
typedef struct tohip_rig {
    int32_t n_cams;
    const float *rig_quats; /* device */
    const float *rig_trans; /* device */
} tohip_rig;

int tohip_abi_version(void);
const char *tohip_error_string(int code);

/* ---- cloud packing -------------------------------------------------------------------------
 * The cloud is constant over an optimisation run (model.py:80,174), so it is packed once into an opaque
 * device blob of tohip_packed_cloud_bytes(N) bytes: the points in Morton order as x[Npad] | y[Npad] |
 * z[Npad] (Npad = tohip_padded_points(N); the pad repeats the last sorted point), the permutation back to
 * the caller's order and its inverse, and one bounding sphere per 256 sorted points.  sort = 0 keeps the caller's order
 * (no spatial coherence: the exact culling then rarely fires — the layout for ModelPose, which culls nothing and then reads
 * masks and writes observations in place, 16 bytes at a time).  Needs tohip_pack_workspace_bytes(N)
 * bytes of scratch. */
int64_t tohip_padded_points(int64_t n_points);
size_t tohip_packed_cloud_bytes(int64_t n_points);
size_t tohip_pack_workspace_bytes(int64_t n_points);
int tohip_pack_cloud(const float *xyz, int64_t n_points, int sort, void *packed, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---- ModelTraj (model.py:200-242 forward, :246 visibility term, autograd backward) ----------
 * Workspace bytes needed by the calls below for n_points and n_virtual = W * max(1,n_cams) (at most 65 536 virtual waypoints).
 * THE WORKSPACE MUST BE ZERO-FILLED ONCE BEFORE ITS FIRST USE (hipMemset): tohip_traj_reward's accumulator word is expected
 * zero and left zero; every forward resets what a step accumulates into, that word included.  The forward leaves its state
 * there (waypoint records, per-waypoint extrema, the list of the pairs that contribute, the candidate slots) and the backward
 * of the same step reads it: do not touch the workspace between the two. */
size_t tohip_traj_workspace_bytes(int64_t n_points, int64_t n_virtual);

/* flags */
#define TOHIP_TRAJ_DENSE 1 /* evaluate every (point, waypoint) pair; default: skip pairs that provably
                              contribute exactly nothing (bitwise identical results, see traj_kernels.hip) */
/* bits 8..23 of flags: the waypoint selection of model.py:215-217 as a stride of the forward's reads — with
 * TOHIP_TRAJ_STRIDE(step) the n_wps evaluated waypoints are rows 0, step, 2 step, ... of poses / quats, read in place (one
 * trajectory; the backward entry points ignore the bits: gradient rows are compact, one per evaluated waypoint). */
#define TOHIP_TRAJ_STRIDE(step) ((((step) - 1) & 0xffff) << 8)
/* tohip_traj_opt.flags only: the two N-sized OUTPUTS of a step — lo_sum and rewards, per trajectory — are written by the run's
 * last step (step_index == n_steps - 1) only.  Every step still computes every reward (their sum, the loss and the gradients need
 * them); what the earlier steps skip is refilling and scattering two vectors of N floats per trajectory that the next step
 * overwrites unread — 64 MB of stores per step for eight trajectories over 1 M points
 * (/root/reference/src/trajectory_optimization.py:147-157 publishes model.rewards once, after the loop). */
#define TOHIP_TRAJ_OPT_LAST_OUTPUTS 2
/* tohip_traj_loss.flags and tohip_traj_opt.flags only: with clearance_weight > 0 the clearance term is the SWEPT one — the hinge on
 * each segment's distance to the cloud (tohip_clearance_segments) in place of each waypoint's; its launches come first, as the point
 * query's do, and clearance_scratch is then tohip_traj_clearance_segments_scratch_bytes.  Without the bit, or with weight 0, every
 * launch is the one without it. */
#define TOHIP_TRAJ_CLEARANCE_SEGMENTS 4
/* tohip_traj_loss.flags and tohip_traj_opt.flags only: with clearance_weight > 0 the caller has ALREADY written clearance_scratch's
 * gradient rows and terms for the current poses, on the same stream, and the step launches no clearance query of its own — how a
 * plan carries a term whose obstacles its struct cannot name (the map's voxels: tohip_clearance_map / _map_segments, below).  With
 * or without TOHIP_TRAJ_CLEARANCE_SEGMENTS, which then only sizes the scratch.  The scratch then holds the caller's data while the
 * step reads and writes its other buffers, so it must be a buffer of its own: a clearance_scratch that is any other device pointer of
 * the struct is TOHIP_EINVAL.  With weight 0 the bit does nothing. */
#define TOHIP_TRAJ_CLEARANCE_PREFILLED 8

/* Forward over the W evaluated waypoints (caller has applied wps_step, model.py:214-217):
 * to_camera_frame -> get_dist_mask * get_fov_mask -> per-waypoint (p-min)/max -> clip -> log-odds,
 * summed over waypoints into lo_sum[0..Npad) IN PACKED (sorted) ORDER (overwritten; this rank's partial
 * sum when the waypoints are sharded over GPUs — every rank packs the same cloud the same way).
 * minmax[v] = (min p, max(p - min p)) per virtual waypoint (for inspection; the backward reads the workspace).
 * replaces model.py:217-231. */
int tohip_traj_forward(const void *packed, int64_t n_points, const float *poses, const float *quats, int64_t n_wps,
                       const tohip_camera *cam_host, const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits,
                       float *lo_sum, float *minmax, float *rewards_half, void *workspace, size_t workspace_bytes,
                       void *stream);
/* rewards_half (may be NULL): N floats that the forward fills with sigmoid(0) = 0.5 on its way — hand the same array to
 * tohip_traj_reward with prefilled = 1 and that call only stores the rewards of the points with a non-zero log-odds (2 % of
 * the cloud on the BASELINE workloads) instead of scattering all N. */
/* occlusion_bits (may be NULL = nothing occluded): per virtual waypoint a row of Npad/32 words, bit i = 1 when the
 * packed (sorted) point i is NOT occluded from that waypoint; an occluded pair has p = 0.  The per-waypoint
 * analogue of ModelPose's occlusion mask (model.py:112-115) that the reference leaves as a TODO (tools.py:61-62).
 * Rows are built with tohip_occlusion_row(s) from a hard-frustum cull + HPR (or z-buffer) of the camera-frame cloud;
 * the bits of the pad positions [N, Npad) repeat the bit of the last sorted point. */
int tohip_inverse_permutation(const void *packed, int64_t n_points, int32_t *inv_perm, void *stream);
int tohip_occlusion_row(int64_t n_points, const int32_t *inv_perm, const int32_t *kept_idx, const int32_t *kept_count,
                        const int32_t *visible_idx_in_kept, const int32_t *visible_count, uint32_t *row, void *stream);
/* The same for n_wps waypoints in four launches.  kept_idx (n_wps, n): waypoint w's kept points in its first kept_count[w]
 * entries (the layout tohip_cull_waypoints writes); vis_idx: the visible ones as positions in that list, waypoint w's in
 * [vis_off[w], vis_off[w+1]) (n_wps+1 device int32); all_visible[w] != 0: nothing of w is occluded.  rows: (n_wps, Npad/32). */
int tohip_occlusion_rows(int64_t n_points, const int32_t *inv_perm, const int32_t *kept_idx, const int32_t *kept_count,
                         const int32_t *vis_idx, const int32_t *vis_off, const int32_t *all_visible, int64_t n_wps,
                         uint32_t *rows, void *stream);

/* The same from per-point visibility VALUES instead of index lists: waypoint w's kept point j is hidden when
 * visible[seg_off[w] + j] == 0 (seg_off: n_wps device int64) — the mask tohip_hidden_pts_removal_batched writes over the waypoints'
 * kept points laid end to end, or tohip_zbuffer_visible_batched's (seg_off[w] = w * n).  A waypoint with fewer than min_points kept
 * points keeps its row of ones (a hull needs 4).  Three launches for all waypoints.  inv_perm may be NULL: kept_idx then holds
 * positions in the packed cloud's order already (the cull ran over the sorted points) in ascending order, and the hidden bits of a
 * word are combined on their way (one atomic per run of neighbours instead of one per hidden point). */
int tohip_occlusion_rows_masked(int64_t n_points, const int32_t *inv_perm, const int32_t *kept_idx, const int32_t *kept_count,
                                const float *visible, const int64_t *seg_off, int32_t min_points, int64_t n_wps, uint32_t *rows,
                                void *stream);

/* rewards[0..N) = sigmoid(lo_sum) in the CALLER'S point order (model.py:237); scalars[0] = mean(rewards),
 * scalars[1] = loss_vis = 1/(mean+eps) (model.py:246), scalars[2] = -loss_vis^2/N (d loss_vis / d reward_n).
 * One launch.  prefilled != 0: the caller promises rewards[0..N) == 0.5 on entry (tohip_traj_forward's rewards_half).
 * workspace: a zero-filled-once region of at least 256 bytes — normally the forward's workspace (none of the forward's
 * state is touched). */
int tohip_traj_reward(const void *packed, const float *lo_sum, int64_t n_points, float eps, int prefilled, float *rewards,
                      float *scalars, void *workspace, size_t workspace_bytes, void *stream);

/* Backward w.r.t. this rank's waypoints: poses_grad (W,3), quats_grad (W,4), for the step whose tohip_traj_forward last
 * used `workspace` (same n_points, n_wps, rig, flags, occlusion_bits).
 * lo_sum = the (all-reduced) log-odds vector in packed order that tohip_traj_reward turned into rewards.
 * The upstream gradient is either grad_rewards (N floats in the caller's order, dL/d rewards: any
 * criterion built on model.rewards, as torch autograd would hand it over), or, when grad_rewards is NULL,
 * the fused visibility loss: scalars (from tohip_traj_reward) and gout = device pointer to dL/d loss_vis.
 * Deterministic: no float atomics anywhere, tie sets of the per-waypoint min()/max() included. */
int tohip_traj_backward(const void *packed, int64_t n_points, int64_t n_wps, const tohip_camera *cam_host,
                        const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits, const float *lo_sum,
                        const float *grad_rewards, const float *scalars, const float *gout, float *poses_grad,
                        float *quats_grad, void *workspace, size_t workspace_bytes, void *stream);

/* ---- several trajectories over one cloud in one pass ("many trajectories optimised concurrently") ----------
 * n_traj trajectories' waypoints laid end to end (poses (W,3), quats (W,4), W = their total); traj_offsets: n_traj + 1 ascending
 * body-waypoint offsets on the DEVICE (int32; [0] = 0, [n_traj] = W; may be NULL when n_traj == 1).  Every trajectory has its
 * own log-odds vector (lo_sum: n_traj x Npad), rewards (n_traj x N), scalars (n_traj x 4) and upstream gradient (gout: n_traj
 * floats; grad_rewards: n_traj x N); the per-waypoint outputs (minmax, gradients) are simply concatenated.  Each trajectory's
 * results are, bit for bit, those of a call with that trajectory alone.  The single-trajectory entry points above are these
 * with n_traj = 1. */
size_t tohip_traj_workspace_bytes_multi(int64_t n_points, int64_t n_virtual, int64_t n_traj);
int tohip_traj_forward_multi(const void *packed, int64_t n_points, const float *poses, const float *quats, int64_t n_wps,
                             const int32_t *traj_offsets, int64_t n_traj, const tohip_camera *cam_host, const tohip_rig *rig_host,
                             int flags, const uint32_t *occlusion_bits, float *lo_sum, float *minmax, float *rewards_half,
                             void *workspace, size_t workspace_bytes, void *stream);
int tohip_traj_reward_multi(const void *packed, const float *lo_sum, int64_t n_points, int64_t n_traj, float eps, int prefilled,
                            float *rewards, float *scalars, void *workspace, size_t workspace_bytes, void *stream);
int tohip_traj_backward_multi(const void *packed, int64_t n_points, int64_t n_wps, int64_t n_traj, const tohip_camera *cam_host,
                              const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits, const float *lo_sum,
                              const float *grad_rewards, const float *scalars, const float *gout, float *poses_grad,
                              float *quats_grad, void *workspace, size_t workspace_bytes, void *stream);

/* tohip_traj_reward + tohip_traj_backward of the fused visibility loss (model.py:237,246 and loss.backward() through them) in two
 * launches instead of three: the rewards / mean / loss scalars and the gradient sums both need only the complete log-odds vector,
 * so they share a launch (the sums are taken with unit dL/d reward and scaled by scalars[2] * gout afterwards: they are linear in
 * it).  Arguments as in the two separate calls; `scalars` and `rewards` are outputs.  rewards and scalars are bitwise those of
 * tohip_traj_reward; the gradients agree with tohip_traj_backward's to rounding (the scale factor is applied once per waypoint
 * in f64 instead of once per point in f32). */
int tohip_traj_reward_backward(const void *packed, int64_t n_points, int64_t n_wps, const tohip_camera *cam_host,
                               const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits, const float *lo_sum, float eps,
                               int prefilled, float *rewards, float *scalars, const float *gout, float *poses_grad,
                               float *quats_grad, void *workspace, size_t workspace_bytes, void *stream);
int tohip_traj_reward_backward_multi(const void *packed, int64_t n_points, int64_t n_wps, int64_t n_traj,
                                     const tohip_camera *cam_host, const tohip_rig *rig_host, int flags,
                                     const uint32_t *occlusion_bits, const float *lo_sum, float eps, int prefilled, float *rewards,
                                     float *scalars, const float *gout, float *poses_grad, float *quats_grad, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* ---- a per-point log-odds prior (prior_kernels.hip) -------------------------------------------------------------------------
 * What is already known of the map, as OctoMap accumulates it: rewards become r_i = sigmoid(lo_sum_i + prior_i), lo_sum the
 * forward's sum over the evaluated waypoints as before (the forward does not change), the prior added last in one f32 add.  A zero
 * prior gives the bits of the calls without one.  prior >= 0 and finite (the integer reward sum is exact for r in [1/2, 1) only).
 * tohip_traj_prior_build turns an (N,) f32 prior in the CALLER'S order into prior_buf (tohip_traj_prior_bytes(N) device bytes): the
 * prior and sigmoid(prior) in packed order and the fixed-point sums the reward kernel starts from.  *status (device int32) is 0, or
 * has bit 0 set for a negative (or NaN) entry and bit 1 for a non-finite one; prior_buf is then not to be used.  Two launches.
 * The _prior variants take the argument lists of tohip_traj_reward, tohip_traj_reward_backward and tohip_traj_backward plus
 * prior_buf (built for the same cloud and N); prior_buf = NULL is the call without a prior.  With a prior: one trajectory, and
 * prefilled must be 0 (every reward is stored).
 * tohip_traj_coverage: out[0..N) (caller's order) = prior + lo_sum (lo_sum in packed order, as the forward writes it; prior_buf may
 * be NULL: lo_sum alone), values above clamp_max set to clamp_max (OctoMap's upper clamping threshold; +inf: none; >= 0) — the fused
 * log-odds map that is the next plan's prior.  One launch. */
size_t tohip_traj_prior_bytes(int64_t n_points);
int tohip_traj_prior_build(const void *packed, int64_t n_points, const float *prior, void *prior_buf, size_t prior_buf_bytes,
                           int32_t *status, void *stream);
int tohip_traj_reward_prior(const void *packed, const float *lo_sum, int64_t n_points, float eps, int prefilled, float *rewards,
                            float *scalars, void *workspace, size_t workspace_bytes, const void *prior_buf, void *stream);
int tohip_traj_reward_backward_prior(const void *packed, int64_t n_points, int64_t n_wps, const tohip_camera *cam_host,
                                     const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits, const float *lo_sum,
                                     float eps, int prefilled, float *rewards, float *scalars, const float *gout, float *poses_grad,
                                     float *quats_grad, void *workspace, size_t workspace_bytes, const void *prior_buf, void *stream);
int tohip_traj_backward_prior(const void *packed, int64_t n_points, int64_t n_wps, const tohip_camera *cam_host,
                              const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits, const float *lo_sum,
                              const float *grad_rewards, const float *scalars, const float *gout, float *poses_grad, float *quats_grad,
                              void *workspace, size_t workspace_bytes, const void *prior_buf, void *stream);
int tohip_traj_coverage(const void *packed, int64_t n_points, const float *lo_sum, const void *prior_buf, float clamp_max, float *out,
                        void *stream);

/* The whole step when NO collective sits between forward and backward (one GPU, or every rank holding all waypoints):
 * tohip_traj_forward + tohip_traj_reward + tohip_traj_backward of the fused visibility loss in FIVE launches — records + probe,
 * pass 1, the sparse kernel (flags, log-odds, rewards, their sum; a block per candidate slot), the gradient sums of the flagged
 * (slot, waypoint) pairs (a wave per pair, dealt evenly to the whole chip), the per-waypoint finish.
 * Outputs as in the separate calls (lo_sum, minmax, rewards, scalars, poses_grad, quats_grad); gout = device pointer(s) to
 * dL/d loss_vis.  rewards, scalars and lo_sum are bitwise those of the separate calls; the gradients agree to rounding (the
 * dL/d reward factor is applied once per waypoint in f64 instead of once per point in f32).  replaces model.py:217-231,:237,:246
 * and loss.backward() through them. */
int tohip_traj_forward_backward(const void *packed, int64_t n_points, const float *poses, const float *quats, int64_t n_wps,
                                const tohip_camera *cam_host, const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits,
                                float *lo_sum, float *minmax, float *rewards, float *scalars, const float *gout,
                                float *poses_grad, float *quats_grad, void *workspace, size_t workspace_bytes, void *stream);
int tohip_traj_forward_backward_multi(const void *packed, int64_t n_points, const float *poses, const float *quats, int64_t n_wps,
                                      const int32_t *traj_offsets, int64_t n_traj, const tohip_camera *cam_host,
                                      const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits, float *lo_sum,
                                      float *minmax, float *rewards, float *scalars, const float *gout, float *poses_grad,
                                      float *quats_grad, void *workspace, size_t workspace_bytes, void *stream);

/* ---- a POINT-sharded step (the alternative to sharding waypoints) ------------------------------------------------
 * Every rank packs N / R of the points and evaluates ALL W waypoints on them.  What the ranks exchange does not grow with N:
 *   tohip_traj_pshard_pass1   records, probe and pass 1 on this rank's points: per-waypoint extrema of ITS points in the workspace
 *   (collective 1)            element-wise MAX over the int32 words tohip_traj_extrema_view points at (4 per virtual waypoint:
 *                             -bits(min p), bits(max p), 0, 0 — p >= 0, so the integer order is the float order), IN PLACE
 *   tohip_traj_pshard_local   flags against the (now global) extrema, log-odds, rewards of this rank's points (complete: the rank
 *                             has every waypoint), the gradient sums of its flagged pairs with unit upstream gradient, and per
 *                             waypoint the 40 sums everything after is linear in -> partial[tohip_traj_pshard_partial_count(V)]
 *   (collective 2)            SUM over `partial` (doubles; [0] the reward sum in fixed point, [1] NaN marks, [2] point counts)
 *   tohip_traj_pshard_finish  mean reward of ALL points, loss_vis, dL/d reward, tie shares, chain -> scalars, poses_grad, quats_grad
 *                             (identical on every rank)
 * n_global = the points of all ranks (the fixed-point scale of the reward sum and the mean's denominator).  lo_sum (Npad_local),
 * minmax (V,2), rewards (n_local, this rank's points in the caller's order): as in tohip_traj_forward_backward.  One trajectory. */
size_t tohip_traj_pshard_partial_count(int64_t n_virtual);
int tohip_traj_extrema_view(int64_t n_points, int64_t n_virtual, void *workspace, size_t workspace_bytes, int32_t **words_out_host,
                            int64_t *n_words_out_host);
int tohip_traj_pshard_pass1(const void *packed, int64_t n_local, int64_t n_global, const float *poses, const float *quats,
                            int64_t n_wps, const tohip_camera *cam_host, const tohip_rig *rig_host, int flags,
                            const uint32_t *occlusion_bits, float *lo_sum, float *rewards, void *workspace, size_t workspace_bytes,
                            void *stream);
int tohip_traj_pshard_local(const void *packed, int64_t n_local, int64_t n_global, int64_t n_wps, const tohip_camera *cam_host,
                            const tohip_rig *rig_host, int flags, const uint32_t *occlusion_bits, float *lo_sum, float *minmax,
                            float *rewards, double *partial, void *workspace, size_t workspace_bytes, void *stream);
int tohip_traj_pshard_finish(int64_t n_local, int64_t n_global, int64_t n_wps, const tohip_camera *cam_host,
                             const tohip_rig *rig_host, const double *partial, const float *gout, float *scalars,
                             float *poses_grad, float *quats_grad, void *workspace, size_t workspace_bytes, void *stream);

/* ---- a waypoint-sharded step's all-reduce, compacted (the one data-path collective) ------------------------------
 * A rank's partial log-odds vector is exactly zero outside the 256-point slots its forward listed as candidates (6-8 % of the
 * slots on the BASELINE workloads).  Instead of all-reducing N floats: (1) tohip_traj_candidate_flags -> one 0/1 int32 per slot
 * of this rank's last forward (Npad/256 of them, device); the ranks MAX-reduce them (RCCL has no OR); (2) tohip_slot_flags_prefix
 * -> prefix[s] = set flags below slot s, prefix[nslots] = their number = the union's slots (nslots + 1 int32, device); (3)
 * tohip_slots_pack(pack = 1) gathers the union's slots of lo_sum into `compact` (256 floats each, in slot order; at most
 * capacity_slots of them); the ranks sum-reduce compact[0 .. 256 * count); (4) tohip_slots_pack(pack = 0) scatters it back.  The
 * slots outside the union are zero on every rank and are not touched. */
int tohip_traj_candidate_flags(int64_t n_points, int64_t n_virtual, int64_t n_traj, const void *workspace, size_t workspace_bytes,
                               int32_t *slot_flags, void *stream);
int tohip_slot_flags_prefix(const int32_t *slot_flags, int64_t n_points, int32_t *prefix, void *stream);
int tohip_slots_pack(const int32_t *slot_flags, const int32_t *prefix, int64_t n_points, float *lo_sum, float *compact,
                     int64_t capacity_slots, int pack, void *stream);

/* ---- ModelTraj.forward() / loss.backward() as one call each ------------------------------------------
 * The reference's loop (trajectory_optimization.py:109-116) is `optimizer.zero_grad(); loss = model(); loss.backward();
 * optimizer.step()`; one step's kernels take 0.05-0.15 ms on an MI355X, so the loop is bound by the host work between them.
 * tohip_traj_loss describes a model once (HOST struct, caller-owned like everything it points to; the library keeps no state):
 * model() is then tohip_traj_loss_forward — waypoint selection (model.py:214-217), visibility + log-odds (:217-231), rewards
 * (:237), criterion (:244-260) — and loss.backward() is tohip_traj_loss_backward.  One trajectory, no occlusion rows, no
 * sharding (those go through the separate calls above). */
typedef struct tohip_traj_loss {
    const void *packed;      /* tohip_pack_cloud's blob */
    int64_t n_points;
    int64_t n_wps;           /* W: ALL waypoints (criterion uses every one, model.py:249-258) */
    int32_t wps_step;        /* every wps_step-th waypoint is evaluated for visibility (model.py:215-217) */
    int32_t flags;           /* TOHIP_TRAJ_* */
    tohip_camera cam;
    tohip_rig rig;           /* n_cams = 0: one camera at the body frame */
    const float *poses0;     /* (W,3) initial positions (model.py:176) */
    float smoothness_weight; /* model.py:166 */
    float traj_length_weight;
    void *workspace;         /* tohip_traj_workspace_bytes(n_points, n_eval * max(1, n_cams)), n_eval = ceil(W / wps_step); zero-filled once */
    size_t workspace_bytes;
    void *scratch;           /* tohip_traj_loss_scratch_bytes(...) bytes: the step's intermediate vectors (layout below) */
    size_t scratch_bytes;
    float *reg_terms;        /* NULL, or (3, W, 3) floats: the gradients of l2, length and smooth separately (callers that
                                differentiate a single entry of model.loss) */
    /* ABI 15, appended after every earlier field: the clearance term (tohip_clearance); clearance_weight = 0: off (model() is then
       exactly the four-term criterion).  On: model() launches the query first (five launches), loss_terms[5] = clearance and total
       includes it; loss.backward() adds gout x its gradient rows to the regularisers' before the visibility rows:
       vis + gout (regularisers + clearance) */
    float clearance_radius;
    float clearance_weight;
    void *clearance_scratch;  /* tohip_traj_clearance_scratch_bytes(W, 1): its gradient rows (W,3) f32 at offset 0, then the terms
                                 (TOHIP_TRAJ_CLEARANCE_SEGMENTS: tohip_traj_clearance_segments_scratch_bytes(W, 1), the same offsets) */
    size_t clearance_scratch_bytes;
} tohip_traj_loss;
size_t tohip_traj_loss_scratch_bytes(int64_t n_points, int64_t n_wps, int32_t wps_step, int32_t n_cams);
/* byte offsets into `scratch` of: [0] poses_e (n_eval,3)  [1] quats_e (n_eval,4)  [2] lo_sum (Npad, packed order)
 * [3] minmax (V,2)  [4] scalars (4: mean reward, loss_vis, d loss_vis / d reward, -)  [5] poses_grad_eval (n_eval,3)
 * [6] quats_grad_eval (n_eval,4)  [7] regularisers' gradient (W,3) — for callers that want to look at them. */
int tohip_traj_loss_scratch_layout(int64_t n_points, int64_t n_wps, int32_t wps_step, int32_t n_cams, int64_t *offsets_host);
/* model(): rewards (N floats, caller's point order), loss_terms[0..4] = vis, l2, length, smooth, total (8 floats).  Leaves the
 * step's state in workspace + scratch for tohip_traj_loss_backward (and for tohip_traj_backward with a general dL/d rewards:
 * the workspace is in the state tohip_traj_forward leaves, lo_sum / scalars are in scratch; see tohip_traj_loss_refresh).
 * Four launches; loss.backward() is one. */
int tohip_traj_loss_forward(const tohip_traj_loss *plan_host, const float *poses, const float *quats, float *rewards,
                            float *loss_terms, void *stream);
/* loss.backward(): gout = DEVICE pointer to dL/d loss (autograd's incoming gradient); poses_grad (W,3), quats_grad (W,4) =
 * gout * d loss / d (poses, quats) of the step whose forward last used the plan's workspace and scratch. */
int tohip_traj_loss_backward(const tohip_traj_loss *plan_host, const float *gout, float *poses_grad, float *quats_grad,
                             void *stream);
/* tohip_traj_backward over the plan's workspace (a general dL/d rewards between model() and loss.backward()) OVERWRITES the pair
 * sums tohip_traj_loss_backward reads: they are then scaled by that call's upstream gradient.  Call this before the next
 * tohip_traj_loss_backward of the same step: it takes the unit-gradient sums again (one launch; same pairs, same bits). */
int tohip_traj_loss_refresh(const tohip_traj_loss *plan_host, void *stream);

/* ---- one step of TrajOpt.run (trajectory_optimization.py:100-127) as one call ----------------------------------
 * `optimizer.zero_grad(); loss = model(); loss.backward(); optimizer.step()` and the early-stop bookkeeping (:119-124) for
 * n_traj equal-length trajectories over one cloud, in the FIVE launches of tohip_traj_forward_backward: the waypoint selection
 * (model.py:215-217) is a stride of the first launch's reads, criterion's regularisers (model.py:244-260) with their gradient and
 * the step's Adam constants are extra blocks of the first launch, and every block of the last launch (one per evaluated waypoint)
 * updates its waypoint's rows of poses / quats (torch.optim.Adam, two groups: trajectory_optimization.py:91-94) and, for a
 * trajectory's first waypoint, writes the loss log and the early-stop state.  One camera or a rig; no occlusion rows, no sharding
 * (those use the separate calls + tohip_traj_step_tail).  HOST struct, caller-owned like everything it points to. */
typedef struct tohip_traj_opt {
    const void *packed;        /* tohip_pack_cloud's blob */
    int64_t n_points;
    int64_t n_wps;             /* W: waypoints of ONE trajectory */
    int32_t wps_step;          /* every wps_step-th waypoint is evaluated for visibility */
    int32_t flags;             /* TOHIP_TRAJ_DENSE, TOHIP_TRAJ_OPT_LAST_OUTPUTS, TOHIP_TRAJ_CLEARANCE_SEGMENTS, TOHIP_TRAJ_CLEARANCE_PREFILLED or 0 */
    int32_t n_traj;            /* trajectories laid end to end: rows b * W .. b * W + W - 1 of every per-waypoint array */
    int32_t n_steps;           /* rows of the logs below */
    const int32_t *traj_offsets; /* n_traj + 1 device int32: b * ceil(W / wps_step) (NULL when n_traj == 1) */
    tohip_camera cam;
    tohip_rig rig;             /* n_cams = 0: one camera at the body frame */
    float *poses, *quats;      /* (n_traj W, 3), (n_traj W, 4): the parameters, updated in place */
    const float *poses0;       /* (n_traj W, 3) */
    float smoothness_weight, traj_length_weight;
    float lr_pose, lr_quat, beta1, beta2, adam_eps;   /* torch.optim.Adam: two groups, shared betas / eps */
    float rewards_th, smoothness_th;                  /* trajectory_optimization.py:100 */
    float *exp_avg_p, *exp_avg_sq_p, *exp_avg_q, *exp_avg_sq_q;   /* Adam moments, zero before the first step */
    float *poses_grad, *quats_grad;   /* outputs (n_traj W, 3 / 4): the step's full gradients (what .grad would hold) */
    float *poses_grad_eval, *quats_grad_eval; /* outputs, may be NULL: (n_traj n_eval, 3 / 4) visibility gradient rows */
    float *lo_sum;             /* n_traj x Npad (packed order); with TOHIP_TRAJ_OPT_LAST_OUTPUTS valid after the last step only */
    float *minmax;             /* (V, 2), V = n_traj * n_eval * max(1, n_cams) */
    float *rewards;            /* n_traj x N, caller's point order; with TOHIP_TRAJ_OPT_LAST_OUTPUTS valid after the last step only */
    float *scalars;            /* n_traj x 4: mean reward, loss_vis, d loss_vis / d reward, - */
    float *loss_log;           /* n_traj x n_steps x 8: row s of a trajectory = (vis, l2, length, smooth, total) of its s-th step */
    float *state_log;          /* n_traj x (n_steps + 1) x 8, row 0 ZERO before the first step: row i = the early-stop state before
                                  step i ([0] reward0 [1] smooth0 [2] stopped [3] steps taken [4] visibility gain [5] smoothness
                                  gain); step i reads row i and writes row i + 1; row n_steps is the run's result */
    void *workspace;           /* tohip_traj_workspace_bytes_multi(n_points, V, n_traj); zero-filled once */
    size_t workspace_bytes;
    void *scratch;             /* tohip_traj_opt_scratch_bytes(n_wps, n_traj) */
    size_t scratch_bytes;
    /* ABI 15, appended after every earlier field: the clearance term (tohip_clearance) of every trajectory; clearance_weight = 0:
       off — the step's launches, grids and outputs are then exactly those without these fields.  On: a SIXTH launch, first, queries
       every waypoint (n_traj W waves); the sparse launch's prologue blocks sum the terms, the finish epilogue's full gradient is
       vis + (regularisers + clearance) and the loss log row gets [5] = clearance (total includes it) */
    float clearance_radius;
    float clearance_weight;
    void *clearance_scratch;   /* tohip_traj_clearance_scratch_bytes(n_wps, n_traj) (TOHIP_TRAJ_CLEARANCE_SEGMENTS:
                                  tohip_traj_clearance_segments_scratch_bytes(n_wps, n_traj); two launches first instead of one) */
    size_t clearance_scratch_bytes;
} tohip_traj_opt;
size_t tohip_traj_opt_scratch_bytes(int64_t n_wps, int64_t n_traj);
/* step_index = 0, 1, ... n_steps - 1, in order.  A trajectory that has stopped (state[2]) stays put; its rewards are still
 * refreshed.  Nothing synchronises. */
int tohip_traj_opt_step(const tohip_traj_opt *opt_host, int32_t step_index, void *stream);

/* ---- ModelPose (model.py:98-127) -------------------------------------------------------------- */
size_t tohip_pose_workspace_bytes(int64_t n_points);

/* observations, occlusion_mask and grad_obs are in the caller's point order.
 * observations[n] = dist_mask*fov_mask (* occlusion_mask[n] when non-NULL, model.py:112-115);
 * scalars[0] = sum(observations), scalars[1] = loss = 1/(sum+eps). */
int tohip_pose_forward(const void *packed, int64_t n_points, const float *trans, const float *quat,
                       const tohip_camera *cam_host, const float *occlusion_mask, float *observations, float *scalars,
                       void *workspace, size_t workspace_bytes, void *stream);
/* Upstream gradient: grad_obs (N floats, dL/d observations) or, when NULL, the fused loss through
 * scalars (from tohip_pose_forward) and gout (device pointer to dL/d loss). */
int tohip_pose_backward(const void *packed, int64_t n_points, const float *trans, const float *quat,
                        const tohip_camera *cam_host, const float *occlusion_mask, const float *grad_obs,
                        const float *scalars, const float *gout, float *trans_grad, float *quat_grad, void *workspace,
                        size_t workspace_bytes, void *stream);

/* tohip_pose_forward + tohip_pose_backward of the fused loss in ONE pass over the cloud (the gradient sums do not depend on the
 * loss: the pass that writes the observations takes them with unit weights, and the finish scales them by -loss^2 gout once the
 * sum is known): observations, scalars, and trans_grad (3) / quat_grad (4) = gout x d loss / d (trans, raw quat); gout = device
 * pointer to dL/d loss, NULL = 1.  Two launches (the pass, its one-block finish).  replaces model.py:98-127 + loss.backward(). */
int tohip_pose_forward_backward(const void *packed, int64_t n_points, const float *trans, const float *quat,
                                const tohip_camera *cam_host, const float *occlusion_mask, float *observations, float *scalars,
                                const float *gout, float *trans_grad, float *quat_grad, void *workspace, size_t workspace_bytes,
                                void *stream);
/* One step of PoseOpt's loop (pose_optimization.py:124-141): the call above, then torch.optim.Adam (two groups: trans @ lr_pose,
 * quat @ lr_quat, pose_optimization.py:93-97) on trans / quat IN PLACE, in the finish launch — still two launches.  step = the
 * 1-based iteration; loss_log[step - 1] = the loss of this step (before the update); trans_grad / quat_grad may be NULL. */
int tohip_pose_opt_step(const void *packed, int64_t n_points, float *trans, float *quat, const tohip_camera *cam_host,
                        const float *occlusion_mask, float *observations, float *scalars, float *trans_grad, float *quat_grad,
                        float *exp_avg_t, float *exp_avg_sq_t, float *exp_avg_q, float *exp_avg_sq_q, float lr_pose, float lr_quat,
                        float beta1, float beta2, float adam_eps, int32_t step, float *loss_log, void *workspace,
                        size_t workspace_bytes, void *stream);

/* The same four calls with an occlusion BIT ROW in place of the float mask: occlusion_bits (non-NULL, Npad/32 words) holds bit i = 1
 * when the packed point i is NOT occluded from this pose — the layout of tohip_traj_forward's rows (a ModelPose cloud is packed with
 * sort = 0, so packed order is the caller's order).  Each bit becomes the weight 1.0f or 0.0f and the arithmetic after it is the float
 * mask's: the results are bitwise those of the float calls given the row unpacked to zeros and ones in the caller's order.  Pads
 * carry no weight whatever their bits.  4 B per point less to read than a float mask. */
int tohip_pose_forward_bits(const void *packed, int64_t n_points, const float *trans, const float *quat, const tohip_camera *cam_host,
                            const uint32_t *occlusion_bits, float *observations, float *scalars, void *workspace, size_t workspace_bytes,
                            void *stream);
int tohip_pose_backward_bits(const void *packed, int64_t n_points, const float *trans, const float *quat, const tohip_camera *cam_host,
                             const uint32_t *occlusion_bits, const float *grad_obs, const float *scalars, const float *gout,
                             float *trans_grad, float *quat_grad, void *workspace, size_t workspace_bytes, void *stream);
int tohip_pose_forward_backward_bits(const void *packed, int64_t n_points, const float *trans, const float *quat,
                                     const tohip_camera *cam_host, const uint32_t *occlusion_bits, float *observations, float *scalars,
                                     const float *gout, float *trans_grad, float *quat_grad, void *workspace, size_t workspace_bytes,
                                     void *stream);
int tohip_pose_opt_step_bits(const void *packed, int64_t n_points, float *trans, float *quat, const tohip_camera *cam_host,
                             const uint32_t *occlusion_bits, float *observations, float *scalars, float *trans_grad, float *quat_grad,
                             float *exp_avg_t, float *exp_avg_sq_t, float *exp_avg_q, float *exp_avg_sq_q, float lr_pose, float lr_quat,
                             float beta1, float beta2, float adam_eps, int32_t step, float *loss_log, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ---- several poses of one camera over one cloud (many starts, candidate views) ------------------
 * B = n_poses poses in rows of trans (B,3) / quat (B,4); every pass over the cloud evaluates a tile of them on the points it holds
 * in registers.  Each pose's sums are taken in the order of the single-pose pass on the same grid: scalars, gradients,
 * observations and Adam updates are bit for bit those of B single-pose calls.  occlusion_mask (N, caller's order, may be NULL)
 * multiplies every pose's observations. */
size_t tohip_pose_workspace_bytes_multi(int64_t n_points, int64_t n_poses);
/* observations (B,N) in the caller's point order, or NULL: nothing is written.  scalars (B,4) as tohip_pose_forward's per pose.
 * trans_grad (B,3) / quat_grad (B,4) = gout[b] x d loss_b / d (trans_b, raw quat_b); gout = device pointer to B floats, NULL = 1.
 * Both gradient pointers NULL: the forward-only pass (scoring candidate views); one of them NULL alone is an error.
 * Two launches. */
int tohip_pose_forward_backward_multi(const void *packed, int64_t n_points, const float *trans, const float *quat, int64_t n_poses,
                                      const tohip_camera *cam_host, const float *occlusion_mask, float *observations, float *scalars,
                                      const float *gout, float *trans_grad, float *quat_grad, void *workspace,
                                      size_t workspace_bytes, void *stream);
/* The same with one occlusion bit row PER POSE: occlusion_bits (B, Npad/32), row b for pose b (layout of tohip_pose_forward_bits);
 * pose b's results are bitwise those of tohip_pose_forward_backward_bits with row b — and of the float call given row b unpacked. */
int tohip_pose_forward_backward_multi_bits(const void *packed, int64_t n_points, const float *trans, const float *quat, int64_t n_poses,
                                           const tohip_camera *cam_host, const uint32_t *occlusion_bits, float *observations,
                                           float *scalars, const float *gout, float *trans_grad, float *quat_grad, void *workspace,
                                           size_t workspace_bytes, void *stream);
/* One step of B independent PoseOpt loops (tohip_pose_opt_step per pose): Adam with two groups per pose (trans @ lr_pose,
 * quat @ lr_quat), shared betas / eps, its own moments per pose.  Filled once, passed by pointer in HOST memory. */
typedef struct tohip_pose_opt {
    const void *packed;        /* tohip_pack_cloud blob */
    int64_t n_points;
    int32_t n_poses;           /* B */
    int32_t n_steps;           /* rows of loss_log per pose */
    tohip_camera cam;
    const float *occlusion_mask;   /* N, caller's order, may be NULL: shared by every pose */
    float *trans, *quat;       /* (B,3), (B,4): the parameters, updated in place */
    float lr_pose, lr_quat, beta1, beta2, adam_eps;
    float *exp_avg_t, *exp_avg_sq_t;   /* (B,3) */
    float *exp_avg_q, *exp_avg_sq_q;   /* (B,4) */
    float *scalars;            /* (B,4): the step's sum and loss per pose */
    float *trans_grad, *quat_grad;     /* (B,3), (B,4), may be NULL: the step's gradients */
    float *loss_log;           /* (B, n_steps): loss_log[b n_steps + step - 1] = pose b's loss of this step (before the update) */
    void *workspace;           /* tohip_pose_workspace_bytes_multi(n_points, n_poses) */
    size_t workspace_bytes;
    const uint32_t *occlusion_bits;   /* ABI 14, appended after every earlier field.  (B, Npad/32) or NULL: each pose's own occlusion
                                         bit row (tohip_pose_forward_backward_multi_bits); giving occlusion_mask too is an error
                                         (TOHIP_EINVAL).  A refresh may replace the pointer between steps. */
} tohip_pose_opt;
/* step = 1, 2, ... n_steps, in order.  observations (B,N) or NULL: pass it on the step that should leave them (the last).
 * Two launches; nothing synchronises. */
int tohip_pose_opt_step_multi(const tohip_pose_opt *opt_host, int32_t step, float *observations, void *stream);

/* ---- element-wise helpers of model.py (forward values) ---------------------------------------- */
/* to_camera_frame (model.py:50-57; normalize=1) / ego_to_cam_torch (pc_processor.py:63-70;
 * normalize=0): bit-identical to the reference's f32 op order.  out_layout 0: (N,3), 1: (3,N). */
int tohip_to_camera_frame(const float *xyz, int64_t n_points, const float *quat, const float *trans, int normalize,
                          int out_layout, float *out, void *stream);
/* get_dist_mask (model.py:13-24) and soft get_fov_mask (model.py:27-47) on (N,3) camera-frame points. */
int tohip_soft_masks(const float *cam_xyz, int64_t n_points, const tohip_camera *cam_host, float *dist_mask,
                     float *fov_mask, void *stream);
/* Their backward passes (the reference's helpers are plain torch ops, differentiable by autograd):
 * grad_xyz (N,3) = grad_dist[n] dD/dp + grad_fov[n] dF/dp (either upstream gradient may be NULL = zero);
 * to_camera_frame: grad_xyz (N,3, may be NULL) = R grad_out, grad_quat (4) w.r.t. the raw quaternion (through F.normalize),
 * grad_trans (3); workspace of tohip_pose_workspace_bytes bytes. */
int tohip_soft_masks_backward(const float *cam_xyz, int64_t n_points, const tohip_camera *cam_host, const float *grad_dist,
                              const float *grad_fov, float *grad_xyz, void *stream);
int tohip_to_camera_frame_backward(const float *xyz, int64_t n_points, const float *quat, const float *trans,
                                   const float *grad_out, float *grad_xyz, float *grad_quat, float *grad_trans,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* ---- hard frustum cull (tools.py:176-187, pc_processor.py:72-83, model.py:34-39) -------------- */
size_t tohip_frustum_workspace_bytes(int64_t n_points);
/* cam_3xN: camera-frame points as (3,N).  dist_mask/fov_mask: N bytes of 0/1 (either may be NULL).
 * kept_idx (capacity N int32, may be NULL): ascending indices with both masks set; *kept_count (device
 * int32) their number.  Bit-exact with the reference's CPU path. */
int tohip_frustum_cull(const float *cam_3xN, int64_t n_points, const tohip_camera *cam_host, float min_dist,
                       float max_dist, uint8_t *dist_mask, uint8_t *fov_mask, int32_t *kept_idx, int32_t *kept_count,
                       void *workspace, size_t workspace_bytes, void *stream);
/* The cull stage of the per-camera pipeline (pc_processor.py:158-170) for n_wps poses at once: exact transform of the cloud
 * (to_camera_frame arithmetic; normalize as in tohip_to_camera_frame), hard frustum test, ordered compaction.
 * kept_idx (n_wps, n) int32 and kept_pts (n_wps, n, 3) f32 (camera frame) receive each pose's kept points in input
 * order in their first kept_count[w] rows (device int32 per pose) — worst-case sized, no host round trip. */
size_t tohip_cull_waypoints_workspace_bytes(int64_t n_points, int64_t n_wps);
int tohip_cull_waypoints(const float *xyz, int64_t n_points, const float *poses, const float *quats, int64_t n_wps,
                         int normalize, const tohip_camera *cam_host, float min_dist, float max_dist, int32_t *kept_idx,
                         float *kept_pts, int32_t *kept_count, void *workspace, size_t workspace_bytes, void *stream);
/* The same with the poses' kept points laid END TO END in kept_pts (what tohip_hidden_pts_removal_batched reads: the occlusion
 * refresh's next stage, pc_processor.py:171-187 per camera): pose w's rows are [seg_off[w], seg_off[w+1]) of kept_pts, seg_off
 * (n_wps + 1 device int64) is written here; kept_idx keeps its (n_wps, n) layout.  kept_pts must still hold n_wps * n rows
 * (nobody knows the counts beforehand).  One launch more than tohip_cull_waypoints, no copy afterwards. */
int tohip_cull_waypoints_packed(const float *xyz, int64_t n_points, const float *poses, const float *quats, int64_t n_wps,
                                int normalize, const tohip_camera *cam_host, float min_dist, float max_dist, int32_t *kept_idx,
                                float *kept_pts, int32_t *kept_count, int64_t *seg_off, void *workspace, size_t workspace_bytes,
                                void *stream);
/* gather rows: out[i,:] = xyz[idx[i],:] for i < min(*count, capacity) (count: device), xyz (N,3) or (3,N) by in_layout.  out_xyz
 * holds capacity rows; a count above capacity writes the first capacity rows and nothing beyond them. */
int tohip_gather_points(const float *xyz, int64_t n_points, int in_layout, const int32_t *idx, const int32_t *count,
                        int64_t capacity, float *out_xyz, void *stream);

/* ---- hidden-point removal (tools.py:38-85) ------------------------------------------------------ */
/* Recommended workspace.  The hull's face pool takes every byte beyond the per-point part; the recommendation holds
 * n/2 faces (HPR of a scene keeps a few % of the points).  A hull that creates more returns TOHIP_ENOSPC: call again
 * with a larger workspace (4x is what the Python host does; 8 faces per point is never exceeded). */
size_t tohip_hpr_workspace_bytes(int64_t n_points);
/* sphericalFlip (tools.py:38-53): flipped (N,3), radius_out[0] = max||p|| * 10^param. Bit-exact.  workspace: at least
 * TOHIP_FLIP_WORKSPACE_BYTES of scratch (the blocks' maxima of the norms). */
#define TOHIP_FLIP_WORKSPACE_BYTES 8192
int tohip_spherical_flip(const float *xyz, int64_t n_points, float param, float *flipped, float *radius_out,
                         void *workspace, size_t workspace_bytes, void *stream);
/* hidden_pts_removal (tools.py:67-85): flip, convex hull of flipped points + origin (double
 * precision quickhull on the GPU), visible = hull vertices in ascending index order minus the LAST
 * one (the reference drops hull.vertices[-1] unconditionally).  visible_idx capacity N int32;
 * *visible_count device int32; mask (N floats of 0/1, may be NULL).  SYNCHRONISES the stream (the hull
 * is built in rounds whose convergence is read back).  The read-back is a 128-byte record that a one-wave kernel writes into mapped
 * host memory and the calling thread polls: the library keeps two such records per (host thread, device) — the one piece of state it
 * holds between calls, allocated on the thread's first build on that device and freed when the thread ends. */
int tohip_hidden_pts_removal(const float *xyz, int64_t n_points, float param, int32_t *visible_idx,
                             int32_t *visible_count, float *mask, void *workspace, size_t workspace_bytes,
                             void *stream);

/* hidden_pts_removal of n_segments independent clouds in one pass, each seen from its own origin: the
 * per-camera use of HPR in pc_processor.py:171-178 (one segment per camera topic / per waypoint).  xyz holds the
 * segments end to end; segment s = rows [seg_offsets_host[s], seg_offsets_host[s+1]) (HOST array, n_segments+1,
 * seg_offsets_host[0] = 0).  Every segment gets its own flip radius (max norm of ITS points) and its own
 * "drop the last hull vertex".  All hulls advance in the same rounds.
 *   visible_idx          capacity n_total int32: rows of xyz, ascending; segment s's visible rows are
 *                        visible_idx[seg_visible_offsets[s] : seg_visible_offsets[s+1]]
 *   seg_visible_offsets  n_segments+1 int32 (device)
 *   mask                 n_total floats 0/1, or NULL
 *   seg_status           n_segments int32 (device) or NULL: 0 ok; 1 fewer than 4 points, 2 flat — scipy raises
 *                        QhullError for both; 3 a NaN among its (flipped) points —
 *                        scipy raises ValueError; here such a segment reports no visible points
 * SYNCHRONISES the stream. */
size_t tohip_hpr_batched_workspace_bytes(int64_t n_total, int32_t n_segments);
int tohip_hidden_pts_removal_batched(const float *xyz, const int64_t *seg_offsets_host, int32_t n_segments, float param,
                                     int32_t *visible_idx, int32_t *seg_visible_offsets, float *mask, int32_t *seg_status,
                                     void *workspace, size_t workspace_bytes, void *stream);

/* convexHull (tools.py:56-64): ascending hull-vertex indices of pts (n,3), optionally with the origin
 * appended as point n.  idx capacity n+1 int32; *count device int32; *rounds_host (may be NULL) the
 * number of insertion rounds.  SYNCHRONISES the stream. */
int tohip_convex_hull_vertices(const float *pts, int64_t n_points, int with_origin, int32_t *idx, int32_t *count,
                               int32_t *rounds_host, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the O(W) remainder of an optimisation step, on the device (no host sync inside a run) ---------
 * criterion's regularisers (model.py:244-260) with analytic gradients.  loss_terms[0..4] = vis (copied from
 * scalars[1]), l2, length, smooth, total.  grad_poses (W,3), may be NULL: the regularisers' gradient, added to
 * the existing content when accumulate != 0 (i.e. on top of the visibility gradient). */
int tohip_traj_regularizers(const float *poses, const float *poses0, int64_t n_wps, float smoothness_weight,
                            float traj_length_weight, float eps, const float *scalars, float *loss_terms,
                            float *grad_poses, int accumulate, const float *state, float *grad_terms, void *stream);
/* grad_terms (may be NULL): (3, W, 3) floats, the gradients of l2, length and smooth separately (their sum is what
 * grad_poses receives) — for callers that differentiate a single term of model.loss. */
/* state (may be NULL): when given, loss_terms is the base of an (n_steps, 8) log and the row written is
 * state[3] = steps taken so far — the launch then carries no per-step host value and can be replayed from a
 * hipGraph.  Same convention for tohip_adam_step (step <= 0: step index = state[3] + 1) and tohip_early_stop. */
/* The same with the clearance term: clearance_terms (W doubles) as tohip_clearance left them in its workspace for these positions,
 * with weight clearance_weight; loss_terms[5] = clearance and loss_terms[4] = the five-term total, rounded once (as
 * tohip_traj_opt_step and tohip_traj_loss_forward write it).  grad_poses / grad_terms: the regularisers' gradients only. */
int tohip_traj_regularizers_clearance(const float *poses, const float *poses0, int64_t n_wps, float smoothness_weight,
                                      float traj_length_weight, float eps, const float *scalars, float *loss_terms,
                                      float *grad_poses, int accumulate, const float *state, float *grad_terms,
                                      float clearance_weight, const double *clearance_terms, void *stream);
/* rows r*step of a (.., cols) array <-> a compact (n_rows, cols) array: the every-wps_step-th waypoint selection
 * of model.py:217 (scatter = 0: gather src[r*step] -> dst[r]; 1: scatter src[r] -> dst[r*step]). */
int tohip_rows_strided(const float *src, int64_t n_rows, int cols, int step, int scatter, float *dst, void *stream);
/* torch.optim.Adam update of one parameter group (defaults of trajectory_optimization.py:91-94); step is the
 * 1-based iteration; a no-op once state[2] != 0 (early stop reached).  state may be NULL.  0 < n <= 2^31 - 1, as in
 * tohip_adam_step_multi. */
int tohip_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                    float beta2, float eps, int32_t step, const float *state, void *stream);
/* The same update for up to TOHIP_ADAM_MAX_GROUPS parameter tensors in ONE launch (the reference's optimiser holds two:
 * poses @ lr_pose, quats @ lr_quat, trajectory_optimization.py:91-94).  groups_host: HOST array. */
#define TOHIP_ADAM_MAX_GROUPS 8
typedef struct tohip_adam_group {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t n;
    float lr, beta1, beta2, eps;
    int32_t step; /* 1-based */
} tohip_adam_group;
int tohip_adam_step_multi(const tohip_adam_group *groups_host, int32_t n_groups, void *stream);
/* early-stop rule of trajectory_optimization.py:100-124 on the device.  state (8 floats, zero-initialised by
 * the caller): [0] reward0 [1] smooth0 [2] stopped [3] steps taken [4] visibility gain [5] smoothness gain. */
int tohip_early_stop(const float *scalars, const float *loss_terms, float rewards_th, float smoothness_th, float *state,
                     int row_from_state, void *stream);

/* The same step remainder in ONE launch (one block; W up to a few thousand): scatter of the evaluated waypoints'
 * visibility gradients (rows r -> waypoint r*step, zero elsewhere) into poses_grad (W,3) / quats_grad (W,4), criterion
 * regularisers and their gradient on top, both Adam updates (step index state[3]+1, skipped once stopped), the loss log
 * row state[3] and the early-stop rule.  Equivalent to tohip_rows_strided x2 + tohip_traj_regularizers +
 * tohip_adam_step x2 + tohip_early_stop with `state`. */
int tohip_traj_step_tail(float *poses, float *quats, const float *poses0, int64_t n_wps, const float *poses_grad_eval,
                         const float *quats_grad_eval, int64_t n_eval, int step, float *poses_grad, float *quats_grad,
                         float *exp_avg_p, float *exp_avg_sq_p, float *exp_avg_q, float *exp_avg_sq_q,
                         float smoothness_weight, float traj_length_weight, float eps, float lr_pose, float lr_quat,
                         float beta1, float beta2, float adam_eps, float rewards_th, float smoothness_th,
                         const float *scalars, float *loss_terms, float *state, void *stream);
/* The same for n_traj equal-length trajectories laid end to end (block b = trajectory b): poses / quats / poses0 / gradients /
 * Adam moments (n_traj x W rows), poses_grad_eval / quats_grad_eval (n_traj x n_eval rows), scalars (n_traj x 4),
 * state (n_traj x 8), loss_terms: trajectory b's log starts at loss_terms + b * loss_terms_stride floats. */
int tohip_traj_step_tail_multi(float *poses, float *quats, const float *poses0, int64_t n_wps, int64_t n_traj,
                               const float *poses_grad_eval, const float *quats_grad_eval, int64_t n_eval, int step,
                               float *poses_grad, float *quats_grad, float *exp_avg_p, float *exp_avg_sq_p, float *exp_avg_q,
                               float *exp_avg_sq_q, float smoothness_weight, float traj_length_weight, float eps, float lr_pose,
                               float lr_quat, float beta1, float beta2, float adam_eps, float rewards_th, float smoothness_th,
                               const float *scalars, float *loss_terms, int64_t loss_terms_stride, float *state, void *stream);
/* tohip_traj_step_tail_multi with the clearance term: clearance_grad (n_traj W, 3) and clearance_terms (n_traj W doubles) as
 * tohip_clearance left them for these positions (its grad rows and its workspace) with weight clearance_weight.  The full gradient is
 * vis + (regularisers + clearance), as in tohip_traj_opt_step; the loss row gets [5] = clearance and total includes it. */
int tohip_traj_step_tail_clearance(float *poses, float *quats, const float *poses0, int64_t n_wps, int64_t n_traj,
                                   const float *poses_grad_eval, const float *quats_grad_eval, int64_t n_eval, int step,
                                   float *poses_grad, float *quats_grad, float *exp_avg_p, float *exp_avg_sq_p, float *exp_avg_q,
                                   float *exp_avg_sq_q, float smoothness_weight, float traj_length_weight, float eps, float lr_pose,
                                   float lr_quat, float beta1, float beta2, float adam_eps, float rewards_th, float smoothness_th,
                                   const float *scalars, float *loss_terms, int64_t loss_terms_stride, float *state,
                                   float clearance_weight, const float *clearance_grad, const double *clearance_terms, void *stream);
int tohip_gather_waypoints_multi(const float *poses, const float *quats, int64_t n_wps, int64_t n_traj, int64_t n_eval, int step,
                                 float *poses_e, float *quats_e, void *stream);
/* poses_e[r] = poses[r*step], quats_e[r] = quats[r*step] for r < n_eval, in one launch. */
int tohip_gather_waypoints(const float *poses, const float *quats, int64_t n_eval, int step, float *poses_e, float *quats_e,
                           void *stream);

/* ---- clearance: how far each waypoint is from the cloud (clearance_kernels.hip) -------------------------------------------
 * For query positions t_w (n_queries, 3) over a packed cloud (sorted or not): d2_w = the smallest fl((dx*dx + dy*dy) + dz*dz),
 * dx = fl(t_w.x - x_i.x) ... in f32 without contraction, over the rows with three finite coordinates; ties go to the lowest caller
 * row.  idx[w] = that row, or -1 when no point has d2 < fl(r*r) (or t_w has a non-finite coordinate); d[w] = (float)sqrt((double)
 * d2_w), +inf when idx[w] = -1.  The term: clearance = weight x sum_w (r - d_w)^2 over the waypoints with idx >= 0, summed in f64
 * in w order and rounded to f32 (value: one device float, may be NULL); its gradient -2 weight (r - d_w)(t_w - x_idx) / d_w in f64,
 * rounded to f32, zero when idx = -1 or d_w = 0, into grad (n_queries, 3; may be NULL), overwritten or (accumulate != 0) added to.
 * workspace: tohip_clearance_workspace_bytes(n_queries); it holds the per-query (r - d_w)^2 (f64, query order) after the call.
 * radius > 0 and weight >= 0, both finite.  One block of 16 waves per query prunes the 256-point tile spheres; no atomics: the results do
 * not depend on the launch.  One launch (two with value). */
size_t tohip_clearance_workspace_bytes(int64_t n_queries);
int tohip_clearance(const void *packed, int64_t n_points, const float *queries, int64_t n_queries, float radius, float weight, float *d,
                    int32_t *idx, float *value, float *grad, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
/* bytes of tohip_traj_loss.clearance_scratch / tohip_traj_opt.clearance_scratch: gradient rows (n_traj W, 3) f32 at offset 0, then
 * the per-waypoint terms */
size_t tohip_traj_clearance_scratch_bytes(int64_t n_wps, int64_t n_traj);

/* The swept term: the same hinge on each SEGMENT's distance to the cloud, so that the straight line between two waypoints stays off
 * it as well.  poses (n_traj n_wps, 3): n_traj trajectories of n_wps >= 2 waypoints laid end to end; segment (b, w), w < n_wps - 1,
 * joins a = waypoint w and b = waypoint w + 1 of trajectory b — never two trajectories.  In f32 without contraction: e = fl(b - a),
 * ee = fl(fl(ex ex + ey ey) + ez ez), inv = fl(1 / ee) when ee > 0, else 0; per point x with three finite coordinates u = fl(x - a),
 * s = fmin(fmax(fl(fl(fl(ux ex + uy ey) + uz ez) inv), 0), 1) (a NaN becomes 0), q = fl(u - fl(s e)), d2 = fl(fl(qx qx + qy qy) + qz qz).
 * idx = the argmin of d2 over d2 < fl(r r), ties to the lowest caller row; -1 when there is none or an end is not finite (a = b is
 * tohip_clearance's query bit for bit).  d = (float)sqrt((double)d2), +inf when idx = -1; s = where along the segment the closest
 * point c lies (0 = a, 1 = b), recomputed in f64 from the f32 coordinates (0 when idx = -1).  d, idx, s: (n_traj (n_wps - 1)).
 * The term: weight x sum over the segments of (r - d)^2, per trajectory, f64 in order, rounded to f32 (value: n_traj device floats,
 * may be NULL).  Its gradient, with n = (c - x) / |c - x|: g_a = -2 weight (r - d)(1 - s) n, g_b = -2 weight (r - d) s n in f64
 * (zero when idx = -1 or |c - x| = 0); grad (n_traj n_wps, 3; may be NULL; overwritten) row w = (float)(g_b of segment w - 1 + g_a
 * of segment w).  workspace: tohip_clearance_segments_workspace_bytes(n_wps, n_traj); after the call it holds (n_traj n_wps) doubles
 * at offset 0 — the segment's (r - d)^2 at its first waypoint's row, 0 at a trajectory's last — which is what
 * tohip_traj_step_tail_clearance, tohip_traj_regularizers_clearance and the team calls take as clearance_terms (with grad as
 * clearance_grad), then the per-segment g_a, g_b.  radius > 0 and weight >= 0, both finite.  One block of 16 waves per segment and one
 * thread per waypoint; no atomics: the results do not depend on the launch.  Two launches (three with value). */
size_t tohip_clearance_segments_workspace_bytes(int64_t n_wps, int64_t n_traj);
int tohip_clearance_segments(const void *packed, int64_t n_points, const float *poses, int64_t n_wps, int64_t n_traj, float radius,
                             float weight, float *d, int32_t *idx, float *s, float *value, float *grad, void *workspace,
                             size_t workspace_bytes, void *stream);
/* bytes of clearance_scratch with TOHIP_TRAJ_CLEARANCE_SEGMENTS: tohip_traj_clearance_scratch_bytes' rows and terms at the same
 * offsets, then the per-segment g_a, g_b */
size_t tohip_traj_clearance_segments_scratch_bytes(int64_t n_wps, int64_t n_traj);

/* The same segment query for n_edges UNRELATED segments: edge e joins a[e] and b[e] (two (n_edges, 3) device arrays).  d, idx, s
 * (n_edges each; any of them may be NULL) are bit for bit what tohip_clearance_segments writes for a trajectory of the two waypoints
 * a[e], b[e] — the definition above — without the term and its gradient.  One wave per edge, four edges to a block (the 16-wave block
 * per segment above is sized for the hundred segments of a path, this for the tens of thousands of pairs of a node set); a sorted or
 * an unsorted packed cloud; no atomics: the results do not depend on the launch.  radius > 0 and finite.  One launch. */
int tohip_clearance_edges(const void *packed, int64_t n_points, const float *a, const float *b, int64_t n_edges, float radius, float *d,
                          int32_t *idx, float *s, void *stream);

/* ---- a collision-checked tour through chosen views (tour_kernels.hip) ----------------------------------------------
 * nodes (n, 3) f32 on the device, 2 <= n <= TOHIP_TOUR_MAX_NODES; node 0 is where the tour starts.  Edge (i, j), i < j, has the index
 * e = i n - i (i + 1) / 2 + (j - i - 1) (the upper triangle, row-major) and is OPEN iff both ends are finite and edge_idx[e] == -1 —
 * edge_idx: the idx of tohip_clearance_edges for a = node i, b = node j (n (n - 1) / 2 int32), or NULL: every edge between finite nodes
 * — and its length fits.  Lengths are integers in units of 2^-20 m: in f64 without contraction dx = (double)x_i - (double)x_j ...,
 * w_ij = llrint(sqrt((dx dx + dy dy) + dz dz) 2^20); an edge with w_ij > 2^40 is closed.
 * Closure: D (n, n) int64 = w_ij on open edges, 0 on the diagonal, INF = 2^62 elsewhere; nxt (n, n) int32 = j on open edges, -1
 * elsewhere; Floyd-Warshall with k ascending: when D[i][k] + D[k][j] < D[i][j] strictly and both terms are below INF, D[i][j] = the
 * sum and nxt[i][j] = nxt[i][k] (one launch per k, one thread per (i, j): row and column k do not change during iteration k, so the
 * sweep is the serial loop).  R = {j : D[0][j] < INF}, m = |R|.  Start order: t[0] = 0, then repeatedly the unvisited j in R with the
 * smallest D[t[last]][j], ties to the lowest j; its length (with closed != 0: back to node 0 included) is nn_length_fixed.
 * 2-opt, best improvement, position 0 fixed: for 1 <= i < j <= m - 1 reversing t[i..j] changes the length by D[t[i-1]][t[j]] +
 * D[t[i]][t[j+1]] - D[t[i-1]][t[i]] - D[t[j]][t[j+1]] (closed: t[m] = t[0]; open and j = m - 1: the two terms that name t[m] are
 * dropped); the move with the most negative change is applied, ties to the lowest i and then the lowest j, until no change is
 * negative (converged = 1) or max_moves moves are done (converged says whether a negative change is left).
 * buf (tohip_tour_bytes(n) device bytes, caller-owned, 256-byte aligned), every section aligned to 256 bytes: [header 32 x int64:
 * [0] m [1] moves [2] converged [3] length_fixed [4] nn_length_fixed [5] status — bit 0: node 0 has a non-finite coordinate (m = 1)]
 * [order n int32: the first m count, -1 behind them] [unreachable n uint8] [D n x n int64] [nxt n x n int32].  The walk from u to v
 * is u, nxt[u][v], nxt[nxt[u][v]][v], ..., v.  n + 2 launches, nothing synchronises; integers throughout: the same bits in every run.
 * tohip_tour_bytes: 0 for an n out of range. */
#define TOHIP_TOUR_MAX_NODES 256
size_t tohip_tour_bytes(int64_t n);
int tohip_tour_plan(const float *nodes, int64_t n, const int32_t *edge_idx, int closed, int64_t max_moves, void *buf, size_t bytes,
                    void *stream);

/* ---- a free-space roadmap (roadmap_kernels.hip) ------------------------------------------------------------------
 * nodes (n_nodes, 3) f32 on the device, 2 <= n_nodes <= TOHIP_ROADMAP_MAX_NODES, supplied by the caller; 1 <= k <= TOHIP_ROADMAP_MAX_K.
 * The key of a pair (i, j), i != j: with lo = min(i, j), hi = max(i, j), in f64 without contraction dx = (double)x_lo - (double)x_hi
 * ..., d2 = (dx dx + dy dy) + dz dz — one value per unordered pair.
 * tohip_roadmap_knn: nbr (n_nodes, k) int32 = the k candidates j != i with the smallest (d2, j), ties to the lower j, in ascending
 * order of that key; both ends finite and d2 <= (double)max_edge^2 (max_edge >= 0; +inf: no limit); -1 in the slots no candidate
 * fills (every slot of a node that is not finite).  len (n_nodes, k) int64 = llrint(sqrt(d2) 2^20), the tour's length (held at 2^42;
 * a slot above 2^40 is stored and never open), -1 in an empty slot.  One launch, no atomics: the same bits in every run.
 * The edge stage is tohip_clearance_edges with a = node min(i, j), b = node max(i, j) for the filled slots; open (n_nodes, k) uint8 is
 * the caller's array: non-zero where the slot is filled, its length fits and that query gave idx == -1.  The graph is undirected:
 * {i, j} is an edge iff an open slot names it in either list.
 * tohip_roadmap_relax: src (n_sources) int32 on the device, 1 <= n_sources <= TOHIP_ROADMAP_MAX_SOURCES; D (n_sources, n_nodes) int64.
 * init != 0: D[s][v] = INF = 2^62, D[s][src[s]] = 0 first.  Then n_sweeps (0 <= n_sweeps <= n_nodes) sweeps over all (source, node,
 * slot) triples, each relaxing both directions of an open slot with a 64-bit integer atomic minimum.  *changed (one device int32) is
 * zeroed and then holds the number (from 1) of the call's last sweep that lowered anything: the table is final when
 * *changed < n_sweeps.  The fixed point — the shortest route lengths over the open edges — does not depend on the order of the
 * relaxations; the number of sweeps it takes may.  At most n_nodes sweeps are ever needed.  Launches only.
 * tohip_roadmap_pred (after convergence): pred (n_sources, n_nodes) int32 = the lowest u with {u, v} open and D[s][u] + len == D[s][v];
 * -1 for the source and for v no route reaches.  Two launches.  Coincident nodes are joined by zero-length edges and may name each
 * other: a walk back from a goal follows pred until it would re-enter a node and then searches the tight edges (D[u] + len == D[v]).
 * tohip_roadmap_routes_bytes: the bytes of one buffer that holds [D][pred][changed], every section aligned to 256 bytes (0 for sizes
 * out of range); the entries take the three pointers, so the caller may also keep them apart.
 * tohip_tour_plan_via: tohip_tour_plan with a roadmap behind it.  via_D: row i (leading dimension via_ld >= n, in int64) holds the
 * roadmap's route lengths from tour node i, its first n columns those to the tour nodes (the tour nodes are the roadmap's first n).
 * The initial leg is w_ij = min(direct, via_D[i][j]) with direct today's value (the integer length of an open straight leg, else
 * INF); via_flag (n, n) uint8 = 1 iff via_D[i][j] < direct strictly; nxt = j where w_ij < INF.  Everything behind that is
 * tohip_tour_plan's. */
#define TOHIP_ROADMAP_MAX_NODES 16384
#define TOHIP_ROADMAP_MAX_K 32
#define TOHIP_ROADMAP_MAX_SOURCES 256
int tohip_roadmap_knn(const float *nodes, int64_t n_nodes, int64_t k, float max_edge, int32_t *nbr, int64_t *len, void *stream);
size_t tohip_roadmap_routes_bytes(int64_t n_nodes, int64_t n_sources);
int tohip_roadmap_relax(const int32_t *nbr, const int64_t *len, const uint8_t *open, int64_t n_nodes, int64_t k, const int32_t *src,
                        int64_t n_sources, int64_t *D, int64_t n_sweeps, int32_t *changed, int init, void *stream);
int tohip_roadmap_pred(const int32_t *nbr, const int64_t *len, const uint8_t *open, int64_t n_nodes, int64_t k, const int32_t *src,
                       int64_t n_sources, const int64_t *D, int32_t *pred, void *stream);
int tohip_tour_plan_via(const float *nodes, int64_t n, const int32_t *edge_idx, const int64_t *via_D, int64_t via_ld, int closed,
                        int64_t max_moves, void *buf, size_t bytes, uint8_t *via_flag, void *stream);

/* ---- refine a planned walk into a trajectory (path_kernels.hip) -----------------------------------------------------
 * nodes (n_nodes, 3) f32 on the device in walking order, 2 <= n_nodes = L <= TOHIP_PATH_MAX_NODES; keep (L) uint8 or NULL: the nodes
 * the result must pass through (nodes 0 and L - 1 always are); quats (L, 4) f32 or NULL; 1 <= window = W <= L - 1.
 * A chord is a pair (i, j), i < j, j - i <= W, of length w_ij = llrint(sqrt(d2) 2^20), the tour's length (d2 in f64 without
 * contraction, the differences lower index minus higher; held at 2^42).  The input leg (i, i + 1) is always open.  A chord with
 * j >= i + 2 is open iff no kept node lies strictly between i and j, w_ij <= 2^40 and open_band[i][j - i - 1] != 0 — open_band (L, W)
 * uint8 is the caller's: non-zero where tohip_clearance_edges gave idx == -1 for a = node i, b = node j (column 0, the input legs,
 * is not read).
 * Search: D[0] = 0, D[j] = min over open (i, j) of D[i] + w_ij; pred[j] = the lowest i that attains it, pred[0] = -1.  The corners
 * c_0 = 0 < ... < c_m = L - 1 follow pred back from L - 1: every kept node is a corner, length_fixed = D[L - 1] <= input_length_fixed
 * = the sum of the input legs, and W = 1 or keep all ones gives the input's nodes.
 * Rows: H = llrint((double)spacing 2^20), at least 1 and held at 2^42 (spacing = 0: corners only, n_q = 1).  Corner leg q from A =
 * node c_q to B = node c_q+1, of length w_q, is cut into n_q = max(1, (w_q + H - 1) / H) equal pieces: row (q, t), 0 <= t < n_q, is per
 * coordinate (float)((double)A + ((double)B - (double)A) ((double)t / (double)n_q)) in f64 without contraction (t = 0: A itself); the
 * last row is node L - 1; R = 1 + the sum of n_q.  row_node (R) int32 = the input index at a corner row, -1 at an interpolated one.
 * With quats: for a row between the consecutive kept corners a and b, u = s_row / S_ab with S_ab the summed lengths of the corner legs
 * from a to b and s_row those before the row's leg plus ((double)w_q (double)t) / (double)n_q (u = 0 when S_ab = 0); q_a, q_b = the
 * two kept rows' quaternions divided by their f64 norms sqrt(((w w + x x) + y y) + z z), q_b negated when q_a . q_b < 0; the row's
 * quaternion is (1 - u) q_a + u q_b divided by its norm, rounded to f32.  A kept row's quaternion is its own, normalised; the
 * quaternions of rows that are not kept are never read.
 * buf (tohip_path_bytes(L, max_rows) device bytes, caller-owned, 256-byte aligned, 1 <= max_rows <= TOHIP_PATH_MAX_ROWS), every
 * section aligned to 256 bytes: [header 32 x int64: [0] m [1] R [2] length_fixed [3] input_length_fixed [4] status [5] the number of
 * open chords with j >= i + 2] [D L int64] [pred L int32] [corner L int32: the first m + 1 count, -1 behind them] [out_poses
 * max_rows x 3 f32] [out_quats max_rows x 4 f32] [row_node max_rows int32].
 * status bit 0: a coordinate of nodes, or a kept row's quaternion, is not finite, or that quaternion is zero: only the header is
 * written, with m = R = 0.  Bit 1: R > max_rows: the header ([1] = the R that is needed), D, pred and corner are written, no row is.
 * One launch of one block, nothing synchronises; integers after the lengths: the same bits in every run.
 * tohip_path_bytes: 0 for sizes out of range.  spacing must be finite and >= 0. */
#define TOHIP_PATH_MAX_NODES 1024
#define TOHIP_PATH_MAX_ROWS 4096
size_t tohip_path_bytes(int64_t n_nodes, int64_t max_rows);
int tohip_path_refine(const float *nodes, const float *quats, const uint8_t *keep, int64_t n_nodes, int64_t window,
                      const uint8_t *open_band, float spacing, int64_t max_rows, void *buf, size_t bytes, void *stream);

/* ---- propose candidate views (propose_kernels.hip) --------------------------------------------------------------------
 * A pre-filter for tohip_views_*: where can a level camera stand, and which way should it look from there?  A heuristic by design: the
 * gate is on RANGE, not on camera depth, and nothing is occluded.
 * tohip_view_histogram: positions (n_positions, 3) f32 and open (n_positions) uint8 on the device, 1 <= n_positions <=
 * TOHIP_VIEW_MAX_POSITIONS; weights (n_points) int32 on the device in the CALLER's row order, each in [0, 32768] (not checked: a value
 * outside gives unspecified sums), or NULL: every point weighs 1; sectors = S in {8, 16, 32, 64, 128}; table_host: 2 (S/4 - 1) floats on
 * the HOST, c_k = (float)cos(2 pi k / S) for k = 1 .. S/4 - 1, then s_k = (float)sin(2 pi k / S) likewise, all finite (read before the
 * call returns; S = 8 has one c and one s); 1e-3 <= min_dist < max_dist and tan_v >= 0 (the tangent of half the vertical field of
 * view), all finite.
 * The pair test of position t and point x, f32 without contraction: d = fl(x - t); hh = fl(fl(dx dx) + fl(dy dy)), zz = fl(dz dz),
 * r2 = fl(hh + zz); range gate fl(min min) <= r2 <= fl(max max); elevation gate zz <= fl(fl(tan_v tan_v) hh); quadrant q and (a, b):
 * q = 0: dx > 0, dy >= 0 -> (dx, dy); q = 1: dx <= 0, dy > 0 -> (dy, -dx); q = 2: dx < 0, dy <= 0 -> (-dx, -dy); q = 3: dx >= 0, dy < 0
 * -> (-dy, dx); sector = q S/4 + #{k : fl(b c_k) >= fl(a s_k)} (a point on a boundary belongs to the upper sector).
 * hist (n_positions, S) int64, overwritten: hist[c][j] = the sum of the weights of the points that pass both gates from position c and
 * fall into sector j, the bearings [2 pi j / S, 2 pi (j + 1) / S) about +z.  Rows of the cloud with a coordinate that is not finite
 * never count; a position with such a coordinate or open = 0 gets a row of zeros.  prune != 0 (the product path): a 256-point tile
 * whose bounding sphere lies wholly outside the shell [min_dist, max_dist] of a position is not tested against it; the exact gates
 * decide every point of a kept tile, so prune changes no bit (0: every tile, for timing).  Integer sums: the same bits in every run,
 * for a sorted and an unsorted packed cloud alike.  One memset and one launch.
 * tohip_view_headings: hist (n_positions, S) int64; 0 <= half_window = hw, 2 hw + 1 <= S; 1 <= n_per <= TOHIP_VIEW_MAX_PER_POSITION;
 * 0 <= sep <= S; min_score >= 0.  score[c][h] = sum over j = -hw .. hw of hist[c][(h + j) mod S].  n_per rounds: h* = the argmax of
 * score over the unsuppressed h with score >= max(min_score, 1), ties to the lowest h; none: the remaining slots are heading -1,
 * score 0; otherwise slot r = (h*, score[h*]) and every h whose circular distance to h* is <= sep is suppressed.
 * heading (n_positions, n_per) int32, score (n_positions, n_per) int64.  One launch.
 * Both: every argument check returns before anything is enqueued. */
#define TOHIP_VIEW_MAX_POSITIONS 65536
#define TOHIP_VIEW_MAX_SECTORS 128
#define TOHIP_VIEW_MAX_PER_POSITION 8
int tohip_view_histogram(const void *packed, int64_t n_points, const float *positions, const uint8_t *open, int64_t n_positions,
                         const int32_t *weights, int32_t sectors, const float *table_host, float min_dist, float max_dist, float tan_v,
                         int32_t prune, int64_t *hist, void *stream);
int tohip_view_headings(const int64_t *hist, int64_t n_positions, int32_t sectors, int32_t half_window, int32_t n_per, int32_t sep,
                        int64_t min_score, int32_t *heading, int64_t *score, void *stream);

/* ---- input formats (pointcloud_utils.py, launch/voxels_filtering.launch) --------------------------------
 * PointCloud2 payload -> (N,3) f32 with non-finite rows removed, in message order
 * (pointcloud2_to_xyz_array, pointcloud_utils.py:197-198, + the callers' cast to f32).  data: the message's
 * byte buffer on the device, n_points = width*height; x/y/z_off and datatype (7 = FLOAT32, 8 = FLOAT64) from
 * its PointFields.  out_xyz capacity n_points rows (rows at and beyond *out_count are unspecified); *out_count device int32.
 * The workspace may hold anything on entry; REUSE it from message to message: from 2 M points on, one of its words remembers
 * whether the last message had invalid rows, and a message after one without any is unpacked with one read of its bytes instead of
 * two (16 M points: 94 instead of 140 us; same output either way — the hint only chooses the schedule). */
size_t tohip_ingest_workspace_bytes(int64_t n_points);
int tohip_pointcloud2_to_xyz(const uint8_t *data, int64_t n_points, int32_t point_step, int32_t x_off, int32_t y_off,
                             int32_t z_off, int32_t datatype, int32_t is_bigendian, int32_t remove_nans, float *out_xyz,
                             int32_t *out_count, void *workspace, size_t workspace_bytes, void *stream);
/* pcl::VoxelGrid as configured by launch/voxels_filtering.launch:11-21: drop non-finite points and points whose
 * filter field (0/1/2 = x/y/z, -1 = none) lies outside [limit_min, limit_max]; one centroid per occupied voxel,
 * voxels in ascending key order.  out_xyz capacity n rows; *out_count device int32: the number of voxels, or -1 when the grid
 * would have more than 2^31 - 1 cells (PCL: "leaf size is too small", it returns its input unfiltered). */
size_t tohip_voxel_grid_workspace_bytes(int64_t n_points);
int tohip_voxel_grid(const float *xyz, int64_t n_points, float leaf_x, float leaf_y, float leaf_z, int32_t filter_field,
                     float limit_min, float limit_max, float *out_xyz, int32_t *out_count, void *workspace,
                     size_t workspace_bytes, void *stream);
/* pc_to_voxel (pointcloud_utils.py:279-288): float64 occupancy grid (nx,ny,nz), 1.0 where a point falls.
 * pc: (n, cols>=3) f32 rows. */
int tohip_pc_to_voxel(const float *pc, int64_t n_points, int32_t cols, double resolution, double x0, double x1, double y0,
                      double y1, double z0, double z1, int32_t nx, int32_t ny, int32_t nz, double *voxel, void *stream);

/* ---- frustum rasterisation (render_pc_image, tools.py:122-173; pulsar itself cannot be pinned, see
 * render_kernels.hip): nearest-depth sphere splat of camera-frame points.  K9_host: row-major intrinsics in
 * HOST memory; image (height,width,3) f32; owner (may be NULL) (height,width) int32 winning point or -1;
 * owns_pixel (may be NULL) n int32 flags: the z-buffer visibility set. */
size_t tohip_render_workspace_bytes(int32_t width, int32_t height);
int tohip_render_points(const float *verts, int64_t n_points, const float *K9_host, int32_t width, int32_t height,
                        float radius, float znear, float zfar, float background, float *image, int32_t *owner,
                        int32_t *owns_pixel, void *workspace, size_t workspace_bytes, void *stream);

/* render_pc_image's `gamma` (tools.py:122, 160-171: pulsar's blending softness): every disc covering a pixel centre contributes with
 * weight (1 - distance to the disc's centre / its radius) * exp(normalised depth / gamma), the background with exp(0); the statement
 * of the blend is in render_kernels.hip (parity unpinned).  Deterministic: integer atomics in fixed point.  gamma > 0, zfar > znear. */
size_t tohip_render_blend_workspace_bytes(int32_t width, int32_t height);
int tohip_render_points_blend(const float *verts, int64_t n_points, const float *K9_host, int32_t width, int32_t height, float radius,
                              float znear, float zfar, float gamma, float background, float *image, void *workspace,
                              size_t workspace_bytes, void *stream);

/* The z-buffer visibility sets of n_clouds camera-frame clouds at once (tohip_render_points' owns_pixel for each): cloud w = the
 * first count[w] (device int32) rows of verts + w * n_stride * 3 — the layout tohip_cull_waypoints writes — with its own z-buffer;
 * visible[w * n_stride + j] = 1.0f when its point j owns a pixel, else 0.  Clouds go through in chunks of as many z-buffers as the
 * workspace holds (tohip_zbuffer_batched_workspace_bytes: up to 2 GB): three launches per chunk. */
size_t tohip_zbuffer_batched_workspace_bytes(int32_t width, int32_t height, int64_t n_clouds);
int tohip_zbuffer_visible_batched(const float *verts, int64_t n_stride, const int32_t *count, int64_t n_clouds, const float *K9_host,
                                  int32_t width, int32_t height, float radius, float znear, float zfar, float *visible,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ---- team coverage: B robots over one cloud behind ONE reward ------------------------
 * The team's visibility term is the entries above over the members' evaluated waypoints laid end to end as one trajectory
 * (n_traj = 1; tohip_gather_waypoints_multi when n_wps is not a multiple of the waypoint step).  The entries below are what stays
 * per member behind that one reward.  Members: n_members equal-length trajectories laid end to end (poses (B n_wps, 3), ...).
 *
 * tohip_team_state_bytes: the per-step state of a run of n_steps, zero-filled once by the caller:
 *   [state (n_steps + 1, B, 8) f32: tohip_traj_opt's state row per member — [0] the team's first mean reward, [1] the member's first
 *    smooth term, [2] stopped, [3] steps taken, [4] visibility gain, [5] the member's smooth gain]
 *   [terms (n_steps + 1, B, 4) f64: l2, length, smooth, - of every member at the positions step i starts from]
 * Row 0 of `terms` is tohip_team_loss's member_terms64 (call it on the starting positions before the first step).
 *
 * tohip_team_step_tail: step `step_index` (0-based, in order) of a run of n_steps, ONE launch, block b = member b: what
 * tohip_traj_step_tail_multi / _clearance do per trajectory — both kernels run ONE block of device code (opt_step.hpp:
 * tail_gradients, tail_adam), so a member's gradients, moments and parameters are a trajectory's bits for any B — with two
 * differences: `scalars` is ONE row, the team's, and the early stop is the team's: visibility gain = mean reward / the team's
 * first; smooth gain per member; the team stops at the first step where the visibility gain > rewards_th and EVERY member's smooth
 * gain > smoothness_th, all members together.  Loss rows (member b's at loss_log + b * loss_log_stride, n_steps rows of 8):
 * [0] vis [1] l2 [2] length [3] smooth [5] clearance of the member, [4] the TEAM total = vis, then l2, length, smooth [, clearance]
 * of every member in member order, one running f64 sum rounded once.  clearance_grad / clearance_terms: both NULL (no clearance
 * term) or the query's rows (B n_wps, 3) and per-waypoint terms (B n_wps). */
#define TOHIP_TEAM_MAX_MEMBERS 256
size_t tohip_team_state_bytes(int64_t n_members, int64_t n_steps);
int tohip_team_step_tail(float *poses, float *quats, const float *poses0, int64_t n_wps, int64_t n_members,
                         const float *poses_grad_eval, const float *quats_grad_eval, int64_t n_eval, int step, float *poses_grad,
                         float *quats_grad, float *exp_avg_p, float *exp_avg_sq_p, float *exp_avg_q, float *exp_avg_sq_q,
                         float smoothness_weight, float traj_length_weight, float eps, float lr_pose, float lr_quat, float beta1,
                         float beta2, float adam_eps, float rewards_th, float smoothness_th, const float *scalars, float *loss_log,
                         int64_t loss_log_stride, void *team_state, size_t team_state_bytes, int32_t n_steps, int32_t step_index,
                         float clearance_weight, const float *clearance_grad, const double *clearance_terms, void *stream);

/* tohip_team_loss: criterion's terms of every member in ONE launch (block b = member b) — member_terms (B, 8): [0] vis (scalars[1];
 * 0 when scalars is NULL) [1] l2 [2] length [3] smooth [5] clearance — with, each optional (NULL): member_terms64 (B, 4) f64 l2,
 * length, smooth, -; total (1): the team total as above (needs scalars); grad_poses (B n_wps, 3): the regularisers' gradient rows
 * (overwritten); grad_terms (B, 3, n_wps, 3): d l2, d length, d smooth of each member.  clearance_terms: NULL or (B n_wps). */
int tohip_team_loss(const float *poses, const float *poses0, int64_t n_wps, int64_t n_members, float smoothness_weight,
                    float traj_length_weight, float eps, const float *scalars, float clearance_weight, const double *clearance_terms,
                    float *member_terms, double *member_terms64, float *total, float *grad_poses, float *grad_terms, void *stream);

/* tohip_team_member_gains: what each member adds.  lo_members (B, npad): the per-member log-odds rows tohip_traj_forward_multi
 * (n_traj = B) leaves, packed order; prior_buf: NULL or the team's prior.  sums (DEVICE int64, tohip_team_member_gains_bytes =
 * 8 (1 + 2 B) bytes, zeroed by the call): [0] the fixed-point sum of sigmoid(S + prior), [1 + b] of sigmoid(S - lo_b + prior),
 * [1 + B + b] the points with lo_b > 0; S = the members' rows summed in member order in f32; fixed point: x 2^(47 - ceil(log2 N)),
 * the reward kernel's.  gain_b = (sums[0] - sums[1 + b]) / 2^shift / N.  Integer sums: the same bits every run.  B <= 16.
 * `packed` is the cloud the rows belong to (it fixes N's padding; the kernel itself reads the rows only).
 * A member whose row is NaN (a waypoint that sees nothing at all: max p == min p, NaN rewards in the reference) counts as absent:
 * its log-odds are taken as 0, its gain and count are 0. */
#define TOHIP_TEAM_MAX_GAINS 16
size_t tohip_team_member_gains_bytes(int64_t n_members);
int tohip_team_member_gains(const void *packed, int64_t n_points, const float *lo_members, int64_t n_members, const void *prior_buf,
                            int64_t *sums, size_t sums_bytes, void *stream);

/* ---- greedy view selection: the best k of M candidate views (views_kernels.hip) --------------------------------
 * A candidate view's log-odds row is the row tohip_traj_forward_multi writes for it taken as a trajectory of one body waypoint
 * (n_traj = M, traj_offsets = 0..M; a rig's C virtual waypoints summed into the one row).  The rows are kept as one CSR structure in
 * `views` (tohip_views_bytes(n_points, n_candidates, nnz_capacity) device bytes, caller-owned; its first 256 bytes — the header — zero-filled once before the first use): per candidate its
 * (packed index u32, log-odds f32) pairs with log-odds > 0, pads excluded, in ascending index order.  Layout, every section aligned
 * to 256 bytes: [header 32 x int64: [0] entries stored [1] entries needed by everything appended so far [2] status — bit 0: the
 * capacity does not hold them, bit 1: an append that did not continue the set [3] candidates appended [4] selection stopped]
 * [offsets (M + 1) int64] [absent M int32] [gain sums M int64] [chosen M int32] [segment counts 256 x ceil(Npad / 8192) int32]
 * [idx capacity u32] [val capacity f32].  Every call takes the three sizes the buffer was sized with.
 *
 * tohip_views_append: rows first .. first + n_rows - 1 of the set from lo_rows (n_rows, Npad) — one chunk of the forward's output,
 * n_rows <= TOHIP_VIEWS_MAX_CHUNK; chunks in order, first = 0 starts the set anew.  A row that holds a NaN (a view that sees nothing
 * at all: max p == min p) makes its candidate ABSENT: no entries, absent[c] = 1, never chosen.  Three launches (count per segment, a
 * one-block scan with the capacity check, ordered write).  A chunk that does not fit writes no entry and no offset: the status and
 * the needed count are all that change, and every later append and select is a no-op on the status.  needed_host = NULL: launches
 * only (read the header when convenient).  Non-NULL: the call SYNCHRONISES the stream, stores the entries needed by everything
 * appended so far and returns TOHIP_ENOSPC when the capacity does not hold them — size a new buffer with that count and append again
 * from first = 0.
 *
 * tohip_views_select: k greedy rounds, two launches each, nothing synchronises.  With F(x) = sum_i reward_fixed(r_i) of the rewards
 * tohip_traj_reward / _prior give for lo_sum = x (prior_buf: NULL or tohip_traj_prior_build's, same cloud), S = 0 and in round j
 * G_c = F(S + lo_c) - F(S) over candidate c's entries for every c neither chosen nor absent; c* = argmax G_c, ties to the lowest
 * index; the selection ends without choosing when no candidate is left, G_c* <= 0 or G_c* / 2^shift / N < min_gain (f64; shift =
 * 47 - ceil(log2 N)); else order[j] = c*, gain_fixed[j] = G_c*, S += lo_c* (f32), *n_selected = j + 1.  S: Npad floats, packed order
 * (zeroed by the call; pads stay 0) — what tohip_traj_coverage and tohip_traj_reward(_prior) take.  order / gain_fixed: k entries.
 * Integer sums: the same result in every run.  The call uses the sums and flags inside `views`: one selection at a time per set.
 *
 * tohip_views_row: candidate c's list scattered back into row (Npad floats: zero where nothing is stored, pads included; NaN at
 * every point for an absent candidate) — for tests and for looking.  Two launches. */
#define TOHIP_VIEWS_MAX_CHUNK 256
#define TOHIP_VIEWS_MAX_CANDIDATES 65536
size_t tohip_views_bytes(int64_t n_points, int64_t n_candidates, int64_t nnz_capacity);
int tohip_views_append(void *views, size_t views_bytes, int64_t n_points, int64_t n_candidates, int64_t nnz_capacity,
                       const float *lo_rows, int64_t first, int64_t n_rows, int64_t *needed_host, void *stream);
int tohip_views_select(void *views, size_t views_bytes, int64_t n_points, int64_t n_candidates, int64_t nnz_capacity,
                       const void *prior_buf, int64_t k, double min_gain, float *S, int32_t *order, int64_t *gain_fixed,
                       int32_t *n_selected, void *stream);
int tohip_views_row(const void *views, size_t views_bytes, int64_t n_points, int64_t n_candidates, int64_t nnz_capacity,
                    int64_t candidate, float *row, void *stream);

/* ---- a voxel-keyed log-odds map: coverage carried across changing clouds (covmap_kernels.hip) --------------------
 * What tohip_traj_coverage returns is indexed by the rows of one cloud.  This map keys it by position: a hash table of voxels on the
 * device that a coverage row is folded into and that ANY later cloud reads its prior from (tohip_traj_prior_build takes the result).
 *
 * Key of a point: per axis i = (int) floorf((x - origin) / resolution), in f32 throughout (correctly rounded division); the three
 * indices + 2^20, 21 bits each, packed x | y | z from the high end into a uint64; all ones marks an empty slot.  A point with a
 * non-finite coordinate or an index outside [-2^20, 2^20) is SKIPPED: counted, stored nowhere, read back as 0.
 *
 * Buffer (tohip_covmap_bytes(capacity) = 256 + 16 x capacity device bytes, caller-owned, 16-byte aligned; capacity a power of two in
 * [16, 2^32]): [header 256 B][capacity slots of 16 B: uint64 key | f32 value | uint32 pending].  Header, int64 words: [0] voxels
 * held [1] capacity [2] status of the last integrate / merge / rehash — bit 0: it would have left the table more than half full,
 * bit 1: a probe gave up (the table filled up while the call ran), bit 2: a merge of maps whose origin or resolution differ
 * [3] voxels the map holds after that call, or would have to hold (with bit 1 a lower bound: size for [0] + n_points instead)
 * [4] points that call skipped [5] rows it skipped for their log-odds (negative or non-finite) [6], [7] scratch; then five f32 at
 * byte 64: origin x, y, z, resolution, clamp_max.  tohip_covmap_init writes all of it (one launch): an empty map.
 *
 * tohip_covmap_integrate: points (n, 3) f32 rows and log_odds (n) f32 in the same order.  The observation of a voxel is the MAXIMUM
 * over the call's points that fall into it; then, one f32 operation per voxel, value = min(max(old, obs), clamp_max)
 * (TOHIP_COVMAP_MAX: a fused row, prior + lo_sum — idempotent) or min(old + obs, clamp_max) (TOHIP_COVMAP_ADD: an independent
 * observation); a voxel not seen before starts from 0 and is created even when its observation is 0.  fold != 0: runs of equal keys
 * in consecutive rows are reduced inside the wave before the table is touched (what the host layer passes: up to 4 x faster on rows
 * sorted by voxel, at most 0.02 ms slower at 1 M unsorted rows — DESIGN.md 10, Measured); 0: every row probes.  Same map either way.  The result — values, count, skipped counts — is the same in every run and under any permutation of the rows;
 * only the slot a key lands in may differ.  A call that would leave the table more than half full changes NOTHING but words 2..5:
 * the status and the needed count.  Allocate a map of capacity >= 2 x needed, tohip_covmap_rehash the old one into it and call again.
 * header_host = NULL: launches only.  Non-NULL (8 int64 on the host): the call SYNCHRONISES the stream, stores header words 0..7 and
 * returns TOHIP_ENOSPC when status bits 0 / 1 are set (TOHIP_EINVAL for bit 2).  Three launches.
 *
 * tohip_covmap_lookup: out[i] = the value of point i's voxel; 0 for a voxel the map does not hold and for a skipped point.  One
 * launch, nothing synchronises, the map is not written.
 * tohip_covmap_merge: every voxel of `other` integrated as one observation with the same two rules (same capacity rule and
 * header_host as integrate).  tohip_covmap_rehash: the same with TOHIP_COVMAP_MAX — into an empty map, a copy: the growth of a table.
 * tohip_covmap_export: the live voxels in no particular order (sort by key for a reproducible one): keys[v] (the packed key as
 * int64), values[v], centres[3 v ..] = origin + (index + 1/2) x resolution; at most out_capacity are written (size with word [0]).
 * tohip_covmap_read_header: SYNCHRONISES; words_host: 8 int64, geometry_host: 5 floats or NULL. */
#define TOHIP_COVMAP_MAX 0
#define TOHIP_COVMAP_ADD 1
size_t tohip_covmap_bytes(int64_t capacity);
int tohip_covmap_init(void *map, size_t map_bytes, int64_t capacity, const float *origin_host, float resolution, float clamp_max,
                      void *stream);
int tohip_covmap_integrate(void *map, size_t map_bytes, int64_t capacity, const float *points, const float *log_odds, int64_t n_points,
                           int mode, int fold, int64_t *header_host, void *stream);
int tohip_covmap_lookup(const void *map, size_t map_bytes, int64_t capacity, const float *points, int64_t n_points, float *out,
                        void *stream);
int tohip_covmap_merge(void *map, size_t map_bytes, int64_t capacity, const void *other, size_t other_bytes, int64_t other_capacity,
                       int mode, int64_t *header_host, void *stream);
int tohip_covmap_rehash(void *map, size_t map_bytes, int64_t capacity, const void *old_map, size_t old_bytes, int64_t old_capacity,
                        int64_t *header_host, void *stream);
int tohip_covmap_export(void *map, size_t map_bytes, int64_t capacity, int64_t out_capacity, int64_t *keys, float *values,
                        float *centres, void *stream);
int tohip_covmap_read_header(const void *map, int64_t *words_host, float *geometry_host, void *stream);

/* ---- occupancy bit grid and exact line-of-sight walks ("Voxel line of sight") -------
 * A dense grid of one bit per voxel, filled from any number of clouds, and an integer voxel traversal through it: "is B visible
 * from A", and a third kind of occlusion bit row beside the hull's and the z-buffer's.
 *
 * Geometry (tohip_occ_geom, a HOST struct handed to every call; the library keeps no state): origin and resolution r > 0 finite,
 * dims each in [1, 2048] with nx ny nz <= 2^31.  Buffer: tohip_occ_bytes(nx, ny, nz) device bytes (0 for bad dims), caller-owned,
 * 8-byte aligned: a 256-byte header, then one 32-bit word per brick of 4 x 4 x 2 voxels.  Nothing public depends on the layout.
 *
 * Coordinate of a position, per axis: g = (p - origin) / r in f32 (correctly rounded: numpy.float32 gives the same value); IN RANGE
 * iff g is finite and -2048 <= g < 4096 (the grid and an apron in which everything is free); q = (int) floorf(g * 256), the unit
 * 1/256 voxel; voxel = q >> 8.
 * tohip_occ_init: every voxel free.  tohip_occ_insert: each row of points (n, 3) f32 on the device whose coordinates are in range
 * and whose voxel lies inside dims sets that voxel's bit (32-bit integer atomic OR); every other row is skipped and counted.  Bits
 * are never cleared.  skipped_host (HOST, may be NULL): the number of skipped rows of this call — the call then synchronises.
 * tohip_occ_lookup: ijk (m, 3) int32 voxel indices -> out (m) uint8, 0 outside dims.
 *
 * The walk from A to B (fixed-point triples, in range): D = B - A, s = sign D, m = |D|, v0 = A >> 8, e = B >> 8; per axis the
 * distance to the next face n = (v+1) 256 - A for s > 0, A - v 256 for s < 0 (0 on a face: that step comes first).  It takes
 * sum |e - v0| steps, each along the axis — among those with v_a != e_a — with the smallest n_a / m_a, compared exactly as
 * n_a m_b < n_b m_a, ties to the lowest axis; then v_a += s_a and n_a += 256.  It visits v0 ... e.  A visited voxel is tested iff
 * cheb(v, v0) >= start_skip and cheb(v, e) > end_skip; the ray is blocked iff a tested voxel inside dims is occupied.  Skips are
 * in [0, 8192].
 * tohip_los_segments: a, b (n_rays, 3) f32 world points on the device -> out (n_rays) uint8: 1 clear, 0 blocked, 2 an endpoint out
 * of range.  tohip_los_rows: rows (n_wps, npad/32) int32 in the layout of tohip_occlusion_rows — bit i = packed position i of
 * `packed` (tohip_pack_cloud), 1 iff tohip_cull_waypoints(normalize = 1) with this camera and these limits keeps the point for
 * waypoint w (the same device functions: the same bit) and the ray from poses[w] to the point is not blocked; a ray with an
 * endpoint out of range counts as clear; pad bits 0.  One launch, nothing read back.  1 <= n_wps <= 65535.  prune != 0 skips the
 * 256-point tiles whose bounding sphere cannot pass the depth gate (never changes a bit).
 * stats (DEVICE uint64 x 2, may be NULL, zero-filled by the caller): += rays walked, += voxels visited.
 * Every argument check returns before anything is enqueued. */
typedef struct tohip_occ_geom {
    float origin[3];
    float resolution;
    int32_t dims[3];
} tohip_occ_geom;
size_t tohip_occ_bytes(int32_t nx, int32_t ny, int32_t nz);
int tohip_occ_init(void *grid, size_t grid_bytes, const tohip_occ_geom *geom, void *stream);
int tohip_occ_insert(void *grid, size_t grid_bytes, const tohip_occ_geom *geom, const float *points, int64_t n_points,
                     int64_t *skipped_host, void *stream);
int tohip_occ_lookup(const void *grid, size_t grid_bytes, const tohip_occ_geom *geom, const int32_t *ijk, int64_t m, uint8_t *out,
                     void *stream);
int tohip_los_segments(const void *grid, size_t grid_bytes, const tohip_occ_geom *geom, const float *a, const float *b, int64_t n_rays,
                       int32_t start_skip, int32_t end_skip, uint8_t *out, uint64_t *stats, void *stream);
int tohip_los_rows(const void *grid, size_t grid_bytes, const tohip_occ_geom *geom, const void *packed, int64_t n_points,
                   const float *poses, const float *quats, int64_t n_wps, const tohip_camera *cam, float min_dist, float max_dist,
                   int32_t start_skip, int32_t end_skip, int32_t prune, int32_t *rows, uint64_t *stats, void *stream);

/* ---- free space and frontiers ("Free space and frontiers") ---------------------------
 * The FREE PLANE is a second occupancy grid of the same geometry (same buffer size, same layout, every call above works on it) whose
 * set bit means "a ray passed through".  State of a voxel inside dims: 2 (occupied) if the occupied bit is set, otherwise 1 (free) if
 * the free bit is set, otherwise 0 (unknown).  State of a position: its voxel's; 3 where a coordinate is out of range or the voxel
 * lies outside dims.
 *
 * tohip_occ_carve: ray i runs from origins + origin_stride * i (origin_stride 0: one origin for all rays; 3: a row per ray) to
 * points + 3 i, all f32 on the device.  A ray with an endpoint out of range is skipped and counted (skipped_host, HOST, may be NULL:
 * the call then synchronises).  A, B: the fixed-point triples, D = B - A, L = floor(sqrt(D . D)) exactly.  max_range_fixed = R in
 * 1/256 voxel, 0 <= R <= 6144 * 256, 0 = none.  With R > 0 and L > R the ray is TRUNCATED: per axis B' = A + sign(D) floor(|D| R /
 * L), and it is not a hit; otherwise B' = B and it is a hit.  The walk A -> B' is the one above (same steps, same tie order); every
 * visited voxel inside dims gets its free bit, except the last voxel of a hit.  Bits are only ever set (32-bit integer atomic OR,
 * issued only where a brick's word lacks one of the gathered bits): any split and order of the rays gives the same plane.  The
 * occupied grid is not an argument.  flags (DEVICE uint8 x n_rays, may be NULL): 0 hit, 1 truncated, 2 skipped.  stats (DEVICE
 * uint64 x 3, may be NULL, zero-filled by the caller): += rays walked, += voxels visited (v_0 ... v_T of each), += atomics issued.
 * tohip_occ_state: positions (m, 3) f32 -> out (m) uint8.
 * tohip_occ_frontier: frontier (a third buffer of the same size, not one of the two) receives the mask of the voxels inside dims
 * whose state is 1 and of whose six face neighbours INSIDE DIMS at least min_unknown (1 .. 6) have state 0; its header and pad bits 0.
 * tohip_occ_count / tohip_occ_export: the set bits of any grid in ascending (word, bit) order — brick order.  count writes the
 * blocks' offsets into workspace (tohip_occ_export_workspace_bytes device bytes, 8-byte aligned; 0 for bad dims) and the total to
 * total_host (HOST, may be NULL; the one synchronisation).  export, handed that workspace and total, writes ijk (total, 3) int32 and
 * centres (total, 3) f32, centre = fl(origin + fl(fl(i + 0.5) r)) per axis; capacity (rows of the outputs) < total: TOHIP_ENOSPC and
 * nothing is written; no row at or beyond capacity is ever written.
 * Every argument check returns before anything is enqueued. */
int tohip_occ_carve(void *free_grid, size_t grid_bytes, const tohip_occ_geom *geom, const float *origins, int64_t origin_stride,
                    const float *points, int64_t n_rays, int64_t max_range_fixed, uint8_t *flags, uint64_t *stats, int64_t *skipped_host,
                    void *stream);
int tohip_occ_state(const void *occupied, const void *free_grid, size_t grid_bytes, const tohip_occ_geom *geom, const float *positions,
                    int64_t m, uint8_t *out, void *stream);
int tohip_occ_frontier(const void *occupied, const void *free_grid, void *frontier, size_t grid_bytes, const tohip_occ_geom *geom,
                       int32_t min_unknown, void *stream);
size_t tohip_occ_export_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int tohip_occ_count(const void *grid, size_t grid_bytes, const tohip_occ_geom *geom, void *workspace, size_t workspace_bytes,
                    int64_t *total_host, void *stream);
int tohip_occ_export(const void *grid, size_t grid_bytes, const tohip_occ_geom *geom, const void *workspace, size_t workspace_bytes,
                     int64_t total, int64_t capacity, int32_t *ijk, float *centres, void *stream);

/* ---- the clearance field ("Clearance field") ------------------------------------------
 * A FIELD has an occupancy grid's geometry and holds one uint16 per voxel inside dims, dense, x fastest (index (z ny + y) nx + x):
 * tohip_field_bytes(nx, ny, nz) = 2 nx ny nz device bytes (0 for bad dims), caller-owned; tohip_field_workspace_bytes is the same.
 * Obstacles: the voxels inside dims whose occupied bit is set and, where free_or_null is a free plane, also those of state 0
 * (neither bit: unknown); nothing outside dims.  Metric: gap2(v, u) = sum over the axes of max(|v_a - u_a| - 1, 0)^2, the squared
 * gap between the two voxel cubes in voxels — an exact integer, and any point of the closed cube of v is at least sqrt(gap2) r from
 * any point of the cube of u.  field[v] = min over the obstacles u of gap2(v, u) where that is <= D^2 (1 <= D <= 254), else 65535.
 * tohip_field_build: three launches (x, y, z), field and workspace ping-pong, the result lies in field; the planes are only read.
 * tohip_field_positions: positions (m, 3) f32 -> d2 (m) int32 — the voxel's value, 65535 in range but outside dims, -1 out of range
 * — and / or dist (m) f32 metres fl(fl(sqrt(d2)) r), +inf for 65535, NaN for -1; either output may be NULL, not both.
 * tohip_field_segments: legs a[e] -> b[e], (n_legs, 3) f32 world points, walked as tohip_los_segments walks (same steps, same tie
 * order, v_0 ... v_T) with no skip rule and no early exit: d2[e] int32 = the minimum of the field over the visited voxels inside
 * dims (65535: none inside dims, or all hold 65535; -1: an endpoint out of range), vox[e] int32 = the linear index of the first
 * visited voxel that attains it (-1 with 65535 or -1).  With edge_d / edge_idx (both or neither; d2 and vox may then be NULL) the
 * answer also comes in tohip_clearance_edges' shape for need2 in [0, 65535]: an open leg (d2 >= need2) +inf / -1, a blocked one
 * metres / vox, a leg with an endpoint out of range 0 / -2.
 * tohip_field_nodes: nodes (an occupancy grid buffer of grid_bytes, none of the inputs) receives the mask of the voxels inside dims
 * with field >= need2, every index i satisfying i % stride == stride / 2 (1 <= stride <= 2048) and — where the two planes of a map
 * are given (both or neither) — state 1; its header and pad bits 0.  tohip_occ_count / tohip_occ_export list it.
 * Every argument check returns before anything is enqueued; nothing synchronises with the host. */
size_t tohip_field_bytes(int32_t nx, int32_t ny, int32_t nz);
size_t tohip_field_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int tohip_field_build(const void *occupied, const void *free_or_null, size_t grid_bytes, const tohip_occ_geom *geom, int32_t D,
                      void *field, size_t field_bytes, void *workspace, size_t workspace_bytes, void *stream);
int tohip_field_positions(const void *field, size_t field_bytes, const tohip_occ_geom *geom, const float *positions, int64_t m,
                          int32_t *d2, float *dist, void *stream);
int tohip_field_segments(const void *field, size_t field_bytes, const tohip_occ_geom *geom, const float *a, const float *b,
                         int64_t n_legs, int32_t *d2, int32_t *vox, int32_t need2, float *edge_d, int32_t *edge_idx, void *stream);
int tohip_field_nodes(const void *field, size_t field_bytes, const void *occupied_or_null, const void *free_or_null, void *nodes,
                      size_t grid_bytes, const tohip_occ_geom *geom, int32_t need2, int32_t stride, void *stream);

/* ---- the evidence map ("Evidence map") ------------------------------------------------
 * An EVIDENCE buffer has an occupancy grid's geometry (origin, resolution, dims, brick layout: word w = ((z>>1) nby + (y>>2)) nbx +
 * (x>>2), bit b = x&3 | (y&3)<<2 | (z&1)<<4) and holds one signed 8-bit log-odds value per voxel IN BRICK ORDER: byte 32 w + b after
 * a 256-byte header (zero), so the 32 voxels of a brick word are 32 consecutive, 32-byte-aligned bytes.  tohip_evid_bytes(nx, ny, nz)
 * = 256 + 32 words device bytes (0 for bad dims), caller-owned, 16-byte aligned.  The value -128 means NEVER OBSERVED; pad voxels
 * (outside dims) hold -128 for ever.  State of a voxel with value L: unknown iff L == -128, otherwise occupied iff L > threshold,
 * otherwise free.  Parameters, all integers: hit and miss in [1, 127], -127 <= lmin <= threshold < lmax <= 127.
 *
 * tohip_evid_init: every voxel -128.
 * tohip_evid_fold: one scan.  hit_plane H and pass_plane M are occupancy grid buffers of the geometry (grid_bytes each; what
 * tohip_occ_insert and tohip_occ_carve fill).  For every voxel inside dims, base = (L == -128 ? 0 : L); where the H bit is set L <-
 * min(base + hit, lmax); otherwise, where the M bit is set, L <- max(base - miss, lmin); otherwise L is unchanged: a hit wins within a
 * scan, and a voxel is updated at most once per scan however many rays cross it.  Bits of H and M outside dims are ignored.  A brick
 * whose H and M words are both zero is not touched at all.  For every other brick the word of occupied_out receives exactly the bits
 * L > threshold and the word of free_out exactly the bits L != -128 and L <= threshold (pad bits 0), stored by the lane that owns the
 * word: handed the two planes of the previous fold over this buffer (empty planes for a fresh buffer), they hold exactly those bits
 * everywhere after every fold.  clear_scan != 0: every word of H and M that was not zero is zeroed — scratch planes are empty again
 * without an init launch; 0: H and M are only read.  counts (DEVICE uint64 x 4, may be NULL, zero-filled by the caller): += voxels
 * updated, += voxels newly known (they left -128), += occupied bits that appeared, += occupied bits that vanished.  Within a scan
 * nothing depends on a row order or a launch shape: the inputs are bit planes.  The five buffers must be five different ones.
 * tohip_evid_positions: positions (m, 3) f32 -> values (m) int8: the voxel's value, -128 also for a position out of range or outside
 * dims — and / or state (m) uint8: 0 unknown, 1 free, 2 occupied (L > threshold, -127 <= threshold <= 126), 3 out of range or
 * outside dims, tohip_occ_state's codes; either output may be NULL, not both.
 * Every argument check returns before anything is enqueued; nothing synchronises with the host. */
size_t tohip_evid_bytes(int32_t nx, int32_t ny, int32_t nz);
int tohip_evid_init(void *evid, size_t evid_bytes, const tohip_occ_geom *geom, void *stream);
int tohip_evid_fold(void *evid, size_t evid_bytes, void *hit_plane, void *pass_plane, void *occupied_out, void *free_out,
                    size_t grid_bytes, const tohip_occ_geom *geom, int32_t hit, int32_t miss, int32_t lmin, int32_t lmax,
                    int32_t threshold, int32_t clear_scan, uint64_t *counts, void *stream);
int tohip_evid_positions(const void *evid, size_t evid_bytes, const tohip_occ_geom *geom, int32_t threshold, const float *positions,
                         int64_t m, int8_t *values, uint8_t *state, void *stream);

/* ---- re-framing and merging maps (reframe_kernels.hip, DESIGN.md §10, "Re-framing and merging maps") ----
 * Voxel content moved from one box into another.  src and dst are two DIFFERENT buffers, each with its own geometry (its own dims);
 * (sx, sy, sz) is an integer voxel shift, each component in [-4096, 4096].  For every voxel v inside dst's dims the SOURCE VALUE is
 * that of src voxel v + s where that lies inside src's dims, otherwise EMPTY: bit 0 of a plane, -128 of an evidence buffer.  origin
 * and resolution of the two geometries are checked as everywhere (finite, r > 0) and not interpreted: the caller computes the shift.
 * Pad bits of dst stay 0, pad bytes stay -128, headers stay as tohip_occ_init / tohip_evid_init leave them.  src is only read; its
 * pads must be as the layer leaves them (0, -128).
 *
 * tohip_occ_transfer: two occupancy grid buffers.  mode 0 (COPY): every dst bit becomes the source bit.  mode 1 (OR): dst |= source.
 * counts (DEVICE uint64 x 1, may be NULL, zero-filled by the caller): += the bits set in dst afterwards that were not set before; for
 * COPY, whose dst is not read: += the bits set afterwards.  One lane owns one dst word: no atomic touches the plane.
 * tohip_evid_transfer: two evidence buffers, and the two derived planes of dst (grid_bytes each, dst's geometry).  With S the source
 * value and D the dst value, mode 0 (COPY): D <- S.  mode 1 (ADD, independent evidence): S == -128 leaves D alone, otherwise D <-
 * clamp((D == -128 ? 0 : D) + S, lmin, lmax).  mode 2 (CONFIDENT): D <- the larger of D and S under the total order with key (|L|, L)
 * and -128 below everything — the stronger belief wins, at equal strength the positive (occupied) one; S outside [lmin, lmax] is
 * clamped first.  CONFIDENT is a lattice join: commutative, associative, idempotent — any merge order and any repetition gives the
 * same bytes.  ADD is commutative, and a map merged twice counts twice.  -127 <= lmin <= threshold < lmax <= 127.  For every dst
 * brick the call writes — every brick in COPY; in ADD and CONFIDENT those with a source value other than -128 inside dst's dims — the
 * words of occupied_out and free_out are rewritten from the new values exactly as tohip_evid_fold derives them (L > threshold; L !=
 * -128 and L <= threshold; pad bits 0): handed the planes that were exact before the call, they are exact everywhere after it.
 * counts (DEVICE uint64 x 4, may be NULL, zero-filled by the caller), tohip_evid_fold's: += values that changed, += voxels newly known,
 * += occupied bits that appeared, += occupied bits that vanished; COPY does not read dst and counts against an empty one (values
 * known afterwards, twice; occupied bits afterwards; 0).  src, dst, occupied_out, free_out and counts must be five different buffers.
 * Both: an argument error is TOHIP_EINVAL, a buffer too small for its geometry TOHIP_ENOSPC; every argument check returns before
 * anything is enqueued; nothing synchronises with the host; integers only — the same bytes in every run and for every launch shape. */
int tohip_occ_transfer(const void *src, size_t src_bytes, const tohip_occ_geom *src_geom, void *dst, size_t dst_bytes,
                       const tohip_occ_geom *dst_geom, int32_t sx, int32_t sy, int32_t sz, int32_t mode, uint64_t *counts, void *stream);
int tohip_evid_transfer(const void *src, size_t src_bytes, const tohip_occ_geom *src_geom, void *dst, size_t dst_bytes,
                        const tohip_occ_geom *dst_geom, void *occupied_out, void *free_out, size_t grid_bytes, int32_t sx, int32_t sy,
                        int32_t sz, int32_t mode, int32_t lmin, int32_t lmax, int32_t threshold, uint64_t *counts, void *stream);

/* ---- resampling maps (resample_kernels.hip, DESIGN.md §10, "Resampling maps") ----
 * The transfers above with a rigid transform and a finer or equal resolution between the two boxes.  affine_host: twelve int64 in HOST
 * memory, read before the call returns — M (3 x 3, row major), then T (3) — in fixed point with frac_bits = TOHIP_RESAMPLE_FRAC_BITS
 * fraction bits; |M| <= 2^21, |T| <= 2^40.  For every voxel d = (i, j, k) inside dst's dims, in int64,
 *     u_a = M[a][0] (2 i + 1) + M[a][1] (2 j + 1) + M[a][2] (2 k + 1) + T[a],     n_a = u_a >> frac_bits  (arithmetic: the floor),
 * u / 2^frac_bits being the source position of d's centre in source voxels (voxel i spans [i, i + 1)) and n its NEAREST source voxel.
 * Origins and resolutions of the two geometries are checked as everywhere and not interpreted: the caller quantises the transform.
 * The SOURCE VALUE S of d is, by rule:
 *   TOHIP_RESAMPLE_NEAREST  the value (bit) of source voxel n; EMPTY (-128, bit 0) where n lies outside src's dims.
 *   TOHIP_RESAMPLE_COVER    (evidence) over the 3 x 3 x 3 source voxels around n: the largest value above `threshold` if there is
 *                           one; otherwise -128 if one of the 27 is -128 or lies outside src's dims; otherwise the largest value —
 *                           the maximum under the key free < unknown < occupied.
 *   TOHIP_RESAMPLE_ANY      (planes) the OR of the 27 bits;  TOHIP_RESAMPLE_ALL: their AND, a voxel outside src's dims counting 0.
 * While dst's resolution is not coarser than src's, every point of a dst voxel lies in one of the 27: COVER / ANY lose no occupied
 * voxel, and COVER / ALL call nothing free that touches a voxel that is not.  NEAREST is unbiased and may open pinholes in a wall one
 * voxel thick.  S is then written or combined exactly as the transfers do it: tohip_occ_resample with mode COPY (0) / OR (1) and one
 * count; tohip_evid_resample with mode COPY (0) / ADD (1) / CONFIDENT (2), the two derived planes, the pads, the headers, the rule
 * that in ADD and CONFIDENT a brick with no S other than -128 inside dst's dims is neither read nor written, and the four counts —
 * all as documented for tohip_evid_transfer; `threshold` also classifies the source values under COVER.  scratch / scratch_bytes:
 * room for an implementation with a pre-pass; this one takes COVER's 27 values in place and neither reads nor writes it (NULL, 0 are
 * fine).  src is only read.  flags is reserved and must be 0.  src, dst, the planes, counts and a scratch that is given must be
 * different buffers.  A bad rule, mode, frac_bits, affine entry or flags, a null affine_host, an aliased buffer: TOHIP_EINVAL; a
 * short buffer: TOHIP_ENOSPC.  Every argument check returns before anything is enqueued; nothing synchronises with the host;
 * integers only, one lane owns a dst word or brick: the same bytes in every run and for every launch shape. */
#define TOHIP_RESAMPLE_FRAC_BITS 20
#define TOHIP_RESAMPLE_NEAREST 0
#define TOHIP_RESAMPLE_COVER 1
#define TOHIP_RESAMPLE_ANY 1
#define TOHIP_RESAMPLE_ALL 2
int tohip_occ_resample(const void *src, size_t src_bytes, const tohip_occ_geom *src_geom, void *dst, size_t dst_bytes,
                       const tohip_occ_geom *dst_geom, const int64_t *affine_host, int32_t frac_bits, int32_t rule, int32_t mode,
                       uint64_t *counts, void *stream, uint32_t flags);
int tohip_evid_resample(const void *src, size_t src_bytes, const tohip_occ_geom *src_geom, void *dst, size_t dst_bytes,
                        const tohip_occ_geom *dst_geom, void *occupied_out, void *free_out, size_t grid_bytes,
                        const int64_t *affine_host, int32_t frac_bits, int32_t rule, int32_t mode, int32_t lmin, int32_t lmax,
                        int32_t threshold, uint64_t *counts, void *scratch, size_t scratch_bytes, void *stream, uint32_t flags);

/* ---- coarsening maps (coarsen_kernels.hip, DESIGN.md §10, "Coarsening maps") ----
 * The transfers above across an integer change of scale: f x f x f source voxels reduced to one dst voxel.  src and dst are two
 * DIFFERENT buffers, each with its own geometry.  factor f in [2, TOHIP_COARSEN_MAX_FACTOR], the same on all axes; (ox, oy, oz) an
 * integer offset, each component in [-2^20, 2^20].  The CHILDREN of dst voxel d are the f^3 source voxels f d + o + e, e in [0, f)^3;
 * a child outside src's dims is EMPTY: -128, bit 0.  Origins and resolutions of the two geometries are checked as everywhere and not
 * interpreted: the caller computes o and checks r_d = f r_s.  The SOURCE VALUE S of d is, by rule:
 *   TOHIP_COARSEN_COVER  (evidence) the maximum of the children under the key free < unknown < occupied, TOHIP_RESAMPLE_COVER's: the
 *                        largest value above `threshold` if there is one; otherwise -128 if a child is -128 or outside; otherwise the
 *                        largest (least free) value.  Conservative for planning: an occupied child makes d occupied, and d is free
 *                        only where all f^3 children lie inside src's dims and are free.
 *   TOHIP_COARSEN_MAX    (evidence) the largest child as a signed byte, -128 only where every child is EMPTY: occupied if any child
 *                        is, and optimistic about the unknown — for display, occlusion and matching, not for collision checks.
 *   TOHIP_COARSEN_ANY    (planes) the OR of the child bits;  TOHIP_COARSEN_ALL: their AND, a child outside src's dims counting 0.
 * veto_or_null (tohip_occ_coarsen, rule ANY only; TOHIP_EINVAL with ALL): a plane of src's geometry and size; with it
 * S = ANY(src) & ~ANY(veto) — the free plane of a three-state map under MAX, vetoed by its occupied plane.  Both keys are total orders
 * on the byte, so the maximum is associative and commutative: factor f1 then f2 equals factor f1 f2 once (offset o1 + f1 o2), and any
 * split of the work gives the same bytes.  S is then written or combined exactly as the transfers do it: tohip_occ_coarsen with mode
 * COPY (0) / OR (1) and one count; tohip_evid_coarsen with mode COPY (0) / ADD (1) / CONFIDENT (2), the two derived planes, the pads,
 * the headers, the rule that in ADD and CONFIDENT a brick with no S other than -128 inside dst's dims is neither read nor written,
 * and the four counts — all as documented for tohip_evid_transfer; `threshold` also classifies the children under COVER.  src and the
 * veto are only read.  flags is reserved and must be 0.  src, the veto, dst, the planes and counts must be different buffers.  A bad
 * factor, offset, rule, mode or flags, an aliased buffer: TOHIP_EINVAL; a short buffer: TOHIP_ENOSPC.  Every argument check returns
 * before anything is enqueued; nothing synchronises with the host; integers only, one lane owns a dst word or brick and no atomic
 * touches a plane or a value: the same bytes in every run and for every launch shape. */
#define TOHIP_COARSEN_MAX_FACTOR 8
#define TOHIP_COARSEN_COVER 0
#define TOHIP_COARSEN_MAX 1
#define TOHIP_COARSEN_ANY 0
#define TOHIP_COARSEN_ALL 1
int tohip_occ_coarsen(const void *src, size_t src_bytes, const tohip_occ_geom *src_geom, const void *veto_or_null, void *dst,
                      size_t dst_bytes, const tohip_occ_geom *dst_geom, int32_t factor, int32_t ox, int32_t oy, int32_t oz, int32_t rule,
                      int32_t mode, uint64_t *counts, void *stream, uint32_t flags);
int tohip_evid_coarsen(const void *src, size_t src_bytes, const tohip_occ_geom *src_geom, void *dst, size_t dst_bytes,
                       const tohip_occ_geom *dst_geom, void *occupied_out, void *free_out, size_t grid_bytes, int32_t factor, int32_t ox,
                       int32_t oy, int32_t oz, int32_t rule, int32_t mode, int32_t lmin, int32_t lmax, int32_t threshold, uint64_t *counts,
                       void *stream, uint32_t flags);

/* ---- clearance from the map (clearance_map_kernels.hip, DESIGN.md §10, "Clearance from the map") -------
 * tohip_clearance and tohip_clearance_segments with the voxels of an occupancy grid as the obstacles.  occupied: a grid buffer of
 * grid_bytes; free_or_null: NULL, or the free plane of the same geometry (not `occupied` itself).  An OBSTACLE is a voxel inside
 * dims whose occupied bit is set and, with a free plane, also one of state 0 (neither bit: unknown) — tohip_field_build's rule.  An
 * obstacle IS the point at its centre, fl(origin_a + fl(fl((float)i_a + 0.5f) resolution)) per axis, tohip_occ_export's bits.  d2,
 * the hinge, the term, s and the gradients are the two definitions above applied to those points; ties go to the lowest linear
 * index (z ny + y) nx + x, and idx is that index (-1: no obstacle has d2 < fl(r r), or a query coordinate is not finite).  So over
 * the obstacle centres C in ascending linear index both calls equal tohip_clearance / tohip_clearance_segments over a packed cloud
 * of C bit for bit, idx through C's index.  A query outside dims, in the apron or beyond it, is an ordinary query.  radius > 0,
 * finite, and at most 64 voxels (radius / resolution <= 64: TOHIP_EINVAL beyond); weight >= 0, finite.  The workspaces are
 * tohip_clearance_workspace_bytes(n_queries) and tohip_clearance_segments_workspace_bytes(n_wps, n_traj), with the same contents
 * after the call.  To fill a plan's clearance_scratch (TOHIP_TRAJ_CLEARANCE_PREFILLED) pass grad = clearance_scratch and workspace =
 * clearance_scratch + align256(12 n_traj n_wps), workspace_bytes = the scratch's bytes less that offset: the rows and the terms
 * (and the per-segment parts) land where the step reads them.  One block of 16 waves per query scans only the bricks within the
 * radius of the waypoint or segment; no atomics: the results do not depend on the launch.  Every argument check returns before
 * anything is enqueued; nothing synchronises with the host. */
int tohip_clearance_map(const void *occupied, const void *free_or_null, size_t grid_bytes, const tohip_occ_geom *geom,
                        const float *queries, int64_t n_queries, float radius, float weight, float *d, int32_t *idx, float *value,
                        float *grad, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
int tohip_clearance_map_segments(const void *occupied, const void *free_or_null, size_t grid_bytes, const tohip_occ_geom *geom,
                                 const float *poses, int64_t n_wps, int64_t n_traj, float radius, float weight, float *d, int32_t *idx,
                                 float *s, float *value, float *grad, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the unknown volume a view would reveal (volume_kernels.hip, DESIGN.md §10, "Unknown volume") -------
 * How much unknown space would a camera see from here?  occupied and free_grid are the two planes of a map (one geometry, grid_bytes
 * each); claimed and mark, where given, are two more grids of that geometry.
 *
 * tohip_occ_unknown: out (a third buffer, not one of the two) receives the mask of the voxels inside dims of state 0 (neither bit);
 * its header and pad bits 0.  tohip_occ_count / tohip_occ_export list it.
 *
 * tohip_view_volume: view w is the pose poses + 3 w, quats + 4 w (wxyz, normalised as tohip_los_rows does, normalize = 1).  A voxel v
 * inside dims is REVEALED by view w iff (1) its state is 0 and, where claimed is given, its bit there is 0; (2) its centre c =
 * fl(origin + fl(fl(i + 0.5) r)) per axis — tohip_occ_export's bits — is kept by tohip_cull_waypoints(normalize = 1) with this camera
 * and these limits (the same device functions: the same bit); (3) tohip_los_segments(occupied, poses[w] -> c, start_skip 1, end_skip 0)
 * gives 1: only occupied voxels block, the camera's own voxel and v itself are not tested, unknown voxels on the way do not block, and
 * a view whose position is out of range reveals nothing.  gains[w] (DEVICE int64 x n_views, overwritten) = the number of revealed
 * voxels: an exact integer, the same in every run.  mark (may be NULL): the revealed voxels of every view scored get their bit there
 * (32-bit integer atomic OR, issued only where a brick's word lacks one of the gathered bits); bits are only ever set.  mark ==
 * claimed (claim what is counted, in one launch) is allowed only where the call scores ONE view — each word is then read and written by
 * one lane — and is TOHIP_EINVAL otherwise.  1 <= n_views <= 65535.
 * view_index (DEVICE int32, may be NULL): the call scores the one view whose number is stored there when the kernel runs — a number
 * another kernel wrote, tohip_view_volume_pick's order + j — out of the n_views rows: gains[*view_index] receives its count, every
 * other entry 0; a number outside [0, n_views) scores nothing.
 * window != 0: per view only the bricks of a box are enumerated that holds every voxel the cull can keep — the camera and the far
 * ends of the four corner rays of the pixel rectangle widened by a pixel, padded by two voxels, clipped to dims, computed on the
 * device — and inside it a brick whose bounding sphere cannot pass the depth gate is not tested.  The window never changes a count
 * or a bit; 0 enumerates every brick.  (It needs K = (fx s cx; 0 fy cy; 0 0 1) with fx, fy > 0: with any other K every brick is
 * enumerated.)
 * stop (DEVICE int32, may be NULL): the launch does nothing — gains all 0, mark untouched — where the word is not 0 when it runs.
 * stats (DEVICE uint64 x 3, may be NULL, zero-filled by the caller): += centres tested, += rays walked, += voxels visited.
 *
 * tohip_view_volume_pick: round `round` (>= 0) of a greedy selection over gains (n_views int64).  Among the candidates c with
 * taken[c] == 0 (DEVICE int32 x n_views) the largest gain wins, ties to the lowest index.  Where that gain is >= min_gain (>= 1):
 * order[round] = c (int32), picked_gain[round] = the gain (int64), taken[c] = 1.  Otherwise — also where no candidate is left —
 * *stop = 1 and nothing else is written.  Where *stop is not 0 when the launch runs it does nothing.  So k rounds of (tohip_view_volume
 * with claimed = R, tohip_view_volume_pick, tohip_view_volume with claimed = mark = R and view_index = order + round), all with one
 * stop word, choose up to k views greedily with nothing read back; the caller pre-fills order with -1.
 * Every argument check returns before anything is enqueued; nothing synchronises with the host. */
int tohip_occ_unknown(const void *occupied, const void *free_grid, void *out, size_t grid_bytes, const tohip_occ_geom *geom, void *stream);
int tohip_view_volume(const void *occupied, const void *free_grid, const void *claimed, void *mark, size_t grid_bytes,
                      const tohip_occ_geom *geom, const float *poses, const float *quats, int64_t n_views, const int32_t *view_index,
                      const tohip_camera *cam, float min_dist, float max_dist, int32_t window, int64_t *gains, const int32_t *stop,
                      uint64_t *stats, void *stream);
int tohip_view_volume_pick(const int64_t *gains, int32_t *taken, int64_t n_views, int64_t min_gain, int32_t round, int32_t *order,
                           int64_t *picked_gain, int32_t *stop, void *stream);

/* ---- information gain (volume_kernels.hip, DESIGN.md §10, "Information gain") -------
 * How much is left to learn about what a camera would see from here?  evidence is an evidence buffer of the geometry (evid_bytes,
 * tohip_evid_bytes); table W is 256 unsigned 16-bit weights in DEVICE memory, indexed by the evidence byte read as unsigned, L + 128:
 * W[0] weighs a voxel never observed.  A voxel v inside dims is a CANDIDATE of the map under W iff W[byte(v)] > 0, whatever its state;
 * pad voxels are never candidates.
 *
 * tohip_evid_weight_plane: plane_out (an occupancy grid buffer of the geometry, grid_bytes, not the evidence buffer) receives the
 * candidate mask — its header zero as tohip_occ_init leaves it, pad bits 0 — and *total_out (DEVICE int64, may be NULL, zero-filled by
 * the caller) += the sum of W[byte(v)] over the voxels inside dims: the map's remaining information under W (one 64-bit integer
 * atomic add per block).  One launch, nothing read back.  Prepared once, the plane serves every tohip_view_information launch until
 * the evidence or the table changes.
 *
 * tohip_view_information: tohip_view_volume's arguments and meaning — view w, claimed, mark, view_index, window, stop, stats,
 * n_views in [1, 65535], mark == claimed only where ONE view is scored — with `candidates` (tohip_evid_weight_plane's plane for this
 * evidence and table) standing where the unknown voxels stood.  A candidate whose claimed bit is 0 is INFORMED by view w under
 * tohip_view_volume's conditions (2) and (3), unchanged: its centre is kept by the cull, and tohip_los_segments(occupied, poses[w] ->
 * centre, start_skip 1, end_skip 0) gives 1 — the target voxel itself is not tested, so a weakly occupied surface voxel can be
 * informed; unknown voxels on the way do not block.  gains[w] (DEVICE int64 x n_views, overwritten) = the sum of W[byte(v)] over the
 * informed voxels: an exact integer, the same in every run.  mark receives the informed voxels.  free_grid is not read; candidates
 * must be none of occupied, free_grid, mark and evidence.  With W[0] = 1 and every other weight 0 on a map whose planes are the
 * evidence's, the gains and the mark plane are tohip_view_volume's.  tohip_view_volume_pick and tohip_view_volume_pick_travel choose
 * among these gains as they are; the travel pick forms gain 2^20 - m cost, so a caller keeps 65535 x voxels x 2^20 below 2^63.
 * flags is reserved (0).  Every argument check returns before anything is enqueued; nothing synchronises with the host. */
int tohip_evid_weight_plane(const void *evidence, size_t evid_bytes, const tohip_occ_geom *geom, const uint16_t *table, void *plane_out,
                            size_t grid_bytes, int64_t *total_out, void *stream, uint32_t flags);
int tohip_view_information(const void *occupied, const void *free_grid, const void *claimed, void *mark, size_t grid_bytes,
                           const tohip_occ_geom *geom, const void *evidence, size_t evid_bytes, const uint16_t *table,
                           const void *candidates, const float *poses, const float *quats, int64_t n_views, const int32_t *view_index,
                           const tohip_camera *cam, float min_dist, float max_dist, int32_t window, int64_t *gains, const int32_t *stop,
                           uint64_t *stats, void *stream, uint32_t flags);

/* ---- ray casts and depth scans (raycast_kernels.hip, DESIGN.md §10, "Ray casts and depth scans") -------
 * Where does this ray stop?  Both entries walk exactly as tohip_los_segments walks (same steps, same tie rule, same tests).
 *
 * The CAST of a segment A -> B (the fixed-point forms of a and b, both in range) with (start_skip, end_skip): the HIT is the first
 * visited voxel that tohip_los_segments would call occupied — cheb(v, v0) >= start_skip and cheb(v, e) > end_skip, inside dims, bit
 * set; with end_skip = 0 the end voxel itself is never tested.  Its ENTRY PARAMETER is the crossing parameter n_a / m_a of the last
 * step the walk took before it stood on the hit (n the distance to the face in 1/256 voxel before the step adds 256, m = |B - A| on
 * that axis), the exact rational 0/1 when no step was taken; it equals the maximum over the axes with k_a > 0 steps taken of
 * (n_a0 + 256 (k_a - 1)) / m_a, compared by integer cross-multiplication.  lam = fl(f32(num) / f32(den)): num and den are exact in
 * f32 and the division is correctly rounded, so equal rationals give equal bits.
 *
 * tohip_cast_segments: a, b (n_rays, 3) f32 world points on the device -> voxel (n_rays) int32: the hit's linear index i + nx (j + ny
 * k), -1 clear, -2 an endpoint out of range; lam (n_rays) f32: the hit's entry parameter, 1.0 clear, NaN out of range.  voxel == -1
 * iff tohip_los_segments gives 1 and voxel == -2 iff it gives 2, with the same skips (each in [0, 8192]).  stats (DEVICE uint64 x 2,
 * may be NULL, zero-filled by the caller): += rays walked, += voxels visited.
 *
 * tohip_depth_scan: view w is the pose poses + 3 w, quats + 4 w (wxyz, normalised as tohip_los_rows does, normalize = 1).  cam: K =
 * (fx 0 cx; 0 fy cy; 0 0 1) with fx, fy > 0, everything finite, W = img_width and H = img_height integral values in [1, 8192]; 1 <=
 * n_views <= 65535 and n_views H W < 2^31; 0 <= min_dist < max_dist, both finite; TOHIP_EINVAL otherwise (cam's own min_dist,
 * max_dist and eps are not read).  Pixel (x, y) is column x of row y; all arithmetic is f32, every operation rounded, no fma:
 * dc = (fl(fl(x - cx) / fx), fl(fl(y - cy) / fy), 1); the far point in the camera frame Fc = (fl(dc.x D), fl(dc.y D), D) with D =
 * max_dist (the range is a z-depth, as in the cull); in the world B = fl(rot(q, Fc) + t) per axis, rot being tohip_to_camera_frame's two
 * Hamilton products with the roles of q and its conjugate exchanged and the same order of terms.  The ray is the cast t -> B with skips
 * (1, 0): the camera's own voxel and B's voxel are not tested.  depth = fl(lam D).  Outputs, each indexed [w][y][x]:
 *   voxel (int32)  the hit's linear index, -1 no hit, -2 skipped;
 *   depth (f32)    fl(lam D) of a hit, +inf without one, NaN skipped;
 *   flags (uint8)  0 a return; 1 no return within D; 2 skipped (t or B out of range); 3 a hit nearer than the sensor's minimum,
 *                  !(depth > min_dist): the ray is blocked and reports no point (voxel and depth still name what blocked it);
 *   points (f32 x 3, may be NULL)  flag 0: the hit voxel's centre fl(origin + fl(fl(i + 0.5) r)), tohip_occ_export's bits; flag 1:
 *                  B; flags 2 and 3: NaN.
 * hit_plane and pass_plane (each may be NULL): grids of the scanned grid's geometry (grid_bytes each), neither the scanned grid nor
 * each other (TOHIP_EINVAL).  hit_plane gets the bit of every flag-0 hit voxel; pass_plane the bit of every voxel inside dims that a
 * ray of flag 0 or 1 visited before its hit — the camera's voxel and every tested, clear voxel; never the hit voxel, never B's voxel.
 * A flag-3 ray marks nothing.  Bits are only ever set (32-bit integer atomic OR, issued only where a word lacks a bit).
 * stats (DEVICE uint64 x 3, may be NULL, zero-filled by the caller): += rays walked, += voxels visited, += plane atomics issued.
 * Every argument check returns before anything is enqueued; nothing synchronises with the host. */
int tohip_cast_segments(const void *grid, size_t grid_bytes, const tohip_occ_geom *geom, const float *a, const float *b, int64_t n_rays,
                        int32_t start_skip, int32_t end_skip, int32_t *voxel, float *lam, uint64_t *stats, void *stream);
int tohip_depth_scan(const void *grid, size_t grid_bytes, const tohip_occ_geom *geom, const float *poses, const float *quats,
                     int64_t n_views, const tohip_camera *cam, float min_dist, float max_dist, void *hit_plane, void *pass_plane,
                     int32_t *voxel, float *depth, uint8_t *flags, float *points, uint64_t *stats, void *stream);

/* ---- the travel field (travel_kernels.hip, DESIGN.md §10, "Travel field") ------------------------------
 * Can the robot get there, and how far is it?  A one-to-all shortest-path field over the voxels a clearance field certifies.
 *
 * TRAVERSABLE set T: the voxels inside dims with field >= need2 (1 <= need2 <= 65535; the sentinel counts) and — where the two planes
 * of a map are given (both or neither, grid_bytes each) — of state 1: tohip_field_nodes' mask at stride 1.  A MOVE goes from v to a
 * voxel u at Chebyshev distance 1 (26 neighbours) and is allowed iff every voxel w with min(v, u) <= w <= max(v, u) per axis (2, 4 or
 * 8 voxels) is in T: no corner is cut, and the straight leg between the two centres stays inside certified cubes.  Weights, in 1/64
 * voxel edge: 64 (face), 91 (edge), 111 (corner).  sources (n_sources >= 1 rows of 3 f32 on the device): a source is SEEDED at cost 0
 * iff its position is in range, its voxel lies inside dims and in T; any other is ignored — no snapping — and seeded (DEVICE uint8 x
 * n_sources, may be NULL) tells which.  cost[v] = the length of the shortest allowed path from any seeded source to v where that is
 * <= limit (0 <= limit <= 2^31 - 1: no sum overflows 32 bits), else 0xFFFFFFFF; every stored value is the exact untruncated distance.
 * Layout: one uint32 per voxel inside dims, dense, x fastest, index (z ny + y) nx + x: tohip_travel_bytes(nx, ny, nz) = 4 nx ny nz
 * device bytes (0 for bad dims), caller-owned.  The answer is the unique fixed point of cost[s] = 0, cost[v] = min over the allowed u
 * of cost[u] + w(u, v): it does not depend on the order of the relaxation — the same bits in every run.
 *
 * tohip_travel_build: fills cost and relaxes it over a worklist of 8 x 8 x 8-voxel tiles in workspace
 * (tohip_travel_workspace_bytes device bytes, 256-byte aligned), two launches per round.  It enqueues rounds_per_check rounds (1 ..
 * 65536), SYNCHRONISES to read one word back — "did the last round have a tile to work on" — and repeats until it had none; rounds
 * after convergence do nothing.  *rounds_host (HOST, may be NULL): the rounds that had work.  cost, workspace and the inputs must all
 * differ.
 * tohip_travel_positions: positions (m, 3) f32 -> cost_out (m) int64: the voxel's cost, -1 unreachable, -2 out of range or outside
 * dims — and / or dist (m) f32 metres fl(fl((float) cost (1/64)) r), +inf for -1, NaN for -2; either may be NULL, not both.
 * tohip_travel_paths: goal e (n_goals rows of 3 f32) -> rows + 3 max_rows e: the voxel centres fl(origin + fl(fl(i + 0.5) r)) from the
 * goal's voxel to a source, and counts[e] (int64) their number; 0 for a goal that is unreachable, out of range or outside dims;
 * -needed where the path has more than max_rows rows (the first max_rows are written).  PATH RULE: the predecessor of a reachable
 * voxel v with cost[v] > 0 is the allowed neighbour u with cost[u] + w(u, v) == cost[v], the lowest move number (dz + 1) 9 + (dy + 1)
 * 3 + (dx + 1) on ties; one exists in every built field.  field, the planes and need2 are the build's.  One launch.
 * tohip_view_volume_pick_travel: tohip_view_volume_pick with a cost row (int64 x n_views: tohip_travel_positions' codes) and a weight
 * 0 <= m < 2^31.  The candidates are those with taken == 0, gain >= min_gain and cost >= 0; gain 2^20 - m cost (int64) decides, ties
 * to the lowest index; picked_gain[round] = the winner's gain.  *stop = 1 where no candidate is left.
 * Every argument check returns before anything is enqueued. */
size_t tohip_travel_bytes(int32_t nx, int32_t ny, int32_t nz);
size_t tohip_travel_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int tohip_travel_build(const void *field, size_t field_bytes, const void *occupied_or_null, const void *free_or_null, size_t grid_bytes,
                       const tohip_occ_geom *geom, int32_t need2, const float *sources, int64_t n_sources, int64_t limit,
                       int32_t rounds_per_check, void *cost, size_t cost_bytes, void *workspace, size_t workspace_bytes, uint8_t *seeded,
                       int64_t *rounds_host, void *stream);
int tohip_travel_positions(const void *cost, size_t cost_bytes, const tohip_occ_geom *geom, const float *positions, int64_t m,
                           int64_t *cost_out, float *dist, void *stream);
int tohip_travel_paths(const void *cost, size_t cost_bytes, const void *field, size_t field_bytes, const void *occupied_or_null,
                       const void *free_or_null, size_t grid_bytes, const tohip_occ_geom *geom, int32_t need2, const float *goals,
                       int64_t n_goals, int64_t max_rows, float *rows, int64_t *counts, void *stream);
int tohip_view_volume_pick_travel(const int64_t *gains, const int64_t *cost, int64_t weight, int32_t *taken, int64_t n_views,
                                  int64_t min_gain, int32_t round, int32_t *order, int64_t *picked_gain, int32_t *stop, void *stream);

/* ---- travel fields in batches (travel_kernels.hip, DESIGN.md §10, "Travel fields in batches") --------------
 * Many-to-all: n_fields (1 .. TOHIP_TRAVEL_MAX_FIELDS) travel fields over ONE traversable set T, built in the same worklist rounds.
 * T, the move rule, the weights, limit and the sentinel are tohip_travel_build's.  cost holds the fields one after the other, each
 * in the single field's layout: field b starts at word b nx ny nz (64-bit indices), tohip_travel_batch_bytes = n_fields 4 nx ny nz
 * (0 for bad dims or a bad n_fields).  source_field (DEVICE int32 x n_sources): source i seeds field source_field[i]; it is seeded
 * iff 0 <= source_field[i] < n_fields and tohip_travel_build's seeding rule holds, else it is ignored and seeded[i] = 0.  A field
 * may have several sources or none (it stays all sentinel).  Field b is bit for bit what tohip_travel_build writes from the sources
 * that name b: each field is the same unique fixed point, and fields share no cost word.
 * One worklist: a work item is (field, tile), packed b n_tiles + t in the bitmaps and the list — n_fields n_tiles must fit 31 bits
 * (TOHIP_EINVAL; tohip_travel_batch_workspace_bytes is 0 then).  A round is two launches for all fields together, one status word
 * comes back per rounds_per_check rounds, *rounds_host = the rounds that had work.  A cost_bytes or workspace_bytes too small is
 * TOHIP_EINVAL.
 * tohip_travel_positions_batch: cost_out (n_fields, m) int64 and / or dist (n_fields, m) f32: row b is tohip_travel_positions on
 * field b.  One launch.
 * tohip_travel_paths_batch: tohip_travel_paths with goal_field (DEVICE int32 x n_goals), the field goal e is walked in; one out of
 * [0, n_fields) gives counts[e] = 0.  One launch.
 * tohip_assign_greedy: cost (n_rows, ld >= n_cols) int64 on the device, 1 <= n_rows <= 64, 1 <= n_cols <= 4096, min_cost >= 0.  A pair
 * (r, c) is a candidate iff cost[r][c] >= min_cost (negative entries: none).  Starting with nothing assigned, the candidate with the
 * smallest key (cost, r, c) among those whose row is unassigned and whose column is unclaimed is assigned, until none is left.
 * col_of_row (n_rows) and row_of_col (n_cols): int32, -1 where nothing was assigned.  One launch of one block, integers only.
 * Every argument check returns before anything is enqueued. */
#define TOHIP_TRAVEL_MAX_FIELDS 256
size_t tohip_travel_batch_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t n_fields);
size_t tohip_travel_batch_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t n_fields);
int tohip_travel_build_batch(const void *field, size_t field_bytes, const void *occupied_or_null, const void *free_or_null,
                             size_t grid_bytes, const tohip_occ_geom *geom, int32_t need2, const float *sources,
                             const int32_t *source_field, int64_t n_sources, int32_t n_fields, int64_t limit, int32_t rounds_per_check,
                             void *cost, size_t cost_bytes, void *workspace, size_t workspace_bytes, uint8_t *seeded,
                             int64_t *rounds_host, void *stream);
int tohip_travel_positions_batch(const void *cost, size_t cost_bytes, const tohip_occ_geom *geom, int32_t n_fields,
                                 const float *positions, int64_t m, int64_t *cost_out, float *dist, void *stream);
int tohip_travel_paths_batch(const void *cost, size_t cost_bytes, const void *field, size_t field_bytes, const void *occupied_or_null,
                             const void *free_or_null, size_t grid_bytes, const tohip_occ_geom *geom, int32_t need2, int32_t n_fields,
                             const float *goals, const int32_t *goal_field, int64_t n_goals, int64_t max_rows, float *rows,
                             int64_t *counts, void *stream);
int tohip_assign_greedy(const int64_t *cost, int32_t n_rows, int32_t n_cols, int64_t ld, int64_t min_cost, int32_t *col_of_row,
                        int32_t *row_of_col, void *stream);

/* ---- weighted travel fields (travel_kernels.hip, DESIGN.md §10, "Weighted travel fields") ------------------
 * A travel field that minimises WEIGHTED length.  weights: a layer kappa of one uint8 per voxel inside dims, dense, x fastest, the
 * cost words' index (z ny + y) nx + x: tohip_travel_weights_bytes(nx, ny, nz) = nx ny nz device bytes (0 for bad dims), caller-owned.
 * 16 <= kappa <= 255; 16 is neutral, 255 costs about 15.9 times as much.  The bytes are the caller's contract: no entry reads them on
 * the host, and a byte below 16 is a discount the fixed-point argument does not cover.  The move m between v and u, of weight w_m in
 * {64, 91, 111}, costs
 *     step(v, u, m) = (w_m (kappa[v] + kappa[u]) + 16) >> 5,
 * symmetric in v and u, an integer, at least w_m, exactly w_m at kappa = 16 and at most (111 x 510 + 16) >> 5 = 1769.  T, the move
 * rule (no corner cut; only the move's two endpoints are priced, not the other voxels of its box), the seeds, limit and the sentinel
 * are tohip_travel_build's; cost is the unique fixed point of cost[s] = 0, cost[v] = min over the allowed u of cost[u] + step — the
 * same bits in every run.  Because step >= w_m a path's geometric length never exceeds its cost: a limit still bounds the length, and
 * a path of cost c still has at most c / 64 moves.  At kappa = 16 everywhere every entry below writes tohip_travel_build_batch's and
 * tohip_travel_paths_batch's bytes.
 *
 * tohip_travel_weights_build: out[v] = lut[min(field[v], n_lut - 1)] for every voxel inside dims — field: a clearance field
 * (tohip_field_build), whose value is the squared gap in voxels; lut: n_lut >= 1 (at most 65536) DEVICE bytes.  With the two planes of
 * a map (both or neither, grid_bytes each) unknown_add (0 .. 255) is added at the voxels that are neither occupied nor known free, and
 * the sum saturates at 255.  out: out_bytes >= tohip_travel_weights_bytes (TOHIP_ENOSPC), sharing no byte with the inputs.  One launch.
 * tohip_travel_build_weighted: tohip_travel_build_batch (n_fields = 1 and source_field all 0: the single field) with the layer, which
 * all fields share: weights_bytes >= tohip_travel_weights_bytes, and the layer shares no byte with cost or workspace (TOHIP_EINVAL).
 * tohip_travel_paths_weighted: tohip_travel_paths_batch with the path rule's test cost[u] + step(v, u, m) == cost[v]; the lowest move
 * number still wins ties.
 * flags behind the stream is reserved: 0, anything else TOHIP_EINVAL.  Every argument check returns before anything is enqueued. */
size_t tohip_travel_weights_bytes(int32_t nx, int32_t ny, int32_t nz);
int tohip_travel_weights_build(const void *field, size_t field_bytes, const void *occupied_or_null, const void *free_or_null,
                               size_t grid_bytes, const tohip_occ_geom *geom, const uint8_t *lut, int32_t n_lut, int32_t unknown_add,
                               uint8_t *out, size_t out_bytes, void *stream, uint32_t flags);
int tohip_travel_build_weighted(const void *field, size_t field_bytes, const void *occupied_or_null, const void *free_or_null,
                                size_t grid_bytes, const tohip_occ_geom *geom, int32_t need2, const float *sources,
                                const int32_t *source_field, int64_t n_sources, int32_t n_fields, int64_t limit,
                                int32_t rounds_per_check, void *cost, size_t cost_bytes, void *workspace, size_t workspace_bytes,
                                uint8_t *seeded, int64_t *rounds_host, const uint8_t *weights, size_t weights_bytes, void *stream,
                                uint32_t flags);
int tohip_travel_paths_weighted(const void *cost, size_t cost_bytes, const void *field, size_t field_bytes, const void *occupied_or_null,
                                const void *free_or_null, size_t grid_bytes, const tohip_occ_geom *geom, int32_t need2, int32_t n_fields,
                                const float *goals, const int32_t *goal_field, int64_t n_goals, int64_t max_rows, float *rows,
                                int64_t *counts, const uint8_t *weights, size_t weights_bytes, void *stream, uint32_t flags);

/* ---- connected components (components_kernels.hip, DESIGN.md §10, "Connected components") ----------------
 * Which voxels belong together?  plane: any bit plane of the occupancy layout (grid_bytes; header and pad bits 0, as every producer
 * here leaves them).  Two set voxels inside dims are ADJACENT iff they differ by at most 1 on every axis and by 1 (connectivity 6),
 * <= 2 (18) or <= 3 (26) axes; there is no corner-cut rule.  A component's ROOT is its lowest linear index v = (z ny + y) nx + x; ids
 * are 0 .. C - 1 in ascending order of the root.  labels: one uint32 per voxel inside dims, dense, x fastest —
 * tohip_components_bytes(nx, ny, nz) = 4 nx ny nz device bytes (0 for bad dims), caller-owned, 4-byte aligned: after the build every
 * set voxel holds its component's id, every clear voxel 0xFFFFFFFF.  The result is a function of the plane and the connectivity
 * alone — the unique fixed point of label[v] = min(v, label[u] over the adjacent u), ranked: the same bits in every run.
 *
 * tohip_components_build: writes label[v] = v and relaxes it over a worklist of 8 x 8 x 8-voxel tiles in workspace
 * (tohip_components_workspace_bytes device bytes, 256-byte aligned), two launches per round; it enqueues rounds_per_check rounds
 * (1 .. 1000), SYNCHRONISES to read one word back and repeats until a round had no tile to work on (*rounds_host, HOST, may be NULL:
 * the rounds that had work).  Then the roots are counted and C is read back into *n_components_host (HOST, required).  C <=
 * roots_capacity: roots[0 .. C) (DEVICE int32) receives the roots in ascending order and the labels become ids.  C > roots_capacity:
 * TOHIP_ENOSPC with C reported, roots untouched and the labels left as root indices; the caller sizes roots beforehand — C never
 * exceeds the plane's set bits (tohip_occ_count) — or builds again.  roots may be NULL with roots_capacity 0.  Bad connectivity,
 * dims or rounds_per_check, a misaligned or aliased buffer: TOHIP_EINVAL; a short one: TOHIP_ENOSPC.
 * tohip_components_stats: one pass over labels (built: ids) -> per component sizes (n_components) int64, sums (n_components, 3)
 * int64 of i, j, k, bbox (n_components, 2, 3) int32 minimum and maximum per axis; integer atomics.  A word that is not an id below
 * n_components counts for nothing.  The centroid of a component is origin + (sum / size + 0.5) resolution.
 * tohip_components_min: values (values_bytes >= 4 nx ny nz, uint32 per voxel in labels' layout, 0xFFFFFFFF = none: a travel field's
 * cost) -> min_value (n_components) int64, the smallest value over the component's voxels, and min_voxel (n_components) int32, the
 * lowest linear index that attains it; -1 / -1 where every voxel holds 0xFFFFFFFF.  Integer atomic minima, two passes.
 * tohip_components_positions: positions (m, 3) f32 -> out (m) int64: the voxel's id, -1 clear, -2 out of range or outside dims
 * (tohip_travel_positions' convention and coordinate rule).
 * Every argument check returns before anything is enqueued. */
size_t tohip_components_bytes(int32_t nx, int32_t ny, int32_t nz);
size_t tohip_components_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int tohip_components_build(const void *plane, size_t grid_bytes, const tohip_occ_geom *geom, int32_t connectivity, void *labels,
                           size_t labels_bytes, void *workspace, size_t workspace_bytes, int32_t rounds_per_check, int32_t *roots,
                           int64_t roots_capacity, int64_t *n_components_host, int64_t *rounds_host, void *stream);
int tohip_components_stats(const void *labels, size_t labels_bytes, const tohip_occ_geom *geom, int64_t n_components, int64_t *sizes,
                           int64_t *sums, int32_t *bbox, void *stream);
int tohip_components_min(const void *labels, size_t labels_bytes, const tohip_occ_geom *geom, const void *values, size_t values_bytes,
                         int64_t n_components, int64_t *min_value, int32_t *min_voxel, void *stream);
int tohip_components_positions(const void *labels, size_t labels_bytes, const tohip_occ_geom *geom, const float *positions, int64_t m,
                               int64_t *out, void *stream);

/* ---- the ground layer ("Ground layer") ------------------------------------------------
 * For a robot that drives on the map's floor: headroom H voxels (1 .. 64) and step s voxels (0 .. 4, s + 1 <= H).  A voxel is CLEAR
 * iff it is not occupied and — with unknown_obstacle = 1, which needs the free plane — known free; a voxel outside dims is clear with
 * unknown_obstacle = 0 and not clear with 1.  All planes are occupancy grid buffers of grid_bytes and one geometry.
 * tohip_ground_build writes four planes (none of them an input or one another; headers and pad bits 0):
 *   support    occupied, and the voxels at z + 1 .. z + H clear.
 *   ground     the support voxels all eight of whose lateral neighbour columns lie inside dims and hold (a) a support voxel at a
 *              level in [z - s, z + s] or (b) an occupied voxel at a level in [z + 1, z + H] (a wall: its own obstacle).  Ledge and pit
 *              rims, risers higher than s, the rim of unseen floor and the outermost ring of the grid are not ground.
 *   obstacles  the occupied voxels that are not FLOOR — floor: the occupied voxels whose contiguous occupied run upwards ends in a
 *              ground voxel — and, with unknown_obstacle = 1, every voxel inside dims that is neither occupied nor free.
 *   drive      the voxels that are not occupied with a ground voxel 1 .. s + 1 levels below: the standing voxel and the s above it.
 * tohip_field_build over (obstacles, NULL) and the travel entry points with the planes (obstacles, drive) as (occupied, free) then give
 * the places a ball whose centre rides in the drive slab can be.  Three launches, integers only, no atomics, nothing read back.
 * tohip_ground_snap: positions (m, 3) f32 -> standing (m, 3) f32 and drop (m) int32.  From the position's voxel (x, y, z) — the
 * coordinate rule of tohip_occ_insert — the first k in 0 .. max_drop (0 <= max_drop <= 2048) with drive at (x, y, z - k) and ground
 * at (x, y, z - k - 1): standing is that voxel's centre fl(origin + fl(fl(i + 0.5) r)), tohip_travel_paths' rule, and drop is k.
 * drop -1: there is none; -2: out of range or outside dims; standing is NaN for both.
 * flags is reserved and must be 0.  Bad flags, H, s, unknown_obstacle or max_drop, a missing, misaligned or aliased plane:
 * TOHIP_EINVAL; a short grid_bytes: TOHIP_ENOSPC.  Every argument check returns before anything is enqueued. */
int tohip_ground_build(const void *occupied, const void *free_or_null, size_t grid_bytes, const tohip_occ_geom *geom, int32_t headroom,
                       int32_t step, int32_t unknown_obstacle, void *support, void *ground, void *obstacles, void *drive, void *stream,
                       uint32_t flags);
int tohip_ground_snap(const void *ground, const void *drive, size_t grid_bytes, const tohip_occ_geom *geom, const float *positions,
                      int64_t m, int32_t max_drop, float *standing, int32_t *drop, void *stream, uint32_t flags);

/* ---- scan matching ("Scan matching") --------------------------------------------------
 * Score a scan — points (n, 3) f32 in the SENSOR frame, 1 <= n <= 2^22 — against an evidence map at candidate poses.  A pose is 12
 * f32: R row-major (9), then t (3).  The world coordinate of point p is, per axis a, fl(fl(fl(fl(R_a0 p_x) + fl(R_a1 p_y)) +
 * fl(R_a2 p_z)) + t_a), and its voxel follows the coordinate rule of tohip_occ_insert.  A point out of range on any axis (NaN, inf)
 * is skipped and not counted in `used`; a point in the apron takes part.  The VALUE of a voxel, with floor_value in [-127, 0] (-127:
 * no floor) and unknown_value in [-127, 0]: max(L, floor_value) inside dims where L != -128; unknown_value where the voxel was never
 * observed or lies outside dims.  The score of a candidate (pose, integer voxel shift s) is the sum over the points not skipped of
 * the value of voxel(p) + s: an int32, the same in every run.
 * tohip_scan_prepare: evidence bytes -> the score table, a buffer of tohip_evid_bytes in brick order: header 256 zero bytes, byte =
 *   128 + value (pad voxels 128 + unknown_value).  table and evid: 16-byte aligned, different.
 * tohip_scan_score: b explicit candidates (1 <= b <= 2^22) — poses (b, 12) f32 and shifts_or_null (b, 3) int32, any values: a shifted voxel
 *   that does not fit 32 bits is outside dims — read from the
 *   evidence bytes themselves -> score, used (points in range), inside (shifted voxel inside dims), known (inside and L != -128), each
 *   (b) int32; zeroed here on the stream.
 * tohip_scan_correlate: k poses (1 <= k <= 256) x the window |dx| <= wx, |dy| <= wy, |dz| <= wz (0 <= wx, wy <= 16, 0 <= wz <= 4),
 *   S = (2wx+1)(2wy+1)(2wz+1), k S <= 2^22, from the TABLE (prepared with the same unknown_value) -> scores[k][dz+wz][dy+wy][dx+wx]
 *   int32 (scores_bytes >= 4 k S) and used (k) int32; zeroed here on the stream.
 * tohip_scan_best: the maximum of the key (score, then smaller dx^2+dy^2+dz^2, then lower flat index) over the k S scores -> best,
 *   int32[8] on the device: flat index, k, dx, dy, dz, score, ties (the candidates whose score equals the best), 0.
 * flags is reserved and must be 0.  A bad window, k, b, n, floor_value, unknown_value or flags, a null, misaligned or aliased buffer:
 * TOHIP_EINVAL; a short buffer: TOHIP_ENOSPC.  Every argument check returns before anything is enqueued.  Nothing is read back. */
int tohip_scan_prepare(const void *evid, size_t evid_bytes, const tohip_occ_geom *geom, int32_t floor_value, int32_t unknown_value,
                       void *table, size_t table_bytes, void *stream, uint32_t flags);
int tohip_scan_score(const void *evid, size_t evid_bytes, const tohip_occ_geom *geom, int32_t floor_value, int32_t unknown_value,
                     const float *points, int64_t n, const float *poses, const int32_t *shifts_or_null, int64_t b, int32_t *score,
                     int32_t *used, int32_t *inside, int32_t *known, void *stream, uint32_t flags);
int tohip_scan_correlate(const void *table, size_t table_bytes, const tohip_occ_geom *geom, int32_t unknown_value, const float *points,
                         int64_t n, const float *poses, int64_t k, int32_t wx, int32_t wy, int32_t wz, int32_t *scores,
                         size_t scores_bytes, int32_t *used, void *stream, uint32_t flags);
int tohip_scan_best(const int32_t *scores, int64_t k, int32_t wx, int32_t wy, int32_t wz, int32_t *best, void *stream, uint32_t flags);

/* ---- particle filter (particle_kernels.hip, DESIGN.md §10, "Particle filter") -------------------------
 * Monte Carlo localisation on the evidence map: n pose hypotheses (1 <= n <= 2^20) kept on the device from scan to scan.
 * state (n, 4) int32, 16-byte aligned: X, Y, Z in 1/256 voxel from the map's origin, clamped to |.| <= 2^24 - 1, and a heading h in
 *   [0, 16384), 1/16384 turn about world z.  log_weight (n) int64: Q16 log2, <= 0, maximum 0 after tohip_mcl_weights, floor -2^40.
 * tables: TOHIP_MCL_TABLE_WORDS int32 the caller builds once (f64, rounded once): word 2 h, 2 h + 1 = round(32768 cos), round(32768
 *   sin) of 2 pi h / 16384; word TOHIP_MCL_GAUSS_WORD + i = round(4096 Phi^-1((i + 0.5) / 1025)), i = 0 .. 1024; word TOHIP_MCL_EXP2_WORD
 *   + j = round(2^20 2^(-j / 256)), j = 0 .. 255.
 * Random numbers: Philox4x32-10, key (seed_lo, seed_hi), counter (particle index, 0, step, stream): stream 0 tohip_mcl_seed_gaussian, 1
 *   tohip_mcl_predict, 2 the resample offset (particle 0), 3 tohip_mcl_seed_positions; the four words serve x, y, z and heading.
 *   noise(u, sigma_q8), sigma_q8 = round(256 sigma) in [0, 2^24]: i = u >> 22, f = (u >> 6) & 0xFFFF, g = (GAUSS[i] (65536 - f) +
 *   GAUSS[i + 1] f) >> 16, noise = (g sigma_q8 + 2^19) >> 20 (arithmetic shifts).
 * tohip_mcl_seed_gaussian: state = clamp(prior_host[a] + noise), heading (prior_host[3] + noise) mod 16384; log_weight = 0.  prior_host
 *   and sigma_q8_host: 4 int32 on the host, |prior| <= 2^24 - 1 (the heading: |.| <= 2^30).
 * tohip_mcl_seed_positions: particle i takes row (word0 mod m) of positions (m, 3) f32 world coordinates, 1 <= m < 2^31: the voxel it
 *   lies in by the coordinate rule of tohip_occ_insert (a row out of range: fixed point 0 on that axis), at 1/256 offsets word1 >> 24,
 *   (word1 >> 16) & 255, word2 >> 24 with jitter = 1 and at the centre (128) with jitter = 0; heading word3 >> 18; log_weight = 0.
 * tohip_mcl_predict: delta_host 4 int32 (a body-frame motion, state units, |.| <= 2^24 - 1), n_a = delta_a + noise; (c, s) = TRIG[h];
 *   X += (c n_x - s n_y + 2^14) >> 15, Y += (s n_x + c n_y + 2^14) >> 15 (64-bit products), Z += n_z, clamped; h = (h + n_h) mod 16384.
 * tohip_mcl_poses: poses (n, 12) f32, 16-byte aligned, scan matching's pose of each particle: R = Rz(h) A with c32 = f32(c) 2^-15 and A
 *   the 9 f32 of attitude_host (row-major; NULL: the identity): row 0 fl(fl(c32 A_0j) - fl(s32 A_1j)), row 1 fl(fl(s32 A_0j) + fl(c32
 *   A_1j)), row 2 A_2j; t_a = fl(fl(f32(X_a) f32(resolution / 256)) + origin_a).
 * tohip_mcl_weigh: for each particle, scan matching's score, used and known (tohip_scan_score at zero shift, under tohip_mcl_poses'
 *   pose) of the scan `points` (p, 3) f32, 1 <= p <= 2^22, read from the evidence bytes -> score, used, known, each (n) int32; zeroed
 *   here on the stream where the points are split over grid rows.
 * tohip_mcl_weights: log_weight += score beta_q (score_or_null NULL: nothing added), beta_q in [1, 65536]; the maximum subtracted, the
 *   floor applied; weights (n) int64: d = -log_weight, w = EXP2[(d & 0xFFFF) >> 8] >> (d >> 16) where d >> 16 <= 20, else 0; record,
 *   TOHIP_MCL_RECORD int64: S1 = sum w, S2 = sum w^2, sum w X, sum w Y, sum w Z, sum w cos, sum w sin (TRIG's integers; the position
 *   sums are exact while n max|X| < 2^43 and wrap modulo 2^64 beyond), the best index (the lowest i with log_weight 0), its score,
 *   known and used (0 where the array is NULL), the verdict (1: n_eff < threshold), n_eff's bits (f64(S1) f64(S1) / f64(S2)), the
 *   maximum subtracted, n, 0.  threshold: finite, >= 0.  workspace: TOHIP_MCL_WORKSPACE_BYTES, 8-byte aligned, contents ignored.
 * tohip_mcl_resample_systematic: the verdict again from record's S1, S2 and `threshold` (record words 11 and 12 rewritten).  If 1: r = (word0 2^32
 *   + word1) mod S1, t_j = (j S1 + r) div n, ancestors[j] = the least i with C_i > t_j (C: the inclusive prefix sum of weights, left in
 *   cumulative (n) uint64), state_out[j] = state[ancestors[j]], log_weight = 0.  If 0: state_out = state, ancestors[j] = j, log_weight
 *   untouched.  weights and record: tohip_mcl_weights' of the same state.
 * flags is reserved and must be 0.  A bad n, p, m, sigma, delta, prior, beta_q, threshold, attitude (not finite) or flags, a null,
 * misaligned or aliased buffer: TOHIP_EINVAL; short tables or workspace: TOHIP_ENOSPC.  Every argument check returns before anything
 * is enqueued.  Nothing is read back. */
#define TOHIP_MCL_TABLE_WORDS 34052
#define TOHIP_MCL_GAUSS_WORD 32768
#define TOHIP_MCL_EXP2_WORD 33796
#define TOHIP_MCL_RECORD 16
#define TOHIP_MCL_WORKSPACE_BYTES 81920
int tohip_mcl_seed_gaussian(int32_t *state, int64_t *log_weight, int64_t n, const int32_t *tables, size_t tables_bytes,
                            const int32_t *prior_host, const int32_t *sigma_q8_host, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                            void *stream, uint32_t flags);
int tohip_mcl_seed_positions(int32_t *state, int64_t *log_weight, int64_t n, const tohip_occ_geom *geom, const float *positions, int64_t m,
                             int32_t jitter, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void *stream, uint32_t flags);
int tohip_mcl_predict(int32_t *state, int64_t n, const int32_t *tables, size_t tables_bytes, const int32_t *delta_host,
                      const int32_t *sigma_q8_host, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void *stream, uint32_t flags);
int tohip_mcl_poses(const int32_t *state, int64_t n, const int32_t *tables, size_t tables_bytes, const tohip_occ_geom *geom,
                    const float *attitude_host, float *poses, void *stream, uint32_t flags);
int tohip_mcl_weigh(const void *evid, size_t evid_bytes, const tohip_occ_geom *geom, int32_t floor_value, int32_t unknown_value,
                    const float *points, int64_t p, const int32_t *state, int64_t n, const int32_t *tables, size_t tables_bytes,
                    const float *attitude_host, int32_t *score, int32_t *used, int32_t *known, void *stream, uint32_t flags);
int tohip_mcl_weights(const int32_t *state, int64_t *log_weight, int64_t n, const int32_t *tables, size_t tables_bytes,
                      const int32_t *score_or_null, const int32_t *used_or_null, const int32_t *known_or_null, int32_t beta_q,
                      double threshold, int64_t *weights, int64_t *record, void *workspace, size_t workspace_bytes, void *stream,
                      uint32_t flags);
int tohip_mcl_resample_systematic(const int32_t *state, int32_t *state_out, int64_t *log_weight, int64_t n, const int64_t *weights, int64_t *record,
                       double threshold, uint64_t *cumulative, int32_t *ancestors, void *workspace, size_t workspace_bytes,
                       uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void *stream, uint32_t flags);

/* ---- relocalisation (scansearch_kernels.hip, DESIGN.md §10, "Relocalisation") -------------------------
 * The best candidate of a WIDE window — |dx| <= wx, |dy| <= wy (0 <= wx, wy <= 2048), |dz| <= wz (0 <= wz <= 4), k rotations (1 <= k
 * <= 256) — by branch and bound, equal to the exhaustive search's under scan matching's key, bit for bit.  Poses, points, values and
 * the score of a candidate are scan matching's; table is tohip_scan_prepare's.  With u = 128 + unknown_value:
 * LEVEL TABLES: T_0 is the table; T_h (1 <= h <= 6) has its size, header and brick order, and for a voxel inside dims T_h(x, y, z) =
 *   max over 0 <= i, j < 2^h of T_0'(x + i, y + j, z), T_0' being T_0 continued by u outside dims; pad voxels hold u.
 * LOOKUP: with b = 2^h - 1, B_h(x, y, z) = u where z is outside [0, nz) or x outside [-b, nx) or y outside [-b, ny); otherwise
 *   T_h(max(x, 0), max(y, 0), z), replaced by max(that, u) where x < 0 or y < 0.
 * NODE: four int32 (k, sx, sy, sz) at a level h: rotation k, dz = sz, dx in [sx, sx + 2^h) and dy in [sy, sy + 2^h), cut to the
 *   window.  Its BOUND: the sum over the points in range under rotation k of B_h(voxel_k(p) + (sx, sy, sz)), less 128 x their number
 *   — an int32, at level 0 the candidate's score.
 * tohip_reloc_levels: table -> levels, h tables of tohip_evid_bytes each, T_1 first (16-byte aligned, not overlapping the table;
 *   levels_bytes >= h x that size).  h launches.
 * tohip_reloc_bounds: m explicit nodes (m, 4) int32 (1 <= m <= 2^22, 16-byte aligned, any order, any shifts) of one level (0 .. 6),
 *   `table` being THAT level's table -> bounds (m) int32 and used (k) int32, the points in range under each rotation; a node whose k
 *   is outside [0, k) gets INT32_MIN.  workspace: tohip_reloc_workspace_bytes(m), 16-byte aligned, contents undefined before and after.
 * tohip_reloc_workspace_bytes(capacity): what a search with that capacity (1 .. 2^24 nodes a level), or bounds of that many nodes,
 *   needs; 0 for a capacity out of range.
 * tohip_reloc_search: the whole search, h levels (0 <= h <= 6; levels_or_null may be NULL for h = 0), enqueued at once.  The top
 *   level holds every node with sx in {-wx, -wx + 2^h, ...} <= wx, sy likewise, every sz and every rotation; per level h .. 1 the node
 *   with the largest bound (then the lowest (k, sz, sy, sx)) is followed greedily to a leaf, the incumbent becomes max(incumbent, the
 *   leaf's score), every node whose bound is below the incumbent is dropped and the others are replaced by their up to four children
 *   (sx, sy) + {0, 2^(h-1)}^2 that start inside the window.  -> record, 18 int64 on the device: the flat index ((k (2wz+1) + dz+wz)
 *   (2wy+1) + dy+wy) (2wx+1) + dx+wx of the winner, k, dx, dy, dz, score, ties, status, incumbent (INT32_MIN for h = 0), evaluated
 *   (all bounds computed, descents included), h, then nodes[0 .. h], the nodes of each level before the drop; the rest 0.  A level
 *   that would hold more than `capacity` nodes stops the search: status = count << 3 | (level + 1), flat index -1, nodes[level] =
 *   count, and nothing is written past a buffer; status 0 otherwise.  The order of a node list in memory is not defined; the record is
 *   the same in every run.
 * flags is reserved and must be 0.  A bad window, k, h, level, n, m, capacity, unknown_value or flags, a null, misaligned or aliased
 * buffer: TOHIP_EINVAL; a short buffer: TOHIP_ENOSPC.  Every argument check returns before anything is enqueued.  Nothing is read back. */
int tohip_reloc_levels(const void *table, size_t table_bytes, const tohip_occ_geom *geom, int32_t unknown_value, int32_t h, void *levels,
                       size_t levels_bytes, void *stream, uint32_t flags);
int tohip_reloc_bounds(const void *table, size_t table_bytes, const tohip_occ_geom *geom, int32_t unknown_value, int32_t level,
                       const float *points, int64_t n, const float *poses, int64_t k, const int32_t *nodes, int64_t m, int32_t *bounds,
                       int32_t *used, void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);
size_t tohip_reloc_workspace_bytes(int64_t capacity);
int tohip_reloc_search(const void *table, size_t table_bytes, const void *levels_or_null, size_t levels_bytes, const tohip_occ_geom *geom,
                       int32_t unknown_value, int32_t h, const float *points, int64_t n, const float *poses, int64_t k, int32_t wx,
                       int32_t wy, int32_t wz, int64_t capacity, int64_t *record, void *workspace, size_t workspace_bytes, void *stream,
                       uint32_t flags);

/* ---- scan registration (scanreg_kernels.hip, DESIGN.md §10, "Scan registration") ----------------------
 * Sub-voxel refinement of B poses (1 <= b <= 256) of one scan by damped Gauss-Newton steps on the trilinear interpolation of the
 * score table.  Poses, points, the transform rule, the skip rule and the table are scan matching's.  All per-point terms are integers
 * on the map's 1/256-voxel fixed point q = the coordinate rule of tohip_occ_insert:
 *   c = q - 128, base voxel c >> 8, fraction f = c & 255, weights 256 - f and f per axis; V[i][j][k] the table byte of the base voxel
 *   + (i, j, k), 128 + unknown_value outside dims;  M24 = sum V wx wy wz;  Gx16 = sum_jk wy wz (V[1][j][k] - V[0][j][k]), Gy16 and Gz16
 *   alike;  e = (255 2^24 - M24 + 2^11) >> 12;  g = (G16 + 2^7) >> 8;  a = (q - q_t + 32) >> 6 with q_t the fixed point of the pose's
 *   own translation;  j = (a x g + 2^11) >> 12;  row J = (g, j): translation in 1/256 byte per voxel, rotation about the sensor's
 *   position in the WORLD frame in 4 byte per radian, e in 1/4096 byte (the residual 255 - M).
 * RECORD of a pose, TOHIP_SCANREG_RECORD int64: [0:21] the upper triangle of sum J J^T, row-major; [21:27] sum J e; [27] sum e^2; [28]
 *   used, the points not skipped; [29] inside, those whose eight corners all lie inside dims; [30:32] 0.  Every sum stays below 2^62
 *   for n <= 2^22.  A pose whose translation is out of range has an all-zero record.
 * STATE of a pose, TOHIP_SCANREG_STATE 8-byte words, f64 unless named int64: [0:3] t in metres; [3:7] q wxyz, UNNORMALISED; [7] lambda;
 *   [8:14] the last step (voxels x3, radians x3); [14] status int64 (0 running, 1 converged, 2 stalled, 3 degenerate, 4 empty: every
 *   value but 0 is frozen); [15] iterations int64; [16] accepted steps int64; [17:20] trial t; [20:24] trial q; [24:56] the record at
 *   [0:7], int64; [56:64] 0.  The caller writes the start: t, q, trial = them, lambda (2^-10), the rest 0, and `poses` = the trial's 12 f32.
 * tohip_scanreg_normal: records (b, 32) int64 of the poses (b, 12) f32, zeroed here on the stream, then one launch.  state_or_null: the
 *   blocks of a pose whose status is not 0 return at once (its record stays 0).  8-byte aligned records and state.
 * tohip_scanreg_step: one step per pose from the records at the trial poses: a frozen pose is left alone; used = 0: empty; the trial
 *   is accepted iff it is the first iteration or (used equals the current used and sum e^2 is smaller): current <- trial, from the
 *   second iteration on lambda <- max(lambda / 8, 2^-30), and converged if the accepted step was within tol_t voxels and tol_r radians
 *   on every axis; rejected: lambda <- 8 lambda, stalled if that exceeds 2^30.  Then A = S H S, rhs = S b / 4096, S = diag(1/256 x3,
 *   4 x3), over the degrees of freedom of dof_mask (bit i of x y z roll pitch yaw; 1 .. 63), A_ii += lambda A_ii, LDL^T without
 *   pivoting (a pivot <= 0 or not finite: degenerate), trial t = t + resolution delta_t, trial q = (1, delta_theta / 2) (x) q, and
 *   poses[12 b ..] = the f32 roundings of R (from the unnormalised q, s = 2 / q.q) and the trial t.  f64 add, multiply, divide and
 *   compare in one fixed order: the same bits in every run.  One launch.
 * flags is reserved and must be 0.  A bad n, b, unknown_value, resolution, dof_mask, tolerance or flags, a null, misaligned or aliased
 * buffer: TOHIP_EINVAL; a short table: TOHIP_ENOSPC.  Every argument check returns before anything is enqueued.  Nothing is read back. */
#define TOHIP_SCANREG_RECORD 32
#define TOHIP_SCANREG_STATE 64
int tohip_scanreg_normal(const void *table, size_t table_bytes, const tohip_occ_geom *geom, int32_t unknown_value, const float *points,
                         int64_t n, const float *poses, int64_t b, const int64_t *state_or_null, int64_t *records, void *stream,
                         uint32_t flags);
int tohip_scanreg_step(const int64_t *records, int64_t *state, int64_t b, float resolution, int32_t dof_mask, double tol_t, double tol_r,
                       float *poses, void *stream, uint32_t flags);

/* ---- pose-graph optimisation (posegraph_kernels.hip, DESIGN.md §10, "Pose graph") ----------------------
 * Nodes: n_nodes poses, 7 f64 each (t in metres, q wxyz, NOT required to be unit; R(q) with s = 2 / q.q).  Edges: ab (e, 2) int32, a = -1
 * an ABSOLUTE edge (node b measured in the world: an edge from the frame t = 0, q = (1, 0, 0, 0)); meas (e, 7) f64, z_t and z_q wxyz;
 * omega (e, 21) f64, the upper triangle of the symmetric 6 x 6 information matrix over (x, y, z, roll, pitch, yaw), row-major.
 * Residual: e_t = R_a^T (t_b - t_a) - z_t;  eps = conj(q_a) (x) q_b (x) conj(z_q);  e_r = 2 vec(eps) / w(eps) (no sqrt, no
 * trigonometry, invariant to the sign and scale of every quaternion; w(eps) = 0 makes the cost non-finite).  s = e^T Omega e; cost =
 * sum rho(s): rho = s, or with robust_c = c > 0 Geman-McClure c^2 s / (c^2 + s) and the IRLS weight (c^2 / (c^2 + s))^2.  A node moves
 * by t + dt, q <- (1, dr / 2) (x) q.  free_mask (n_nodes) int32: bit i frees degree of freedom i of a node, 0 fixes it; a locked one has
 * an identity row and column and a zero right-hand side.  row_ptr (n_nodes + 1) and incident (n_incident) int32: node i's incident
 * edges incident[row_ptr[i] .. row_ptr[i + 1]), each 2 edge + side (0: the node is a, 1: it is b), in ascending edge index; a and b
 * of an edge differ.  The caller builds them (synth.pose_graph_incidence); the kernels trust them within the sizes given.
 * EDGE RECORD, TOHIP_POSEGRAPH_EDGE f64: [0:6] e; [6] s; [7] the weight w; [8] rho; [9] 0; with W = w Omega and the columns of locked
 *   degrees of freedom of Ja, Jb cleared: [10:31] Ja^T W Ja and [31:52] Jb^T W Jb (upper triangles), [52:88] Ja^T W Jb, [88:94] Ja^T W e,
 *   [94:100] Jb^T W e.  800 bytes an edge, two buffers of them (current and trial).
 * WORKSPACE: tohip_posegraph_workspace_bytes(n, e) bytes, 8-byte aligned; tohip_posegraph_layout gives the word offsets of its
 *   TOHIP_POSEGRAPH_REGIONS regions: the scalars (3 copies of TOHIP_POSEGRAPH_SCALARS words; copy 1 is current between calls: lambda, cost,
 *   initial cost, status int64 (0 running, 1 converged, 2 stalled, 3 degenerate, 4 non-finite), iterations, accepted, CG iterations in
 *   total, the current buffer 0 / 1, r.z, its first value, the CG stop flag, whether a trial was ever accepted), poses (8 n), the
 *   pending step x (6 n), the edge records (2 e 100), the node blocks D (21) and g (6) (2 n 27), L d L^T (21 n), r, z (6 n each), p
 *   (2 x 6 n), A p (6 n), the partial arrays of the cost, r.z, p.Ap, the small-step and bad-pivot flags, the trial cost with the
 *   small-step flags' conjunction behind it (2 words), the total.
 * tohip_posegraph_start: the poses from `nodes`, x = 0, the three copies of the scalars 0 but lambda = 2^-10, the small-step flags 1.
 *   Every other region stays as it was allocated: each is written before it is read.  One launch.
 * tohip_posegraph_linearize: the records at the TRIAL poses (current moved by x) into the buffer that is not current, and the cost's
 *   block partials.  tohip_posegraph_gather: each node's D and g over its incident edges, and the trial cost.  One launch each.
 * tohip_posegraph_step: k_scan_step's state machine on the trial cost (non-finite: status 4; the first trial, or a strictly lower
 *   cost: accepted, from the second on lambda <- max(lambda / 8, 2^-30) and converged if the accepted step was within tol_t and tol_r on
 *   every node; else lambda <- 8 lambda, stalled past 2^30), then (H + lambda diag H) x = -g by conjugate gradients from x = 0,
 *   preconditioned by the L d L^T of each damped diagonal block (a pivot <= 0 or not finite: status 3): 1 + 2 cg_iterations launches;
 *   the solve stops at r.z <= cg_tol^2 (r.z)_0 or p.Ap <= 0, after which the remaining launches return at once.
 * tohip_posegraph_optimize: `iterations` rounds of linearize, gather, step, enqueued at once.  tohip_posegraph_result: out (16 + 7 n +
 *   2 e) f64: the current scalars, the poses, s and w of every edge at the current poses (0 before any acceptance).
 * Every sum has one order: the same bits in every run, and synth.pose_graph_*_ref's.  flags is reserved and must be 0.  A
 * bad size, count, tolerance or flags, a null or misaligned buffer, or a workspace (or out) that shares a byte with an input (or
 * with the workspace), by address ranges: TOHIP_EINVAL; a short workspace: TOHIP_ENOSPC (tohip_posegraph_workspace_bytes: 0).  Every argument check returns before anything is enqueued.  Nothing is
 * read back. */
#define TOHIP_POSEGRAPH_EDGE 100
#define TOHIP_POSEGRAPH_SCALARS 16
#define TOHIP_POSEGRAPH_REGIONS 17
#define TOHIP_POSEGRAPH_MAX_ITERATIONS 256
#define TOHIP_POSEGRAPH_MAX_CG 4096
size_t tohip_posegraph_workspace_bytes(int64_t n_nodes, int64_t n_edges, uint32_t flags);
int tohip_posegraph_layout(int64_t n_nodes, int64_t n_edges, int64_t *offsets_host, uint32_t flags);
int tohip_posegraph_start(const double *nodes, int64_t n_nodes, int64_t n_edges, void *workspace, size_t workspace_bytes, void *stream,
                          uint32_t flags);
int tohip_posegraph_linearize(const int32_t *ab, const double *meas, const double *omega, const int32_t *row_ptr, const int32_t *incident,
                              const int32_t *free_mask, int64_t n_nodes, int64_t n_edges, int64_t n_incident, double robust_c,
                              void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);
int tohip_posegraph_gather(const int32_t *ab, const double *meas, const double *omega, const int32_t *row_ptr, const int32_t *incident,
                           const int32_t *free_mask, int64_t n_nodes, int64_t n_edges, int64_t n_incident, void *workspace,
                           size_t workspace_bytes, void *stream, uint32_t flags);
int tohip_posegraph_step(const int32_t *ab, const double *meas, const double *omega, const int32_t *row_ptr, const int32_t *incident,
                         const int32_t *free_mask, int64_t n_nodes, int64_t n_edges, int64_t n_incident, int64_t cg_iterations,
                         double cg_tol, double tol_t, double tol_r, void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);
int tohip_posegraph_optimize(const int32_t *ab, const double *meas, const double *omega, const int32_t *row_ptr, const int32_t *incident,
                             const int32_t *free_mask, int64_t n_nodes, int64_t n_edges, int64_t n_incident, int64_t iterations,
                             int64_t cg_iterations, double cg_tol, double robust_c, double tol_t, double tol_r, void *workspace,
                             size_t workspace_bytes, void *stream, uint32_t flags);
int tohip_posegraph_result(int64_t n_nodes, int64_t n_edges, const void *workspace, size_t workspace_bytes, double *out, void *stream,
                           uint32_t flags);

/* ---- optional per-kernel timing (bench.py's roofline leg) -----------------------------------------
 * When enabled, every launch of the big kernels is bracketed by hipEventRecord on its own stream.
 * tohip_profile_read synchronises on those events and returns, per kernel id < TOHIP_PROF_NKERNELS,
 * the summed milliseconds and the number of launches since the last read (HOST arrays). */
#define TOHIP_PROF_NKERNELS 6
int tohip_profile_enable(int on);
const char *tohip_profile_name(int id);
int tohip_profile_read(double *ms_sum_host, int64_t *counts_host);
/* Diagnostic: while a device buffer is set, every block of k_traj_pass1 (the dense kernel) stores two 64-bit words — its
 * lifetime in shader-clock ticks (s_memtime) and in 100 MHz ticks (s_memrealtime) — at [2*block], then four words per block
 * (start, end, HW_ID, XCC_ID) from [2*grid]; grid = tohip_profile_clock_blocks(n_points, n_virtual, flags, with_occlusion) blocks
 * (6 words each); NULL switches it off.  Their quotient x 100 MHz is the clock
 * the chip actually holds under this kernel (it gives clock back under load).  Never set during a timed pass.
 * The XCC_ID word's low four bits are the XCD (mask with 0xf); bit 8 (0x100) is set by the wide dense kernel (sixteen points per
 * lane: the one a long dense launch without occlusion bits is routed to) and clear from the narrow one — which kernel ran. */
int tohip_profile_clock(void *device_buffer);
int64_t tohip_profile_clock_blocks(int64_t n_points, int64_t n_virtual, int flags, int with_occlusion);

/* Diagnostic: what the last forward over `workspace` found.  stats (DEVICE int64 x 5, zero-filled by the caller):
 * [0] flagged (256-point slot, virtual waypoint) pairs — the pairs with a non-zero log-odds term or a gradient;
 * [1] candidate (slot, trajectory) items of pass 1; [2] slots; [3] virtual waypoints; [4] the (slot, waypoint) pairs the last
 * culled pass 1 evaluated (stale after a dense one). */
int tohip_traj_step_stats(int64_t n_points, int64_t n_virtual, int64_t n_traj, const void *workspace, size_t workspace_bytes,
                          int64_t *stats, void *stream);

/* ---- self tests of cross-lane primitives (used by tests/, cheap) -------------------------------- */
int tohip_selftest_wave_reduce(const float *in64xK, int32_t k, float *out_sum, float *out_min, float *out_max,
                               void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJOPT_HIP_H */
