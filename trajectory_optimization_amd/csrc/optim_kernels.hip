// optim_kernels.hip — the O(W) remainder of one optimisation step on the device:
// the regularisers of ModelTraj.criterion with their analytic gradients, the total loss, Adam, and the
// reference's early-stop rule, so that an optimisation run enqueues kernels only and never syncs the host.
//
//   criterion: l2 / smooth / length   /root/reference/src/model.py:244-260, :135-155
//   Adam (two parameter groups)       /root/reference/src/trajectory_optimization.py:91-94 (torch.optim.Adam defaults)
//   early stop                        /root/reference/src/trajectory_optimization.py:100-124
//
// Everything here is a single small block: W is tens to a few thousand waypoints.  The step tail's own block — scatter,
// regularisers, clearance merge, Adam — is opt_step.hpp's (tail_gradients, tail_adam), shared with team_kernels.hip's tail; its
// argument check and struct fill (tail_args_ok, tail_args_fill) stand behind every tail entry point of both files.
#include "common.hpp"
#include "opt_step.hpp"

// loss_terms[0..4] = vis, l2, length, smooth, total.  grad_poses (W,3) receives the regularisers' gradient (ADDED to what the
// visibility backward wrote when accumulate != 0).  state (may be NULL): the loss row written is state[3] (steps taken so far).
// clr_terms (may be NULL): the clearance query's per-waypoint terms; the loss row then gets [5] = clearance and the five-term total.
__global__ void __launch_bounds__(TO_BLOCK)
k_traj_regularizers(const float* __restrict__ poses, const float* __restrict__ poses0, int W, float smooth_w,
                    float length_w, float eps, const float* __restrict__ scalars, float* __restrict__ loss_terms,
                    float* __restrict__ grad_poses, int accumulate, const float* __restrict__ state,
                    float* __restrict__ grad_terms, const double* __restrict__ clr_terms, float clr_w) {
    __shared__ double lds[TO_BLOCK / 64];
    __shared__ double sh[4];
    RegOut o = regularizers_eval(poses, poses0, W, smooth_w, length_w, eps, grad_poses, accumulate, grad_terms, lds, sh);
    if (threadIdx.x != 0) return;
    if (clr_terms) { o.has_clr = true; o.clr = clearance_sum(clr_terms, W, clr_w); }
    write_loss_terms(state ? loss_terms + 8 * (int)state[3] : loss_terms, (double)scalars[1], o);
}

// scatter the gradient rows of the evaluated waypoints (every wps_step-th) into full (W,3)/(W,4) arrays
__global__ void k_scatter_rows(const float* __restrict__ src, int n_rows, int cols, int step, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * cols) return;
    const int r = i / cols, c = i - r * cols;
    dst[(int64_t)r * step * cols + c] = src[i];
}
__global__ void k_gather_rows(const float* __restrict__ src, int n_rows, int cols, int step, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * cols) return;
    const int r = i / cols, c = i - r * cols;
    dst[i] = src[(int64_t)r * step * cols + c];
}

// torch.optim.Adam (defaults betas=(0.9,0.999), eps=1e-8, no weight decay / amsgrad), one call per parameter group.
// No-op once state[2] (stopped) is set.  `t` = 1-based step index.
__global__ void k_adam(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v,
                       int n, float lr, float beta1, float beta2, float eps, int t, const float* __restrict__ state) {
    if (state && state[2] != 0.f) return;
    if (t <= 0) t = (int)state[3] + 1;  // step index kept on the device: the same launch can be replayed from a hipGraph
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) adam_element(param, grad[i], m, v, i, lr, beta1, beta2, eps, t);
}

// The reference's early-stop rule, evaluated after the step: gains relative to the first step's values.
__device__ __forceinline__ void early_stop_rule(const float* __restrict__ scalars, const float* __restrict__ loss_terms,
                                                float rewards_th, float smoothness_th, float* __restrict__ state,
                                                int row_from_state) {
    if (row_from_state) loss_terms += 8 * (int)state[3];
    early_stop_next(state, state, scalars[0], loss_terms[3], rewards_th, smoothness_th);   // loss_terms: this step's row
}

__global__ void k_early_stop(const float* __restrict__ scalars /* [0] = mean reward */, const float* __restrict__ loss_terms,
                             float rewards_th, float smoothness_th, float* __restrict__ state, int row_from_state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) early_stop_rule(scalars, loss_terms, rewards_th, smoothness_th, state, row_from_state);
}

// One block does the whole O(W) remainder of an optimisation step (optimizer.optimize_trajectory's separate-calls path): scatter of
// the evaluated waypoints' visibility gradients into full (W,3)/(W,4) arrays, criterion regularisers + their gradient on top, the
// two Adam updates (opt_step.hpp: tail_gradients, tail_adam — the block a team member runs too), then what is the trajectory's
// alone: its loss row, and the early-stop rule on its state in place — five launches and two memsets otherwise.
// Block b = trajectory b: equal-length trajectories laid end to end, each with its own state, scalars and log.
struct StepTail : TailArgs {
    float* state;   // (n_traj, 8), updated in place
};

__global__ void __launch_bounds__(TO_BLOCK) k_traj_step_tail(StepTail a) {
    __shared__ double lds[TO_BLOCK / 64];
    __shared__ double sh[4];
    const int64_t b = blockIdx.x;
    const float* scalars = a.scalars + b * 4;
    float* state = a.state + b * 8;
    float* loss_log = a.loss_log + b * a.log_stride;
    const TailArgs r = tail_block(a, b);
    RegOut o = tail_gradients(r, lds, sh);
    if (state[2] == 0.f) tail_adam(r, (int)state[3] + 1);   // not stopped yet (uniform)
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (a.clr) { o.has_clr = true; o.clr = clearance_sum(a.clr_term + b * a.W, a.W, a.clr_w); }
    write_loss_terms(loss_log + 8 * (int)state[3], (double)scalars[1], o);
    early_stop_rule(scalars, loss_log, a.rewards_th, a.smoothness_th, state, 1);
}

// poses_e[r] = poses[r * step], quats_e[r] = quats[r * step] in one launch (model.py:217's waypoint selection)
__global__ void k_gather_waypoints(const float* __restrict__ poses, const float* __restrict__ quats, int n_eval, int step,
                                   float* __restrict__ poses_e, float* __restrict__ quats_e) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_eval * 3) { const int r = i / 3, k = i - 3 * r; poses_e[i] = poses[(int64_t)r * step * 3 + k]; }
    if (i < n_eval * 4) { const int r = i >> 2, k = i & 3; quats_e[i] = quats[(int64_t)r * step * 4 + k]; }
}

// several equal-length trajectories laid end to end: rows r*step of each (blockIdx.y = trajectory)
__global__ void k_gather_waypoints_multi(const float* __restrict__ poses, const float* __restrict__ quats, int W, int n_eval, int step,
                                         float* __restrict__ poses_e, float* __restrict__ quats_e) {
    const int64_t b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_eval * 3) { const int r = i / 3, kk = i - 3 * r; poses_e[b * n_eval * 3 + i] = poses[(b * W + (int64_t)r * step) * 3 + kk]; }
    if (i < n_eval * 4) { const int r = i >> 2, kk = i & 3; quats_e[b * n_eval * 4 + i] = quats[(b * W + (int64_t)r * step) * 4 + kk]; }
}

extern "C" int tohip_gather_waypoints_multi(const float* poses, const float* quats, int64_t W, int64_t n_traj, int64_t n_eval, int step,
                                            float* poses_e, float* quats_e, void* stream_) {
    if (!poses || !quats || !poses_e || !quats_e || n_eval <= 0 || step <= 0 || W <= 0 || n_traj <= 0 || n_traj > 65535) return TOHIP_EINVAL;
    const int n = (int)(n_eval * 4);
    k_gather_waypoints_multi<<<dim3((n + 255) / 256, (unsigned)n_traj), 256, 0, (hipStream_t)stream_>>>(poses, quats, (int)W, (int)n_eval, step,
                                                                                                       poses_e, quats_e);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_gather_waypoints(const float* poses, const float* quats, int64_t n_eval, int step, float* poses_e,
                                      float* quats_e, void* stream_) {
    if (!poses || !quats || !poses_e || !quats_e || n_eval <= 0 || step <= 0) return TOHIP_EINVAL;
    const int n = (int)(n_eval * 4);
    k_gather_waypoints<<<(n + 255) / 256, 256, 0, (hipStream_t)stream_>>>(poses, quats, (int)n_eval, step, poses_e, quats_e);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

// the one check, struct fill and launch behind tohip_traj_step_tail, _multi and _clearance (clearance_grad NULL: no clearance term)
static int traj_step_tail_launch(float* poses, float* quats, const float* poses0, int64_t W, int64_t n_traj,
                                 const float* poses_grad_eval, const float* quats_grad_eval, int64_t n_eval, int step,
                                 float* poses_grad, float* quats_grad, float* exp_avg_p, float* exp_avg_sq_p, float* exp_avg_q,
                                 float* exp_avg_sq_q, float smoothness_weight, float traj_length_weight, float eps,
                                 float lr_pose, float lr_quat, float beta1, float beta2, float adam_eps, float rewards_th,
                                 float smoothness_th, const float* scalars, float* loss_terms, int64_t loss_terms_stride,
                                 float* state, float clearance_weight, const float* clearance_grad,
                                 const double* clearance_terms, void* stream_) {
    StepTail a;
    tail_args_fill(a, poses, quats, poses0, W, poses_grad_eval, quats_grad_eval, n_eval, step, poses_grad, quats_grad, exp_avg_p, exp_avg_sq_p,
                   exp_avg_q, exp_avg_sq_q, smoothness_weight, traj_length_weight, eps, lr_pose, lr_quat, beta1, beta2, adam_eps, rewards_th,
                   smoothness_th, scalars, loss_terms, loss_terms_stride, clearance_weight, clearance_grad, clearance_terms);
    a.state = state;
    if (!tail_args_ok(a, W, n_eval, n_traj) || !state) return TOHIP_EINVAL;
    k_traj_step_tail<<<(int)n_traj, TO_BLOCK, 0, (hipStream_t)stream_>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_traj_step_tail_multi(float* poses, float* quats, const float* poses0, int64_t W, int64_t n_traj,
                                          const float* poses_grad_eval, const float* quats_grad_eval, int64_t n_eval, int step,
                                          float* poses_grad, float* quats_grad, float* exp_avg_p, float* exp_avg_sq_p, float* exp_avg_q,
                                          float* exp_avg_sq_q, float smoothness_weight, float traj_length_weight, float eps,
                                          float lr_pose, float lr_quat, float beta1, float beta2, float adam_eps, float rewards_th,
                                          float smoothness_th, const float* scalars, float* loss_terms, int64_t loss_terms_stride,
                                          float* state, void* stream_) {
    return traj_step_tail_launch(poses, quats, poses0, W, n_traj, poses_grad_eval, quats_grad_eval, n_eval, step, poses_grad, quats_grad,
                                 exp_avg_p, exp_avg_sq_p, exp_avg_q, exp_avg_sq_q, smoothness_weight, traj_length_weight, eps, lr_pose, lr_quat,
                                 beta1, beta2, adam_eps, rewards_th, smoothness_th, scalars, loss_terms, loss_terms_stride, state, 0.f, nullptr, nullptr, stream_);
}

extern "C" int tohip_traj_step_tail_clearance(float* poses, float* quats, const float* poses0, int64_t W, int64_t n_traj,
                                              const float* poses_grad_eval, const float* quats_grad_eval, int64_t n_eval, int step,
                                              float* poses_grad, float* quats_grad, float* exp_avg_p, float* exp_avg_sq_p, float* exp_avg_q,
                                              float* exp_avg_sq_q, float smoothness_weight, float traj_length_weight, float eps,
                                              float lr_pose, float lr_quat, float beta1, float beta2, float adam_eps, float rewards_th,
                                              float smoothness_th, const float* scalars, float* loss_terms, int64_t loss_terms_stride,
                                              float* state, float clearance_weight, const float* clearance_grad,
                                              const double* clearance_terms, void* stream_) {
    if (!clearance_grad || !clearance_terms) return TOHIP_EINVAL;
    return traj_step_tail_launch(poses, quats, poses0, W, n_traj, poses_grad_eval, quats_grad_eval, n_eval, step, poses_grad, quats_grad,
                                 exp_avg_p, exp_avg_sq_p, exp_avg_q, exp_avg_sq_q, smoothness_weight, traj_length_weight, eps, lr_pose, lr_quat,
                                 beta1, beta2, adam_eps, rewards_th, smoothness_th, scalars, loss_terms, loss_terms_stride, state, clearance_weight, clearance_grad,
                                 clearance_terms, stream_);
}

extern "C" int tohip_traj_step_tail(float* poses, float* quats, const float* poses0, int64_t W, const float* poses_grad_eval,
                                    const float* quats_grad_eval, int64_t n_eval, int step, float* poses_grad, float* quats_grad,
                                    float* exp_avg_p, float* exp_avg_sq_p, float* exp_avg_q, float* exp_avg_sq_q,
                                    float smoothness_weight, float traj_length_weight, float eps, float lr_pose, float lr_quat,
                                    float beta1, float beta2, float adam_eps, float rewards_th, float smoothness_th,
                                    const float* scalars, float* loss_terms, float* state, void* stream_) {
    return traj_step_tail_launch(poses, quats, poses0, W, 1, poses_grad_eval, quats_grad_eval, n_eval, step, poses_grad, quats_grad,
                                 exp_avg_p, exp_avg_sq_p, exp_avg_q, exp_avg_sq_q, smoothness_weight, traj_length_weight, eps, lr_pose, lr_quat,
                                 beta1, beta2, adam_eps, rewards_th, smoothness_th, scalars, loss_terms, 0, state, 0.f, nullptr, nullptr, stream_);
}

// the one launch behind tohip_traj_regularizers and _clearance (clearance_terms NULL: no clearance term)
static int traj_regularizers_launch(const float* poses, const float* poses0, int64_t W, float smoothness_weight, float traj_length_weight,
                                    float eps, const float* scalars, float* loss_terms, float* grad_poses, int accumulate,
                                    const float* state, float* grad_terms, float clearance_weight, const double* clearance_terms,
                                    void* stream_) {
    if (!poses || !poses0 || !scalars || !loss_terms || W < 3) return TOHIP_EINVAL;
    k_traj_regularizers<<<1, TO_BLOCK, 0, (hipStream_t)stream_>>>(poses, poses0, (int)W, smoothness_weight, traj_length_weight, eps, scalars,
                                                                  loss_terms, grad_poses, accumulate, state, grad_terms, clearance_terms,
                                                                  clearance_weight);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_traj_regularizers(const float* poses, const float* poses0, int64_t W, float smoothness_weight,
                                       float traj_length_weight, float eps, const float* scalars, float* loss_terms,
                                       float* grad_poses, int accumulate, const float* state, float* grad_terms,
                                       void* stream_) {
    return traj_regularizers_launch(poses, poses0, W, smoothness_weight, traj_length_weight, eps, scalars, loss_terms, grad_poses, accumulate,
                                    state, grad_terms, 0.f, nullptr, stream_);
}

extern "C" int tohip_traj_regularizers_clearance(const float* poses, const float* poses0, int64_t W, float smoothness_weight,
                                                 float traj_length_weight, float eps, const float* scalars, float* loss_terms,
                                                 float* grad_poses, int accumulate, const float* state, float* grad_terms,
                                                 float clearance_weight, const double* clearance_terms, void* stream_) {
    if (!clearance_terms || !std::isfinite(clearance_weight) || !(clearance_weight >= 0.f)) return TOHIP_EINVAL;
    return traj_regularizers_launch(poses, poses0, W, smoothness_weight, traj_length_weight, eps, scalars, loss_terms, grad_poses, accumulate,
                                    state, grad_terms, clearance_weight, clearance_terms, stream_);
}

extern "C" int tohip_rows_strided(const float* src, int64_t n_rows, int cols, int step, int scatter, float* dst,
                                  void* stream_) {
    if (!src || !dst || n_rows <= 0 || cols <= 0 || step <= 0) return TOHIP_EINVAL;
    const int n = (int)(n_rows * cols);
    if (scatter) k_scatter_rows<<<(n + 255) / 256, 256, 0, (hipStream_t)stream_>>>(src, (int)n_rows, cols, step, dst);
    else k_gather_rows<<<(n + 255) / 256, 256, 0, (hipStream_t)stream_>>>(src, (int)n_rows, cols, step, dst);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                               float beta1, float beta2, float eps, int32_t step, const float* state, void* stream_) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || n > 0x7fffffff || (step < 1 && !state)) return TOHIP_EINVAL;
    k_adam<<<(int)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>(param, grad, exp_avg, exp_avg_sq, (int)n, lr, beta1, beta2,
                                                                      eps, step, state);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

// torch.optim.Adam's update of up to TOHIP_ADAM_MAX_GROUPS parameter tensors in ONE launch (blockIdx.y = tensor): the reference's
// optimiser holds two (poses @ lr_pose, quats @ lr_quat; trajectory_optimization.py:91-94), torch launches ~7 kernels for each.
struct AdamMulti { tohip_adam_group g[TOHIP_ADAM_MAX_GROUPS]; };
__global__ void __launch_bounds__(256) k_adam_multi(AdamMulti a) {
    const tohip_adam_group& g = a.g[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * blockDim.x)
        adam_element(g.param, g.grad[i], g.exp_avg, g.exp_avg_sq, (int)i, g.lr, g.beta1, g.beta2, g.eps, g.step);
}

extern "C" int tohip_adam_step_multi(const tohip_adam_group* groups, int32_t n_groups, void* stream_) {
    if (!groups || n_groups <= 0 || n_groups > TOHIP_ADAM_MAX_GROUPS) return TOHIP_EINVAL;
    AdamMulti a;
    int64_t nmax = 0;
    for (int i = 0; i < n_groups; ++i) {
        const tohip_adam_group& g = groups[i];
        if (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq || g.n <= 0 || g.n > 0x7fffffff || g.step < 1) return TOHIP_EINVAL;
        a.g[i] = g;
        if (g.n > nmax) nmax = g.n;
    }
    int64_t nb = (nmax + 255) / 256;
    if (nb > 1024) nb = 1024;
    k_adam_multi<<<dim3((unsigned)nb, (unsigned)n_groups), 256, 0, (hipStream_t)stream_>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_early_stop(const float* scalars, const float* loss_terms, float rewards_th, float smoothness_th,
                                float* state, int row_from_state, void* stream_) {
    if (!scalars || !loss_terms || !state) return TOHIP_EINVAL;
    k_early_stop<<<1, 64, 0, (hipStream_t)stream_>>>(scalars, loss_terms, rewards_th, smoothness_th, state, row_from_state);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
