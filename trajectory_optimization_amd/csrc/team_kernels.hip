// team_kernels.hip — team coverage: B robots over one cloud, optimised in the same steps behind ONE reward, for gfx950.
//
// The team's visibility term is the existing forward / reward / backward over the members' evaluated waypoints laid end to end as one
// trajectory (n_traj = 1).  What is per member behind that one reward lives here:
//
//   k_team_step_tail     block b = member b: the block k_traj_step_tail runs for a trajectory (opt_step.hpp's tail_gradients and tail_adam:
//                        scatter of the visibility rows, regularisers and clearance rows, Adam) against ONE scalars row; its own are the
//                        team total, the TEAM's early-stop rule and the terms of the positions it leaves
//   k_team_loss          block b = member b: criterion's terms and the regularisers' gradient rows of every member, and the team total
//   k_team_member_gains  one pass over the members' log-odds rows: what each member adds to the team's mean reward
//
// The early stop needs every member's smoothness of THIS step, and no block may wait for another inside a launch.  A member's terms
// depend on its positions only, and those are final when its block's Adam update is done: the block then evaluates the terms of the
// positions it has just written (one forward evaluation more, beside the other members' blocks, not O(B W) in one) and leaves them in
// row i + 1 of a per-step log.  Step i reads row i of every member — written by the launch before, or by k_team_loss before the
// first step — and writes row i + 1: the decision is taken in the step it belongs to, by every block from the same numbers.
// (The alternative, one block summing all B members' regularisers, puts O(B W) f64 work in series into the step's tail.)
//
//   team state (tohip_team_state_bytes): [state: (n_steps + 1, B, 8) f32] [terms: (n_steps + 1, B, 4) f64 = l2, length, smooth, -]
//   state row: opt_step.hpp's ([0] reward0 of the team, [1] the member's smooth0, [2] stopped, [3] steps, [4] visibility gain,
//   [5] the member's smooth gain)
#include "common.hpp"
#include "opt_step.hpp"

namespace {

struct TeamTail : TailArgs {     // (scalars: the TEAM's one row; pg_eval / qg_eval: the team's visibility rows, member b's at b * n_eval)
    const float* state_in;           // (B, 8): this step's rows
    float* state_out;                //   ... and the next step's
    const double* terms_in;          // (B, 4): every member's l2, length, smooth at its current positions
    double* terms_out;               //   ... and at the positions this step leaves
    int B;
};

__global__ void __launch_bounds__(TO_BLOCK) k_team_step_tail(TeamTail a) {
    __shared__ double lds[TO_BLOCK / 64];
    __shared__ double sh[4];
    __shared__ double clrs[TO_BLOCK];   // every member's clearance term (B <= TO_BLOCK)
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float* in = a.state_in + b * TO_OPT_STATE;
    if (a.clr && t < a.B) clrs[t] = clearance_sum(a.clr_term + (int64_t)t * a.W, a.W, a.clr_w);   // thread m: member m's, each the one-thread sum
    // the member's own terms and rows: the trajectory tail's block (its first barrier also publishes clrs)
    const TailArgs r = tail_block(a, b);
    const RegOut o = tail_gradients(r, lds, sh);
    const bool stopped = in[2] != 0.f;   // before this step (uniform, and the same in every block)
    if (t == 0) {
        // the team total: vis, then every member's l2, length, smooth [, clearance], members ascending — one running f64 sum, rounded
        // once; and whether every OTHER member's smooth gain passes (this member's own is early_stop_next's)
        const double vis = (double)a.scalars[1];
        double tot = vis;
        bool others = true;
        for (int m = 0; m < a.B; ++m) {
            const double* p = a.terms_in + (int64_t)m * 4;
            if (m == (int)b) {
                tot += o.l2; tot += o.length; tot += o.smooth;
            } else {
                tot += p[0]; tot += p[1]; tot += p[2];
                const float sm = (float)p[2];
                const float s0 = in[3] == 0.f ? sm : a.state_in[(int64_t)m * TO_OPT_STATE + 1];   // the first step sets smooth0
                others = others && (s0 / sm > a.smoothness_th);
            }
            if (a.clr) tot += clrs[m];
        }
        if (!stopped) {
            float* row = a.loss_log + b * a.log_stride + 8 * (int)in[3];
            row[0] = (float)vis; row[1] = (float)o.l2; row[2] = (float)o.length; row[3] = (float)o.smooth; row[4] = (float)tot;
            if (a.clr) row[5] = (float)clrs[b];
        }
        // the rule itself: the member's own gain against the threshold, the others' through a threshold nothing passes.  The own
        // smoothness is taken from the row the OTHER blocks read of this member (the same bits as o.smooth: same device function, same
        // inputs, no FMA contraction; tests/test_hip_team.py checks it), so that every block decides from the same numbers by construction
        early_stop_next(in, a.state_out + b * TO_OPT_STATE, a.scalars[0], (float)a.terms_in[b * 4 + 2], a.rewards_th,
                        others ? a.smoothness_th : INFINITY);
    }
    if (!stopped) tail_adam(r, (int)in[3] + 1);
    __syncthreads();
    // the terms of the positions this step leaves: what the next step's blocks read of this member
    const RegOut nx = regularizers_eval(r.poses, r.poses0, a.W, a.smooth_w, a.length_w, a.eps, nullptr, 0, nullptr, lds, sh);
    if (t == 0) {
        double* p = a.terms_out + b * 4;
        p[0] = nx.l2; p[1] = nx.length; p[2] = nx.smooth; p[3] = 0.0;
    }
}

struct TeamLoss {
    const float *poses, *poses0;
    const float* scalars;      // NULL, or the team's ([1] = loss_vis)
    const double* clr_term;    // NULL, or (B W) per-waypoint clearance terms
    float* terms;              // (B, 8): [0] vis [1] l2 [2] length [3] smooth [5] clearance
    double* terms64;           // NULL, or (B, 4): l2, length, smooth, -
    float* total;              // NULL, or the team total
    float* grad;               // NULL, or (B W, 3): the regularisers' gradient rows
    float* grad_terms;         // NULL, or (B, 3, W, 3): d l2, d length, d smooth of each member
    int W, B;
    float smooth_w, length_w, eps, clr_w;
};

__global__ void __launch_bounds__(TO_BLOCK) k_team_loss(TeamLoss a) {
    __shared__ double lds[TO_BLOCK / 64];
    __shared__ double sh[4];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const RegOut o = regularizers_eval(a.poses + b * a.W * 3, a.poses0 + b * a.W * 3, a.W, a.smooth_w, a.length_w, a.eps,
                                       a.grad ? a.grad + b * a.W * 3 : nullptr, 0, a.grad_terms ? a.grad_terms + b * a.W * 9 : nullptr, lds, sh);
    const double vis = a.scalars ? (double)a.scalars[1] : 0.0;
    double tot = 0.0;
    if (t == 0) {
        const double clr = a.clr_term ? clearance_sum(a.clr_term + b * a.W, a.W, a.clr_w) : 0.0;
        float* row = a.terms + b * 8;
        row[0] = (float)vis; row[1] = (float)o.l2; row[2] = (float)o.length; row[3] = (float)o.smooth; row[4] = 0.f;
        row[5] = (float)clr; row[6] = 0.f; row[7] = 0.f;
        if (a.terms64) { double* p = a.terms64 + b * 4; p[0] = o.l2; p[1] = o.length; p[2] = o.smooth; p[3] = 0.0; }
        tot = vis; tot += o.l2; tot += o.length; tot += o.smooth;
        if (a.clr_term) tot += clr;
    }
    if (b != 0 || !a.total) return;   // (uniform)
    // block 0 alone takes the other members' terms again (forward sums only) for the total: nothing here waits for another block
    for (int m = 1; m < a.B; ++m) {
        __syncthreads();
        const RegOut om = regularizers_eval(a.poses + (int64_t)m * a.W * 3, a.poses0 + (int64_t)m * a.W * 3, a.W, a.smooth_w, a.length_w,
                                            a.eps, nullptr, 0, nullptr, lds, sh);
        if (t == 0) {
            tot += om.l2; tot += om.length; tot += om.smooth;
            if (a.clr_term) tot += clearance_sum(a.clr_term + (int64_t)m * a.W, a.W, a.clr_w);
        }
    }
    if (t == 0) a.total[0] = (float)tot;
}

// sums: [0] fixed sum of the team's rewards sigmoid(S + prior), [1 + b] of sigmoid(S - lo_b + prior), [1 + B + b] the points with
// lo_b > 0; S = the members' log-odds summed in member order, f32.  A member whose row is NaN — one of its waypoints sees nothing at
// all, max p == min p, which makes the reference's rewards NaN — counts as absent: its log-odds are taken as 0, it adds nothing.
// Thread per four packed positions, grid-strided; NB >= B accumulators a thread, in registers.
template <int NB>
__global__ void __launch_bounds__(TO_BLOCK)
k_team_member_gains(const float* __restrict__ lo, int64_t n, int64_t npad, int B, const float* __restrict__ prior, int shift,
                    long long* __restrict__ sums) {
    __shared__ long long lds[TO_BLOCK / 64][2 * NB + 1];
    long long team = 0, without[NB];
    int count[NB];
#pragma unroll
    for (int m = 0; m < NB; ++m) { without[m] = 0; count[m] = 0; }
    const int64_t stride = (int64_t)gridDim.x * TO_BLOCK * 4;
    for (int64_t i0 = ((int64_t)blockIdx.x * TO_BLOCK + threadIdx.x) * 4; i0 < n; i0 += stride) {   // npad is a multiple of 2048: aligned, in bounds
        float v[NB][4];
        float S[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            if (m < B) {
                const float4 l4 = *reinterpret_cast<const float4*>(lo + (int64_t)m * npad + i0);
                v[m][0] = l4.x; v[m][1] = l4.y; v[m][2] = l4.z; v[m][3] = l4.w;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (v[m][j] != v[m][j]) v[m][j] = 0.f;
                    S[j] += v[m][j];
                }
            }
        }
        float p[4] = {0.f, 0.f, 0.f, 0.f};
        if (prior) { const float4 p4 = *reinterpret_cast<const float4*>(prior + i0); p[0] = p4.x; p[1] = p4.y; p[2] = p4.z; p[3] = p4.w; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j >= n) continue;
            const float lt = prior ? S[j] + p[j] : S[j];
            const long long fr = reward_fixed(reward_sigmoid(lt), shift);
            team += fr;
#pragma unroll
            for (int m = 0; m < NB; ++m) {
                if (m < B) {
                    const float lm = v[m][j];
                    if (lm > 0.f) count[m] += 1;
                    if (lm == 0.f) { without[m] += fr; continue; }   // S - 0 is S: the same reward, to the bit
                    const float lw = prior ? (S[j] - lm) + p[j] : S[j] - lm;
                    without[m] += reward_fixed(reward_sigmoid(lw), shift);
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = 32; s > 0; s >>= 1) team += __shfl_xor(team, s);
    if (lane == 0) lds[wave][0] = team;
#pragma unroll
    for (int m = 0; m < NB; ++m) {
        if (m < B) {
            long long w = without[m], c = count[m];
            for (int s = 32; s > 0; s >>= 1) { w += __shfl_xor(w, s); c += __shfl_xor(c, s); }
            if (lane == 0) { lds[wave][1 + m] = w; lds[wave][1 + NB + m] = c; }
        }
    }
    __syncthreads();
    // one integer atomic per block and sum (integers: any order gives the same bits)
    const int k = threadIdx.x;
    if (k > 2 * B) return;
    const int col = k == 0 ? 0 : (k <= B ? k : 1 + NB + (k - 1 - B));
    long long tot = 0;
    for (int w = 0; w < TO_BLOCK / 64; ++w) tot += lds[w][col];
    atomicAdd(reinterpret_cast<unsigned long long*>(sums + k), (unsigned long long)tot);
}

inline size_t team_state_bytes(int64_t B, int64_t n_steps) { return B > 0 && n_steps > 0 ? (size_t)64 * B * (n_steps + 1) : 0; }
inline size_t team_gains_bytes(int64_t B) { return B > 0 ? (size_t)8 * (1 + 2 * B) : 0; }

}  // namespace

extern "C" size_t tohip_team_state_bytes(int64_t n_members, int64_t n_steps) { return team_state_bytes(n_members, n_steps); }

extern "C" size_t tohip_team_member_gains_bytes(int64_t n_members) { return team_gains_bytes(n_members); }

extern "C" int tohip_team_step_tail(float* poses, float* quats, const float* poses0, int64_t W, int64_t n_members,
                                    const float* poses_grad_eval, const float* quats_grad_eval, int64_t n_eval, int step, float* poses_grad,
                                    float* quats_grad, float* exp_avg_p, float* exp_avg_sq_p, float* exp_avg_q, float* exp_avg_sq_q,
                                    float smoothness_weight, float traj_length_weight, float eps, float lr_pose, float lr_quat, float beta1,
                                    float beta2, float adam_eps, float rewards_th, float smoothness_th, const float* scalars,
                                    float* loss_log, int64_t loss_log_stride, void* team_state, size_t team_state_bytes_, int32_t n_steps,
                                    int32_t step_index, float clearance_weight, const float* clearance_grad,
                                    const double* clearance_terms, void* stream_) {
    TeamTail a;
    tail_args_fill(a, poses, quats, poses0, W, poses_grad_eval, quats_grad_eval, n_eval, step, poses_grad, quats_grad, exp_avg_p, exp_avg_sq_p,
                   exp_avg_q, exp_avg_sq_q, smoothness_weight, traj_length_weight, eps, lr_pose, lr_quat, beta1, beta2, adam_eps, rewards_th,
                   smoothness_th, scalars, loss_log, loss_log_stride, clearance_weight, clearance_grad, clearance_terms);
    if (!tail_args_ok(a, W, n_eval, n_members) || !team_state || W > (1 << 24) || n_members > TOHIP_TEAM_MAX_MEMBERS || n_steps <= 0 ||
        step_index < 0 || step_index >= n_steps || (n_members > 1 && loss_log_stride < 8 * (int64_t)n_steps))
        return TOHIP_EINVAL;
    if (team_state_bytes_ < team_state_bytes(n_members, n_steps)) return TOHIP_ENOSPC;
    float* state = (float*)team_state;
    double* terms = (double*)((char*)team_state + (size_t)32 * n_members * (n_steps + 1));
    a.state_in = state + (int64_t)step_index * n_members * TO_OPT_STATE;
    a.state_out = state + (int64_t)(step_index + 1) * n_members * TO_OPT_STATE;
    a.terms_in = terms + (int64_t)step_index * n_members * 4;
    a.terms_out = terms + (int64_t)(step_index + 1) * n_members * 4;
    a.B = (int)n_members;
    k_team_step_tail<<<(int)n_members, TO_BLOCK, 0, (hipStream_t)stream_>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_team_loss(const float* poses, const float* poses0, int64_t W, int64_t n_members, float smoothness_weight,
                               float traj_length_weight, float eps, const float* scalars, float clearance_weight,
                               const double* clearance_terms, float* member_terms, double* member_terms64, float* total,
                               float* grad_poses, float* grad_terms, void* stream_) {
    if (!poses || !poses0 || !member_terms || W < 3 || W > (1 << 24) || n_members <= 0 || n_members > TOHIP_TEAM_MAX_MEMBERS ||
        (total && !scalars) || (clearance_terms && (!std::isfinite(clearance_weight) || !(clearance_weight >= 0.f))))
        return TOHIP_EINVAL;
    TeamLoss a;
    a.poses = poses; a.poses0 = poses0; a.scalars = scalars; a.clr_term = clearance_terms; a.terms = member_terms;
    a.terms64 = member_terms64; a.total = total; a.grad = grad_poses; a.grad_terms = grad_terms;
    a.W = (int)W; a.B = (int)n_members;
    a.smooth_w = smoothness_weight; a.length_w = traj_length_weight; a.eps = eps; a.clr_w = clearance_terms ? clearance_weight : 0.f;
    k_team_loss<<<(int)n_members, TO_BLOCK, 0, (hipStream_t)stream_>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_team_member_gains(const void* packed, int64_t n, const float* lo_members, int64_t n_members, const void* prior_buf,
                                       int64_t* sums, size_t sums_bytes, void* stream_) {
    if (!packed || !lo_members || !sums || n <= 0 || n_members <= 0 || n_members > TOHIP_TEAM_MAX_GAINS) return TOHIP_EINVAL;
    if (sums_bytes < team_gains_bytes(n_members)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(sums, 0, team_gains_bytes(n_members), st);
    if (e != hipSuccess) return (int)e;
    const int64_t npad = tohip_padded_points(n);
    const float* prior = prior_buf ? prior_view(prior_buf, n).prior : nullptr;
    int64_t blocks = (n + 4 * TO_BLOCK - 1) / (4 * TO_BLOCK);
    if (blocks > 2048) blocks = 2048;
    const int B = (int)n_members, shift = reward_shift(n);
    long long* out = reinterpret_cast<long long*>(sums);
    if (B <= 2) k_team_member_gains<2><<<(unsigned)blocks, TO_BLOCK, 0, st>>>(lo_members, n, npad, B, prior, shift, out);
    else if (B <= 4) k_team_member_gains<4><<<(unsigned)blocks, TO_BLOCK, 0, st>>>(lo_members, n, npad, B, prior, shift, out);
    else if (B <= 8) k_team_member_gains<8><<<(unsigned)blocks, TO_BLOCK, 0, st>>>(lo_members, n, npad, B, prior, shift, out);
    else k_team_member_gains<16><<<(unsigned)blocks, TO_BLOCK, 0, st>>>(lo_members, n, npad, B, prior, shift, out);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
