// prior_kernels.hip — a per-point log-odds prior for ModelTraj's reward: r_i = sigmoid(lo_sum_i + prior_i), for gfx950.
//
// OctoMap accumulates the log-odds of every observation of a cell; a plan that starts from zero rewards the points a robot has
// just seen as much as those it has never seen.  The prior is what is already known: a non-negative log-odds per point (the
// model's own log-odds are >= 0 — p is clipped at 1/2 — and the integer reward sum is exact for r in [1/2, 1) only).
//
// Nothing of a step's forward changes: lo_sum is today's sum over the evaluated waypoints, and the prior is added last, one f32
// add, where the reward and its derivative r (1 - r) are taken (traj_kernels.hip: reward_block<true>, pair_sums<.., true>).  A zero
// prior gives today's bits (lo + 0 == lo).
//
//   k_prior_build     once per prior: the gather into packed order, sigmoid(prior) with exactly the reward kernel's expression (at
//                     lo_sum = 0), and per reward block the fixed-point sum of those sigmoids — the base the reward kernel's block
//                     starts from, so that it need only add fixed(r) - fixed(sigmoid(prior)) over the points a waypoint touched.
//                     A negative or non-finite entry sets a status bit.
//   k_prior_coverage  prior + lo_sum (optionally clamped: OctoMap's upper clamping threshold) to the caller's order: the fused map,
//                     which is the next plan's prior.
//
// Buffer (tohip_traj_prior_bytes): [base: TO_REWARD_BLOCKS x i64 | total i64 | pad to 2 KB] [prior f32 npad] [sigmoid f32 npad],
// both vectors in packed order, 0 at the pads.

namespace {

constexpr size_t kPriorHdr = 2048;
static_assert(TO_REWARD_BLOCKS * 8 + 8 <= kPriorHdr, "the prior's header holds the block bases and their total");

inline size_t prior_bytes(int64_t n) { return n > 0 ? kPriorHdr + 8 * (size_t)tohip_padded_points(n) : 0; }

inline PriorView prior_view(const void* buf, int64_t n) {
    const int64_t npad = tohip_padded_points(n);
    const char* b = (const char*)buf;
    return PriorView{(const long long*)b, (const float*)(b + kPriorHdr), (const float*)(b + kPriorHdr) + npad};
}

#define TO_PRIOR_NEG 1       // status bits
#define TO_PRIOR_NONFINITE 2

// the reward kernel's partition (block bx of nbx, 1024 threads, four points a thread, stride nbx * 4096) so that base[bx] is the
// sum over exactly the points that block of the reward kernel visits
__global__ void __launch_bounds__(TO_SP_THREADS)
k_prior_build(const float* __restrict__ prior_in, const int* __restrict__ perm, int64_t n, int shift, long long* __restrict__ base,
              float* __restrict__ prior, float* __restrict__ sig, int32_t* __restrict__ status) {
    __shared__ long long lds[TO_SP_WAVES];
    long long s = 0;
    int bad = 0;
    const int64_t stride = (int64_t)gridDim.x * TO_SP_THREADS * 4;
    for (int64_t i0 = ((int64_t)blockIdx.x * TO_SP_THREADS + threadIdx.x) * 4; i0 < n; i0 += stride) {
        const int4 o4 = *reinterpret_cast<const int4*>(perm + i0);   // npad is a multiple of 2048: aligned, in bounds
        const int o[4] = {o4.x, o4.y, o4.z, o4.w};
        float p[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < n) {
                p[j] = prior_in[o[j]];
                if (!(p[j] >= 0.f)) bad |= TO_PRIOR_NEG;   // (a NaN as well)
                if (!(p[j] < INFINITY)) bad |= TO_PRIOR_NONFINITE;
                g[j] = reward_sigmoid(0.0f + p[j]);   // reward_block<true>'s r at lo_sum = 0
                s += reward_fixed(g[j], shift);
            }
        }
        *reinterpret_cast<float4*>(prior + i0) = make_float4(p[0], p[1], p[2], p[3]);
        *reinterpret_cast<float4*>(sig + i0) = make_float4(g[0], g[1], g[2], g[3]);
    }
    for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
    for (int sh = 32; sh > 0; sh >>= 1) bad |= __shfl_xor(bad, sh);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        lds[wave] = s;
        if (bad) atomicOr(status, bad);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long tot = 0;
    for (int w = 0; w < TO_SP_WAVES; ++w) tot += lds[w];
    base[blockIdx.x] = tot;
    atomicAdd(reinterpret_cast<unsigned long long*>(base + TO_REWARD_BLOCKS), (unsigned long long)tot);   // the total (integer: any order)
}

// thread per four packed positions: out[perm[i]] = min(lo_sum[i] + prior[i], clamp_max) (a NaN stays NaN)
__global__ void __launch_bounds__(256)
k_prior_coverage(const float* __restrict__ lo_sum, const float* __restrict__ prior, const int* __restrict__ perm, int64_t n, float clamp_max,
                 float* __restrict__ out) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const float4 l4 = *reinterpret_cast<const float4*>(lo_sum + i0);
    const float4 p4 = prior ? *reinterpret_cast<const float4*>(prior + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int4 o4 = *reinterpret_cast<const int4*>(perm + i0);
    const float v[4] = {prior ? p4.x + l4.x : l4.x, prior ? p4.y + l4.y : l4.y, prior ? p4.z + l4.z : l4.z, prior ? p4.w + l4.w : l4.w};
    const int o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) out[o[j]] = v[j] > clamp_max ? clamp_max : v[j];
}

}  // namespace

extern "C" size_t tohip_traj_prior_bytes(int64_t n_points) { return prior_bytes(n_points); }

extern "C" int tohip_traj_prior_build(const void* packed, int64_t n, const float* prior, void* prior_buf, size_t prior_buf_bytes,
                                      int32_t* status, void* stream_) {
    if (!packed || !prior || !prior_buf || !status || n <= 0) return TOHIP_EINVAL;
    if (prior_buf_bytes < prior_bytes(n)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const CloudView cv = cloud_view(packed, n);
    hipError_t e = hipMemsetAsync(prior_buf, 0, prior_bytes(n), st);   // the total, and the vectors' pads
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const PriorView pv = prior_view(prior_buf, n);
    k_prior_build<<<reward_blocks(n), TO_SP_THREADS, 0, st>>>(prior, cv.perm, n, reward_shift(n), const_cast<long long*>(pv.base),
                                                              const_cast<float*>(pv.prior), const_cast<float*>(pv.sig), status);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_traj_reward_prior(const void* packed, const float* lo_sum, int64_t n, float eps, int prefilled, float* rewards,
                                       float* scalars, void* workspace, size_t workspace_bytes, const void* prior_buf, void* stream_) {
    if (!prior_buf) return tohip_traj_reward(packed, lo_sum, n, eps, prefilled, rewards, scalars, workspace, workspace_bytes, stream_);
    if (!packed || !lo_sum || !rewards || !scalars || !workspace || n <= 0 || prefilled) return TOHIP_EINVAL;
    if (workspace_bytes < sizeof(RewardAcc)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const CloudView cv = cloud_view(packed, n);
    TO_PROF(TOHIP_PROF_REWARD, st);
    k_traj_reward_prior<<<reward_blocks(n), TO_SP_THREADS, 0, st>>>(lo_sum, cv.perm, n, cv.npad, eps, reward_shift(n), rewards,
                                                                    (RewardAcc*)workspace, scalars, prior_view(prior_buf, n));
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_traj_reward_backward_prior(const void* packed, int64_t n, int64_t W, const tohip_camera* cam, const tohip_rig* rig,
                                                int flags, const uint32_t* occlusion_bits, const float* lo_sum, float eps, int prefilled,
                                                float* rewards, float* scalars, const float* gout, float* poses_grad, float* quats_grad,
                                                void* workspace, size_t workspace_bytes, const void* prior_buf, void* stream_) {
    if (!prior_buf)
        return tohip_traj_reward_backward(packed, n, W, cam, rig, flags, occlusion_bits, lo_sum, eps, prefilled, rewards, scalars, gout,
                                          poses_grad, quats_grad, workspace, workspace_bytes, stream_);
    if (!rewards || !scalars || !gout || prefilled) return TOHIP_EINVAL;
    const FusedReward f{eps, 0, rewards, scalars};
    const PriorView pv = prior_view(prior_buf, n > 0 ? n : 1);
    return traj_backward_impl(packed, n, W, 1, cam, rig, flags, occlusion_bits, const_cast<float*>(lo_sum), nullptr, scalars, gout, poses_grad,
                              quats_grad, workspace, workspace_bytes, stream_, &f, &pv);
}

extern "C" int tohip_traj_backward_prior(const void* packed, int64_t n, int64_t W, const tohip_camera* cam, const tohip_rig* rig, int flags,
                                         const uint32_t* occlusion_bits, const float* lo_sum, const float* grad_rewards, const float* scalars,
                                         const float* gout, float* poses_grad, float* quats_grad, void* workspace, size_t workspace_bytes,
                                         const void* prior_buf, void* stream_) {
    if (!prior_buf)
        return tohip_traj_backward(packed, n, W, cam, rig, flags, occlusion_bits, lo_sum, grad_rewards, scalars, gout, poses_grad,
                                   quats_grad, workspace, workspace_bytes, stream_);
    const PriorView pv = prior_view(prior_buf, n > 0 ? n : 1);
    return traj_backward_impl(packed, n, W, 1, cam, rig, flags, occlusion_bits, const_cast<float*>(lo_sum), grad_rewards, scalars, gout,
                              poses_grad, quats_grad, workspace, workspace_bytes, stream_, nullptr, &pv);
}

extern "C" int tohip_traj_coverage(const void* packed, int64_t n, const float* lo_sum, const void* prior_buf, float clamp_max, float* out,
                                   void* stream_) {
    if (!packed || !lo_sum || !out || n <= 0 || !(clamp_max >= 0.f)) return TOHIP_EINVAL;   // (no threshold: +inf)
    hipStream_t st = (hipStream_t)stream_;
    const CloudView cv = cloud_view(packed, n);
    const int64_t blocks = (n + 1023) / 1024;
    k_prior_coverage<<<(unsigned)blocks, 256, 0, st>>>(lo_sum, prior_buf ? prior_view(prior_buf, n).prior : nullptr, cv.perm, n, clamp_max, out);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
