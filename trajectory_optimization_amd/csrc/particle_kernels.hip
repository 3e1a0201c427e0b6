// particle_kernels.hip — Monte Carlo localisation on the evidence map ("Particle filter"), for gfx950: N pose hypotheses
// carried from scan to scan — seeded, moved by odometry with noise, weighed by scan matching's score, resampled — with the state on the
// device, integers only and nothing read back.  Included right after scanmatch_kernels.hip: the geometry, the coordinate rule, the
// brick layout and the pose convention are the map layer's and scan matching's (OccGeom, occ_locate, occ_word, occ_bit, scan_voxel,
// evid_check).
//
// STATE: (N, 4) int32 — X, Y, Z in 1/256 voxel from the map's origin, |.| <= 2^24 - 1 (exact in f32), and a heading h in [0, 16384),
// 1/16384 turn about world z.  LOG-WEIGHT: (N) int64, Q16 log2, <= 0, floored at -2^40.  TABLES: int32 words the host builds once in
// f64 — TRIG (16384 x 2: round(32768 cos), round(32768 sin)) at word 0, GAUSS (1025 knots of a Q12 standard normal) at word 32768,
// EXP2 (256: round(2^20 2^(-j/256))) at word 33796.  RANDOM NUMBERS: Philox4x32-10, key (seed_lo, seed_hi), counter (particle, 0,
// step, stream) — streams 0 Gaussian seeding, 1 predict, 2 the resample offset (particle 0), 3 seeding from positions; the four words
// serve x, y, z and heading.
//
//   k_mcl_seed_gaussian / k_mcl_seed_positions / k_mcl_predict / k_mcl_poses   one lane per particle, Philox in registers.
//   k_mcl_weigh       the hot path.  A lane owns a PARTICLE and keeps its 12-float pose in registers; the scan goes through LDS in
//                     tiles of 256 points, one float4 each, which every lane reads at the same address — a broadcast, no bank
//                     conflict — and the lane adds the value of the voxel each point falls in into its own integer sums: nothing
//                     crosses lanes.  The evidence byte is loaded unconditionally (byte 0 where the voxel lies outside dims, and
//                     not used), so that the unrolled body's gathers are in flight together.  Where N alone does not fill the
//                     device the tiles are split over gridDim.y and the sums go out with one integer atomic per lane and counter
//                     into zeroed outputs, consecutive lanes to consecutive addresses; one grid row stores them.
//   k_mcl_logw / k_mcl_weights / k_mcl_record   log-weight += score beta_q and the block maxima; maximum subtracted, floor, EXP2 and
//                     the blocks' sums; one block folds at most 1024 blocks' sums into the record.  Integer sums, fixed shape.
//   k_mcl_scan_blocks / k_mcl_scan_top / k_mcl_scan_apply   the inclusive prefix sum of at most 2^20 uint64 in three plain launches:
//                     1024 elements a block, one block over at most 1024 block sums, then the offsets added.  No block waits for
//                     another block of its launch.
//   k_mcl_pick        one lane per output j: the verdict from the record, t_j = (j S1 + r) div N, a binary search in the prefix
//                     sums, the row copy into the second state buffer.
//
// No float atomics, no process-wide state, nothing read back; every argument check returns before anything is enqueued.
#include <climits>

namespace {

constexpr long long kMclMaxN = 1ll << 20;
constexpr int kMclTrig = 0, kMclGauss = 32768, kMclExp2 = 33796;
constexpr int kMclClamp = (1 << 24) - 1;
constexpr int kMclMaxSigma = 1 << 24;
constexpr long long kMclFloor = -(1ll << 40);
constexpr int kMclChunk = 1024;            // elements a block of the reductions and of the prefix sum takes: 256 lanes x 4
constexpr int kMclPartial = 8;             // int64 words a block leaves: S1, S2, sums of w X, w Y, w Z, w cos, w sin, lowest best index
constexpr int kMclWsMax = 0, kMclWsPartial = 1024, kMclWsScan = 1024 + 1024 * kMclPartial;   // the workspace's int64 words
constexpr int kMclWeighBlocks = 2048;      // blocks a weigh launch aims at (eight per CU)

struct MclKey {
    unsigned lo, hi, step;
};
struct MclAttitude {
    float a[9];
};
struct MclVec4 {
    int v[4];
};

__device__ __forceinline__ void mcl_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// a Q12 standard normal from a 32-bit word, times sigma_q8 / 256, rounded: state units
__device__ __forceinline__ int mcl_noise(const int* __restrict__ tables, unsigned u, int sigma_q8) {
    const int i = (int)(u >> 22), f = (int)((u >> 6) & 0xFFFFu);
    const long long g = ((long long)tables[kMclGauss + i] * (65536 - f) + (long long)tables[kMclGauss + i + 1] * f) >> 16;
    return (int)((g * sigma_q8 + (1ll << 19)) >> 20);
}

__device__ __forceinline__ int mcl_clamp(long long v) { return (int)(v < -kMclClamp ? -kMclClamp : (v > kMclClamp ? kMclClamp : v)); }

// the 12 f32 of scan matching for one particle: R = Rz(h) A, t = X r / 256 + origin
__device__ __forceinline__ void mcl_pose(const int* __restrict__ tables, const OccGeom& g, const MclAttitude& A, int X, int Y, int Z, int h,
                                         float (&T)[12]) {
    h &= 16383;
    const float c = (float)tables[kMclTrig + 2 * h] * (1.f / 32768.f), s = (float)tables[kMclTrig + 2 * h + 1] * (1.f / 32768.f);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        T[j] = __fsub_rn(__fmul_rn(c, A.a[j]), __fmul_rn(s, A.a[3 + j]));
        T[3 + j] = __fadd_rn(__fmul_rn(s, A.a[j]), __fmul_rn(c, A.a[3 + j]));
        T[6 + j] = A.a[6 + j];
    }
    const float r256 = g.r * (1.f / 256.f);
    T[9] = __fadd_rn(__fmul_rn((float)X, r256), g.ox);
    T[10] = __fadd_rn(__fmul_rn((float)Y, r256), g.oy);
    T[11] = __fadd_rn(__fmul_rn((float)Z, r256), g.oz);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_seed_gaussian(int* __restrict__ state, long long* __restrict__ log_weight, int n, const int* __restrict__ tables, MclVec4 prior,
                    MclVec4 sigma, MclKey key) {
    const int i = blockIdx.x * TO_BLOCK + threadIdx.x;
    if (i >= n) return;
    unsigned u[4];
    mcl_philox((unsigned)i, 0u, key.step, 0u, key.lo, key.hi, u);
    int4 s;
    s.x = mcl_clamp((long long)prior.v[0] + mcl_noise(tables, u[0], sigma.v[0]));
    s.y = mcl_clamp((long long)prior.v[1] + mcl_noise(tables, u[1], sigma.v[1]));
    s.z = mcl_clamp((long long)prior.v[2] + mcl_noise(tables, u[2], sigma.v[2]));
    s.w = (prior.v[3] + mcl_noise(tables, u[3], sigma.v[3])) & 16383;
    reinterpret_cast<int4*>(state)[i] = s;
    log_weight[i] = 0;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_seed_positions(int* __restrict__ state, long long* __restrict__ log_weight, int n, OccGeom g, const float* __restrict__ positions,
                     unsigned m, int jitter, MclKey key) {
    const int i = blockIdx.x * TO_BLOCK + threadIdx.x;
    if (i >= n) return;
    unsigned u[4];
    mcl_philox((unsigned)i, 0u, key.step, 3u, key.lo, key.hi, u);
    const float* p = positions + 3ll * (u[0] % m);
    int x, y, z;
    (void)occ_locate(g, p, x, y, z);   // (a row out of range: the voxel of fixed point 0 on that axis)
    const int jx = jitter ? (int)(u[1] >> 24) : 128, jy = jitter ? (int)((u[1] >> 16) & 0xFFu) : 128, jz = jitter ? (int)(u[2] >> 24) : 128;
    reinterpret_cast<int4*>(state)[i] = make_int4(x * 256 + jx, y * 256 + jy, z * 256 + jz, (int)(u[3] >> 18));
    log_weight[i] = 0;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_predict(int* __restrict__ state, int n, const int* __restrict__ tables, MclVec4 delta, MclVec4 sigma, MclKey key) {
    const int i = blockIdx.x * TO_BLOCK + threadIdx.x;
    if (i >= n) return;
    unsigned u[4];
    mcl_philox((unsigned)i, 0u, key.step, 1u, key.lo, key.hi, u);
    int4 s = reinterpret_cast<int4*>(state)[i];
    const int h = s.w & 16383;
    const long long c = tables[kMclTrig + 2 * h], sn = tables[kMclTrig + 2 * h + 1];
    const long long nx = (long long)delta.v[0] + mcl_noise(tables, u[0], sigma.v[0]);
    const long long ny = (long long)delta.v[1] + mcl_noise(tables, u[1], sigma.v[1]);
    const long long nz = (long long)delta.v[2] + mcl_noise(tables, u[2], sigma.v[2]);
    s.x = mcl_clamp((long long)s.x + ((c * nx - sn * ny + (1ll << 14)) >> 15));
    s.y = mcl_clamp((long long)s.y + ((sn * nx + c * ny + (1ll << 14)) >> 15));
    s.z = mcl_clamp((long long)s.z + nz);
    s.w = (h + delta.v[3] + mcl_noise(tables, u[3], sigma.v[3])) & 16383;
    reinterpret_cast<int4*>(state)[i] = s;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_poses(const int* __restrict__ state, int n, const int* __restrict__ tables, OccGeom g, MclAttitude A, float* __restrict__ poses) {
    const int i = blockIdx.x * TO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int4 s = reinterpret_cast<const int4*>(state)[i];
    float T[12];
    mcl_pose(tables, g, A, s.x, s.y, s.z, s.w, T);
    float4* out = reinterpret_cast<float4*>(poses + 12ll * i);
    out[0] = make_float4(T[0], T[1], T[2], T[3]);
    out[1] = make_float4(T[4], T[5], T[6], T[7]);
    out[2] = make_float4(T[8], T[9], T[10], T[11]);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_weigh(const signed char* __restrict__ vals, OccGeom g, int floor_value, int unknown_value, const float* __restrict__ pts, int n_pts,
            const int* __restrict__ state, int n, const int* __restrict__ tables, MclAttitude A, int* __restrict__ score,
            int* __restrict__ used, int* __restrict__ known) {
    __shared__ float4 s_p[TO_BLOCK];
    const int t = threadIdx.x, i = blockIdx.x * TO_BLOCK + t;
    const bool live = i < n;
    float T[12];
    {
        const int4 s = live ? reinterpret_cast<const int4*>(state)[i] : make_int4(0, 0, 0, 0);
        mcl_pose(tables, g, A, s.x, s.y, s.z, s.w, T);
    }
    int sum = 0, n_used = 0, n_known = 0;
    const int n_tiles = (n_pts + TO_BLOCK - 1) / TO_BLOCK;
    for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        __syncthreads();   // (the tile before is read to its end)
        const int base = tile * TO_BLOCK, cnt = min(TO_BLOCK, n_pts - base);
        if (t < cnt) {
            const float* p = pts + 3ll * (base + t);
            s_p[t] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
        if (!live) continue;
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const float4 q = s_p[k];
            const float p[3] = {q.x, q.y, q.z};
            int x, y, z;
            const bool ok = scan_voxel(g, T, p, x, y, z);
            const bool in = ok && occ_inside(g, x, y, z);
            const int L = vals[in ? 32ll * occ_word(g, x, y, z) + occ_bit(x, y, z) : 0ll];
            const bool kn = in && L != kEvidUnknown;
            sum += ok ? (kn ? max(L, floor_value) : unknown_value) : 0;
            n_used += ok ? 1 : 0;
            n_known += kn ? 1 : 0;
        }
    }
    if (!live) return;
    if (gridDim.y == 1) {
        score[i] = sum, used[i] = n_used, known[i] = n_known;
    } else {
        if (sum != 0) __hip_atomic_fetch_add(score + i, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_used != 0) __hip_atomic_fetch_add(used + i, n_used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_known != 0) __hip_atomic_fetch_add(known + i, n_known, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- block-wide folds of one int64 per lane (blocks of at most 1024 lanes): the result in every lane -------------------------------
enum MclOp { kMclSum, kMclMin, kMclMax };

template <MclOp OP>
__device__ __forceinline__ long long mcl_op(long long a, long long b) {
    return OP == kMclSum ? (long long)((unsigned long long)a + (unsigned long long)b) : (OP == kMclMin ? (a < b ? a : b) : (a > b ? a : b));
}

template <MclOp OP>
__device__ __forceinline__ long long mcl_fold(long long v, long long* s_wave /* [16] */) {
    for (int sh = 32; sh > 0; sh >>= 1) v = mcl_op<OP>(v, __shfl_xor(v, sh));
    __syncthreads();   // (s_wave of the fold before is read to its end)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    const int n_waves = (int)(blockDim.x >> 6);
    long long r = s_wave[0];
    for (int w = 1; w < n_waves; ++w) r = mcl_op<OP>(r, s_wave[w]);
    return r;
}

// the exclusive prefix of one uint64 per lane over the block, and the block's total
__device__ __forceinline__ unsigned long long mcl_block_scan(unsigned long long v, unsigned long long* s_wave /* [16] */, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = (int)(blockDim.x >> 6);
    unsigned long long inc = v;
    for (int sh = 1; sh < 64; sh <<= 1) {
        const unsigned long long up = __shfl_up(inc, sh);
        if (lane >= sh) inc += up;
    }
    __syncthreads();
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned long long before = 0ull;
    total = 0ull;
    for (int w = 0; w < n_waves; ++w) {
        const unsigned long long s = s_wave[w];
        if (w < wave) before += s;
        total += s;
    }
    return before + inc - v;
}

// log_weight += score beta_q (where there are scores), and each block's maximum
__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_logw(long long* __restrict__ log_weight, int n, const int* __restrict__ score, int beta_q, long long* __restrict__ ws) {
    __shared__ long long s_wave[16];
    long long m = LLONG_MIN;
    const int base = blockIdx.x * kMclChunk + 4 * threadIdx.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = base + e;
        if (i < n) {
            long long lw = log_weight[i];
            if (score) {
                lw += (long long)score[i] * beta_q;
                log_weight[i] = lw;
            }
            m = lw > m ? lw : m;
        }
    }
    m = mcl_fold<kMclMax>(m, s_wave);
    if (threadIdx.x == 0) ws[kMclWsMax + blockIdx.x] = m;
}

__device__ __forceinline__ long long mcl_weight(const int* __restrict__ tables, long long lw) {
    const long long d = -lw, q = d >> 16;
    return q <= 20 ? (long long)(tables[kMclExp2 + (int)((d & 0xFFFF) >> 8)] >> (int)q) : 0ll;
}

// the maximum subtracted, the floor, the weights and each block's sums
__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_weights(const int* __restrict__ state, long long* __restrict__ log_weight, int n, int n_blocks, const int* __restrict__ tables,
              long long* __restrict__ weights, long long* __restrict__ ws) {
    __shared__ long long s_wave[16];
    long long m = LLONG_MIN;
    for (int b = threadIdx.x; b < n_blocks; b += TO_BLOCK) m = max(m, ws[kMclWsMax + b]);
    m = mcl_fold<kMclMax>(m, s_wave);
    long long acc[kMclPartial] = {0, 0, 0, 0, 0, 0, 0, LLONG_MAX};
    const int base = blockIdx.x * kMclChunk + 4 * threadIdx.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = base + e;
        if (i < n) {
            long long lw = log_weight[i] - m;
            lw = lw < kMclFloor ? kMclFloor : lw;
            log_weight[i] = lw;
            const long long w = mcl_weight(tables, lw);
            weights[i] = w;
            const int4 s = reinterpret_cast<const int4*>(state)[i];
            const int h = s.w & 16383;
            // (sums of w X wrap modulo 2^64 where N max|X| reaches 2^43: never with positions inside the map's range)
            acc[0] += w, acc[1] += w * w;
            acc[2] += w * s.x, acc[3] += w * s.y, acc[4] += w * s.z;
            acc[5] += w * tables[kMclTrig + 2 * h], acc[6] += w * tables[kMclTrig + 2 * h + 1];
            if (lw == 0 && i < acc[7]) acc[7] = i;
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = mcl_fold<kMclSum>(acc[k], s_wave);
    acc[7] = mcl_fold<kMclMin>(acc[7], s_wave);
    if (threadIdx.x < kMclPartial) {
        long long v = acc[0];
#pragma unroll
        for (int k = 1; k < kMclPartial; ++k) v = (int)threadIdx.x == k ? acc[k] : v;
        ws[kMclWsPartial + (long long)blockIdx.x * kMclPartial + threadIdx.x] = v;
    }
}

__device__ __forceinline__ double mcl_n_eff(long long s1, long long s2) { return (double)s1 * (double)s1 / (double)s2; }

// the blocks' sums -> the record (16 int64): S1, S2, sums of w X, w Y, w Z, w cos, w sin; the best index, its score, known and used;
// the verdict; n_eff's bits; the maximum subtracted; N; 0
__global__ void __launch_bounds__(1024)
k_mcl_record(int n, int n_blocks, const int* __restrict__ score, const int* __restrict__ used, const int* __restrict__ known,
             double threshold, const long long* __restrict__ ws, long long* __restrict__ record) {
    __shared__ long long s_wave[16];
    const int b = threadIdx.x;
    const bool live = b < n_blocks;
    long long acc[kMclPartial];
#pragma unroll
    for (int k = 0; k < kMclPartial; ++k) acc[k] = live ? ws[kMclWsPartial + (long long)b * kMclPartial + k] : (k == 7 ? LLONG_MAX : 0ll);
    long long m = live ? ws[kMclWsMax + b] : LLONG_MIN;
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = mcl_fold<kMclSum>(acc[k], s_wave);
    acc[7] = mcl_fold<kMclMin>(acc[7], s_wave);
    m = mcl_fold<kMclMax>(m, s_wave);
    if (b == 0) {
#pragma unroll
        for (int k = 0; k < kMclPartial; ++k) record[k] = acc[k];
        const int best = acc[7] < n ? (int)acc[7] : 0;   // (some log-weight is the maximum: always inside)
        record[8] = score ? score[best] : 0;
        record[9] = known ? known[best] : 0;
        record[10] = used ? used[best] : 0;
        const double n_eff = mcl_n_eff(acc[0], acc[1]);
        record[11] = n_eff < threshold ? 1 : 0;
        record[12] = __double_as_longlong(n_eff);
        record[13] = m;
        record[14] = n;
        record[15] = 0;
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_scan_blocks(const long long* __restrict__ weights, int n, unsigned long long* __restrict__ cumulative, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long s_wave[16];
    const int base = blockIdx.x * kMclChunk + 4 * threadIdx.x;
    unsigned long long v[4], mine = 0ull;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = base + e < n ? (unsigned long long)weights[base + e] : 0ull;
        mine += v[e];
    }
    unsigned long long total;
    unsigned long long run = mcl_block_scan(mine, s_wave, total);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        run += v[e];
        if (base + e < n) cumulative[base + e] = run;
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024)
k_mcl_scan_top(unsigned long long* __restrict__ sums, int n_blocks) {
    __shared__ unsigned long long s_wave[16];
    const int b = threadIdx.x;
    const unsigned long long v = b < n_blocks ? sums[b] : 0ull;
    unsigned long long total;
    const unsigned long long before = mcl_block_scan(v, s_wave, total);
    if (b < n_blocks) sums[b] = before;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_scan_apply(unsigned long long* __restrict__ cumulative, int n, const unsigned long long* __restrict__ sums) {
    const unsigned long long before = sums[blockIdx.x];
    const int base = blockIdx.x * kMclChunk + 4 * threadIdx.x;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (base + e < n) cumulative[base + e] += before;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_mcl_pick(const int* __restrict__ state, int* __restrict__ state_out, long long* __restrict__ log_weight, int n,
           const unsigned long long* __restrict__ cumulative, long long* __restrict__ record, double threshold, MclKey key,
           int* __restrict__ ancestors) {
    const int j = blockIdx.x * TO_BLOCK + threadIdx.x;
    if (j >= n) return;
    const unsigned long long s1 = (unsigned long long)record[0];
    const double n_eff = mcl_n_eff(record[0], record[1]);
    const bool resample = n_eff < threshold && s1 != 0ull;   // (S1 >= 2^20 in a record of k_mcl_record)
    int a = j;
    if (resample) {
        unsigned u[4];
        mcl_philox(0u, 0u, key.step, 2u, key.lo, key.hi, u);
        const unsigned long long r = (((unsigned long long)u[0] << 32) | u[1]) % s1;
        const unsigned long long tj = ((unsigned long long)j * s1 + r) / (unsigned long long)n;
        int lo = 0, hi = n - 1;   // (t_j < S1 = C[n - 1]: the search ends inside)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cumulative[mid] > tj) hi = mid; else lo = mid + 1;
        }
        a = lo;
        log_weight[j] = 0;
    }
    reinterpret_cast<int4*>(state_out)[j] = reinterpret_cast<const int4*>(state)[a];
    ancestors[j] = a;
    if (j == 0) {   // (words 11 and 12: no lane reads them)
        record[11] = resample ? 1 : 0;
        record[12] = __double_as_longlong(n_eff);
    }
}

inline bool mcl_n_ok(int64_t n) { return n >= 1 && n <= kMclMaxN; }
inline int mcl_blocks(int64_t n) { return (int)((n + TO_BLOCK - 1) / TO_BLOCK); }
inline int mcl_chunks(int64_t n) { return (int)((n + kMclChunk - 1) / kMclChunk); }
inline bool mcl_vec4(const int32_t* v_host, int lo, int hi, bool heading, MclVec4& out) {
    if (!v_host) return false;
    for (int a = 0; a < 4; ++a) {
        const bool ok = heading && a == 3 ? (v_host[a] >= -(1 << 30) && v_host[a] <= (1 << 30)) : (v_host[a] >= lo && v_host[a] <= hi);
        if (!ok) return false;
        out.v[a] = v_host[a];
    }
    return true;
}
inline bool mcl_attitude(const float* attitude_host, MclAttitude& A) {
    for (int k = 0; k < 9; ++k) {
        A.a[k] = attitude_host ? attitude_host[k] : (k % 4 == 0 ? 1.f : 0.f);
        if (!std::isfinite(A.a[k])) return false;
    }
    return true;
}
// the geometry alone (occ_check's rules, no buffer)
inline int mcl_geom(const tohip_occ_geom* geom, OccGeom& g) { return geom ? occ_check(geom, ~(size_t)0, geom, g) : TOHIP_EINVAL; }
inline bool mcl_threshold_ok(double threshold) { return threshold >= 0.0 && std::isfinite(threshold); }

}  // namespace

extern "C" int tohip_mcl_seed_gaussian(int32_t* state, int64_t* log_weight, int64_t n, const int32_t* tables, size_t tables_bytes,
                                       const int32_t* prior_host, const int32_t* sigma_q8_host, uint32_t seed_lo, uint32_t seed_hi,
                                       uint32_t step, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    MclVec4 prior, sigma;
    if (!mcl_n_ok(n) || !state || !log_weight || !tables || !scan_aligned(state, 16) || !scan_aligned(log_weight, 8) || !scan_aligned(tables, 4) ||
        (const void*)state == (const void*)log_weight || !mcl_vec4(prior_host, -kMclClamp, kMclClamp, true, prior) ||
        !mcl_vec4(sigma_q8_host, 0, kMclMaxSigma, false, sigma))
        return TOHIP_EINVAL;
    if (tables_bytes < TOHIP_MCL_TABLE_WORDS * sizeof(int32_t)) return TOHIP_ENOSPC;
    k_mcl_seed_gaussian<<<mcl_blocks(n), TO_BLOCK, 0, (hipStream_t)stream_>>>(state, (long long*)log_weight, (int)n, tables, prior, sigma,
                                                                             MclKey{seed_lo, seed_hi, step});
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_mcl_seed_positions(int32_t* state, int64_t* log_weight, int64_t n, const tohip_occ_geom* geom, const float* positions,
                                        int64_t m, int32_t jitter, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void* stream_,
                                        uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = mcl_geom(geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!mcl_n_ok(n) || !state || !log_weight || !positions || m < 1 || m > 0x7FFFFFFFll || (jitter != 0 && jitter != 1) ||
        !scan_aligned(state, 16) || !scan_aligned(log_weight, 8) || !scan_aligned(positions, 4) || (const void*)state == (const void*)log_weight ||
        (const void*)state == (const void*)positions || (const void*)log_weight == (const void*)positions)
        return TOHIP_EINVAL;
    k_mcl_seed_positions<<<mcl_blocks(n), TO_BLOCK, 0, (hipStream_t)stream_>>>(state, (long long*)log_weight, (int)n, g, positions, (unsigned)m,
                                                                              jitter, MclKey{seed_lo, seed_hi, step});
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_mcl_predict(int32_t* state, int64_t n, const int32_t* tables, size_t tables_bytes, const int32_t* delta_host,
                                 const int32_t* sigma_q8_host, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void* stream_,
                                 uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    MclVec4 delta, sigma;
    if (!mcl_n_ok(n) || !state || !tables || !scan_aligned(state, 16) || !scan_aligned(tables, 4) ||
        !mcl_vec4(delta_host, -kMclClamp, kMclClamp, true, delta) || !mcl_vec4(sigma_q8_host, 0, kMclMaxSigma, false, sigma))
        return TOHIP_EINVAL;
    if (tables_bytes < TOHIP_MCL_TABLE_WORDS * sizeof(int32_t)) return TOHIP_ENOSPC;
    k_mcl_predict<<<mcl_blocks(n), TO_BLOCK, 0, (hipStream_t)stream_>>>(state, (int)n, tables, delta, sigma, MclKey{seed_lo, seed_hi, step});
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_mcl_poses(const int32_t* state, int64_t n, const int32_t* tables, size_t tables_bytes, const tohip_occ_geom* geom,
                               const float* attitude_host, float* poses, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = mcl_geom(geom, g);
    if (rc != TOHIP_OK) return rc;
    MclAttitude A;
    if (!mcl_n_ok(n) || !state || !tables || !poses || !scan_aligned(state, 16) || !scan_aligned(tables, 4) || !scan_aligned(poses, 16) ||
        (const void*)poses == (const void*)state || (const void*)poses == (const void*)tables || !mcl_attitude(attitude_host, A))
        return TOHIP_EINVAL;
    if (tables_bytes < TOHIP_MCL_TABLE_WORDS * sizeof(int32_t)) return TOHIP_ENOSPC;
    k_mcl_poses<<<mcl_blocks(n), TO_BLOCK, 0, (hipStream_t)stream_>>>(state, (int)n, tables, g, A, poses);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_mcl_weigh(const void* evid, size_t evid_bytes, const tohip_occ_geom* geom, int32_t floor_value, int32_t unknown_value,
                               const float* points, int64_t p, const int32_t* state, int64_t n, const int32_t* tables, size_t tables_bytes,
                               const float* attitude_host, int32_t* score, int32_t* used, int32_t* known, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = evid_check(evid, evid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    MclAttitude A;
    if (!scan_value_ok(floor_value, unknown_value) || p < 1 || p > kScanMaxPoints || !mcl_n_ok(n) || !points || !state || !tables || !score ||
        !used || !known || !scan_aligned(state, 16) || !mcl_attitude(attitude_host, A))
        return TOHIP_EINVAL;
    const void* bufs[7] = {score, used, known, points, state, tables, evid};
    for (int i = 0; i < 7; ++i) {
        if (!scan_aligned(bufs[i], 4)) return TOHIP_EINVAL;
        for (int j = 0; j < 3; ++j)   // no output is an input or another output
            if (i > j && bufs[i] == bufs[j]) return TOHIP_EINVAL;
    }
    if (tables_bytes < TOHIP_MCL_TABLE_WORDS * sizeof(int32_t)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const int bx = mcl_blocks(n), n_tiles = (int)((p + TO_BLOCK - 1) / TO_BLOCK);
    const int per = (kMclWeighBlocks + bx - 1) / bx;   // grid rows: the launch holds about kMclWeighBlocks blocks
    const int by = per < n_tiles ? per : n_tiles;
    if (by > 1) {
        int32_t* outs[3] = {score, used, known};
        for (int i = 0; i < 3; ++i) {
            const hipError_t e = hipMemsetAsync(outs[i], 0, (size_t)n * sizeof(int32_t), st);
            if (e != hipSuccess) return (int)e;
        }
    }
    k_mcl_weigh<<<dim3((unsigned)bx, (unsigned)by), TO_BLOCK, 0, st>>>((const signed char*)evid + kEvidHdr, g, floor_value, unknown_value, points,
                                                                      (int)p, state, (int)n, tables, A, score, used, known);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_mcl_weights(const int32_t* state, int64_t* log_weight, int64_t n, const int32_t* tables, size_t tables_bytes,
                                 const int32_t* score_or_null, const int32_t* used_or_null, const int32_t* known_or_null, int32_t beta_q,
                                 double threshold, int64_t* weights, int64_t* record, void* workspace, size_t workspace_bytes, void* stream_,
                                 uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    if (!mcl_n_ok(n) || !state || !log_weight || !tables || !weights || !record || !workspace || beta_q < 1 || beta_q > 65536 ||
        !mcl_threshold_ok(threshold) || !scan_aligned(state, 16) || !scan_aligned(tables, 4) || !scan_aligned(score_or_null, 4) ||
        !scan_aligned(used_or_null, 4) || !scan_aligned(known_or_null, 4))
        return TOHIP_EINVAL;
    const void* bufs[9] = {log_weight, weights, record, workspace, state, tables, score_or_null, used_or_null, known_or_null};
    for (int i = 0; i < 9; ++i) {
        if (i < 4 && !scan_aligned(bufs[i], 8)) return TOHIP_EINVAL;
        for (int j = 0; j < 4; ++j)   // no output is an input or another output
            if (i > j && bufs[i] == bufs[j]) return TOHIP_EINVAL;
    }
    if (tables_bytes < TOHIP_MCL_TABLE_WORDS * sizeof(int32_t) || workspace_bytes < (size_t)TOHIP_MCL_WORKSPACE_BYTES) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const int nb = mcl_chunks(n);
    long long* ws = (long long*)workspace;
    k_mcl_logw<<<nb, TO_BLOCK, 0, st>>>((long long*)log_weight, (int)n, score_or_null, beta_q, ws);
    TO_HIP_CHECK_LAUNCH();
    k_mcl_weights<<<nb, TO_BLOCK, 0, st>>>(state, (long long*)log_weight, (int)n, nb, tables, (long long*)weights, ws);
    TO_HIP_CHECK_LAUNCH();
    k_mcl_record<<<1, 1024, 0, st>>>((int)n, nb, score_or_null, used_or_null, known_or_null, threshold, ws, (long long*)record);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_mcl_resample_systematic(const int32_t* state, int32_t* state_out, int64_t* log_weight, int64_t n, const int64_t* weights,
                                  int64_t* record, double threshold, uint64_t* cumulative, int32_t* ancestors, void* workspace,
                                  size_t workspace_bytes, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    if (!mcl_n_ok(n) || !state || !state_out || !log_weight || !weights || !record || !cumulative || !ancestors || !workspace ||
        !mcl_threshold_ok(threshold) || !scan_aligned(state, 16) || !scan_aligned(state_out, 16) || !scan_aligned(ancestors, 4))
        return TOHIP_EINVAL;
    const void* bufs[8] = {state_out, log_weight, record, cumulative, workspace, ancestors, state, weights};
    for (int i = 0; i < 8; ++i) {
        if (i != 0 && i != 5 && i != 6 && !scan_aligned(bufs[i], 8)) return TOHIP_EINVAL;
        for (int j = 0; j < 6; ++j)   // no output is an input or another output
            if (i > j && bufs[i] == bufs[j]) return TOHIP_EINVAL;
    }
    if (workspace_bytes < (size_t)TOHIP_MCL_WORKSPACE_BYTES) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const int nb = mcl_chunks(n);
    unsigned long long* sums = (unsigned long long*)workspace + kMclWsScan;
    k_mcl_scan_blocks<<<nb, TO_BLOCK, 0, st>>>((const long long*)weights, (int)n, (unsigned long long*)cumulative, sums);
    TO_HIP_CHECK_LAUNCH();
    k_mcl_scan_top<<<1, 1024, 0, st>>>(sums, nb);
    TO_HIP_CHECK_LAUNCH();
    k_mcl_scan_apply<<<nb, TO_BLOCK, 0, st>>>((unsigned long long*)cumulative, (int)n, sums);
    TO_HIP_CHECK_LAUNCH();
    k_mcl_pick<<<mcl_blocks(n), TO_BLOCK, 0, st>>>(state, state_out, (long long*)log_weight, (int)n, (const unsigned long long*)cumulative,
                                                  (long long*)record, threshold, MclKey{seed_lo, seed_hi, step}, ancestors);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
