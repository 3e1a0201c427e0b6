// scanreg_kernels.hip — fine scan registration on the evidence map ("Scan registration"), for gfx950: a few damped
// Gauss–Newton steps on a trilinear copy of the score table, from a pose scan matching found to one voxel, to a sub-voxel translation
// and a continuous rotation.  Included after scanmatch_kernels.hip: poses, the f32 transform rule, occ_fixed, the score table, the
// skip rule and the brick-outside-dims predicate are scan matching's.
//
// PER POINT (all integers; w the world coordinate by scan_voxel's rule, accepted by occ_fixed):
//   q = occ_fixed(w) in 1/256 voxel; c = q - 128 (voxel CENTRES are the lattice); base voxel b = c >> 8; fraction f = c & 255; weights
//   per axis w0 = 256 - f, w1 = f.  V[i][j][k]: the table byte of voxel b + (i, j, k), 128 + unknown_value outside dims.
//   M24 = sum V wx wy wz <= 255 2^24;  Gx16 = sum_jk wy wz (V[1][j][k] - V[0][j][k]), Gy16, Gz16 alike, |G16| <= 254 2^16;
//   e = (255 2^24 - M24 + 2^11) >> 12 in 1/4096 byte, 0 <= e < 2^20;  g = (G16 + 2^7) >> 8 in 1/256 byte per voxel, |g| < 2^16;
//   a = (q - q_t + 32) >> 6 in 1/4 voxel, q_t = occ_fixed(t) of the pose's translation, |a| < 2^15 (|q - q_t| < 6144 x 256);
//   j = (a x g + 2^11) >> 12, the cross product exact in int64, |a x g| < 2 x 2^15 x 2^16 = 2^32, |j| <= 2^20, unit 4 byte per radian
//   (a rotation about the sensor's position, perturbed in the WORLD frame).  Row J = (g, j).
// THE RECORD of a pose, int64[32]: [0:21] the upper triangle of H = sum J J^T, row-major; [21:27] sum J e; [27] sum e^2; [28] used;
//   [29] inside (all eight corners inside dims); [30:32] 0.
// THE BOUND.  Every entry of J and e fits 21 bits with its sign, so every product is below 2^20 x 2^20 = 2^40 in magnitude, and a sum
//   over N <= 2^22 points stays below 2^62: int64 holds every partial sum in any order, and the order does not matter to the result.
//
//   k_scan_normal  the hot path.  Grid (point tiles, B): each lane transforms one point per tile in a grid-stride loop over the
//                  tiles.  The eight bytes are four (y, z) rows of two x neighbours: within a brick word the two share a dword
//                  unless x & 3 == 3, so a row is one dword load, or two, and a funnel shift; a brick outside dims gives 128 +
//                  unknown_value from k_scan_correlate's predicate (dword 0 is loaded in its place): nothing is loaded out of bounds.
//                  The trilinear sums are factored through the four x-interpolated rows (integers: the same bits as the
//                  definition's sums).  Each of the 28 products is one 32 x 32 + 64 multiply-add into an int64 accumulator in
//                  registers.  After the block's last tile: a wave reduction, the four waves meet in LDS, one 64-bit integer atomic
//                  per non-zero sum and block.  The blocks of a frozen pose, and of a pose whose t is out of range, return at once.
//   k_scan_step    one lane per pose: accept or reject the trial pose by its record, adapt lambda, solve the damped normal
//                  equations in f64 (add, multiply, divide, compare: no sqrt, no sin or cos, nothing contracted — the file is
//                  compiled with -ffp-contract=off, and the pragma below says so again), write the next trial pose (12 f32).
//
// No float atomics, no process-wide state, nothing read back; every argument check returns before anything is enqueued.
namespace {

constexpr int kRegRecord = TOHIP_SCANREG_RECORD;   // int64 words
constexpr int kRegState = TOHIP_SCANREG_STATE;     // 8-byte words
constexpr int kRegSums = 30;                       // the record's words that are sums
constexpr int kRegMaxPoses = 256;
// the state's words (f64 unless named an integer)
constexpr int kRegT = 0, kRegQ = 3, kRegLambda = 7, kRegDelta = 8, kRegStatus = 14 /* int */, kRegIter = 15 /* int */, kRegAccepted = 16 /* int */,
              kRegTrialT = 17, kRegTrialQ = 20, kRegRec = 24 /* int[32] */;
enum { kRegRunning = 0, kRegConverged = 1, kRegStalled = 2, kRegDegenerate = 3, kRegEmpty = 4 };

__global__ void __launch_bounds__(TO_BLOCK)
k_scan_normal(const unsigned* __restrict__ table, OccGeom g, unsigned unknown4, const float* __restrict__ pts, long long n,
              const float* __restrict__ poses, const long long* __restrict__ state, long long* __restrict__ records) {
    __shared__ long long s_part[TO_WAVES_PER_BLOCK][kRegSums];
    const int t = threadIdx.x, b = blockIdx.y;
    if (state && state[(long long)b * kRegState + kRegStatus] != kRegRunning) return;   // (uniform: a frozen pose)
    const float* T = poses + 12 * (long long)b;
    int qt[3];
    if (!occ_fixed(g, T[9], T[10], T[11], qt[0], qt[1], qt[2])) return;                  // (uniform: t out of range, the record stays 0)
    long long acc[28];
#pragma unroll
    for (int s = 0; s < 28; ++s) acc[s] = 0;
    int n_used = 0, n_in = 0;
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long i = tile * TO_BLOCK + t;
        if (i >= n) continue;
        const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        float w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
            w[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[3 * a], px), __fmul_rn(T[3 * a + 1], py)), __fmul_rn(T[3 * a + 2], pz)), T[9 + a]);
        int q[3];
        if (!occ_fixed(g, w[0], w[1], w[2], q[0], q[1], q[2])) continue;
        const int cx = q[0] - 128, cy = q[1] - 128, cz = q[2] - 128;
        const int bx = cx >> 8, by = cy >> 8, bz = cz >> 8;
        const int fx = cx & 255, fy = cy & 255, fz = cz & 255;
        const int xb = bx >> 2, sh = 8 * (bx & 3);
        const bool two = (bx & 3) == 3;           // the x neighbour lies in the next brick
        int rx[2][2], dx[2][2];                   // [j][k]: the row interpolated along x (<= 255 x 256), and V[1] - V[0]
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int y = by + j, z = bz + k;
                const bool row_ok = (unsigned)y < (unsigned)g.ny && (unsigned)z < (unsigned)g.nz;
                // the row's dword of brick xb (at most 2^29 dwords a table; meaningless, and not used, where the brick lies outside dims)
                const int first = (((z >> 1) * g.nby + (y >> 2)) * g.nbx + xb) * 8 + ((y & 3) | ((z & 1) << 2));
                const bool in0 = row_ok && (unsigned)xb < (unsigned)g.nbx;
                const unsigned v0 = table[in0 ? first : 0];
                unsigned lo = in0 ? v0 : unknown4, hi = 0u;
                if (two) {
                    const bool in1 = row_ok && (unsigned)(xb + 1) < (unsigned)g.nbx;
                    const unsigned v1 = table[in1 ? first + 8 : 0];
                    hi = in1 ? v1 : unknown4;
                }
                const unsigned v = (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
                const int V0 = (int)(v & 0xFFu), V1 = (int)((v >> 8) & 0xFFu);
                rx[j][k] = V0 * (256 - fx) + V1 * fx;
                dx[j][k] = V1 - V0;
            }
        }
        const int wy[2] = {256 - fy, fy}, wz[2] = {256 - fz, fz};
        unsigned M24 = 0u;
        int G[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                M24 += (unsigned)rx[j][k] * (unsigned)(wy[j] * wz[k]);
                G[0] += dx[j][k] * (wy[j] * wz[k]);
            }
            G[1] += wz[k] * (rx[1][k] - rx[0][k]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) G[2] += wy[j] * (rx[j][1] - rx[j][0]);
        const int e = (int)(((255u << 24) - M24 + 2048u) >> 12);
        int J[6], a[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            J[c] = (G[c] + 128) >> 8;
            a[c] = (q[c] - qt[c] + 32) >> 6;
        }
        J[3] = (int)(((long long)a[1] * J[2] - (long long)a[2] * J[1] + 2048) >> 12);
        J[4] = (int)(((long long)a[2] * J[0] - (long long)a[0] * J[2] + 2048) >> 12);
        J[5] = (int)(((long long)a[0] * J[1] - (long long)a[1] * J[0] + 2048) >> 12);
        int s = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = r; c < 6; ++c) acc[s++] += (long long)J[r] * J[c];
            acc[21 + r] += (long long)J[r] * e;
        }
        acc[27] += (long long)e * e;
        ++n_used;
        n_in += (int)(bx >= 0 && bx + 1 < g.nx && by >= 0 && by + 1 < g.ny && bz >= 0 && bz + 1 < g.nz);
    }
    const int lane = t & (TO_WAVE - 1), wave = t / TO_WAVE;
#pragma unroll
    for (int s = 0; s < kRegSums; ++s) {
        long long v = s < 28 ? acc[s < 28 ? s : 0] : (long long)(s == 28 ? n_used : n_in);
        for (int m = TO_WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) s_part[wave][s] = v;
    }
    __syncthreads();
    if (t < kRegSums) {
        long long v = 0;
#pragma unroll
        for (int wv = 0; wv < TO_WAVES_PER_BLOCK; ++wv) v += s_part[wv][t];
        if (v != 0) __hip_atomic_fetch_add(records + (long long)b * kRegRecord + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#pragma clang fp contract(off)

// the damped solve over the free degrees of freedom -> false: a pivot <= 0 or not finite.  One fixed operation order (synth.scan_solve_ref)
__device__ __forceinline__ bool reg_solve(const long long* __restrict__ rec, double lam, int mask, double* __restrict__ x) {
    const double S[6] = {1.0 / 256.0, 1.0 / 256.0, 1.0 / 256.0, 4.0, 4.0, 4.0};
    double A[6][6], rhs[6], L[6][6], d[6], y[6];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const bool free_ij = ((mask >> i) & 1) && ((mask >> j) & 1);
            const double v = free_ij ? (double)rec[n] * S[i] * S[j] : (i == j ? 1.0 : 0.0);
            A[i][j] = A[j][i] = v;
            ++n;
        }
        rhs[i] = ((mask >> i) & 1) ? (double)rec[21 + i] * S[i] * (1.0 / 4096.0) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if ((mask >> i) & 1) A[i][i] = A[i][i] + lam * A[i][i];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double v = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) v = v - L[j][k] * (L[j][k] * d[k]);
        if (!(v > 0.0) || !(v < __builtin_inf())) return false;
        d[j] = v;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double u = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) u = u - L[i][k] * (L[j][k] * d[k]);
            L[i][j] = u / v;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
        x[i] = v;
    }
    return true;
}

__global__ void __launch_bounds__(TO_WAVE)
k_scan_step(const long long* __restrict__ records, long long* __restrict__ state, int n_poses, double r, int mask, double tol_t, double tol_r,
            float* __restrict__ poses) {
    const int b = blockIdx.x * TO_WAVE + threadIdx.x;
    if (b >= n_poses) return;
    long long* I = state + (long long)b * kRegState;
    double* D = reinterpret_cast<double*>(I);
    if (I[kRegStatus] != kRegRunning) return;
    const bool first = I[kRegIter] == 0;
    I[kRegIter] += 1;
    const long long* rec = records + (long long)b * kRegRecord;
    if (rec[28] == 0) {
        I[kRegStatus] = kRegEmpty;
        return;
    }
    long long* cur = I + kRegRec;
    double lam = D[kRegLambda];
    if (first || (rec[28] == cur[28] && rec[27] < cur[27])) {
#pragma unroll
        for (int k = 0; k < 3; ++k) D[kRegT + k] = D[kRegTrialT + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) D[kRegQ + k] = D[kRegTrialQ + k];
        for (int k = 0; k < kRegRecord; ++k) cur[k] = rec[k];
        if (!first) {
            I[kRegAccepted] += 1;
            lam = lam / 8.0;
            lam = lam > 0x1p-30 ? lam : 0x1p-30;
            D[kRegLambda] = lam;
            bool small = true;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double v = D[kRegDelta + k], tol = k < 3 ? tol_t : tol_r;
                small = small && v <= tol && -v <= tol;
            }
            if (small) {
                I[kRegStatus] = kRegConverged;
                return;
            }
        }
    } else {
        lam = lam * 8.0;
        D[kRegLambda] = lam;
        if (lam > 0x1p30) {
            I[kRegStatus] = kRegStalled;
            return;
        }
    }
    double x[6];
    if (!reg_solve(cur, lam, mask, x)) {
        I[kRegStatus] = kRegDegenerate;
        return;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) D[kRegDelta + k] = x[k];
    const double tx = D[kRegT] + r * x[0], ty = D[kRegT + 1] + r * x[1], tz = D[kRegT + 2] + r * x[2];
    const double qw = D[kRegQ], qx = D[kRegQ + 1], qy = D[kRegQ + 2], qz = D[kRegQ + 3];
    const double hx = 0.5 * x[3], hy = 0.5 * x[4], hz = 0.5 * x[5];
    // (1, h) (x) q, the Hamilton product on the left
    const double nw = ((qw - hx * qx) - hy * qy) - hz * qz;
    const double nx = ((qx + hx * qw) + hy * qz) - hz * qy;
    const double ny = ((qy - hx * qz) + hy * qw) + hz * qx;
    const double nz = ((qz + hx * qy) - hy * qx) + hz * qw;
    D[kRegTrialT] = tx, D[kRegTrialT + 1] = ty, D[kRegTrialT + 2] = tz;
    D[kRegTrialQ] = nw, D[kRegTrialQ + 1] = nx, D[kRegTrialQ + 2] = ny, D[kRegTrialQ + 3] = nz;
    // R of the unnormalised quaternion, s = 2 / (q . q) (synth.scan_pose12_ref)
    const double s = 2.0 / (((nw * nw + nx * nx) + ny * ny) + nz * nz);
    float* P = poses + 12 * (long long)b;
    P[0] = (float)(1.0 - s * (ny * ny + nz * nz)), P[1] = (float)(s * (nx * ny - nw * nz)), P[2] = (float)(s * (nx * nz + nw * ny));
    P[3] = (float)(s * (nx * ny + nw * nz)), P[4] = (float)(1.0 - s * (nx * nx + nz * nz)), P[5] = (float)(s * (ny * nz - nw * nx));
    P[6] = (float)(s * (nx * nz - nw * ny)), P[7] = (float)(s * (ny * nz + nw * nx)), P[8] = (float)(1.0 - s * (nx * nx + ny * ny));
    P[9] = (float)tx, P[10] = (float)ty, P[11] = (float)tz;
}

}  // namespace

extern "C" int tohip_scanreg_normal(const void* table, size_t table_bytes, const tohip_occ_geom* geom, int32_t unknown_value, const float* points,
                                    int64_t n, const float* poses, int64_t b, const int64_t* state_or_null, int64_t* records, void* stream_,
                                    uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = evid_check(table, table_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!scan_value_ok(0, unknown_value) || n < 1 || n > kScanMaxPoints || b < 1 || b > kRegMaxPoses || !points || !poses || !records)
        return TOHIP_EINVAL;
    if (!scan_aligned(points, 4) || !scan_aligned(poses, 4) || !scan_aligned(state_or_null, 8) || !scan_aligned(records, 8)) return TOHIP_EINVAL;
    const void* ins[4] = {points, poses, state_or_null, table};
    for (int i = 0; i < 4; ++i)   // the output is no input
        if (ins[i] == (const void*)records) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(records, 0, (size_t)b * kRegRecord * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    const long long per = (kScanBlocks + b - 1) / b;   // tile blocks per pose: the launch holds about kScanBlocks blocks
    const dim3 grid((unsigned)(per < n_tiles ? per : n_tiles), (unsigned)b);
    const unsigned unknown4 = (unsigned)(128 + unknown_value) * 0x01010101u;
    k_scan_normal<<<grid, TO_BLOCK, 0, st>>>(reinterpret_cast<const unsigned*>((const char*)table + kEvidHdr), g, unknown4, points, n, poses,
                                             reinterpret_cast<const long long*>(state_or_null), reinterpret_cast<long long*>(records));
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_scanreg_step(const int64_t* records, int64_t* state, int64_t b, float resolution, int32_t dof_mask, double tol_t, double tol_r,
                                  float* poses, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    if (b < 1 || b > kRegMaxPoses || !records || !state || !poses || !(resolution > 0.f) || !std::isfinite(resolution) || dof_mask < 1 ||
        dof_mask > 63 || !(tol_t >= 0.0) || !(tol_r >= 0.0) || !std::isfinite(tol_t) || !std::isfinite(tol_r))
        return TOHIP_EINVAL;
    if (!scan_aligned(records, 8) || !scan_aligned(state, 8) || !scan_aligned(poses, 4)) return TOHIP_EINVAL;
    if ((const void*)records == (const void*)state || (const void*)records == (const void*)poses || (const void*)state == (const void*)poses)
        return TOHIP_EINVAL;
    k_scan_step<<<(unsigned)((b + TO_WAVE - 1) / TO_WAVE), TO_WAVE, 0, (hipStream_t)stream_>>>(
        reinterpret_cast<const long long*>(records), reinterpret_cast<long long*>(state), (int)b, (double)resolution, dof_mask, tol_t, tol_r, poses);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
