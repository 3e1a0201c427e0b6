// clearance_kernels.hip — the clearance term of a trajectory: a hinge on each waypoint's distance to its nearest cloud point.
//
// For waypoint position t_w (every waypoint, like the other regularisers):
//   d2_w = min_i fl((dx*dx + dy*dy) + dz*dz), dx = fl(t_w.x - x_i.x) ...  (f32, no contraction), over the rows whose three
//          coordinates are finite (pads never count); ties go to the lowest caller row; i*_w = that row, or -1 when no point has
//          d2 < fl(r*r) (and for a waypoint with a non-finite coordinate)
//   d_w  = sqrt((double)d2_w)
//   clearance = weight * sum_w (r - d_w)^2 over the waypoints with i*_w >= 0, the sum in f64 in w order, rounded to f32
//   d clearance / d t_w = -2 weight (r - d_w) (t_w - x_{i*}) / d_w in f64, rounded to f32; zero when i* = -1 or d_w = 0
//
// One block of 16 waves per query over the packed cloud (each wave a sixteenth of the tiles) (tohip_pack_cloud: SoA in Morton order, one bounding sphere per 256 points).  The
// lanes stride over the tile spheres and keep a tile when |t - c| <= R + rad with a relative and an absolute slack (rad: the
// search radius, r at first, then the distance of the best point so far); a sphere with a non-finite centre or radius (a tile
// with a NaN or inf coordinate) is always kept, since its finite points still count.  The wave scans each kept tile's 256 points,
// 4 per lane, and keeps per lane the smallest 64-bit key (float bits of d2) << 32 | caller row: for d2 >= 0 the unsigned order is
// the float order, so the wave's minimum is the argmin with its tie rule, whatever order the lanes met the points in.  No
// atomics; the per-query results do not depend on the launch.  (One wave per query walked the 4 096 spheres of a 1 M-point cloud in
// 64 dependent steps: 40 us for 128 queries on a chip that had 128 waves to run.)
#include "common.hpp"
#include "opt_step.hpp"

#define TO_CLR_WAVES 16   // waves per query (one block): each takes every 16th group of 64 tile spheres

struct ClrArgs {
    CloudView cv;
    const float* q;        // (nq, 3) query positions
    int64_t nq;
    float r, weight;
    float* d;              // may be NULL: (nq) distance, +inf when no point is within r
    int* idx;              // may be NULL: (nq) caller row of the nearest point, -1 when none is within r
    double* term;          // may be NULL: (nq) (r - d)^2 in f64 (0 when idx = -1)
    float* grad;           // may be NULL: (nq, 3) gradient rows, overwritten or (accumulate) added to
    int accumulate;
};

__device__ __forceinline__ unsigned long long clr_wave_min(unsigned long long v) {
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, s), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), s);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ bool clr_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ void __launch_bounds__(TO_CLR_WAVES * 64) k_clearance(ClrArgs a) {
    __shared__ unsigned long long sbest[TO_CLR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = blockIdx.x;   // the query
    const float tx = a.q[3 * w], ty = a.q[3 * w + 1], tz = a.q[3 * w + 2];
    const float r2 = __fmul_rn(a.r, a.r);
    unsigned long long best = ~0ull;
    if (clr_finite3(tx, ty, tz)) {
        const int64_t npad = a.cv.npad, n = a.cv.n;
        const int ntiles = (int)(npad / 256);
        const float* X = a.cv.soa;
        const float* Y = X + npad;
        const float* Z = Y + npad;
        const float ta = fmaxf(fmaxf(fabsf(tx), fabsf(ty)), fabsf(tz));
        float rad = a.r;
        auto cand = [&](float x, float y, float z, int64_t s, int row) {
            if (s >= n || row < 0 || !clr_finite3(x, y, z)) return;
            const float dx = __fsub_rn(tx, x), dy = __fsub_rn(ty, y), dz = __fsub_rn(tz, z);
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            if (d2 < r2) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)row;
                best = key < best ? key : best;
            }
        };
        for (int base = 64 * wave; base < ntiles; base += 64 * TO_CLR_WAVES) {
            const int tile = base + lane;
            bool keep = false;
            if (tile < ntiles) {
                const float4 b = a.cv.bounds[tile];
                if (!(clr_finite3(b.x, b.y, b.z) && isfinite(b.w))) {
                    keep = true;
                } else {
                    const float dx = tx - b.x, dy = ty - b.y, dz = tz - b.z;
                    const float dc = sqrtf(dx * dx + dy * dy + dz * dz);
                    const float amax = fmaxf(ta, fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fabsf(b.z)));
                    // |t - c| - R > rad, with room for the rounding of dc, of the sphere and of each point's d2
                    keep = dc <= (b.w + rad) * 1.0001f + 1e-5f * amax + 1e-6f;
                }
            }
            unsigned long long kept = __ballot(keep);
            if (!kept) continue;
            while (kept) {
                const int k = __ffsll((long long)kept) - 1;
                kept &= kept - 1;
                const int64_t p0 = (int64_t)(base + k) * 256 + 4 * lane;
                const float4 x4 = *(const float4*)(X + p0), y4 = *(const float4*)(Y + p0), z4 = *(const float4*)(Z + p0);
                const int4 i4 = *(const int4*)(a.cv.perm + p0);
                cand(x4.x, y4.x, z4.x, p0, i4.x);
                cand(x4.y, y4.y, z4.y, p0 + 1, i4.y);
                cand(x4.z, y4.z, z4.z, p0 + 2, i4.z);
                cand(x4.w, y4.w, z4.w, p0 + 3, i4.w);
            }
            best = clr_wave_min(best);   // uniform from here: the search radius shrinks to the best distance so far
            if (best != ~0ull) rad = sqrtf(__uint_as_float((unsigned)(best >> 32)));
        }
        best = clr_wave_min(best);
    }
    // the block's minimum: the waves' keys in LDS, one thread folds them (min is order-free: the same bits whatever the schedule)
    if (lane == 0) sbest[wave] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 0; k < TO_CLR_WAVES; ++k) best = sbest[k] < best ? sbest[k] : best;
    float dout = INFINITY, g[3] = {0.f, 0.f, 0.f};
    int iout = -1;
    double term = 0.0;
    if (best != ~0ull) {
        const float d2 = __uint_as_float((unsigned)(best >> 32));
        iout = (int)(unsigned)(best & 0xffffffffull);
        const double d = sqrt((double)d2);
        dout = (float)d;
        const double h = (double)a.r - d;
        term = h * h;
        if (d > 0.0) {
            const int64_t s = a.cv.inv[iout];
            const double c = -2.0 * (double)a.weight * h;
            const double t3[3] = {(double)tx, (double)ty, (double)tz};
            const float* P = a.cv.soa;
            for (int k = 0; k < 3; ++k) g[k] = (float)(c * (t3[k] - (double)P[k * a.cv.npad + s]) / d);
        }
    }
    if (a.d) a.d[w] = dout;
    if (a.idx) a.idx[w] = iout;
    if (a.term) a.term[w] = term;
    if (a.grad)
        for (int k = 0; k < 3; ++k) a.grad[3 * w + k] = a.accumulate ? a.grad[3 * w + k] + g[k] : g[k];
}

// value = weight * sum of the n_seg terms of segment blockIdx.x (in order, f64), rounded to f32 — one thread per segment
__global__ void k_clearance_value(const double* __restrict__ term, int64_t n_seg, float weight, float* __restrict__ value) {
    if (threadIdx.x == 0) value[blockIdx.x] = (float)clearance_sum(term + (int64_t)blockIdx.x * n_seg, n_seg, weight);
}

static inline bool clearance_args_ok(float r, float weight) { return std::isfinite(r) && r > 0.f && std::isfinite(weight) && weight >= 0.f; }

// the query kernel for the paths that carry the term (tohip_clearance, the one-call step, the one-call model, the step tail)
static inline int clearance_launch(const void* packed, int64_t n_points, const float* q, int64_t nq, float r, float weight, float* d,
                                   int* idx, double* term, float* grad, int accumulate, hipStream_t st) {
    ClrArgs a;
    a.cv = cloud_view(packed, n_points);
    a.q = q; a.nq = nq; a.r = r; a.weight = weight;
    a.d = d; a.idx = idx; a.term = term; a.grad = grad; a.accumulate = accumulate;
    k_clearance<<<(unsigned)nq, TO_CLR_WAVES * 64, 0, st>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

// the scratch of a plan / run that carries the term: gradient rows (nq, 3) f32 | terms (nq) f64
static inline size_t clearance_scratch_bytes(int64_t nq) { return align_up((size_t)nq * 12, 256) + align_up((size_t)nq * 8, 256); }
static inline float* clearance_scratch_grad(void* s) { return (float*)s; }
static inline double* clearance_scratch_term(void* s, int64_t nq) { return (double*)((char*)s + align_up((size_t)nq * 12, 256)); }

extern "C" size_t tohip_clearance_workspace_bytes(int64_t n_queries) {
    return n_queries > 0 ? align_up((size_t)n_queries * 8, 256) : 0;
}

extern "C" size_t tohip_traj_clearance_scratch_bytes(int64_t n_wps, int64_t n_traj) {
    return (n_wps > 0 && n_traj > 0) ? clearance_scratch_bytes(n_wps * n_traj) : 0;
}

extern "C" int tohip_clearance(const void* packed, int64_t n_points, const float* queries, int64_t n_queries, float radius, float weight,
                               float* d, int32_t* idx, float* value, float* grad, int accumulate, void* workspace, size_t workspace_bytes,
                               void* stream) {
    if (!packed || !queries || !d || !idx || !workspace || n_points <= 0 || n_points > INT32_MAX || n_queries <= 0 ||
        n_queries > (int64_t)INT32_MAX || !clearance_args_ok(radius, weight))
        return TOHIP_EINVAL;
    if (workspace_bytes < tohip_clearance_workspace_bytes(n_queries)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    double* term = (double*)workspace;
    int rc = clearance_launch(packed, n_points, queries, n_queries, radius, weight, d, idx, term, grad, accumulate, st);
    if (rc != TOHIP_OK || !value) return rc;
    k_clearance_value<<<1, 64, 0, st>>>(term, n_queries, weight, value);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
