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

// ---- the swept term: the same hinge on each SEGMENT's distance to its nearest cloud point ('segments' mode) --------------------
// For consecutive waypoints a = t_w, b = t_{w+1} of ONE trajectory (never across two trajectories laid end to end), all f32 without
// contraction:  e = fl(b - a), ee = fl(fl(ex ex + ey ey) + ez ez), inv = fl(1 / ee) (0 when ee is not > 0);  per finite point x:
// u = fl(x - a), s = fmin(fmax(fl(fl(fl(ux ex + uy ey) + uz ez) inv), 0), 1) (a NaN becomes 0), q = fl(u - fl(s e)),
// d2 = fl(fl(qx qx + qy qy) + qz qz).  The winner is the argmin of d2 over d2 < fl(r r), ties to the lowest caller row (-1: none, or
// an endpoint that is not finite); a = b is the point query above, bit for bit.  One thread finishes in f64: d = sqrt((double)d2),
// s* and the closest point c recomputed in f64 from the f32 coordinates, n = (c - x) / |c - x|, term = (r - d)^2,
// g_a = -2 weight (r - d)(1 - s*) n, g_b = -2 weight (r - d) s* n (the envelope theorem: s* is a minimiser or sits on its clamp),
// both zero when |c - x| = 0.  The per-segment parts go to scratch; k_clearance_seg_rows adds them per waypoint.
// The same block shape as k_clearance; the prune measures the sphere's centre against the segment (same clamp, plain f32).
struct ClrSegArgs {
    CloudView cv;
    const float* p;        // (n_traj W, 3) waypoint positions, trajectories end to end
    int W;                 // waypoints of one trajectory (>= 2): segment blockIdx.x = (b, w), b = blockIdx.x / (W - 1)
    float r, weight;
    float* d;              // may be NULL: (n_traj (W - 1)) distance, +inf when no point is within r
    int* idx;              // may be NULL: (n_traj (W - 1)) caller row of the nearest point, -1 when none
    float* s;              // may be NULL: (n_traj (W - 1)) where along the segment the closest point lies (0 = a, 1 = b; 0 when idx = -1)
    double* term;          // (n_traj W) per-waypoint terms: entry b W + w = (r - d)^2 of segment (b, w)
    double* part;          // (n_traj (W - 1), 6) g_a, g_b of every segment in f64
};

__global__ void __launch_bounds__(TO_CLR_WAVES * 64) k_clearance_seg(ClrSegArgs a) {
    __shared__ unsigned long long sbest[TO_CLR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t seg = blockIdx.x;
    const int64_t row = seg / (a.W - 1) * a.W + seg % (a.W - 1);   // the waypoint row of the segment's first end
    const float ax = a.p[3 * row], ay = a.p[3 * row + 1], az = a.p[3 * row + 2];
    const float bx = a.p[3 * row + 3], by = a.p[3 * row + 4], bz = a.p[3 * row + 5];
    const float r2 = __fmul_rn(a.r, a.r);
    unsigned long long best = ~0ull;
    if (clr_finite3(ax, ay, az) && clr_finite3(bx, by, bz)) {
        const int64_t npad = a.cv.npad, n = a.cv.n;
        const int ntiles = (int)(npad / 256);
        const float* X = a.cv.soa;
        const float* Y = X + npad;
        const float* Z = Y + npad;
        const float ex = __fsub_rn(bx, ax), ey = __fsub_rn(by, ay), ez = __fsub_rn(bz, az);
        const float ee = __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
        const float inv = ee > 0.f ? __fdiv_rn(1.f, ee) : 0.f;
        const float ta = fmaxf(fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fabsf(az)), fmaxf(fmaxf(fabsf(bx), fabsf(by)), fabsf(bz)));
        float rad = a.r;
        auto cand = [&](float x, float y, float z, int64_t s, int prow) {
            if (s >= n || prow < 0 || !clr_finite3(x, y, z)) return;
            const float ux = __fsub_rn(x, ax), uy = __fsub_rn(y, ay), uz = __fsub_rn(z, az);
            const float dot = __fadd_rn(__fadd_rn(__fmul_rn(ux, ex), __fmul_rn(uy, ey)), __fmul_rn(uz, ez));
            const float t = fminf(fmaxf(__fmul_rn(dot, inv), 0.f), 1.f);   // fmaxf(NaN, 0) = 0
            const float qx = __fsub_rn(ux, __fmul_rn(t, ex)), qy = __fsub_rn(uy, __fmul_rn(t, ey)), qz = __fsub_rn(uz, __fmul_rn(t, ez));
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(qx, qx), __fmul_rn(qy, qy)), __fmul_rn(qz, qz));
            if (d2 < r2) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)prow;
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
                    const float ux = b.x - ax, uy = b.y - ay, uz = b.z - az;
                    const float t = fminf(fmaxf((ux * ex + uy * ey + uz * ez) * inv, 0.f), 1.f);
                    const float qx = ux - t * ex, qy = uy - t * ey, qz = uz - t * ez;
                    const float dc = sqrtf(qx * qx + qy * qy + qz * qz);
                    const float amax = fmaxf(ta, fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fabsf(b.z)));
                    // |c - segment| - R > rad, with room for the rounding of dc, of the sphere and of each point's d2; (a dc that is
                    // not a number — an overflow — keeps the tile)
                    keep = !(dc > (b.w + rad) * 1.0001f + 1e-5f * amax + 1e-6f);
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
    if (lane == 0) sbest[wave] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 0; k < TO_CLR_WAVES; ++k) best = sbest[k] < best ? sbest[k] : best;
    float dout = INFINITY, sout = 0.f;
    int iout = -1;
    double term = 0.0, g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (best != ~0ull) {
        const float d2 = __uint_as_float((unsigned)(best >> 32));
        iout = (int)(unsigned)(best & 0xffffffffull);
        const double d = sqrt((double)d2);
        dout = (float)d;
        const double h = (double)a.r - d;
        term = h * h;
        const int64_t slot = a.cv.inv[iout];
        const float* P = a.cv.soa;
        const double a3[3] = {(double)ax, (double)ay, (double)az}, b3[3] = {(double)bx, (double)by, (double)bz};
        double e3[3], u3[3], v3[3], ee = 0.0, dot = 0.0, vv = 0.0;
        for (int k = 0; k < 3; ++k) {
            e3[k] = b3[k] - a3[k];
            u3[k] = (double)P[k * a.cv.npad + slot] - a3[k];
            ee += e3[k] * e3[k];
            dot += u3[k] * e3[k];
        }
        const double t = ee > 0.0 ? fmin(fmax(dot / ee, 0.0), 1.0) : 0.0;
        sout = (float)t;
        for (int k = 0; k < 3; ++k) {
            v3[k] = t * e3[k] - u3[k];   // c - x
            vv += v3[k] * v3[k];
        }
        if (vv > 0.0) {
            const double c = -2.0 * (double)a.weight * h / sqrt(vv);
            for (int k = 0; k < 3; ++k) {
                g[k] = c * (1.0 - t) * v3[k];
                g[3 + k] = c * t * v3[k];
            }
        }
    }
    if (a.d) a.d[seg] = dout;
    if (a.idx) a.idx[seg] = iout;
    if (a.s) a.s[seg] = sout;
    a.term[row] = term;
    for (int k = 0; k < 6; ++k) a.part[6 * seg + k] = g[k];
}

// one thread per waypoint row: gradient row w = (float)(g_b of segment w - 1 + g_a of segment w), added in f64 in that order and
// rounded once; the last waypoint of a trajectory starts no segment: its term is 0
__global__ void __launch_bounds__(256) k_clearance_seg_rows(const double* __restrict__ part, int W, int64_t n_rows, double* __restrict__ term,
                                                             float* __restrict__ grad) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const int w = (int)(row % W);
    const int64_t seg = row / W * (W - 1) + w;
    if (w == W - 1) term[row] = 0.0;
    if (!grad) return;
    for (int k = 0; k < 3; ++k) {
        const double gb = w > 0 ? part[6 * (seg - 1) + 3 + k] : 0.0, ga = w < W - 1 ? part[6 * seg + k] : 0.0;
        grad[3 * row + k] = (float)(gb + ga);
    }
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

// ---- 'segments' mode: the entry points -------------------------------------------------------------------------------------------
static inline size_t clearance_seg_part_bytes(int64_t W, int64_t n_traj) { return align_up((size_t)(n_traj * (W - 1)) * 48, 256); }

// the two launches behind every path that carries the swept term: the segment query, then the per-waypoint rows and terms
static inline int clearance_seg_launch(const void* packed, int64_t n_points, const float* poses, int64_t W, int64_t n_traj, float r,
                                       float weight, float* d, int* idx, float* s, double* term, double* part, float* grad, hipStream_t st) {
    ClrSegArgs a;
    a.cv = cloud_view(packed, n_points);
    a.p = poses; a.W = (int)W; a.r = r; a.weight = weight;
    a.d = d; a.idx = idx; a.s = s; a.term = term; a.part = part;
    k_clearance_seg<<<(unsigned)(n_traj * (W - 1)), TO_CLR_WAVES * 64, 0, st>>>(a);
    TO_HIP_CHECK_LAUNCH();
    const int64_t rows = n_traj * W;
    k_clearance_seg_rows<<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(part, (int)W, rows, term, grad);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

// the scratch of a plan / run that carries the swept term: clearance_scratch_bytes' rows and terms at their offsets, then the
// per-segment parts
static inline size_t clearance_seg_scratch_bytes(int64_t W, int64_t n_traj) {
    return clearance_scratch_bytes(W * n_traj) + clearance_seg_part_bytes(W, n_traj);
}
static inline double* clearance_seg_scratch_part(void* s, int64_t nq) { return (double*)((char*)s + clearance_scratch_bytes(nq)); }

// the query of a plan / run in either mode into its clearance scratch (segments: TOHIP_TRAJ_CLEARANCE_SEGMENTS in its flags)
static inline int clearance_scratch_launch(const void* packed, int64_t n_points, const float* poses, int64_t W, int64_t n_traj, float r,
                                           float weight, bool segments, void* scratch, hipStream_t st) {
    float* rows = clearance_scratch_grad(scratch);
    double* term = clearance_scratch_term(scratch, W * n_traj);
    if (!segments) return clearance_launch(packed, n_points, poses, W * n_traj, r, weight, nullptr, nullptr, term, rows, 0, st);
    return clearance_seg_launch(packed, n_points, poses, W, n_traj, r, weight, nullptr, nullptr, nullptr, term,
                                clearance_seg_scratch_part(scratch, W * n_traj), rows, st);
}

static inline bool clearance_seg_counts_ok(int64_t n_wps, int64_t n_traj) {
    return n_wps >= 2 && n_traj >= 1 && n_wps <= (int64_t)INT32_MAX && n_traj <= (int64_t)INT32_MAX / n_wps;
}

extern "C" size_t tohip_clearance_segments_workspace_bytes(int64_t n_wps, int64_t n_traj) {
    if (!clearance_seg_counts_ok(n_wps, n_traj)) return 0;
    return align_up((size_t)(n_wps * n_traj) * 8, 256) + clearance_seg_part_bytes(n_wps, n_traj);
}

extern "C" size_t tohip_traj_clearance_segments_scratch_bytes(int64_t n_wps, int64_t n_traj) {
    return clearance_seg_counts_ok(n_wps, n_traj) ? clearance_seg_scratch_bytes(n_wps, n_traj) : 0;
}

extern "C" int tohip_clearance_segments(const void* packed, int64_t n_points, const float* poses, int64_t n_wps, int64_t n_traj, float radius,
                                        float weight, float* d, int32_t* idx, float* s, float* value, float* grad, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (!packed || !poses || !d || !idx || !s || !workspace || n_points <= 0 || n_points > INT32_MAX || !clearance_seg_counts_ok(n_wps, n_traj) ||
        !clearance_args_ok(radius, weight))
        return TOHIP_EINVAL;
    if (workspace_bytes < tohip_clearance_segments_workspace_bytes(n_wps, n_traj)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    double* term = (double*)workspace;
    double* part = (double*)((char*)workspace + align_up((size_t)(n_wps * n_traj) * 8, 256));
    int rc = clearance_seg_launch(packed, n_points, poses, n_wps, n_traj, radius, weight, d, idx, s, term, part, grad, st);
    if (rc != TOHIP_OK || !value) return rc;
    k_clearance_value<<<(unsigned)n_traj, 64, 0, st>>>(term, n_wps, weight, value);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

// ---- arbitrary segments, one WAVE each: the edge stage of tools.plan_tour (tour_kernels.hip) -----------------------------------
// tohip_clearance_segments with n_wps = 2 answers E unrelated segments with E blocks of 16 waves; all pairs of 257 nodes are 32 896 of
// them, far more than the chip has room for at once, so the 16 waves of a block buy no latency and cost a block-wide fold each.  Here
// a wave owns an edge (TO_EDGE_WAVES edges to a block, no LDS, no barrier): its lanes stride over ALL the tile spheres with
// k_clearance_seg's inequality, it scans the kept tiles of each group of 64 four points per lane and shrinks the radius after each
// group.  The key, the per-point arithmetic and the f64 finish are k_clearance_seg's, so (d, idx, s) are its bits for the same two
// ends: the prune only ever drops tiles that hold no point within the current radius, whatever the order the tiles are met in.
#define TO_EDGE_WAVES 4

struct ClrEdgeArgs {
    CloudView cv;
    const float* a;        // (E, 3) first ends
    const float* b;        // (E, 3) second ends
    int64_t E;
    float r;
    float* d;              // may be NULL: (E) distance, +inf when no point is within r
    int* idx;              // may be NULL: (E) caller row of the nearest point, -1 when none
    float* s;              // may be NULL: (E) where along the edge the closest point lies
};

__global__ void __launch_bounds__(TO_EDGE_WAVES * 64) k_clearance_edge(ClrEdgeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * TO_EDGE_WAVES + (threadIdx.x >> 6);
    if (e >= a.E) return;   // (wave-uniform)
    const float ax = a.a[3 * e], ay = a.a[3 * e + 1], az = a.a[3 * e + 2];
    const float bx = a.b[3 * e], by = a.b[3 * e + 1], bz = a.b[3 * e + 2];
    const float r2 = __fmul_rn(a.r, a.r);
    unsigned long long best = ~0ull;
    if (clr_finite3(ax, ay, az) && clr_finite3(bx, by, bz)) {
        const int64_t npad = a.cv.npad, n = a.cv.n;
        const int ntiles = (int)(npad / 256);
        const float* X = a.cv.soa;
        const float* Y = X + npad;
        const float* Z = Y + npad;
        const float ex = __fsub_rn(bx, ax), ey = __fsub_rn(by, ay), ez = __fsub_rn(bz, az);
        const float ee = __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
        const float inv = ee > 0.f ? __fdiv_rn(1.f, ee) : 0.f;
        const float ta = fmaxf(fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fabsf(az)), fmaxf(fmaxf(fabsf(bx), fabsf(by)), fabsf(bz)));
        float rad = a.r;
        auto cand = [&](float x, float y, float z, int64_t s, int prow) {
            if (s >= n || prow < 0 || !clr_finite3(x, y, z)) return;
            const float ux = __fsub_rn(x, ax), uy = __fsub_rn(y, ay), uz = __fsub_rn(z, az);
            const float dot = __fadd_rn(__fadd_rn(__fmul_rn(ux, ex), __fmul_rn(uy, ey)), __fmul_rn(uz, ez));
            const float t = fminf(fmaxf(__fmul_rn(dot, inv), 0.f), 1.f);   // fmaxf(NaN, 0) = 0
            const float qx = __fsub_rn(ux, __fmul_rn(t, ex)), qy = __fsub_rn(uy, __fmul_rn(t, ey)), qz = __fsub_rn(uz, __fmul_rn(t, ez));
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(qx, qx), __fmul_rn(qy, qy)), __fmul_rn(qz, qz));
            if (d2 < r2) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)prow;
                best = key < best ? key : best;
            }
        };
        for (int base = 0; base < ntiles; base += 64) {
            const int tile = base + lane;
            bool keep = false;
            if (tile < ntiles) {
                const float4 b = a.cv.bounds[tile];
                if (!(clr_finite3(b.x, b.y, b.z) && isfinite(b.w))) {
                    keep = true;
                } else {
                    const float ux = b.x - ax, uy = b.y - ay, uz = b.z - az;
                    const float t = fminf(fmaxf((ux * ex + uy * ey + uz * ez) * inv, 0.f), 1.f);
                    const float qx = ux - t * ex, qy = uy - t * ey, qz = uz - t * ez;
                    const float dc = sqrtf(qx * qx + qy * qy + qz * qz);
                    const float amax = fmaxf(ta, fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fabsf(b.z)));
                    keep = !(dc > (b.w + rad) * 1.0001f + 1e-5f * amax + 1e-6f);   // k_clearance_seg's inequality
                }
            }
            unsigned long long kept = __ballot(keep);
            if (!kept) continue;
            while (kept) {
                const int k = __ffsll((long long)kept) - 1;
                kept &= kept - 1;
                const int64_t p0 = (int64_t)(base + k) * 256 + 4 * lane;   // base + k < ntiles: only lanes with tile < ntiles vote
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
    if (lane != 0) return;
    float dout = INFINITY, sout = 0.f;
    int iout = -1;
    if (best != ~0ull) {   // k_clearance_seg's finish, without the term and the gradient
        const float d2 = __uint_as_float((unsigned)(best >> 32));
        iout = (int)(unsigned)(best & 0xffffffffull);
        dout = (float)sqrt((double)d2);
        const int64_t slot = a.cv.inv[iout];
        const float* P = a.cv.soa;
        const double a3[3] = {(double)ax, (double)ay, (double)az}, b3[3] = {(double)bx, (double)by, (double)bz};
        double ee = 0.0, dot = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double ek = b3[k] - a3[k], uk = (double)P[k * a.cv.npad + slot] - a3[k];
            ee += ek * ek;
            dot += uk * ek;
        }
        sout = (float)(ee > 0.0 ? fmin(fmax(dot / ee, 0.0), 1.0) : 0.0);
    }
    if (a.d) a.d[e] = dout;
    if (a.idx) a.idx[e] = iout;
    if (a.s) a.s[e] = sout;
}

extern "C" int tohip_clearance_edges(const void* packed, int64_t n_points, const float* a, const float* b, int64_t n_edges, float radius,
                                     float* d, int32_t* idx, float* s, void* stream) {
    if (!packed || !a || !b || n_points <= 0 || n_points > INT32_MAX || n_edges <= 0 || n_edges > (int64_t)INT32_MAX ||
        !clearance_args_ok(radius, 0.f))
        return TOHIP_EINVAL;
    ClrEdgeArgs g;
    g.cv = cloud_view(packed, n_points);
    g.a = a; g.b = b; g.E = n_edges; g.r = radius;
    g.d = d; g.idx = idx; g.s = s;
    k_clearance_edge<<<(unsigned)((n_edges + TO_EDGE_WAVES - 1) / TO_EDGE_WAVES), TO_EDGE_WAVES * 64, 0, (hipStream_t)stream>>>(g);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
