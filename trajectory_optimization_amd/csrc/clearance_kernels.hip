// clearance_kernels.hip — the clearance term of a trajectory: a hinge on the distance from each waypoint ('waypoints' mode), or from
// each segment between two waypoints ('segments' mode, and the edge stage of tools.plan_tour), to its nearest cloud point.
//
// ONE nearest-point search (clr_search) serves the three query kernels.  It is a template on a query GEOMETRY, which says what
// is measured, and on the number of WAVES that share a query.  The kernels differ in three things only:
//   1. the geometry      k_clearance: ClrPoint;  k_clearance_seg and k_clearance_edge: ClrSegment
//   2. waves per query   k_clearance and k_clearance_seg: a block of TO_CLR_WAVES waves per query, folded through LDS (clr_block_min);
//                        k_clearance_edge: one wave per query, TO_EDGE_WAVES queries to a block, no LDS and no barrier
//   3. the finish        k_clearance: clr_point_finish;  the other two: clr_seg_finish, to which k_clearance_seg adds the term and
//                        the gradient parts (clr_seg_write).  A finish takes the winner's three f32 coordinates, read here from the
//                        packed cloud (clr_cloud_point): the kernels whose obstacles are a map's voxels (clearance_map_kernels.hip)
//                        hand it a voxel centre and share everything from there on
// So "a = b is the point query" and "an edge's (d, idx, s) are the segment query's" hold bit for bit: ClrSegment::d2 with a = b
// rounds to ClrPoint::d2's bits for every point (u - 0 e = u, and (-v)(-v) = v v), the two segment kernels instantiate the same
// geometry and call the same finish, and the winner does not depend on how many waves looked for it (below).
//
// The point query, for waypoint position t_w (every waypoint, like the other regularisers):
//   d2_w = min_i fl((dx*dx + dy*dy) + dz*dz), dx = fl(t_w.x - x_i.x) ...  (f32, no contraction), over the rows whose three
//          coordinates are finite (pads never count); ties go to the lowest caller row; i*_w = that row, or -1 when no point has
//          d2 < fl(r*r) (and for a waypoint with a non-finite coordinate)
//   d_w  = sqrt((double)d2_w)
//   clearance = weight * sum_w (r - d_w)^2 over the waypoints with i*_w >= 0, the sum in f64 in w order, rounded to f32
//   d clearance / d t_w = -2 weight (r - d_w) (t_w - x_{i*}) / d_w in f64, rounded to f32; zero when i* = -1 or d_w = 0
//
// The segment query, for consecutive waypoints a = t_w, b = t_{w+1} of ONE trajectory (never across two trajectories laid end to
// end) or the two ends of an edge, all f32 without contraction:  e = fl(b - a), ee = fl(fl(ex ex + ey ey) + ez ez), inv = fl(1 / ee)
// (0 when ee is not > 0);  per finite point x: u = fl(x - a), s = fmin(fmax(fl(fl(fl(ux ex + uy ey) + uz ez) inv), 0), 1) (a NaN
// becomes 0), q = fl(u - fl(s e)), d2 = fl(fl(qx qx + qy qy) + qz qz).  The winner is the argmin of d2 over d2 < fl(r r), ties to the
// lowest caller row (-1: none, or an endpoint that is not finite).  One thread finishes in f64: d = sqrt((double)d2), s* and the
// closest point c recomputed in f64 from the f32 coordinates, n = (c - x) / |c - x|, term = (r - d)^2,
// g_a = -2 weight (r - d)(1 - s*) n, g_b = -2 weight (r - d) s* n (the envelope theorem: s* is a minimiser or sits on its clamp),
// both zero when |c - x| = 0.  The per-segment parts go to scratch; k_clearance_seg_rows adds them per waypoint.
//
// The search, over the packed cloud (tohip_pack_cloud: SoA in Morton order, one bounding sphere per 256 points): wave k of WAVES
// takes the groups of 64 tile spheres k, k + WAVES, ...  Its lanes stride over a group's spheres and keep a tile unless the distance
// from the sphere's centre to the query exceeds R + rad with a relative and an absolute slack (rad: the search radius, r at first,
// then the distance of the wave's best point so far); a sphere with a non-finite centre or radius (a tile with a NaN or inf
// coordinate) is always kept, since its finite points still count.  The wave scans each kept tile's 256 points, 4 per lane, and
// keeps per lane the smallest 64-bit key (float bits of d2) << 32 | caller row: for d2 >= 0 the unsigned order is the float order,
// so the minimum is the argmin with its tie rule, whatever order the lanes met the points in.  The prune only ever drops tiles that
// hold no point within the current radius, so the minimum is the same for any number of waves and any order of the tiles.  No
// atomics; the per-query results do not depend on the launch.  (One wave per query walked the 4 096 spheres of a 1 M-point cloud in
// 64 dependent steps: 40 us for 128 queries on a chip that had 128 waves to run.  The edge stage asks all pairs of 257 nodes, 32 896
// queries, far more than the chip has room for at once: there 16 waves to a query buy no latency and cost a block-wide fold each.)
#include <initializer_list>

#include "common.hpp"
#include "opt_step.hpp"

#define TO_CLR_WAVES 16   // waves per query (one block) of k_clearance and k_clearance_seg
#define TO_EDGE_WAVES 4   // queries per block, one wave each, of k_clearance_edge

// ---- the two geometries: finite(), the exact f32 d2 of a point, and for the prune the plain-f32 distance of a sphere's centre and
// the query's max |coordinate| -----------------------------------------------------------------------------------------------------
struct ClrPoint {
    float tx, ty, tz;
    __device__ explicit ClrPoint(const float* t) : tx(t[0]), ty(t[1]), tz(t[2]) {}
    __device__ bool finite() const { return finite3(tx, ty, tz); }
    __device__ float max_abs() const { return fmaxf(fmaxf(fabsf(tx), fabsf(ty)), fabsf(tz)); }
    __device__ float d2(float x, float y, float z) const {
        const float dx = __fsub_rn(tx, x), dy = __fsub_rn(ty, y), dz = __fsub_rn(tz, z);
        return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    }
    __device__ float centre_dist(const float4& b) const {
        const float dx = tx - b.x, dy = ty - b.y, dz = tz - b.z;
        return sqrtf(dx * dx + dy * dy + dz * dz);
    }
};

struct ClrSegment {
    float ax, ay, az, bx, by, bz;
    float ex, ey, ez, inv;   // e = fl(b - a), inv = fl(1 / fl(e.e)) or 0
    __device__ ClrSegment(const float* a, const float* b) : ax(a[0]), ay(a[1]), az(a[2]), bx(b[0]), by(b[1]), bz(b[2]) {
        ex = __fsub_rn(bx, ax), ey = __fsub_rn(by, ay), ez = __fsub_rn(bz, az);
        const float ee = __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
        inv = ee > 0.f ? __fdiv_rn(1.f, ee) : 0.f;
    }
    __device__ bool finite() const { return finite3(ax, ay, az) && finite3(bx, by, bz); }
    __device__ float max_abs() const {
        return fmaxf(fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fabsf(az)), fmaxf(fmaxf(fabsf(bx), fabsf(by)), fabsf(bz)));
    }
    __device__ float d2(float x, float y, float z) const {
        const float ux = __fsub_rn(x, ax), uy = __fsub_rn(y, ay), uz = __fsub_rn(z, az);
        const float dot = __fadd_rn(__fadd_rn(__fmul_rn(ux, ex), __fmul_rn(uy, ey)), __fmul_rn(uz, ez));
        const float t = fminf(fmaxf(__fmul_rn(dot, inv), 0.f), 1.f);   // fmaxf(NaN, 0) = 0
        const float qx = __fsub_rn(ux, __fmul_rn(t, ex)), qy = __fsub_rn(uy, __fmul_rn(t, ey)), qz = __fsub_rn(uz, __fmul_rn(t, ez));
        return __fadd_rn(__fadd_rn(__fmul_rn(qx, qx), __fmul_rn(qy, qy)), __fmul_rn(qz, qz));
    }
    __device__ float centre_dist(const float4& b) const {   // the same clamp
        const float ux = b.x - ax, uy = b.y - ay, uz = b.z - az;
        const float t = fminf(fmaxf((ux * ex + uy * ey + uz * ez) * inv, 0.f), 1.f);
        const float qx = ux - t * ex, qy = uy - t * ey, qz = uz - t * ez;
        return sqrtf(qx * qx + qy * qy + qz * qz);
    }
};

__device__ __forceinline__ unsigned long long clr_wave_min(unsigned long long v) {
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, s), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), s);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// ---- the search: the smallest key over this wave's share of the tiles, the same in every lane; ~0 when no point has d2 < fl(r r) or
// the query is not finite.  wave of WAVES: this wave's index among the waves that share the query. ---------------------------------
template <int WAVES, class Geom>
__device__ __forceinline__ unsigned long long clr_search(const CloudView& cv, const Geom& g, float r, int wave) {
    unsigned long long best = ~0ull;
    if (!g.finite()) return best;
    const int lane = threadIdx.x & 63;
    const int64_t npad = cv.npad, n = cv.n;
    const int ntiles = (int)(npad / 256);
    const float* X = cv.soa;
    const float* Y = X + npad;
    const float* Z = Y + npad;
    const float r2 = __fmul_rn(r, r), ta = g.max_abs();
    float rad = r;
    auto cand = [&](float x, float y, float z, int64_t s, int row) {
        if (s >= n || row < 0 || !finite3(x, y, z)) return;
        const float d2 = g.d2(x, y, z);
        if (d2 < r2) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)row;
            best = key < best ? key : best;
        }
    };
    for (int base = 64 * wave; base < ntiles; base += 64 * WAVES) {
        const int tile = base + lane;
        bool keep = false;
        if (tile < ntiles) {
            const float4 b = cv.bounds[tile];
            if (!(finite3(b.x, b.y, b.z) && isfinite(b.w))) {
                keep = true;
            } else {
                const float dc = g.centre_dist(b);
                const float amax = fmaxf(ta, fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fabsf(b.z)));
                // dropped when |c - query| - R > rad, with room for the rounding of dc, of the sphere and of each point's d2.  Written
                // as !(>) so that a dc that is not a number (a segment's overflow: inf - inf) keeps the tile.  A point's dc is the
                // square root of a sum of squares of differences of finite numbers: +inf at most, never NaN, and the bound is never
                // NaN either (finite terms, or one infinite product), so for the point query this is dc <= bound
                keep = !(dc > (b.w + rad) * 1.0001f + 1e-5f * amax + 1e-6f);
            }
        }
        unsigned long long kept = __ballot(keep);
        if (!kept) continue;
        while (kept) {
            const int k = __ffsll((long long)kept) - 1;
            kept &= kept - 1;
            const int64_t p0 = (int64_t)(base + k) * 256 + 4 * lane;   // base + k < ntiles: only lanes with tile < ntiles vote
            const float4 x4 = *(const float4*)(X + p0), y4 = *(const float4*)(Y + p0), z4 = *(const float4*)(Z + p0);
            const int4 i4 = *(const int4*)(cv.perm + p0);
            cand(x4.x, y4.x, z4.x, p0, i4.x);
            cand(x4.y, y4.y, z4.y, p0 + 1, i4.y);
            cand(x4.z, y4.z, z4.z, p0 + 2, i4.z);
            cand(x4.w, y4.w, z4.w, p0 + 3, i4.w);
        }
        best = clr_wave_min(best);   // uniform from here: the search radius shrinks to the best distance so far
        if (best != ~0ull) rad = sqrtf(__uint_as_float((unsigned)(best >> 32)));
    }
    return clr_wave_min(best);
}

// the block's minimum: the waves' keys in LDS, thread 0 folds them (min is order-free: the same bits whatever the schedule).  True in
// thread 0 alone, where best becomes the minimum
__device__ __forceinline__ bool clr_block_min(unsigned long long& best, unsigned long long (&sbest)[TO_CLR_WAVES]) {
    if ((threadIdx.x & 63) == 0) sbest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return false;
    for (int k = 0; k < TO_CLR_WAVES; ++k) best = sbest[k] < best ? sbest[k] : best;
    return true;
}

// ---- the point query ---------------------------------------------------------------------------------------------------------------
struct ClrQuery {          // what the point query asks and writes, whatever its obstacles are (the cloud here; the map's voxels:
                           // clearance_map_kernels.hip)
    const float* q;        // (nq, 3) query positions
    int64_t nq;
    float r, weight;
    float* d;              // may be NULL: (nq) distance, +inf when no point is within r
    int* idx;              // may be NULL: (nq) caller row of the nearest point, -1 when none is within r
    double* term;          // may be NULL: (nq) (r - d)^2 in f64 (0 when idx = -1)
    float* grad;           // may be NULL: (nq, 3) gradient rows, overwritten or (accumulate) added to
    int accumulate;
};
struct ClrArgs : ClrQuery {
    CloudView cv;
};

// the winner's three f32 coordinates as the cloud holds them (zeros when there is none)
__device__ __forceinline__ void clr_cloud_point(const CloudView& cv, unsigned long long best, float (&x)[3]) {
    x[0] = x[1] = x[2] = 0.f;
    if (best == ~0ull) return;
    const int64_t s = cv.inv[(int)(unsigned)(best & 0xffffffffull)];
    for (int k = 0; k < 3; ++k) x[k] = cv.soa[k * cv.npad + s];
}

// x: the winner's coordinates (not read when best = ~0)
// (its gradient divides by d = sqrt((double)d2), the segment's by |c - x| recomputed in f64: not the same bits, so not one formula)
__device__ __forceinline__ void clr_point_finish(const ClrQuery& a, const ClrPoint& t, int64_t w, unsigned long long best, const float (&x)[3]) {
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
            const double c = -2.0 * (double)a.weight * h;
            const double t3[3] = {(double)t.tx, (double)t.ty, (double)t.tz};
            for (int k = 0; k < 3; ++k) g[k] = (float)(c * (t3[k] - (double)x[k]) / d);
        }
    }
    if (a.d) a.d[w] = dout;
    if (a.idx) a.idx[w] = iout;
    if (a.term) a.term[w] = term;
    if (a.grad)
        for (int k = 0; k < 3; ++k) a.grad[3 * w + k] = a.accumulate ? a.grad[3 * w + k] + g[k] : g[k];
}

__global__ void __launch_bounds__(TO_CLR_WAVES * 64) k_clearance(ClrArgs a) {
    __shared__ unsigned long long sbest[TO_CLR_WAVES];
    const int64_t w = blockIdx.x;   // the query
    const ClrPoint t(a.q + 3 * w);
    unsigned long long best = clr_search<TO_CLR_WAVES>(a.cv, t, a.r, threadIdx.x >> 6);
    if (!clr_block_min(best, sbest)) return;
    float x[3];
    clr_cloud_point(a.cv, best, x);
    clr_point_finish(a, t, w, best, x);
}

// ---- the segment queries -----------------------------------------------------------------------------------------------------------
struct ClrSegHit {
    int idx;          // caller row of the nearest point, -1 when none is within r
    double d, s;      // its distance (+inf when none) and where along the segment the closest point c lies (0 = a, 1 = b; 0 when none)
    double v[3];      // c - x
};

// x: the winner's coordinates (not read when best = ~0)
__device__ __forceinline__ ClrSegHit clr_seg_finish(const ClrSegment& g, unsigned long long best, const float (&x)[3]) {
    ClrSegHit o = {-1, (double)INFINITY, 0.0, {0.0, 0.0, 0.0}};
    if (best == ~0ull) return o;
    const float d2 = __uint_as_float((unsigned)(best >> 32));
    o.idx = (int)(unsigned)(best & 0xffffffffull);
    o.d = sqrt((double)d2);
    const double a3[3] = {(double)g.ax, (double)g.ay, (double)g.az}, b3[3] = {(double)g.bx, (double)g.by, (double)g.bz};
    double e3[3], u3[3], ee = 0.0, dot = 0.0;
    for (int k = 0; k < 3; ++k) {
        e3[k] = b3[k] - a3[k];
        u3[k] = (double)x[k] - a3[k];
        ee += e3[k] * e3[k];
        dot += u3[k] * e3[k];
    }
    o.s = ee > 0.0 ? fmin(fmax(dot / ee, 0.0), 1.0) : 0.0;
    for (int k = 0; k < 3; ++k) o.v[k] = o.s * e3[k] - u3[k];
    return o;
}

struct ClrSegQuery {       // what the segment query asks and writes, whatever its obstacles are
    const float* p;        // (n_traj W, 3) waypoint positions, trajectories end to end
    int W;                 // waypoints of one trajectory (>= 2): segment blockIdx.x = (b, w), b = blockIdx.x / (W - 1)
    float r, weight;
    float* d;              // may be NULL: (n_traj (W - 1)) distance, +inf when no point is within r
    int* idx;              // may be NULL: (n_traj (W - 1)) caller row of the nearest point, -1 when none
    float* s;              // may be NULL: (n_traj (W - 1)) where along the segment the closest point lies (0 = a, 1 = b; 0 when idx = -1)
    double* term;          // (n_traj W) per-waypoint terms: entry b W + w = (r - d)^2 of segment (b, w)
    double* part;          // (n_traj (W - 1), 6) g_a, g_b of every segment in f64
};

struct ClrSegArgs : ClrSegQuery {
    CloudView cv;
};

// the waypoint row of segment seg's first end
__device__ __forceinline__ int64_t clr_seg_row(int64_t seg, int W) { return seg / (W - 1) * W + seg % (W - 1); }

// one thread: the segment's outputs, its term and its gradient parts from the block's winner
__device__ __forceinline__ void clr_seg_write(const ClrSegQuery& a, const ClrSegment& g, int64_t seg, int64_t row, unsigned long long best,
                                              const float (&x)[3]) {
    const ClrSegHit hit = clr_seg_finish(g, best, x);
    double term = 0.0, part[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (hit.idx >= 0) {
        const double h = (double)a.r - hit.d;
        term = h * h;
        double vv = 0.0;
        for (int k = 0; k < 3; ++k) vv += hit.v[k] * hit.v[k];
        if (vv > 0.0) {
            const double c = -2.0 * (double)a.weight * h / sqrt(vv);
            for (int k = 0; k < 3; ++k) {
                part[k] = c * (1.0 - hit.s) * hit.v[k];
                part[3 + k] = c * hit.s * hit.v[k];
            }
        }
    }
    if (a.d) a.d[seg] = (float)hit.d;
    if (a.idx) a.idx[seg] = hit.idx;
    if (a.s) a.s[seg] = (float)hit.s;
    a.term[row] = term;
    for (int k = 0; k < 6; ++k) a.part[6 * seg + k] = part[k];
}

__global__ void __launch_bounds__(TO_CLR_WAVES * 64) k_clearance_seg(ClrSegArgs a) {
    __shared__ unsigned long long sbest[TO_CLR_WAVES];
    const int64_t seg = blockIdx.x;
    const int64_t row = clr_seg_row(seg, a.W);
    const ClrSegment g(a.p + 3 * row, a.p + 3 * row + 3);
    unsigned long long best = clr_search<TO_CLR_WAVES>(a.cv, g, a.r, threadIdx.x >> 6);
    if (!clr_block_min(best, sbest)) return;
    float x[3];
    clr_cloud_point(a.cv, best, x);
    clr_seg_write(a, g, seg, row, best, x);
}

// arbitrary segments, one WAVE each: tohip_clearance_segments with n_wps = 2 would answer them with a block of 16 waves apiece
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
    const int64_t e = (int64_t)blockIdx.x * TO_EDGE_WAVES + (threadIdx.x >> 6);
    if (e >= a.E) return;   // (wave-uniform)
    const ClrSegment g(a.a + 3 * e, a.b + 3 * e);
    const unsigned long long best = clr_search<1>(a.cv, g, a.r, 0);
    if ((threadIdx.x & 63) != 0) return;
    float x[3];
    clr_cloud_point(a.cv, best, x);
    const ClrSegHit hit = clr_seg_finish(g, best, x);
    if (a.d) a.d[e] = (float)hit.d;
    if (a.idx) a.idx[e] = hit.idx;
    if (a.s) a.s[e] = (float)hit.s;
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

// TOHIP_TRAJ_CLEARANCE_PREFILLED: the scratch holds the caller's rows and terms while the step reads and writes its other buffers, so
// it must be a buffer of its own — none of `others`, the plan's other device buffers
static inline bool clearance_prefilled_ok(const void* scratch, std::initializer_list<const void*> others) {
    for (const void* o : others)
        if (o == scratch) return false;
    return true;
}

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

// tohip_clearance_segments' workspace: terms (n_traj W) f64 | the per-segment parts
static inline size_t clearance_seg_ws_term_bytes(int64_t W, int64_t n_traj) { return align_up((size_t)(W * n_traj) * 8, 256); }
static inline size_t clearance_seg_ws_bytes(int64_t W, int64_t n_traj) {
    return clearance_seg_ws_term_bytes(W, n_traj) + clearance_seg_part_bytes(W, n_traj);
}
static inline double* clearance_seg_ws_term(void* ws) { return (double*)ws; }
static inline double* clearance_seg_ws_part(void* ws, int64_t W, int64_t n_traj) {
    return (double*)((char*)ws + clearance_seg_ws_term_bytes(W, n_traj));
}

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
    return clearance_seg_counts_ok(n_wps, n_traj) ? clearance_seg_ws_bytes(n_wps, n_traj) : 0;
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
    double* term = clearance_seg_ws_term(workspace);
    int rc = clearance_seg_launch(packed, n_points, poses, n_wps, n_traj, radius, weight, d, idx, s, term,
                                  clearance_seg_ws_part(workspace, n_wps, n_traj), grad, st);
    if (rc != TOHIP_OK || !value) return rc;
    k_clearance_value<<<(unsigned)n_traj, 64, 0, st>>>(term, n_wps, weight, value);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
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
