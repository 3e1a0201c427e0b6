// occupancy_kernels.hip — a dense occupancy bit grid and exact integer line-of-sight walks through it, for gfx950.
//
// The grid: origin (3 x f32), resolution r, dims (nx, ny, nz), one bit per voxel.  A 32-bit word holds a brick of 4 x 4 x 2 voxels
// (bit = x&3 | (y&3)<<2 | (z&1)<<4), the bricks lie x fastest: a walk that stays inside a brick costs no load, and a ray along any
// axis changes word every second to fourth step.
//
//   coordinate of p  per axis g = (p - origin) / r in f32 (the division correctly rounded: numpy.float32 gives the same value), IN
//                    RANGE iff -2048 <= g < 4096 (false for NaN and inf) — the grid plus an apron in which everything is free —
//                    then q = (int) floorf(g * 256), the unit 1/256 voxel (the product is exact), voxel = q >> 8.
//   k_occ_insert     a row in range whose voxel lies inside dims: one 32-bit atomic OR; every other row is counted (per wave, one
//                    add per wave).  Bits are never cleared: two inserts = one insert of the concatenation, in any order.
//   k_occ_lookup     (M,3) int32 voxel indices -> uint8 (outside dims: 0).
//   occ_walk         the one walk of the map layer, A -> B in fixed point: D = B - A, s = sign D, m = |D|, v = A >> 8, e = B >> 8; per
//                    axis the distance to the next face n = (v+1)*256 - A (s > 0) or A - v*256 (s < 0, may be 0); sum |e - v| steps,
//                    each along the axis — among those with v_a != e_a — of the smallest n_a / m_a, compared as n_a m_b < n_b m_a in
//                    integers, ties to the lowest axis; then v_a += s_a, n_a += 256.  The three cross terms n_a m_b - n_b m_a (up to
//                    2^42: 64-bit) are kept incrementally — a step adds 256 m to two of them — so the loop has no multiply.
//                    occ_walk(state, stop_at, visit) calls visit at every voxel with cheb(v, e) > stop_at, in walk order, then steps;
//                    the state is left where the walk ended.  What happens at a voxel is the visitor's: line of sight here, the
//                    carve in frontier_kernels.hip, the field's minimum in field_kernels.hip.
//   los_walk         the visitor of line of sight, stop_at = end_skip: a visited voxel is TESTED iff cheb(v, v0) >= start_skip; the
//                    ray is blocked iff a tested voxel inside dims is occupied.  The last word loaded stays in a register.
//   k_los_segments   one lane per ray (a, b in world f32): 1 clear, 0 blocked, 2 an endpoint out of range.
//   k_los_rows       the occlusion refresh in one launch, grid (runs of 8 packed 256-point tiles) x (waypoints): per point the exact
//                    transform and frustum_pred — the device functions tohip_cull_waypoints runs, hence its bits — the kept points of
//                    the run are queued in LDS, the block's lanes walk the queue (a tenth of the points are kept: walking them where
//                    they lie leaves nine lanes of ten idle), a blocked ray clears its bit in LDS, and the run's words go out with
//                    one 32-bit store per 32 points.  A tile whose bounding sphere cannot pass the depth gate (with slack for every
//                    rounding involved: the prune never changes a bit) is not read at all.
//
// No float atomics, no process-wide state, nothing read back: the row refresh never synchronises with the host.
#include <cmath>

namespace {

constexpr size_t kOccHdr = 256;        // [0] u64: rows the last insert skipped
constexpr int kOccMaxDim = 2048;
constexpr int kOccBlocks = 2048;
constexpr int kLosRunTiles = 8;        // 256-point tiles per block of k_los_rows
constexpr int kLosRunPoints = kLosRunTiles * TO_BLOCK;

struct OccGeom {
    float ox, oy, oz, r;
    int nx, ny, nz;
    int nbx, nby;   // bricks along x and y
};

inline bool occ_dims_ok(int64_t nx, int64_t ny, int64_t nz) {
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= kOccMaxDim && ny <= kOccMaxDim && nz <= kOccMaxDim && nx * ny * nz <= (int64_t)1 << 31;
}
inline size_t occ_words(int64_t nx, int64_t ny, int64_t nz) { return (size_t)((nx + 3) / 4) * (size_t)((ny + 3) / 4) * (size_t)((nz + 1) / 2); }

inline int occ_check(const void* grid, size_t bytes, const tohip_occ_geom* geom, OccGeom& g) {
    if (!grid || !geom || !occ_dims_ok(geom->dims[0], geom->dims[1], geom->dims[2])) return TOHIP_EINVAL;
    if (!(geom->resolution > 0.f) || !std::isfinite(geom->resolution)) return TOHIP_EINVAL;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(geom->origin[a])) return TOHIP_EINVAL;
    g = OccGeom{geom->origin[0], geom->origin[1], geom->origin[2], geom->resolution, geom->dims[0], geom->dims[1], geom->dims[2],
                (geom->dims[0] + 3) / 4, (geom->dims[1] + 3) / 4};
    return bytes < kOccHdr + occ_words(g.nx, g.ny, g.nz) * 4 ? TOHIP_ENOSPC : TOHIP_OK;
}

inline unsigned* occ_data(void* grid) { return reinterpret_cast<unsigned*>((char*)grid + kOccHdr); }
inline const unsigned* occ_data(const void* grid) { return reinterpret_cast<const unsigned*>((const char*)grid + kOccHdr); }

inline int occ_grid_blocks(int64_t n) {
    const int64_t b = (n + TO_BLOCK - 1) / TO_BLOCK;
    return (int)(b < 1 ? 1 : (b > kOccBlocks ? kOccBlocks : b));
}

// fixed-point coordinate along one axis; false = out of range (q = 0 then)
__device__ __forceinline__ bool occ_axis(float p, float o, float r, int& q) {
    const float g = (p - o) / r;
    const bool ok = g >= -2048.f && g < 4096.f;   // (false for NaN)
    q = ok ? (int)floorf(g * 256.f) : 0;
    return ok;
}

__device__ __forceinline__ bool occ_fixed(const OccGeom& g, float x, float y, float z, int& qx, int& qy, int& qz) {
    return occ_axis(x, g.ox, g.r, qx) & occ_axis(y, g.oy, g.r, qy) & occ_axis(z, g.oz, g.r, qz);
}

__device__ __forceinline__ bool occ_inside(const OccGeom& g, int x, int y, int z) {
    return (unsigned)x < (unsigned)g.nx && (unsigned)y < (unsigned)g.ny && (unsigned)z < (unsigned)g.nz;
}
// word and bit of a voxel inside dims (at most 2^28 words)
__device__ __forceinline__ int occ_word(const OccGeom& g, int x, int y, int z) { return ((z >> 1) * g.nby + (y >> 2)) * g.nbx + (x >> 2); }
__device__ __forceinline__ int occ_bit(int x, int y, int z) { return (x & 3) | ((y & 3) << 2) | ((z & 1) << 4); }
// ... and back: the brick of word w, the voxel of a brick's bit
__device__ __forceinline__ void occ_brick(const OccGeom& g, long long w, int& bx, int& by, int& bz) {
    bx = (int)(w % g.nbx), by = (int)((w / g.nbx) % g.nby), bz = (int)(w / ((long long)g.nbx * g.nby));
}
__device__ __forceinline__ void occ_voxel(int bx, int by, int bz, int bit, int& x, int& y, int& z) {
    x = 4 * bx + (bit & 3), y = 4 * by + ((bit >> 2) & 3), z = 2 * bz + (bit >> 4);
}

// where the world point p[0 .. 2] lies, and its voxel (that of fixed point 0 on an axis out of range)
enum OccPlace { kOccOutOfRange, kOccOutsideDims, kOccInside };
__device__ __forceinline__ OccPlace occ_locate(const OccGeom& g, const float* __restrict__ p, int& x, int& y, int& z) {
    int qx, qy, qz;
    const bool ok = occ_fixed(g, p[0], p[1], p[2], qx, qy, qz);
    x = qx >> 8, y = qy >> 8, z = qz >> 8;
    return !ok ? kOccOutOfRange : (occ_inside(g, x, y, z) ? kOccInside : kOccOutsideDims);
}

// both ends of a leg a -> b in fixed point; false = an endpoint out of range
__device__ __forceinline__ bool occ_fixed_leg(const OccGeom& g, const float* __restrict__ a, const float* __restrict__ b, int& ax, int& ay, int& az,
                                              int& bx, int& by, int& bz) {
    return occ_fixed(g, a[0], a[1], a[2], ax, ay, az) & occ_fixed(g, b[0], b[1], b[2], bx, by, bz);
}

// sum over the wave, added once per wave (every lane of the wave calls this)
__device__ __forceinline__ void occ_count(unsigned long long* word, long long c) {
    for (int sh = 32; sh > 0; sh >>= 1) c += __shfl_xor(c, sh);
    if ((threadIdx.x & 63) == 0 && c != 0) __hip_atomic_fetch_add(word, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_insert(unsigned long long* __restrict__ hdr, unsigned* __restrict__ words, OccGeom g, const float* __restrict__ pts, long long n) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    long long skipped = 0;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n; i += stride) {
        int x, y, z;
        if (occ_locate(g, pts + 3 * i, x, y, z) == kOccInside)
            __hip_atomic_fetch_or(words + occ_word(g, x, y, z), 1u << occ_bit(x, y, z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            ++skipped;
    }
    occ_count(hdr, skipped);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_lookup(const unsigned* __restrict__ words, OccGeom g, const int* __restrict__ ijk, long long m, uint8_t* __restrict__ out) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < m; i += stride) {
        const int x = ijk[3 * i], y = ijk[3 * i + 1], z = ijk[3 * i + 2];
        out[i] = occ_inside(g, x, y, z) ? (uint8_t)((words[occ_word(g, x, y, z)] >> occ_bit(x, y, z)) & 1u) : (uint8_t)0;
    }
}

struct LosAxis {
    int v, s, rem, taken;   // voxel, direction, |e - v|, steps taken along this axis
    long long m;            // |D|
};

__device__ __forceinline__ LosAxis los_axis(int a, int b, long long& n) {
    LosAxis x;
    const int d = b - a;
    x.v = a >> 8;
    x.s = d > 0 ? 1 : (d < 0 ? -1 : 0);
    x.m = d < 0 ? -(long long)d : (long long)d;
    const int e = b >> 8;
    x.rem = e > x.v ? e - x.v : x.v - e;
    x.taken = 0;
    n = x.s > 0 ? (long long)(x.v + 1) * 256 - a : (long long)a - (long long)x.v * 256;
    return x;
}

struct OccWalk {
    LosAxis X, Y, Z;
    long long c01, c02, c12, sx, sy, sz;   // the cross terms n_a m_b - n_b m_a and their increments 256 m
};

__device__ __forceinline__ OccWalk occ_walk_begin(int ax, int ay, int az, int bx, int by, int bz) {
    OccWalk k;
    long long n0, n1, n2;
    k.X = los_axis(ax, bx, n0), k.Y = los_axis(ay, by, n1), k.Z = los_axis(az, bz, n2);
    k.c01 = n0 * k.Y.m - n1 * k.X.m, k.c02 = n0 * k.Z.m - n2 * k.X.m, k.c12 = n1 * k.Z.m - n2 * k.Y.m;
    k.sx = 256 * k.X.m, k.sy = 256 * k.Y.m, k.sz = 256 * k.Z.m;
    return k;
}

// visit(k) at every voxel whose Chebyshev distance to the end voxel exceeds stop_at, in walk order, then the step; true = the visitor
// stopped the walk.  k is left at the voxel where the walk ended.  (The distance only falls along the walk.)
template <class Visit>
__device__ __forceinline__ bool occ_walk(OccWalk& k, int stop_at, Visit&& visit) {
    LosAxis &X = k.X, &Y = k.Y, &Z = k.Z;
    for (;;) {
        if (max(X.rem, max(Y.rem, Z.rem)) <= stop_at) return false;
        if (visit(k)) return true;
        // (some axis is active)
        const bool a0 = X.rem > 0, a1 = Y.rem > 0, a2 = Z.rem > 0;
        if (a0 && (!a1 || k.c01 <= 0) && (!a2 || k.c02 <= 0)) {
            X.v += X.s; --X.rem; ++X.taken; k.c01 += k.sy; k.c02 += k.sz;
        } else if (a1 && (!a2 || k.c12 <= 0)) {
            Y.v += Y.s; --Y.rem; ++Y.taken; k.c01 -= k.sx; k.c12 += k.sz;
        } else {
            Z.v += Z.s; --Z.rem; ++Z.taken; k.c02 -= k.sx; k.c12 -= k.sy;
        }
    }
}

// 1 = clear, 0 = blocked; visits: the voxels the walk looked at (for the statistics)
__device__ __forceinline__ int los_walk(const unsigned* __restrict__ words, const OccGeom& g, int ax, int ay, int az, int bx, int by, int bz,
                                        int start_skip, int end_skip, unsigned& visits) {
    OccWalk k = occ_walk_begin(ax, ay, az, bx, by, bz);
    int cur = -1;
    unsigned word = 0;
    return !occ_walk(k, end_skip, [&](const OccWalk& at) {
        const int x = at.X.v, y = at.Y.v, z = at.Z.v;
        ++visits;
        if (max(at.X.taken, max(at.Y.taken, at.Z.taken)) < start_skip || !occ_inside(g, x, y, z)) return false;
        const int w = occ_word(g, x, y, z);
        if (w != cur) { word = words[w]; cur = w; }
        return (bool)((word >> occ_bit(x, y, z)) & 1u);
    });
}

__global__ void __launch_bounds__(TO_BLOCK)
k_los_segments(const unsigned* __restrict__ words, OccGeom g, const float* __restrict__ a, const float* __restrict__ b, long long n_rays,
               int start_skip, int end_skip, uint8_t* __restrict__ out, unsigned long long* __restrict__ stats) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    long long rays = 0, visits = 0;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n_rays; i += stride) {
        int ax, ay, az, bx, by, bz;
        const bool ok = occ_fixed_leg(g, a + 3 * i, b + 3 * i, ax, ay, az, bx, by, bz);
        int r = 2;
        if (ok) {
            unsigned v = 0;
            r = los_walk(words, g, ax, ay, az, bx, by, bz, start_skip, end_skip, v);
            ++rays;
            visits += v;
        }
        out[i] = (uint8_t)r;
    }
    if (stats) { occ_count(stats, rays); occ_count(stats + 1, visits); }
}

struct LosRowsArgs {
    const unsigned* words;
    OccGeom g;
    CloudView cv;
    const float* poses;
    const float* quats;
    FrustumConsts f;
    int start_skip, end_skip, prune;
    int row_words;   // npad / 32
    int* rows;
    unsigned long long* stats;
};

// can any point of the tile's bounding sphere pass the depth gate of this camera?  Z of a point = Z of the centre + (unit axis) .
// (p - c): within rad of it in exact arithmetic; the slack covers the rounding of the centre's and of every point's transform (a few
// ulp of the coordinates and of |p - t|, taken a hundredfold) and of a quaternion whose norm is 1 to a few ulp.
__device__ __forceinline__ bool los_tile_reachable(const ExactPose& e, const FrustumConsts& f, const float4 b) {
    if (!(finite3(b.x, b.y, b.z) && isfinite(b.w))) return true;
    float X, Y, Z;
    exact_to_cam(e, b.x, b.y, b.z, X, Y, Z);
    const float reach = fabsf(X) + fabsf(Y) + fabsf(Z) + b.w;   // >= |p - t| of every point of the tile
    const float big = fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fabsf(b.z)) + b.w + fmaxf(fmaxf(fabsf(e.t[0]), fabsf(e.t[1])), fabsf(e.t[2]));
    const float slack = 1e-5f * (big + reach) + 1e-6f;
    const float rad = b.w * 1.0001f + slack;
    if (!isfinite(Z) || !isfinite(rad)) return true;
    return !(Z - rad >= f.dmax) && !(Z + rad <= f.dmin);
}

__global__ void __launch_bounds__(TO_BLOCK) k_los_rows(LosRowsArgs a) {
    __shared__ unsigned s_words[kLosRunPoints / 32];
    __shared__ unsigned short s_queue[kLosRunPoints];
    __shared__ int s_count;
    const int w = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long ntiles = a.cv.npad / TO_BLOCK;
    const long long tile_first = (long long)blockIdx.x * kLosRunTiles;
    const ExactPose e = exact_pose(a.quats + 4 * w, a.poses + 3 * w, 1);
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    // pass 1: the exact cull of every point of the run; the kept points' bits and a queue of their places
    for (int j = 0; j < kLosRunTiles; ++j) {
        const long long tile = tile_first + j;
        if (tile >= ntiles) break;   // (uniform)
        unsigned long long kept = 0ull;
        if (!a.prune || los_tile_reachable(e, a.f, a.cv.bounds[tile])) {   // (uniform)
            const long long i = tile * TO_BLOCK + threadIdx.x;
            bool d = false, v = false;
            if (i < a.cv.n) {
                float X, Y, Z;
                exact_to_cam(e, a.cv.soa[i], a.cv.soa[a.cv.npad + i], a.cv.soa[2 * a.cv.npad + i], X, Y, Z);
                frustum_pred(a.f, X, Y, Z, d, v);
            }
            kept = __ballot(d && v);
            if (kept != 0ull) {   // (wave-uniform)
                int base = 0;
                if (lane == 0) base = atomicAdd(&s_count, __popcll(kept));
                base = __shfl(base, 0);
                if ((kept >> lane) & 1ull) s_queue[base + __popcll(kept & ((1ull << lane) - 1ull))] = (unsigned short)(j * TO_BLOCK + threadIdx.x);
            }
        }
        if (lane == 0) {
            s_words[j * (TO_BLOCK / 32) + 2 * wave] = (unsigned)kept;
            s_words[j * (TO_BLOCK / 32) + 2 * wave + 1] = (unsigned)(kept >> 32);
        }
    }
    __syncthreads();
    // pass 2: the block's lanes walk the queue; a blocked ray clears its bit.  A camera out of range: every ray is skipped = clear.
    long long rays = 0, visits = 0;
    int cx, cy, cz;
    const bool cam_ok = occ_fixed(a.g, e.t[0], e.t[1], e.t[2], cx, cy, cz);   // (uniform)
    const int count = cam_ok ? s_count : 0;
    for (int k = threadIdx.x; k < count; k += TO_BLOCK) {
        const int li = s_queue[k];
        const long long i = tile_first * TO_BLOCK + li;
        int px, py, pz;
        if (!occ_fixed(a.g, a.cv.soa[i], a.cv.soa[a.cv.npad + i], a.cv.soa[2 * a.cv.npad + i], px, py, pz)) continue;
        unsigned v = 0;
        const int clear = los_walk(a.words, a.g, cx, cy, cz, px, py, pz, a.start_skip, a.end_skip, v);
        if (!clear) atomicAnd(&s_words[li >> 5], ~(1u << (li & 31)));
        ++rays;
        visits += v;
    }
    __syncthreads();
    const long long word0 = tile_first * (TO_BLOCK / 32);
    if ((int)threadIdx.x < kLosRunPoints / 32 && word0 + threadIdx.x < a.row_words)
        a.rows[(long long)w * a.row_words + word0 + threadIdx.x] = (int)s_words[threadIdx.x];
    if (a.stats) { occ_count(a.stats, rays); occ_count(a.stats + 1, visits); }
}

// the row count of a query
inline bool occ_count_ok(int64_t n) { return n >= 0 && n <= (int64_t)1 << 40; }

// one int64 of device memory -> *host (null: not asked, nothing is read back); synchronises
inline int occ_read_back(int64_t* host, const void* dev, hipStream_t st) {
    if (!host) return TOHIP_OK;
    hipError_t e = hipMemcpyAsync(host, dev, sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? TOHIP_OK : (int)e;
}

inline bool los_skips_ok(int start_skip, int end_skip) { return start_skip >= 0 && end_skip >= 0 && start_skip <= 8192 && end_skip <= 8192; }

}  // namespace

extern "C" size_t tohip_occ_bytes(int32_t nx, int32_t ny, int32_t nz) {
    return occ_dims_ok(nx, ny, nz) ? kOccHdr + occ_words(nx, ny, nz) * 4 : 0;
}

extern "C" int tohip_occ_init(void* grid, size_t grid_bytes, const tohip_occ_geom* geom, void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    const hipError_t e = hipMemsetAsync(grid, 0, kOccHdr + occ_words(g.nx, g.ny, g.nz) * 4, (hipStream_t)stream_);
    return e == hipSuccess ? TOHIP_OK : (int)e;
}

extern "C" int tohip_occ_insert(void* grid, size_t grid_bytes, const tohip_occ_geom* geom, const float* points, int64_t n,
                                int64_t* skipped_host, void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occ_count_ok(n) || (n > 0 && !points)) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(grid, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    if (n > 0) {
        k_occ_insert<<<occ_grid_blocks(n), TO_BLOCK, 0, st>>>((unsigned long long*)grid, occ_data(grid), g, points, n);
        TO_HIP_CHECK_LAUNCH();
    }
    return occ_read_back(skipped_host, grid, st);
}

extern "C" int tohip_occ_lookup(const void* grid, size_t grid_bytes, const tohip_occ_geom* geom, const int32_t* ijk, int64_t m, uint8_t* out,
                                void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occ_count_ok(m) || (m > 0 && (!ijk || !out))) return TOHIP_EINVAL;
    if (m == 0) return TOHIP_OK;
    k_occ_lookup<<<occ_grid_blocks(m), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(grid), g, ijk, m, out);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_los_segments(const void* grid, size_t grid_bytes, const tohip_occ_geom* geom, const float* a, const float* b,
                                  int64_t n_rays, int32_t start_skip, int32_t end_skip, uint8_t* out, uint64_t* stats, void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occ_count_ok(n_rays) || (n_rays > 0 && (!a || !b || !out)) || !los_skips_ok(start_skip, end_skip)) return TOHIP_EINVAL;
    if (n_rays == 0) return TOHIP_OK;
    k_los_segments<<<occ_grid_blocks(n_rays), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(grid), g, a, b, n_rays, start_skip, end_skip, out,
                                                                                  (unsigned long long*)stats);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_los_rows(const void* grid, size_t grid_bytes, const tohip_occ_geom* geom, const void* packed, int64_t n_points,
                              const float* poses, const float* quats, int64_t n_wps, const tohip_camera* cam, float min_dist, float max_dist,
                              int32_t start_skip, int32_t end_skip, int32_t prune, int32_t* rows, uint64_t* stats, void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!packed || !poses || !quats || !cam || !rows || n_points <= 0 || n_points > (int64_t)0x7fffffff || n_wps <= 0 || n_wps > 65535 ||
        !los_skips_ok(start_skip, end_skip))
        return TOHIP_EINVAL;
    LosRowsArgs a;
    a.words = occ_data(grid);
    a.g = g;
    a.cv = cloud_view(packed, n_points);
    a.poses = poses;
    a.quats = quats;
    for (int i = 0; i < 9; ++i) a.f.k[i] = cam->K[i];
    a.f.wl = (float)((double)cam->img_width - 1.0);
    a.f.hl = (float)((double)cam->img_height - 1.0);
    a.f.dmin = min_dist;
    a.f.dmax = max_dist;
    a.start_skip = start_skip;
    a.end_skip = end_skip;
    a.prune = prune;
    a.row_words = (int)(a.cv.npad / 32);
    a.rows = rows;
    a.stats = (unsigned long long*)stats;
    const int64_t ntiles = a.cv.npad / TO_BLOCK;
    const dim3 grid_dim((unsigned)((ntiles + kLosRunTiles - 1) / kLosRunTiles), (unsigned)n_wps);
    k_los_rows<<<grid_dim, TO_BLOCK, 0, (hipStream_t)stream_>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
