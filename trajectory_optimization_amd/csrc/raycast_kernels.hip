// raycast_kernels.hip — where a ray through the map stops: first hits of segments, and the depth image a sensor at a pose would
// return ("Ray casts and depth scans"), for gfx950.  Included after volume_kernels.hip: the geometry, the fixed-point
// coordinates, the brick layout and the walk (occ_walk, occ_fixed, occ_word / occ_bit) are the occupancy file's, the gathered marks
// (carve_mark / carve_flush) the frontier file's, the pose (exact_pose) the cull's.  No kernel of those files is edited.
//
// The CAST of A -> B (fixed point, both in range) with (start_skip, end_skip): occ_walk, unchanged; the HIT is the first visited
// voxel that los_walk would call occupied — cheb(v, v0) >= start_skip, cheb(v, e) > end_skip (the walk's own stop), inside dims, bit
// set.  Its ENTRY PARAMETER is the crossing parameter n_a / m_a (n before the += 256) of the last step taken before the walk stood
// on it, 0/1 with no step taken: max over the axes with k_a > 0 steps of (n_a0 + 256 (k_a - 1)) / m_a, compared by cross products
// in 64-bit integers (every term < 2^21).  lam = fl(f32(num) / f32(den)): both exact in f32, one correctly rounded division, so
// equal rationals give equal bits.
//
//   cast_walk         the visitor: los_walk's test with the last loaded word in a register; the state is left at the hit, and the
//                     entry rational is formed once, behind the walk, from the steps taken per axis.
//   cast_mark         the first `n` voxels of the same walk get their bit in a pass plane (carve_mark, flushed on exit).  It is a
//                     second walk and not part of cast_walk: whether a ray of a scan marks anything is known only at its hit (a
//                     hit nearer than min_dist marks nothing), and bits that are only ever set cannot be taken back.
//   k_cast_segments   one lane per ray in k_los_segments' grid-stride launch: voxel (linear index, -1 clear, -2 out of range) and
//                     lam (1 clear, NaN out of range).
//   k_depth_scan      grid (16 x 16 pixel tiles) x (views), 256 lanes, a wave an 8 x 8 sub-tile: neighbouring rays share bricks
//                     (the cached word hits) and have walks of similar length.  The pose is uniform per block.  Per lane the ray
//                     in f32, every operation rounded (-ffp-contract=off): dc = ((x - cx) / fx, (y - cy) / fy, 1), Fc = (dc.x D,
//                     dc.y D, D), B = rot(q, Fc) + t — exact_to_cam's two Hamilton products with q and its conjugate exchanged —
//                     then occ_fixed of both ends, the cast with skip (1, 0), the outputs, the marks.  hit_plane: one atomic OR
//                     per flag-0 hit, issued only where the word lacks the bit (k_occ_carve's rule).
//
// No float atomics, no process-wide state, nothing read back; every argument check returns before anything is enqueued.
namespace {

constexpr int kScanTile = 16;        // pixels per side of a block's tile (TO_BLOCK = 16 x 16 lanes)
constexpr int kScanMaxSide = 8192;   // pixels per side of an image

struct CastResult {
    bool hit;
    int x, y, z;          // the hit voxel
    long long num, den;   // its entry parameter
};

// n_a0 + 256 (k_a - 1) over m_a joins the maximum
__device__ __forceinline__ void cast_entry_axis(const LosAxis& X, int a, long long& num, long long& den) {
    if (X.taken <= 0) return;
    const int v0 = a >> 8;
    const long long n0 = X.s > 0 ? (long long)(v0 + 1) * 256 - a : (long long)a - (long long)v0 * 256;
    const long long n = n0 + 256ll * (X.taken - 1);
    if (n * den > num * X.m) { num = n; den = X.m; }
}

// A -> B in fixed point (both in range).  visits: the voxels the walk looked at.
__device__ __forceinline__ CastResult cast_walk(const unsigned* __restrict__ words, const OccGeom& g, int ax, int ay, int az, int bx, int by, int bz,
                                                int start_skip, int end_skip, unsigned& visits) {
    OccWalk k = occ_walk_begin(ax, ay, az, bx, by, bz);
    int cur = -1;
    unsigned word = 0;
    CastResult r;
    r.hit = occ_walk(k, end_skip, [&](const OccWalk& at) {
        const int x = at.X.v, y = at.Y.v, z = at.Z.v;
        ++visits;
        if (max(at.X.taken, max(at.Y.taken, at.Z.taken)) < start_skip || !occ_inside(g, x, y, z)) return false;
        const int w = occ_word(g, x, y, z);
        if (w != cur) { word = words[w]; cur = w; }
        return (bool)((word >> occ_bit(x, y, z)) & 1u);
    });
    r.x = k.X.v, r.y = k.Y.v, r.z = k.Z.v;
    r.num = 0, r.den = 1;
    if (r.hit) {
        cast_entry_axis(k.X, ax, r.num, r.den);
        cast_entry_axis(k.Y, ay, r.num, r.den);
        cast_entry_axis(k.Z, az, r.num, r.den);
    }
    return r;
}

__device__ __forceinline__ float cast_lam(const CastResult& r) { return (float)r.num / (float)r.den; }
__device__ __forceinline__ int cast_index(const OccGeom& g, const CastResult& r) { return r.x + g.nx * (r.y + g.ny * r.z); }

// the first n voxels of the walk A -> B (stop_at 0) that lie inside dims get their bit in `pass`
__device__ __forceinline__ void cast_mark(unsigned* pass, const OccGeom& g, int ax, int ay, int az, int bx, int by, int bz, unsigned n,
                                          unsigned& atomics) {
    OccWalk k = occ_walk_begin(ax, ay, az, bx, by, bz);
    int cur = -1;
    unsigned bits = 0;
    occ_walk(k, 0, [&](const OccWalk& at) {
        if (n == 0u) return true;
        --n;
        return carve_mark(pass, g, at, cur, bits, atomics);
    });
    carve_flush(pass, cur, bits, atomics);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_cast_segments(const unsigned* __restrict__ words, OccGeom g, const float* __restrict__ a, const float* __restrict__ b, long long n_rays,
                int start_skip, int end_skip, int* __restrict__ voxel, float* __restrict__ lam, unsigned long long* __restrict__ stats) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    long long rays = 0, visits = 0;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n_rays; i += stride) {
        int ax, ay, az, bx, by, bz;
        const bool ok = occ_fixed_leg(g, a + 3 * i, b + 3 * i, ax, ay, az, bx, by, bz);
        int v = -2;
        float l = __int_as_float(0x7fc00000);
        if (ok) {
            unsigned n = 0;
            const CastResult r = cast_walk(words, g, ax, ay, az, bx, by, bz, start_skip, end_skip, n);
            v = r.hit ? cast_index(g, r) : -1;
            l = r.hit ? cast_lam(r) : 1.f;
            ++rays;
            visits += n;
        }
        voxel[i] = v;
        lam[i] = l;
    }
    if (stats) { occ_count(stats, rays); occ_count(stats + 1, visits); }
}

struct DepthScanArgs {
    const unsigned* words;
    unsigned* hit;    // may be null
    unsigned* pass;   // may be null
    OccGeom g;
    const float* poses;
    const float* quats;
    float fx, fy, cx, cy, dmin, dmax;
    int W, H, tiles_x;
    int* voxel;
    float* depth;
    uint8_t* flags;
    float* points;    // may be null
    unsigned long long* stats;
};

// q (0, v) conj(q): exact_to_cam's two products, the roles of q and its conjugate exchanged, the same order of terms
__device__ __forceinline__ void scan_rotate(const ExactPose& e, float bx, float by, float bz, float& r0, float& r1, float& r2) {
    const float aw = e.q[0], ax = e.q[1], ay = e.q[2], az = e.q[3];
    const float cw = e.q[0], cx = -e.q[1], cy = -e.q[2], cz = -e.q[3];
    const float bw = 0.f;
    const float ow = aw * bw - ax * bx - ay * by - az * bz;
    const float ox = aw * bx + ax * bw + ay * bz - az * by;
    const float oy = aw * by - ax * bz + ay * bw + az * bx;
    const float oz = aw * bz + ax * by - ay * bx + az * bw;
    r0 = ow * cx + ox * cw + oy * cz - oz * cy;
    r1 = ow * cy - ox * cz + oy * cw + oz * cx;
    r2 = ow * cz + ox * cy - oy * cx + oz * cw;
}

__global__ void __launch_bounds__(TO_BLOCK) k_depth_scan(DepthScanArgs a) {
    const int w = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int x = tx * kScanTile + (wave & 1) * 8 + (lane & 7), y = ty * kScanTile + (wave >> 1) * 8 + (lane >> 3);
    const ExactPose e = exact_pose(a.quats + 4 * (long long)w, a.poses + 3 * (long long)w, 1);   // (uniform)
    int cx, cy, cz;
    const bool cam_ok = occ_fixed(a.g, e.t[0], e.t[1], e.t[2], cx, cy, cz);   // (uniform)
    long long rays = 0, visits = 0, atomics = 0;
    if (x < a.W && y < a.H) {
        const float D = a.dmax, nan = __int_as_float(0x7fc00000);
        const float dx = ((float)x - a.cx) / a.fx, dy = ((float)y - a.cy) / a.fy;
        float r0, r1, r2;
        scan_rotate(e, dx * D, dy * D, D, r0, r1, r2);
        const float Bx = r0 + e.t[0], By = r1 + e.t[1], Bz = r2 + e.t[2];
        int bx, by, bz;
        const bool ok = occ_fixed(a.g, Bx, By, Bz, bx, by, bz) & cam_ok;
        int vox = -2, flag = 2;
        float dep = nan, px = nan, py = nan, pz = nan;
        if (ok) {
            unsigned n = 0, at = 0;
            const CastResult r = cast_walk(a.words, a.g, cx, cy, cz, bx, by, bz, 1, 0, n);
            ++rays;
            visits += n;
            if (r.hit) {
                vox = cast_index(a.g, r);
                dep = cast_lam(r) * D;
                flag = dep > a.dmin ? 0 : 3;
            } else {
                vox = -1, flag = 1, dep = __int_as_float(0x7f800000);
                px = Bx, py = By, pz = Bz;
            }
            if (flag == 0) {
                vol_centre(a.g, r.x, r.y, r.z, px, py, pz);
                if (a.hit) {
                    const int hw = occ_word(a.g, r.x, r.y, r.z);
                    const unsigned bit = 1u << occ_bit(r.x, r.y, r.z);
                    if (!(a.hit[hw] & bit)) {
                        __hip_atomic_fetch_or(a.hit + hw, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ++at;
                    }
                }
            }
            // the voxels in front of the hit (every visited voxel of a clear ray); a hit nearer than min_dist marks nothing
            if (a.pass && flag != 3) cast_mark(a.pass, a.g, cx, cy, cz, bx, by, bz, r.hit ? n - 1u : n, at);
            atomics += at;
        }
        const long long o = ((long long)w * a.H + y) * a.W + x;
        a.voxel[o] = vox;
        a.depth[o] = dep;
        a.flags[o] = (uint8_t)flag;
        if (a.points) { a.points[3 * o] = px; a.points[3 * o + 1] = py; a.points[3 * o + 2] = pz; }
    }
    if (a.stats) { occ_count(a.stats, rays); occ_count(a.stats + 1, visits); occ_count(a.stats + 2, atomics); }
}

// an image side: an integral value in [1, 8192]
inline bool scan_side_ok(float v, int& out) {
    if (!(v >= 1.f && v <= (float)kScanMaxSide) || v != std::floor(v)) return false;
    out = (int)v;
    return true;
}

}  // namespace

extern "C" int tohip_cast_segments(const void* grid, size_t grid_bytes, const tohip_occ_geom* geom, const float* a, const float* b,
                                   int64_t n_rays, int32_t start_skip, int32_t end_skip, int32_t* voxel, float* lam, uint64_t* stats,
                                   void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occ_count_ok(n_rays) || (n_rays > 0 && (!a || !b || !voxel || !lam)) || !los_skips_ok(start_skip, end_skip)) return TOHIP_EINVAL;
    if (n_rays == 0) return TOHIP_OK;
    k_cast_segments<<<occ_grid_blocks(n_rays), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(grid), g, a, b, n_rays, start_skip, end_skip, voxel,
                                                                                   lam, (unsigned long long*)stats);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_depth_scan(const void* grid, size_t grid_bytes, const tohip_occ_geom* geom, const float* poses, const float* quats,
                                int64_t n_views, const tohip_camera* cam, float min_dist, float max_dist, void* hit_plane, void* pass_plane,
                                int32_t* voxel, float* depth, uint8_t* flags, float* points, uint64_t* stats, void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!poses || !quats || !cam || !voxel || !depth || !flags || n_views < 1 || n_views > 65535) return TOHIP_EINVAL;
    const float* K = cam->K;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(K[i])) return TOHIP_EINVAL;
    if (!(K[0] > 0.f) || !(K[4] > 0.f) || K[1] != 0.f || K[3] != 0.f || K[6] != 0.f || K[7] != 0.f || K[8] != 1.f) return TOHIP_EINVAL;
    int W, H;
    if (!scan_side_ok(cam->img_width, W) || !scan_side_ok(cam->img_height, H)) return TOHIP_EINVAL;
    if (n_views * (int64_t)H * (int64_t)W >= (int64_t)1 << 31) return TOHIP_EINVAL;
    if (!std::isfinite(min_dist) || !std::isfinite(max_dist) || !(min_dist >= 0.f) || !(min_dist < max_dist)) return TOHIP_EINVAL;
    if ((hit_plane && hit_plane == grid) || (pass_plane && pass_plane == grid) || (hit_plane && hit_plane == pass_plane)) return TOHIP_EINVAL;
    DepthScanArgs a;
    a.words = occ_data(grid);
    a.hit = hit_plane ? occ_data(hit_plane) : nullptr;
    a.pass = pass_plane ? occ_data(pass_plane) : nullptr;
    a.g = g;
    a.poses = poses;
    a.quats = quats;
    a.fx = K[0], a.fy = K[4], a.cx = K[2], a.cy = K[5];
    a.dmin = min_dist, a.dmax = max_dist;
    a.W = W, a.H = H;
    a.tiles_x = (W + kScanTile - 1) / kScanTile;
    a.voxel = voxel;
    a.depth = depth;
    a.flags = flags;
    a.points = points;
    a.stats = (unsigned long long*)stats;
    const dim3 grid_dim((unsigned)(a.tiles_x * ((H + kScanTile - 1) / kScanTile)), (unsigned)n_views);
    k_depth_scan<<<grid_dim, TO_BLOCK, 0, (hipStream_t)stream_>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
