// clearance_map_kernels.hip — the clearance term asked of the MAP: the obstacles are the voxels of an occupancy grid (DESIGN.md §10,
// "Clearance from the map"), not the points of a cloud.  Everything but the search is clearance_kernels.hip's: the two geometries
// (ClrPoint::d2, ClrSegment::d2), the key (float bits of d2) << 32 | index, the wave and block folds, the two finishes and the
// buffers they fill.  k_clearance_seg_rows and k_clearance_value follow unchanged.
//
//   obstacles   the occupied voxels inside dims; with a free plane (unknown = 'obstacle') the voxels of state 0 as well: per brick
//               word (occ | ~fre) & occ_brick_mask, field_row_nibble's rule.  A voxel IS the point at its centre, computed bit for
//               bit as k_occ_scatter (export) writes it: fl(o_a + fl(fl((float)i_a + 0.5f) r)) per axis.
//   winner      the argmin of d2 over d2 < fl(r r), ties to the lowest linear index (z ny + y) nx + x (31 bits: nx ny nz <= 2^31);
//               idx = that index, -1 when there is none or the query has a coordinate that is not finite.  So over the centres C
//               in ascending linear index the query equals the cloud query over a cloud of C bit for bit, idx through C's index.
//   window      the bricks that overlap the query's box — the waypoint, or the segment's two ends — grown by r and a slack of one
//               voxel plus the rounding of the float division, computed in float and clamped to the brick array BEFORE any
//               conversion to int (a waypoint 1e30 m away gets an empty window, not an overflow).  A superset: any centre with
//               d2 < fl(r r) lies in the box grown by r (1 + a few ulp), far inside the slack.
//   search      wave k of WAVES takes the window's words k 64 + lane, + WAVES 64, ...: a lane loads its word, skips it when it is
//               zero or when the brick's centre is farther from the query than rad plus the brick's half diagonal (3 voxels) with
//               clr_search's slack, in its !(>) form (a NaN keeps the brick), and walks the set bits with __ffs.  After each pass
//               of 64 words rad shrinks to the distance of the wave's best so far.  The prune only drops bricks that hold no
//               centre within rad, the minimum of the keys is order-free: the same bits for any number of waves.  No atomics.
//
// radius / resolution is at most 64 voxels (the entry points refuse more): a waypoint's window is at most 34 x 34 x 67 bricks.
namespace {

constexpr float kClrMapMaxVoxels = 64.f;

// the query's box (lo, hi per axis) and max |coordinate|
__device__ __forceinline__ void clr_box(const ClrPoint& t, float (&lo)[3], float (&hi)[3]) {
    lo[0] = hi[0] = t.tx, lo[1] = hi[1] = t.ty, lo[2] = hi[2] = t.tz;
}
__device__ __forceinline__ void clr_box(const ClrSegment& s, float (&lo)[3], float (&hi)[3]) {
    lo[0] = fminf(s.ax, s.bx), lo[1] = fminf(s.ay, s.by), lo[2] = fminf(s.az, s.bz);
    hi[0] = fmaxf(s.ax, s.bx), hi[1] = fmaxf(s.ay, s.by), hi[2] = fmaxf(s.az, s.bz);
}

// the bricks [b0, b0 + n) along one axis that can hold a centre within r of [lo, hi]; nb: bricks of the array along the axis, per:
// voxels per brick.  Float until clamped into [0, nb]
__device__ __forceinline__ void clr_window_axis(float lo, float hi, float r, float o, float res, float slack, int nb, float per, int& b0, int& n) {
    const float v0 = (lo - r - o) / res - slack, v1 = (hi + r - o) / res + slack;   // in voxels
    const float f0 = fminf(fmaxf(floorf(v0 / per), 0.f), (float)nb), f1 = fminf(fmaxf(floorf(v1 / per) + 1.f, 0.f), (float)nb);
    b0 = (int)f0;
    n = max((int)f1 - b0, 0);
}

struct ClrMap {
    const unsigned* occ;   // the occupied plane's words
    const unsigned* fre;   // the free plane's words, or NULL: unknown is free
    OccGeom g;
};

// the centre of voxel (x, y, z), export's bits
__device__ __forceinline__ void clr_map_centre(const OccGeom& g, int x, int y, int z, float (&c)[3]) {
    c[0] = __fadd_rn(g.ox, __fmul_rn((float)x + 0.5f, g.r));
    c[1] = __fadd_rn(g.oy, __fmul_rn((float)y + 0.5f, g.r));
    c[2] = __fadd_rn(g.oz, __fmul_rn((float)z + 0.5f, g.r));
}

// the winner's centre from its key (zeros when there is none)
__device__ __forceinline__ void clr_map_point(const OccGeom& g, unsigned long long best, float (&c)[3]) {
    c[0] = c[1] = c[2] = 0.f;
    if (best == ~0ull) return;
    const unsigned lin = (unsigned)(best & 0xffffffffull);
    clr_map_centre(g, (int)(lin % (unsigned)g.nx), (int)((lin / (unsigned)g.nx) % (unsigned)g.ny), (int)(lin / ((unsigned)g.nx * (unsigned)g.ny)), c);
}

// ---- the search: the smallest key over this wave's share of the window, the same in every lane; ~0 when no obstacle centre has
// d2 < fl(r r) or the query is not finite ----------------------------------------------------------------------------------------
template <int WAVES, class Geom>
__device__ __forceinline__ unsigned long long clr_map_search(const ClrMap& m, const Geom& q, float r, int wave) {
    unsigned long long best = ~0ull;
    if (!q.finite()) return best;
    const OccGeom& g = m.g;
    const int lane = threadIdx.x & 63;
    const float r2 = __fmul_rn(r, r);
    const float amax = fmaxf(q.max_abs(), fmaxf(fmaxf(fabsf(g.ox), fabsf(g.oy)), fabsf(g.oz)));
    float lo[3], hi[3];
    clr_box(q, lo, hi);
    const float slack = 1.f + 4e-6f * amax / g.r;   // one voxel, and the rounding of (p - o) / res and of the centres
    int bx0, by0, bz0, wx, wy, wz;
    clr_window_axis(lo[0], hi[0], r, g.ox, g.r, slack, g.nbx, 4.f, bx0, wx);
    clr_window_axis(lo[1], hi[1], r, g.oy, g.r, slack, g.nby, 4.f, by0, wy);
    clr_window_axis(lo[2], hi[2], r, g.oz, g.r, slack, (g.nz + 1) / 2, 2.f, bz0, wz);
    const int n_win = wx * wy * wz;   // at most the brick array's words, 2^28
    const float half = 3.f * g.r;     // a brick's half diagonal: 0.5 sqrt(16 + 16 + 4) voxels
    float rad = r;
    for (int base = 64 * wave; base < n_win; base += 64 * WAVES) {
        const int i = base + lane;
        if (i < n_win) {
            const int bx = bx0 + i % wx, by = by0 + (i / wx) % wy, bz = bz0 + i / (wx * wy);
            const int w = (bz * g.nby + by) * g.nbx + bx;
            unsigned bits = m.occ[w];
            if (m.fre) bits |= ~m.fre[w];
            bits &= occ_brick_mask(g, bx, by, bz);
            if (bits != 0u) {
                float c[3];   // the brick's centre, the corner of voxel (4 bx + 2, 4 by + 2, 2 bz + 1), in plain f32
                const float dc = q.centre_dist(make_float4(g.ox + (float)(4 * bx + 2) * g.r, g.oy + (float)(4 * by + 2) * g.r,
                                                           g.oz + (float)(2 * bz + 1) * g.r, 0.f));
                // dropped when |brick centre - query| - half > rad, with clr_search's room for the roundings; !(>): a NaN keeps it
                if (!(dc > (half + rad) * 1.0001f + 1e-5f * amax + 1e-6f)) {
                    while (bits != 0u) {
                        const int bit = __ffs(bits) - 1;
                        bits &= bits - 1u;
                        int x, y, z;
                        occ_voxel(bx, by, bz, bit, x, y, z);
                        clr_map_centre(g, x, y, z, c);
                        const float d2 = q.d2(c[0], c[1], c[2]);
                        if (d2 < r2) {
                            const unsigned lin = ((unsigned)z * (unsigned)g.ny + (unsigned)y) * (unsigned)g.nx + (unsigned)x;
                            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | lin;
                            best = key < best ? key : best;
                        }
                    }
                }
            }
        }
        best = clr_wave_min(best);   // uniform from here: the search radius shrinks to the best distance so far
        if (best != ~0ull) rad = sqrtf(__uint_as_float((unsigned)(best >> 32)));
    }
    return clr_wave_min(best);
}

struct ClrMapArgs : ClrQuery {
    ClrMap m;
};

__global__ void __launch_bounds__(TO_CLR_WAVES * 64) k_clearance_map(ClrMapArgs a) {
    __shared__ unsigned long long sbest[TO_CLR_WAVES];
    const int64_t w = blockIdx.x;   // the query
    const ClrPoint t(a.q + 3 * w);
    unsigned long long best = clr_map_search<TO_CLR_WAVES>(a.m, t, a.r, threadIdx.x >> 6);
    if (!clr_block_min(best, sbest)) return;
    float c[3];
    clr_map_point(a.m.g, best, c);
    clr_point_finish(a, t, w, best, c);
}

struct ClrMapSegArgs : ClrSegQuery {
    ClrMap m;
};

__global__ void __launch_bounds__(TO_CLR_WAVES * 64) k_clearance_map_seg(ClrMapSegArgs a) {
    __shared__ unsigned long long sbest[TO_CLR_WAVES];
    const int64_t seg = blockIdx.x;
    const int64_t row = clr_seg_row(seg, a.W);
    const ClrSegment g(a.p + 3 * row, a.p + 3 * row + 3);
    unsigned long long best = clr_map_search<TO_CLR_WAVES>(a.m, g, a.r, threadIdx.x >> 6);
    if (!clr_block_min(best, sbest)) return;
    float c[3];
    clr_map_point(a.m.g, best, c);
    clr_seg_write(a, g, seg, row, best, c);
}

// the map and the term's settings (occ_check's rules, then the planes, the radius and its cap); nothing is enqueued before this passes
inline int clearance_map_check(const void* occupied, const void* free_or_null, size_t grid_bytes, const tohip_occ_geom* geom, float radius,
                               float weight, ClrMap& m) {
    const int rc = occ_check(occupied, grid_bytes, geom, m.g);
    if (rc != TOHIP_OK) return rc;
    if (free_or_null == occupied || !clearance_args_ok(radius, weight)) return TOHIP_EINVAL;
    if (!((double)radius / (double)m.g.r <= (double)kClrMapMaxVoxels)) return TOHIP_EINVAL;
    m.occ = occ_data(occupied);
    m.fre = free_or_null ? occ_data(free_or_null) : nullptr;
    return TOHIP_OK;
}

}  // namespace

extern "C" int tohip_clearance_map(const void* occupied, const void* free_or_null, size_t grid_bytes, const tohip_occ_geom* geom,
                                   const float* queries, int64_t n_queries, float radius, float weight, float* d, int32_t* idx, float* value,
                                   float* grad, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    ClrMapArgs a;
    const int rc = clearance_map_check(occupied, free_or_null, grid_bytes, geom, radius, weight, a.m);
    if (rc != TOHIP_OK) return rc;
    if (!queries || !d || !idx || !workspace || n_queries <= 0 || n_queries > (int64_t)INT32_MAX) return TOHIP_EINVAL;
    if (workspace_bytes < tohip_clearance_workspace_bytes(n_queries)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    a.q = queries; a.nq = n_queries; a.r = radius; a.weight = weight;
    a.d = d; a.idx = idx; a.term = (double*)workspace; a.grad = grad; a.accumulate = accumulate;
    k_clearance_map<<<(unsigned)n_queries, TO_CLR_WAVES * 64, 0, st>>>(a);
    TO_HIP_CHECK_LAUNCH();
    if (!value) return TOHIP_OK;
    k_clearance_value<<<1, 64, 0, st>>>(a.term, n_queries, weight, value);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_clearance_map_segments(const void* occupied, const void* free_or_null, size_t grid_bytes, const tohip_occ_geom* geom,
                                            const float* poses, int64_t n_wps, int64_t n_traj, float radius, float weight, float* d,
                                            int32_t* idx, float* s, float* value, float* grad, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    ClrMapSegArgs a;
    const int rc = clearance_map_check(occupied, free_or_null, grid_bytes, geom, radius, weight, a.m);
    if (rc != TOHIP_OK) return rc;
    if (!poses || !d || !idx || !s || !workspace || !clearance_seg_counts_ok(n_wps, n_traj)) return TOHIP_EINVAL;
    if (workspace_bytes < tohip_clearance_segments_workspace_bytes(n_wps, n_traj)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    a.p = poses; a.W = (int)n_wps; a.r = radius; a.weight = weight;
    a.d = d; a.idx = idx; a.s = s;
    a.term = clearance_seg_ws_term(workspace);
    a.part = clearance_seg_ws_part(workspace, n_wps, n_traj);
    k_clearance_map_seg<<<(unsigned)(n_traj * (n_wps - 1)), TO_CLR_WAVES * 64, 0, st>>>(a);
    TO_HIP_CHECK_LAUNCH();
    const int64_t rows = n_traj * n_wps;
    k_clearance_seg_rows<<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(a.part, (int)n_wps, rows, a.term, grad);
    TO_HIP_CHECK_LAUNCH();
    if (!value) return TOHIP_OK;
    k_clearance_value<<<(unsigned)n_traj, 64, 0, st>>>(a.term, n_wps, weight, value);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
