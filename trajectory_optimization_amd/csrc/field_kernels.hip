// field_kernels.hip — a conservative clearance field over the occupancy grid ("Clearance field"), for gfx950.  Included
// right after frontier_kernels.hip: the geometry, the fixed-point coordinates, the brick layout, the brick mask and the walk
// (occ_walk) are those files'.
//
// The FIELD has the grid's geometry and one uint16 per voxel inside dims, dense, x fastest: index (z ny + y) nx + x.  Obstacles: the
// occupied voxels inside dims and, with a free plane, also the voxels of state 0 (neither bit).  Metric: the gap between voxel cubes,
// gap2(v, u) = sum over the axes of max(|v_a - u_a| - 1, 0)^2 — an exact integer and a lower bound, in voxels, on the distance
// between any point of the one cube and any point of the other.  field[v] = min over the obstacles u of gap2(v, u) where that is
// <= D^2 (1 <= D <= 254), else the sentinel 65535.
//
//   k_field_x        one lane per voxel in a grid-stride loop: the nearest obstacle bit of the voxel's own x row on either side,
//                    found a brick at a time — the four x bits of the row in a word are one nibble, clz / ffs name the nearest — and
//                    the search ends at the brick whose nearest voxel is no nearer than the best found or than D + 1.
//   k_field_axis     the y and the z pass, min-plus with the per-axis cost max(|k| - 1, 0)^2 over the window +-(D + 1), values above
//                    D^2 dropped: one lane per voxel with x fastest, so a wave's loads at every offset are contiguous in x; offsets
//                    run outward from 0 and the loop ends once the offset's own cost reaches the best so far, which makes a voxel
//                    near an obstacle cheap.  The three passes ping-pong: x -> field, y -> workspace, z -> field.  A nearest
//                    obstacle within D has every partial sum <= D^2 and every finite value is some obstacle's true value, so the
//                    truncated passes give the exact truncated minimum.
//   k_field_positions  (M,3) f32 positions -> int32: the voxel's value, 65535 in range but outside dims, -1 out of range; optionally
//                    metres, fl(fl(sqrt(d2)) r), +inf for 65535, NaN for -1.
//   edt_walk         occ_walk with stop_at = 0 and a visitor that never stops it, v_T behind the walk: the minimum of the field over
//                    v_0 ... v_T inside dims and the first voxel that attains it stay in registers.
//   k_field_segments one lane per leg in a grid-stride loop, as k_los_segments: d2 / vox, and optionally the (d, idx) a clearance
//                    edge query gives for need2.
//   k_field_nodes    one lane per brick word: the voxels inside dims with field >= need2, every index = stride / 2 modulo stride and,
//                    with a map's two planes, state 1; one word of an occupancy grid's layout out.
//
// No float atomics (no atomics at all), no process-wide state; every argument check returns before anything is enqueued.
namespace {

constexpr int kFieldSentinel = 65535;
constexpr int kFieldMaxD = 254;

inline size_t field_voxels(int64_t nx, int64_t ny, int64_t nz) { return (size_t)nx * (size_t)ny * (size_t)nz; }
inline size_t field_voxels(const OccGeom& g) { return field_voxels(g.nx, g.ny, g.nz); }
inline bool field_fits(size_t bytes, const OccGeom& g) { return bytes >= field_voxels(g) * sizeof(uint16_t); }

// the geometry (occ_check's rules) and the field buffer's size
inline int field_check(const void* field, size_t bytes, const tohip_occ_geom* geom, OccGeom& g) {
    const int rc = occ_check(field, ~(size_t)0, geom, g);
    if (rc != TOHIP_OK) return rc;
    return field_fits(bytes, g) ? TOHIP_OK : TOHIP_ENOSPC;
}

__device__ __forceinline__ long long field_index(const OccGeom& g, int x, int y, int z) { return ((long long)z * g.ny + y) * g.nx + x; }

// the obstacle bits of the x row (y, z) in brick bx (inside the brick array): bit i = voxel 4 bx + i
__device__ __forceinline__ unsigned field_row_nibble(const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, const OccGeom& g, int bx,
                                                     int y, int z) {
    const int w = ((z >> 1) * g.nby + (y >> 2)) * g.nbx + bx;
    unsigned bits = occ[w];
    if (fre) bits |= ~fre[w];
    bits &= occ_brick_mask(g, bx, y >> 2, z >> 1);
    return (bits >> (((y & 3) << 2) | ((z & 1) << 4))) & 0xFu;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_field_x(const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, OccGeom g, int D, long long n_vox, uint16_t* __restrict__ out) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n_vox; i += stride) {
        const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / ((long long)g.nx * g.ny));
        const int bx = x >> 2;
        int best = D + 2;   // the nearest obstacle's |x - x'|; D + 2: none within the window
        bool left = true, right = true;
        for (int b = 0; ; ++b) {
            // (the nearest voxel of the bricks bx -+ b is max(4 b - 3, 0) away)
            if (b > 0 && 4 * b - 3 >= best) break;
            if (left && bx - b >= 0) {
                unsigned m = field_row_nibble(occ, fre, g, bx - b, y, z);
                if (b == 0) m &= (2u << (x & 3)) - 1u;
                if (m) { best = min(best, x - (4 * (bx - b) + (31 - __clz((int)m)))); left = false; }
            }
            if (right && bx + b < g.nbx) {
                unsigned m = field_row_nibble(occ, fre, g, bx + b, y, z);
                if (b == 0) m &= 0xFu << (x & 3);
                if (m) { best = min(best, 4 * (bx + b) + (__ffs((int)m) - 1) - x); right = false; }
            }
            if (!(left && bx - b > 0) && !(right && bx + b + 1 < g.nbx)) break;
        }
        const int gap = max(best - 1, 0);
        out[i] = (uint16_t)(gap <= D ? gap * gap : kFieldSentinel);
    }
}

// out[v] = min over |k| <= D + 1 with v + k e_axis inside dims of in[v + k e_axis] + max(|k| - 1, 0)^2 where <= D^2, else the sentinel.
// step: the pass axis's stride in voxels (nx for y, nx ny for z); n: its extent.
__global__ void __launch_bounds__(TO_BLOCK)
k_field_axis(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, OccGeom g, int axis, int D, long long n_vox) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    const long long step = axis == 1 ? (long long)g.nx : (long long)g.nx * g.ny;
    const int n = axis == 1 ? g.ny : g.nz;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n_vox; i += stride) {
        const int p = axis == 1 ? (int)((i / g.nx) % g.ny) : (int)(i / ((long long)g.nx * g.ny));
        int best = in[i];
        for (int k = 1; k <= D + 1; ++k) {
            const int c = (k - 1) * (k - 1);
            if (c >= best) break;   // (nothing further out can be smaller)
            if (p - k >= 0) best = min(best, (int)in[i - k * step] + c);
            if (p + k < n) best = min(best, (int)in[i + k * step] + c);
        }
        out[i] = (uint16_t)(best <= D * D ? best : kFieldSentinel);
    }
}

// metres of a query's d2: fl(fl(sqrt(d2)) r); +inf for the sentinel, NaN for -1
__device__ __forceinline__ float field_metres(int d2, float r) {
    if (d2 < 0) return __builtin_nanf("");
    if (d2 == kFieldSentinel) return __builtin_inff();
    return __fmul_rn(sqrtf((float)d2), r);   // (sqrtf: correctly rounded; __fsqrt_rn is the native, approximate one here)
}

__global__ void __launch_bounds__(TO_BLOCK)
k_field_positions(const uint16_t* __restrict__ field, OccGeom g, const float* __restrict__ pos, long long m, int* __restrict__ d2_out,
                  float* __restrict__ dist_out) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < m; i += stride) {
        int x, y, z, d2 = -1;
        const OccPlace at = occ_locate(g, pos + 3 * i, x, y, z);
        if (at != kOccOutOfRange) d2 = at == kOccInside ? (int)field[field_index(g, x, y, z)] : kFieldSentinel;
        if (d2_out) d2_out[i] = d2;
        if (dist_out) dist_out[i] = field_metres(d2, g.r);
    }
}

// the voxel the walk stands on joins the running minimum: a strict < keeps the first voxel, in walk order, that attains it.  A visitor
// that never stops the walk.
__device__ __forceinline__ bool edt_visit(const uint16_t* __restrict__ field, const OccGeom& g, const OccWalk& k, int& best, int& arg) {
    if (!occ_inside(g, k.X.v, k.Y.v, k.Z.v)) return false;
    const long long at = field_index(g, k.X.v, k.Y.v, k.Z.v);
    const int v = field[at];
    if (v < best) { best = v; arg = (int)at; }
    return false;
}

// A -> B in fixed point (both in range): the minimum of the field over v0 ... v_T inside dims and where it is first attained
// (65535, -1: no visited voxel inside dims holds a value)
__device__ __forceinline__ void edt_walk(const uint16_t* __restrict__ field, const OccGeom& g, int ax, int ay, int az, int bx, int by, int bz,
                                         int& best, int& arg) {
    OccWalk k = occ_walk_begin(ax, ay, az, bx, by, bz);
    best = kFieldSentinel;
    arg = -1;
    occ_walk(k, 0, [&](const OccWalk& at) { return edt_visit(field, g, at, best, arg); });
    edt_visit(field, g, k, best, arg);
}

// d2 / vox (either may be null) and, with edge_d and edge_idx, the answer in a clearance edge query's shape for need2: an open leg
// (d2 >= need2) +inf / -1, a blocked one metres / vox, a leg with an endpoint out of range 0 / -2.
__global__ void __launch_bounds__(TO_BLOCK)
k_field_segments(const uint16_t* __restrict__ field, OccGeom g, const float* __restrict__ a, const float* __restrict__ b, long long n_legs,
                 int* __restrict__ d2_out, int* __restrict__ vox_out, int need2, float* __restrict__ edge_d, int* __restrict__ edge_idx) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n_legs; i += stride) {
        int ax, ay, az, bx, by, bz;
        const bool ok = occ_fixed_leg(g, a + 3 * i, b + 3 * i, ax, ay, az, bx, by, bz);
        int d2 = -1, vox = -1;
        if (ok) edt_walk(field, g, ax, ay, az, bx, by, bz, d2, vox);
        if (d2_out) d2_out[i] = d2;
        if (vox_out) vox_out[i] = vox;
        if (edge_d) {
            const bool open = d2 >= need2;
            edge_d[i] = d2 < 0 ? 0.f : (open ? __builtin_inff() : field_metres(d2, g.r));
            edge_idx[i] = d2 < 0 ? -2 : (open ? -1 : vox);
        }
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_field_nodes(const uint16_t* __restrict__ field, const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, unsigned* __restrict__ out,
              OccGeom g, long long n_words, int need2, int stride) {
    const long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    if (w >= n_words) return;
    int bx, by, bz;
    occ_brick(g, w, bx, by, bz);
    unsigned cand = occ_brick_mask(g, bx, by, bz);
    if (occ) cand &= fre[w] & ~occ[w];   // state 1
    const int phase = stride >> 1;
    unsigned word = 0u;
    while (cand != 0u) {
        const int bit = __ffs(cand) - 1;
        cand &= cand - 1u;
        int x, y, z;
        occ_voxel(bx, by, bz, bit, x, y, z);
        if (x % stride != phase || y % stride != phase || z % stride != phase) continue;
        if ((int)field[field_index(g, x, y, z)] >= need2) word |= 1u << bit;
    }
    out[w] = word;
}

}  // namespace

extern "C" size_t tohip_field_bytes(int32_t nx, int32_t ny, int32_t nz) {
    return occ_dims_ok(nx, ny, nz) ? field_voxels(nx, ny, nz) * sizeof(uint16_t) : 0;
}

extern "C" size_t tohip_field_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) { return tohip_field_bytes(nx, ny, nz); }

extern "C" int tohip_field_build(const void* occupied, const void* free_or_null, size_t grid_bytes, const tohip_occ_geom* geom, int32_t D,
                                 void* field, size_t field_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    OccGeom g;
    int rc = occ_check(occupied, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!field || !workspace || field == workspace || D < 1 || D > kFieldMaxD) return TOHIP_EINVAL;
    if (field == occupied || workspace == occupied || (free_or_null && (free_or_null == occupied || free_or_null == field || free_or_null == workspace)))
        return TOHIP_EINVAL;
    if (!field_fits(field_bytes, g) || !field_fits(workspace_bytes, g)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const long long n = (long long)field_voxels(g);
    const int blocks = occ_grid_blocks(n);
    uint16_t* f = (uint16_t*)field;
    uint16_t* w = (uint16_t*)workspace;
    k_field_x<<<blocks, TO_BLOCK, 0, st>>>(occ_data(occupied), free_or_null ? occ_data(free_or_null) : nullptr, g, D, n, f);
    TO_HIP_CHECK_LAUNCH();
    k_field_axis<<<blocks, TO_BLOCK, 0, st>>>(f, w, g, 1, D, n);
    TO_HIP_CHECK_LAUNCH();
    k_field_axis<<<blocks, TO_BLOCK, 0, st>>>(w, f, g, 2, D, n);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_field_positions(const void* field, size_t field_bytes, const tohip_occ_geom* geom, const float* positions, int64_t m,
                                     int32_t* d2, float* dist, void* stream_) {
    OccGeom g;
    const int rc = field_check(field, field_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occ_count_ok(m) || (m > 0 && (!positions || (!d2 && !dist)))) return TOHIP_EINVAL;
    if (m == 0) return TOHIP_OK;
    k_field_positions<<<occ_grid_blocks(m), TO_BLOCK, 0, (hipStream_t)stream_>>>((const uint16_t*)field, g, positions, m, d2, dist);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_field_segments(const void* field, size_t field_bytes, const tohip_occ_geom* geom, const float* a, const float* b,
                                    int64_t n_legs, int32_t* d2, int32_t* vox, int32_t need2, float* edge_d, int32_t* edge_idx, void* stream_) {
    OccGeom g;
    const int rc = field_check(field, field_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occ_count_ok(n_legs) || (n_legs > 0 && (!a || !b))) return TOHIP_EINVAL;
    if ((edge_d == nullptr) != (edge_idx == nullptr) || (edge_d && (need2 < 0 || need2 > kFieldSentinel))) return TOHIP_EINVAL;
    if (n_legs > 0 && !edge_d && (!d2 || !vox)) return TOHIP_EINVAL;
    if (n_legs == 0) return TOHIP_OK;
    k_field_segments<<<occ_grid_blocks(n_legs), TO_BLOCK, 0, (hipStream_t)stream_>>>((const uint16_t*)field, g, a, b, n_legs, d2, vox, need2,
                                                                                    edge_d, edge_idx);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_field_nodes(const void* field, size_t field_bytes, const void* occupied_or_null, const void* free_or_null, void* nodes,
                                 size_t grid_bytes, const tohip_occ_geom* geom, int32_t need2, int32_t stride, void* stream_) {
    OccGeom g;
    int rc = occ_check(nodes, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!field || (occupied_or_null == nullptr) != (free_or_null == nullptr) || nodes == occupied_or_null || nodes == free_or_null ||
        nodes == field || need2 < 0 || need2 > kFieldSentinel || stride < 1 || stride > kOccMaxDim)
        return TOHIP_EINVAL;
    if (!field_fits(field_bytes, g)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const OccMaskLaunch m = occ_mask_begin(nodes, g, st);
    if (m.rc != TOHIP_OK) return m.rc;
    k_field_nodes<<<m.blocks, TO_BLOCK, 0, st>>>((const uint16_t*)field, occupied_or_null ? occ_data(occupied_or_null) : nullptr,
                                                 free_or_null ? occ_data(free_or_null) : nullptr, occ_data(nodes), g, m.n_words, need2, stride);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
