// ground_kernels.hip — the ground layer of a map ("Ground layer"), for gfx950: where a robot of height H voxels that
// climbs steps of s voxels can stand, what is an obstacle FOR IT, and the slab of air its centre rides in.  Included after
// components_kernels.hip: the geometry, the brick layout and occ_brick_mask are occupancy_kernels.hip's and frontier_kernels.hip's.
//
// A voxel is CLEAR iff it is not occupied and — with unknown = obstacle — known free; a voxel outside dims is clear under unknown =
// free and not clear under obstacle.  In a brick word the level above or below is a 16-bit shift (bit = x&3 | (y&3)<<2 | (z&1)<<4),
// the next brick up one word stride away; a LEVEL below is 16 bits: the 4 x 4 columns of one brick column at one z.
//
//   k_ground_support   support = occupied and the H voxels above clear.  One lane per word: the AND of the clear levels z + 1 .. z + H
//                      for the word's two levels, from at most ceil(H / 2) + 1 words upwards; it ends as soon as both are empty.
//   k_ground_rim       ground = the support voxels all eight of whose lateral neighbour columns are FINE: inside dims and holding
//                      (a) a support voxel at a level in [z - s, z + s] or (b) an occupied voxel at a level in [z + 1, z + H] (a
//                      wall or a box: it is its own obstacle).  One lane per word; a word without support is done at once.  Per
//                      level the fine columns of the 3 x 3 brick columns around the word are 16-bit masks — the OR of the levels
//                      named — and the eight neighbours are those masks moved by one column: across x inside a row of bricks,
//                      then across y, as the frontier kernel moves its masks.
//   k_ground_planes    floor = the occupied voxels whose occupied run upwards ends in a ground voxel; obstacles = occupied and not
//                      floor (with unknown = obstacle: and every unknown voxel); drive = the non-occupied voxels with ground 1 ..
//                      s + 1 levels below.  One lane per word: the run is followed upwards word by word while a column of the word
//                      is still undecided — ground is final, it was a launch of its own, which is why the rim is not fused into this
//                      kernel: a lane would have to derive the ground of every word above it again.
//   k_ground_snap      (M,3) positions -> the standing voxel at or below each: from the position's voxel down, at most max_drop
//                      voxels, the first drive voxel whose voxel below is ground; its centre fl(origin + fl(fl(i + 0.5) r)) — the
//                      rule of tohip_travel_paths — and the drop in voxels, -1 none, -2 out of range or outside dims (NaN rows).
//
// Integers only, no atomics (every output word has one writer), 64-bit word indices, grid-stride; the outputs' headers and pad bits
// are 0; nothing is read back; every argument check returns before anything is enqueued.
namespace {

constexpr int kGroundMaxHeadroom = 64;
constexpr int kGroundMaxStep = 4;
constexpr int kGroundMaxDrop = 2048;
constexpr int kGroundBlocks = 512;   // blocks of a plane kernel: two per CU; larger planes take more than one grid-stride pass

inline int ground_blocks(long long n_words) {
    const long long b = (n_words + TO_BLOCK - 1) / TO_BLOCK;
    return (int)(b < 1 ? 1 : (b > kGroundBlocks ? kGroundBlocks : b));
}

struct GroundArgs {
    OccGeom g;
    int nbz, H, s, known;   // known: unknown = obstacle (fre is then a plane)
    long long n_words;
};

// the 16 columns of brick column (bx, by) that lie inside dims
__device__ __forceinline__ unsigned ground_columns(const OccGeom& g, int bx, int by) { return occ_brick_mask(g, bx, by, 0) & 0xFFFFu; }

// the OR of the levels za .. zb (clipped to dims) of the brick column whose word at bz = 0 is `col`; sz: the word stride of bz
__device__ __forceinline__ unsigned ground_or_levels(const unsigned* __restrict__ words, long long col, long long sz, int nz, int za, int zb) {
    za = max(za, 0), zb = min(zb, nz - 1);
    unsigned acc = 0u;
    for (int wz = za >> 1; wz <= (zb >> 1); ++wz) {
        const unsigned v = words[col + wz * sz];
        if (2 * wz >= za) acc |= v;
        if (2 * wz + 1 <= zb) acc |= v >> 16;
    }
    return acc & 0xFFFFu;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_ground_support(const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, unsigned* __restrict__ support, GroundArgs a) {
    const long long stride = (long long)gridDim.x * TO_BLOCK, sz = (long long)a.g.nbx * a.g.nby;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < a.n_words; w += stride) {
        int bx, by, bz;
        occ_brick(a.g, w, bx, by, bz);
        const unsigned o = occ[w] & occ_brick_mask(a.g, bx, by, bz);
        unsigned out = 0u;
        if (o != 0u) {
            // lo / hi: the columns whose levels z0 + 1 .. z0 + H / z0 + 2 .. z0 + 1 + H have all been clear so far
            unsigned lo = o & 0xFFFFu, hi = o >> 16;
            const int z0 = 2 * bz;
            unsigned word = 0u;
            for (int k = 1; k <= a.H + 1 && (lo | hi) != 0u; ++k) {
                const int z = z0 + k;
                unsigned clear;
                if (z >= a.g.nz) {
                    clear = a.known ? 0u : 0xFFFFu;
                } else {
                    if ((z & 1) == 0 || k == 1) {   // (a new word; k = 1 is this word's upper level)
                        const long long u = w + (long long)((z >> 1) - bz) * sz;
                        word = ~occ[u];
                        if (a.known) word &= fre[u];
                    }
                    clear = (z & 1) ? word >> 16 : word & 0xFFFFu;
                }
                if (k <= a.H) lo &= clear;
                if (k >= 2) hi &= clear;
            }
            out = lo | (hi << 16);
        }
        support[w] = out;
    }
}

// a 3 x 3 block of 16-bit column masks m[dy + 1][dx + 1] around a brick column -> the AND over the eight lateral neighbours of each
// of its 16 columns (a brick column beyond the array holds 0: nothing outside dims is fine)
__device__ __forceinline__ unsigned ground_all_neighbours(const unsigned m[3][3]) {
    unsigned xm[3], xp[3];   // per row of bricks: the column at x - 1 / x + 1
    for (int r = 0; r < 3; ++r) {
        xm[r] = ((m[r][1] << 1) & 0xEEEEu) | ((m[r][0] & 0x8888u) >> 3);
        xp[r] = ((m[r][1] >> 1) & 0x7777u) | ((m[r][2] & 0x1111u) << 3);
    }
    const unsigned mid[3] = {m[0][1], m[1][1], m[2][1]};
    // across y: the column at y - 1 and the one at y + 1 of a mask and its two neighbouring rows of bricks
    auto both_y = [](const unsigned* v) {
        return (((v[1] << 4) & 0xFFF0u) | ((v[0] & 0xF000u) >> 12)) & (((v[1] >> 4) & 0x0FFFu) | ((v[2] & 0x000Fu) << 12));
    };
    const unsigned all = xm[1] & xp[1] & both_y(xm) & both_y(mid) & both_y(xp);
    return all;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_ground_rim(const unsigned* __restrict__ occ, const unsigned* __restrict__ support, unsigned* __restrict__ ground, GroundArgs a) {
    const long long stride = (long long)gridDim.x * TO_BLOCK, sz = (long long)a.g.nbx * a.g.nby;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < a.n_words; w += stride) {
        const unsigned sup = support[w];
        unsigned out = 0u;
        if (sup != 0u) {
            int bx, by, bz;
            occ_brick(a.g, w, bx, by, bz);
            for (int half = 0; half < 2; ++half) {
                const unsigned mine = half ? sup >> 16 : sup & 0xFFFFu;
                if (mine == 0u) continue;
                const int z = 2 * bz + half;
                unsigned fine[3][3];
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int cx = bx + dx, cy = by + dy;
                        unsigned f = 0u;
                        if ((unsigned)cx < (unsigned)a.g.nbx && (unsigned)cy < (unsigned)a.g.nby) {
                            const long long col = (long long)cy * a.g.nbx + cx;
                            f = (ground_or_levels(support, col, sz, a.g.nz, z - a.s, z + a.s) |
                                 ground_or_levels(occ, col, sz, a.g.nz, z + 1, z + a.H)) & ground_columns(a.g, cx, cy);
                        }
                        fine[dy + 1][dx + 1] = f;
                    }
                out |= (mine & ground_all_neighbours(fine)) << (16 * half);
            }
        }
        ground[w] = out;
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_ground_planes(const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, const unsigned* __restrict__ ground,
                unsigned* __restrict__ obstacles, unsigned* __restrict__ drive, GroundArgs a) {
    const long long stride = (long long)gridDim.x * TO_BLOCK, sz = (long long)a.g.nbx * a.g.nby;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < a.n_words; w += stride) {
        int bx, by, bz;
        occ_brick(a.g, w, bx, by, bz);
        const unsigned in = occ_brick_mask(a.g, bx, by, bz), o = occ[w] & in, gr = ground[w];
        // floor: a column of the upper level that is occupied and not ground is decided by the run above it
        unsigned floor_hi = (o >> 16) & (gr >> 16);
        unsigned pending = (o >> 16) & ~(gr >> 16);
        for (int uz = bz + 1; pending != 0u && uz < a.nbz; ++uz) {
            const long long u = w + (long long)(uz - bz) * sz;
            const unsigned ou = occ[u] & occ_brick_mask(a.g, bx, by, uz), gu = ground[u];
            floor_hi |= pending & gu;                 // the run ends in a ground voxel of the lower level
            pending &= ou & ~gu;                      // ... or goes on through an occupied one
            floor_hi |= pending & (gu >> 16);
            pending &= (ou >> 16) & ~(gu >> 16);
        }
        const unsigned floor_lo = o & 0xFFFFu & (gr | floor_hi);
        unsigned obst = o & ~(floor_lo | (floor_hi << 16));
        if (a.known) obst |= ~occ[w] & ~fre[w] & in;
        obstacles[w] = obst;
        // drive: ground at z - 1 .. z - s - 1
        const long long col = (long long)by * a.g.nbx + bx;
        const int z0 = 2 * bz;
        const unsigned under_lo = ground_or_levels(ground, col, sz, a.g.nz, z0 - 1 - a.s, z0 - 1);
        const unsigned under_hi = ground_or_levels(ground, col, sz, a.g.nz, z0 - a.s, z0);
        drive[w] = (under_lo | (under_hi << 16)) & ~o & in;
    }
}

__device__ __forceinline__ bool ground_bit(const unsigned* __restrict__ words, const OccGeom& g, int x, int y, int z) {
    return (words[occ_word(g, x, y, z)] >> occ_bit(x, y, z)) & 1u;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_ground_snap(const unsigned* __restrict__ ground, const unsigned* __restrict__ drive, OccGeom g, const float* __restrict__ pos, long long m,
              int max_drop, float* __restrict__ standing, int* __restrict__ drop) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < m; i += stride) {
        int x, y, z, k = -2;
        if (occ_locate(g, pos + 3 * i, x, y, z) == kOccInside) {
            k = -1;
            for (int d = 0; d <= max_drop && z - d >= 1; ++d)
                if (ground_bit(drive, g, x, y, z - d) && ground_bit(ground, g, x, y, z - d - 1)) {
                    k = d;
                    break;
                }
        }
        const float nan = __int_as_float(0x7fc00000);
        standing[3 * i] = k >= 0 ? __fadd_rn(g.ox, __fmul_rn((float)x + 0.5f, g.r)) : nan;
        standing[3 * i + 1] = k >= 0 ? __fadd_rn(g.oy, __fmul_rn((float)y + 0.5f, g.r)) : nan;
        standing[3 * i + 2] = k >= 0 ? __fadd_rn(g.oz, __fmul_rn((float)(z - k) + 0.5f, g.r)) : nan;
        drop[i] = k;
    }
}

}  // namespace

extern "C" int tohip_ground_build(const void* occupied, const void* free_or_null, size_t grid_bytes, const tohip_occ_geom* geom, int32_t headroom,
                                  int32_t step, int32_t unknown_obstacle, void* support, void* ground, void* obstacles, void* drive, void* stream_,
                                  uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = occ_check(occupied, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (headroom < 1 || headroom > kGroundMaxHeadroom || step < 0 || step > kGroundMaxStep || step + 1 > headroom ||
        (unknown_obstacle != 0 && unknown_obstacle != 1) || (unknown_obstacle == 1 && !free_or_null) || !support || !ground || !obstacles || !drive)
        return TOHIP_EINVAL;
    const void* planes[6] = {occupied, free_or_null, support, ground, obstacles, drive};
    for (int i = 0; i < 6; ++i) {
        if (!comp_aligned(planes[i], 4)) return TOHIP_EINVAL;
        for (int j = 2; j < 6; ++j)   // no output is an input or another output
            if (i < j && planes[i] == planes[j]) return TOHIP_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream_;
    GroundArgs a{g, (g.nz + 1) / 2, headroom, step, unknown_obstacle, (long long)occ_words(g.nx, g.ny, g.nz)};
    void* outs[4] = {support, ground, obstacles, drive};
    for (int i = 0; i < 4; ++i) {
        const OccMaskLaunch m = occ_mask_begin(outs[i], g, st);
        if (m.rc != TOHIP_OK) return m.rc;
    }
    const unsigned* fre = unknown_obstacle ? occ_data(free_or_null) : nullptr;
    const int blocks = ground_blocks(a.n_words);
    k_ground_support<<<blocks, TO_BLOCK, 0, st>>>(occ_data(occupied), fre, occ_data(support), a);
    TO_HIP_CHECK_LAUNCH();
    k_ground_rim<<<blocks, TO_BLOCK, 0, st>>>(occ_data(occupied), occ_data(support), occ_data(ground), a);
    TO_HIP_CHECK_LAUNCH();
    k_ground_planes<<<blocks, TO_BLOCK, 0, st>>>(occ_data(occupied), fre, occ_data(ground), occ_data(obstacles), occ_data(drive), a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_ground_snap(const void* ground, const void* drive, size_t grid_bytes, const tohip_occ_geom* geom, const float* positions,
                                 int64_t m, int32_t max_drop, float* standing, int32_t* drop, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = occ_check(ground, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!drive || !comp_aligned(ground, 4) || !comp_aligned(drive, 4) || max_drop < 0 || max_drop > kGroundMaxDrop ||
        !occ_count_ok(m) || (m > 0 && (!positions || !standing || !drop)))
        return TOHIP_EINVAL;
    if (m == 0) return TOHIP_OK;
    k_ground_snap<<<occ_grid_blocks(m), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(ground), occ_data(drive), g, positions, m, max_drop, standing,
                                                                            drop);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
