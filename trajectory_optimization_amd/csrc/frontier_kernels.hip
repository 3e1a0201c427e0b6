// frontier_kernels.hip — free-space carving, the three-state map, frontier extraction and the ordered listing of a grid's set bits
// ("Free space and frontiers"), for gfx950.  Included right after occupancy_kernels.hip: the geometry, the fixed-point
// coordinates, the brick layout and the walk (occ_walk) are that file's.
//
// The FREE PLANE is a second occupancy grid of the same geometry whose set bit means "a ray passed through".  State of a voxel
// inside dims: 2 occupied (the occupied bit wins), else 1 free, else 0 unknown; 3 for a position out of range or outside dims.
//
//   k_occ_carve      one lane per ray a -> b in a grid-stride loop.  An endpoint out of range: skipped and counted.  D = B - A,
//                    L = isqrt(D.D) (a double sqrt and a +-1 fix-up: D.D < 2^43 is exact in a double); with R > 0 and L > R the ray
//                    is TRUNCATED to B' = A + sign(D) floor(|D| R / L) per axis (products < 2^42) and is not a hit.  A -> B' is
//                    walked by occ_walk with stop_at = 0, and every visited voxel inside dims gets its free bit: v_0 .. v_T-1 from
//                    the visitor, v_T behind the walk, except for a hit.  The bits of consecutive steps that fall into one brick
//                    are gathered in a register and flushed when the walk leaves the word: a plain load first, and the 32-bit atomic
//                    OR only where the word lacks one of the bits.  Bits are only ever set, so a stale cached word can only cause
//                    a redundant atomic, never a missed bit; re-carving mapped space costs loads alone.
//   k_occ_state      (M,3) f32 positions -> uint8 state.
//   k_occ_frontier   one lane per brick word: the word of both planes and of the six neighbouring bricks; free & ~occ and unknown =
//                    ~free & ~occ & (inside dims) as 32-bit masks; the six neighbour masks by shifts of 1, 4 and 16 under the edge
//                    masks plus the facing edge bits of the neighbour words; a bit-sliced count per voxel; one mask word out.
//                    Bricks beyond the array and voxels beyond dims are not unknown.
//   k_occ_popcount / k_occ_scan / k_occ_scatter   the set bits of any grid in ascending (word, bit) order — the order a kernel gives
//                    without a sort: per-block counts, an exclusive scan over the blocks in one block, then every lane writes the
//                    ijk and centres of its word's bits at the block's base plus its prefix within the block.
//
// No float atomics, no process-wide state; every argument check returns before anything is enqueued.
namespace {

constexpr long long kCarveMaxRange = 6144ll * 256;   // R, in 1/256 voxel: the span of the grid and its apron

// floor(sqrt(dd)) for 0 <= dd < 2^53
__device__ __forceinline__ long long carve_isqrt(long long dd) {
    long long L = (long long)sqrt((double)dd);
    while (L * L > dd) --L;
    while ((L + 1) * (L + 1) <= dd) ++L;
    return L;
}

// B -> B' where the ray is longer than R; true = a hit (not truncated)
__device__ __forceinline__ bool carve_clip(int ax, int ay, int az, int& bx, int& by, int& bz, long long R) {
    if (R <= 0) return true;
    const long long dx = (long long)bx - ax, dy = (long long)by - ay, dz = (long long)bz - az;
    const long long L = carve_isqrt(dx * dx + dy * dy + dz * dz);
    if (L <= R) return true;
    bx = ax + (int)(dx < 0 ? -(-dx * R / L) : dx * R / L);
    by = ay + (int)(dy < 0 ? -(-dy * R / L) : dy * R / L);
    bz = az + (int)(dz < 0 ? -(-dz * R / L) : dz * R / L);
    return false;
}

// the gathered bits of word `cur` go out: a plain load, and the atomic only where a bit is missing.  Bits are monotonic: a stale
// cached word can only cause a redundant atomic, never a missed bit.
__device__ __forceinline__ void carve_flush(unsigned* words, int cur, unsigned bits, unsigned& atomics) {
    if (cur < 0 || bits == 0u) return;
    if ((words[cur] & bits) != bits) {
        __hip_atomic_fetch_or(words + cur, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++atomics;
    }
}

// the voxel the walk stands on joins the gathered bits; leaving the word flushes it.  A visitor that never stops the walk.
__device__ __forceinline__ bool carve_mark(unsigned* words, const OccGeom& g, const OccWalk& at, int& cur, unsigned& bits, unsigned& atomics) {
    const int x = at.X.v, y = at.Y.v, z = at.Z.v;
    if (!occ_inside(g, x, y, z)) return false;
    const int w = occ_word(g, x, y, z);
    if (w != cur) { carve_flush(words, cur, bits, atomics); cur = w; bits = 0u; }
    bits |= 1u << occ_bit(x, y, z);
    return false;
}

// A -> B in fixed point (both in range): v0 ... v_T get their free bit where they lie inside dims, v_T only when !hit
__device__ __forceinline__ void carve_walk(unsigned* words, const OccGeom& g, int ax, int ay, int az, int bx, int by, int bz, bool hit,
                                           unsigned& visits, unsigned& atomics) {
    OccWalk k = occ_walk_begin(ax, ay, az, bx, by, bz);
    int cur = -1;
    unsigned bits = 0;
    visits += 1u + (unsigned)(k.X.rem + k.Y.rem + k.Z.rem);   // v0 ... v_T
    occ_walk(k, 0, [&](const OccWalk& at) { return carve_mark(words, g, at, cur, bits, atomics); });
    if (!hit) carve_mark(words, g, k, cur, bits, atomics);
    carve_flush(words, cur, bits, atomics);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_carve(unsigned long long* __restrict__ hdr, unsigned* words, OccGeom g, const float* __restrict__ origins, int origin_stride,
            const float* __restrict__ pts, long long n, long long R, uint8_t* __restrict__ flags, unsigned long long* __restrict__ stats) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    long long skipped = 0, rays = 0, visits = 0, atomics = 0;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n; i += stride) {
        const float* o = origins + (long long)origin_stride * i;
        int ax, ay, az, bx, by, bz;
        const bool ok = occ_fixed_leg(g, o, pts + 3 * i, ax, ay, az, bx, by, bz);
        int flag = 2;
        if (ok) {
            const bool hit = carve_clip(ax, ay, az, bx, by, bz, R);
            unsigned v = 0, at = 0;
            carve_walk(words, g, ax, ay, az, bx, by, bz, hit, v, at);
            flag = hit ? 0 : 1;
            ++rays;
            visits += v;
            atomics += at;
        } else {
            ++skipped;
        }
        if (flags) flags[i] = (uint8_t)flag;
    }
    occ_count(hdr, skipped);
    if (stats) { occ_count(stats, rays); occ_count(stats + 1, visits); occ_count(stats + 2, atomics); }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_state(const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, OccGeom g, const float* __restrict__ pos, long long m,
            uint8_t* __restrict__ out) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < m; i += stride) {
        int x, y, z, s = 3;
        if (occ_locate(g, pos + 3 * i, x, y, z) == kOccInside) {
            const int w = occ_word(g, x, y, z), b = occ_bit(x, y, z);
            s = ((occ[w] >> b) & 1u) ? 2 : (int)((fre[w] >> b) & 1u);
        }
        out[i] = (uint8_t)s;
    }
}

// the bits of brick (bx, by, bz) whose voxels lie inside dims (the brick itself lies inside the brick array)
__device__ __forceinline__ unsigned occ_brick_mask(const OccGeom& g, int bx, int by, int bz) {
    const int cx = min(4, g.nx - 4 * bx), cy = min(4, g.ny - 4 * by), cz = min(2, g.nz - 2 * bz);
    const unsigned row = (1u << cx) - 1u;                          // x < cx
    const unsigned plane = (row * 0x1111u) & ((1u << (4 * cy)) - 1u);   // ... and y < cy
    return cz == 2 ? plane | (plane << 16) : plane;
}

// the frontier word of one brick.  cand: free and not occupied, inside dims.  u: this brick's unknown voxels; uxm .. uzp: the
// unknown voxels of the six neighbouring bricks (0 beyond the array).  bit = x | y << 2 | z << 4.
__device__ __forceinline__ unsigned occ_frontier_word(unsigned cand, unsigned u, unsigned uxm, unsigned uxp, unsigned uym, unsigned uyp,
                                                      unsigned uzm, unsigned uzp, int min_unknown) {
    const unsigned m[6] = {
        ((u << 1) & 0xEEEEEEEEu) | ((uxm & 0x88888888u) >> 3),    // the neighbour at x - 1
        ((u >> 1) & 0x77777777u) | ((uxp & 0x11111111u) << 3),    // x + 1
        ((u << 4) & 0xFFF0FFF0u) | ((uym & 0xF000F000u) >> 12),   // y - 1
        ((u >> 4) & 0x0FFF0FFFu) | ((uyp & 0x000F000Fu) << 12),   // y + 1
        (u << 16) | (uzm >> 16),                                  // z - 1
        (u >> 16) | (uzp << 16),                                  // z + 1
    };
    unsigned c0 = 0u, c1 = 0u, c2 = 0u;   // the count of unknown neighbours per voxel, bit-sliced (at most 6)
    for (int k = 0; k < 6; ++k) {
        const unsigned k0 = c0 & m[k];
        c0 ^= m[k];
        const unsigned k1 = c1 & k0;
        c1 ^= k0;
        c2 ^= k1;
    }
    unsigned ge;
    switch (min_unknown) {
        case 1: ge = c0 | c1 | c2; break;
        case 2: ge = c1 | c2; break;
        case 3: ge = c2 | (c1 & c0); break;
        case 4: ge = c2; break;
        case 5: ge = c2 & (c0 | c1); break;
        default: ge = c2 & c1; break;
    }
    return cand & ge;
}

// the frontier word of brick word w < n_words: the two planes' words of the brick and of its six neighbours
__device__ __forceinline__ unsigned occ_frontier_at(const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, const OccGeom& g, int nbz,
                                                    long long w, int min_unknown) {
    int bx, by, bz;
    occ_brick(g, w, bx, by, bz);
    const long long sy = g.nbx, sz = (long long)g.nbx * g.nby;
    const unsigned o = occ[w], f = fre[w], in = occ_brick_mask(g, bx, by, bz);
    const unsigned cand = f & ~o & in, u = ~f & ~o & in;
    unsigned un[6];
    const long long nw[6] = {w - 1, w + 1, w - sy, w + sy, w - sz, w + sz};
    const bool has[6] = {bx > 0, bx + 1 < g.nbx, by > 0, by + 1 < g.nby, bz > 0, bz + 1 < nbz};
    const int dx[6] = {-1, 1, 0, 0, 0, 0}, dy[6] = {0, 0, -1, 1, 0, 0}, dz[6] = {0, 0, 0, 0, -1, 1};
    for (int k = 0; k < 6; ++k)
        un[k] = has[k] ? (~fre[nw[k]] & ~occ[nw[k]] & occ_brick_mask(g, bx + dx[k], by + dy[k], bz + dz[k])) : 0u;
    return occ_frontier_word(cand, u, un[0], un[1], un[2], un[3], un[4], un[5], min_unknown);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_frontier(const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, unsigned* __restrict__ out, OccGeom g, int nbz,
               long long n_words, int min_unknown) {
    const long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    if (w < n_words) out[w] = occ_frontier_at(occ, fre, g, nbz, w, min_unknown);
}

// ---- the ordered listing ---------------------------------------------------------------------------------------------------------

// the set bits of word w that lie inside dims (no insert, carve or frontier sets another; a foreign buffer might)
__device__ __forceinline__ unsigned occ_listed_bits(const unsigned* __restrict__ words, const OccGeom& g, long long w, long long n_words,
                                                    int& bx, int& by, int& bz) {
    bx = by = bz = 0;
    if (w >= n_words) return 0u;
    occ_brick(g, w, bx, by, bz);
    return words[w] & occ_brick_mask(g, bx, by, bz);
}

// inclusive sum over the block's TO_BLOCK lanes -> (this lane's inclusive prefix, the block's total); every lane calls it
__device__ __forceinline__ void occ_block_scan(int c, int* s_wave, int& incl, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v = c;
    for (int sh = 1; sh < 64; sh <<= 1) {
        const int t = __shfl_up(v, sh);
        if (lane >= sh) v += t;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int k = 0; k < TO_BLOCK / 64; ++k) {
        if (k < wave) base += s_wave[k];
        total += s_wave[k];
    }
    incl = base + v;
    __syncthreads();
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_popcount(const unsigned* __restrict__ words, OccGeom g, long long n_words, long long* __restrict__ counts) {
    __shared__ int s_wave[TO_BLOCK / 64];
    int bx, by, bz, incl, total;
    const unsigned bits = occ_listed_bits(words, g, (long long)blockIdx.x * TO_BLOCK + threadIdx.x, n_words, bx, by, bz);
    occ_block_scan(__popc(bits), s_wave, incl, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[0 .. nb) -> their exclusive prefix sums in place, counts[nb] = the total.  One block; each lane owns a run of the entries.
__global__ void __launch_bounds__(TO_BLOCK) k_occ_scan(long long* __restrict__ counts, long long nb) {
    __shared__ long long s_sum[TO_BLOCK];
    const long long run = (nb + TO_BLOCK - 1) / TO_BLOCK;
    const long long lo = min(nb, run * threadIdx.x), hi = min(nb, lo + run);
    long long s = 0;
    for (long long i = lo; i < hi; ++i) s += counts[i];
    s_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long acc = 0;
        for (int k = 0; k < TO_BLOCK; ++k) { const long long t = s_sum[k]; s_sum[k] = acc; acc += t; }
        counts[nb] = acc;
    }
    __syncthreads();
    long long acc = s_sum[threadIdx.x];
    for (long long i = lo; i < hi; ++i) { const long long t = counts[i]; counts[i] = acc; acc += t; }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_scatter(const unsigned* __restrict__ words, OccGeom g, long long n_words, const long long* __restrict__ offsets, long long capacity,
              int* __restrict__ ijk, float* __restrict__ centres) {
    __shared__ int s_wave[TO_BLOCK / 64];
    int bx, by, bz, incl, total;
    unsigned bits = occ_listed_bits(words, g, (long long)blockIdx.x * TO_BLOCK + threadIdx.x, n_words, bx, by, bz);
    const int c = __popc(bits);
    occ_block_scan(c, s_wave, incl, total);
    long long at = offsets[blockIdx.x] + (incl - c);
    while (bits != 0u) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1u;
        if (at >= capacity) return;   // (offsets of another grid: nothing is written past the outputs)
        int x, y, z;
        occ_voxel(bx, by, bz, b, x, y, z);
        ijk[3 * at] = x;
        ijk[3 * at + 1] = y;
        ijk[3 * at + 2] = z;
        centres[3 * at] = __fadd_rn(g.ox, __fmul_rn((float)x + 0.5f, g.r));
        centres[3 * at + 1] = __fadd_rn(g.oy, __fmul_rn((float)y + 0.5f, g.r));
        centres[3 * at + 2] = __fadd_rn(g.oz, __fmul_rn((float)z + 0.5f, g.r));
        ++at;
    }
}

inline int64_t occ_list_blocks(const OccGeom& g) { return ((int64_t)occ_words(g.nx, g.ny, g.nz) + TO_BLOCK - 1) / TO_BLOCK; }

// an output mask plane begins: its header is cleared (rc), and a kernel with one lane per word is sized
struct OccMaskLaunch { int rc; unsigned blocks; long long n_words; };
inline OccMaskLaunch occ_mask_begin(void* plane, const OccGeom& g, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(plane, 0, kOccHdr, st);
    return {e == hipSuccess ? TOHIP_OK : (int)e, (unsigned)occ_list_blocks(g), (long long)occ_words(g.nx, g.ny, g.nz)};
}

}  // namespace

extern "C" int tohip_occ_carve(void* free_grid, size_t grid_bytes, const tohip_occ_geom* geom, const float* origins, int64_t origin_stride,
                               const float* points, int64_t n_rays, int64_t max_range_fixed, uint8_t* flags, uint64_t* stats,
                               int64_t* skipped_host, void* stream_) {
    OccGeom g;
    const int rc = occ_check(free_grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occ_count_ok(n_rays) || (n_rays > 0 && (!origins || !points))) return TOHIP_EINVAL;
    if ((origin_stride != 0 && origin_stride != 3) || max_range_fixed < 0 || max_range_fixed > kCarveMaxRange) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(free_grid, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    if (n_rays > 0) {
        k_occ_carve<<<occ_grid_blocks(n_rays), TO_BLOCK, 0, st>>>((unsigned long long*)free_grid, occ_data(free_grid), g, origins,
                                                                  (int)origin_stride, points, n_rays, max_range_fixed, flags,
                                                                  (unsigned long long*)stats);
        TO_HIP_CHECK_LAUNCH();
    }
    return occ_read_back(skipped_host, free_grid, st);
}

extern "C" int tohip_occ_state(const void* occupied, const void* free_grid, size_t grid_bytes, const tohip_occ_geom* geom,
                               const float* positions, int64_t m, uint8_t* out, void* stream_) {
    OccGeom g;
    const int rc = occ_check(occupied, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!free_grid || !occ_count_ok(m) || (m > 0 && (!positions || !out))) return TOHIP_EINVAL;
    if (m == 0) return TOHIP_OK;
    k_occ_state<<<occ_grid_blocks(m), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(occupied), occ_data(free_grid), g, positions, m, out);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_occ_frontier(const void* occupied, const void* free_grid, void* frontier, size_t grid_bytes, const tohip_occ_geom* geom,
                                  int32_t min_unknown, void* stream_) {
    OccGeom g;
    const int rc = occ_check(frontier, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occupied || !free_grid || frontier == occupied || frontier == free_grid || min_unknown < 1 || min_unknown > 6) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    const OccMaskLaunch m = occ_mask_begin(frontier, g, st);
    if (m.rc != TOHIP_OK) return m.rc;
    k_occ_frontier<<<m.blocks, TO_BLOCK, 0, st>>>(occ_data(occupied), occ_data(free_grid), occ_data(frontier), g, (g.nz + 1) / 2, m.n_words,
                                                  min_unknown);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" size_t tohip_occ_export_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (!occ_dims_ok(nx, ny, nz)) return 0;
    return (size_t)((occ_words(nx, ny, nz) + TO_BLOCK - 1) / TO_BLOCK + 1) * sizeof(int64_t);
}

extern "C" int tohip_occ_count(const void* grid, size_t grid_bytes, const tohip_occ_geom* geom, void* workspace, size_t workspace_bytes,
                               int64_t* total_host, void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!workspace) return TOHIP_EINVAL;
    if (workspace_bytes < tohip_occ_export_workspace_bytes(g.nx, g.ny, g.nz)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const int64_t nb = occ_list_blocks(g);
    long long* counts = (long long*)workspace;
    k_occ_popcount<<<(unsigned)nb, TO_BLOCK, 0, st>>>(occ_data(grid), g, (long long)occ_words(g.nx, g.ny, g.nz), counts);
    TO_HIP_CHECK_LAUNCH();
    k_occ_scan<<<1, TO_BLOCK, 0, st>>>(counts, nb);
    TO_HIP_CHECK_LAUNCH();
    return occ_read_back(total_host, counts + nb, st);
}

extern "C" int tohip_occ_export(const void* grid, size_t grid_bytes, const tohip_occ_geom* geom, const void* workspace,
                                size_t workspace_bytes, int64_t total, int64_t capacity, int32_t* ijk, float* centres, void* stream_) {
    OccGeom g;
    const int rc = occ_check(grid, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!workspace || total < 0 || capacity < 0 || (total > 0 && (!ijk || !centres))) return TOHIP_EINVAL;
    if (workspace_bytes < tohip_occ_export_workspace_bytes(g.nx, g.ny, g.nz) || capacity < total) return TOHIP_ENOSPC;
    if (total == 0) return TOHIP_OK;
    k_occ_scatter<<<(unsigned)occ_list_blocks(g), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(grid), g, (long long)occ_words(g.nx, g.ny, g.nz),
                                                                                     (const long long*)workspace, capacity, ijk, centres);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
