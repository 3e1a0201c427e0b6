// components_kernels.hip — connected components of a bit plane ("Connected components"), for gfx950.  Included after
// travel_kernels.hip: the geometry, the brick layout and field_index are occupancy_kernels.hip's, frontier_kernels.hip's and
// field_kernels.hip's; the tile worklist (travel_tiles, the two bitmaps, k_travel_compact, the header words) is travel_kernels.hip's.
//
// Two set voxels inside dims are ADJACENT iff they differ by at most 1 on every axis and by 1 (c = 6), <= 2 (c = 18) or <= 3 (c = 26)
// axes; there is no corner-cut rule.  label (uint32, one word per voxel inside dims, x fastest, v = (z ny + y) nx + x): after the
// rounds every set voxel holds its component's ROOT, the lowest linear index of the component, every clear voxel 0xFFFFFFFF — the
// unique fixed point of label[v] = min(v, label[u] over the adjacent u), whatever the order of the relaxation; then the roots are
// listed in ascending order and every set voxel's label becomes its root's rank, the component's ID 0 .. C - 1.
//
//   k_components_init        one lane per brick word: label[v] = v for the word's set bits, the sentinel for its other voxels inside
//                            dims, and the bit of the word's 8 x 8 x 8 tile in bitmap 0 where the word has a set bit.
//   k_travel_compact         (travel_kernels.hip) the round's bitmap -> the tile list.
//   k_components_relax<c>    one block per listed tile, two voxels per lane.  The tile and a one-voxel halo of labels (10^3 words)
//                            go to LDS — a clear voxel and a voxel outside dims hold the sentinel, so the labels carry the set /
//                            clear state too; each voxel's mask of adjacent set voxels is derived once (a voxel with none never
//                            sweeps); the block sweeps label[v] = min(label[v], label[u]) in LDS until __syncthreads_or reports no
//                            change.  A word has one writer, values only fall and every value ever stored is the index of a voxel
//                            of the same component, so a read that races with a write sees an upper bound of the root either way.
//                            Only the tile's own voxels that fell are written back; a neighbouring tile that c can reach gets its
//                            bit in the NEXT round's bitmap iff the block lowered a voxel of the layer that touches it.
//   k_components_roots<w>    the roots (label[v] == v) in ascending order: a block owns 4096 consecutive voxels, a lane 16 of them;
//                            w = 0 counts per block, k_occ_scan (frontier_kernels.hip) scans the counts, w = 1 writes roots[] at
//                            the block's base plus the lane's prefix — nothing at or beyond the capacity.
//   k_components_relabel     label[v] <- the rank of label[v] in roots (a binary search: the workspace stays proportional to C).
//   k_components_stats       one pass over the ids: size, sums of i, j, k (64-bit integer adds), the box (32-bit integer min / max).
//                            Where all set voxels of a wave's 64 share one id the wave reduces first and keeps the sum while the id
//                            stays; ended runs gather in a 16-slot table in LDS that goes to memory once per block; otherwise each
//                            lane issues its own atomics.
//   k_components_min_value / _min_voxel   per component the smallest word of a value volume that is not the sentinel (an atomic min
//                            behind a plain pre-check: the minimum only falls, so a stale read can only cause a redundant atomic),
//                            then the lowest linear index that attains it.
//   k_components_positions   (M,3) f32 positions -> int64 id, -1 clear, -2 out of range or outside dims.
//
// Every kernel ends on its own: no block waits for another, nothing is handed from block to block inside a launch.  Integer atomics
// only, no process-wide state; every argument check returns before anything is enqueued.
namespace {

constexpr unsigned kCompSentinel = 0xFFFFFFFFu;
constexpr int kCompMaxRoundsPerCheck = 1000;
constexpr int kCompRootRun = 16;                          // consecutive voxels of a lane of k_components_roots
constexpr long long kCompRootChunk = (long long)TO_BLOCK * kCompRootRun;   // ... of a block

// moves are numbered as the travel field numbers them: m = (dz + 1) 9 + (dy + 1) 3 + (dx + 1), 13 the voxel itself
__device__ __forceinline__ constexpr int comp_axes(int m) { return (travel_dx(m) != 0) + (travel_dy(m) != 0) + (travel_dz(m) != 0); }
template <int C> __device__ __forceinline__ constexpr bool comp_adjacent(int m) {
    return m != 13 && comp_axes(m) <= (C == 6 ? 1 : (C == 18 ? 2 : 3));
}
template <int C> __device__ __forceinline__ constexpr unsigned comp_mask() {
    unsigned mask = 0u;
    for (int m = 0; m < 27; ++m)
        if (comp_adjacent<C>(m)) mask |= 1u << m;
    return mask;
}

inline long long comp_root_blocks(long long n_vox) { return (n_vox + kCompRootChunk - 1) / kCompRootChunk; }

__global__ void __launch_bounds__(TO_BLOCK)
k_components_init(const unsigned* __restrict__ words, OccGeom g, long long n_words, unsigned* __restrict__ label, unsigned* __restrict__ bitmap,
                  long long ntx, long long nty) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < n_words; w += stride) {
        int bx, by, bz;
        occ_brick(g, w, bx, by, bz);
        const unsigned in = occ_brick_mask(g, bx, by, bz), bits = words[w] & in;
#pragma unroll
        for (int row = 0; row < 8; ++row) {   // a row of the brick: four voxels along x
            if (!((in >> (4 * row)) & 1u)) continue;   // (x = 4 bx lies inside dims wherever the row does)
            const int y = 4 * by + (row & 3), z = 2 * bz + (row >> 2);
            const long long v0 = field_index(g, 4 * bx, y, z);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if ((in >> (4 * row + i)) & 1u) label[v0 + i] = ((bits >> (4 * row + i)) & 1u) ? (unsigned)(v0 + i) : kCompSentinel;
        }
        if (bits != 0u) {
            const long long t = ((long long)(bz >> 2) * nty + (by >> 1)) * ntx + (bx >> 1);
            __hip_atomic_fetch_or(bitmap + (t >> 5), 1u << (t & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int C>
__global__ void __launch_bounds__(TO_BLOCK)
k_components_relax(OccGeom g, unsigned* label, const int* __restrict__ list, unsigned* __restrict__ hdr32, int parity, unsigned* __restrict__ next,
                   int ntx, int nty, int ntz) {
    __shared__ unsigned s_lab[kTravelHaloN];
    __shared__ unsigned s_touch;
    const unsigned count = hdr32[2 + parity];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the bookkeeping of the round, as the travel field keeps it: the other round's count starts from zero, and the status word
        hdr32[2 + (parity ^ 1)] = 0u;
        const unsigned rounds = hdr32[4] + (count != 0u ? 1u : 0u);
        hdr32[4] = rounds;
        hdr32[0] = count;
        hdr32[1] = rounds;
    }
    constexpr unsigned kAdj = comp_mask<C>();
    for (unsigned item = blockIdx.x; item < count; item += gridDim.x) {
        const int t = list[item];
        const int tx = t % ntx, ty = (t / ntx) % nty, tz = t / (ntx * nty);
        const int x0 = tx * kTravelTile - 1, y0 = ty * kTravelTile - 1, z0 = tz * kTravelTile - 1;   // the halo's corner
        if (threadIdx.x == 0) s_touch = 0u;
        for (int i = threadIdx.x; i < kTravelHaloN; i += TO_BLOCK) {
            const int x = x0 + i % kTravelHalo, y = y0 + (i / kTravelHalo) % kTravelHalo, z = z0 + i / (kTravelHalo * kTravelHalo);
            s_lab[i] = occ_inside(g, x, y, z) ? label[field_index(g, x, y, z)] : kCompSentinel;
        }
        __syncthreads();
        int at[2];
        unsigned first[2], mine[2];
        bool sweeps[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int l = threadIdx.x + k * TO_BLOCK;
            at[k] = (((l >> 6) + 1) * kTravelHalo + ((l >> 3) & 7) + 1) * kTravelHalo + (l & 7) + 1;
            first[k] = mine[k] = s_lab[at[k]];
            unsigned around = 0u;   // the adjacent set voxels, from the 27 surrounding states
#pragma unroll
            for (int m = 0; m < 27; ++m)
                if ((kAdj >> m) & 1u)
                    around |= (s_lab[at[k] + (travel_dz(m) * kTravelHalo + travel_dy(m)) * kTravelHalo + travel_dx(m)] != kCompSentinel ? 1u : 0u) << m;
            sweeps[k] = mine[k] != kCompSentinel && around != 0u;
        }
        bool changed;
        do {
            changed = false;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!sweeps[k]) continue;
                unsigned best = mine[k];
#pragma unroll
                for (int m = 0; m < 27; ++m)
                    if ((kAdj >> m) & 1u)   // (a clear neighbour holds the sentinel: it never wins)
                        best = min(best, s_lab[at[k] + (travel_dz(m) * kTravelHalo + travel_dy(m)) * kTravelHalo + travel_dx(m)]);
                if (best < mine[k]) {
                    mine[k] = best;
                    s_lab[at[k]] = best;
                    changed = true;
                }
            }
        } while (__syncthreads_or(changed));
        // what fell goes back, and names the neighbouring tiles that c can reach from it
        unsigned touch = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (mine[k] >= first[k]) continue;
            const int l = threadIdx.x + k * TO_BLOCK;
            const int lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
            label[field_index(g, x0 + 1 + lx, y0 + 1 + ly, z0 + 1 + lz)] = mine[k];   // (a set voxel: inside dims)
            const int ax = lx == 0 ? -1 : (lx == 7 ? 1 : 0), ay = ly == 0 ? -1 : (ly == 7 ? 1 : 0), az = lz == 0 ? -1 : (lz == 7 ? 1 : 0);
#pragma unroll
            for (int i = 1; i < 8; ++i) {
                const int ex = (i & 1) ? ax : 0, ey = (i & 2) ? ay : 0, ez = (i & 4) ? az : 0;
                if (((i & 1) && ax == 0) || ((i & 2) && ay == 0) || ((i & 4) && az == 0)) continue;
                touch |= 1u << ((ez + 1) * 9 + (ey + 1) * 3 + (ex + 1));
            }
        }
        touch &= kAdj;   // a tile across an edge or a corner holds no voxel adjacent to this one under a smaller c
        for (int sh = 32; sh > 0; sh >>= 1) touch |= __shfl_xor(touch, sh);
        if ((threadIdx.x & 63) == 0 && touch != 0u) atomicOr(&s_touch, touch);
        __syncthreads();
        if (threadIdx.x < 27 && threadIdx.x != 13 && ((s_touch >> threadIdx.x) & 1u)) {
            const int ux = tx + travel_dx(threadIdx.x), uy = ty + travel_dy(threadIdx.x), uz = tz + travel_dz(threadIdx.x);
            if ((unsigned)ux < (unsigned)ntx && (unsigned)uy < (unsigned)nty && (unsigned)uz < (unsigned)ntz) {
                const int u = (uz * nty + uy) * ntx + ux;
                __hip_atomic_fetch_or(next + (u >> 5), 1u << (u & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();   // (s_touch and the halo block are the next item's)
    }
}

// WRITE = 0: counts[block] = the roots among the block's voxels; WRITE = 1: they go to roots[offsets[block] ...) in ascending order
template <int WRITE>
__global__ void __launch_bounds__(TO_BLOCK)
k_components_roots(const unsigned* __restrict__ label, long long n_vox, long long* __restrict__ counts, long long capacity, int* __restrict__ roots) {
    __shared__ int s_wave[TO_BLOCK / 64];
    const long long lo = (long long)blockIdx.x * kCompRootChunk + (long long)threadIdx.x * kCompRootRun;
    unsigned is_root = 0u;
#pragma unroll
    for (int i = 0; i < kCompRootRun; ++i)
        if (lo + i < n_vox && label[lo + i] == (unsigned)(lo + i)) is_root |= 1u << i;
    const int c = __popc(is_root);
    int incl, total;
    occ_block_scan(c, s_wave, incl, total);
    if (WRITE == 0) {
        if (threadIdx.x == 0) counts[blockIdx.x] = total;
    } else {
        long long at = counts[blockIdx.x] + (incl - c);
        while (is_root != 0u) {
            const int i = __ffs(is_root) - 1;
            is_root &= is_root - 1u;
            if (at >= capacity) return;   // (nothing is written past the output)
            roots[at++] = (int)(lo + i);
        }
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_components_relabel(unsigned* __restrict__ label, long long n_vox, const int* __restrict__ roots, int n_roots) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long v = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; v < n_vox; v += stride) {
        const unsigned root = label[v];
        if (root == kCompSentinel) continue;
        int lo = 0, hi = n_roots;   // the first entry >= root: the root itself
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((unsigned)roots[mid] < root) lo = mid + 1; else hi = mid;
        }
        label[v] = (unsigned)lo;
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_components_stats_init(long long n, long long* __restrict__ sizes, long long* __restrict__ sums, int* __restrict__ bbox) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n; i += stride) {
        sizes[i] = 0;
        for (int a = 0; a < 3; ++a) {
            sums[3 * i + a] = 0;
            bbox[6 * i + a] = 0x7fffffff;
            bbox[6 * i + 3 + a] = -1;
        }
    }
}

// one record joins a component's totals.  The box only tightens, so what a plain load sees bounds it: the atomic is issued only where
// the record would move it
__device__ __forceinline__ void comp_stats_add(long long id, long long n, long long sx, long long sy, long long sz, const int* lo, const int* hi,
                                               unsigned long long* sizes, unsigned long long* sums, int* bbox) {
    __hip_atomic_fetch_add(sizes + id, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(sums + 3 * id, (unsigned long long)sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(sums + 3 * id + 1, (unsigned long long)sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(sums + 3 * id + 2, (unsigned long long)sz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int a = 0; a < 3; ++a) {
        if (lo[a] < bbox[6 * id + a]) __hip_atomic_fetch_min(bbox + 6 * id + a, lo[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (hi[a] > bbox[6 * id + 3 + a]) __hip_atomic_fetch_max(bbox + 6 * id + 3 + a, hi[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// what a wave has gathered for one component and not yet added: every lane holds the same values
struct CompRun {
    long long id, n, sx, sy, sz;   // id < 0: nothing
    int lo[3], hi[3];
};
__device__ __forceinline__ void comp_run_reset(CompRun& r, long long id) {
    r.id = id, r.n = r.sx = r.sy = r.sz = 0;
    for (int a = 0; a < 3; ++a) r.lo[a] = 0x7fffffff, r.hi[a] = -1;
}

constexpr int kCompSlots = 16;   // components a block of k_components_stats gathers in LDS before it touches memory
constexpr int kCompPeels = 4;    // ids of one wave's 64 voxels that are looked at as groups
constexpr int kCompGroup = 8;    // lanes from which a group is reduced by shuffles

// the block's table: a run goes to the slot that holds its id or to an empty one (claimed by a compare-and-swap), else to memory
struct CompTable {
    unsigned long long id[kCompSlots];   // ~0: empty
    unsigned long long acc[kCompSlots][4];
    int lo[kCompSlots][3], hi[kCompSlots][3];
};
__device__ __forceinline__ void comp_table_add(CompTable& t, const CompRun& r, unsigned long long* sizes, unsigned long long* sums, int* bbox) {
    const unsigned long long id = (unsigned long long)r.id;
    for (int probe = 0; probe < kCompSlots; ++probe) {
        const int k = (int)((id + probe) % kCompSlots);
        const unsigned long long was = atomicCAS(&t.id[k], ~0ull, id);
        if (was != ~0ull && was != id) continue;
        atomicAdd(&t.acc[k][0], (unsigned long long)r.n);
        atomicAdd(&t.acc[k][1], (unsigned long long)r.sx);
        atomicAdd(&t.acc[k][2], (unsigned long long)r.sy);
        atomicAdd(&t.acc[k][3], (unsigned long long)r.sz);
        for (int a = 0; a < 3; ++a) atomicMin(&t.lo[k][a], r.lo[a]), atomicMax(&t.hi[k][a], r.hi[a]);
        return;
    }
    comp_stats_add(r.id, r.n, r.sx, r.sy, r.sz, r.lo, r.hi, sizes, sums, bbox);
}

// a word that is not an id below n_components (a clear voxel, or a volume that holds something else) counts for nothing.  The set
// voxels of a wave's 64 are taken one id after another; the only group of a wave, and any group of 8 lanes or more, is reduced by
// shuffles.  Where it is the whole wave (inside a large component) the sum stays in registers for as long as the id stays; a run that ends, and a group that is
// only part of a wave (a row along x that crosses a one-voxel wall between two large components), goes to the block's table in
// LDS, and the table goes to memory once, when the block is done: a component of millions of voxels costs a few atomics per
// block, not per wave and pass.  Smaller groups add for themselves.  Integer sums: the grouping changes no bit.
__global__ void __launch_bounds__(TO_BLOCK)
k_components_stats(const unsigned* __restrict__ label, OccGeom g, long long n_vox, unsigned n_components, unsigned long long* sizes,
                   unsigned long long* sums, int* bbox) {
    __shared__ CompTable s_t;
    if (threadIdx.x < kCompSlots) {
        s_t.id[threadIdx.x] = ~0ull;
        for (int a = 0; a < 4; ++a) s_t.acc[threadIdx.x][a] = 0ull;
        for (int a = 0; a < 3; ++a) s_t.lo[threadIdx.x][a] = 0x7fffffff, s_t.hi[threadIdx.x][a] = -1;
    }
    __syncthreads();
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    const int lane = threadIdx.x & 63;
    const unsigned plane = (unsigned)g.nx * (unsigned)g.ny;
    CompRun run;
    comp_run_reset(run, -1);
    for (long long base = (long long)blockIdx.x * TO_BLOCK + (threadIdx.x - lane); base < n_vox; base += stride) {   // (uniform per wave)
        const long long v = base + lane;
        const unsigned id = v < n_vox ? label[v] : kCompSentinel;
        const bool set = id < n_components;
        const unsigned long long votes = __ballot(set);
        if (votes == 0ull) continue;
        const unsigned u = (unsigned)v;   // (v < 2^31)
        const int z = (int)(u / plane), y = (int)((u - (unsigned)z * plane) / (unsigned)g.nx), x = (int)(u - (unsigned)z * plane - (unsigned)y * (unsigned)g.nx);
        const int at[3] = {x, y, z};
        // the wave's set voxels, one id after another (at most kCompPeels of them): the group that is the whole wave's and any group
        // of kCompGroup lanes or more is reduced by shuffles — the whole wave's joins the run, a part's goes to the table; the lanes
        // of smaller groups add for themselves
        unsigned long long left = votes;
        for (int peel = 0; peel < kCompPeels && left != 0ull; ++peel) {   // (uniform)
            const unsigned lead = __shfl(id, __ffsll((long long)left) - 1);
            const bool mine = set && id == lead;
            const unsigned long long group = __ballot(mine);
            left &= ~group;
            if (group != votes && __popcll(group) < kCompGroup) {   // (a wave of one id is reduced whatever its size)
                if (mine) comp_stats_add(id, 1, x, y, z, at, at, sizes, sums, bbox);
                continue;
            }
            int n = mine ? 1 : 0, sx = mine ? x : 0, sy = mine ? y : 0, sz = mine ? z : 0;   // (64 lanes x 2047 fits an int)
            int lo[3], hi[3];
            for (int a = 0; a < 3; ++a) lo[a] = mine ? at[a] : 0x7fffffff, hi[a] = mine ? at[a] : -1;
            for (int sh = 32; sh > 0; sh >>= 1) {
                n += __shfl_xor(n, sh), sx += __shfl_xor(sx, sh), sy += __shfl_xor(sy, sh), sz += __shfl_xor(sz, sh);
                for (int a = 0; a < 3; ++a) lo[a] = min(lo[a], __shfl_xor(lo[a], sh)), hi[a] = max(hi[a], __shfl_xor(hi[a], sh));
            }
            if (group == votes) {   // the whole wave: it joins the run (every lane holds the run)
                if (run.id != (long long)lead) {
                    if (run.id >= 0 && lane == 0) comp_table_add(s_t, run, sizes, sums, bbox);
                    comp_run_reset(run, lead);
                }
                run.n += n, run.sx += sx, run.sy += sy, run.sz += sz;
                for (int a = 0; a < 3; ++a) run.lo[a] = min(run.lo[a], lo[a]), run.hi[a] = max(run.hi[a], hi[a]);
            } else if (lane == 0) {
                CompRun part;
                part.id = lead, part.n = n, part.sx = sx, part.sy = sy, part.sz = sz;
                for (int a = 0; a < 3; ++a) part.lo[a] = lo[a], part.hi[a] = hi[a];
                comp_table_add(s_t, part, sizes, sums, bbox);
            }
        }
        if (set && ((left >> lane) & 1ull)) comp_stats_add(id, 1, x, y, z, at, at, sizes, sums, bbox);
    }
    if (run.id >= 0 && lane == 0) comp_table_add(s_t, run, sizes, sums, bbox);
    __syncthreads();
    if (threadIdx.x < kCompSlots && s_t.id[threadIdx.x] != ~0ull) {
        const int k = threadIdx.x;
        comp_stats_add((long long)s_t.id[k], (long long)s_t.acc[k][0], (long long)s_t.acc[k][1], (long long)s_t.acc[k][2], (long long)s_t.acc[k][3],
                       s_t.lo[k], s_t.hi[k], sizes, sums, bbox);
    }
}

constexpr long long kCompNoValue = 0xFFFFFFFFll;   // min_value between the launches: no voxel of the component holds a value yet
constexpr int kCompNoVoxel = 0x7fffffff;

__global__ void __launch_bounds__(TO_BLOCK)
k_components_min_init(long long n, long long* __restrict__ min_value, int* __restrict__ min_voxel) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n; i += stride) {
        min_value[i] = kCompNoValue;
        min_voxel[i] = kCompNoVoxel;
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_components_min_value(const unsigned* __restrict__ label, const unsigned* __restrict__ values, long long n_vox, unsigned n_components,
                       long long* min_value) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long v = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; v < n_vox; v += stride) {
        const unsigned id = label[v];
        if (id >= n_components) continue;
        const long long c = (long long)values[v];
        // (the minimum only falls: what a plain load sees is an upper bound of it, so skipping on it is safe)
        if (c != kCompNoValue && c < min_value[id]) __hip_atomic_fetch_min(min_value + id, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// (a launch of its own: min_value is final)
__global__ void __launch_bounds__(TO_BLOCK)
k_components_min_voxel(const unsigned* __restrict__ label, const unsigned* __restrict__ values, long long n_vox, unsigned n_components,
                       const long long* __restrict__ min_value, int* min_voxel) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long v = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; v < n_vox; v += stride) {
        const unsigned id = label[v];
        if (id >= n_components) continue;
        const long long c = (long long)values[v];
        if (c != kCompNoValue && c == min_value[id] && (int)v < min_voxel[id])
            __hip_atomic_fetch_min(min_voxel + id, (int)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_components_min_finish(long long n, long long* __restrict__ min_value, int* __restrict__ min_voxel) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n; i += stride)
        if (min_value[i] == kCompNoValue) {
            min_value[i] = -1;
            min_voxel[i] = -1;
        }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_components_positions(const unsigned* __restrict__ label, OccGeom g, const float* __restrict__ pos, long long m, long long* __restrict__ out) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < m; i += stride) {
        int x, y, z;
        long long id = -2;
        if (occ_locate(g, pos + 3 * i, x, y, z) == kOccInside) {
            const unsigned v = label[field_index(g, x, y, z)];
            id = v == kCompSentinel ? -1 : (long long)v;
        }
        out[i] = id;
    }
}

inline bool comp_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// a label volume and its geometry (argument checks only)
inline int comp_labels(const void* labels, size_t labels_bytes, const tohip_occ_geom* geom, OccGeom& g) {
    const int rc = occ_check(labels, ~(size_t)0, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!comp_aligned(labels, 4)) return TOHIP_EINVAL;
    return labels_bytes < travel_cost_bytes(g) ? TOHIP_ENOSPC : TOHIP_OK;
}

template <int C>
inline void comp_relax_launch(unsigned blocks, hipStream_t st, const OccGeom& g, unsigned* label, const int* list, unsigned* hdr32, int parity,
                              unsigned* next, const TravelTiles& t) {
    k_components_relax<C><<<blocks, TO_BLOCK, 0, st>>>(g, label, list, hdr32, parity, next, (int)t.ntx, (int)t.nty, (int)t.ntz);
}

}  // namespace

extern "C" size_t tohip_components_bytes(int32_t nx, int32_t ny, int32_t nz) {
    return occ_dims_ok(nx, ny, nz) ? field_voxels(nx, ny, nz) * sizeof(uint32_t) : 0;
}

// the header words, the two bitmaps and the tile list as the travel field lays them out, then the root counts of the blocks + 1
extern "C" size_t tohip_components_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (!occ_dims_ok(nx, ny, nz)) return 0;
    return tohip_travel_workspace_bytes(nx, ny, nz) +
           travel_align((size_t)(comp_root_blocks((long long)field_voxels(nx, ny, nz)) + 1) * sizeof(int64_t));
}

extern "C" int tohip_components_build(const void* plane, size_t grid_bytes, const tohip_occ_geom* geom, int32_t connectivity, void* labels,
                                      size_t labels_bytes, void* workspace, size_t workspace_bytes, int32_t rounds_per_check, int32_t* roots,
                                      int64_t roots_capacity, int64_t* n_components_host, int64_t* rounds_host, void* stream_) {
    OccGeom g;
    const int rc = occ_check(plane, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if ((connectivity != 6 && connectivity != 18 && connectivity != 26) || rounds_per_check < 1 || rounds_per_check > kCompMaxRoundsPerCheck ||
        !labels || !workspace || !n_components_host || roots_capacity < 0 || (roots_capacity > 0 && !roots))
        return TOHIP_EINVAL;
    if (!comp_aligned(plane, 4) || !comp_aligned(labels, 4) || !comp_aligned(workspace, 256) || !comp_aligned(roots, 4)) return TOHIP_EINVAL;
    if (labels == plane || labels == workspace || workspace == plane || (roots && ((void*)roots == labels || (void*)roots == workspace)))
        return TOHIP_EINVAL;
    if (labels_bytes < travel_cost_bytes(g) || workspace_bytes < tohip_components_workspace_bytes(g.nx, g.ny, g.nz)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const TravelTiles t = travel_tiles(g.nx, g.ny, g.nz);
    const size_t bm = travel_bitmap_bytes(t);
    unsigned* hdr32 = (unsigned*)workspace;
    unsigned* bitmap[2] = {(unsigned*)((char*)workspace + kTravelHdr), (unsigned*)((char*)workspace + kTravelHdr + bm)};
    int* list = (int*)((char*)workspace + kTravelHdr + 2 * bm);
    long long* counts = (long long*)((char*)workspace + tohip_travel_workspace_bytes(g.nx, g.ny, g.nz));
    unsigned* lab = (unsigned*)labels;
    hipError_t e = hipMemsetAsync(workspace, 0, kTravelHdr + 2 * bm, st);
    if (e != hipSuccess) return (int)e;
    const long long n_vox = (long long)field_voxels(g), n_words = (long long)occ_words(g.nx, g.ny, g.nz);
    k_components_init<<<occ_grid_blocks(n_words), TO_BLOCK, 0, st>>>(occ_data(plane), g, n_words, lab, bitmap[0], t.ntx, t.nty);
    TO_HIP_CHECK_LAUNCH();
    const unsigned compact_blocks = (unsigned)((t.words + TO_BLOCK - 1) / TO_BLOCK);
    const unsigned relax_blocks = (unsigned)(t.n < kTravelRelaxBlocks ? t.n : kTravelRelaxBlocks);
    int parity = 0;
    for (bool busy = true; busy;) {
        for (int r = 0; r < rounds_per_check; ++r, parity ^= 1) {
            k_travel_compact<<<compact_blocks, TO_BLOCK, 0, st>>>(bitmap[parity], t.words, list, hdr32 + 2 + parity);
            TO_HIP_CHECK_LAUNCH();
            if (connectivity == 6) comp_relax_launch<6>(relax_blocks, st, g, lab, list, hdr32, parity, bitmap[parity ^ 1], t);
            else if (connectivity == 18) comp_relax_launch<18>(relax_blocks, st, g, lab, list, hdr32, parity, bitmap[parity ^ 1], t);
            else comp_relax_launch<26>(relax_blocks, st, g, lab, list, hdr32, parity, bitmap[parity ^ 1], t);
            TO_HIP_CHECK_LAUNCH();
        }
        // one word back: the tiles the last round worked on (none: nothing was activated after it) and the rounds that had work
        int64_t status = 0;
        const int back = occ_read_back(&status, workspace, st);
        if (back != TOHIP_OK) return back;
        busy = (uint32_t)status != 0u;
        if (!busy && rounds_host) *rounds_host = status >> 32;
    }
    // the roots, counted and listed in ascending order; C comes back once
    const long long nb = comp_root_blocks(n_vox);
    k_components_roots<0><<<(unsigned)nb, TO_BLOCK, 0, st>>>(lab, n_vox, counts, 0, nullptr);
    TO_HIP_CHECK_LAUNCH();
    k_occ_scan<<<1, TO_BLOCK, 0, st>>>(counts, nb);
    TO_HIP_CHECK_LAUNCH();
    const int back = occ_read_back(n_components_host, counts + nb, st);
    if (back != TOHIP_OK) return back;
    const int64_t C = *n_components_host;
    if (C > roots_capacity) return TOHIP_ENOSPC;   // (the labels stay root indices; roots is untouched)
    if (C == 0) return TOHIP_OK;
    k_components_roots<1><<<(unsigned)nb, TO_BLOCK, 0, st>>>(lab, n_vox, counts, roots_capacity, roots);
    TO_HIP_CHECK_LAUNCH();
    k_components_relabel<<<occ_grid_blocks(n_vox), TO_BLOCK, 0, st>>>(lab, n_vox, roots, (int)C);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_components_stats(const void* labels, size_t labels_bytes, const tohip_occ_geom* geom, int64_t n_components, int64_t* sizes,
                                      int64_t* sums, int32_t* bbox, void* stream_) {
    OccGeom g;
    const int rc = comp_labels(labels, labels_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (n_components < 0 || n_components > (int64_t)1 << 31 || (n_components > 0 && (!sizes || !sums || !bbox))) return TOHIP_EINVAL;
    if (!comp_aligned(sizes, 8) || !comp_aligned(sums, 8) || !comp_aligned(bbox, 4)) return TOHIP_EINVAL;
    if (n_components == 0) return TOHIP_OK;
    hipStream_t st = (hipStream_t)stream_;
    const long long n_vox = (long long)field_voxels(g);
    k_components_stats_init<<<occ_grid_blocks(n_components), TO_BLOCK, 0, st>>>(n_components, (long long*)sizes, (long long*)sums, bbox);
    TO_HIP_CHECK_LAUNCH();
    k_components_stats<<<occ_grid_blocks(n_vox), TO_BLOCK, 0, st>>>((const unsigned*)labels, g, n_vox, (unsigned)n_components,
                                                                    (unsigned long long*)sizes, (unsigned long long*)sums, bbox);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_components_min(const void* labels, size_t labels_bytes, const tohip_occ_geom* geom, const void* values, size_t values_bytes,
                                    int64_t n_components, int64_t* min_value, int32_t* min_voxel, void* stream_) {
    OccGeom g;
    const int rc = comp_labels(labels, labels_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!values || !comp_aligned(values, 4) || values == labels || n_components < 0 || n_components > (int64_t)1 << 31 ||
        (n_components > 0 && (!min_value || !min_voxel)) || !comp_aligned(min_value, 8) || !comp_aligned(min_voxel, 4))
        return TOHIP_EINVAL;
    if (values_bytes < travel_cost_bytes(g)) return TOHIP_ENOSPC;
    if (n_components == 0) return TOHIP_OK;
    hipStream_t st = (hipStream_t)stream_;
    const long long n_vox = (long long)field_voxels(g);
    const int small = occ_grid_blocks(n_components), big = occ_grid_blocks(n_vox);
    k_components_min_init<<<small, TO_BLOCK, 0, st>>>(n_components, (long long*)min_value, min_voxel);
    TO_HIP_CHECK_LAUNCH();
    k_components_min_value<<<big, TO_BLOCK, 0, st>>>((const unsigned*)labels, (const unsigned*)values, n_vox, (unsigned)n_components,
                                                     (long long*)min_value);
    TO_HIP_CHECK_LAUNCH();
    k_components_min_voxel<<<big, TO_BLOCK, 0, st>>>((const unsigned*)labels, (const unsigned*)values, n_vox, (unsigned)n_components,
                                                     (const long long*)min_value, min_voxel);
    TO_HIP_CHECK_LAUNCH();
    k_components_min_finish<<<small, TO_BLOCK, 0, st>>>(n_components, (long long*)min_value, min_voxel);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_components_positions(const void* labels, size_t labels_bytes, const tohip_occ_geom* geom, const float* positions, int64_t m,
                                          int64_t* out, void* stream_) {
    OccGeom g;
    const int rc = comp_labels(labels, labels_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occ_count_ok(m) || (m > 0 && (!positions || !out))) return TOHIP_EINVAL;
    if (m == 0) return TOHIP_OK;
    k_components_positions<<<occ_grid_blocks(m), TO_BLOCK, 0, (hipStream_t)stream_>>>((const unsigned*)labels, g, positions, m, (long long*)out);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
