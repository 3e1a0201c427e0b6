// travel_kernels.hip — a travel field over the clearance field ("Travel field"), for gfx950.  Included after
// field_kernels.hip (behind evidence_kernels.hip): the geometry, occ_locate, the brick layout and field_index are that file's and
// frontier_kernels.hip's.
//
// The TRAVERSABLE set T: the voxels inside dims with field >= need2 and, with a map's two planes, state 1 — tohip_field_nodes' mask
// at stride 1.  A MOVE goes from v to one of its 26 neighbours u and is allowed iff every voxel of the box spanned by v and u (2, 4
// or 8 voxels) is in T: no corner is cut.  Weights in 1/64 voxel edge: 64 (face), 91 (edge), 111 (corner).  cost[v] (uint32, one
// word per voxel inside dims, x fastest) = the length of the shortest allowed path from a seeded source, 0xFFFFFFFF where there is
// none of length <= limit (limit < 2^31: no sum overflows).  The answer is the unique fixed point of cost[s] = 0, cost[v] = min
// over the allowed u of cost[u] + w: it does not depend on the order of the relaxation, so every schedule below gives the same bits.
//
//   k_travel_fill     every word of cost <- the sentinel (grid-stride, 64-bit index).
//   k_travel_seed     one lane per source: a position in range whose voxel lies inside dims and in T gets cost 0, seeded[i] = 1 and
//                     the bit in bitmap 0 of its tile and of every neighbouring tile whose halo it lies in; any other source is
//                     ignored, seeded[i] = 0.
//   k_travel_compact  one lane per word of the round's bitmap: the set bits become entries of the tile list (an integer atomic add
//                     per word reserves their places; the order of the list is of no consequence), the word is cleared.
//   k_travel_relax    one block per listed tile of 8 x 8 x 8 voxels (a block strides over the list), two voxels per lane.  The
//                     tile and a one-voxel halo of costs (10^3 words) and of T (10^3 bytes) go to LDS, each voxel's 26-bit mask of
//                     allowed moves is derived once, and the block relaxes in place in LDS until a whole sweep changes nothing
//                     (__syncthreads_or): a word has one writer, values only fall and every value ever stored is the length of a
//                     real path, so a read that races with a write sees an upper bound either way.  Only the tile's own voxels
//                     that fell are written back; for each of the 26 neighbouring tiles the block sets that tile's bit in the NEXT
//                     round's bitmap iff it lowered a voxel of the layer that touches it.  A halo word read while its owner
//                     writes it is old or new — both upper bounds — and the owner's lowering re-activates the reader.
//   k_travel_positions (M,3) f32 positions -> int64 cost (-1 unreachable, -2 out of range or outside dims) and / or f32 metres.
//   k_travel_paths    one wave per goal: lanes 0 .. 26 (13 idle) each test one move against the path rule — allowed, and cost[u] +
//                     w == cost[v] — and a ballot names the lowest; rows are the voxel centres from the goal to its source.
//   k_view_volume_pick_travel   k_view_volume_pick with a cost row: gain 2^20 - m cost decides, among the reachable candidates.
//   k_assign_greedy   one block: rows (robots) take columns (openings) in ascending order of the key (cost, row, column).
//
// FIELDS IN BATCHES ("Travel fields in batches"): n_fields cost volumes one after the other (field b starts at word b
// nx ny nz), one T, one worklist.  A work item is (field, tile) packed as b n_tiles + t — a bit of the bitmaps, an entry of the list —
// and the kernels above are the batch's: the single build is their n_fields = 1 (b = 0 everywhere, the same words in the same order).
// Fields share no cost word, so the fixed-point argument holds field by field.
//
// WEIGHTED FIELDS ("Weighted travel fields"): a layer kappa of one byte per voxel inside dims (dense, x fastest, the
// cost words' index), 16 <= kappa <= 255, 16 neutral.  The move m between v and u costs step = (w_m (kappa[v] + kappa[u]) + 16) >> 5:
// symmetric, an integer, >= w_m, exactly w_m at kappa = 16, at most (111 x 510 + 16) >> 5 = 1769.  T, the move rule, the seeds, limit
// and the sentinel stay; the answer is the same unique fixed point with step in place of w.  k_travel_relax<true> and
// k_travel_paths<true> are the kernels above with a third halo array (10^3 bytes of kappa) and the step formed per move; <false> is
// the unweighted kernel, instruction for instruction (the switch is a template parameter).
//   k_travel_weights  one lane per voxel: kappa[v] = lut[min(field[v], n_lut - 1)], + unknown_add (saturating at 255) where the map's
//                     two planes are given and v is neither occupied nor known free.
//
// Every kernel ends on its own: no block waits for another.  No float atomics, no process-wide state; every argument check returns
// before anything is enqueued.
namespace {

constexpr unsigned kTravelSentinel = 0xFFFFFFFFu;
constexpr unsigned kTravelInf = 0xFFFFFF00u;          // "no path" inside LDS: + 111 does not wrap, and exceeds every limit
constexpr unsigned kTravelInfWeighted = 0xFFFFF000u;  // the same for a weighted field: + 1769, the largest step, does not wrap
constexpr long long kTravelMaxLimit = 0x7fffffffll;
constexpr int kTravelTile = 8;                        // voxels per tile edge
constexpr int kTravelHalo = kTravelTile + 2;
constexpr int kTravelHaloN = kTravelHalo * kTravelHalo * kTravelHalo;
constexpr int kTravelRelaxBlocks = 4096;              // blocks of a relax launch: they stride over the list
constexpr size_t kTravelHdr = 256;                    // [0] u64 status = rounds with work << 32 | tiles of the last round;
                                                      // [2], [3] u32 the two rounds' list counts; [4] u32 rounds with work;
                                                      // [5] u32 the most items of one round; [6] u64 the items of all rounds
                                                      // (what tools/time_travel_batch.py reads: items per round)
constexpr int kTravelMaxRoundsPerCheck = 65536;
constexpr long long kTravelMaxItems = 0x7fffffffll;   // (field, tile) items of a batch: a list entry is an int

struct TravelTiles { long long ntx, nty, ntz, n, words; };
inline TravelTiles travel_tiles(int64_t nx, int64_t ny, int64_t nz) {
    TravelTiles t;
    t.ntx = (nx + kTravelTile - 1) / kTravelTile, t.nty = (ny + kTravelTile - 1) / kTravelTile, t.ntz = (nz + kTravelTile - 1) / kTravelTile;
    t.n = t.ntx * t.nty * t.ntz;
    t.words = (t.n + 31) / 32;
    return t;
}
inline size_t travel_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t travel_bitmap_bytes(const TravelTiles& t, int n_fields = 1) { return travel_align((size_t)t.words * 4 * (size_t)n_fields); }

// what decides T, in one argument
struct TravelSet {
    const uint16_t* field;
    const unsigned* occ;   // both planes or neither
    const unsigned* fre;
    OccGeom g;
    int need2;
};

__device__ __forceinline__ bool travel_in_set(const TravelSet& s, int x, int y, int z) {
    if (!occ_inside(s.g, x, y, z)) return false;
    if ((int)s.field[field_index(s.g, x, y, z)] < s.need2) return false;
    if (s.occ) {
        const int w = occ_word(s.g, x, y, z), b = occ_bit(x, y, z);
        if (!(((s.fre[w] & ~s.occ[w]) >> b) & 1u)) return false;   // state 1
    }
    return true;
}

// move m = (dz + 1) 9 + (dy + 1) 3 + (dx + 1), m != 13
__device__ __forceinline__ constexpr int travel_dx(int m) { return m % 3 - 1; }
__device__ __forceinline__ constexpr int travel_dy(int m) { return (m / 3) % 3 - 1; }
__device__ __forceinline__ constexpr int travel_dz(int m) { return m / 9 - 1; }
__device__ __forceinline__ constexpr unsigned travel_weight(int m) {
    const int k = (travel_dx(m) != 0) + (travel_dy(m) != 0) + (travel_dz(m) != 0);
    return k == 1 ? 64u : (k == 2 ? 91u : 111u);
}
// the bits of a 27-voxel neighbourhood mask (bit = the move's number, 13 the voxel itself) that move m needs: its box
__device__ __forceinline__ constexpr unsigned travel_box(int m) {
    unsigned need = 0u;
    for (int i = 0; i < 8; ++i) {
        const int ex = (i & 1) ? travel_dx(m) : 0, ey = (i & 2) ? travel_dy(m) : 0, ez = (i & 4) ? travel_dz(m) : 0;
        need |= 1u << ((ez + 1) * 9 + (ey + 1) * 3 + (ex + 1));
    }
    return need;
}

// the weighted cost of a move of weight w between voxels of factors ka and kb (16 = neutral: exactly w)
__device__ __forceinline__ constexpr unsigned travel_step(unsigned w, unsigned ka, unsigned kb) { return (w * (ka + kb) + 16u) >> 5; }

__device__ __forceinline__ float travel_centre(float o, int i, float r) { return __fadd_rn(o, __fmul_rn((float)i + 0.5f, r)); }

__global__ void __launch_bounds__(TO_BLOCK) k_travel_fill(unsigned* __restrict__ cost, long long n_vox) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n_vox; i += stride) cost[i] = kTravelSentinel;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_travel_seed(TravelSet s, const float* __restrict__ src, const int* __restrict__ src_field, int n_fields, long long n_src,
              unsigned* __restrict__ cost, long long n_vox, unsigned* __restrict__ bitmap, long long ntx, long long nty, long long n_tiles,
              uint8_t* __restrict__ seeded) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n_src; i += stride) {
        int x, y, z;
        const int b = src_field ? src_field[i] : 0;   // (no row of fields: the single build, field 0)
        const bool ok = b >= 0 && b < n_fields && occ_locate(s.g, src + 3 * i, x, y, z) == kOccInside && travel_in_set(s, x, y, z);
        if (ok) {
            cost[b * n_vox + field_index(s.g, x, y, z)] = 0u;   // (two sources in one voxel store the same word)
            // its tile, and every neighbouring tile whose halo it lies in: a seed in a border layer whose neighbours inside its own
            // tile are all closed lowers nothing there, so the relaxation of its own tile alone would never wake the tile next door
            const long long ntz = n_tiles / (ntx * nty);
            const int tx = x >> 3, ty = y >> 3, tz = z >> 3;
            const int ax = (x & 7) == 0 ? -1 : ((x & 7) == 7 ? 1 : 0), ay = (y & 7) == 0 ? -1 : ((y & 7) == 7 ? 1 : 0),
                      az = (z & 7) == 0 ? -1 : ((z & 7) == 7 ? 1 : 0);
            for (int k = 0; k < 8; ++k) {
                if (((k & 1) && ax == 0) || ((k & 2) && ay == 0) || ((k & 4) && az == 0)) continue;
                const int ux = tx + ((k & 1) ? ax : 0), uy = ty + ((k & 2) ? ay : 0), uz = tz + ((k & 4) ? az : 0);
                if ((unsigned)ux >= (unsigned)ntx || (unsigned)uy >= (unsigned)nty || (unsigned)uz >= (unsigned)ntz) continue;
                const long long t = b * n_tiles + ((long long)uz * nty + uy) * ntx + ux;
                __hip_atomic_fetch_or(bitmap + (t >> 5), 1u << (t & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (seeded) seeded[i] = ok ? 1 : 0;
    }
}

// the set bits of the round's bitmap -> list[0 .. *count), the bitmap cleared.  *count is zero when the launch begins.
__global__ void __launch_bounds__(TO_BLOCK)
k_travel_compact(unsigned* __restrict__ bitmap, long long words, int* __restrict__ list, unsigned* __restrict__ count) {
    const long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    if (w >= words) return;
    unsigned bits = bitmap[w];
    if (bits == 0u) return;
    bitmap[w] = 0u;
    unsigned at = __hip_atomic_fetch_add(count, (unsigned)__popc(bits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (bits != 0u) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1u;
        list[at++] = (int)(w * 32 + b);   // (at most 2^31 - 1 items)
    }
}

// kWeighted: the moves cost travel_step over the layer kappa (one byte per voxel, the cost words' index); else kappa is not read
template <bool kWeighted>
__global__ void __launch_bounds__(TO_BLOCK)
k_travel_relax(TravelSet s, unsigned* cost_all, long long n_vox, unsigned limit, const int* __restrict__ list, unsigned* __restrict__ hdr32,
               int parity, unsigned* __restrict__ next_all, int ntx, int nty, int ntz, int n_tiles, const uint8_t* __restrict__ kappa) {
    __shared__ unsigned s_cost[kTravelHaloN];
    __shared__ unsigned char s_in[kTravelHaloN];
    __shared__ unsigned s_touch;
    unsigned char* s_kappa = nullptr;
    if constexpr (kWeighted) {
        __shared__ unsigned char s_kappa_halo[kTravelHaloN];
        s_kappa = s_kappa_halo;
    }
    constexpr unsigned kInf = kWeighted ? kTravelInfWeighted : kTravelInf;
    const unsigned count = hdr32[2 + parity];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the bookkeeping of the round: the other round's count starts from zero, and the status word the host reads
        hdr32[2 + (parity ^ 1)] = 0u;
        const unsigned rounds = hdr32[4] + (count != 0u ? 1u : 0u);
        hdr32[4] = rounds;
        hdr32[0] = count;
        hdr32[1] = rounds;
        if (count > hdr32[5]) hdr32[5] = count;
        *(unsigned long long*)(hdr32 + 6) += count;
    }
    const OccGeom& g = s.g;
    for (unsigned item = blockIdx.x; item < count; item += gridDim.x) {
        const int e = list[item];
        const int fb = e / n_tiles, t = e - fb * n_tiles;   // the item's field and tile
        unsigned* cost = cost_all + fb * n_vox;
        const long long next_at = (long long)fb * n_tiles;
        const int tx = t % ntx, ty = (t / ntx) % nty, tz = t / (ntx * nty);
        const int x0 = tx * kTravelTile - 1, y0 = ty * kTravelTile - 1, z0 = tz * kTravelTile - 1;   // the halo's corner
        if (threadIdx.x == 0) s_touch = 0u;
        for (int i = threadIdx.x; i < kTravelHaloN; i += TO_BLOCK) {
            const int x = x0 + i % kTravelHalo, y = y0 + (i / kTravelHalo) % kTravelHalo, z = z0 + i / (kTravelHalo * kTravelHalo);
            const bool in = travel_in_set(s, x, y, z);
            unsigned c = kInf;
            if (in) {
                c = cost[field_index(g, x, y, z)];
                if (c > limit) c = kInf;   // (the sentinel)
            }
            s_cost[i] = c;
            s_in[i] = in ? 1 : 0;
            if constexpr (kWeighted) s_kappa[i] = in ? kappa[field_index(g, x, y, z)] : 0;   // (outside T: never an endpoint)
        }
        __syncthreads();
        // this lane's two voxels: their place in the halo block, the moves they may make, the value they came with
        int at[2];
        unsigned allowed[2], first[2], mine[2], own[2];   // (own: the lane's two factors, weighted fields only)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int l = threadIdx.x + k * TO_BLOCK;
            at[k] = (((l >> 6) + 1) * kTravelHalo + ((l >> 3) & 7) + 1) * kTravelHalo + (l & 7) + 1;
            unsigned around = 0u;
#pragma unroll
            for (int m = 0; m < 27; ++m)
                around |= (unsigned)s_in[at[k] + (travel_dz(m) * kTravelHalo + travel_dy(m)) * kTravelHalo + travel_dx(m)] << m;
            unsigned ok = 0u;
            if ((around >> 13) & 1u) {
#pragma unroll
                for (int m = 0; m < 27; ++m)
                    if (m != 13 && (around & travel_box(m)) == travel_box(m)) ok |= 1u << m;
            }
            allowed[k] = ok;
            first[k] = mine[k] = s_cost[at[k]];
            if constexpr (kWeighted) own[k] = s_kappa[at[k]];
        }
        bool changed;
        do {
            changed = false;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (allowed[k] == 0u) continue;
                unsigned best = mine[k];
#pragma unroll
                for (int m = 0; m < 27; ++m) {
                    if (m == 13) continue;
                    const int nb = at[k] + (travel_dz(m) * kTravelHalo + travel_dy(m)) * kTravelHalo + travel_dx(m);
                    unsigned c;
                    if constexpr (kWeighted) c = s_cost[nb] + travel_step(travel_weight(m), own[k], s_kappa[nb]);
                    else c = s_cost[nb] + travel_weight(m);
                    if (((allowed[k] >> m) & 1u) && c < best) best = c;
                }
                if (best < mine[k] && best <= limit) {
                    mine[k] = best;
                    s_cost[at[k]] = best;
                    changed = true;
                }
            }
        } while (__syncthreads_or(changed));
        // what fell goes back, and names the neighbouring tiles whose halo it lies in
        unsigned touch = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (mine[k] >= first[k]) continue;
            const int l = threadIdx.x + k * TO_BLOCK;
            const int lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
            cost[field_index(g, x0 + 1 + lx, y0 + 1 + ly, z0 + 1 + lz)] = mine[k];   // (in T: inside dims)
            const int ax = lx == 0 ? -1 : (lx == 7 ? 1 : 0), ay = ly == 0 ? -1 : (ly == 7 ? 1 : 0), az = lz == 0 ? -1 : (lz == 7 ? 1 : 0);
#pragma unroll
            for (int i = 1; i < 8; ++i) {
                const int ex = (i & 1) ? ax : 0, ey = (i & 2) ? ay : 0, ez = (i & 4) ? az : 0;
                if (((i & 1) && ax == 0) || ((i & 2) && ay == 0) || ((i & 4) && az == 0)) continue;
                touch |= 1u << ((ez + 1) * 9 + (ey + 1) * 3 + (ex + 1));
            }
        }
        for (int sh = 32; sh > 0; sh >>= 1) touch |= __shfl_xor(touch, sh);
        if ((threadIdx.x & 63) == 0 && touch != 0u) atomicOr(&s_touch, touch);
        __syncthreads();
        if (threadIdx.x < 27 && threadIdx.x != 13 && ((s_touch >> threadIdx.x) & 1u)) {
            const int ux = tx + travel_dx(threadIdx.x), uy = ty + travel_dy(threadIdx.x), uz = tz + travel_dz(threadIdx.x);
            if ((unsigned)ux < (unsigned)ntx && (unsigned)uy < (unsigned)nty && (unsigned)uz < (unsigned)ntz) {
                const long long u = next_at + (uz * nty + uy) * ntx + ux;
                __hip_atomic_fetch_or(next_all + (u >> 5), 1u << (u & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();   // (s_touch and the halo block are the next item's)
    }
}

// metres of a cost: fl(fl((float) cost (1/64)) r); +inf unreachable, NaN for -2
__device__ __forceinline__ float travel_metres(long long c, float r) {
    if (c == -2) return __builtin_nanf("");
    if (c < 0) return __builtin_inff();
    return __fmul_rn(__fmul_rn((float)c, 0.015625f), r);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_travel_positions(const unsigned* __restrict__ cost, long long n_vox, OccGeom g, const float* __restrict__ pos, long long m, long long total,
                   long long* __restrict__ cost_out, float* __restrict__ dist_out) {
    // total = n_fields m: row b of the outputs is field b's answer
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < total; i += stride) {
        int x, y, z;
        long long c = -2;
        const long long b = i / m;
        if (occ_locate(g, pos + 3 * (i - b * m), x, y, z) == kOccInside) {
            const unsigned v = cost[b * n_vox + field_index(g, x, y, z)];
            c = v == kTravelSentinel ? -1 : (long long)v;
        }
        if (cost_out) cost_out[i] = c;
        if (dist_out) dist_out[i] = travel_metres(c, g.r);
    }
}

// one wave per goal; rows (n_goals, max_rows, 3): the voxel centres goal -> source; counts: rows, 0 unreachable (or the goal out of
// range or outside dims), -needed where the path does not fit.  kWeighted: the predecessor test is there + travel_step == here over
// the layer kappa, which all fields share
template <bool kWeighted>
__global__ void __launch_bounds__(TO_BLOCK)
k_travel_paths(TravelSet s, const unsigned* __restrict__ cost_all, long long n_vox, const float* __restrict__ goals,
               const int* __restrict__ goal_field, int n_fields, long long n_goals, long long max_rows, float* __restrict__ rows,
               long long* __restrict__ counts, const uint8_t* __restrict__ kappa) {
    const int lane = threadIdx.x & 63;
    const long long goal = (long long)blockIdx.x * (TO_BLOCK / 64) + (threadIdx.x >> 6);
    if (goal >= n_goals) return;   // (a whole wave)
    const OccGeom& g = s.g;
    int x, y, z;
    long long n = 0;
    const int fb = goal_field ? goal_field[goal] : 0;   // the field the goal is walked in (no row of fields: field 0)
    const unsigned* cost = cost_all + (fb >= 0 && fb < n_fields ? fb : 0) * n_vox;
    if (fb >= 0 && fb < n_fields && occ_locate(g, goals + 3 * goal, x, y, z) == kOccInside) {
        unsigned here = cost[field_index(g, x, y, z)];
        if (here != kTravelSentinel) {
            float* out = rows + goal * max_rows * 3;
            const int dx = lane < 27 ? travel_dx(lane) : 0, dy = lane < 27 ? travel_dy(lane) : 0, dz = lane < 27 ? travel_dz(lane) : 0;
            const unsigned w = lane < 27 ? travel_weight(lane) : 0u;
            for (;;) {
                if (lane == 0 && n < max_rows) {
                    out[3 * n] = travel_centre(g.ox, x, g.r);
                    out[3 * n + 1] = travel_centre(g.oy, y, g.r);
                    out[3 * n + 2] = travel_centre(g.oz, z, g.r);
                }
                ++n;
                if (here == 0u) break;   // a source
                bool take = false;
                unsigned there = 0u;
                if (lane < 27 && lane != 13 && occ_inside(g, x + dx, y + dy, z + dz)) {
                    there = cost[field_index(g, x + dx, y + dy, z + dz)];
                    unsigned step = w;
                    if constexpr (kWeighted)   // (a neighbour outside T holds the sentinel: its byte decides nothing)
                        step = travel_step(w, kappa[field_index(g, x, y, z)], kappa[field_index(g, x + dx, y + dy, z + dz)]);
                    if (there != kTravelSentinel && there + step == here) {
                        take = true;
                        for (int i = 1; i < 8 && take; ++i) {   // the box of the move (its far corner holds a cost: it is in T)
                            if (((i & 1) && dx == 0) || ((i & 2) && dy == 0) || ((i & 4) && dz == 0)) continue;
                            take = travel_in_set(s, x + ((i & 1) ? dx : 0), y + ((i & 2) ? dy : 0), z + ((i & 4) ? dz : 0));
                        }
                    }
                }
                const unsigned long long votes = __ballot(take);
                if (votes == 0ull) { n = 0; break; }   // (not a built field: no predecessor)
                const int m = __ffsll((long long)votes) - 1;
                x += travel_dx(m), y += travel_dy(m), z += travel_dz(m);
                here = __shfl(there, m);
            }
        }
    }
    if (lane == 0) counts[goal] = n > max_rows ? -n : n;
}

// a weight layer from a clearance field: kappa[v] = lut[min(field[v], n_lut - 1)]; with the two planes, + unknown_add where v is
// neither occupied nor known free, saturating at 255.  One lane per voxel inside dims (grid-stride, 64-bit index).
__global__ void __launch_bounds__(TO_BLOCK)
k_travel_weights(const uint16_t* __restrict__ field, const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, OccGeom g,
                 const uint8_t* __restrict__ lut, int n_lut, unsigned unknown_add, uint8_t* __restrict__ out, long long n_vox) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < n_vox; i += stride) {
        const int d2 = (int)field[i];
        unsigned k = lut[d2 < n_lut ? d2 : n_lut - 1];
        if (occ) {
            const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / ((long long)g.nx * g.ny));
            const int w = occ_word(g, x, y, z), b = occ_bit(x, y, z);
            if (!(((occ[w] | fre[w]) >> b) & 1u)) k = k + unknown_add > 255u ? 255u : k + unknown_add;   // state 0: unknown
        }
        out[i] = (uint8_t)k;
    }
}

// round `round` of a greedy selection that prices the trip: gain 2^20 - m cost decides among the candidates not taken with gain >=
// min_gain and cost >= 0; the lowest index on ties
__global__ void __launch_bounds__(TO_BLOCK)
k_view_volume_pick_travel(const long long* __restrict__ gains, const long long* __restrict__ cost, long long weight, int* __restrict__ taken,
                          long long n, long long min_gain, int round, int* __restrict__ order, long long* __restrict__ picked_gain,
                          int* __restrict__ stop) {
    __shared__ long long s_score[TO_BLOCK];
    __shared__ long long s_idx[TO_BLOCK];
    if (*stop != 0) return;   // (uniform)
    long long best = 0, at = -1;
    for (long long i = threadIdx.x; i < n; i += TO_BLOCK) {   // (ascending: the first of equal scores stays)
        if (taken[i] || gains[i] < min_gain || cost[i] < 0) continue;
        const long long sc = gains[i] * (1ll << 20) - weight * cost[i];
        if (at < 0 || sc > best) { best = sc; at = i; }
    }
    s_score[threadIdx.x] = best;
    s_idx[threadIdx.x] = at;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TO_BLOCK; ++k) {
            if (s_idx[k] < 0) continue;
            if (at < 0 || s_score[k] > best || (s_score[k] == best && s_idx[k] < at)) { best = s_score[k]; at = s_idx[k]; }
        }
        if (at < 0) {
            *stop = 1;
        } else {
            order[round] = (int)at;
            picked_gain[round] = gains[at];
            taken[at] = 1;
        }
    }
}

constexpr int kAssignMaxRows = 64;
constexpr int kAssignMaxCols = 4096;

// the smaller of two (cost, index) keys, across a wave; cost < 0: none
__device__ __forceinline__ void assign_wave_min(long long& c, int& at) {
    for (int sh = 32; sh > 0; sh >>= 1) {
        const long long oc = __shfl_xor(c, sh);
        const int oat = __shfl_xor(at, sh);
        if (oc >= 0 && (c < 0 || oc < c || (oc == c && oat < at))) { c = oc; at = oat; }
    }
}

// greedy assignment in one block: every open row keeps its best unclaimed column (the smallest (cost, column)); the smallest
// (cost, row) among those is the smallest (cost, row, column) of all candidates and is assigned; only the rows whose best column
// was just claimed look again.  Integers only: the same answer in every run.
__global__ void __launch_bounds__(TO_BLOCK)
k_assign_greedy(const long long* __restrict__ cost, int n_rows, int n_cols, long long ld, long long min_cost, int* __restrict__ col_of_row,
                int* __restrict__ row_of_col) {
    __shared__ unsigned char s_claimed[kAssignMaxCols];
    __shared__ long long s_best[kAssignMaxRows];
    __shared__ int s_col[kAssignMaxRows];
    __shared__ unsigned char s_look[kAssignMaxRows];   // 1: the row must look for its best column (again)
    __shared__ unsigned char s_open[kAssignMaxRows];   // 1: the row is unassigned and may still have a candidate
    __shared__ int s_win;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < n_cols; c += TO_BLOCK) { s_claimed[c] = 0; row_of_col[c] = -1; }
    for (int r = threadIdx.x; r < n_rows; r += TO_BLOCK) { s_look[r] = 1; s_open[r] = 1; col_of_row[r] = -1; }
    __syncthreads();
    for (;;) {
        for (int r = wave; r < n_rows; r += TO_BLOCK / 64) {   // (uniform per wave)
            if (!s_open[r] || !s_look[r]) continue;
            long long best = -1;
            int at = -1;
            for (int c = lane; c < n_cols; c += 64) {   // (ascending: the first of equal costs stays)
                const long long v = cost[r * ld + c];
                if (v >= min_cost && !s_claimed[c] && (best < 0 || v < best)) { best = v; at = c; }
            }
            assign_wave_min(best, at);
            if (lane == 0) {
                s_best[r] = best;
                s_col[r] = at;
                s_look[r] = 0;
                if (best < 0) s_open[r] = 0;   // no candidate now: none later, columns are only ever claimed
            }
        }
        __syncthreads();
        if (wave == 0) {
            long long best = lane < n_rows && s_open[lane] ? s_best[lane] : -1;
            int at = lane;
            assign_wave_min(best, at);
            if (lane == 0) s_win = best < 0 ? -1 : at;
        }
        __syncthreads();
        const int win = s_win;
        if (win < 0) return;   // (uniform)
        const int col = s_col[win];
        __syncthreads();       // (everyone has read the winner before it changes)
        if (threadIdx.x == 0) {
            col_of_row[win] = col;
            row_of_col[col] = win;
            s_claimed[col] = 1;
            s_open[win] = 0;
        }
        if (threadIdx.x < n_rows && threadIdx.x != win && s_open[threadIdx.x] && s_col[threadIdx.x] == col) s_look[threadIdx.x] = 1;
        __syncthreads();
    }
}

inline size_t travel_cost_bytes(const OccGeom& g) { return field_voxels(g) * sizeof(uint32_t); }
inline bool travel_fields_ok(int64_t n_fields) { return n_fields >= 1 && n_fields <= TOHIP_TRAVEL_MAX_FIELDS; }

// the field, the planes and the geometry of a call -> its TravelSet (argument checks only)
inline int travel_set(const void* field, size_t field_bytes, const void* occupied_or_null, const void* free_or_null, size_t grid_bytes,
                      const tohip_occ_geom* geom, int32_t need2, TravelSet& s) {
    OccGeom g;
    int rc = field_check(field, field_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if ((occupied_or_null == nullptr) != (free_or_null == nullptr) || need2 < 1 || need2 > kFieldSentinel) return TOHIP_EINVAL;
    if (occupied_or_null) {
        if (occupied_or_null == free_or_null) return TOHIP_EINVAL;
        rc = occ_check(occupied_or_null, grid_bytes, geom, g);
        if (rc != TOHIP_OK) return rc;
    }
    s.field = (const uint16_t*)field;
    s.occ = occupied_or_null ? occ_data(occupied_or_null) : nullptr;
    s.fre = free_or_null ? occ_data(free_or_null) : nullptr;
    s.g = g;
    s.need2 = need2;
    return TOHIP_OK;
}

}  // namespace

extern "C" size_t tohip_travel_bytes(int32_t nx, int32_t ny, int32_t nz) {
    return occ_dims_ok(nx, ny, nz) ? field_voxels(nx, ny, nz) * sizeof(uint32_t) : 0;
}

namespace {

inline size_t travel_workspace_bytes(int64_t nx, int64_t ny, int64_t nz, int n_fields) {
    const TravelTiles t = travel_tiles(nx, ny, nz);
    return kTravelHdr + 2 * travel_bitmap_bytes(t, n_fields) + travel_align((size_t)t.n * (size_t)n_fields * sizeof(int32_t));
}

// the build of n_fields fields in the same rounds; source_field null: every source seeds field 0 (the single build); kappa null: the
// unweighted field
int travel_build(const TravelSet& s, const float* sources, const int32_t* source_field, int64_t n_sources, int n_fields, int64_t limit,
                 int32_t rounds_per_check, void* cost, void* workspace, uint8_t* seeded, int64_t* rounds_host, hipStream_t st,
                 const uint8_t* kappa = nullptr) {
    const TravelTiles t = travel_tiles(s.g.nx, s.g.ny, s.g.nz);
    const size_t bm = travel_bitmap_bytes(t, n_fields);
    const long long items = t.n * n_fields, words = (items + 31) / 32;
    unsigned* hdr32 = (unsigned*)workspace;
    unsigned* bitmap[2] = {(unsigned*)((char*)workspace + kTravelHdr), (unsigned*)((char*)workspace + kTravelHdr + bm)};
    int* list = (int*)((char*)workspace + kTravelHdr + 2 * bm);
    unsigned* c = (unsigned*)cost;
    hipError_t e = hipMemsetAsync(workspace, 0, kTravelHdr + 2 * bm, st);
    if (e != hipSuccess) return (int)e;
    const long long n_vox = (long long)field_voxels(s.g);
    k_travel_fill<<<occ_grid_blocks(n_vox * n_fields), TO_BLOCK, 0, st>>>(c, n_vox * n_fields);
    TO_HIP_CHECK_LAUNCH();
    k_travel_seed<<<occ_grid_blocks(n_sources), TO_BLOCK, 0, st>>>(s, sources, source_field, n_fields, n_sources, c, n_vox, bitmap[0], t.ntx,
                                                                  t.nty, t.n, seeded);
    TO_HIP_CHECK_LAUNCH();
    const unsigned compact_blocks = (unsigned)((words + TO_BLOCK - 1) / TO_BLOCK);
    const unsigned relax_blocks = (unsigned)(items < kTravelRelaxBlocks ? items : kTravelRelaxBlocks);
    int parity = 0;
    for (;;) {
        for (int r = 0; r < rounds_per_check; ++r, parity ^= 1) {
            k_travel_compact<<<compact_blocks, TO_BLOCK, 0, st>>>(bitmap[parity], words, list, hdr32 + 2 + parity);
            TO_HIP_CHECK_LAUNCH();
            if (kappa)
                k_travel_relax<true><<<relax_blocks, TO_BLOCK, 0, st>>>(s, c, n_vox, (unsigned)limit, list, hdr32, parity, bitmap[parity ^ 1],
                                                                        (int)t.ntx, (int)t.nty, (int)t.ntz, (int)t.n, kappa);
            else
                k_travel_relax<false><<<relax_blocks, TO_BLOCK, 0, st>>>(s, c, n_vox, (unsigned)limit, list, hdr32, parity, bitmap[parity ^ 1],
                                                                         (int)t.ntx, (int)t.nty, (int)t.ntz, (int)t.n, nullptr);
            TO_HIP_CHECK_LAUNCH();
        }
        // one word back: the items the last round worked on (none: nothing was activated after it) and the rounds that had work
        int64_t status = 0;
        const int back = occ_read_back(&status, workspace, st);
        if (back != TOHIP_OK) return back;
        if ((uint32_t)status == 0u) {
            if (rounds_host) *rounds_host = status >> 32;
            return TOHIP_OK;
        }
    }
}

// what the single and the batched build ask of their arguments alike (T is checked before)
inline int travel_build_check(const void* field, const void* occupied_or_null, const void* free_or_null, const float* sources, int64_t n_sources,
                              int64_t limit, int32_t rounds_per_check, const void* cost, const void* workspace) {
    if (!sources || n_sources < 1 || !occ_count_ok(n_sources) || limit < 0 || limit > kTravelMaxLimit || rounds_per_check < 1 ||
        rounds_per_check > kTravelMaxRoundsPerCheck || !cost || !workspace)
        return TOHIP_EINVAL;
    const void* ins[3] = {field, occupied_or_null, free_or_null};
    for (const void* p : ins)
        if (p && (p == cost || p == workspace)) return TOHIP_EINVAL;
    if (cost == workspace) return TOHIP_EINVAL;
    return TOHIP_OK;
}

}  // namespace

extern "C" size_t tohip_travel_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    return occ_dims_ok(nx, ny, nz) ? travel_workspace_bytes(nx, ny, nz, 1) : 0;
}

extern "C" size_t tohip_travel_batch_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t n_fields) {
    return occ_dims_ok(nx, ny, nz) && travel_fields_ok(n_fields) ? field_voxels(nx, ny, nz) * sizeof(uint32_t) * (size_t)n_fields : 0;
}

extern "C" size_t tohip_travel_batch_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t n_fields) {
    if (!occ_dims_ok(nx, ny, nz) || !travel_fields_ok(n_fields) || travel_tiles(nx, ny, nz).n * n_fields > kTravelMaxItems) return 0;
    return travel_workspace_bytes(nx, ny, nz, n_fields);
}

extern "C" int tohip_travel_build(const void* field, size_t field_bytes, const void* occupied_or_null, const void* free_or_null,
                                  size_t grid_bytes, const tohip_occ_geom* geom, int32_t need2, const float* sources, int64_t n_sources,
                                  int64_t limit, int32_t rounds_per_check, void* cost, size_t cost_bytes, void* workspace,
                                  size_t workspace_bytes, uint8_t* seeded, int64_t* rounds_host, void* stream_) {
    TravelSet s;
    int rc = travel_set(field, field_bytes, occupied_or_null, free_or_null, grid_bytes, geom, need2, s);
    if (rc != TOHIP_OK) return rc;
    rc = travel_build_check(field, occupied_or_null, free_or_null, sources, n_sources, limit, rounds_per_check, cost, workspace);
    if (rc != TOHIP_OK) return rc;
    if (cost_bytes < travel_cost_bytes(s.g) || workspace_bytes < travel_workspace_bytes(s.g.nx, s.g.ny, s.g.nz, 1)) return TOHIP_ENOSPC;
    return travel_build(s, sources, nullptr, n_sources, 1, limit, rounds_per_check, cost, workspace, seeded, rounds_host, (hipStream_t)stream_);
}

extern "C" int tohip_travel_build_batch(const void* field, size_t field_bytes, const void* occupied_or_null, const void* free_or_null,
                                        size_t grid_bytes, const tohip_occ_geom* geom, int32_t need2, const float* sources,
                                        const int32_t* source_field, int64_t n_sources, int32_t n_fields, int64_t limit,
                                        int32_t rounds_per_check, void* cost, size_t cost_bytes, void* workspace, size_t workspace_bytes,
                                        uint8_t* seeded, int64_t* rounds_host, void* stream_) {
    TravelSet s;
    int rc = travel_set(field, field_bytes, occupied_or_null, free_or_null, grid_bytes, geom, need2, s);
    if (rc != TOHIP_OK) return rc;
    rc = travel_build_check(field, occupied_or_null, free_or_null, sources, n_sources, limit, rounds_per_check, cost, workspace);
    if (rc != TOHIP_OK) return rc;
    if (!source_field || !travel_fields_ok(n_fields) || travel_tiles(s.g.nx, s.g.ny, s.g.nz).n * n_fields > kTravelMaxItems) return TOHIP_EINVAL;
    if (cost_bytes < travel_cost_bytes(s.g) * (size_t)n_fields || workspace_bytes < travel_workspace_bytes(s.g.nx, s.g.ny, s.g.nz, n_fields))
        return TOHIP_EINVAL;
    return travel_build(s, sources, source_field, n_sources, n_fields, limit, rounds_per_check, cost, workspace, seeded, rounds_host,
                        (hipStream_t)stream_);
}

namespace {

int travel_positions(const void* cost, size_t cost_bytes, const tohip_occ_geom* geom, int64_t n_fields, const float* positions, int64_t m,
                     int64_t* cost_out, float* dist, void* stream_) {
    OccGeom g;
    const int rc = occ_check(cost, ~(size_t)0, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!travel_fields_ok(n_fields)) return TOHIP_EINVAL;
    if (cost_bytes < travel_cost_bytes(g) * (size_t)n_fields) return TOHIP_ENOSPC;
    if (!occ_count_ok(m) || !occ_count_ok(m * n_fields) || (m > 0 && (!positions || (!cost_out && !dist)))) return TOHIP_EINVAL;
    if (m == 0) return TOHIP_OK;
    k_travel_positions<<<occ_grid_blocks(m * n_fields), TO_BLOCK, 0, (hipStream_t)stream_>>>(
        (const unsigned*)cost, (long long)field_voxels(g), g, positions, m, m * n_fields, (long long*)cost_out, dist);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

int travel_paths(const void* cost, size_t cost_bytes, const void* field, size_t field_bytes, const void* occupied_or_null,
                 const void* free_or_null, size_t grid_bytes, const tohip_occ_geom* geom, int32_t need2, int64_t n_fields, const float* goals,
                 const int32_t* goal_field, int64_t n_goals, int64_t max_rows, float* rows, int64_t* counts, void* stream_,
                 const uint8_t* kappa = nullptr) {
    TravelSet s;
    const int rc = travel_set(field, field_bytes, occupied_or_null, free_or_null, grid_bytes, geom, need2, s);
    if (rc != TOHIP_OK) return rc;
    if (!cost || !travel_fields_ok(n_fields) || n_goals < 0 || n_goals > (int64_t)1 << 30 || max_rows < 1 || max_rows > (int64_t)1 << 31 ||
        (n_goals > 0 && (!goals || !rows || !counts)))
        return TOHIP_EINVAL;
    if (cost_bytes < travel_cost_bytes(s.g) * (size_t)n_fields) return TOHIP_ENOSPC;
    if (n_goals == 0) return TOHIP_OK;
    const unsigned blocks = (unsigned)((n_goals + TO_BLOCK / 64 - 1) / (TO_BLOCK / 64));
    if (kappa)
        k_travel_paths<true><<<blocks, TO_BLOCK, 0, (hipStream_t)stream_>>>(s, (const unsigned*)cost, (long long)field_voxels(s.g), goals, goal_field,
                                                                            (int)n_fields, n_goals, max_rows, rows, (long long*)counts, kappa);
    else
        k_travel_paths<false><<<blocks, TO_BLOCK, 0, (hipStream_t)stream_>>>(s, (const unsigned*)cost, (long long)field_voxels(s.g), goals, goal_field,
                                                                             (int)n_fields, n_goals, max_rows, rows, (long long*)counts, nullptr);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

}  // namespace

extern "C" int tohip_travel_positions(const void* cost, size_t cost_bytes, const tohip_occ_geom* geom, const float* positions, int64_t m,
                                      int64_t* cost_out, float* dist, void* stream_) {
    return travel_positions(cost, cost_bytes, geom, 1, positions, m, cost_out, dist, stream_);
}

extern "C" int tohip_travel_positions_batch(const void* cost, size_t cost_bytes, const tohip_occ_geom* geom, int32_t n_fields,
                                            const float* positions, int64_t m, int64_t* cost_out, float* dist, void* stream_) {
    return travel_positions(cost, cost_bytes, geom, n_fields, positions, m, cost_out, dist, stream_);
}

extern "C" int tohip_travel_paths(const void* cost, size_t cost_bytes, const void* field, size_t field_bytes, const void* occupied_or_null,
                                  const void* free_or_null, size_t grid_bytes, const tohip_occ_geom* geom, int32_t need2, const float* goals,
                                  int64_t n_goals, int64_t max_rows, float* rows, int64_t* counts, void* stream_) {
    return travel_paths(cost, cost_bytes, field, field_bytes, occupied_or_null, free_or_null, grid_bytes, geom, need2, 1, goals, nullptr,
                        n_goals, max_rows, rows, counts, stream_);
}

extern "C" int tohip_travel_paths_batch(const void* cost, size_t cost_bytes, const void* field, size_t field_bytes,
                                        const void* occupied_or_null, const void* free_or_null, size_t grid_bytes, const tohip_occ_geom* geom,
                                        int32_t need2, int32_t n_fields, const float* goals, const int32_t* goal_field, int64_t n_goals,
                                        int64_t max_rows, float* rows, int64_t* counts, void* stream_) {
    if (n_goals > 0 && !goal_field) return TOHIP_EINVAL;
    return travel_paths(cost, cost_bytes, field, field_bytes, occupied_or_null, free_or_null, grid_bytes, geom, need2, n_fields, goals,
                        goal_field, n_goals, max_rows, rows, counts, stream_);
}

// ---- weighted fields: the batch's entries with a layer kappa.  The bytes of kappa are the caller's contract (16 .. 255).

namespace {

inline size_t travel_weights_bytes(const OccGeom& g) { return field_voxels(g); }

// [a, a + na) and [b, b + nb) share a byte
inline bool travel_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" size_t tohip_travel_weights_bytes(int32_t nx, int32_t ny, int32_t nz) {
    return occ_dims_ok(nx, ny, nz) ? field_voxels(nx, ny, nz) : 0;
}

extern "C" int tohip_travel_weights_build(const void* field, size_t field_bytes, const void* occupied_or_null, const void* free_or_null,
                                          size_t grid_bytes, const tohip_occ_geom* geom, const uint8_t* lut, int32_t n_lut,
                                          int32_t unknown_add, uint8_t* out, size_t out_bytes, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    TravelSet s;
    const int rc = travel_set(field, field_bytes, occupied_or_null, free_or_null, grid_bytes, geom, 1, s);
    if (rc != TOHIP_OK) return rc;
    if (!lut || n_lut < 1 || n_lut > kFieldSentinel + 1 || unknown_add < 0 || unknown_add > 255 || !out) return TOHIP_EINVAL;
    if (out_bytes < travel_weights_bytes(s.g)) return TOHIP_ENOSPC;
    const size_t nb = travel_weights_bytes(s.g);
    if (travel_overlap(out, nb, field, nb * sizeof(uint16_t)) || travel_overlap(out, nb, lut, (size_t)n_lut) ||
        (occupied_or_null && (travel_overlap(out, nb, occupied_or_null, grid_bytes) || travel_overlap(out, nb, free_or_null, grid_bytes))))
        return TOHIP_EINVAL;
    const long long n_vox = (long long)field_voxels(s.g);
    k_travel_weights<<<occ_grid_blocks(n_vox), TO_BLOCK, 0, (hipStream_t)stream_>>>(s.field, s.occ, s.fre, s.g, lut, n_lut, (unsigned)unknown_add,
                                                                                   out, n_vox);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_travel_build_weighted(const void* field, size_t field_bytes, const void* occupied_or_null, const void* free_or_null,
                                           size_t grid_bytes, const tohip_occ_geom* geom, int32_t need2, const float* sources,
                                           const int32_t* source_field, int64_t n_sources, int32_t n_fields, int64_t limit,
                                           int32_t rounds_per_check, void* cost, size_t cost_bytes, void* workspace, size_t workspace_bytes,
                                           uint8_t* seeded, int64_t* rounds_host, const uint8_t* weights, size_t weights_bytes, void* stream_,
                                           uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    TravelSet s;
    int rc = travel_set(field, field_bytes, occupied_or_null, free_or_null, grid_bytes, geom, need2, s);
    if (rc != TOHIP_OK) return rc;
    rc = travel_build_check(field, occupied_or_null, free_or_null, sources, n_sources, limit, rounds_per_check, cost, workspace);
    if (rc != TOHIP_OK) return rc;
    if (!source_field || !travel_fields_ok(n_fields) || travel_tiles(s.g.nx, s.g.ny, s.g.nz).n * n_fields > kTravelMaxItems) return TOHIP_EINVAL;
    const size_t cb = travel_cost_bytes(s.g) * (size_t)n_fields, wb = travel_workspace_bytes(s.g.nx, s.g.ny, s.g.nz, n_fields);
    if (cost_bytes < cb || workspace_bytes < wb) return TOHIP_EINVAL;
    if (!weights || weights_bytes < travel_weights_bytes(s.g)) return TOHIP_EINVAL;
    if (travel_overlap(weights, travel_weights_bytes(s.g), cost, cb) || travel_overlap(weights, travel_weights_bytes(s.g), workspace, wb))
        return TOHIP_EINVAL;
    return travel_build(s, sources, source_field, n_sources, n_fields, limit, rounds_per_check, cost, workspace, seeded, rounds_host,
                        (hipStream_t)stream_, weights);
}

extern "C" int tohip_travel_paths_weighted(const void* cost, size_t cost_bytes, const void* field, size_t field_bytes,
                                           const void* occupied_or_null, const void* free_or_null, size_t grid_bytes,
                                           const tohip_occ_geom* geom, int32_t need2, int32_t n_fields, const float* goals,
                                           const int32_t* goal_field, int64_t n_goals, int64_t max_rows, float* rows, int64_t* counts,
                                           const uint8_t* weights, size_t weights_bytes, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    if (n_goals > 0 && !goal_field) return TOHIP_EINVAL;
    OccGeom g;
    const int rc = field_check(field, field_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!weights || weights_bytes < travel_weights_bytes(g)) return TOHIP_EINVAL;
    return travel_paths(cost, cost_bytes, field, field_bytes, occupied_or_null, free_or_null, grid_bytes, geom, need2, n_fields, goals,
                        goal_field, n_goals, max_rows, rows, counts, stream_, weights);
}

extern "C" int tohip_assign_greedy(const int64_t* cost, int32_t n_rows, int32_t n_cols, int64_t ld, int64_t min_cost, int32_t* col_of_row,
                                   int32_t* row_of_col, void* stream_) {
    if (!cost || !col_of_row || !row_of_col || n_rows < 1 || n_rows > kAssignMaxRows || n_cols < 1 || n_cols > kAssignMaxCols ||
        ld < n_cols || ld > (int64_t)1 << 40 || min_cost < 0)
        return TOHIP_EINVAL;
    k_assign_greedy<<<1, TO_BLOCK, 0, (hipStream_t)stream_>>>((const long long*)cost, n_rows, n_cols, (long long)ld, (long long)min_cost,
                                                             col_of_row, row_of_col);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_view_volume_pick_travel(const int64_t* gains, const int64_t* cost, int64_t weight, int32_t* taken, int64_t n_views,
                                             int64_t min_gain, int32_t round, int32_t* order, int64_t* picked_gain, int32_t* stop,
                                             void* stream_) {
    if (!gains || !cost || !taken || !order || !picked_gain || !stop || n_views < 1 || n_views > (int64_t)0x7fffffff || min_gain < 1 ||
        round < 0 || weight < 0 || weight > kTravelMaxLimit)
        return TOHIP_EINVAL;
    k_view_volume_pick_travel<<<1, TO_BLOCK, 0, (hipStream_t)stream_>>>((const long long*)gains, (const long long*)cost, (long long)weight, taken,
                                                                        (long long)n_views, (long long)min_gain, round, order,
                                                                        (long long*)picked_gain, stop);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
