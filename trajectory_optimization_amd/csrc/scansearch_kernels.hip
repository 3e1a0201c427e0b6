// scansearch_kernels.hip — relocalisation: exact branch-and-bound scan matching over wide windows ("Relocalisation"),
// for gfx950.  Included right after scanmatch_kernels.hip: the pose, the voxel of a point, the score table and the key of the best
// candidate are scan matching's (scan_voxel, ScanBest's rule), the geometry and the brick layout the map layer's (OccGeom, occ_word,
// occ_bit, evid_check, evid_brick, evid_size).
//
// LEVEL TABLES.  T_0 is the score table.  T_h (h = 1 .. 6) has its size, header and brick order and holds, for a voxel inside dims,
// the maximum of T_0' over the 2^h x 2^h block of voxels that starts there in x and y (T_0': T_0 continued by 128 + unknown_value
// outside dims); pad voxels hold 128 + unknown_value.  T_h follows from T_{h-1} by a four-way maximum at stride 2^{h-1}.
// LOOKUP.  With u = 128 + unknown_value and b = 2^h - 1, B_h(x, y, z) = u where z is outside [0, nz) or x outside [-b, nx) or y outside
// [-b, ny); otherwise T_h(max(x, 0), max(y, 0), z), raised to u where x < 0 or y < 0: an upper bound of T_0' over the block [x, x + 2^h)
// x [y, y + 2^h) x {z}, and T_0' itself for h = 0.
// NODE.  (k, sx, sy, sz) at level h: rotation k, dz = sz, dx in [sx, sx + 2^h) and dy likewise, cut to the window.  Its BOUND: the sum
// over the points in range under rotation k of B_h(voxel_k(p) + (sx, sy, sz)), less 128 x their number: the score at level 0.
//
//   k_reloc_level     T_{h-1} -> T_h.  One lane per brick word: the brick and its up to three neighbours at stride 2^{h-1} in x and y
//                     (whole bricks from h = 3 on, a byte funnel below) as 16-byte loads, a bytewise maximum, two 16-byte stores.  A
//                     brick beyond the array gives u from a predicate.  No atomics.
//   k_reloc_count     per rotation, how many nodes the next list holds: the children of every node whose bound is not below the
//                     incumbent (or, for a list of explicit nodes, the nodes themselves).  A histogram per block in LDS, one integer
//                     atomic per block and rotation.
//   k_reloc_offsets   one block: the rotations' offsets in the next list (it is grouped by rotation), its 256-node chunks, the capacity
//                     check — a list that does not fit sets the status, and every later kernel returns at once — and how many shares
//                     of the scan's tiles each chunk is spread over.
//   k_reloc_scatter   writes the next list: every kept node's children (sx, sy) + {0, 2^{h-1}}^2 that start inside the window, at a
//                     slot claimed from the rotation's cursor, bound 0.
//   k_reloc_bound     the hot path.  A block walks work items (chunk, share): the chunk's 256 nodes belong to one rotation, a lane owns
//                     one node, and for each 256-point tile of its share the block transforms the points once, packs those in range
//                     into LDS, and every lane sums B_h over them (LDS broadcast reads, one byte load per lookup, the "outside" cases
//                     are predicates: byte 0 of the table is loaded in their place).  One integer atomic per node and share.
//   k_reloc_pick      one block: the list's best node (largest bound, then lowest (k, sz, sy, sx)) -> the state's descent node.
//   k_reloc_step      one block, one level of the greedy descent: the up to four children's bounds over all points, the best child by
//                     the same key -> the descent node; behind level 0 the incumbent becomes max(incumbent, the leaf's score).
//   k_reloc_final     one block over the level-0 list: the maximum of the key (score, smaller |s|^2, lower flat index — an int64) and
//                     the number of nodes that share the best score -> the record.
//
// The counts live in device memory: launches are sized by the capacity and stride over the counts, nothing is read back between
// levels.  No float atomics, no process-wide state; every argument check returns before anything is enqueued.
#include <climits>

namespace {

constexpr int kRelocMaxLevels = 6;
constexpr int kRelocMaxWxy = kOccMaxDim;
constexpr long long kRelocMaxCapacity = 1ll << 24;
constexpr int kRelocRecord = 11 + kRelocMaxLevels + 1;   // int64 words of the record
constexpr int kRelocItems = 4096;          // work items (chunk, share) a bound launch aims at
constexpr int kRelocBlock = 1024;          // of the one-block kernels
constexpr int kRelocShiftClamp = 8192;     // an explicit node's shift beyond it: every voxel is outside either way

struct RelocPick {
    int bound, k, sz, sy, sx;   // k < 0: none
};

// larger bound first, then the lowest (k, sz, sy, sx)
__device__ __forceinline__ bool reloc_before(const RelocPick& a, const RelocPick& b) {
    if (b.k < 0) return true;
    if (a.k < 0) return false;
    if (a.bound != b.bound) return a.bound > b.bound;
    if (a.k != b.k) return a.k < b.k;
    if (a.sz != b.sz) return a.sz < b.sz;
    if (a.sy != b.sy) return a.sy < b.sy;
    return a.sx < b.sx;
}

struct RelocState {
    int status;        // 0, or 1: a list did not fit (the record says which)
    int total, prev;   // nodes of the current list, of the one before
    int n_chunks, ysplit;
    int incumbent;
    int K;
    int pad_;
    long long evaluated;
    int cnt[kScanMaxK], off[kScanMaxK], cursor[kScanMaxK], chunk[kScanMaxK];
    RelocPick at;      // the descent's node
};

struct RelocWin {
    int wx, wy, wz;
    long long nxw, nyw, nzw;
};

inline size_t reloc_align(size_t v) { return (v + 255u) & ~(size_t)255u; }

// B_h at (x, y, z): T the level's bytes behind its header
__device__ __forceinline__ int reloc_lookup(const unsigned char* __restrict__ T, const OccGeom& g, int b, int u, int x, int y, int z) {
    const bool in = (unsigned)z < (unsigned)g.nz && x >= -b && x < g.nx && y >= -b && y < g.ny;
    const int xc = max(x, 0), yc = max(y, 0);
    const long long at = in ? 32ll * occ_word(g, xc, yc, z) + occ_bit(xc, yc, z) : 0ll;   // (outside: byte 0 is loaded and not used)
    int c = (int)T[at];
    if (x < 0 || y < 0) c = max(c, u);
    return in ? c : u;
}

__device__ __forceinline__ unsigned reloc_max4(unsigned a, unsigned b) {
    unsigned r = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) r |= max(a & (0xFFu << (8 * j)), b & (0xFFu << (8 * j)));
    return r;
}

struct RelocBrick {
    unsigned v[8];   // dword (y & 3) | (z & 1) << 2: the four x of a row
};

__device__ __forceinline__ RelocBrick reloc_brick(const uint4* __restrict__ T, const OccGeom& g, int bx, int by, int bz, unsigned u4) {
    const bool in = bx < g.nbx && by < g.nby;
    const long long w = in ? ((long long)bz * g.nby + by) * g.nbx + bx : 0ll;   // (beyond the array: word 0 is loaded and not used)
    const uint4 lo = T[2 * w], hi = T[2 * w + 1];
    RelocBrick r{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
    if (!in) {
#pragma unroll
        for (int i = 0; i < 8; ++i) r.v[i] = u4;
    }
    return r;
}

// S: the stride 2^{h-1} where it is 1 or 2 (neighbours inside the brick and the next one), 0: a multiple of 4 (q bricks away)
template <int S>
__global__ void __launch_bounds__(TO_BLOCK)
k_reloc_level(const uint4* __restrict__ src, uint4* __restrict__ dst, OccGeom g, long long n_words, int q, unsigned u4) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < n_words; w += stride) {
        int bx, by, bz;
        evid_brick(g, (unsigned)w, bx, by, bz);
        const RelocBrick a = reloc_brick(src, g, bx, by, bz, u4), ax = reloc_brick(src, g, bx + q, by, bz, u4),
                         ay = reloc_brick(src, g, bx, by + q, bz, u4), axy = reloc_brick(src, g, bx + q, by + q, bz, u4);
        unsigned out[8];
        if (S == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) out[i] = reloc_max4(reloc_max4(a.v[i], ax.v[i]), reloc_max4(ay.v[i], axy.v[i]));
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int y = i & 3, zb = i & 4, y2 = y + S;
                // the row at y + S: this brick's or the next one's along y
                const unsigned r0 = y2 < 4 ? a.v[y2 | zb] : ay.v[(y2 - 4) | zb], r1 = y2 < 4 ? ax.v[y2 | zb] : axy.v[(y2 - 4) | zb];
                const unsigned here = a.v[i], here_x = (unsigned)((((unsigned long long)ax.v[i] << 32) | here) >> (8 * S));
                const unsigned up = r0, up_x = (unsigned)((((unsigned long long)r1 << 32) | r0) >> (8 * S));
                out[i] = reloc_max4(reloc_max4(here, here_x), reloc_max4(up, up_x));
            }
        }
        dst[2 * w] = make_uint4(out[0], out[1], out[2], out[3]);
        dst[2 * w + 1] = make_uint4(out[4], out[5], out[6], out[7]);
    }
}

// the children a node of the list gets: 0 where its bound is below the incumbent, else those that start inside the window
__device__ __forceinline__ int reloc_children(const int4& nd, int bound, int incumbent, const RelocWin& win, int half) {
    if (bound < incumbent) return 0;
    return (1 + (nd.y + half <= win.wx ? 1 : 0)) * (1 + (nd.z + half <= win.wy ? 1 : 0));
}

__global__ void __launch_bounds__(TO_BLOCK)
k_reloc_count(RelocState* __restrict__ st, const int4* __restrict__ nodes, const int* __restrict__ bounds, RelocWin win, int half, int K,
              long long m_explicit) {
    __shared__ int s_cnt[kScanMaxK];
    if (st->status != 0) return;
    const int t = threadIdx.x;
    s_cnt[t] = 0;
    __syncthreads();
    const long long total = m_explicit >= 0 ? m_explicit : (long long)st->total;
    const int incumbent = st->incumbent;
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + t; i < total; i += stride) {
        const int4 nd = nodes[i];
        int c;
        if (m_explicit >= 0)
            c = (unsigned)nd.x < (unsigned)K ? 1 : 0;
        else
            c = reloc_children(nd, bounds[i], incumbent, win, half);
        if (c != 0) atomicAdd(&s_cnt[nd.x], c);
    }
    __syncthreads();
    if (s_cnt[t] != 0) __hip_atomic_fetch_add(&st->cnt[t], s_cnt[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kScanMaxK)
k_reloc_offsets(RelocState* __restrict__ st, long long* __restrict__ record, int level, int H, int K, long long capacity, long long n_tiles) {
    __shared__ int s_a[kScanMaxK], s_b[kScanMaxK];
    if (st->status != 0) return;
    const int t = threadIdx.x;
    const int c = st->cnt[t], ch = (c + TO_BLOCK - 1) / TO_BLOCK;
    s_a[t] = c, s_b[t] = ch;
    __syncthreads();
    for (int d = 1; d < kScanMaxK; d <<= 1) {
        const int a = t >= d ? s_a[t - d] : 0, b = t >= d ? s_b[t - d] : 0;
        __syncthreads();
        s_a[t] += a, s_b[t] += b;
        __syncthreads();
    }
    st->off[t] = s_a[t] - c, st->cursor[t] = s_a[t] - c, st->chunk[t] = s_b[t] - ch;
    if (t == kScanMaxK - 1) {
        const int total = s_a[t], n_chunks = s_b[t];
        st->prev = st->total;
        st->total = total, st->n_chunks = n_chunks, st->K = K;
        long long y = n_chunks > 0 ? (kRelocItems + n_chunks - 1) / n_chunks : 1;
        st->ysplit = (int)(y < n_tiles ? y : n_tiles);
        if ((long long)total > capacity) {
            st->status = 1;
            if (record) {
                record[0] = -1;
                record[7] = ((long long)total << 3) | (long long)(level + 1);
                record[8] = st->incumbent, record[9] = st->evaluated, record[10] = H, record[11 + level] = total;
            }
        } else {
            st->evaluated += total;
        }
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_reloc_scatter(RelocState* __restrict__ st, const int4* __restrict__ nodes, const int* __restrict__ bounds, int4* __restrict__ out,
                int* __restrict__ out_bounds, int* __restrict__ src, RelocWin win, int half, int K, long long m_explicit) {
    if (st->status != 0) return;
    const long long total = m_explicit >= 0 ? m_explicit : (long long)st->prev;
    const int incumbent = st->incumbent;
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < total; i += stride) {
        const int4 nd = nodes[i];
        if (m_explicit >= 0) {
            if ((unsigned)nd.x >= (unsigned)K) {
                out_bounds[i] = INT_MIN;   // (no such rotation)
                continue;
            }
            const int slot = __hip_atomic_fetch_add(&st->cursor[nd.x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            out[slot] = make_int4(nd.x, min(max(nd.y, -kRelocShiftClamp), kRelocShiftClamp), min(max(nd.z, -kRelocShiftClamp), kRelocShiftClamp),
                                  min(max(nd.w, -kRelocShiftClamp), kRelocShiftClamp));
            src[slot] = (int)i;
            out_bounds[i] = 0;
            continue;
        }
        const int c = reloc_children(nd, bounds[i], incumbent, win, half);
        if (c == 0) continue;
        int slot = __hip_atomic_fetch_add(&st->cursor[nd.x], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int j = 0; j < 4; ++j) {
            const int sx = nd.y + (j & 1) * half, sy = nd.z + (j >> 1) * half;
            if (sx > win.wx || sy > win.wy) continue;
            out[slot] = make_int4(nd.x, sx, sy, nd.w);
            out_bounds[slot] = 0;
            ++slot;
        }
    }
}

// the top level's list, grouped by rotation: k slowest, then sz, sy, sx
__global__ void __launch_bounds__(TO_BLOCK)
k_reloc_top(RelocState* __restrict__ st, long long* __restrict__ record, int4* __restrict__ nodes, int* __restrict__ bounds, RelocWin win,
            int step, int ntx, int nty, int K, int H) {
    const int per_k = (int)win.nzw * nty * ntx;
    const long long total = (long long)K * per_k;
    if (blockIdx.x == 0) {
        st->cnt[threadIdx.x] = (int)threadIdx.x < K ? per_k : 0;
        if (threadIdx.x == 0) st->incumbent = INT_MIN, record[8] = INT_MIN, record[10] = H;
    }
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < total; i += stride) {
        const int k = (int)(i / per_k), r = (int)(i - (long long)k * per_k);
        const int zi = r / (nty * ntx), r2 = r - zi * nty * ntx, yi = r2 / ntx, xi = r2 - yi * ntx;
        nodes[i] = make_int4(k, -win.wx + xi * step, -win.wy + yi * step, zi - win.wz);
        bounds[i] = 0;
    }
}

// the top level alone is more than the capacity: the record says so, nothing else runs
__global__ void k_reloc_fail(long long* __restrict__ record, long long total, int H) {
    record[0] = -1;
    record[7] = (total << 3) | (long long)(H + 1);
    record[8] = INT_MIN, record[10] = H, record[11 + H] = total;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_reloc_bound(const unsigned char* __restrict__ T, OccGeom g, int b, int u, const float* __restrict__ pts, long long n,
              const float* __restrict__ poses, const RelocState* __restrict__ st, const int4* __restrict__ nodes, const int* __restrict__ src,
              int* __restrict__ bounds) {
    __shared__ int s_pts[3 * TO_BLOCK];   // the tile's points in range: base voxels, packed
    __shared__ int s_n;
    if (st->status != 0) return;
    const int t = threadIdx.x;
    const int ysplit = st->ysplit, K = st->K;
    const long long items = (long long)st->n_chunks * ysplit;
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        const int chunk = (int)(w / ysplit), part = (int)(w - (long long)chunk * ysplit);
        int k = 0, hi = K;   // the last rotation whose first chunk is not behind this one
        while (hi - k > 1) {
            const int mid = (k + hi) >> 1;
            if (st->chunk[mid] <= chunk) k = mid; else hi = mid;
        }
        const int i = st->off[k] + TO_BLOCK * (chunk - st->chunk[k]) + t;
        const bool have = i < st->off[k] + st->cnt[k];
        const int4 nd = have ? nodes[i] : make_int4(0, 0, 0, 0);
        const float* P = poses + 12 * (long long)k;
        int acc = 0, used = 0;
        for (long long tile = part; tile < n_tiles; tile += ysplit) {
            __syncthreads();   // (the tile before is read to its end)
            if (t == 0) s_n = 0;
            __syncthreads();
            {
                const long long p = tile * TO_BLOCK + t;
                int x, y, z;
                if (p < n && scan_voxel(g, P, pts + 3 * p, x, y, z)) {
                    const int slot = atomicAdd(&s_n, 1);
                    s_pts[3 * slot] = x, s_pts[3 * slot + 1] = y, s_pts[3 * slot + 2] = z;
                }
            }
            __syncthreads();
            const int nv = s_n;
            used += nv;
            if (have) {
#pragma unroll 4
                for (int p = 0; p < nv; ++p)
                    acc += reloc_lookup(T, g, b, u, s_pts[3 * p] + nd.y, s_pts[3 * p + 1] + nd.z, s_pts[3 * p + 2] + nd.w);
            }
        }
        const int v = acc - 128 * used;
        if (have && v != 0) __hip_atomic_fetch_add(bounds + (src ? src[i] : i), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the points in range under each rotation
__global__ void __launch_bounds__(TO_BLOCK)
k_reloc_used(OccGeom g, const float* __restrict__ pts, long long n, const float* __restrict__ poses, int* __restrict__ used) {
    const int k = blockIdx.y;
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    int c = 0;
    for (long long base = (long long)blockIdx.x * TO_BLOCK; base < n; base += stride) {
        const long long p = base + threadIdx.x;
        int x, y, z;
        if (p < n && scan_voxel(g, poses + 12 * (long long)k, pts + 3 * p, x, y, z)) ++c;
    }
    scan_count(used + k, c);
}

// the list's best node -> the state's descent node; the list's count -> the record; the counts of the next list start from zero
__global__ void __launch_bounds__(kRelocBlock)
k_reloc_pick(RelocState* __restrict__ st, long long* __restrict__ record, const int4* __restrict__ nodes, const int* __restrict__ bounds, int h) {
    __shared__ RelocPick s_pick[kRelocBlock];
    if (st->status != 0) return;
    const int t = threadIdx.x;
    if (t < kScanMaxK) st->cnt[t] = 0;   // (the list's bounds are complete)
    const int total = st->total;
    RelocPick mine{0, -1, 0, 0, 0};
    for (int i = t; i < total; i += kRelocBlock) {
        const int4 nd = nodes[i];
        const RelocPick c{bounds[i], nd.x, nd.w, nd.z, nd.y};
        if (reloc_before(c, mine)) mine = c;
    }
    s_pick[t] = mine;
    __syncthreads();
    for (int half = kRelocBlock / 2; half > 0; half >>= 1) {
        if (t < half && reloc_before(s_pick[t + half], s_pick[t])) s_pick[t] = s_pick[t + half];
        __syncthreads();
    }
    if (t == 0) {
        st->at = s_pick[0];
        record[11 + h] = total;
    }
}

// one step of the descent: the up to four children of the state's descent node at the level of T (half = 2^level), their bounds over
// all points, the best of them -> the descent node; last: the level is 0 and the incumbent takes the leaf's score
__global__ void __launch_bounds__(kRelocBlock)
k_reloc_step(RelocState* __restrict__ st, const unsigned char* __restrict__ T, OccGeom g, int b, int u, const float* __restrict__ pts,
             long long n, const float* __restrict__ poses, RelocWin win, int half, int last) {
    __shared__ int s_sum[kRelocBlock / 64][5];
    if (st->status != 0) return;
    const int t = threadIdx.x;
    RelocPick at;   // (written by the launch before this one: read from memory, field by field)
    at.bound = __hip_atomic_load(&st->at.bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    at.k = __hip_atomic_load(&st->at.k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    at.sz = __hip_atomic_load(&st->at.sz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    at.sy = __hip_atomic_load(&st->at.sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    at.sx = __hip_atomic_load(&st->at.sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (at.k < 0) return;   // (an empty list: there is none, the best node's line always survives)
    const float* P = poses + 12 * (long long)at.k;
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0, used = 0;
    for (long long p = t; p < n; p += kRelocBlock) {
        int x, y, z;
        if (!scan_voxel(g, P, pts + 3 * p, x, y, z)) continue;
        ++used;
        x += at.sx, y += at.sy, z += at.sz;
        a0 += reloc_lookup(T, g, b, u, x, y, z);
        a1 += reloc_lookup(T, g, b, u, x + half, y, z);
        a2 += reloc_lookup(T, g, b, u, x, y + half, z);
        a3 += reloc_lookup(T, g, b, u, x + half, y + half, z);
    }
    for (int sh = 32; sh > 0; sh >>= 1) {
        a0 += __shfl_xor(a0, sh), a1 += __shfl_xor(a1, sh), a2 += __shfl_xor(a2, sh), a3 += __shfl_xor(a3, sh), used += __shfl_xor(used, sh);
    }
    if ((t & 63) == 0) {
        int* row = s_sum[t >> 6];
        row[0] = a0, row[1] = a1, row[2] = a2, row[3] = a3, row[4] = used;
    }
    __syncthreads();   // (every lane has read the descent node by now)
    if (t != 0) return;
    int t0 = 0, t1 = 0, t2 = 0, t3 = 0, n_used = 0;
    for (int wv = 0; wv < kRelocBlock / 64; ++wv) {
        const int* row = s_sum[wv];
        t0 += row[0], t1 += row[1], t2 += row[2], t3 += row[3], n_used += row[4];
    }
    // the children in the order of (sy, sx): a later one wins only with a larger bound
    const bool wide = at.sx + half <= win.wx, tall = at.sy + half <= win.wy;
    const int evals = (wide ? 2 : 1) * (tall ? 2 : 1);
    RelocPick best{t0 - 128 * n_used, at.k, at.sz, at.sy, at.sx};
    if (wide && t1 - 128 * n_used > best.bound) best = RelocPick{t1 - 128 * n_used, at.k, at.sz, at.sy, at.sx + half};
    if (tall && t2 - 128 * n_used > best.bound) best = RelocPick{t2 - 128 * n_used, at.k, at.sz, at.sy + half, at.sx};
    if (wide && tall && t3 - 128 * n_used > best.bound) best = RelocPick{t3 - 128 * n_used, at.k, at.sz, at.sy + half, at.sx + half};
    st->at = best;
    st->evaluated += evals;
    if (last) st->incumbent = max(st->incumbent, best.bound);
}

struct RelocBest {
    int score, d2;
    long long idx;   // -1: none
    long long ties;
};

__device__ __forceinline__ RelocBest reloc_better(const RelocBest& a, const RelocBest& b) {
    if (a.idx < 0) return b;
    if (b.idx < 0) return a;
    RelocBest r;
    if (a.score != b.score) {
        r = a.score > b.score ? a : b;
    } else {
        const bool first = a.d2 != b.d2 ? a.d2 < b.d2 : a.idx < b.idx;
        r = first ? a : b;
        r.ties = a.ties + b.ties;
    }
    return r;
}

__global__ void __launch_bounds__(kRelocBlock)
k_reloc_final(const RelocState* __restrict__ st, long long* __restrict__ record, const int4* __restrict__ nodes, const int* __restrict__ bounds,
              RelocWin win, int H) {
    __shared__ RelocBest s_best[kRelocBlock];
    if (st->status != 0) return;
    const int t = threadIdx.x, total = st->total;
    RelocBest mine{0, 0, -1, 0};
    for (int i = t; i < total; i += kRelocBlock) {
        const int sc = bounds[i];
        if (mine.idx >= 0 && sc < mine.score) continue;
        const int4 nd = nodes[i];
        const long long flat = (((long long)nd.x * win.nzw + (nd.w + win.wz)) * win.nyw + (nd.z + win.wy)) * win.nxw + (nd.y + win.wx);
        mine = reloc_better(mine, RelocBest{sc, nd.y * nd.y + nd.z * nd.z + nd.w * nd.w, flat, 1});
    }
    s_best[t] = mine;
    __syncthreads();
    for (int half = kRelocBlock / 2; half > 0; half >>= 1) {
        if (t < half) s_best[t] = reloc_better(s_best[t], s_best[t + half]);
        __syncthreads();
    }
    if (t == 0) {
        const RelocBest b = s_best[0];
        const long long S2 = win.nxw * win.nyw, S = S2 * win.nzw;
        const long long k = b.idx / S, s = b.idx - k * S, dzi = s / S2, rem = s - dzi * S2, dyi = rem / win.nxw;
        record[0] = b.idx, record[1] = k, record[2] = rem - dyi * win.nxw - win.wx, record[3] = dyi - win.wy, record[4] = dzi - win.wz;
        record[5] = b.score, record[6] = b.ties, record[7] = 0, record[8] = st->incumbent, record[9] = st->evaluated, record[10] = H;
        record[11] = total;
    }
}

inline bool reloc_window_ok(int wx, int wy, int wz) {
    return wx >= 0 && wx <= kRelocMaxWxy && wy >= 0 && wy <= kRelocMaxWxy && wz >= 0 && wz <= kScanMaxWz;
}
inline RelocWin reloc_window(int wx, int wy, int wz) { return RelocWin{wx, wy, wz, 2ll * wx + 1, 2ll * wy + 1, 2ll * wz + 1}; }

// the workspace: the state, two node lists and their bounds (a list of explicit nodes uses the first list and the second's bounds
// as the nodes' source rows)
struct RelocSpace {
    RelocState* st;
    int4* nodes[2];
    int* bounds[2];
};
inline size_t reloc_space_bytes(long long capacity) {
    return reloc_align(sizeof(RelocState)) + 2 * reloc_align((size_t)capacity * sizeof(int4)) + 2 * reloc_align((size_t)capacity * sizeof(int));
}
inline RelocSpace reloc_space(void* workspace, long long capacity) {
    char* p = (char*)workspace;
    RelocSpace s;
    s.st = (RelocState*)p, p += reloc_align(sizeof(RelocState));
    for (int i = 0; i < 2; ++i) s.nodes[i] = (int4*)p, p += reloc_align((size_t)capacity * sizeof(int4));
    for (int i = 0; i < 2; ++i) s.bounds[i] = (int*)p, p += reloc_align((size_t)capacity * sizeof(int));
    return s;
}

inline const unsigned char* reloc_level_bytes(const void* table, const void* levels, size_t level_bytes, int h) {
    return (h == 0 ? (const unsigned char*)table : (const unsigned char*)levels + (size_t)(h - 1) * level_bytes) + kEvidHdr;
}

}  // namespace

extern "C" size_t tohip_reloc_workspace_bytes(int64_t capacity) {
    return capacity >= 1 && capacity <= kRelocMaxCapacity ? reloc_space_bytes(capacity) : 0;
}

extern "C" int tohip_reloc_levels(const void* table, size_t table_bytes, const tohip_occ_geom* geom, int32_t unknown_value, int32_t h,
                                  void* levels, size_t levels_bytes, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    int rc = evid_check(table, table_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!scan_value_ok(0, unknown_value) || h < 1 || h > kRelocMaxLevels || !levels || !scan_aligned(levels, 16)) return TOHIP_EINVAL;
    const size_t one = evid_size(g.nx, g.ny, g.nz);
    const char *a = (const char*)table, *b = (const char*)levels;
    if (a < b + (size_t)h * one && b < a + one) return TOHIP_EINVAL;   // (the levels must not overlap the table)
    if (levels_bytes < (size_t)h * one) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const long long n_words = (long long)occ_words(g.nx, g.ny, g.nz);
    const unsigned u4 = (unsigned)(128 + unknown_value) * 0x01010101u;
    for (int lev = 1; lev <= h; ++lev) {
        const char* src = lev == 1 ? (const char*)table : (const char*)levels + (size_t)(lev - 2) * one;
        char* dst = (char*)levels + (size_t)(lev - 1) * one;
        const hipError_t e = hipMemsetAsync(dst, 0, kEvidHdr, st);
        if (e != hipSuccess) return (int)e;
        const uint4* s4 = reinterpret_cast<const uint4*>(src + kEvidHdr);
        uint4* d4 = reinterpret_cast<uint4*>(dst + kEvidHdr);
        const int stride = 1 << (lev - 1), blocks = occ_grid_blocks(n_words);
        if (stride == 1) k_reloc_level<1><<<blocks, TO_BLOCK, 0, st>>>(s4, d4, g, n_words, 1, u4);
        else if (stride == 2) k_reloc_level<2><<<blocks, TO_BLOCK, 0, st>>>(s4, d4, g, n_words, 1, u4);
        else k_reloc_level<0><<<blocks, TO_BLOCK, 0, st>>>(s4, d4, g, n_words, stride / 4, u4);
        TO_HIP_CHECK_LAUNCH();
    }
    return TOHIP_OK;
}

extern "C" int tohip_reloc_bounds(const void* table, size_t table_bytes, const tohip_occ_geom* geom, int32_t unknown_value, int32_t level,
                                  const float* points, int64_t n, const float* poses, int64_t k, const int32_t* nodes, int64_t m,
                                  int32_t* bounds, int32_t* used, void* workspace, size_t workspace_bytes, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = evid_check(table, table_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!scan_value_ok(0, unknown_value) || level < 0 || level > kRelocMaxLevels || n < 1 || n > kScanMaxPoints || k < 1 || k > kScanMaxK ||
        m < 1 || m > kScanMaxCandidates || !points || !poses || !nodes || !bounds || !used || !workspace)
        return TOHIP_EINVAL;
    const void* bufs[7] = {bounds, used, workspace, points, poses, nodes, table};
    for (int i = 0; i < 7; ++i) {
        if (!scan_aligned(bufs[i], i == 2 || i == 5 ? 16 : 4)) return TOHIP_EINVAL;
        for (int j = 0; j < 3; ++j)   // no output is an input or another output
            if (i > j && bufs[i] == bufs[j]) return TOHIP_EINVAL;
    }
    if (workspace_bytes < reloc_space_bytes(m)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const RelocSpace sp = reloc_space(workspace, m);
    hipError_t e = hipMemsetAsync(sp.st, 0, sizeof(RelocState), st);
    if (e == hipSuccess) e = hipMemsetAsync(used, 0, (size_t)k * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const RelocWin win = reloc_window(0, 0, 0);
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    const int blocks = occ_grid_blocks(m);
    const int4* in = reinterpret_cast<const int4*>(nodes);
    k_reloc_count<<<blocks, TO_BLOCK, 0, st>>>(sp.st, in, nullptr, win, 0, (int)k, m);
    TO_HIP_CHECK_LAUNCH();
    k_reloc_offsets<<<1, kScanMaxK, 0, st>>>(sp.st, nullptr, level, level, (int)k, m, n_tiles);
    TO_HIP_CHECK_LAUNCH();
    k_reloc_scatter<<<blocks, TO_BLOCK, 0, st>>>(sp.st, in, nullptr, sp.nodes[0], bounds, sp.bounds[1], win, 0, (int)k, m);
    TO_HIP_CHECK_LAUNCH();
    const long long per = (kScanBlocks + k - 1) / k;
    k_reloc_used<<<dim3((unsigned)(per < n_tiles ? per : n_tiles), (unsigned)k), TO_BLOCK, 0, st>>>(g, points, n, poses, used);
    TO_HIP_CHECK_LAUNCH();
    k_reloc_bound<<<kScanBlocks, TO_BLOCK, 0, st>>>((const unsigned char*)table + kEvidHdr, g, (1 << level) - 1, 128 + unknown_value, points, n,
                                                    poses, sp.st, sp.nodes[0], sp.bounds[1], bounds);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_reloc_search(const void* table, size_t table_bytes, const void* levels_or_null, size_t levels_bytes,
                                  const tohip_occ_geom* geom, int32_t unknown_value, int32_t h, const float* points, int64_t n,
                                  const float* poses, int64_t k, int32_t wx, int32_t wy, int32_t wz, int64_t capacity, int64_t* record,
                                  void* workspace, size_t workspace_bytes, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = evid_check(table, table_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!scan_value_ok(0, unknown_value) || h < 0 || h > kRelocMaxLevels || !reloc_window_ok(wx, wy, wz) || n < 1 || n > kScanMaxPoints ||
        k < 1 || k > kScanMaxK || capacity < 1 || capacity > kRelocMaxCapacity || !points || !poses || !record || !workspace ||
        (h > 0 && (!levels_or_null || !scan_aligned(levels_or_null, 16))))
        return TOHIP_EINVAL;
    const void* bufs[6] = {record, workspace, points, poses, table, levels_or_null};
    for (int i = 0; i < 6; ++i) {
        if (!scan_aligned(bufs[i], i == 0 ? 8 : (i == 1 ? 16 : 4))) return TOHIP_EINVAL;
        for (int j = 0; j < 2; ++j)
            if (i > j && bufs[i] == bufs[j]) return TOHIP_EINVAL;
    }
    const size_t one = evid_size(g.nx, g.ny, g.nz);
    if (levels_bytes < (size_t)h * one || workspace_bytes < reloc_space_bytes(capacity)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const RelocSpace sp = reloc_space(workspace, capacity);
    hipError_t e = hipMemsetAsync(sp.st, 0, sizeof(RelocState), st);
    if (e == hipSuccess) e = hipMemsetAsync(record, 0, kRelocRecord * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    const RelocWin win = reloc_window(wx, wy, wz);
    const int step = 1 << h, ntx = (int)((win.nxw + step - 1) / step), nty = (int)((win.nyw + step - 1) / step);
    const long long top = (long long)k * win.nzw * nty * ntx;
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    const int u = 128 + unknown_value;
    long long* rec = reinterpret_cast<long long*>(record);
    if (top > capacity) {
        k_reloc_fail<<<1, 1, 0, st>>>(rec, top, h);
        TO_HIP_CHECK_LAUNCH();
        return TOHIP_OK;
    }
    const int list_blocks = occ_grid_blocks(capacity);
    k_reloc_top<<<occ_grid_blocks(top), TO_BLOCK, 0, st>>>(sp.st, rec, sp.nodes[0], sp.bounds[0], win, step, ntx, nty, (int)k, h);
    TO_HIP_CHECK_LAUNCH();
    k_reloc_offsets<<<1, kScanMaxK, 0, st>>>(sp.st, rec, h, h, (int)k, capacity, n_tiles);
    TO_HIP_CHECK_LAUNCH();
    k_reloc_bound<<<kScanBlocks, TO_BLOCK, 0, st>>>(reloc_level_bytes(table, levels_or_null, one, h), g, step - 1, u, points, n, poses, sp.st,
                                                    sp.nodes[0], nullptr, sp.bounds[0]);
    TO_HIP_CHECK_LAUNCH();
    int cur = 0;
    for (int lev = h; lev >= 1; --lev) {
        const int half = 1 << (lev - 1);
        k_reloc_pick<<<1, kRelocBlock, 0, st>>>(sp.st, rec, sp.nodes[cur], sp.bounds[cur], lev);
        TO_HIP_CHECK_LAUNCH();
        for (int d = lev - 1; d >= 0; --d) {
            k_reloc_step<<<1, kRelocBlock, 0, st>>>(sp.st, reloc_level_bytes(table, levels_or_null, one, d), g, (1 << d) - 1, u, points, n, poses, win,
                                                    1 << d, d == 0 ? 1 : 0);
            TO_HIP_CHECK_LAUNCH();
        }
        k_reloc_count<<<list_blocks, TO_BLOCK, 0, st>>>(sp.st, sp.nodes[cur], sp.bounds[cur], win, half, (int)k, -1);
        TO_HIP_CHECK_LAUNCH();
        k_reloc_offsets<<<1, kScanMaxK, 0, st>>>(sp.st, rec, lev - 1, h, (int)k, capacity, n_tiles);
        TO_HIP_CHECK_LAUNCH();
        k_reloc_scatter<<<list_blocks, TO_BLOCK, 0, st>>>(sp.st, sp.nodes[cur], sp.bounds[cur], sp.nodes[cur ^ 1], sp.bounds[cur ^ 1], nullptr, win,
                                                          half, (int)k, -1);
        TO_HIP_CHECK_LAUNCH();
        cur ^= 1;
        k_reloc_bound<<<kScanBlocks, TO_BLOCK, 0, st>>>(reloc_level_bytes(table, levels_or_null, one, lev - 1), g, half - 1, u, points, n, poses,
                                                        sp.st, sp.nodes[cur], nullptr, sp.bounds[cur]);
        TO_HIP_CHECK_LAUNCH();
    }
    k_reloc_final<<<1, kRelocBlock, 0, st>>>(sp.st, rec, sp.nodes[cur], sp.bounds[cur], win, h);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
