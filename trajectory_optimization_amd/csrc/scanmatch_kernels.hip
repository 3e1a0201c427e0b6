// scanmatch_kernels.hip — scan-to-map registration on the evidence map ("Scan matching"), for gfx950: score a scan of
// sensor-frame points against the map's log-odds at every pose of a search window — K rotations x (2wx+1)(2wy+1)(2wz+1) integer voxel
// shifts — and name the best.  Included right after evidence_kernels.hip: the geometry, the coordinate rule, the brick layout, the
// evidence buffer's checks and the per-wave count are the map layer's (OccGeom, occ_locate, occ_word, occ_bit, occ_brick_mask,
// evid_check, evid_size, occ_count).
//
// A POSE is 12 f32: R row-major, then t.  The world coordinate of a sensor-frame point p is, per axis a,
// fl(fl(fl(fl(R_a0 p_x) + fl(R_a1 p_y)) + fl(R_a2 p_z)) + t_a); its voxel is occ_locate's.  A point out of range on any axis (NaN
// and inf included) is skipped; a point in the apron takes part.  The VALUE of a voxel: max(L, floor) inside dims where L != -128,
// unknown_value everywhere else.  score[k][s] = the sum over the points not skipped of V(voxel_k(p) + s).  All integers.
//
//   k_scan_prepare    evidence bytes -> the SCORE TABLE: the same size and brick order, header 256 zero bytes, byte = 128 + V (pad
//                     voxels 128 + unknown_value).  One lane per brick word: two 16-byte loads, two 16-byte stores.
//   k_scan_score      B explicit candidates (pose, optional shift) from the evidence bytes themselves, V applied per lookup: score,
//                     used (points in range), inside (shifted voxel inside dims), known (inside and L != -128).  Grid candidates x
//                     point tiles, a grid-stride loop over the tiles, a wave reduction and one integer atomic per wave and counter.
//   k_scan_correlate  the hot path, from the table.  A block owns one rotation and walks tiles of 256 points: each lane transforms
//                     one point and the tile's points in range are packed into LDS (their order does not matter to an integer
//                     sum).  Then lanes own ROWS of the window — one (dy, dz) and all its dx — and, where the window has fewer
//                     than 128 rows, a share of the tile's points each.  For one point a row is 2 wx + 1 consecutive voxels along
//                     x: bytes that are consecutive in the brick words of consecutive x bricks, 32 bytes apart.  The lane loads the
//                     G + 1 dwords that cover its G = ceil((2 wx + 1) / 4) groups of four, funnels each adjacent pair by
//                     (x0 & 3) bytes and adds v & 0x00FF00FF and (v >> 8) & 0x00FF00FF into two registers of 16-bit sums per
//                     group: 256 points x 255 fit 16 bits.  Per four lookups that is one load, one funnel shift, two ands, one
//                     shift and two adds; the row's address is computed once per point, and nothing crosses lanes.  Where the
//                     whole span lies inside dims the G + 1 loads share one address and differ by an immediate offset; otherwise a
//                     brick outside dims gives 128 + unknown_value from a predicate (dword 0 of the table is loaded in its place):
//                     nothing is loaded out of bounds.  After a tile the
//                     sums are unpacked into the block's int32 window in LDS (LDS atomics: shares of one row meet there); after
//                     the block's last tile the window, less 128 x the points used, goes out with one integer atomic per shift,
//                     consecutive lanes to consecutive addresses.
//   k_scan_best       one block over the K S scores: the maximum of the key (score, smaller |s|^2, lower flat index) and the number
//                     of candidates that share the best score -> int32[8]: flat index, k, dx, dy, dz, score, ties, 0.
//
// No float atomics, no process-wide state, nothing read back; every argument check returns before anything is enqueued.
namespace {

constexpr int kScanMaxWxy = 16;
constexpr int kScanMaxWz = 4;
constexpr int kScanMaxK = 256;
constexpr long long kScanMaxPoints = 1ll << 22;
constexpr long long kScanMaxCandidates = 1ll << 22;
constexpr int kScanBlocks = 2048;          // blocks of a launch the tiles are spread over (eight per CU); more tiles: grid-stride
constexpr int kScanBestBlock = 1024;

struct ScanValue {
    int floor_u, unknown_u;   // 128 + floor, 128 + unknown_value
};

inline bool scan_value_ok(int floor_value, int unknown_value) {
    return floor_value >= -127 && floor_value <= 0 && unknown_value >= -127 && unknown_value <= 0;
}
inline bool scan_window_ok(int wx, int wy, int wz) {
    return wx >= 0 && wx <= kScanMaxWxy && wy >= 0 && wy <= kScanMaxWxy && wz >= 0 && wz <= kScanMaxWz;
}
inline long long scan_window_size(int wx, int wy, int wz) { return (long long)(2 * wx + 1) * (2 * wy + 1) * (2 * wz + 1); }
inline bool scan_aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1u)) == 0; }

// the voxel of sensor-frame point p under pose T (12 f32) -> false: skipped
__device__ __forceinline__ bool scan_voxel(const OccGeom& g, const float* __restrict__ T, const float* __restrict__ p, int& x, int& y, int& z) {
    const float px = p[0], py = p[1], pz = p[2];
    float w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        w[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[3 * a], px), __fmul_rn(T[3 * a + 1], py)), __fmul_rn(T[3 * a + 2], pz)), T[9 + a]);
    return occ_locate(g, w, x, y, z) != kOccOutOfRange;
}

// four table bytes from four evidence bytes: u = L + 128, 0 = never observed
__device__ __forceinline__ unsigned scan_table4(unsigned v, unsigned in4, const ScanValue& p) {
    const unsigned x = v ^ 0x80808080u;
    unsigned out = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int u = (int)((x >> (8 * j)) & 0xFFu);
        const int t = (u == 0 || ((in4 >> j) & 1u) == 0u) ? p.unknown_u : max(u, p.floor_u);
        out |= (unsigned)t << (8 * j);
    }
    return out;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_scan_prepare(const uint4* __restrict__ vals, uint4* __restrict__ table, OccGeom g, long long n_words, ScanValue p) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < n_words; w += stride) {
        int bx, by, bz;
        evid_brick(g, (unsigned)w, bx, by, bz);
        const unsigned in = occ_brick_mask(g, bx, by, bz);
        const uint4 lo = vals[2 * w], hi = vals[2 * w + 1];
        unsigned v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = scan_table4(v[k], (in >> (4 * k)) & 0xFu, p);
        table[2 * w] = make_uint4(v[0], v[1], v[2], v[3]);
        table[2 * w + 1] = make_uint4(v[4], v[5], v[6], v[7]);
    }
}

// sum over the wave, added once per wave (every lane of the wave calls this)
__device__ __forceinline__ void scan_count(int* word, int c) {
    for (int sh = 32; sh > 0; sh >>= 1) c += __shfl_xor(c, sh);
    if ((threadIdx.x & 63) == 0 && c != 0) __hip_atomic_fetch_add(word, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_scan_score(const signed char* __restrict__ vals, OccGeom g, int floor_value, int unknown_value, const float* __restrict__ pts, long long n,
             const float* __restrict__ poses, const int* __restrict__ shifts, long long n_cand, int* __restrict__ score, int* __restrict__ used,
             int* __restrict__ inside, int* __restrict__ known) {
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    for (long long b = blockIdx.x; b < n_cand; b += gridDim.x) {
        const float* T = poses + 12 * b;
        const int sx = shifts ? shifts[3 * b] : 0, sy = shifts ? shifts[3 * b + 1] : 0, sz = shifts ? shifts[3 * b + 2] : 0;
        int sum = 0, n_used = 0, n_in = 0, n_known = 0;
        for (long long tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
            const long long i = tile * TO_BLOCK + threadIdx.x;
            int x, y, z;
            if (i < n && scan_voxel(g, T, pts + 3 * i, x, y, z)) {
                // (a shift is any int32: the sums are taken in 64 bits, and a voxel that does not fit 32 is outside dims)
                const long long xs = (long long)x + sx, ys = (long long)y + sy, zs = (long long)z + sz;
                int V = unknown_value;
                if (xs >= 0 && xs < g.nx && ys >= 0 && ys < g.ny && zs >= 0 && zs < g.nz) {
                    x = (int)xs, y = (int)ys, z = (int)zs;
                    const int L = vals[32ll * occ_word(g, x, y, z) + occ_bit(x, y, z)];
                    ++n_in;
                    if (L != kEvidUnknown) {
                        ++n_known;
                        V = max(L, floor_value);
                    }
                }
                sum += V;
                ++n_used;
            }
        }
        scan_count(score + b, sum);
        scan_count(used + b, n_used);
        scan_count(inside + b, n_in);
        scan_count(known + b, n_known);
    }
}

struct ScanWindow {
    int wx, wy, wz;
    int nxw, nyw;      // 2 wx + 1, 2 wy + 1
    int rows;          // (2 wy + 1)(2 wz + 1)
    int split;         // shares of a tile's points per row: max(1, 256 / rows)
    int S;
};

template <int G>
__global__ void __launch_bounds__(TO_BLOCK)
k_scan_correlate(const unsigned* __restrict__ table, OccGeom g, unsigned unknown4, const float* __restrict__ pts, long long n,
                 const float* __restrict__ poses, ScanWindow win, int* __restrict__ scores, int* __restrict__ used) {
    extern __shared__ int s_sum[];             // the block's window: sums of table bytes, [row][dx]
    __shared__ int s_pts[3 * TO_BLOCK];        // the tile's points in range: base voxels, packed
    __shared__ int s_n, s_used;
    const int t = threadIdx.x, k = blockIdx.y;
    const float* T = poses + 12 * (long long)k;
    for (int s = t; s < win.S; s += TO_BLOCK) s_sum[s] = 0;
    if (t == 0) s_used = 0;
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    const int units = win.rows * win.split;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();   // (the tile before is read to its end; s_sum and s_used are zero)
        if (t == 0) s_n = 0;
        __syncthreads();
        {
            const long long i = tile * TO_BLOCK + t;
            int x, y, z;
            if (i < n && scan_voxel(g, T, pts + 3 * i, x, y, z)) {
                const int slot = atomicAdd(&s_n, 1);
                s_pts[3 * slot] = x, s_pts[3 * slot + 1] = y, s_pts[3 * slot + 2] = z;
            }
        }
        __syncthreads();
        const int nv = s_n;
        if (t == 0) s_used += nv;
        for (int u = t; u < units; u += TO_BLOCK) {
            const int row = u % win.rows, share = u / win.rows;
            const int dzi = row / win.nyw, dyi = row - dzi * win.nyw;
            const int dy = dyi - win.wy, dz = dzi - win.wz;
            unsigned lo[G], hi[G];
#pragma unroll
            for (int q = 0; q < G; ++q) lo[q] = hi[q] = 0u;
            for (int p = share; p < nv; p += win.split) {
                const int xs = s_pts[3 * p] - win.wx, y = s_pts[3 * p + 1] + dy, z = s_pts[3 * p + 2] + dz;
                const bool row_ok = (unsigned)y < (unsigned)g.ny && (unsigned)z < (unsigned)g.nz;
                const int xb = xs >> 2, sh = 8 * (xs & 3);
                // the span's first dword: word ((z>>1) nby + (y>>2)) nbx + xb, eight dwords a word, dword (y&3) | (z&1)<<2 of it (at
                // most 2^29 dwords a table; meaningless, and not used, where the row lies outside dims)
                const unsigned first = (unsigned)(((z >> 1) * g.nby + (y >> 2)) * g.nbx + xb) * 8u + (unsigned)((y & 3) | ((z & 1) << 2));
                unsigned w[G + 1];
                if (row_ok && xb >= 0 && xb + G < g.nbx) {   // the whole span inside dims: one address, G + 1 loads 32 bytes apart
                    const unsigned* span = table + first;
#pragma unroll
                    for (int q = 0; q <= G; ++q) w[q] = span[8 * q];
                } else {
#pragma unroll
                    for (int q = 0; q <= G; ++q) {   // (a brick outside dims: dword 0 is loaded in its place and not used)
                        const bool in = row_ok && (unsigned)(xb + q) < (unsigned)g.nbx;
                        const unsigned v = table[in ? first + 8u * q : 0u];
                        w[q] = in ? v : unknown4;
                    }
                }
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const unsigned v = (unsigned)((((unsigned long long)w[q + 1] << 32) | w[q]) >> sh);
                    lo[q] += v & 0x00FF00FFu;
                    hi[q] += (v >> 8) & 0x00FF00FFu;
                }
            }
            int* out = s_sum + row * win.nxw;
#pragma unroll
            for (int q = 0; q < G; ++q) {
                const int sums[4] = {(int)(lo[q] & 0xFFFFu), (int)(hi[q] & 0xFFFFu), (int)(lo[q] >> 16), (int)(hi[q] >> 16)};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * q + j < win.nxw && sums[j] != 0) atomicAdd(out + 4 * q + j, sums[j]);
            }
        }
    }
    __syncthreads();
    const int n_used = s_used;
    if (n_used == 0) return;
    if (t == 0) __hip_atomic_fetch_add(used + k, n_used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int* dst = scores + (long long)k * win.S;
    for (int s = t; s < win.S; s += TO_BLOCK) {
        const int v = s_sum[s] - 128 * n_used;
        if (v != 0) __hip_atomic_fetch_add(dst + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct ScanBest {
    int score, d2;
    int idx;       // -1: none
    int ties;
};

// the better of two under the key (score, smaller d2, lower index); ties of the best score add up
__device__ __forceinline__ ScanBest scan_better(const ScanBest& a, const ScanBest& b) {
    if (a.idx < 0) return b;
    if (b.idx < 0) return a;
    ScanBest r;
    if (a.score != b.score) {
        r = a.score > b.score ? a : b;
    } else {
        const bool first = a.d2 != b.d2 ? a.d2 < b.d2 : a.idx < b.idx;
        r = first ? a : b;
        r.ties = a.ties + b.ties;
    }
    return r;
}

__device__ __forceinline__ void scan_decode(const ScanWindow& win, int idx, int& k, int& dx, int& dy, int& dz) {
    k = idx / win.S;
    const int s = idx - k * win.S;
    const int dzi = s / (win.nxw * win.nyw), rem = s - dzi * win.nxw * win.nyw;
    const int dyi = rem / win.nxw;
    dx = rem - dyi * win.nxw - win.wx, dy = dyi - win.wy, dz = dzi - win.wz;
}

__global__ void __launch_bounds__(kScanBestBlock)
k_scan_best(const int* __restrict__ scores, int total, ScanWindow win, int* __restrict__ best) {
    __shared__ ScanBest s_best[kScanBestBlock];
    const int t = threadIdx.x;
    ScanBest mine{0, 0, -1, 0};
    for (int i = t; i < total; i += kScanBestBlock) {
        const int sc = scores[i];
        if (mine.idx >= 0 && sc < mine.score) continue;
        int k, dx, dy, dz;
        scan_decode(win, i, k, dx, dy, dz);
        mine = scan_better(mine, ScanBest{sc, dx * dx + dy * dy + dz * dz, i, 1});
    }
    s_best[t] = mine;
    __syncthreads();
    for (int half = kScanBestBlock / 2; half > 0; half >>= 1) {
        if (t < half) s_best[t] = scan_better(s_best[t], s_best[t + half]);
        __syncthreads();
    }
    if (t == 0) {
        const ScanBest b = s_best[0];
        int k, dx, dy, dz;
        scan_decode(win, b.idx, k, dx, dy, dz);
        best[0] = b.idx, best[1] = k, best[2] = dx, best[3] = dy, best[4] = dz, best[5] = b.score, best[6] = b.ties, best[7] = 0;
    }
}

inline ScanWindow scan_window(int wx, int wy, int wz) {
    ScanWindow w{wx, wy, wz, 2 * wx + 1, 2 * wy + 1, (2 * wy + 1) * (2 * wz + 1), 1, 0};
    w.split = w.rows >= TO_BLOCK ? 1 : TO_BLOCK / w.rows;
    w.S = (int)scan_window_size(wx, wy, wz);
    return w;
}

template <int G>
inline void scan_correlate_launch(dim3 grid, hipStream_t st, const unsigned* table, const OccGeom& g, unsigned unknown4, const float* pts,
                                  long long n, const float* poses, const ScanWindow& win, int* scores, int* used) {
    k_scan_correlate<G><<<grid, TO_BLOCK, (size_t)win.S * sizeof(int), st>>>(table, g, unknown4, pts, n, poses, win, scores, used);
}

}  // namespace

extern "C" int tohip_scan_prepare(const void* evid, size_t evid_bytes, const tohip_occ_geom* geom, int32_t floor_value, int32_t unknown_value,
                                  void* table, size_t table_bytes, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    int rc = evid_check(evid, evid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    rc = evid_check(table, table_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (table == evid || !scan_value_ok(floor_value, unknown_value)) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(table, 0, kEvidHdr, st);
    if (e != hipSuccess) return (int)e;
    const long long n_words = (long long)occ_words(g.nx, g.ny, g.nz);
    k_scan_prepare<<<occ_grid_blocks(n_words), TO_BLOCK, 0, st>>>(reinterpret_cast<const uint4*>((const char*)evid + kEvidHdr),
                                                                 reinterpret_cast<uint4*>((char*)table + kEvidHdr), g, n_words,
                                                                 ScanValue{128 + floor_value, 128 + unknown_value});
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_scan_score(const void* evid, size_t evid_bytes, const tohip_occ_geom* geom, int32_t floor_value, int32_t unknown_value,
                                const float* points, int64_t n, const float* poses, const int32_t* shifts_or_null, int64_t b, int32_t* score,
                                int32_t* used, int32_t* inside, int32_t* known, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = evid_check(evid, evid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!scan_value_ok(floor_value, unknown_value) || n < 1 || n > kScanMaxPoints || b < 1 || b > kScanMaxCandidates || !points || !poses ||
        !score || !used || !inside || !known)
        return TOHIP_EINVAL;
    const void* bufs[8] = {score, used, inside, known, points, poses, shifts_or_null, evid};
    for (int i = 0; i < 8; ++i) {
        if (!scan_aligned(bufs[i], 4)) return TOHIP_EINVAL;
        for (int j = 0; j < 4; ++j)   // no output is an input or another output
            if (i > j && bufs[i] == bufs[j]) return TOHIP_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream_;
    int32_t* outs[4] = {score, used, inside, known};
    for (int i = 0; i < 4; ++i) {
        const hipError_t e = hipMemsetAsync(outs[i], 0, (size_t)b * sizeof(int32_t), st);
        if (e != hipSuccess) return (int)e;
    }
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    const long long per = (kScanBlocks + b - 1) / b;   // tile blocks per candidate: the launch holds about kScanBlocks blocks
    const dim3 grid((unsigned)(b < (1ll << 20) ? b : (1ll << 20)), (unsigned)(per < n_tiles ? per : n_tiles));
    k_scan_score<<<grid, TO_BLOCK, 0, st>>>((const signed char*)evid + kEvidHdr, g, floor_value, unknown_value, points, n, poses, shifts_or_null, b,
                                            score, used, inside, known);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_scan_correlate(const void* table, size_t table_bytes, const tohip_occ_geom* geom, int32_t unknown_value, const float* points,
                                    int64_t n, const float* poses, int64_t k, int32_t wx, int32_t wy, int32_t wz, int32_t* scores,
                                    size_t scores_bytes, int32_t* used, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    const int rc = evid_check(table, table_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!scan_value_ok(0, unknown_value) || !scan_window_ok(wx, wy, wz) || n < 1 || n > kScanMaxPoints || k < 1 || k > kScanMaxK || !points ||
        !poses || !scores || !used)
        return TOHIP_EINVAL;
    const long long S = scan_window_size(wx, wy, wz);
    if (k * S > kScanMaxCandidates) return TOHIP_EINVAL;
    const void* bufs[5] = {scores, used, points, poses, table};
    for (int i = 0; i < 5; ++i) {
        if (!scan_aligned(bufs[i], 4)) return TOHIP_EINVAL;
        for (int j = 0; j < 2; ++j)
            if (i > j && bufs[i] == bufs[j]) return TOHIP_EINVAL;
    }
    if (scores_bytes < (size_t)(k * S) * sizeof(int32_t)) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    hipError_t e = hipMemsetAsync(scores, 0, (size_t)(k * S) * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(used, 0, (size_t)k * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const ScanWindow win = scan_window(wx, wy, wz);
    const long long n_tiles = (n + TO_BLOCK - 1) / TO_BLOCK;
    const long long per = (kScanBlocks + k - 1) / k;
    const dim3 grid((unsigned)(per < n_tiles ? per : n_tiles), (unsigned)k);
    const unsigned unknown4 = (unsigned)(128 + unknown_value) * 0x01010101u;
    const unsigned* tab = reinterpret_cast<const unsigned*>((const char*)table + kEvidHdr);
    switch ((win.nxw + 3) / 4) {
        case 1: scan_correlate_launch<1>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
        case 2: scan_correlate_launch<2>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
        case 3: scan_correlate_launch<3>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
        case 4: scan_correlate_launch<4>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
        case 5: scan_correlate_launch<5>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
        case 6: scan_correlate_launch<6>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
        case 7: scan_correlate_launch<7>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
        case 8: scan_correlate_launch<8>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
        default: scan_correlate_launch<9>(grid, st, tab, g, unknown4, points, n, poses, win, scores, used); break;
    }
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_scan_best(const int32_t* scores, int64_t k, int32_t wx, int32_t wy, int32_t wz, int32_t* best, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    if (!scan_window_ok(wx, wy, wz) || k < 1 || k > kScanMaxK || !scores || !best || (const void*)scores == (const void*)best ||
        !scan_aligned(scores, 4) || !scan_aligned(best, 4))
        return TOHIP_EINVAL;
    const long long S = scan_window_size(wx, wy, wz);
    if (k * S > kScanMaxCandidates) return TOHIP_EINVAL;
    k_scan_best<<<1, kScanBestBlock, 0, (hipStream_t)stream_>>>(scores, (int)(k * S), scan_window(wx, wy, wz), best);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
