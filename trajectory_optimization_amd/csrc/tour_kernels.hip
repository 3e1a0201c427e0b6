// tour_kernels.hip — a collision-checked tour through chosen views (tools.plan_tour), for gfx950.
//
// Nodes P (n, 3) f32, 2 <= n <= TOHIP_TOUR_MAX_NODES, node 0 the start.  Edge (i, j), i < j, has index e = i n - i (i + 1) / 2 + (j - i - 1)
// (the upper triangle in row-major order) and is OPEN iff both ends are finite, edge_idx[e] == -1 (tohip_clearance_edges' answer for
// a = P_i, b = P_j; no array: every edge between finite nodes) and its length fits.  Everything after the lengths is integer:
//
//   k_tour_init    w_ij = llrint(sqrt((dx dx + dy dy) + dz dz) 2^20) in f64 without contraction (dx = (double)x_lo - (double)x_hi, lo < hi:
//                  one value per pair); closed when w > 2^40.  D = w on open edges, 0 on the diagonal, INF = 2^62 elsewhere; nxt = j
//                  on open edges, -1 elsewhere.  With a roadmap's routes (tohip_tour_plan_via): w = min(w, via_D[i][j]), flagged.
//   k_tour_fw      one launch per k, ascending, one thread per (i, j): D[i][k] + D[k][j] < D[i][j] strictly, both terms below INF ->
//                  D[i][j] = the sum, nxt[i][j] = nxt[i][k].  D[k][k] = 0, so row k and column k do not change during iteration k
//                  (D[i][k] + 0 < D[i][k] never holds): the threads of a sweep read only what none of them writes, and the parallel
//                  sweep IS the serial Floyd-Warshall loop, tie rule included.
//   k_tour_route   one block of 1 024 threads.  R = {j : D[0][j] < INF}, m = |R|.  Nearest neighbour from node 0 (wave 0 alone: each
//                  lane owns the nodes lane + 64 q and keeps their visited bits in a register, the argmin of (D, j) by shuffles — no
//                  barrier in its m - 1 dependent steps).  Then best-improvement 2-opt with position 0 fixed: wave w takes the rows
//                  i = 1 + w + 16 q, lane l the columns j = i + 1 + l + 64 q, both ascending, so a strict `<` keeps the lowest (i, j)
//                  per thread; across threads the minimum of (change, i << 8 | j) as k_views_pick folds its (gain, index).  The order
//                  and the lengths of its consecutive legs live in LDS, D stays in L2 (512 KB at n = 256: two gathers per candidate).
//                  Changes are exact integers: every move shortens the tour, the loop ends with or without the cap.
//
// No atomics, no float compare after k_tour_init: the same bits in every run.
//
// Buffer (tohip_tour_bytes(n)), every section aligned to 256 B:
//   [header 32 x i64 — [0] m [1] moves [2] converged [3] length_fixed [4] nn_length_fixed [5] status (bit 0: node 0 is not finite)]
//   [order n i32 (the first m count, -1 behind them)] [unreachable n u8] [D n x n i64] [nxt n x n i32]
#include <climits>
#include <cmath>

namespace {

constexpr size_t kTourHdr = 256;
constexpr long long kTourInf = 1ll << 62;
constexpr long long kTourMaxLen = 1ll << 40;

struct TourLayout {
    size_t off_order, off_unreach, off_D, off_nxt, total;
};

inline bool tour_size_ok(int64_t n) { return n >= 2 && n <= TOHIP_TOUR_MAX_NODES; }

inline TourLayout tour_layout(int64_t n) {
    TourLayout l;
    size_t o = kTourHdr;
    l.off_order = o;   o += align_up((size_t)n * 4, 256);
    l.off_unreach = o; o += align_up((size_t)n, 256);
    l.off_D = o;       o += align_up((size_t)(n * n) * 8, 256);
    l.off_nxt = o;     o += align_up((size_t)(n * n) * 4, 256);
    l.total = o;
    return l;
}

// the key of a pair: the squared distance in f64 without contraction, differences taken lower index minus higher
__device__ __forceinline__ double tour_d2(float xl, float yl, float zl, float xh, float yh, float zh) {
    const double dx = (double)xl - (double)xh, dy = (double)yl - (double)yh, dz = (double)zl - (double)zh;
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// llrint(sqrt(d2) 2^20), held at 2^42 so that llrint stays in range; anything above kTourMaxLen is closed anyway
__device__ __forceinline__ long long tour_len_fixed(double d2) {
    const double L = sqrt(d2) * 1048576.0;
    return L < 4398046511104.0 ? llrint(L) : (1ll << 42);
}

// the straight leg (i, j), i != j: its integer length when it is open, INF otherwise
__device__ __forceinline__ long long tour_direct(const float* __restrict__ P, int n, const int* __restrict__ edge_idx, int i, int j) {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const float xl = P[3 * lo], yl = P[3 * lo + 1], zl = P[3 * lo + 2], xh = P[3 * hi], yh = P[3 * hi + 1], zh = P[3 * hi + 2];
    const bool finite = finite3(xl, yl, zl) && finite3(xh, yh, zh);
    const int e = lo * n - lo * (lo + 1) / 2 + (hi - lo - 1);
    if (finite && (!edge_idx || edge_idx[e] == -1)) {
        const long long q = tour_len_fixed(tour_d2(xl, yl, zl, xh, yh, zh));
        if (q <= kTourMaxLen) return q;
    }
    return kTourInf;
}

// one thread per (i, j).  With a roadmap behind the legs (via_D, or null): w_ij = min(direct, via), via = via_D[i][j] (row i: the routes
// from node i over the roadmap, leading dimension ld); via_flag (or null) = 1 where the roadmap's route is strictly shorter than the
// straight leg (or that leg is closed).  Both branches are on kernel arguments: uniform over the grid
__global__ void __launch_bounds__(256)
k_tour_init(const float* __restrict__ P, int n, const int* __restrict__ edge_idx, const long long* __restrict__ via_D, long long ld,
            long long* __restrict__ D, int* __restrict__ nxt, unsigned char* __restrict__ via_flag) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n * n) return;
    const int i = c / n, j = c % n;
    long long w = 0;
    unsigned char f = 0;
    if (i != j) {
        w = tour_direct(P, n, edge_idx, i, j);
        if (via_D) {
            const long long via = via_D[(long long)i * ld + j];
            if (via < w) { w = via; f = 1; }
        }
    }
    D[c] = w;
    nxt[c] = (i != j && w < kTourInf) ? j : -1;
    if (via_flag) via_flag[c] = f;
}

// iteration k of Floyd-Warshall, one thread per (i, j): reads row k and column k, which no thread of this sweep writes
__global__ void __launch_bounds__(256) k_tour_fw(int n, int k, long long* __restrict__ D, int* __restrict__ nxt) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n * n) return;
    const int i = c / n, j = c % n;
    const long long a = D[i * n + k], b = D[k * n + j];
    if (a >= kTourInf || b >= kTourInf) return;
    if (a + b < D[c]) {
        D[c] = a + b;
        nxt[c] = nxt[i * n + k];
    }
}

struct TourRoute {
    long long* hdr;
    int* order;
    unsigned char* unreach;
    const long long* D;
    const float* P;
    int n, closed;
    long long max_moves;
};

// the smaller of two (value, code) pairs, ties to the lower code
__device__ __forceinline__ void tour_min(long long& v, int& c, long long ov, int oc) {
    if (ov < v || (ov == v && oc < c)) { v = ov; c = oc; }
}

__device__ __forceinline__ void tour_wave_min(long long& v, int& c) {
    for (int sh = 32; sh > 0; sh >>= 1) {
        const long long ov = __shfl_xor(v, sh);
        const int oc = __shfl_xor(c, sh);
        tour_min(v, c, ov, oc);
    }
}

__global__ void __launch_bounds__(1024) k_tour_route(TourRoute a) {
    __shared__ int t[TOHIP_TOUR_MAX_NODES + 1];          // the order; t[m] = t[0] when closed
    __shared__ long long seg[TOHIP_TOUR_MAX_NODES];      // seg[p] = D[t[p]][t[p + 1]]: the legs of the order (p = m - 1: the closing one, or 0)
    __shared__ long long bv[16];
    __shared__ int bc[16];
    __shared__ int cnt[4];
    __shared__ long long s_len;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const long long* D = a.D;

    // the reachable set
    bool reach = false;
    if (tid < TOHIP_TOUR_MAX_NODES) {
        reach = tid < n && D[tid] < kTourInf;
        if (tid < n) a.unreach[tid] = reach ? 0 : 1;
        const unsigned long long bal = __ballot(reach);
        if (lane == 0) cnt[wave] = __popcll(bal);
    }
    __syncthreads();
    const int m = cnt[0] + cnt[1] + cnt[2] + cnt[3];

    // nearest neighbour, wave 0: lane l owns the nodes l + 64 q
    if (wave == 0) {
        unsigned open = 0;   // bit q: node lane + 64 q is reachable and not visited
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q;
            if (j < n && j != 0 && D[j] < kTourInf) open |= 1u << q;
        }
        int last = 0;
        long long len = 0;
        if (lane == 0) t[0] = 0;
        for (int p = 1; p < m; ++p) {
            long long v = LLONG_MAX;
            int c = 0x7fffffff;
            for (int q = 0; q < 4; ++q) {   // ascending j: a later equal distance does not replace an earlier one
                if (!(open >> q & 1)) continue;
                const int j = lane + 64 * q;
                const long long d = D[last * n + j];
                if (d < v) { v = d; c = j; }
            }
            tour_wave_min(v, c);
            if ((c & 63) == lane) open &= ~(1u << (c >> 6));
            if (lane == 0) t[p] = c;
            len += v;
            last = c;
        }
        if (a.closed && m > 1) len += D[last * n];   // back to node 0
        if (lane == 0) s_len = len;
    }
    __syncthreads();
    const long long nn_len = s_len;
    if (tid == 0) t[m] = t[0];
    __syncthreads();

    // 2-opt, best improvement
    long long len = nn_len, moves = 0;
    int converged = 0;
    for (;;) {
        if (tid < m) seg[tid] = (tid + 1 < m || a.closed) ? D[t[tid] * n + t[tid + 1]] : 0;
        __syncthreads();
        long long v = 0;   // only a negative change is a move
        int c = 0x7fffffff;
        for (int i = 1 + wave; i < m - 1; i += 16) {
            const int tp = t[i - 1], ti = t[i];
            const long long sp = seg[i - 1];
            for (int j = i + 1 + lane; j < m; j += 64) {
                // reversing t[i..j]: the legs (i - 1, i) and (j, j + 1) give way to (i - 1, j) and (i, j + 1); an open tour has no
                // leg behind its last position
                const bool has_next = a.closed || j + 1 < m;
                long long d = D[tp * n + t[j]] - sp;
                if (has_next) d += D[ti * n + t[j + 1]] - seg[j];
                if (d < v) { v = d; c = i << 8 | j; }
            }
        }
        tour_wave_min(v, c);
        if (lane == 0) { bv[wave] = v; bc[wave] = c; }
        __syncthreads();
        v = bv[0]; c = bc[0];
        for (int w = 1; w < 16; ++w) tour_min(v, c, bv[w], bc[w]);
        if (v >= 0) { converged = 1; break; }   // (uniform: every thread folds the same sixteen pairs)
        if (moves >= a.max_moves) break;
        const int i = c >> 8, j = c & 255;
        __syncthreads();   // everyone has read bv / bc and the order
        if (tid < (j - i + 1) / 2) {
            const int x = t[i + tid];
            t[i + tid] = t[j - tid];
            t[j - tid] = x;
        }
        len += v;
        ++moves;
        __syncthreads();
    }

    if (tid < n) a.order[tid] = tid < m ? t[tid] : -1;
    if (tid == 0) {
        a.hdr[0] = m;
        a.hdr[1] = moves;
        a.hdr[2] = converged;
        a.hdr[3] = len;
        a.hdr[4] = nn_len;
        a.hdr[5] = finite3(a.P[0], a.P[1], a.P[2]) ? 0 : 1;
    }
}

}  // namespace

extern "C" size_t tohip_tour_bytes(int64_t n) { return tour_size_ok(n) ? tour_layout(n).total : 0; }

namespace {

// the stages behind both entries: the leg matrix (with or without a roadmap's routes), Floyd-Warshall, the route
int tour_run(const float* nodes, int64_t n, const int32_t* edge_idx, const long long* via_D, int64_t via_ld, unsigned char* via_flag,
             int closed, int64_t max_moves, void* buf, size_t bytes, void* stream) {
    if (!nodes || !buf || !tour_size_ok(n) || max_moves < 0) return TOHIP_EINVAL;
    const TourLayout l = tour_layout(n);
    if (bytes < l.total) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    char* b = (char*)buf;
    long long* D = (long long*)(b + l.off_D);
    int* nxt = (int*)(b + l.off_nxt);
    const int N = (int)n;
    const unsigned blocks = (unsigned)((N * N + 255) / 256);
    k_tour_init<<<blocks, 256, 0, st>>>(nodes, N, edge_idx, via_D, (long long)via_ld, D, nxt, via_flag);
    TO_HIP_CHECK_LAUNCH();
    for (int k = 0; k < N; ++k) {
        k_tour_fw<<<blocks, 256, 0, st>>>(N, k, D, nxt);
        TO_HIP_CHECK_LAUNCH();
    }
    TourRoute a;
    a.hdr = (long long*)b; a.order = (int*)(b + l.off_order); a.unreach = (unsigned char*)(b + l.off_unreach);
    a.D = D; a.P = nodes; a.n = N; a.closed = closed != 0; a.max_moves = max_moves;
    k_tour_route<<<1, 1024, 0, st>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

}  // namespace

extern "C" int tohip_tour_plan(const float* nodes, int64_t n, const int32_t* edge_idx, int closed, int64_t max_moves, void* buf, size_t bytes,
                               void* stream) {
    return tour_run(nodes, n, edge_idx, nullptr, 0, nullptr, closed, max_moves, buf, bytes, stream);
}

extern "C" int tohip_tour_plan_via(const float* nodes, int64_t n, const int32_t* edge_idx, const int64_t* via_D, int64_t via_ld, int closed,
                                   int64_t max_moves, void* buf, size_t bytes, uint8_t* via_flag, void* stream) {
    if (!via_D || !via_flag || via_ld < n) return TOHIP_EINVAL;
    return tour_run(nodes, n, edge_idx, (const long long*)via_D, via_ld, via_flag, closed, max_moves, buf, bytes, stream);
}
