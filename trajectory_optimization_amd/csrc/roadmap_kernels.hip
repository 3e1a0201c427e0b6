// roadmap_kernels.hip — a free-space roadmap (tools.build_roadmap / plan_path / plan_tour(via=...)), for gfx950.
//
// Nodes Q (M, 3) f32, 2 <= M <= TOHIP_ROADMAP_MAX_NODES, supplied by the caller.  The key of a pair is tour_d2 (tour_kernels.hip): the
// squared distance in f64 without contraction, one value per unordered pair.  Everything after the lengths is integer:
//
//   k_rm_knn     nbr[i][0..k): the k candidates j != i with the smallest (d2, j), ties to the lower j, ascending; both ends finite and
//                d2 <= d2_max; -1 in the slots no candidate fills.  len[i][s] = tour_len_fixed(d2) (-1 in an empty slot).  One wave per
//                query node, four to a block; the block stages 256 candidates at a time through LDS (3 KB), each wave walks them 64 at
//                a time.  The wave keeps its k best in lanes 0..k-1, sorted: a candidate below the k-th key (lane k - 1's) is put in
//                by one ballot (its rank) and one shuffle (the tail moves up a lane).  After the first tiles few candidates pass the
//                threshold (about k ln(M / k) per query in all), so the loop is the M^2 keys and the compare.
//   k_rm_init    D[s][v] = INF, D[s][src[s]] = 0; pred = -1.
//   k_rm_relax   one sweep, one thread per (source, node, slot): an open slot {i, j} of length L relaxes both directions with a 64-bit
//                integer atomicMin on D — D[s][i] + L < D[s][j] -> D[s][j] = the sum, and the reverse.  Integer min only: whatever
//                order the hardware takes, the fixed point is the one shortest-route table.  A thread that lowered anything stores the
//                sweep's tag into *changed (every writer of a sweep stores the same value).
//   k_rm_pred    after convergence: pred[s][v] = the lowest u with {u, v} open and D[s][u] + len == D[s][v] (unsigned atomicMin over
//                0xffffffff = -1); -1 for the source and the unreachable.
//
// The edge stage is tohip_clearance_edges (clearance_kernels.hip) over the filled slots, asked from the lower index; `open` is an input
// of the relax and pred entries.  No cooperative launch, no spin: the host reads *changed once per batch of sweeps.
#include <climits>

namespace {

constexpr int kRmWaves = 4;                  // query nodes (waves) per block of k_rm_knn
constexpr int kRmTile = 64 * kRmWaves;       // candidates staged per tile: one per thread

inline bool rm_sizes_ok(int64_t M, int64_t k) { return M >= 2 && M <= TOHIP_ROADMAP_MAX_NODES && k >= 1 && k <= TOHIP_ROADMAP_MAX_K; }

// (d, j) < (od, oj), ties to the lower index
__device__ __forceinline__ bool rm_key_less(double d, int j, double od, int oj) { return d < od || (d == od && j < oj); }

__global__ void __launch_bounds__(64 * kRmWaves)
k_rm_knn(const float* __restrict__ Q, int M, int k, double d2_max, int* __restrict__ nbr, long long* __restrict__ len) {
    __shared__ float sx[kRmTile], sy[kRmTile], sz[kRmTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kRmWaves + wave;   // this wave's query node (>= M: it stages tiles and keeps nothing)
    const bool live = i < M;
    const float qx = live ? Q[3 * i] : 0.f, qy = live ? Q[3 * i + 1] : 0.f, qz = live ? Q[3 * i + 2] : 0.f;
    const bool q_ok = live && finite3(qx, qy, qz);
    // lane s < k holds the s-th best key so far; an empty slot is (+inf, INT_MAX), above every candidate
    double bd = __builtin_inf();
    int bj = INT_MAX;
    for (int base = 0; base < M; base += kRmTile) {
        __syncthreads();   // the previous tile has been read by every wave
        {
            const int c = base + tid;
            const bool in = c < M;
            sx[tid] = in ? Q[3 * c] : __builtin_nanf("");   // a row past the end is never a candidate
            sy[tid] = in ? Q[3 * c + 1] : 0.f;
            sz[tid] = in ? Q[3 * c + 2] : 0.f;
        }
        __syncthreads();
        if (!q_ok) continue;
        for (int q = 0; q < kRmWaves; ++q) {
            const int t = 64 * q + lane, j = base + t;
            const float cx = sx[t], cy = sy[t], cz = sz[t];
            const bool lower = i < j;
            const double d2 = lower ? tour_d2(qx, qy, qz, cx, cy, cz) : tour_d2(cx, cy, cz, qx, qy, qz);
            const double td = __shfl(bd, k - 1);   // the k-th key so far
            const int tj = __shfl(bj, k - 1);
            const bool cand = j != i && finite3(cx, cy, cz) && d2 <= d2_max && rm_key_less(d2, j, td, tj);
            unsigned long long bal = __ballot(cand);
            while (bal) {   // wave-uniform
                const int srcl = __ffsll((long long)bal) - 1;
                bal &= bal - 1;
                const double cd = __shfl(d2, srcl);
                const int cj = __shfl(j, srcl);
                // its rank among the kept keys: they are sorted, so the lanes below it are a prefix
                const unsigned long long below = __ballot(lane < k && rm_key_less(bd, bj, cd, cj));
                const int pos = __popcll(below);
                const double ud = __shfl_up(bd, 1);
                const int uj = __shfl_up(bj, 1);
                if (pos < k) {   // (uniform) an earlier insert of this tile may have moved the threshold below it
                    if (lane == pos) { bd = cd; bj = cj; }
                    else if (lane > pos && lane < k) { bd = ud; bj = uj; }
                }
            }
        }
    }
    if (live && lane < k) {
        const bool filled = bj != INT_MAX;
        nbr[(size_t)i * k + lane] = filled ? bj : -1;
        len[(size_t)i * k + lane] = filled ? tour_len_fixed(bd) : -1;
    }
}

// one thread per (source, node)
__global__ void __launch_bounds__(256)
k_rm_init(const int* __restrict__ src, int M, long long* __restrict__ D, int* __restrict__ pred) {
    const int v = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (v >= M) return;
    if (D) D[(size_t)s * M + v] = v == src[s] ? 0 : kTourInf;   // (a source out of range: a row of INF)
    if (pred) pred[(size_t)s * M + v] = -1;
}

// one sweep: one thread per (source, node, slot)
__global__ void __launch_bounds__(256)
k_rm_relax(const int* __restrict__ nbr, const long long* __restrict__ len, const unsigned char* __restrict__ open, int M, int k,
           long long* __restrict__ D, int tag, int* __restrict__ changed) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= M * k || !open[c]) return;
    const int i = c / k, j = nbr[c];
    if (j < 0 || j >= M) return;   // (open is the caller's array: an empty slot marked open is skipped)
    const long long L = len[c];
    if (L < 0 || L > kTourMaxLen) return;
    long long* Ds = D + (size_t)blockIdx.y * M;
    const long long di = Ds[i], dj = Ds[j];
    bool low = false;
    if (di < kTourInf && di + L < dj) { atomicMin(&Ds[j], di + L); low = true; }
    if (dj < kTourInf && dj + L < di) { atomicMin(&Ds[i], dj + L); low = true; }
    if (low) *changed = tag;
}

__global__ void __launch_bounds__(256)
k_rm_pred(const int* __restrict__ nbr, const long long* __restrict__ len, const unsigned char* __restrict__ open, int M, int k,
          const int* __restrict__ src, const long long* __restrict__ D, int* __restrict__ pred) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= M * k || !open[c]) return;
    const int i = c / k, j = nbr[c];
    if (j < 0 || j >= M) return;
    const long long L = len[c];
    if (L < 0 || L > kTourMaxLen) return;
    const int s = blockIdx.y, so = src[s];
    const long long* Ds = D + (size_t)s * M;
    unsigned* ps = (unsigned*)pred + (size_t)s * M;
    const long long di = Ds[i], dj = Ds[j];
    if (di < kTourInf && di + L == dj && j != so) atomicMin(&ps[j], (unsigned)i);
    if (dj < kTourInf && dj + L == di && i != so) atomicMin(&ps[i], (unsigned)j);
}

struct RoutesLayout {
    size_t off_pred, off_changed, total;
};

inline bool rm_routes_ok(int64_t M, int64_t S) { return M >= 2 && M <= TOHIP_ROADMAP_MAX_NODES && S >= 1 && S <= TOHIP_ROADMAP_MAX_SOURCES; }

inline RoutesLayout rm_routes_layout(int64_t M, int64_t S) {
    RoutesLayout l;
    size_t o = align_up((size_t)(M * S) * 8, 256);
    l.off_pred = o;    o += align_up((size_t)(M * S) * 4, 256);
    l.off_changed = o; o += 256;
    l.total = o;
    return l;
}

}  // namespace

extern "C" int tohip_roadmap_knn(const float* nodes, int64_t n_nodes, int64_t k, float max_edge, int32_t* nbr, int64_t* len, void* stream) {
    if (!nodes || !nbr || !len || !rm_sizes_ok(n_nodes, k) || !(max_edge >= 0.f)) return TOHIP_EINVAL;   // (a NaN fails the compare)
    const int M = (int)n_nodes;
    const double d2_max = (double)max_edge * (double)max_edge;   // +inf stays +inf: no limit
    k_rm_knn<<<(unsigned)((M + kRmWaves - 1) / kRmWaves), 64 * kRmWaves, 0, (hipStream_t)stream>>>(nodes, M, (int)k, d2_max, nbr,
                                                                                                  (long long*)len);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" size_t tohip_roadmap_routes_bytes(int64_t n_nodes, int64_t n_sources) {
    return rm_routes_ok(n_nodes, n_sources) ? rm_routes_layout(n_nodes, n_sources).total : 0;
}

extern "C" int tohip_roadmap_relax(const int32_t* nbr, const int64_t* len, const uint8_t* open, int64_t n_nodes, int64_t k, const int32_t* src,
                                   int64_t n_sources, int64_t* D, int64_t n_sweeps, int32_t* changed, int init, void* stream) {
    if (!nbr || !len || !open || !src || !D || !changed || !rm_sizes_ok(n_nodes, k) || !rm_routes_ok(n_nodes, n_sources) || n_sweeps < 0 ||
        n_sweeps > n_nodes)
        return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)n_nodes, K = (int)k, S = (int)n_sources;
    if (init) {
        k_rm_init<<<dim3((unsigned)((M + 255) / 256), (unsigned)S), 256, 0, st>>>(src, M, (long long*)D, nullptr);
        TO_HIP_CHECK_LAUNCH();
    }
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)((M * K + 255) / 256), (unsigned)S);
    for (int t = 1; t <= (int)n_sweeps; ++t) {
        k_rm_relax<<<grid, 256, 0, st>>>(nbr, (const long long*)len, open, M, K, (long long*)D, t, changed);
        TO_HIP_CHECK_LAUNCH();
    }
    return TOHIP_OK;
}

extern "C" int tohip_roadmap_pred(const int32_t* nbr, const int64_t* len, const uint8_t* open, int64_t n_nodes, int64_t k, const int32_t* src,
                                  int64_t n_sources, const int64_t* D, int32_t* pred, void* stream) {
    if (!nbr || !len || !open || !src || !D || !pred || !rm_sizes_ok(n_nodes, k) || !rm_routes_ok(n_nodes, n_sources)) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)n_nodes, K = (int)k, S = (int)n_sources;
    k_rm_init<<<dim3((unsigned)((M + 255) / 256), (unsigned)S), 256, 0, st>>>(src, M, nullptr, pred);
    TO_HIP_CHECK_LAUNCH();
    k_rm_pred<<<dim3((unsigned)((M * K + 255) / 256), (unsigned)S), 256, 0, st>>>(nbr, (const long long*)len, open, M, K, src,
                                                                                (const long long*)D, pred);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
