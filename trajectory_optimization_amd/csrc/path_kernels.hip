// path_kernels.hip — refine a planned walk into a trajectory (tools.refine_path), for gfx950.
//
// Nodes P (L, 3) f32, 2 <= L <= TOHIP_PATH_MAX_NODES, in walking order; kept(i) = i == 0 || i == L - 1 || keep[i] != 0.  A chord is a
// pair (i, j), i < j, j - i <= W.  Its length is the tour's: w_ij = tour_len_fixed(tour_d2(P_i, P_j)) (tour_kernels.hip: f64 without
// contraction, lower index minus higher, held at 2^42).  The input leg (i, i + 1) is always open; a chord with j >= i + 2 is open iff no
// kept node lies strictly between its ends, w_ij <= 2^40 and open_band[i][j - i - 1] != 0.  Everything after the lengths is integer:
//
//   search   D[0] = 0, D[j] = min over open (i, j) of D[i] + w_ij, pred[j] = the lowest i that attains it.  A forward recurrence: for
//            each j the block's threads stride over the candidates i in [max(j - W, the last kept node below j), j), compute w_ij on the
//            fly and fold the 64-bit key (D[i] + w_ij, i) — by shuffles inside a wave, through LDS across the four waves.  The waves'
//            slots are double-buffered on the parity of j and every thread folds them itself, so D[j] reaches the next step in a
//            register and through LDS the step after: ONE barrier per j.
//   corners  c_0 = 0 < ... < c_m = L - 1 by following pred back from L - 1 (one thread: m dependent LDS reads).
//   legs     w_q = the length of corner leg q, n_q = max(1, (w_q + H - 1) / H) pieces (1 without a spacing); the exclusive prefix sums
//            of both, in int64, by one scan over the block each.
//   rows     one thread per output row finds its leg by binary search in the prefix of n_q: row (q, t) = A + (B - A) (t / n_q) per
//            coordinate in f64, rounded to f32 (t = 0: A itself); the last row is P[L - 1]; row_node = the input index at a corner row,
//            -1 elsewhere.  With quats: between the kept corners a and b around the row, u = s_row / S_ab (lengths along the corner
//            legs, exact integers below 2^53 in f64), the row's quaternion = normalise((1 - u) q_a + u q_b) in f64 with q_a, q_b
//            normalised and q_b negated when q_a . q_b < 0; a kept row's quaternion is its own, normalised.
//
// One launch of one block; no atomics, no float compare that decides anything after the lengths: the same bits in every run, whatever
// the block size.
//
// Buffer (tohip_path_bytes(L, max_rows)), every section aligned to 256 B:
//   [header 32 x i64 — [0] m [1] R [2] length_fixed [3] input_length_fixed [4] status [5] n_open (the open chords with j >= i + 2)]
//   [D L i64] [pred L i32] [corner L i32 (the first m + 1 count, -1 behind them)]
//   [out_poses max_rows x 3 f32] [out_quats max_rows x 4 f32] [row_node max_rows i32]
// status bit 0: a coordinate of P, or a kept row's quaternion, is not finite, or that quaternion is zero — only the header is written
// (m = R = 0).  Bit 1: R > max_rows — D, pred, corner and the header (R = the rows needed) are written, no row is.
#include <climits>
#include <cmath>

namespace {

constexpr int kPathBlock = 256;
constexpr int kPathWaves = kPathBlock / 64;
constexpr int kPathPerThread = TOHIP_PATH_MAX_NODES / kPathBlock;   // items of a scan each thread owns
constexpr size_t kPathHdr = 256;
constexpr long long kPathMaxStep = 1ll << 42;   // H is held here: no leg is longer, so any larger spacing cuts nothing either

struct PathLayout {
    size_t off_D, off_pred, off_corner, off_poses, off_quats, off_row_node, total;
};

inline bool path_sizes_ok(int64_t L, int64_t max_rows) {
    return L >= 2 && L <= TOHIP_PATH_MAX_NODES && max_rows >= 1 && max_rows <= TOHIP_PATH_MAX_ROWS;
}

inline PathLayout path_layout(int64_t L, int64_t max_rows) {
    PathLayout l;
    size_t o = kPathHdr;
    l.off_D = o;        o += align_up((size_t)L * 8, 256);
    l.off_pred = o;     o += align_up((size_t)L * 4, 256);
    l.off_corner = o;   o += align_up((size_t)L * 4, 256);
    l.off_poses = o;    o += align_up((size_t)max_rows * 12, 256);
    l.off_quats = o;    o += align_up((size_t)max_rows * 16, 256);
    l.off_row_node = o; o += align_up((size_t)max_rows * 4, 256);
    l.total = o;
    return l;
}

struct PathArgs {
    const float* P;
    const float* quats;            // may be NULL
    const unsigned char* keep;     // may be NULL
    const unsigned char* band;
    int L, W, max_rows;
    long long H;                   // 0: corners only
    long long* hdr;
    long long* D;
    int* pred;
    int* corner;
    float* out_poses;
    float* out_quats;
    int* row_node;
};

__device__ __forceinline__ bool path_kept(const PathArgs& a, int i) { return i == 0 || i == a.L - 1 || (a.keep && a.keep[i]); }

// q / |q| in f64, |q|^2 = ((w w + x x) + y y) + z z
__device__ __forceinline__ void path_unit_quat(const float* __restrict__ q, double (&o)[4]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double n = sqrt(((w * w + x * x) + y * y) + z * z);
    o[0] = w / n; o[1] = x / n; o[2] = y / n; o[3] = z / n;
}

// in place: a[0..n) -> its exclusive prefix sums, n <= kPathPerThread * kPathBlock; every thread gets the total.  Thread t owns the
// items kPathPerThread t ...; a shuffle scan inside each wave, the waves' totals through LDS.  Integers: any order gives these sums.
__device__ __forceinline__ long long path_block_scan(long long* a, int n, long long* wave_tot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = kPathPerThread * tid;
    long long v[kPathPerThread], s = 0;
#pragma unroll
    for (int k = 0; k < kPathPerThread; ++k) {
        v[k] = b + k < n ? a[b + k] : 0;
        s += v[k];
    }
    long long inc = s;
    for (int sh = 1; sh < 64; sh <<= 1) {
        const long long up = __shfl_up(inc, sh);
        if (lane >= sh) inc += up;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    long long run = inc - s, total = 0;
    for (int w = 0; w < kPathWaves; ++w) {
        if (w < wave) run += wave_tot[w];
        total += wave_tot[w];
    }
#pragma unroll
    for (int k = 0; k < kPathPerThread; ++k) {
        if (b + k < n) a[b + k] = run;
        run += v[k];
    }
    __syncthreads();   // the prefix is in place, and wave_tot may be written again
    return total;
}

__global__ void __launch_bounds__(kPathBlock) k_path_refine(PathArgs a) {
    constexpr int N = TOHIP_PATH_MAX_NODES;
    __shared__ float sP[3 * N];
    __shared__ long long sD[N];     // D during the search; then the exclusive prefix of the corner legs' lengths ([m]: their sum)
    __shared__ long long sRow[N];   // the exclusive prefix of n_q ([m]: R - 1)
    __shared__ int sPred[N];
    __shared__ int sLast[N];        // the largest kept node <= i
    __shared__ int sNext[N];        // the smallest kept node >= i
    __shared__ int sRev[N];         // the corners as the walk back finds them
    __shared__ int sCorner[N];
    __shared__ int sPos[N];         // a corner's position in the corner list
    __shared__ long long bv[2][kPathWaves];
    __shared__ int bc[2][kPathWaves];
    __shared__ long long wave_tot[kPathWaves], red_len[kPathWaves];
    __shared__ int red_open[kPathWaves];
    __shared__ int s_m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, W = a.W;

    // the nodes into LDS; status bit 0
    int bad = 0;
    for (int i = tid; i < L; i += kPathBlock) {
        const float x = a.P[3 * i], y = a.P[3 * i + 1], z = a.P[3 * i + 2];
        sP[3 * i] = x; sP[3 * i + 1] = y; sP[3 * i + 2] = z;
        bad |= !finite3(x, y, z);
        if (a.quats && path_kept(a, i)) {
            const float q0 = a.quats[4 * i], q1 = a.quats[4 * i + 1], q2 = a.quats[4 * i + 2], q3 = a.quats[4 * i + 3];
            bad |= !(isfinite(q0) && isfinite(q1) && isfinite(q2) && isfinite(q3)) || (q0 == 0.f && q1 == 0.f && q2 == 0.f && q3 == 0.f);
        }
    }
    if (__syncthreads_or(bad)) {
        if (tid < 32) a.hdr[tid] = tid == 4 ? 1 : 0;
        return;
    }

    // the kept node at or below / at or above every node: wave 0 walks up, wave 1 walks down, 64 nodes at a time by one ballot
    if (wave == 0) {
        int carry = -1;
        for (int base = 0; base < L; base += 64) {
            const int i = base + lane;
            const unsigned long long bal = __ballot(i < L && path_kept(a, i));
            const unsigned long long upto = bal & (~0ull >> (63 - lane));
            if (i < L) sLast[i] = upto ? base + 63 - __clzll((long long)upto) : carry;
            if (bal) carry = base + 63 - __clzll((long long)bal);
        }
    } else if (wave == 1) {
        int carry = L - 1;
        for (int base = (L - 1) / 64 * 64; base >= 0; base -= 64) {
            const int i = base + lane;
            const unsigned long long bal = __ballot(i < L && path_kept(a, i));
            const unsigned long long from = bal & (~0ull << lane);
            if (i < L) sNext[i] = from ? base + __ffsll((long long)from) - 1 : carry;
            if (bal) carry = base + __ffsll((long long)bal) - 1;
        }
    }
    if (tid == 0) {
        sD[0] = 0; sPred[0] = -1;
        a.D[0] = 0; a.pred[0] = -1;
    }
    __syncthreads();

    // the search
    long long in_len = 0, Dprev = 0;
    int n_open = 0;
    for (int j = 1; j < L; ++j) {
        const int lo = max(j - W, sLast[j - 1]);   // below it a chord is too long or passes a kept node
        const float xj = sP[3 * j], yj = sP[3 * j + 1], zj = sP[3 * j + 2];
        long long v = LLONG_MAX;
        int c = INT_MAX;
        for (int i = lo + tid; i < j; i += kPathBlock) {   // ascending i: a later equal key does not replace an earlier one
            const long long w = tour_len_fixed(tour_d2(sP[3 * i], sP[3 * i + 1], sP[3 * i + 2], xj, yj, zj));
            const bool leg = i == j - 1;
            bool open = leg;
            if (leg) in_len += w;
            else if (w <= kTourMaxLen && a.band[(size_t)i * W + (j - i - 1)]) { open = true; ++n_open; }
            if (open) {
                const long long key = (leg ? Dprev : sD[i]) + w;   // D[j - 1] is not in LDS for everyone yet
                if (key < v) { v = key; c = i; }
            }
        }
        tour_wave_min(v, c);
        const int s = j & 1;
        if (lane == 0) { bv[s][wave] = v; bc[s][wave] = c; }
        __syncthreads();   // (slot s is written again at j + 2, behind the barrier of j + 1: everyone has read it by then)
        v = bv[s][0]; c = bc[s][0];
        for (int w = 1; w < kPathWaves; ++w) tour_min(v, c, bv[s][w], bc[s][w]);
        Dprev = v;
        if (tid == 0) {
            sD[j] = v; sPred[j] = c;
            a.D[j] = v; a.pred[j] = c;
        }
    }
    for (int sh = 32; sh > 0; sh >>= 1) { in_len += __shfl_xor(in_len, sh); n_open += __shfl_xor(n_open, sh); }
    if (lane == 0) { red_len[wave] = in_len; red_open[wave] = n_open; }
    __syncthreads();

    // the corners: back from L - 1 (pred[j] < j: it ends at 0)
    if (tid == 0) {
        int k = 0, c = L - 1;
        sRev[0] = c;
        while (c != 0) { c = sPred[c]; sRev[++k] = c; }
        s_m = k;
    }
    __syncthreads();
    const int m = s_m;
    for (int q = tid; q < L; q += kPathBlock) {
        const int node = q <= m ? sRev[m - q] : -1;
        sCorner[q] = node;
        a.corner[q] = node;
        if (node >= 0) sPos[node] = q;
    }
    __syncthreads();

    // the corner legs: lengths and pieces, then their exclusive prefix sums (sD is free: the search is over)
    for (int q = tid; q < m; q += kPathBlock) {
        const int na = sCorner[q], nb = sCorner[q + 1];
        const long long w = tour_len_fixed(tour_d2(sP[3 * na], sP[3 * na + 1], sP[3 * na + 2], sP[3 * nb], sP[3 * nb + 1], sP[3 * nb + 2]));
        sD[q] = w;
        sRow[q] = a.H > 0 && w > a.H ? (w + a.H - 1) / a.H : 1;
    }
    __syncthreads();
    const long long len_total = path_block_scan(sD, m, wave_tot);
    const long long rows_total = path_block_scan(sRow, m, wave_tot);
    if (tid == 0) { sD[m] = len_total; sRow[m] = rows_total; }   // (m <= L - 1: in range)
    const long long R = rows_total + 1;
    const int status = R > a.max_rows ? 2 : 0;
    if (tid < 32) {
        long long h = 0;
        if (tid == 0) h = m;
        if (tid == 1) h = R;
        if (tid == 2) h = Dprev;   // D[L - 1] (= len_total: the corner legs are the chords the search summed)
        if (tid == 3) for (int w = 0; w < kPathWaves; ++w) h += red_len[w];
        if (tid == 4) h = status;
        if (tid == 5) for (int w = 0; w < kPathWaves; ++w) h += red_open[w];
        a.hdr[tid] = h;
    }
    if (status) return;   // (uniform)
    __syncthreads();

    // the rows
    const int Rn = (int)R;
    for (int r = tid; r < Rn; r += kPathBlock) {
        int q = m;
        long long t = 0, n = 1;
        if (r < Rn - 1) {
            int lo = 0, hi = m;   // the last q with sRow[q] <= r (n_q >= 1: the prefix is strictly increasing)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (sRow[mid] <= r) lo = mid; else hi = mid;
            }
            q = lo;
            t = r - sRow[q];
            n = sRow[q + 1] - sRow[q];
        }
        const int na = sCorner[q];
        const double f = (double)t / (double)n;
        if (t == 0) {
            a.out_poses[3 * r] = sP[3 * na]; a.out_poses[3 * r + 1] = sP[3 * na + 1]; a.out_poses[3 * r + 2] = sP[3 * na + 2];
        } else {
            const int nb = sCorner[q + 1];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double A = sP[3 * na + k], B = sP[3 * nb + k];
                a.out_poses[3 * r + k] = (float)(A + (B - A) * f);
            }
        }
        a.row_node[r] = t == 0 ? na : -1;
        if (!a.quats) continue;
        double o[4];
        if (t == 0 && path_kept(a, na)) {
            path_unit_quat(a.quats + 4 * na, o);
        } else {   // (na < L - 1 here: the last row is kept)
            const int ka = sLast[na], kb = sNext[na + 1];
            const int pa = sPos[ka], pb = sPos[kb];
            const double S = (double)(sD[pb] - sD[pa]);
            const double s = (double)(sD[q] - sD[pa]) + (double)(sD[q + 1] - sD[q]) * (double)t / (double)n;
            const double u = S > 0.0 ? s / S : 0.0;
            double qa[4], qb[4];
            path_unit_quat(a.quats + 4 * ka, qa);
            path_unit_quat(a.quats + 4 * kb, qb);
            const double dot = ((qa[0] * qb[0] + qa[1] * qb[1]) + qa[2] * qb[2]) + qa[3] * qb[3];
            const double sg = dot < 0.0 ? -1.0 : 1.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (1.0 - u) * qa[k] + u * (sg * qb[k]);
            const double nn = sqrt(((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = o[k] / nn;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a.out_quats[4 * r + k] = (float)o[k];
    }
}

}  // namespace

extern "C" size_t tohip_path_bytes(int64_t n_nodes, int64_t max_rows) {
    return path_sizes_ok(n_nodes, max_rows) ? path_layout(n_nodes, max_rows).total : 0;
}

extern "C" int tohip_path_refine(const float* nodes, const float* quats, const uint8_t* keep, int64_t n_nodes, int64_t window,
                                 const uint8_t* open_band, float spacing, int64_t max_rows, void* buf, size_t bytes, void* stream) {
    if (!nodes || !open_band || !buf || !path_sizes_ok(n_nodes, max_rows) || window < 1 || window > n_nodes - 1 || !(spacing >= 0.f) ||
        !std::isfinite(spacing))
        return TOHIP_EINVAL;   // (a NaN fails the compare)
    const PathLayout l = path_layout(n_nodes, max_rows);
    if (bytes < l.total) return TOHIP_ENOSPC;
    char* b = (char*)buf;
    PathArgs a;
    a.P = nodes; a.quats = quats; a.keep = keep; a.band = open_band;
    a.L = (int)n_nodes; a.W = (int)window; a.max_rows = (int)max_rows;
    a.H = 0;
    if (spacing > 0.f) {
        const double h = (double)spacing * 1048576.0;
        a.H = h < (double)kPathMaxStep ? llrint(h) : kPathMaxStep;
        if (a.H < 1) a.H = 1;
    }
    a.hdr = (long long*)b; a.D = (long long*)(b + l.off_D); a.pred = (int*)(b + l.off_pred); a.corner = (int*)(b + l.off_corner);
    a.out_poses = (float*)(b + l.off_poses); a.out_quats = (float*)(b + l.off_quats); a.row_node = (int*)(b + l.off_row_node);
    k_path_refine<<<1, kPathBlock, 0, (hipStream_t)stream>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
