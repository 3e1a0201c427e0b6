// propose_kernels.hip — candidate views from free positions (tools.propose_views), for gfx950.
//
// For every position t (M of them) and every cloud point x the PAIR TEST, all f32 without contraction:
//   d = fl(x - t);  hh = fl(fl(dx dx) + fl(dy dy)), zz = fl(dz dz), r2 = fl(hh + zz)
//   range gate      fl(min min) <= r2 <= fl(max max)           (on range, not on camera depth)
//   elevation gate  zz <= fl(fl(tan_v tan_v) hh)               (a level camera's vertical field of view)
//   quadrant q and (a, b):  q0: dx > 0, dy >= 0 -> (dx, dy);  q1: dx <= 0, dy > 0 -> (dy, -dx);  q2: dx < 0, dy <= 0 -> (-dx, -dy);
//                           q3: dx >= 0, dy < 0 -> (-dy, dx)   (dx = dy = 0 has none; the gates have excluded it already)
//   sector = q S/4 + #{k in 1..S/4-1 : fl(b c_k) >= fl(a s_k)},  c_k = (float)cos(2 pi k / S), s_k = (float)sin(2 pi k / S) from the host
// hist[t][j] = the sum of the integer weights of the points that pass both gates from t and fall into sector j (bearings
// [2 pi j / S, 2 pi (j + 1) / S) about +z).  Rows with a coordinate that is not finite and pads never count; a position that is not
// finite or not open counts nothing.  Sums are integers: the same bits in every run and for every order of the points.
//
//   k_view_hist      grid (tiles of 64 positions) x (runs of cloud tiles).  Lane l of every wave holds position l of the block's tile;
//                    a wave takes every fourth 256-point tile of the run.  Per tile one ballot says which of the 64 positions the
//                    tile's bounding sphere can reach — the sphere is dropped for a position when it lies wholly beyond max_dist or
//                    wholly inside min_dist of it, with clr_search's slack; a sphere that is not finite is kept — and the wave walks
//                    the set bits: the position comes out of its lane by a uniform read (SGPRs), each lane tests its 4 points
//                    against it with the EXACT gates, so the prune never changes a bit.  The count over the boundary table is a
//                    binary search (the predicates are monotone in k for gated points).  A hit is one ds add into the block's
//                    LDS histogram of 64 x S 32-bit words; a block sees at most 256 tiles = 65 536 points of weight <= 32 768, so a
//                    word stays below 2^32.  The non-zero words are flushed with 64-bit integer atomic adds.  No float atomics.
//   k_view_headings  one wave per position, <= 2 bins per lane: circular window sums score[h] = sum_{|j| <= hw} hist[(h + j) mod S]
//                    through the wave's LDS row, then n_per rounds of: argmax over the unsuppressed h with score >= max(min_score, 1),
//                    ties to the lowest h; suppress every h within sep (circular) of it.  Slots no round fills: heading -1, score 0.
#include <climits>

namespace {

constexpr int kVhWaves = 4;        // waves per block of k_view_hist
constexpr int kVhP = 64;           // positions per block: one per lane of the prune's ballot
constexpr int kVhMaxTiles = 256;   // 256-point tiles per block: 65 536 points x 32 768 = 2^31 < 2^32
constexpr int kVhMaxQ = TOHIP_VIEW_MAX_SECTORS / 4;
constexpr int kVhdWaves = 4;       // positions (waves) per block of k_view_headings

struct ViewHistArgs {
    CloudView cv;
    const float* pos;              // (M, 3)
    const unsigned char* open;     // (M)
    const int* weights;            // (n) in the caller's order, or NULL: every point weighs 1
    int M, tiles_per_run, prune;
    float min_d, max_d, min2, max2, tv2;
    unsigned long long* hist;      // (M, S), zero on entry
    float c[kVhMaxQ], s[kVhMaxQ];  // entries 1..S/4-1
};

template <int S>
__device__ __forceinline__ void vh_pair(float tx, float ty, float tz, float x, float y, float z, unsigned w, float min2, float max2, float tv2,
                                        const float* sc, const float* ss, unsigned* row) {
    constexpr int Q = S / 4;
    if (!w) return;
    const float dx = __fsub_rn(x, tx), dy = __fsub_rn(y, ty), dz = __fsub_rn(z, tz);
    const float hh = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), zz = __fmul_rn(dz, dz);
    const float r2 = __fadd_rn(hh, zz);
    if (!(r2 >= min2 && r2 <= max2)) return;
    if (!(zz <= __fmul_rn(tv2, hh))) return;
    int q;
    float a, b;
    if (dx > 0.f && dy >= 0.f) { q = 0; a = dx; b = dy; }
    else if (dx <= 0.f && dy > 0.f) { q = 1; a = dy; b = -dx; }
    else if (dx < 0.f && dy <= 0.f) { q = 2; a = -dx; b = -dy; }
    else if (dx >= 0.f && dy < 0.f) { q = 3; a = -dy; b = dx; }
    else return;
    int cnt = 0;   // the predicates hold for k <= cnt: the count is the largest k that holds
#pragma unroll
    for (int step = Q / 2; step >= 1; step >>= 1) {
        const int k = cnt + step;
        if (__fmul_rn(b, sc[k]) >= __fmul_rn(a, ss[k])) cnt = k;
    }
    atomicAdd(&row[q * Q + cnt], w);
}

template <int S>
__global__ void __launch_bounds__(64 * kVhWaves) k_view_hist(ViewHistArgs a) {
    constexpr int Q = S / 4;
    __shared__ unsigned sh[kVhP * S];
    __shared__ float sc[Q], ss[Q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < kVhP * S; i += 64 * kVhWaves) sh[i] = 0u;
    if (tid < Q) { sc[tid] = a.c[tid]; ss[tid] = a.s[tid]; }
    const int p0 = blockIdx.x * kVhP, pi = p0 + lane;
    float px = 0.f, py = 0.f, pz = 0.f;
    bool live = false;
    if (pi < a.M) {
        px = a.pos[3 * pi], py = a.pos[3 * pi + 1], pz = a.pos[3 * pi + 2];
        live = a.open[pi] != 0 && finite3(px, py, pz);
    }
    __syncthreads();
    const unsigned long long live_mask = __ballot(live);   // the same in every wave
    if (live_mask) {
        const int64_t npad = a.cv.npad, n = a.cv.n;
        const int ntiles = (int)(npad / 256);
        const float* X = a.cv.soa;
        const float* Y = X + npad;
        const float* Z = Y + npad;
        const float pa = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
        const int t0 = (int)blockIdx.y * a.tiles_per_run;
        const int t1 = t0 + a.tiles_per_run < ntiles ? t0 + a.tiles_per_run : ntiles;
        for (int tile = t0 + wave; tile < t1; tile += kVhWaves) {
            unsigned long long mask = live_mask;
            if (a.prune) {
                const float4 b = a.cv.bounds[tile];
                bool keep = live;
                if (live && finite3(b.x, b.y, b.z) && isfinite(b.w)) {
                    const float dx = px - b.x, dy = py - b.y, dz = pz - b.z;
                    const float dc = sqrtf(dx * dx + dy * dy + dz * dz);
                    const float slack = 1e-5f * fmaxf(pa, fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fabsf(b.z))) + 1e-6f;
                    // dropped when every point of the sphere is beyond max_dist or nearer than min_dist, with room for the rounding of
                    // dc, of the sphere and of each point's r2; a dc that overflowed keeps the tile
                    if (isfinite(dc)) keep = !(dc > (b.w + a.max_d) * 1.0001f + slack) && !((dc + b.w) * 1.0001f + slack < a.min_d);
                }
                mask = __ballot(keep);
            }
            if (!mask) continue;   // (wave-uniform)
            const int64_t s0 = (int64_t)tile * 256 + 4 * lane;   // tile < ntiles: s0 + 3 < npad
            const float4 x4 = *(const float4*)(X + s0), y4 = *(const float4*)(Y + s0), z4 = *(const float4*)(Z + s0);
            const int4 i4 = *(const int4*)(a.cv.perm + s0);
            auto weight = [&](float x, float y, float z, int64_t s, int row) -> unsigned {
                if (s >= n || row < 0 || !finite3(x, y, z)) return 0u;
                return a.weights ? (unsigned)a.weights[row] : 1u;
            };
            const unsigned w0 = weight(x4.x, y4.x, z4.x, s0, i4.x), w1 = weight(x4.y, y4.y, z4.y, s0 + 1, i4.y);
            const unsigned w2 = weight(x4.z, y4.z, z4.z, s0 + 2, i4.z), w3 = weight(x4.w, y4.w, z4.w, s0 + 3, i4.w);
            if (!__ballot((w0 | w1 | w2 | w3) != 0u)) continue;
            while (mask) {
                const int k = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const float tx = __shfl(px, k), ty = __shfl(py, k), tz = __shfl(pz, k);   // k is uniform: scalar reads of lane k
                unsigned* row = sh + k * S;
                vh_pair<S>(tx, ty, tz, x4.x, y4.x, z4.x, w0, a.min2, a.max2, a.tv2, sc, ss, row);
                vh_pair<S>(tx, ty, tz, x4.y, y4.y, z4.y, w1, a.min2, a.max2, a.tv2, sc, ss, row);
                vh_pair<S>(tx, ty, tz, x4.z, y4.z, z4.z, w2, a.min2, a.max2, a.tv2, sc, ss, row);
                vh_pair<S>(tx, ty, tz, x4.w, y4.w, z4.w, w3, a.min2, a.max2, a.tv2, sc, ss, row);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < kVhP * S; i += 64 * kVhWaves) {
        const unsigned v = sh[i];
        const int p = p0 + i / S;
        if (v != 0u && p < a.M) atomicAdd(&a.hist[(size_t)p * S + (i % S)], (unsigned long long)v);
    }
}

template <int S>
inline void vh_launch(const ViewHistArgs& a, dim3 grid, hipStream_t st) {
    k_view_hist<S><<<grid, 64 * kVhWaves, 0, st>>>(a);
}

inline bool vh_sectors_ok(int32_t S) { return S == 8 || S == 16 || S == 32 || S == 64 || S == 128; }

__global__ void __launch_bounds__(64 * kVhdWaves)
k_view_headings(const long long* __restrict__ hist, int M, int S, int hw, int n_per, int sep, long long min_score, int* __restrict__ heading,
                long long* __restrict__ score) {
    __shared__ long long sh[kVhdWaves][TOHIP_VIEW_MAX_SECTORS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * kVhdWaves + wave;
    const bool live = c < M;
    const int h0 = lane, h1 = lane + 64;
    if (h0 < S) sh[wave][h0] = live ? hist[(size_t)c * S + h0] : 0;
    if (h1 < S) sh[wave][h1] = live ? hist[(size_t)c * S + h1] : 0;
    __syncthreads();
    if (!live) return;   // (wave-uniform; no barrier below)
    long long s0 = 0, s1 = 0;
    for (int j = -hw; j <= hw; ++j) {
        s0 += sh[wave][(h0 + j + S) & (S - 1)];   // S is a power of two; lanes with h >= S are never candidates
        s1 += sh[wave][(h1 + j + S) & (S - 1)];
    }
    const long long thr = min_score > 1 ? min_score : 1;
    bool open0 = h0 < S && s0 >= thr, open1 = h1 < S && s1 >= thr;
    int r = 0;
    for (; r < n_per; ++r) {
        long long bs = LLONG_MIN;
        int bh = INT_MAX;
        if (open0) { bs = s0; bh = h0; }
        if (open1 && s1 > bs) { bs = s1; bh = h1; }   // (a tie inside the lane stays with the lower heading)
        for (int m = 32; m > 0; m >>= 1) {
            const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(unsigned long long)bs, m);
            const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)bs >> 32), m);
            const long long os = (long long)(((unsigned long long)hi << 32) | lo);
            const int oh = __shfl_xor(bh, m);
            if (os > bs || (os == bs && oh < bh)) { bs = os; bh = oh; }
        }
        if (bh == INT_MAX) break;   // (uniform) nothing left
        if (lane == 0) { heading[(size_t)c * n_per + r] = bh; score[(size_t)c * n_per + r] = bs; }
        int d0 = h0 > bh ? h0 - bh : bh - h0, d1 = h1 > bh ? h1 - bh : bh - h1;
        d0 = d0 < S - d0 ? d0 : S - d0;
        d1 = d1 < S - d1 ? d1 : S - d1;
        open0 = open0 && d0 > sep;
        open1 = open1 && d1 > sep;
    }
    if (lane == 0)
        for (; r < n_per; ++r) { heading[(size_t)c * n_per + r] = -1; score[(size_t)c * n_per + r] = 0; }
}

}  // namespace

extern "C" int tohip_view_histogram(const void* packed, int64_t n_points, const float* positions, const uint8_t* open, int64_t n_positions,
                                    const int32_t* weights, int32_t sectors, const float* table_host, float min_dist, float max_dist, float tan_v,
                                    int32_t prune, int64_t* hist, void* stream) {
    if (!packed || !positions || !open || !table_host || !hist || n_points <= 0 || n_points > INT32_MAX || n_positions < 1 ||
        n_positions > TOHIP_VIEW_MAX_POSITIONS || !vh_sectors_ok(sectors))
        return TOHIP_EINVAL;
    if (!(std::isfinite(min_dist) && std::isfinite(max_dist) && min_dist >= 1e-3f && min_dist < max_dist && std::isfinite(tan_v) && tan_v >= 0.f))
        return TOHIP_EINVAL;
    const int Q = sectors / 4;
    for (int k = 0; k < 2 * (Q - 1); ++k)
        if (!std::isfinite(table_host[k])) return TOHIP_EINVAL;
    ViewHistArgs a;
    a.cv = cloud_view(packed, n_points);
    a.pos = positions; a.open = open; a.weights = weights;
    a.M = (int)n_positions; a.prune = prune != 0;
    a.min_d = min_dist; a.max_d = max_dist;
    a.min2 = min_dist * min_dist; a.max2 = max_dist * max_dist; a.tv2 = tan_v * tan_v;   // f32 products (no contraction in this unit)
    a.hist = (unsigned long long*)hist;
    for (int k = 0; k < kVhMaxQ; ++k) a.c[k] = a.s[k] = 0.f;
    for (int k = 1; k < Q; ++k) { a.c[k] = table_host[k - 1]; a.s[k] = table_host[Q - 1 + k - 1]; }
    // enough blocks to fill the chip several times over (the prune leaves them uneven), never more than kVhMaxTiles tiles to a block
    const int64_t ntiles = a.cv.npad / 256, ptiles = (n_positions + kVhP - 1) / kVhP;
    const int64_t want = (4096 + ptiles - 1) / ptiles;
    int64_t T = ((ntiles + want - 1) / want + kVhWaves - 1) / kVhWaves * kVhWaves;
    T = T < kVhWaves ? kVhWaves : (T > kVhMaxTiles ? kVhMaxTiles : T);
    a.tiles_per_run = (int)T;
    const dim3 grid((unsigned)ptiles, (unsigned)((ntiles + T - 1) / T));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n_positions * sectors * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    switch (sectors) {
        case 8: vh_launch<8>(a, grid, st); break;
        case 16: vh_launch<16>(a, grid, st); break;
        case 32: vh_launch<32>(a, grid, st); break;
        case 64: vh_launch<64>(a, grid, st); break;
        default: vh_launch<128>(a, grid, st); break;
    }
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_view_headings(const int64_t* hist, int64_t n_positions, int32_t sectors, int32_t half_window, int32_t n_per, int32_t sep,
                                   int64_t min_score, int32_t* heading, int64_t* score, void* stream) {
    if (!hist || !heading || !score || n_positions < 1 || n_positions > TOHIP_VIEW_MAX_POSITIONS || !vh_sectors_ok(sectors) || half_window < 0 ||
        2 * (int64_t)half_window + 1 > sectors || n_per < 1 || n_per > TOHIP_VIEW_MAX_PER_POSITION || sep < 0 || sep > sectors || min_score < 0)
        return TOHIP_EINVAL;
    const int M = (int)n_positions;
    k_view_headings<<<(unsigned)((M + kVhdWaves - 1) / kVhdWaves), 64 * kVhdWaves, 0, (hipStream_t)stream>>>(
        (const long long*)hist, M, sectors, half_window, n_per, sep, (long long)min_score, heading, (long long*)score);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
