// views_kernels.hip — greedy view selection: choose the best k of M candidate views on the device, for gfx950.
//
// A candidate view's log-odds row (tohip_traj_forward_multi, the candidate as a trajectory of one body waypoint) is non-zero on a
// fraction of a percent of the cloud.  The rows are kept as ONE CSR structure — per candidate its (packed index, log-odds) pairs in
// ascending index order — and a greedy round touches those entries only:
//
//   k_views_count / k_views_scan / k_views_write   compaction of a chunk of dense rows (count per 8 192-point segment, one-block
//                        scan + capacity check, ordered write).  A row that holds a NaN makes its candidate ABSENT: no entries.
//   k_views_gain         every stored entry against S (the chosen views' summed log-odds) and the prior: the two rewards with the
//                        reward kernel's expression, their fixed-point difference, summed per candidate — entries, not candidates, are
//                        dealt to the waves (a contiguous run each), wave shuffles, one 64-bit integer atomic per (wave, candidate)
//   k_views_pick         one block: argmax with ties to the lowest index, the stop rules, the outputs, S += the winner's list, the
//                        reset of the sums.  Once stopped, both kernels return on the header's flag (opt_step.hpp's pattern).
//
// No float atomics: a gain is an integer sum, the same in every run; S is the f32 sum of the chosen rows in selection order.
//
// Buffer (tohip_views_bytes), every section aligned to 256 B:
//   [header: 32 x i64 — [0] entries stored [1] entries needed by everything appended [2] status (bit 0: capacity exceeded, bit 1: an
//    append out of sequence) [3] candidates appended [4] the running selection has stopped]
//   [offsets (M + 1) i64] [absent M i32] [gain sums M i64] [chosen M i32] [segment counts 256 x nseg i32] [idx cap u32] [val cap f32]
#include <climits>
#include <cmath>

namespace {

constexpr size_t kViewsHdr = 256;
constexpr int kViewsSeg = 8192;            // points per compaction block: 256 threads x 32 consecutive points (one 128-byte line each)
constexpr int kViewsGainBlocks = 1024;     // x 4 waves: the runs the entries are dealt into (256 CUs x 4 blocks)

struct ViewsLayout {
    size_t off_offsets, off_absent, off_gain, off_chosen, off_blk, off_idx, off_val, total;
    int64_t nseg;
};

inline bool views_sizes_ok(int64_t n, int64_t M, int64_t cap) {
    return n > 0 && n <= (int64_t)1 << 30 && M > 0 && M <= TOHIP_VIEWS_MAX_CANDIDATES && cap > 0 && cap <= (int64_t)1 << 40;
}

inline ViewsLayout views_layout(int64_t n, int64_t M, int64_t cap) {
    ViewsLayout l;
    l.nseg = (tohip_padded_points(n) + kViewsSeg - 1) / kViewsSeg;
    size_t o = kViewsHdr;
    l.off_offsets = o; o += align_up((size_t)(M + 1) * 8, 256);
    l.off_absent = o;  o += align_up((size_t)M * 4, 256);
    l.off_gain = o;    o += align_up((size_t)M * 8, 256);
    l.off_chosen = o;  o += align_up((size_t)M * 4, 256);
    l.off_blk = o;     o += align_up((size_t)TOHIP_VIEWS_MAX_CHUNK * l.nseg * 4, 256);
    l.off_idx = o;     o += align_up((size_t)cap * 4, 256);
    l.off_val = o;     o += align_up((size_t)cap * 4, 256);
    l.total = o;
    return l;
}

struct ViewsPtrs {
    long long* hdr;
    long long* offsets;
    int* absent;
    long long* gain;
    int* chosen;
    int* blk;
    unsigned* idx;
    float* val;
};

inline ViewsPtrs views_ptrs(void* buf, const ViewsLayout& l) {
    char* b = (char*)buf;
    return ViewsPtrs{(long long*)b, (long long*)(b + l.off_offsets), (int*)(b + l.off_absent), (long long*)(b + l.off_gain),
                     (int*)(b + l.off_chosen), (int*)(b + l.off_blk), (unsigned*)(b + l.off_idx), (float*)(b + l.off_val)};
}

// the 32 consecutive points of thread t in segment s of a row: entries > 0 below n are stored; a NaN marks the row
__device__ __forceinline__ int views_load32(const float* __restrict__ row, int64_t i0, int64_t n, int64_t npad, float v[32], bool& nan_) {
    int c = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int64_t i = i0 + 4 * q;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < npad) f = *reinterpret_cast<const float4*>(row + i);   // npad is a multiple of 2048: whole quads, aligned
        const float w[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i + j < n;       // pads are not points
            const float x = in ? w[j] : 0.f;
            if (x != x) nan_ = true;
            v[4 * q + j] = x;
            c += (x > 0.f) ? 1 : 0;
        }
    }
    return c;
}

// grid (nseg, T): blk[t * nseg + s] = the entries row t has in segment s; absent[t] |= 1 when the row holds a NaN
__global__ void __launch_bounds__(256)
k_views_count(const float* __restrict__ lo, int64_t n, int64_t npad, int nseg, int* __restrict__ blk, int* __restrict__ absent) {
    __shared__ int part[4];
    const int s = blockIdx.x, t = blockIdx.y;
    const float* row = lo + (int64_t)t * npad;
    float v[32];
    bool nan_ = false;
    int c = views_load32(row, (int64_t)s * kViewsSeg + (int64_t)threadIdx.x * 32, n, npad, v, nan_);
    for (int sh = 32; sh > 0; sh >>= 1) c += __shfl_xor(c, sh);
    nan_ = __any(nan_);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        part[wave] = c;
        if (nan_) atomicOr(absent + t, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) blk[(int64_t)t * nseg + s] = part[0] + part[1] + part[2] + part[3];
}

// one block: the segment counts of each row become exclusive prefixes, the rows' totals are appended to `offsets` — unless the
// capacity does not hold them, or the chunk does not continue the set: then only the needed count and the status change
__global__ void __launch_bounds__(TOHIP_VIEWS_MAX_CHUNK)
k_views_scan(int* __restrict__ blk, int nseg, int T, int64_t first, int64_t cap, long long* __restrict__ hdr, long long* __restrict__ offsets,
             const int* __restrict__ absent) {
    __shared__ long long tot[TOHIP_VIEWS_MAX_CHUNK];
    const int t = threadIdx.x;
    if (t < T) {
        int run = 0;
        for (int s = 0; s < nseg; ++s) {
            const int c = blk[(int64_t)t * nseg + s];
            blk[(int64_t)t * nseg + s] = run;
            run += c;
        }
        tot[t] = absent[t] ? 0 : run;
    }
    __syncthreads();
    if (t != 0) return;
    const bool restart = first == 0;   // the first chunk starts the set anew
    const long long base = restart ? 0 : hdr[0];
    long long needed = restart ? 0 : hdr[1];
    long long status = restart ? 0 : hdr[2];
    if (!restart && status == 0 && hdr[3] != first) status |= 2;   // (a set that did not fit no longer advances: its chunks still count)
    long long chunk = 0;
    for (int r = 0; r < T; ++r) chunk += tot[r];
    needed += chunk;
    if (base + chunk > cap) status |= 1;
    if (status == 0) {
        long long run = base;
        offsets[first] = run;
        for (int r = 0; r < T; ++r) { run += tot[r]; offsets[first + r + 1] = run; }
        hdr[0] = run;
        hdr[3] = first + T;
    } else if (restart) {
        hdr[0] = 0;
        hdr[3] = 0;
    }
    hdr[1] = needed;
    hdr[2] = status;
    hdr[4] = 0;
}

// grid (nseg, T): row t's entries of segment s, in ascending index order, behind those of the segments before it
__global__ void __launch_bounds__(256)
k_views_write(const float* __restrict__ lo, int64_t n, int64_t npad, int nseg, const int* __restrict__ blk, const int* __restrict__ absent,
              const long long* __restrict__ hdr, const long long* __restrict__ offsets, unsigned* __restrict__ idx, float* __restrict__ val) {
    __shared__ int part[4];
    const int s = blockIdx.x, t = blockIdx.y;
    if (hdr[2] != 0 || absent[t]) return;   // (uniform) nothing of a set that did not fit, or of an absent candidate, is written
    const float* row = lo + (int64_t)t * npad;
    const int64_t i0 = (int64_t)s * kViewsSeg + (int64_t)threadIdx.x * 32;
    float v[32];
    bool nan_ = false;
    const int c = views_load32(row, i0, n, npad, v, nan_);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = c;   // inclusive scan over the wave, then over the four waves
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int before = inc - c;
    for (int w = 0; w < wave; ++w) before += part[w];
    int64_t e = offsets[t] + blk[(int64_t)t * nseg + s] + before;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (v[j] > 0.f) {
            idx[e] = (unsigned)(i0 + j);
            val[e] = v[j];
            ++e;
        }
    }
}

// the reward of one packed point as k_traj_reward / k_traj_reward_prior take it (reward_block), in fixed point
__device__ __forceinline__ long long views_fixed(float lo, float p, bool prior, int shift) {
    const float lt = prior ? lo + p : lo;
    return reward_fixed(reward_sigmoid(lt), shift);
}

__device__ __forceinline__ void views_flush(long long acc, int c, long long* __restrict__ gain) {
    for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh);
    if ((threadIdx.x & 63) == 0 && c >= 0 && acc != 0) atomicAdd(reinterpret_cast<unsigned long long*>(gain + c), (unsigned long long)acc);
}

// wave w of all takes the entries [w L, (w + 1) L): gain[c] += sum over c's entries of fixed(r(S + lo)) - fixed(r(S))
__global__ void __launch_bounds__(256)
k_views_gain(const long long* __restrict__ hdr, const long long* __restrict__ offsets, const int* __restrict__ chosen, int M,
             const unsigned* __restrict__ idx, const float* __restrict__ val, const float* __restrict__ S, const float* __restrict__ prior,
             int shift, long long* __restrict__ gain) {
    if (hdr[4] != 0 || hdr[2] != 0 || hdr[3] != M) return;   // stopped, or not a set to select from (uniform)
    const long long nnz = hdr[0];
    const long long nwaves = (long long)gridDim.x * 4;
    long long L = (nnz + nwaves - 1) / nwaves;
    L = (L + 63) / 64 * 64;
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long start = gw * L;
    if (start >= nnz) return;
    const long long end = start + L < nnz ? start + L : nnz;
    // the candidate of the first entry: the smallest c with offsets[c + 1] > start
    int lo_c = 0, hi_c = M - 1;
    while (lo_c < hi_c) {
        const int mid = (lo_c + hi_c) >> 1;
        if (offsets[mid + 1] > start) hi_c = mid; else lo_c = mid + 1;
    }
    int c0 = lo_c;
    long long c0_end = offsets[c0 + 1];
    int cur = -1;        // the candidate `acc` belongs to
    bool skip = false;   //   ... and whether it is chosen already
    long long acc = 0;
    const bool has_prior = prior != nullptr;
    for (long long e0 = start; e0 < end; e0 += 64) {
        while (e0 >= c0_end) { ++c0; c0_end = offsets[c0 + 1]; }   // (uniform; e0 < nnz = offsets[M])
        const long long e = e0 + lane;
        const bool valid = e < end;
        const long long last = (e0 + 64 < end ? e0 + 64 : end) - 1;
        if (last < c0_end) {   // the common case: the 64 entries are one candidate's
            if (c0 != cur) {
                views_flush(acc, cur, gain);
                acc = 0; cur = c0; skip = chosen[c0] != 0;
            }
            if (valid && !skip) {
                const unsigned i = idx[e];
                const float v = val[e], s = S[i], p = has_prior ? prior[i] : 0.f;
                acc += views_fixed(s + v, p, has_prior, shift) - views_fixed(s, p, has_prior, shift);
            }
            continue;
        }
        // a candidate ends among them: each lane finds its own, and the wave sums candidate by candidate
        views_flush(acc, cur, gain);
        acc = 0; cur = -1;
        int c = c0;
        long long d = 0;
        if (valid) {
            while (e >= offsets[c + 1]) ++c;
            if (!chosen[c]) {
                const unsigned i = idx[e];
                const float v = val[e], s = S[i], p = has_prior ? prior[i] : 0.f;
                d = views_fixed(s + v, p, has_prior, shift) - views_fixed(s, p, has_prior, shift);
            }
        } else {
            c = 0x7fffffff;
        }
        for (;;) {
            int cmin = c;
            for (int sh = 32; sh > 0; sh >>= 1) { const int o = __shfl_xor(cmin, sh); cmin = o < cmin ? o : cmin; }
            if (cmin == 0x7fffffff) break;
            views_flush(c == cmin ? d : 0ll, cmin, gain);
            if (c == cmin) c = 0x7fffffff;
        }
    }
    views_flush(acc, cur, gain);
}

struct ViewsPick {
    long long* hdr;
    const long long* offsets;
    const int* absent;
    int* chosen;
    long long* gain;
    const unsigned* idx;
    const float* val;
    float* S;
    int32_t* order;
    int64_t* gain_out;
    int32_t* n_selected;
    double min_gain, scale;   // scale = 2^shift
    int64_t n;
    int M, round;
};

__global__ void __launch_bounds__(1024) k_views_pick(ViewsPick a) {
    __shared__ long long bg[16];
    __shared__ int bc[16];
    if (a.hdr[4] != 0) return;   // (uniform)
    const int t = threadIdx.x;
    const bool usable = a.hdr[2] == 0 && a.hdr[3] == a.M;
    long long g = LLONG_MIN;
    int c = 0x7fffffff;
    if (usable) {
        for (int m = t; m < a.M; m += 1024) {   // ascending: a later equal gain does not replace an earlier one
            if (a.chosen[m] || a.absent[m]) continue;
            const long long gm = a.gain[m];
            if (gm > g) { g = gm; c = m; }
        }
    }
    for (int sh = 32; sh > 0; sh >>= 1) {
        const long long og = __shfl_xor(g, sh);
        const int oc = __shfl_xor(c, sh);
        if (og > g || (og == g && oc < c)) { g = og; c = oc; }
    }
    if ((t & 63) == 0) { bg[t >> 6] = g; bc[t >> 6] = c; }
    __syncthreads();
    g = bg[0]; c = bc[0];
    for (int w = 1; w < 16; ++w)
        if (bg[w] > g || (bg[w] == g && bc[w] < c)) { g = bg[w]; c = bc[w]; }
    const bool stop = c == 0x7fffffff || g <= 0 || (double)g / a.scale / (double)a.n < a.min_gain;
    if (stop) {
        if (t == 0) a.hdr[4] = 1;
        return;
    }
    if (t == 0) {
        a.order[a.round] = c;
        a.gain_out[a.round] = g;
        a.n_selected[0] = a.round + 1;
        a.chosen[c] = 1;
    }
    const long long e1 = a.offsets[c + 1];
    for (long long e = a.offsets[c] + t; e < e1; e += 1024) {   // the indices of a list are distinct: plain stores
        const unsigned i = a.idx[e];
        a.S[i] = a.S[i] + a.val[e];
    }
    for (int m = t; m < a.M; m += 1024) a.gain[m] = 0;
}

// row[0..npad) = candidate c's list scattered (the caller zero-filled it); an absent candidate: NaN at every point
__global__ void __launch_bounds__(256)
k_views_row(const long long* __restrict__ hdr, const long long* __restrict__ offsets, const int* __restrict__ absent, int64_t c, int64_t n,
            const unsigned* __restrict__ idx, const float* __restrict__ val, float* __restrict__ row) {
    if (hdr[2] != 0 || c >= hdr[3]) return;
    const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (absent[c]) {
        for (int64_t i = t0; i < n; i += stride) row[i] = __builtin_nanf("");
        return;
    }
    const long long e1 = offsets[c + 1];
    for (long long e = offsets[c] + t0; e < e1; e += stride) row[idx[e]] = val[e];
}

}  // namespace

extern "C" size_t tohip_views_bytes(int64_t n_points, int64_t n_candidates, int64_t nnz_capacity) {
    return views_sizes_ok(n_points, n_candidates, nnz_capacity) ? views_layout(n_points, n_candidates, nnz_capacity).total : 0;
}

extern "C" int tohip_views_append(void* views, size_t views_bytes, int64_t n, int64_t M, int64_t cap, const float* lo_rows, int64_t first,
                                  int64_t n_rows, int64_t* needed_host, void* stream_) {
    if (!views || !lo_rows || !views_sizes_ok(n, M, cap) || first < 0 || n_rows <= 0 || n_rows > TOHIP_VIEWS_MAX_CHUNK) return TOHIP_EINVAL;
    if (first + n_rows > M) return TOHIP_ENOSPC;
    const ViewsLayout l = views_layout(n, M, cap);
    if (views_bytes < l.total) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const ViewsPtrs p = views_ptrs(views, l);
    const int64_t npad = tohip_padded_points(n);
    const int nseg = (int)l.nseg, T = (int)n_rows;
    hipError_t e = hipMemsetAsync(p.absent + first, 0, (size_t)T * 4, st);
    if (e != hipSuccess) return (int)e;
    k_views_count<<<dim3(nseg, T), 256, 0, st>>>(lo_rows, n, npad, nseg, p.blk, p.absent + first);
    TO_HIP_CHECK_LAUNCH();
    k_views_scan<<<1, TOHIP_VIEWS_MAX_CHUNK, 0, st>>>(p.blk, nseg, T, first, cap, p.hdr, p.offsets, p.absent + first);
    TO_HIP_CHECK_LAUNCH();
    k_views_write<<<dim3(nseg, T), 256, 0, st>>>(lo_rows, n, npad, nseg, p.blk, p.absent + first, p.hdr, p.offsets + first, p.idx, p.val);
    TO_HIP_CHECK_LAUNCH();
    if (!needed_host) return TOHIP_OK;
    long long h[4];
    e = hipMemcpyAsync(h, p.hdr, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    *needed_host = h[1];
    if (h[2] & 2) return TOHIP_EINVAL;
    return (h[2] & 1) ? TOHIP_ENOSPC : TOHIP_OK;
}

extern "C" int tohip_views_select(void* views, size_t views_bytes, int64_t n, int64_t M, int64_t cap, const void* prior_buf, int64_t k,
                                  double min_gain, float* S, int32_t* order, int64_t* gain_fixed, int32_t* n_selected, void* stream_) {
    if (!views || !S || !order || !gain_fixed || !n_selected || !views_sizes_ok(n, M, cap) || k <= 0 || k > M || !(min_gain >= 0.0) ||
        !std::isfinite(min_gain))
        return TOHIP_EINVAL;
    const ViewsLayout l = views_layout(n, M, cap);
    if (views_bytes < l.total) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const ViewsPtrs p = views_ptrs(views, l);
    const int64_t npad = tohip_padded_points(n);
    hipError_t e = hipMemsetAsync(S, 0, (size_t)npad * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p.gain, 0, (size_t)M * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(p.chosen, 0, (size_t)M * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p.hdr + 4, 0, 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(n_selected, 0, 4, st);
    if (e != hipSuccess) return (int)e;
    const float* prior = prior_buf ? prior_view(prior_buf, n).prior : nullptr;
    const int shift = reward_shift(n);
    ViewsPick a;
    a.hdr = p.hdr; a.offsets = p.offsets; a.absent = p.absent; a.chosen = p.chosen; a.gain = p.gain; a.idx = p.idx; a.val = p.val;
    a.S = S; a.order = order; a.gain_out = gain_fixed; a.n_selected = n_selected;
    a.min_gain = min_gain; a.scale = std::ldexp(1.0, shift); a.n = n; a.M = (int)M;
    for (int64_t j = 0; j < k; ++j) {
        k_views_gain<<<kViewsGainBlocks, 256, 0, st>>>(p.hdr, p.offsets, p.chosen, (int)M, p.idx, p.val, S, prior, shift, p.gain);
        TO_HIP_CHECK_LAUNCH();
        a.round = (int)j;
        k_views_pick<<<1, 1024, 0, st>>>(a);
        TO_HIP_CHECK_LAUNCH();
    }
    return TOHIP_OK;
}

extern "C" int tohip_views_row(const void* views, size_t views_bytes, int64_t n, int64_t M, int64_t cap, int64_t candidate, float* row,
                               void* stream_) {
    if (!views || !row || !views_sizes_ok(n, M, cap) || candidate < 0 || candidate >= M) return TOHIP_EINVAL;
    const ViewsLayout l = views_layout(n, M, cap);
    if (views_bytes < l.total) return TOHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream_;
    const ViewsPtrs p = views_ptrs(const_cast<void*>(views), l);
    const hipError_t e = hipMemsetAsync(row, 0, (size_t)tohip_padded_points(n) * 4, st);
    if (e != hipSuccess) return (int)e;
    k_views_row<<<64, 256, 0, st>>>(p.hdr, p.offsets, p.absent, candidate, n, p.idx, p.val, row);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
