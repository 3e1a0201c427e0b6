// covmap_kernels.hip — a device-resident, voxel-keyed log-odds map, for gfx950.
//
// What has been seen, keyed by position instead of by row of one cloud: a coverage row (tohip_traj_coverage) is folded into a hash
// table of voxels, and any later cloud — other rows, another count, another order — reads its prior back from it.
//
//   key of a point   per axis i = (int) floorf((x - origin) / r), all f32 (the division correctly rounded: numpy.float32 gives the
//                    same index); the three indices biased by 2^20 and packed 21 bits each, x highest; all ones = an empty slot.
//                    A non-finite coordinate or an index outside [-2^20, 2^20) makes the point SKIPPED.
//   k_covmap_integrate   one streaming pass over points and row: the slot of the point's voxel is found or claimed (64-bit
//                    compare-and-swap on the key) and the observation folded into the slot's `pending` word with a 32-bit integer
//                    atomic max (values are >= 0: their bit patterns order as unsigned integers).  Runs of equal keys in neighbouring
//                    lanes — a Morton-sorted or voxel-filtered cloud — are folded inside the wave first; only a run's head lane probes.
//   k_covmap_rehash  the live slots of another table as observations: merge, and the growth of a table.
//   k_covmap_commit  over the slots: value = min(rule(value, pending), clamp), pending = 0 — one f32 operation per voxel and call,
//                    whatever the order the points came in.  A call that would leave the table above half full is rolled back here:
//                    the slots it claimed become empty again and only the status and the needed count remain of it.
//   k_covmap_lookup  key, probe, one 4-byte store per point.
//   k_covmap_export  the live slots, compacted with one cursor add per wave (the host sorts by key: the order here means nothing).
//
// A slot claimed during a call keeps value = kCovFresh (all ones, no f32 a map can hold) until the commit: that is how the commit tells
// the slots of this call from the ones before it.  Removing exactly those restores the table as it was: every older key was placed
// when none of them existed.  No float atomics; nothing observable depends on the slot a key lands in.
//
// Buffer (tohip_covmap_bytes): [header 256 B][capacity x slot 16 B: u64 key | f32 value | u32 pending]
//   header, int64 words: [0] voxels held [1] capacity [2] status of the last integrate / merge / rehash (bit 0: it would have left
//   the table above half full, bit 1: a probe gave up — [3] is then a lower bound, bit 2: merge of maps whose origin or resolution
//   differ) [3] voxels the map holds, or would have to, after that call [4] points it skipped [5] rows it skipped for their
//   log-odds (negative or non-finite) [6] slots it claimed [7] export cursor; f32 at byte 64: origin x y z, resolution, clamp_max.
#include <cmath>

namespace {

constexpr size_t kCovHdr = 256;
constexpr unsigned long long kCovEmpty = ~0ull;
constexpr unsigned kCovFresh = 0xffffffffu;
constexpr int kCovBias = 1 << 20;
constexpr int kCovProbeLimit = 256;    // a table at most half full has no run of this length (P ~ e^-49 per slot): longer = overfull
constexpr int kCovBlocks = 2048;       // 256 CUs x 8 blocks of 256: every kernel strides over its input with this grid at most

struct __attribute__((aligned(16))) CovSlot {
    unsigned long long key;
    unsigned value;     // f32 bits; kCovFresh while the call that claimed the slot runs
    unsigned pending;   // f32 bits of the call's observation (max over its points)
};

struct CovGeom { float ox, oy, oz, r, clamp; };

inline bool covmap_capacity_ok(int64_t cap) { return cap >= 16 && cap <= (int64_t)1 << 32 && (cap & (cap - 1)) == 0; }

__device__ __forceinline__ CovGeom cov_geom(const long long* __restrict__ hdr) {
    const float* g = reinterpret_cast<const float*>(hdr + 8);
    return CovGeom{g[0], g[1], g[2], g[3], g[4]};
}

__device__ __forceinline__ bool cov_axis(float x, float o, float r, unsigned long long& i) {
    const float f = floorf((x - o) / r);
    const bool ok = f >= -(float)kCovBias && f < (float)kCovBias;   // (false for NaN)
    i = (unsigned long long)((ok ? (int)f : 0) + kCovBias);
    return ok;
}

__device__ __forceinline__ unsigned long long cov_key(float x, float y, float z, const CovGeom& g) {
    unsigned long long ix, iy, iz;
    const bool ok = cov_axis(x, g.ox, g.r, ix) & cov_axis(y, g.oy, g.r, iy) & cov_axis(z, g.oz, g.r, iz);
    return ok ? (ix << 42) | (iy << 21) | iz : kCovEmpty;
}

__device__ __forceinline__ unsigned long long cov_hash(unsigned long long k) {   // (splitmix64's finaliser)
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}

__device__ __forceinline__ uint4 cov_load(const CovSlot* s) { return *reinterpret_cast<const uint4*>(s); }
__device__ __forceinline__ unsigned long long cov_slot_key(const uint4& v) { return ((unsigned long long)v.y << 32) | v.x; }

__device__ __forceinline__ long long cov_status(const long long* hdr) {
    return __hip_atomic_load(hdr + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slot of `key`, claimed when the table does not hold it (claimed = true then); -1 when the probe gives up (status bit 1 is set)
__device__ __forceinline__ long long cov_insert(CovSlot* __restrict__ slots, unsigned long long mask, unsigned long long key, long long* hdr,
                                                bool& claimed) {
    unsigned long long s = cov_hash(key) & mask;
    const unsigned long long limit = mask + 1 < (unsigned long long)kCovProbeLimit ? mask + 1 : (unsigned long long)kCovProbeLimit;
    for (unsigned long long p = 0; p < limit; ++p, s = (s + 1) & mask) {
        // (the key alone, as one 64-bit atomic load: it races with the other lanes' compare-and-swaps)
        unsigned long long k = __hip_atomic_load(&slots[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kCovEmpty) {
            unsigned long long expected = kCovEmpty;
            if (__hip_atomic_compare_exchange_strong(&slots[s].key, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                claimed = true;
                return (long long)s;
            }
            k = expected;
        }
        if (k == key) return (long long)s;
        if ((p & 63) == 63 && (cov_status(hdr) & 2)) return -1;
    }
    __hip_atomic_fetch_or(reinterpret_cast<unsigned long long*>(hdr + 2), 2ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return -1;
}

__device__ __forceinline__ void cov_fold(CovSlot* __restrict__ slots, long long s, unsigned obs) {
    if (obs != 0) __hip_atomic_fetch_max(&slots[s].pending, obs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void cov_count(long long* hdr, int word, long long c) {
    for (int sh = 32; sh > 0; sh >>= 1) c += __shfl_xor(c, sh);
    if ((threadIdx.x & 63) == 0 && c != 0)
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(hdr + word), (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) k_covmap_init(long long* __restrict__ hdr, CovSlot* __restrict__ slots, long long cap, CovGeom g) {
    const long long stride = (long long)gridDim.x * 256, t0 = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long s = t0; s < cap; s += stride) *reinterpret_cast<uint4*>(slots + s) = make_uint4(~0u, ~0u, kCovFresh, 0u);
    if (t0 < 32) hdr[t0] = t0 == 1 ? cap : 0;
    __syncthreads();   // (t0 < 32 are all in block 0: the floats go over words 8..10 after the zeros)
    if (t0 == 0) {
        float* f = reinterpret_cast<float*>(hdr + 8);
        f[0] = g.ox; f[1] = g.oy; f[2] = g.oz; f[3] = g.r; f[4] = g.clamp;
    }
}

// FOLD: the observation of a run of equal keys in consecutive lanes is reduced by shuffles and issued by the run's first lane alone
template <bool FOLD>
__global__ void __launch_bounds__(256)
k_covmap_integrate(long long* __restrict__ hdr, CovSlot* __restrict__ slots, long long cap, const float* __restrict__ pts,
                   const float* __restrict__ row, long long n) {
    const CovGeom g = cov_geom(hdr);
    const unsigned long long mask = (unsigned long long)cap - 1;
    const long long stride = (long long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    long long n_claimed = 0, n_skip_pt = 0, n_skip_row = 0;
    // (whole waves iterate together: base is the wave's first point)
    for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x - lane); base < n; base += stride) {
        if (__any((int)(cov_status(hdr) & 2))) break;   // (uniform: the shuffles below need whole waves) the call is rolled back
        const long long i = base + lane;
        unsigned long long key = kCovEmpty;
        unsigned obs = 0;
        if (i < n) {
            const float v = row[i];
            key = cov_key(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], g);
            const bool row_ok = v >= 0.f && v < __builtin_inff();
            n_skip_pt += key == kCovEmpty;
            n_skip_row += !row_ok;
            if (!row_ok) key = kCovEmpty;
            obs = __float_as_uint(v + 0.f);   // (-0 -> +0)
        }
        bool head = key != kCovEmpty;
        if (FOLD) {
            const unsigned long long prev = __shfl_up(key, 1);
            head = head && (lane == 0 || prev != key);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long ok = __shfl_down(key, d);
                const unsigned oo = __shfl_down(obs, d);
                if (lane + d < 64 && ok == key) obs = oo > obs ? oo : obs;   // (an equal key beyond the run is the same voxel: harmless)
            }
        }
        if (head) {
            bool claimed = false;
            const long long s = cov_insert(slots, mask, key, hdr, claimed);
            n_claimed += claimed;
            if (s >= 0) cov_fold(slots, s, obs);
        }
    }
    cov_count(hdr, 6, n_claimed);
    cov_count(hdr, 4, n_skip_pt);
    cov_count(hdr, 5, n_skip_row);
}

// the live slots of `src` as observations of `dst` (keys of one table are distinct: nothing to fold)
__global__ void __launch_bounds__(256)
k_covmap_rehash(long long* __restrict__ hdr, CovSlot* __restrict__ slots, long long cap, const long long* __restrict__ src_hdr,
                const CovSlot* __restrict__ src, long long src_cap) {
    const CovGeom a = cov_geom(hdr), b = cov_geom(src_hdr);
    if (!(a.ox == b.ox && a.oy == b.oy && a.oz == b.oz && a.r == b.r)) {   // (uniform)
        if (blockIdx.x == 0 && threadIdx.x == 0) hdr[2] |= 4;
        return;
    }
    const unsigned long long mask = (unsigned long long)cap - 1;
    const long long stride = (long long)gridDim.x * 256;
    long long n_claimed = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < src_cap; i += stride) {
        if (cov_status(hdr) & 2) break;
        const uint4 v = cov_load(src + i);
        const unsigned long long key = cov_slot_key(v);
        if (key == kCovEmpty) continue;
        bool claimed = false;
        const long long s = cov_insert(slots, mask, key, hdr, claimed);
        n_claimed += claimed;
        if (s >= 0) cov_fold(slots, s, v.z);
    }
    cov_count(hdr, 6, n_claimed);
}

// mode 0: max, 1: add.  A call whose status is set leaves the table as it found it.
__global__ void __launch_bounds__(256) k_covmap_commit(long long* __restrict__ hdr, CovSlot* __restrict__ slots, long long cap, int mode) {
    const long long needed = hdr[0] + hdr[6];
    const bool fail = hdr[2] != 0 || 2 * needed > cap;   // (written by the kernel before; k_covmap_finish updates them after this one)
    const float clamp = cov_geom(hdr).clamp;
    const long long stride = (long long)gridDim.x * 256, t0 = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long s = t0; s < cap; s += stride) {
        uint4 v = cov_load(slots + s);
        if (cov_slot_key(v) == kCovEmpty) continue;
        const bool fresh = v.z == kCovFresh;
        if (fail) {
            if (fresh) v.x = v.y = ~0u;
        } else {
            const float old = fresh ? 0.f : __uint_as_float(v.z), obs = __uint_as_float(v.w);
            const float nv = mode == 0 ? fmaxf(old, obs) : old + obs;
            v.z = __float_as_uint(fminf(nv, clamp));
        }
        v.w = 0u;
        *reinterpret_cast<uint4*>(slots + s) = v;
    }
}

// after the commit (a kernel of its own: every block of the commit reads words 0, 2 and 6)
__global__ void k_covmap_finish(long long* __restrict__ hdr, long long cap) {
    const long long needed = hdr[0] + hdr[6];
    if (2 * needed > cap) hdr[2] |= 1;
    hdr[3] = needed;
    if (hdr[2] == 0) hdr[0] = needed;
    hdr[6] = 0;
}

__global__ void __launch_bounds__(256)
k_covmap_lookup(const long long* __restrict__ hdr, const CovSlot* __restrict__ slots, long long cap, const float* __restrict__ pts, long long n,
                float* __restrict__ out) {
    const CovGeom g = cov_geom(hdr);
    const unsigned long long mask = (unsigned long long)cap - 1;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const unsigned long long key = cov_key(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], g);
        float r = 0.f;
        if (key != kCovEmpty) {
            unsigned long long s = cov_hash(key) & mask;
            for (long long p = 0; p < cap; ++p, s = (s + 1) & mask) {   // (a table at most half full: an empty slot ends every probe)
                const uint4 v = cov_load(slots + s);
                const unsigned long long k = cov_slot_key(v);
                if (k == key) { r = __uint_as_float(v.z); break; }
                if (k == kCovEmpty) break;
            }
        }
        out[i] = r;
    }
}

// the live slots in any order: key, value and the voxel's centre origin + (i + 1/2) r; at most out_cap of them are written
__global__ void __launch_bounds__(256)
k_covmap_export(long long* __restrict__ hdr, const CovSlot* __restrict__ slots, long long cap, long long out_cap, long long* __restrict__ keys,
                float* __restrict__ values, float* __restrict__ centres) {
    const CovGeom g = cov_geom(hdr);
    const long long stride = (long long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x - lane); base < cap; base += stride) {
        const long long s = base + lane;
        uint4 v = make_uint4(~0u, ~0u, 0u, 0u);
        if (s < cap) v = cov_load(slots + s);
        const unsigned long long key = cov_slot_key(v);
        const bool live = key != kCovEmpty;
        const unsigned long long b = __ballot(live);
        if (b == 0) continue;
        long long at = 0;
        if (lane == 0)
            at = (long long)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(hdr + 7), (unsigned long long)__popcll(b), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
        at = __shfl(at, 0) + __popcll(b & ((1ull << lane) - 1));
        if (live && at < out_cap) {
            keys[at] = (long long)key;
            values[at] = __uint_as_float(v.z);
            const float ix = (float)((int)(key >> 42) - kCovBias), iy = (float)((int)((key >> 21) & 0x1fffff) - kCovBias),
                        iz = (float)((int)(key & 0x1fffff) - kCovBias);
            centres[3 * at] = g.ox + (ix + 0.5f) * g.r;
            centres[3 * at + 1] = g.oy + (iy + 0.5f) * g.r;
            centres[3 * at + 2] = g.oz + (iz + 0.5f) * g.r;
        }
    }
}

inline int cov_grid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > kCovBlocks ? kCovBlocks : b));
}

inline CovSlot* cov_slots(void* map) { return reinterpret_cast<CovSlot*>((char*)map + kCovHdr); }

inline int cov_check(const void* map, size_t bytes, int64_t cap) {
    if (!map || !covmap_capacity_ok(cap)) return TOHIP_EINVAL;
    return bytes < kCovHdr + (size_t)cap * sizeof(CovSlot) ? TOHIP_ENOSPC : TOHIP_OK;
}

// the commit of a call and, with header_host, its outcome on the host (the one synchronisation)
inline int cov_close(void* map, int64_t cap, int mode, int64_t* header_host, hipStream_t st) {
    long long* hdr = (long long*)map;
    k_covmap_commit<<<cov_grid(cap), 256, 0, st>>>(hdr, cov_slots(map), cap, mode);
    TO_HIP_CHECK_LAUNCH();
    k_covmap_finish<<<1, 1, 0, st>>>(hdr, cap);
    TO_HIP_CHECK_LAUNCH();
    if (!header_host) return TOHIP_OK;
    hipError_t e = hipMemcpyAsync(header_host, hdr, 8 * sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (header_host[2] & 4) return TOHIP_EINVAL;
    return (header_host[2] & 3) ? TOHIP_ENOSPC : TOHIP_OK;
}

inline int cov_merge(void* map, size_t bytes, int64_t cap, const void* other, size_t other_bytes, int64_t other_cap, int mode,
                     int64_t* header_host, void* stream_) {
    int rc = cov_check(map, bytes, cap);
    if (rc == TOHIP_OK) rc = cov_check(other, other_bytes, other_cap);
    if (rc != TOHIP_OK) return rc;
    if (map == other || (mode != TOHIP_COVMAP_MAX && mode != TOHIP_COVMAP_ADD)) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    long long* hdr = (long long*)map;
    const hipError_t e = hipMemsetAsync(hdr + 2, 0, 5 * sizeof(long long), st);
    if (e != hipSuccess) return (int)e;
    k_covmap_rehash<<<cov_grid(other_cap), 256, 0, st>>>(hdr, cov_slots(map), cap, (const long long*)other,
                                                         cov_slots(const_cast<void*>(other)), other_cap);
    TO_HIP_CHECK_LAUNCH();
    return cov_close(map, cap, mode, header_host, st);
}

}  // namespace

extern "C" size_t tohip_covmap_bytes(int64_t capacity) {
    return covmap_capacity_ok(capacity) ? kCovHdr + (size_t)capacity * sizeof(CovSlot) : 0;
}

extern "C" int tohip_covmap_init(void* map, size_t map_bytes, int64_t capacity, const float* origin_host, float resolution, float clamp_max,
                                 void* stream_) {
    const int rc = cov_check(map, map_bytes, capacity);
    if (rc != TOHIP_OK) return rc;
    if (!origin_host || !(resolution > 0.f) || !std::isfinite(resolution) || !(clamp_max >= 0.f)) return TOHIP_EINVAL;   // (+inf: no clamp)
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin_host[a])) return TOHIP_EINVAL;
    const CovGeom g{origin_host[0], origin_host[1], origin_host[2], resolution, clamp_max};
    k_covmap_init<<<cov_grid(capacity), 256, 0, (hipStream_t)stream_>>>((long long*)map, cov_slots(map), capacity, g);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_covmap_integrate(void* map, size_t map_bytes, int64_t capacity, const float* points, const float* log_odds, int64_t n,
                                      int mode, int fold, int64_t* header_host, void* stream_) {
    const int rc = cov_check(map, map_bytes, capacity);
    if (rc != TOHIP_OK) return rc;
    if (n < 0 || n > (int64_t)1 << 40 || (n > 0 && (!points || !log_odds)) || (mode != TOHIP_COVMAP_MAX && mode != TOHIP_COVMAP_ADD))
        return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    long long* hdr = (long long*)map;
    const hipError_t e = hipMemsetAsync(hdr + 2, 0, 5 * sizeof(long long), st);
    if (e != hipSuccess) return (int)e;
    if (n > 0) {
        if (fold)
            k_covmap_integrate<true><<<cov_grid(n), 256, 0, st>>>(hdr, cov_slots(map), capacity, points, log_odds, n);
        else
            k_covmap_integrate<false><<<cov_grid(n), 256, 0, st>>>(hdr, cov_slots(map), capacity, points, log_odds, n);
        TO_HIP_CHECK_LAUNCH();
    }
    return cov_close(map, capacity, mode, header_host, st);
}

extern "C" int tohip_covmap_lookup(const void* map, size_t map_bytes, int64_t capacity, const float* points, int64_t n, float* out,
                                   void* stream_) {
    const int rc = cov_check(map, map_bytes, capacity);
    if (rc != TOHIP_OK) return rc;
    if (n < 0 || n > (int64_t)1 << 40 || (n > 0 && (!points || !out))) return TOHIP_EINVAL;
    if (n == 0) return TOHIP_OK;
    k_covmap_lookup<<<cov_grid(n), 256, 0, (hipStream_t)stream_>>>((const long long*)map, cov_slots(const_cast<void*>(map)), capacity, points, n,
                                                                  out);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_covmap_merge(void* map, size_t map_bytes, int64_t capacity, const void* other, size_t other_bytes, int64_t other_capacity,
                                  int mode, int64_t* header_host, void* stream) {
    return cov_merge(map, map_bytes, capacity, other, other_bytes, other_capacity, mode, header_host, stream);
}

extern "C" int tohip_covmap_rehash(void* map, size_t map_bytes, int64_t capacity, const void* old_map, size_t old_bytes, int64_t old_capacity,
                                   int64_t* header_host, void* stream) {
    return cov_merge(map, map_bytes, capacity, old_map, old_bytes, old_capacity, TOHIP_COVMAP_MAX, header_host, stream);
}

extern "C" int tohip_covmap_export(void* map, size_t map_bytes, int64_t capacity, int64_t out_capacity, int64_t* keys, float* values,
                                   float* centres, void* stream_) {
    const int rc = cov_check(map, map_bytes, capacity);
    if (rc != TOHIP_OK) return rc;
    if (out_capacity < 0 || (out_capacity > 0 && (!keys || !values || !centres))) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    long long* hdr = (long long*)map;
    const hipError_t e = hipMemsetAsync(hdr + 7, 0, sizeof(long long), st);
    if (e != hipSuccess) return (int)e;
    k_covmap_export<<<cov_grid(capacity), 256, 0, st>>>(hdr, cov_slots(map), capacity, out_capacity, (long long*)keys, values, centres);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_covmap_read_header(const void* map, int64_t* words_host, float* geometry_host, void* stream_) {
    if (!map || !words_host) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    long long h[11];
    hipError_t e = hipMemcpyAsync(h, map, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    for (int i = 0; i < 8; ++i) words_host[i] = h[i];
    if (geometry_host) std::memcpy(geometry_host, h + 8, 5 * sizeof(float));
    return TOHIP_OK;
}
