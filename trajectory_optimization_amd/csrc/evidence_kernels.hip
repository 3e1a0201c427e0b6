// evidence_kernels.hip — a hit/miss evidence map under the occupancy grid's planes ("Evidence map"), for gfx950.  Included
// right after field_kernels.hip: the geometry, the fixed-point coordinates, the brick layout, the brick mask and the per-wave count are
// the map layer's (OccGeom, occ_brick_mask, occ_locate, occ_word, occ_bit, occ_count, occ_grid_blocks).
//
// The EVIDENCE buffer has an occupancy grid's geometry and one signed 8-bit log-odds value per voxel IN BRICK ORDER: a 256-byte header
// (zero), then byte 32 w + b for word w = ((z>>1) nby + (y>>2)) nbx + (x>>2) and bit b = x&3 | (y&3)<<2 | (z&1)<<4 — the 32 voxels of
// a brick word are 32 consecutive, 32-byte-aligned bytes, so a lane that owns a word moves its values as two 16-byte accesses.  -128:
// never observed; pad voxels (outside dims) hold -128 for ever.  State of a value L: unknown iff L == -128, else occupied iff L >
// threshold, else free.
//
//   k_evid_fold       one scan's evidence: a hit plane H and a pass plane M (bit planes of the geometry).  One lane per brick word in a
//                     grid-stride loop: the word of H and of M; both zero: nothing else is touched (8 bytes of traffic).  Otherwise
//                     the brick's 32 values (two 16-byte loads), per voxel inside dims base = (L == -128 ? 0 : L), with the H bit
//                     L <- min(base + hit, lmax), else with the M bit L <- max(base - miss, lmin), else unchanged; two 16-byte stores;
//                     the brick's occupied word (L > threshold) and free word (L != -128 and L <= threshold) are built from the new
//                     values and stored by the same lane (pad bits 0); with clear_scan the consumed words of H and M are zeroed.
//                     counts (u64 x 4): += voxels updated, += voxels newly known, += occupied bits that appeared, += that vanished
//                     — summed per wave (occ_count), the only atomics.
//   k_evid_positions  (M,3) f32 positions -> int8 value (-128 unknown, and -128 out of range or outside dims) and / or uint8 state: 0
//                     unknown, 1 free, 2 occupied, 3 out of range or outside dims — SpaceMap.state's codes.
//
// No LDS, no float atomics, no process-wide state; every argument check returns before anything is enqueued.
namespace {

constexpr size_t kEvidHdr = 256;
constexpr int kEvidUnknown = -128;

struct EvidParams {
    int hit, miss, lmin, lmax, threshold;   // (the kernel's copy holds lmin, lmax and threshold + 128: the bytes are biased there)
};

inline size_t evid_size(int64_t nx, int64_t ny, int64_t nz) { return kEvidHdr + occ_words(nx, ny, nz) * 32; }

inline bool evid_params_ok(int hit, int miss, int lmin, int lmax, int threshold) {
    return hit >= 1 && hit <= 127 && miss >= 1 && miss <= 127 && lmin >= -127 && lmin <= threshold && threshold < lmax && lmax <= 127;
}

// the geometry (occ_check's rules), the buffer's size and its alignment (the values are moved 16 bytes at a time)
inline int evid_check(const void* evid, size_t bytes, const tohip_occ_geom* geom, OccGeom& g) {
    const int rc = occ_check(evid, ~(size_t)0, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (((uintptr_t)evid & 15u) != 0) return TOHIP_EINVAL;
    return bytes < evid_size(g.nx, g.ny, g.nz) ? TOHIP_ENOSPC : TOHIP_OK;
}

// Four values — the bytes of v, the voxels 4 k .. 4 k + 3 of the brick — under the nibbles h and m of the brick's hit and pass bits
// (masked to dims, m without the bits of h) -> the new four bytes; the nibbles of the occupied bits before and after and of the
// voxels that held -128.  Byte-parallel in spirit: the bytes are biased to u = L + 128 in [0, 255] (0: never observed) and every
// choice is a mask, not a branch or a condition register — 32 voxels a lane leave no room for 32 lane masks in the scalar file.
__device__ __forceinline__ unsigned evid_update4(unsigned v, unsigned h, unsigned m, const EvidParams& p, unsigned& occ_old, unsigned& occ_new,
                                                 unsigned& unk_old) {
    const unsigned x = v ^ 0x80808080u;
    unsigned out = 0u;
    occ_old = occ_new = unk_old = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int u = (int)((x >> (8 * j)) & 0xFFu);
        const unsigned ub = (unsigned)(u - 1) >> 31;   // 1 iff never observed
        const int base = u | (int)(ub << 7);           // ... which counts as L = 0
        const int up = min(base + p.hit, p.lmax), down = max(base - p.miss, p.lmin);
        const int hm = -(int)((h >> j) & 1u), mm = -(int)((m >> j) & 1u);
        const int un = (up & hm) | (down & mm) | (u & ~(hm | mm));
        occ_old |= ((unsigned)(p.threshold - u) >> 31) << j;   // (u = 0 is below every threshold)
        occ_new |= ((unsigned)(p.threshold - un) >> 31) << j;
        unk_old |= ub << j;
        out |= (unsigned)un << (8 * j);
    }
    return out ^ 0x80808080u;
}

// The brick of word w, as occ_brick gives it, in 32-bit arithmetic (a grid has at most 2^28 words): occ_brick divides 64-bit integers,
// which the chip does in software.  Fewer instructions; no difference in the kernel's measured time.
__device__ __forceinline__ void evid_brick(const OccGeom& g, unsigned w, int& bx, int& by, int& bz) {
    const unsigned row = w / (unsigned)g.nbx;
    bx = (int)(w - row * (unsigned)g.nbx);
    bz = (int)(row / (unsigned)g.nby);
    by = (int)(row - (unsigned)bz * (unsigned)g.nby);
}

__global__ void __launch_bounds__(TO_BLOCK)
k_evid_fold(uint4* __restrict__ vals, unsigned* __restrict__ hit_w, unsigned* __restrict__ pass_w, unsigned* __restrict__ occ_out,
            unsigned* __restrict__ fre_out, OccGeom g, long long n_words, EvidParams p, int clear_scan, unsigned long long* __restrict__ counts) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    long long updated = 0, known = 0, appeared = 0, vanished = 0;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < n_words; w += stride) {
        const unsigned h_raw = hit_w[w], m_raw = pass_w[w];
        if ((h_raw | m_raw) == 0u) continue;
        int bx, by, bz;
        evid_brick(g, (unsigned)w, bx, by, bz);
        const unsigned in = occ_brick_mask(g, bx, by, bz);
        const unsigned h = h_raw & in, m = m_raw & in & ~h_raw;   // (a hit wins)
        uint4 lo = vals[2 * w], hi = vals[2 * w + 1];
        unsigned v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        unsigned occ_old = 0u, occ_new = 0u, unk_old = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            unsigned o4, n4, u4;
            v[k] = evid_update4(v[k], (h >> (4 * k)) & 0xFu, (m >> (4 * k)) & 0xFu, p, o4, n4, u4);
            occ_old |= o4 << (4 * k), occ_new |= n4 << (4 * k), unk_old |= u4 << (4 * k);
        }
        const unsigned touched = h | m;
        const unsigned fre_new = ~(occ_new | (unk_old & ~touched));   // (a pad voxel is never touched: it stays unknown, both bits 0)
        const unsigned newly = unk_old & touched;
        vals[2 * w] = make_uint4(v[0], v[1], v[2], v[3]);
        vals[2 * w + 1] = make_uint4(v[4], v[5], v[6], v[7]);
        occ_out[w] = occ_new;
        fre_out[w] = fre_new;
        if (clear_scan) {
            if (h_raw != 0u) hit_w[w] = 0u;
            if (m_raw != 0u) pass_w[w] = 0u;
        }
        updated += __popc(touched);
        known += __popc(newly);
        appeared += __popc(occ_new & ~occ_old);
        vanished += __popc(occ_old & ~occ_new);
    }
    if (counts) {
        occ_count(counts, updated);
        occ_count(counts + 1, known);
        occ_count(counts + 2, appeared);
        occ_count(counts + 3, vanished);
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_evid_positions(const signed char* __restrict__ vals, OccGeom g, int threshold, const float* __restrict__ pos, long long m,
                 signed char* __restrict__ val_out, uint8_t* __restrict__ state_out) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    for (long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; i < m; i += stride) {
        int x, y, z, L = kEvidUnknown, s = 3;
        if (occ_locate(g, pos + 3 * i, x, y, z) == kOccInside) {
            L = vals[32ll * occ_word(g, x, y, z) + occ_bit(x, y, z)];
            s = L == kEvidUnknown ? 0 : (L > threshold ? 2 : 1);
        }
        if (val_out) val_out[i] = (signed char)L;
        if (state_out) state_out[i] = (uint8_t)s;
    }
}

}  // namespace

extern "C" size_t tohip_evid_bytes(int32_t nx, int32_t ny, int32_t nz) { return occ_dims_ok(nx, ny, nz) ? evid_size(nx, ny, nz) : 0; }

extern "C" int tohip_evid_init(void* evid, size_t evid_bytes, const tohip_occ_geom* geom, void* stream_) {
    OccGeom g;
    const int rc = evid_check(evid, evid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    hipStream_t st = (hipStream_t)stream_;
    hipError_t e = hipMemsetAsync(evid, 0, kEvidHdr, st);
    if (e == hipSuccess) e = hipMemsetAsync((char*)evid + kEvidHdr, 0x80, evid_size(g.nx, g.ny, g.nz) - kEvidHdr, st);
    return e == hipSuccess ? TOHIP_OK : (int)e;
}

extern "C" int tohip_evid_fold(void* evid, size_t evid_bytes, void* hit_plane, void* pass_plane, void* occupied_out, void* free_out,
                               size_t grid_bytes, const tohip_occ_geom* geom, int32_t hit, int32_t miss, int32_t lmin, int32_t lmax,
                               int32_t threshold, int32_t clear_scan, uint64_t* counts, void* stream_) {
    OccGeom g;
    int rc = evid_check(evid, evid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    rc = occ_check(hit_plane, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!pass_plane || !occupied_out || !free_out || !evid_params_ok(hit, miss, lmin, lmax, threshold)) return TOHIP_EINVAL;
    const void* planes[5] = {hit_plane, pass_plane, occupied_out, free_out, evid};
    for (int a = 0; a < 5; ++a)
        for (int b = a + 1; b < 5; ++b)
            if (planes[a] == planes[b]) return TOHIP_EINVAL;
    const long long n_words = (long long)occ_words(g.nx, g.ny, g.nz);
    k_evid_fold<<<occ_grid_blocks(n_words), TO_BLOCK, 0, (hipStream_t)stream_>>>(
        reinterpret_cast<uint4*>((char*)evid + kEvidHdr), occ_data(hit_plane), occ_data(pass_plane), occ_data(occupied_out), occ_data(free_out), g,
        n_words, EvidParams{hit, miss, lmin + 128, lmax + 128, threshold + 128}, clear_scan != 0, (unsigned long long*)counts);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_evid_positions(const void* evid, size_t evid_bytes, const tohip_occ_geom* geom, int32_t threshold, const float* positions,
                                    int64_t m, int8_t* values, uint8_t* state, void* stream_) {
    OccGeom g;
    const int rc = evid_check(evid, evid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (threshold < -127 || threshold > 126 || !occ_count_ok(m) || (m > 0 && (!positions || (!values && !state)))) return TOHIP_EINVAL;
    if (m == 0) return TOHIP_OK;
    k_evid_positions<<<occ_grid_blocks(m), TO_BLOCK, 0, (hipStream_t)stream_>>>((const signed char*)evid + kEvidHdr, g, threshold, positions, m,
                                                                               (signed char*)values, state);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
