// reframe_kernels.hip — move voxel content from one box into another at an integer voxel shift ("Re-framing and
// merging maps"), for gfx950.  Included after evidence_kernels.hip: the geometry, the brick layout, the brick mask and the per-wave
// count are the map layer's (OccGeom, occ_check, evid_check, occ_brick_mask, evid_brick, occ_count, occ_grid_blocks).
//
// src and dst are two buffers with their own dims; (sx, sy, sz) is an integer voxel shift.  For every voxel v inside dst's dims the
// SOURCE VALUE is that of src voxel v + s where it lies inside src's dims, otherwise EMPTY (bit 0, value -128).  Origins and
// resolutions are not interpreted: the host computes the shift.
//
//   k_occ_transfer    one lane per dst word in a grid-stride loop.  With q = floor(s / brick), r = s - brick q per axis (brick = 4, 4,
//                     2), the dst brick b is composed from the source words of the bricks b + q + {0, 1}^3 — a word beyond the source's
//                     brick range is 0 and is not loaded, one whose axis has r = 0 is not needed — in three funnel stages: x within
//                     every 4-bit row, ((A >> rx) & lo) | ((B << (4 - rx)) & hi) with the nibble masks replicated eight times; y the
//                     same in units of 4 bits within each 16-bit half; z a 16-bit funnel; then dst's pad mask.  The source's pad bits
//                     are 0 (the layer guarantees it), so a voxel outside the source's dims reads as 0 without a test of its own.
//                     A brick-aligned shift loads one word.  COPY stores it; OR loads dst's word and stores the union.
//   k_evid_transfer   one lane per dst brick, its 32 values as two 16-byte halves (z & 1).  The half z of a dst brick reads one half of
//                     up to 2 x 2 source bricks (x, y) — four 16-byte loads, a dword per row of four x values — and composes them
//                     with byte funnels: per row, the 8 bytes (A, B) >> 8 rx; then row j + ry of the eight rows (A, B) along y.  A
//                     half beyond the source's brick range is 0x80 bytes and is not loaded.  The combine is evid_update4's style:
//                     bytes biased to u = L + 128, masks instead of branches.  The lane stores its two halves and the brick's occupied
//                     and free words, built from the new values as k_evid_fold builds them.  In ADD and CONFIDENT a brick whose source
//                     values are all -128 is neither loaded from dst nor written.
//
// Integers only, no atomics on a plane or on the values (one lane owns a word), no LDS, nothing read back; every argument check returns
// before anything is enqueued.
namespace {

constexpr int kXferMaxShift = 4096;
enum { kXferCopy = 0, kXferOr = 1, kXferAdd = 1, kXferConfident = 2 };

struct XferShift {
    int qx, qy, qz;   // floor(s / (4, 4, 2)): the source brick of dst brick b is b + q (+ 1 where r != 0)
    int rx, ry, rz;   // s - (4, 4, 2) q, in [0, 4), [0, 4), [0, 2)
    int sz;           // the z shift itself (the evidence kernel works in half bricks)
};

inline XferShift xfer_shift(int sx, int sy, int sz) {
    return XferShift{sx >> 2, sy >> 2, sz >> 1, sx & 3, sy & 3, sz & 1, sz};   // (>> of a negative int is arithmetic: floor)
}
inline bool xfer_shift_ok(int sx, int sy, int sz) {
    return sx >= -kXferMaxShift && sx <= kXferMaxShift && sy >= -kXferMaxShift && sy <= kXferMaxShift && sz >= -kXferMaxShift && sz <= kXferMaxShift;
}

__device__ __forceinline__ unsigned xfer_word(const unsigned* __restrict__ src, const OccGeom& gs, int nbz, int bx, int by, int bz) {
    const bool in = (unsigned)bx < (unsigned)gs.nbx && (unsigned)by < (unsigned)gs.nby && (unsigned)bz < (unsigned)nbz;
    return in ? src[((long long)bz * gs.nby + by) * gs.nbx + bx] : 0u;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_transfer(const unsigned* __restrict__ src, OccGeom gs, int nbz_s, unsigned* __restrict__ dst, OccGeom gd, long long n_words, XferShift s,
               int mode, unsigned long long* __restrict__ counts) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    const unsigned lo_x = (0xFu >> s.rx) * 0x11111111u, lo_y = (0xFFFFu >> (4 * s.ry)) * 0x10001u;
    long long added = 0;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < n_words; w += stride) {
        int bx, by, bz;
        evid_brick(gd, (unsigned)w, bx, by, bz);
        const int ax = bx + s.qx, ay = by + s.qy, az = bz + s.qz;
        unsigned zs[2] = {0u, 0u};
#pragma unroll
        for (int dz = 0; dz < 2; ++dz) {
            if (dz && !s.rz) break;   // (uniform)
            unsigned ys[2] = {0u, 0u};
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                if (dy && !s.ry) break;   // (uniform)
                const unsigned A = xfer_word(src, gs, nbz_s, ax, ay + dy, az + dz);
                const unsigned B = s.rx ? xfer_word(src, gs, nbz_s, ax + 1, ay + dy, az + dz) : 0u;
                ys[dy] = ((A >> s.rx) & lo_x) | ((B << (4 - s.rx)) & ~lo_x);   // (rx = 0: lo_x is all ones)
            }
            zs[dz] = ((ys[0] >> (4 * s.ry)) & lo_y) | ((ys[1] << (16 - 4 * s.ry)) & ~lo_y);
        }
        const unsigned got = (s.rz ? (zs[0] >> 16) | (zs[1] << 16) : zs[0]) & occ_brick_mask(gd, bx, by, bz);
        if (mode == kXferCopy) {
            dst[w] = got;
            added += __popc(got);
        } else if (got != 0u) {
            const unsigned old = dst[w];
            if ((got & ~old) != 0u) dst[w] = old | got;
            added += __popc(got & ~old);
        }
    }
    if (counts) occ_count(counts, added);
}

// the four source rows (dwords: four x values each) of dst rows 0 .. 3 along y: row j is row j + ry of the eight rows (A, B)
__device__ __forceinline__ void xfer_rows(const unsigned (&a)[8], int ry, unsigned (&out)[4]) {
    switch (ry) {   // (uniform; a register file has no indexed read)
        case 0: out[0] = a[0], out[1] = a[1], out[2] = a[2], out[3] = a[3]; break;
        case 1: out[0] = a[1], out[1] = a[2], out[2] = a[3], out[3] = a[4]; break;
        case 2: out[0] = a[2], out[1] = a[3], out[2] = a[4], out[3] = a[5]; break;
        default: out[0] = a[3], out[1] = a[4], out[2] = a[5], out[3] = a[6]; break;
    }
}

// one 16-byte half (half = z & 1) of the source brick (bx, by, bz); beyond the brick range: never observed, not loaded
__device__ __forceinline__ uint4 xfer_half(const uint4* __restrict__ src, const OccGeom& gs, int nbz, int bx, int by, int bz, int half) {
    const bool in = (unsigned)bx < (unsigned)gs.nbx && (unsigned)by < (unsigned)gs.nby && (unsigned)bz < (unsigned)nbz;
    return in ? src[2 * (((long long)bz * gs.nby + by) * gs.nbx + bx) + half] : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
}

// Four values: the bytes of d (dst) and of sv (the source values), `in` the nibble of the voxels inside dst's dims -> the new four
// bytes; the nibbles of: a source value that is known (inside dims), the occupied bits before and after, the bytes that changed, the
// bytes that left -128, the bytes that are not -128 afterwards.  Biased bytes u = L + 128 (0: never observed), as evid_update4.
__device__ __forceinline__ unsigned xfer_combine4(unsigned d, unsigned sv, unsigned in, int mode, const EvidParams& p, unsigned& occ_old,
                                                  unsigned& occ_new, unsigned& changed, unsigned& newly, unsigned& known) {
    const unsigned xd = d ^ 0x80808080u, xs = sv ^ 0x80808080u;
    unsigned out = 0u;
    occ_old = occ_new = changed = newly = known = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ud = (int)((xd >> (8 * j)) & 0xFFu);
        const int us = ((in >> j) & 1u) ? (int)((xs >> (8 * j)) & 0xFFu) : 0;   // (a pad voxel takes nothing)
        int un;
        if (mode == kXferCopy) {
            un = us;
        } else if (mode == kXferAdd) {
            const int sum = min(max((ud ? ud : 128) + us - 128, p.lmin), p.lmax);   // (biased: L_d + L_s + 128)
            un = us ? sum : ud;
        } else {
            const int uc = us ? min(max(us, p.lmin), p.lmax) : 0;
            // the order's key: -1 for never observed, else 2 |L| + (L > 0)
            const int ks = uc ? 2 * abs(uc - 128) + (uc > 128) : -1, kd = ud ? 2 * abs(ud - 128) + (ud > 128) : -1;
            un = ks > kd ? uc : ud;
        }
        occ_old |= ((unsigned)(p.threshold - ud) >> 31) << j;   // (u = 0 is below every threshold)
        occ_new |= ((unsigned)(p.threshold - un) >> 31) << j;
        changed |= (unsigned)(un != ud) << j;
        newly |= (unsigned)(ud == 0 && un != 0) << j;
        known |= (unsigned)(un != 0) << j;
        out |= (unsigned)un << (8 * j);
    }
    return out ^ 0x80808080u;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_evid_transfer(const uint4* __restrict__ src, OccGeom gs, int nbz_s, uint4* __restrict__ dst, OccGeom gd, unsigned* __restrict__ occ_out,
                unsigned* __restrict__ fre_out, long long n_words, XferShift s, int mode, EvidParams p, unsigned long long* __restrict__ counts) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    long long n_changed = 0, n_known = 0, appeared = 0, vanished = 0;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < n_words; w += stride) {
        int bx, by, bz;
        evid_brick(gd, (unsigned)w, bx, by, bz);
        const int ax = bx + s.qx, ay = by + s.qy;
        const unsigned in = occ_brick_mask(gd, bx, by, bz);
        unsigned v[8];   // the source values of the brick's eight rows
        unsigned any = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int z = 2 * bz + k + s.sz, az = z >> 1, half = z & 1;   // (>>: floor)
            unsigned rows[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                if (dy && !s.ry) break;   // (uniform)
                const uint4 A = xfer_half(src, gs, nbz_s, ax, ay + dy, az, half);
                const uint4 B = s.rx ? xfer_half(src, gs, nbz_s, ax + 1, ay + dy, az, half) : A;
                const unsigned a4[4] = {A.x, A.y, A.z, A.w}, b4[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)   // bytes rx .. rx + 3 of the eight bytes (A, B) of the row
                    rows[4 * dy + j] = (unsigned)((((unsigned long long)b4[j] << 32) | a4[j]) >> (8 * s.rx));
            }
            unsigned r4[4];
            xfer_rows(rows, s.ry, r4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[4 * k + j] = r4[j];
                // a known source value inside dst's dims?
                const unsigned x = r4[j] ^ 0x80808080u, nib = (in >> (16 * k + 4 * j)) & 0xFu;
                any |= (x & 0xFFu ? nib & 1u : 0u) | (x & 0xFF00u ? nib & 2u : 0u) | (x & 0xFF0000u ? nib & 4u : 0u) | (x & 0xFF000000u ? nib & 8u : 0u);
            }
        }
        if (mode != kXferCopy && any == 0u) continue;   // nothing to merge into this brick
        unsigned d[8];
        if (mode == kXferCopy) {
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = 0x80808080u;   // (dst's old content is not read: counted as empty)
        } else {
            const uint4 lo = dst[2 * w], hi = dst[2 * w + 1];
            d[0] = lo.x, d[1] = lo.y, d[2] = lo.z, d[3] = lo.w, d[4] = hi.x, d[5] = hi.y, d[6] = hi.z, d[7] = hi.w;
        }
        unsigned occ_old = 0u, occ_new = 0u, changed = 0u, newly = 0u, known = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            unsigned o4, n4, c4, w4, k4;
            d[k] = xfer_combine4(d[k], v[k], (in >> (4 * k)) & 0xFu, mode, p, o4, n4, c4, w4, k4);
            occ_old |= o4 << (4 * k), occ_new |= n4 << (4 * k), changed |= c4 << (4 * k), newly |= w4 << (4 * k), known |= k4 << (4 * k);
        }
        dst[2 * w] = make_uint4(d[0], d[1], d[2], d[3]);
        dst[2 * w + 1] = make_uint4(d[4], d[5], d[6], d[7]);
        occ_out[w] = occ_new;
        fre_out[w] = known & ~occ_new;
        n_changed += __popc(changed);
        n_known += __popc(newly);
        appeared += __popc(occ_new & ~occ_old);
        vanished += __popc(occ_old & ~occ_new);
    }
    if (counts) {
        occ_count(counts, n_changed);
        occ_count(counts + 1, n_known);
        occ_count(counts + 2, appeared);
        occ_count(counts + 3, vanished);
    }
}

}  // namespace

extern "C" int tohip_occ_transfer(const void* src, size_t src_bytes, const tohip_occ_geom* src_geom, void* dst, size_t dst_bytes,
                                  const tohip_occ_geom* dst_geom, int32_t sx, int32_t sy, int32_t sz, int32_t mode, uint64_t* counts,
                                  void* stream_) {
    OccGeom gs, gd;
    int rc = occ_check(src, src_bytes, src_geom, gs);
    if (rc != TOHIP_OK) return rc;
    rc = occ_check(dst, dst_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    if (src == dst || (const void*)counts == src || (void*)counts == dst || (mode != kXferCopy && mode != kXferOr) || !xfer_shift_ok(sx, sy, sz))
        return TOHIP_EINVAL;
    const long long n_words = (long long)occ_words(gd.nx, gd.ny, gd.nz);
    k_occ_transfer<<<occ_grid_blocks(n_words), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(src), gs, (gs.nz + 1) / 2, occ_data(dst), gd, n_words,
                                                                                   xfer_shift(sx, sy, sz), mode, (unsigned long long*)counts);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_evid_transfer(const void* src, size_t src_bytes, const tohip_occ_geom* src_geom, void* dst, size_t dst_bytes,
                                   const tohip_occ_geom* dst_geom, void* occupied_out, void* free_out, size_t grid_bytes, int32_t sx, int32_t sy,
                                   int32_t sz, int32_t mode, int32_t lmin, int32_t lmax, int32_t threshold, uint64_t* counts, void* stream_) {
    OccGeom gs, gd;
    int rc = evid_check(src, src_bytes, src_geom, gs);
    if (rc != TOHIP_OK) return rc;
    rc = evid_check(dst, dst_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    rc = occ_check(occupied_out, grid_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    if (!free_out || mode < kXferCopy || mode > kXferConfident || !xfer_shift_ok(sx, sy, sz) || !evid_params_ok(1, 1, lmin, lmax, threshold))
        return TOHIP_EINVAL;
    const void* bufs[5] = {src, dst, occupied_out, free_out, counts};
    for (int a = 0; a < 5; ++a)
        for (int b = a + 1; b < 5; ++b)
            if (bufs[a] == bufs[b]) return TOHIP_EINVAL;
    const long long n_words = (long long)occ_words(gd.nx, gd.ny, gd.nz);
    k_evid_transfer<<<occ_grid_blocks(n_words), TO_BLOCK, 0, (hipStream_t)stream_>>>(
        reinterpret_cast<const uint4*>((const char*)src + kEvidHdr), gs, (gs.nz + 1) / 2, reinterpret_cast<uint4*>((char*)dst + kEvidHdr), gd,
        occ_data(occupied_out), occ_data(free_out), n_words, xfer_shift(sx, sy, sz), mode, EvidParams{0, 0, lmin + 128, lmax + 128, threshold + 128},
        (unsigned long long*)counts);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
