// resample_kernels.hip — voxel content of one box read in another under a rigid transform and a change of resolution (DESIGN.md §10,
// "Resampling maps"), for gfx950.  Included after reframe_kernels.hip: the geometry, the brick layout, the brick mask, the per-wave
// count and the combine of two evidence values are the map layer's (OccGeom, occ_check, evid_check, occ_brick_mask, evid_brick,
// occ_word, occ_bit, occ_inside, occ_count, occ_grid_blocks, xfer_combine4).
//
// The host hands over twelve integers, M (3 x 3, row major) and T (3), in fixed point with F = 20 fraction bits: the source position
// of the centre of dst voxel d = (i, j, k), in source voxels, is u / 2^F with
//     u_a = M[a][0] (2 i + 1) + M[a][1] (2 j + 1) + M[a][2] (2 k + 1) + T[a]          (int64; |M| <= 2^21, |T| <= 2^40: below 2^42)
// and its NEAREST source voxel n_a = u_a >> F (an arithmetic shift: the floor).  Origins and resolutions are not interpreted.
//
//   k_evid_resample   one lane per dst brick in a grid-stride loop, as k_evid_transfer: u of the brick's first voxel by three
//                     multiplies per axis, every other voxel by adds of the columns 2 M[.][x], 2 M[.][y], 2 M[.][z].  NEAREST: the
//                     byte of n, -128 outside the source's dims.  COVER: the maximum over the 3 x 3 x 3 source voxels around n of
//                     the key free < unknown < occupied (128 + L for L <= threshold; 256 for -128 and outside dims; 640 + L above
//                     the threshold), decoded again: 27 byte loads a voxel, neighbours in the source, no pre-pass and no scratch.
//                     The sampled 32 values then go through k_evid_transfer's tail unchanged: xfer_combine4 (COPY / ADD /
//                     CONFIDENT), two 16-byte stores, the two plane words, the four counts; in ADD and CONFIDENT a brick whose
//                     sampled values are all -128 inside dst's dims is neither loaded nor written.
//   k_occ_resample    one lane per dst word: the bit of n (NEAREST), the OR (ANY) or the AND (ALL, a bit outside dims counts 0) of the
//                     27 bits around n; dst's pad mask; COPY stores, OR loads dst's word and stores the union where it differs.
//
// The reads are a gather through the caches (a wave's 64 bricks lie side by side in dst, so their sources lie within a few bricks
// of one another), the writes are k_evid_transfer's.  Integers only, no atomics on a plane or on the values (one lane owns a word),
// no LDS, nothing read back; every argument check returns before anything is enqueued.
namespace {

constexpr int kRsFrac = 20;
constexpr long long kRsMaxM = 1ll << 21, kRsMaxT = 1ll << 40;
enum { kRsNearest = 0, kRsCover = 1, kRsAny = 1, kRsAll = 2 };

struct RsAffine {
    long long m[9];   // row major: u_a = m[3 a] (2 i + 1) + m[3 a + 1] (2 j + 1) + m[3 a + 2] (2 k + 1) + t[a]
    long long t[3];
};

inline bool rs_affine_ok(const int64_t* a, int frac_bits, RsAffine& out) {
    if (!a || frac_bits != kRsFrac) return false;
    for (int i = 0; i < 9; ++i) {
        if (a[i] < -kRsMaxM || a[i] > kRsMaxM) return false;
        out.m[i] = a[i];
    }
    for (int i = 0; i < 3; ++i) {
        if (a[9 + i] < -kRsMaxT || a[9 + i] > kRsMaxT) return false;
        out.t[i] = a[9 + i];
    }
    return true;
}

// u of dst voxel (i, j, k) along source axis a
__device__ __forceinline__ long long rs_u(const RsAffine& A, int a, int i, int j, int k) {
    return A.m[3 * a] * (2 * i + 1) + A.m[3 * a + 1] * (2 * j + 1) + A.m[3 * a + 2] * (2 * k + 1) + A.t[a];
}

// the value of source voxel (x, y, z): a byte of its brick, -128 outside dims
__device__ __forceinline__ int rs_value(const signed char* __restrict__ vals, const OccGeom& gs, int x, int y, int z) {
    return occ_inside(gs, x, y, z) ? (int)vals[32ll * occ_word(gs, x, y, z) + occ_bit(x, y, z)] : kEvidUnknown;
}
__device__ __forceinline__ unsigned rs_bit(const unsigned* __restrict__ words, const OccGeom& gs, int x, int y, int z) {
    return occ_inside(gs, x, y, z) ? (words[occ_word(gs, x, y, z)] >> occ_bit(x, y, z)) & 1u : 0u;
}

// COVER: the 27 values around (x, y, z) under the key free < unknown < occupied, the largest decoded (threshold unbiased here)
__device__ __forceinline__ int rs_cover(const signed char* __restrict__ vals, const OccGeom& gs, int x, int y, int z, int threshold) {
    int best = 0;
#pragma unroll 1
    for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll 1
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int L = rs_value(vals, gs, x + dx, y + dy, z + dz);
                best = max(best, L == kEvidUnknown ? 256 : (L > threshold ? 640 + L : 128 + L));
            }
        }
    }
    return best > 512 ? best - 640 : (best == 256 ? kEvidUnknown : best - 128);
}

template <int RULE>
__global__ void __launch_bounds__(TO_BLOCK)
k_evid_resample(const signed char* __restrict__ src, OccGeom gs, uint4* __restrict__ dst, OccGeom gd, unsigned* __restrict__ occ_out,
                unsigned* __restrict__ fre_out, long long n_words, RsAffine A, int mode, EvidParams p, unsigned long long* __restrict__ counts) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    long long n_changed = 0, n_known = 0, appeared = 0, vanished = 0;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < n_words; w += stride) {
        int bx, by, bz;
        evid_brick(gd, (unsigned)w, bx, by, bz);
        const unsigned in = occ_brick_mask(gd, bx, by, bz);
        const long long u0[3] = {rs_u(A, 0, 4 * bx, 4 * by, 2 * bz), rs_u(A, 1, 4 * bx, 4 * by, 2 * bz), rs_u(A, 2, 4 * bx, 4 * by, 2 * bz)};
        unsigned v[8];   // the sampled values of the brick's eight rows
        unsigned any = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {   // row k: z = k >> 2, y = k & 3
            unsigned row = 0u;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                int n[3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    n[a] = (int)((u0[a] + 2 * (x * A.m[3 * a] + (k & 3) * A.m[3 * a + 1] + (k >> 2) * A.m[3 * a + 2])) >> kRsFrac);
                const int S = RULE == kRsNearest ? rs_value(src, gs, n[0], n[1], n[2]) : rs_cover(src, gs, n[0], n[1], n[2], p.threshold - 128);
                row |= (unsigned)(S & 0xFF) << (8 * x);
                any |= (unsigned)(S != kEvidUnknown) & (in >> (4 * k + x));
            }
            v[k] = row;
        }
        if (mode != kXferCopy && (any & 1u) == 0u) continue;   // nothing to merge into this brick
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

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_resample(const unsigned* __restrict__ src, OccGeom gs, unsigned* __restrict__ dst, OccGeom gd, long long n_words, RsAffine A, int rule,
               int mode, unsigned long long* __restrict__ counts) {
    const long long stride = (long long)gridDim.x * TO_BLOCK;
    long long added = 0;
    for (long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x; w < n_words; w += stride) {
        int bx, by, bz;
        evid_brick(gd, (unsigned)w, bx, by, bz);
        const unsigned in = occ_brick_mask(gd, bx, by, bz);
        const long long u0[3] = {rs_u(A, 0, 4 * bx, 4 * by, 2 * bz), rs_u(A, 1, 4 * bx, 4 * by, 2 * bz), rs_u(A, 2, 4 * bx, 4 * by, 2 * bz)};
        unsigned got = 0u;
#pragma unroll 1
        for (int b = 0; b < 32; ++b) {   // bit b: x = b & 3, y = (b >> 2) & 3, z = b >> 4
            if (((in >> b) & 1u) == 0u) continue;
            int n[3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                n[a] = (int)((u0[a] + 2 * ((b & 3) * A.m[3 * a] + ((b >> 2) & 3) * A.m[3 * a + 1] + (b >> 4) * A.m[3 * a + 2])) >> kRsFrac);
            unsigned bit;
            if (rule == kRsNearest) {
                bit = rs_bit(src, gs, n[0], n[1], n[2]);
            } else {
                unsigned any = 0u, all = 1u;
#pragma unroll 1
                for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll 1
                    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const unsigned s = rs_bit(src, gs, n[0] + dx, n[1] + dy, n[2] + dz);
                            any |= s, all &= s;
                        }
                    }
                }
                bit = rule == kRsAny ? any : all;
            }
            got |= bit << b;
        }
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

}  // namespace

extern "C" int tohip_occ_resample(const void* src, size_t src_bytes, const tohip_occ_geom* src_geom, void* dst, size_t dst_bytes,
                                  const tohip_occ_geom* dst_geom, const int64_t* affine_host, int32_t frac_bits, int32_t rule, int32_t mode,
                                  uint64_t* counts, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom gs, gd;
    int rc = occ_check(src, src_bytes, src_geom, gs);
    if (rc != TOHIP_OK) return rc;
    rc = occ_check(dst, dst_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    RsAffine A;
    if (src == dst || (const void*)counts == src || (void*)counts == dst || (mode != kXferCopy && mode != kXferOr) || rule < kRsNearest ||
        rule > kRsAll || !rs_affine_ok(affine_host, frac_bits, A))
        return TOHIP_EINVAL;
    const long long n_words = (long long)occ_words(gd.nx, gd.ny, gd.nz);
    k_occ_resample<<<occ_grid_blocks(n_words), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(src), gs, occ_data(dst), gd, n_words, A, rule, mode,
                                                                                   (unsigned long long*)counts);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_evid_resample(const void* src, size_t src_bytes, const tohip_occ_geom* src_geom, void* dst, size_t dst_bytes,
                                   const tohip_occ_geom* dst_geom, void* occupied_out, void* free_out, size_t grid_bytes,
                                   const int64_t* affine_host, int32_t frac_bits, int32_t rule, int32_t mode, int32_t lmin, int32_t lmax,
                                   int32_t threshold, uint64_t* counts, void* scratch, size_t scratch_bytes, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    (void)scratch_bytes;   // (COVER takes its 27 taps in place: no pre-pass, the scratch is not touched)
    OccGeom gs, gd;
    int rc = evid_check(src, src_bytes, src_geom, gs);
    if (rc != TOHIP_OK) return rc;
    rc = evid_check(dst, dst_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    rc = occ_check(occupied_out, grid_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    RsAffine A;
    if (!free_out || mode < kXferCopy || mode > kXferConfident || (rule != kRsNearest && rule != kRsCover) ||
        !evid_params_ok(1, 1, lmin, lmax, threshold) || !rs_affine_ok(affine_host, frac_bits, A))
        return TOHIP_EINVAL;
    const void* bufs[6] = {src, dst, occupied_out, free_out, counts, scratch};
    for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b)
            if (bufs[a] && bufs[a] == bufs[b]) return TOHIP_EINVAL;
    const long long n_words = (long long)occ_words(gd.nx, gd.ny, gd.nz);
    const signed char* vals = (const signed char*)src + kEvidHdr;
    uint4* out = reinterpret_cast<uint4*>((char*)dst + kEvidHdr);
    const EvidParams p{0, 0, lmin + 128, lmax + 128, threshold + 128};
    const int blocks = occ_grid_blocks(n_words);
    hipStream_t st = (hipStream_t)stream_;
    if (rule == kRsNearest)
        k_evid_resample<kRsNearest><<<blocks, TO_BLOCK, 0, st>>>(vals, gs, out, gd, occ_data(occupied_out), occ_data(free_out), n_words, A, mode, p,
                                                                 (unsigned long long*)counts);
    else
        k_evid_resample<kRsCover><<<blocks, TO_BLOCK, 0, st>>>(vals, gs, out, gd, occ_data(occupied_out), occ_data(free_out), n_words, A, mode, p,
                                                               (unsigned long long*)counts);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
