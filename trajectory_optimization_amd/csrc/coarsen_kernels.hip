// coarsen_kernels.hip — f x f x f voxels of one box reduced to one voxel of a coarser box ("Coarsening maps"), for
// gfx950.  Included after resample_kernels.hip: the geometry, the brick layout, the brick mask, the per-wave count and the combine
// of two evidence values are the map layer's (OccGeom, occ_check, evid_check, occ_brick_mask, evid_brick, occ_inside, occ_count,
// xfer_combine4, the kXfer modes).
//
// A factor f in [2, 8] and an integer offset o: the CHILDREN of dst voxel d are the f^3 source voxels f d + o + e, e in [0, f)^3;
// a child outside src's dims is EMPTY (-128, bit 0).  Origins and resolutions are not interpreted: the host computes o.
//
// The work scales with the source, not with dst: G = 1, 2, 4 or 8 adjacent lanes share one dst voxel (f = 2, 3, 4, 5 .. 8), so a
// block of 256 lanes holds 8 / G dst bricks.  The f^2 rows (e_y, e_z) of a voxel's children are dealt round robin to its G lanes;
// a row of f children along x lies in at most three aligned dwords of the source's bricks (a brick row of four x values is one
// dword), which are loaded whole and masked to the children — the same loads for every offset, aligned or not.  Each lane keeps the
// maximum of a key that is a total order on the byte, the G lanes join theirs with wave shuffles (exact: a maximum is associative and
// commutative), lane 0 of the group puts the decoded byte into LDS, and after one barrier ONE lane per dst brick reads its 32 bytes
// and runs k_evid_transfer's tail unchanged: xfer_combine4, two 16-byte stores, the two plane words, the four counts.
//
//   keys (u = L + 128, T = threshold + 128; 0 is below every key and stands for "not a child"):
//     COVER   free u in [1, T] -> u;  unknown -> T + 1;  occupied u in [T + 1, 255] -> u + 1      (free < unknown < occupied)
//     MAX     u + 1                                                                              (the signed byte; -128 lowest)
//   planes: three bits joined by OR — a child is set; a child is clear or outside; a child of the veto plane is set.
//
// LDS is double buffered by the trip's parity, so one barrier per trip suffices: a lane can run at most one trip ahead of the
// assembling lane.  Integers only, no atomics on a plane or on the values, nothing read back; every argument check returns before
// anything is enqueued.
namespace {

constexpr int kCzMinFactor = 2, kCzMaxFactor = TOHIP_COARSEN_MAX_FACTOR, kCzMaxOffset = 1 << 20;
constexpr int kCzSlots = TO_BLOCK / 32;   // dst bricks of a block at one lane per voxel

struct CzPlan {
    int f, ox, oy, oz;
    int lg;    // log2 of the lanes per dst voxel
    int inv;   // ceil(1024 / f): r / f = (r inv) >> 10 for r < 64
};

inline bool cz_plan_ok(int f, int ox, int oy, int oz, CzPlan& c) {
    if (f < kCzMinFactor || f > kCzMaxFactor || ox < -kCzMaxOffset || ox > kCzMaxOffset || oy < -kCzMaxOffset || oy > kCzMaxOffset ||
        oz < -kCzMaxOffset || oz > kCzMaxOffset)
        return false;
    c = CzPlan{f, ox, oy, oz, f == 2 ? 0 : (f == 3 ? 1 : (f == 4 ? 2 : 3)), (1024 + f - 1) / f};
    return true;
}
inline int cz_blocks(long long n_words, const CzPlan& c) {
    const long long per = kCzSlots >> c.lg, b = (n_words + per - 1) / per;
    return (int)(b < 1 ? 1 : (b > kOccBlocks ? kOccBlocks : b));
}

// the lane's place in its block: the dst brick slot, the voxel of the brick (its bit) and the lane of the voxel's group
struct CzLane {
    int slot, vox, sub;
};
__device__ __forceinline__ CzLane cz_lane(const CzPlan& c) {
    const int t = (int)threadIdx.x;
    return CzLane{t >> (c.lg + 5), (t >> c.lg) & 31, t & ((1 << c.lg) - 1)};
}

// the evidence key of the lane's rows of the children of dst voxel (dx, dy, dz)
template <int RULE>
__device__ __forceinline__ unsigned cz_evid_rows(const signed char* __restrict__ vals, const OccGeom& gs, const CzPlan& c, int dx, int dy, int dz,
                                                 int sub, unsigned T) {
    const int x0 = c.f * dx + c.ox, y0 = c.f * dy + c.oy, z0 = c.f * dz + c.oz;
    const int b0 = x0 >> 2, b1 = (x0 + c.f - 1) >> 2;   // (>>: floor) the dwords of a row, at most three
    const unsigned empty = RULE == TOHIP_COARSEN_COVER ? T + 1u : 1u;
    unsigned best = 0u;
    for (int r = sub; r < c.f * c.f; r += 1 << c.lg) {
        const int ez = (r * c.inv) >> 10, ey = r - ez * c.f;
        const int y = y0 + ey, z = z0 + ez;
        if ((unsigned)y >= (unsigned)gs.ny || (unsigned)z >= (unsigned)gs.nz) {
            best = max(best, empty);
            continue;
        }
        const signed char* row = vals + 32ll * (((z >> 1) * gs.nby + (y >> 2)) * gs.nbx) + (((y & 3) << 2) | ((z & 1) << 4));
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int b = b0 + t;
            if (b > b1) break;
            if ((unsigned)b >= (unsigned)gs.nbx) {   // (a dword of the range holds at least one child)
                best = max(best, empty);
                continue;
            }
            const unsigned q = *reinterpret_cast<const unsigned*>(row + 32ll * b) ^ 0x80808080u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = 4 * b + j;
                const unsigned u = x < gs.nx ? (q >> (8 * j)) & 0xFFu : 0u;
                const unsigned key = RULE == TOHIP_COARSEN_COVER ? (u == 0u ? T + 1u : (u <= T ? u : u + 1u)) : u + 1u;
                best = max(best, x >= x0 && x < x0 + c.f ? key : 0u);
            }
        }
    }
    return best;
}

template <int RULE>
__global__ void __launch_bounds__(TO_BLOCK)
k_evid_coarsen(const signed char* __restrict__ src, OccGeom gs, uint4* __restrict__ dst, OccGeom gd, unsigned* __restrict__ occ_out,
               unsigned* __restrict__ fre_out, long long n_words, CzPlan c, int mode, EvidParams p, unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_vals[2][kCzSlots][8];   // [trip parity][dst brick of the block][row]: the brick's 32 source values
    const CzLane ln = cz_lane(c);
    const int per = kCzSlots >> c.lg;   // dst bricks per block and trip
    const long long n_trips = (n_words + per - 1) / per;
    const unsigned T = (unsigned)p.threshold;   // (biased)
    long long n_changed = 0, n_known = 0, appeared = 0, vanished = 0;
    int parity = 0;
    for (long long trip = blockIdx.x; trip < n_trips; trip += gridDim.x, parity ^= 1) {
        const long long w = trip * per + ln.slot;
        unsigned key = 0u;
        if (w < n_words) {
            int bx, by, bz;
            evid_brick(gd, (unsigned)w, bx, by, bz);
            const int dx = 4 * bx + (ln.vox & 3), dy = 4 * by + ((ln.vox >> 2) & 3), dz = 2 * bz + (ln.vox >> 4);
            if (occ_inside(gd, dx, dy, dz)) key = cz_evid_rows<RULE>(src, gs, c, dx, dy, dz, ln.sub, T);
        }
        for (int sh = 1; sh < (1 << c.lg); sh <<= 1) key = max(key, (unsigned)__shfl_xor((int)key, sh));
        if (ln.sub == 0) {
            // the key decoded to the biased byte, then to the value's own byte; a pad voxel of dst (key 0) holds -128
            const unsigned u = RULE == TOHIP_COARSEN_COVER ? (key <= T ? key : (key == T + 1u ? 0u : key - 1u)) : (key ? key - 1u : 0u);
            reinterpret_cast<unsigned char*>(s_vals[parity][ln.slot])[ln.vox] = (unsigned char)(u ^ 0x80u);
        }
        __syncthreads();
        const long long wb = trip * per + threadIdx.x;   // the lane that owns a dst brick: lanes 0 .. per - 1
        if ((int)threadIdx.x < per && wb < n_words) {
            int bx, by, bz;
            evid_brick(gd, (unsigned)wb, bx, by, bz);
            const unsigned in = occ_brick_mask(gd, bx, by, bz);
            unsigned v[8];
            unsigned any = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                v[k] = s_vals[parity][threadIdx.x][k];
                const unsigned x = v[k] ^ 0x80808080u, nib = (in >> (4 * k)) & 0xFu;
                any |= (x & 0xFFu ? nib & 1u : 0u) | (x & 0xFF00u ? nib & 2u : 0u) | (x & 0xFF0000u ? nib & 4u : 0u) | (x & 0xFF000000u ? nib & 8u : 0u);
            }
            if (mode == kXferCopy || any != 0u) {   // (otherwise: nothing to merge into this brick)
                unsigned d[8];
                if (mode == kXferCopy) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) d[k] = 0x80808080u;   // (dst's old content is not read: counted as empty)
                } else {
                    const uint4 lo = dst[2 * wb], hi = dst[2 * wb + 1];
                    d[0] = lo.x, d[1] = lo.y, d[2] = lo.z, d[3] = lo.w, d[4] = hi.x, d[5] = hi.y, d[6] = hi.z, d[7] = hi.w;
                }
                unsigned occ_old = 0u, occ_new = 0u, changed = 0u, newly = 0u, known = 0u;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    unsigned o4, n4, c4, w4, k4;
                    d[k] = xfer_combine4(d[k], v[k], (in >> (4 * k)) & 0xFu, mode, p, o4, n4, c4, w4, k4);
                    occ_old |= o4 << (4 * k), occ_new |= n4 << (4 * k), changed |= c4 << (4 * k), newly |= w4 << (4 * k), known |= k4 << (4 * k);
                }
                dst[2 * wb] = make_uint4(d[0], d[1], d[2], d[3]);
                dst[2 * wb + 1] = make_uint4(d[4], d[5], d[6], d[7]);
                occ_out[wb] = occ_new;
                fre_out[wb] = known & ~occ_new;
                n_changed += __popc(changed);
                n_known += __popc(newly);
                appeared += __popc(occ_new & ~occ_old);
                vanished += __popc(occ_old & ~occ_new);
            }
        }
    }
    if (counts && threadIdx.x < 64) {   // (the owning lanes all sit in the block's first wave)
        occ_count(counts, n_changed);
        occ_count(counts + 1, n_known);
        occ_count(counts + 2, appeared);
        occ_count(counts + 3, vanished);
    }
}

// the three bits of the lane's rows: 1 a child is set, 2 a child is clear or outside src's dims, 4 a child of the veto plane is set
__device__ __forceinline__ unsigned cz_occ_rows(const unsigned* __restrict__ words, const unsigned* __restrict__ veto, const OccGeom& gs,
                                                const CzPlan& c, int dx, int dy, int dz, int sub) {
    const int x0 = c.f * dx + c.ox, y0 = c.f * dy + c.oy, z0 = c.f * dz + c.oz;
    const int b0 = x0 >> 2, b1 = (x0 + c.f - 1) >> 2;
    unsigned got = 0u;
    for (int r = sub; r < c.f * c.f; r += 1 << c.lg) {
        const int ez = (r * c.inv) >> 10, ey = r - ez * c.f;
        const int y = y0 + ey, z = z0 + ez;
        if ((unsigned)y >= (unsigned)gs.ny || (unsigned)z >= (unsigned)gs.nz) {
            got |= 2u;
            continue;
        }
        const long long w0 = (long long)((z >> 1) * gs.nby + (y >> 2)) * gs.nbx;
        const int sh = ((y & 3) << 2) | ((z & 1) << 4);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int b = b0 + t;
            if (b > b1) break;
            if ((unsigned)b >= (unsigned)gs.nbx) {
                got |= 2u;
                continue;
            }
            // the children among the dword's four x values, and those of them inside dims
            const int lo = max(x0 - 4 * b, 0), hi = min(x0 + c.f - 4 * b, 4), hin = min(hi, gs.nx - 4 * b);
            const unsigned child = (0xFu >> (4 - hi)) & (0xFu << lo), inside = hin > lo ? (0xFu >> (4 - hin)) & child : 0u;
            const unsigned nib = (words[w0 + b] >> sh) & inside;
            got |= (nib != 0u ? 1u : 0u) | (nib != child ? 2u : 0u);
            if (veto) got |= ((veto[w0 + b] >> sh) & inside) != 0u ? 4u : 0u;
        }
    }
    return got;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_coarsen(const unsigned* __restrict__ src, const unsigned* __restrict__ veto, OccGeom gs, unsigned* __restrict__ dst, OccGeom gd,
              long long n_words, CzPlan c, int rule, int mode, unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_bits[2][kCzSlots][8];   // a byte per dst voxel: 1 where its source bit is set
    const CzLane ln = cz_lane(c);
    const int per = kCzSlots >> c.lg;
    const long long n_trips = (n_words + per - 1) / per;
    long long added = 0;
    int parity = 0;
    for (long long trip = blockIdx.x; trip < n_trips; trip += gridDim.x, parity ^= 1) {
        const long long w = trip * per + ln.slot;
        unsigned got = 2u;   // (a pad voxel of dst, or no brick: nothing set)
        if (w < n_words) {
            int bx, by, bz;
            evid_brick(gd, (unsigned)w, bx, by, bz);
            const int dx = 4 * bx + (ln.vox & 3), dy = 4 * by + ((ln.vox >> 2) & 3), dz = 2 * bz + (ln.vox >> 4);
            if (occ_inside(gd, dx, dy, dz)) got = cz_occ_rows(src, veto, gs, c, dx, dy, dz, ln.sub);
        }
        for (int sh = 1; sh < (1 << c.lg); sh <<= 1) got |= (unsigned)__shfl_xor((int)got, sh);
        if (ln.sub == 0) {
            const unsigned bit = rule == TOHIP_COARSEN_ANY ? (got & 1u) & ~(got >> 2) : ((got >> 1) & 1u) ^ 1u;
            reinterpret_cast<unsigned char*>(s_bits[parity][ln.slot])[ln.vox] = (unsigned char)bit;
        }
        __syncthreads();
        const long long wb = trip * per + threadIdx.x;
        if ((int)threadIdx.x < per && wb < n_words) {
            unsigned word = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {   // the low bits of four bytes -> a nibble
                const unsigned q = s_bits[parity][threadIdx.x][k];
                word |= ((q & 1u) | ((q >> 7) & 2u) | ((q >> 14) & 4u) | ((q >> 21) & 8u)) << (4 * k);
            }
            if (mode == kXferCopy) {
                dst[wb] = word;
                added += __popc(word);
            } else if (word != 0u) {
                const unsigned old = dst[wb];
                if ((word & ~old) != 0u) dst[wb] = old | word;
                added += __popc(word & ~old);
            }
        }
    }
    if (counts && threadIdx.x < 64) occ_count(counts, added);
}

}  // namespace

extern "C" int tohip_occ_coarsen(const void* src, size_t src_bytes, const tohip_occ_geom* src_geom, const void* veto_or_null, void* dst,
                                 size_t dst_bytes, const tohip_occ_geom* dst_geom, int32_t factor, int32_t ox, int32_t oy, int32_t oz, int32_t rule,
                                 int32_t mode, uint64_t* counts, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom gs, gd;
    int rc = occ_check(src, src_bytes, src_geom, gs);
    if (rc != TOHIP_OK) return rc;
    rc = occ_check(dst, dst_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    CzPlan c;
    if (src == dst || veto_or_null == dst || veto_or_null == src || (const void*)counts == src || (void*)counts == dst ||
        (counts && (const void*)counts == veto_or_null) || (mode != kXferCopy && mode != kXferOr) ||
        (rule != TOHIP_COARSEN_ANY && rule != TOHIP_COARSEN_ALL) || (veto_or_null && rule != TOHIP_COARSEN_ANY) || !cz_plan_ok(factor, ox, oy, oz, c))
        return TOHIP_EINVAL;
    const long long n_words = (long long)occ_words(gd.nx, gd.ny, gd.nz);
    k_occ_coarsen<<<cz_blocks(n_words, c), TO_BLOCK, 0, (hipStream_t)stream_>>>(occ_data(src), veto_or_null ? occ_data(veto_or_null) : nullptr, gs,
                                                                               occ_data(dst), gd, n_words, c, rule, mode, (unsigned long long*)counts);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_evid_coarsen(const void* src, size_t src_bytes, const tohip_occ_geom* src_geom, void* dst, size_t dst_bytes,
                                  const tohip_occ_geom* dst_geom, void* occupied_out, void* free_out, size_t grid_bytes, int32_t factor, int32_t ox,
                                  int32_t oy, int32_t oz, int32_t rule, int32_t mode, int32_t lmin, int32_t lmax, int32_t threshold, uint64_t* counts,
                                  void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom gs, gd;
    int rc = evid_check(src, src_bytes, src_geom, gs);
    if (rc != TOHIP_OK) return rc;
    rc = evid_check(dst, dst_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    rc = occ_check(occupied_out, grid_bytes, dst_geom, gd);
    if (rc != TOHIP_OK) return rc;
    CzPlan c;
    if (!free_out || mode < kXferCopy || mode > kXferConfident || (rule != TOHIP_COARSEN_COVER && rule != TOHIP_COARSEN_MAX) ||
        !evid_params_ok(1, 1, lmin, lmax, threshold) || !cz_plan_ok(factor, ox, oy, oz, c))
        return TOHIP_EINVAL;
    const void* bufs[5] = {src, dst, occupied_out, free_out, counts};
    for (int a = 0; a < 5; ++a)
        for (int b = a + 1; b < 5; ++b)
            if (bufs[a] == bufs[b]) return TOHIP_EINVAL;
    const long long n_words = (long long)occ_words(gd.nx, gd.ny, gd.nz);
    const signed char* vals = (const signed char*)src + kEvidHdr;
    uint4* out = reinterpret_cast<uint4*>((char*)dst + kEvidHdr);
    const EvidParams p{0, 0, lmin + 128, lmax + 128, threshold + 128};
    const int blocks = cz_blocks(n_words, c);
    hipStream_t st = (hipStream_t)stream_;
    if (rule == TOHIP_COARSEN_COVER)
        k_evid_coarsen<TOHIP_COARSEN_COVER><<<blocks, TO_BLOCK, 0, st>>>(vals, gs, out, gd, occ_data(occupied_out), occ_data(free_out), n_words, c,
                                                                         mode, p, (unsigned long long*)counts);
    else
        k_evid_coarsen<TOHIP_COARSEN_MAX><<<blocks, TO_BLOCK, 0, st>>>(vals, gs, out, gd, occ_data(occupied_out), occ_data(free_out), n_words, c, mode,
                                                                       p, (unsigned long long*)counts);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
