// volume_kernels.hip — the unknown volume a view would reveal, and the greedy choice of views by it ("Unknown volume"),
// for gfx950.  Included after frontier_kernels.hip (behind the field and evidence files): the geometry, the fixed-point coordinates,
// the brick layout, the walk (los_walk), the dims mask (occ_brick_mask) and the centre rule of the listing are the occupancy and
// frontier files'; the cull is exact_pose / exact_to_cam / frustum_pred, the device functions tohip_cull_waypoints runs.
//
// A voxel v inside dims is REVEALED by a view (t, q) when its state is 0 (neither plane's bit) and its `claimed` bit is 0, its centre
// c = fl(origin + fl(fl(i + 0.5) r)) is kept by the cull (dist && fov), and los_walk(occupied, t -> c, start_skip 1, end_skip 0) is
// clear.  gain(view) = the number of revealed voxels.
//
//   k_occ_unknown      one lane per brick word: ~occ & ~free & (inside dims).
//   k_view_volume      grid (slabs of the view's brick window) x (views), two passes per slab like k_los_rows.  A slab is 256 bricks
//                      of the window, one word per lane: 8192 voxels at most, which is the queue's capacity — a slab of fully unknown,
//                      fully kept bricks (an unexplored map) fills it exactly.  Pass 1: the lane's word of the three planes, zero:
//                      done; per set bit the centre, the exact transform and frustum_pred; the kept bits of the wave are given
//                      their places in the LDS queue with one LDS counter add per wave.  Pass 2: the block's lanes drain the queue,
//                      one los_walk each; survivors are counted and, with a mark plane, gathered per brick word in LDS; the lane
//                      that owns the word issues the 32-bit atomic OR only where the word lacks a bit.  One 64-bit integer atomic
//                      add per block into gains[view].
//   the window         per view a box of bricks that holds every voxel the cull can keep: the apex and the four corner rays of the
//                      pixel rectangle widened by a pixel, at max_dist, rotated by the pose, padded by two voxels and a rounding
//                      slack, clipped to dims — computed by every block from the pose, so poses never visit the host.  Inside the
//                      window a brick whose bounding sphere cannot pass the depth gate is not tested (los_tile_reachable's slack).
//                      window = 0 enumerates every brick and tests every unknown voxel: the same counts.
//   k_view_volume_pick one block: the largest gain among the candidates not taken, the lowest index on ties.
//
//
// INFORMATION GAIN ("Information gain"): the same kernel scores a view by what is left to learn about the voxels it
// sees.  A table W of 256 unsigned 16-bit weights is indexed by the evidence byte read as unsigned, L + 128; a voxel inside dims is a
// CANDIDATE iff W[byte] > 0, whatever its state; it is INFORMED by a view under the cull and the walk above (the target voxel is not
// tested, so a weakly occupied surface voxel can be informed); gain(view) = the sum of W[byte] over the informed voxels.
//
//   k_evid_weight_plane  one lane per brick word: the table staged in LDS (512 B), the lane's 32 bytes as two 16-byte loads, the
//                        candidate word (pad bits 0) stored; block 0 zeroes the header; with a total, one 64-bit integer atomic add
//                        per block of the weights of the block's voxels inside dims.
//   k_view_volume<true>  the weighted instantiation (the switch is a template parameter; the unweighted kernel is the code it was):
//                        the candidate word comes from the plane, the table is staged in LDS, and pass 2 gathers W[byte at 32 w + b]
//                        of each queued voxel in front of its walk (one register stays live across the walk, the load hides
//                        under it) and adds it per survivor instead of 1.
//
// Integer counts, integer atomics, no process-wide state, nothing read back: a selection never synchronises with the host.
namespace {

constexpr int kVolSlab = TO_BLOCK;        // brick words per slab, one per lane
constexpr int kVolQueue = kVolSlab * 32;  // every voxel of a slab: the queue cannot overflow
constexpr int kVolMaxSlabBlocks = 2048;   // blocks along x; a view with more slabs strides

__global__ void __launch_bounds__(TO_BLOCK)
k_occ_unknown(const unsigned* __restrict__ occ, const unsigned* __restrict__ fre, unsigned* __restrict__ out, OccGeom g, long long n_words) {
    const long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    if (w >= n_words) return;
    int bx, by, bz;
    occ_brick(g, w, bx, by, bz);
    out[w] = ~occ[w] & ~fre[w] & occ_brick_mask(g, bx, by, bz);
}

// the candidate word of every brick under a weight table, and the map's remaining information
__global__ void __launch_bounds__(TO_BLOCK)
k_evid_weight_plane(const uint4* __restrict__ vals, const unsigned short* __restrict__ table, unsigned* __restrict__ hdr, unsigned* __restrict__ out,
                    OccGeom g, long long n_words, unsigned long long* __restrict__ total) {
    __shared__ unsigned short s_table[256];
    __shared__ unsigned long long s_wave[TO_BLOCK / 64];
    static_assert(TO_BLOCK == 256, "one table entry per lane");
    s_table[threadIdx.x] = table[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x < (int)(kOccHdr / 4)) hdr[threadIdx.x] = 0u;   // the header as tohip_occ_init leaves it
    __syncthreads();
    const long long w = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    unsigned long long sum = 0;
    if (w < n_words) {
        int bx, by, bz;
        evid_brick(g, (unsigned)w, bx, by, bz);
        const unsigned in = occ_brick_mask(g, bx, by, bz);
        const uint4 lo = vals[2 * w], hi = vals[2 * w + 1];
        const unsigned v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        unsigned cand = 0u, lane_sum = 0u;   // (32 weights below 2^16)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned x = v[k] ^ 0x80808080u;   // the bytes biased to L + 128
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned wt = ((in >> (4 * k + j)) & 1u) ? (unsigned)s_table[(x >> (8 * j)) & 0xFFu] : 0u;
                cand |= (wt != 0u ? 1u : 0u) << (4 * k + j);
                lane_sum += wt;
            }
        }
        out[w] = cand;
        sum = lane_sum;
    }
    if (total) {   // (uniform)
        for (int sh = 32; sh > 0; sh >>= 1) sum += __shfl_xor(sum, sh);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long t = 0;
            for (int k = 0; k < TO_BLOCK / 64; ++k) t += s_wave[k];
            if (t != 0) __hip_atomic_fetch_add(total, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

struct ViewVolumeArgs {
    const unsigned* occ;
    const unsigned* fre;
    const unsigned* claimed;   // may be null; may be `mark` when one view is scored
    unsigned* mark;            // may be null
    OccGeom g;
    int nbz;
    const float* poses;
    const float* quats;
    int n_views;
    const int* view_index;     // may be null
    FrustumConsts f;
    int window;
    double ray_x[4], ray_y[4];   // X / Z and Y / Z of the widened pixel rectangle's corner rays
    unsigned long long* gains;
    const int* stop;
    unsigned long long* stats;
    // the weighted instantiation only (behind every earlier field: the unweighted kernel's argument offsets stay)
    const unsigned* cand;            // the candidate plane's words: stands where ~occ & ~free stood
    const unsigned char* bytes;      // the evidence values in brick order, byte 32 w + b
    const unsigned short* table;     // 256 weights, indexed by L + 128
};

struct VolWindow {
    int x0, y0, z0, wx, wy, wz;   // in bricks
};

// the voxel range [v0, v1] of one axis that holds world [lo, hi] padded by `pad` voxels, clipped to [0, n); v0 > v1: none
__device__ __forceinline__ void vol_axis(double lo, double hi, double o, double r, double pad, int n, int& v0, int& v1) {
    const double glo = (lo - o) / r - pad, ghi = (hi - o) / r + pad;
    v0 = glo <= 0.0 ? 0 : (glo >= (double)n ? n : (int)glo);
    v1 = ghi >= (double)(n - 1) ? n - 1 : (ghi < 0.0 ? -1 : (int)ghi);
}

// the brick box of a view: a superset of every voxel whose centre the cull can keep.  Anything not finite: the whole grid.
__device__ __forceinline__ VolWindow vol_window(const ViewVolumeArgs& a, const ExactPose& e) {
    const VolWindow all = {0, 0, 0, a.g.nbx, a.g.nby, a.nbz};
    if (!a.window) return all;
    const double qw = e.q[0], qx = e.q[1], qy = e.q[2], qz = e.q[3];
    const double n2 = qw * qw + qx * qx + qy * qy + qz * qz;
    if (!(n2 > 0.5 && n2 < 2.0)) return all;
    // camera -> world: p = R cam / n2^2 + t with R = n2 x the rotation of q (exact_to_cam applies conj(q) . q without dividing by n2)
    const double R[3][3] = {{(qw * qw + qx * qx - qy * qy - qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)},
                            {2.0 * (qx * qy + qw * qz), (qw * qw - qx * qx + qy * qy - qz * qz), 2.0 * (qy * qz - qw * qx)},
                            {2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), (qw * qw - qx * qx - qy * qy + qz * qz)}};
    const double D = (double)a.f.dmax * 1.0001 / (n2 * n2);
    const double t[3] = {e.t[0], e.t[1], e.t[2]};
    double lo[3] = {t[0], t[1], t[2]}, hi[3] = {t[0], t[1], t[2]}, spread = 1.0;
    bool bad = false;
    for (int k = 0; k < 4; ++k) {
        const double c[3] = {a.ray_x[k] * D, a.ray_y[k] * D, D};
        spread = fmax(spread, fmax(fabs(a.ray_x[k]), fabs(a.ray_y[k])));
        for (int ax = 0; ax < 3; ++ax) {
            const double p = t[ax] + R[ax][0] * c[0] + R[ax][1] * c[1] + R[ax][2] * c[2];
            bad |= !isfinite(p);
            lo[ax] = p < lo[ax] ? p : lo[ax];
            hi[ax] = p > hi[ax] ? p : hi[ax];
        }
    }
    const double o[3] = {a.g.ox, a.g.oy, a.g.oz}, r = a.g.r;
    const double big = fmax(fmax(fabs(t[0]), fabs(t[1])), fabs(t[2])) + fmax(fmax(fabs(o[0]), fabs(o[1])), fabs(o[2])) + fabs(D) * (1.0 + 2.0 * spread);
    const double pad = 2.0 + 1e-5 * big / r;   // two voxels, and every rounding of the f32 transform a hundredfold
    if (bad || !isfinite(pad)) return all;
    int x0, x1, y0, y1, z0, z1;
    vol_axis(lo[0], hi[0], o[0], r, pad, a.g.nx, x0, x1);
    vol_axis(lo[1], hi[1], o[1], r, pad, a.g.ny, y0, y1);
    vol_axis(lo[2], hi[2], o[2], r, pad, a.g.nz, z0, z1);
    if (x0 > x1 || y0 > y1 || z0 > z1) return VolWindow{0, 0, 0, 0, 0, 0};
    return VolWindow{x0 >> 2, y0 >> 2, z0 >> 1, (x1 >> 2) - (x0 >> 2) + 1, (y1 >> 2) - (y0 >> 2) + 1, (z1 >> 1) - (z0 >> 1) + 1};
}

// brick number li of the window, x fastest
__device__ __forceinline__ void vol_brick(const VolWindow& w, long long li, int& bx, int& by, int& bz) {
    bx = w.x0 + (int)(li % w.wx), by = w.y0 + (int)((li / w.wx) % w.wy), bz = w.z0 + (int)(li / ((long long)w.wx * w.wy));
}

// the centre of voxel (x, y, z): tohip_occ_export's bits
__device__ __forceinline__ void vol_centre(const OccGeom& g, int x, int y, int z, float& cx, float& cy, float& cz) {
    cx = __fadd_rn(g.ox, __fmul_rn((float)x + 0.5f, g.r));
    cy = __fadd_rn(g.oy, __fmul_rn((float)y + 0.5f, g.r));
    cz = __fadd_rn(g.oz, __fmul_rn((float)z + 0.5f, g.r));
}

// can a voxel centre of the brick pass the depth gate?  Its centres lie within 3 r of the brick's middle (half extents 2 r, 2 r, r).
__device__ __forceinline__ bool vol_brick_reachable(const OccGeom& g, const ExactPose& e, const FrustumConsts& f, int bx, int by, int bz) {
    const float4 b = {g.ox + (float)(4 * bx + 2) * g.r, g.oy + (float)(4 * by + 2) * g.r, g.oz + (float)(2 * bz + 1) * g.r, 3.03f * g.r};
    return los_tile_reachable(e, f, b);
}

// kWeighted: the candidates are the plane's and a survivor adds its weight from the table; else neither the plane, the bytes nor the
// table is read
template <bool kWeighted>
__global__ void __launch_bounds__(TO_BLOCK) k_view_volume(ViewVolumeArgs a) {
    __shared__ unsigned short s_queue[kVolQueue];
    __shared__ unsigned s_mark[kVolSlab];
    __shared__ long long s_wave[TO_BLOCK / 64];
    __shared__ int s_count;
    if (a.stop && *a.stop != 0) return;   // (uniform)
    int view = blockIdx.y;
    if (a.view_index) {
        view = *a.view_index;
        if (view < 0 || view >= a.n_views) return;   // (uniform)
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ExactPose e = exact_pose(a.quats + 4 * (long long)view, a.poses + 3 * (long long)view, 1);
    int cx, cy, cz;
    if (!occ_fixed(a.g, e.t[0], e.t[1], e.t[2], cx, cy, cz)) return;   // (uniform) a camera out of range reveals nothing
    const VolWindow win = vol_window(a, e);
    const long long nw = (long long)win.wx * win.wy * win.wz;
    long long revealed = 0, centres = 0, rays = 0, visits = 0;
    const unsigned short* weight = nullptr;
    if constexpr (kWeighted) {
        __shared__ unsigned short s_table[256];
        static_assert(TO_BLOCK == 256, "one table entry per lane");
        s_table[threadIdx.x] = a.table[threadIdx.x];   // (visible behind the first barrier of the slab loop)
        weight = s_table;
    }
    for (long long first = (long long)blockIdx.x * kVolSlab; first < nw; first += (long long)gridDim.x * kVolSlab) {   // (uniform)
        if (threadIdx.x == 0) s_count = 0;
        s_mark[threadIdx.x] = 0u;
        __syncthreads();
        // pass 1: this lane's brick word; the exact cull of the centre of every unknown, unclaimed voxel
        const long long li = first + threadIdx.x;
        long long w = -1;
        unsigned kept = 0u;
        if (li < nw) {
            int bx, by, bz;
            vol_brick(win, li, bx, by, bz);
            w = ((long long)bz * a.g.nby + by) * a.g.nbx + bx;
            unsigned u;
            if constexpr (kWeighted) u = a.cand[w];   // (pad bits 0: k_evid_weight_plane masked them)
            else u = ~a.occ[w] & ~a.fre[w] & occ_brick_mask(a.g, bx, by, bz);
            if (a.claimed) u &= ~a.claimed[w];
            if (u != 0u && a.window && !vol_brick_reachable(a.g, e, a.f, bx, by, bz)) u = 0u;
            while (u != 0u) {
                const int b = __ffs(u) - 1;
                u &= u - 1u;
                int x, y, z;
                occ_voxel(bx, by, bz, b, x, y, z);
                float px, py, pz, X, Y, Z;
                vol_centre(a.g, x, y, z, px, py, pz);
                exact_to_cam(e, px, py, pz, X, Y, Z);
                bool d, v;
                frustum_pred(a.f, X, Y, Z, d, v);
                ++centres;
                if (d && v) kept |= 1u << b;
            }
        }
        // the wave's kept voxels get their places in the queue: one LDS add per wave
        const int c = __popc(kept);
        int incl = c;
        for (int sh = 1; sh < 64; sh <<= 1) {
            const int t = __shfl_up(incl, sh);
            if (lane >= sh) incl += t;
        }
        int base = 0;
        if (lane == 63 && incl != 0) base = atomicAdd(&s_count, incl);
        base = __shfl(base, 63);
        int at = base + incl - c;
        while (kept != 0u) {
            const int b = __ffs(kept) - 1;
            kept &= kept - 1u;
            s_queue[at++] = (unsigned short)((threadIdx.x << 5) | b);
        }
        __syncthreads();
        // pass 2: the block's lanes drain the queue, one walk each
        const int count = s_count;
        for (int k = threadIdx.x; k < count; k += TO_BLOCK) {
            const int ent = s_queue[k], l = ent >> 5, b = ent & 31;
            int bx, by, bz, x, y, z, tx, ty, tz;
            vol_brick(win, first + l, bx, by, bz);
            occ_voxel(bx, by, bz, b, x, y, z);
            float px, py, pz;
            vol_centre(a.g, x, y, z, px, py, pz);
            if (!occ_fixed(a.g, px, py, pz, tx, ty, tz)) continue;
            [[maybe_unused]] unsigned wt = 1u;   // the byte is gathered before the walk: its latency hides under it, and only the weight stays live
            if constexpr (kWeighted) wt = weight[a.bytes[32 * (((long long)bz * a.g.nby + by) * a.g.nbx + bx) + b] ^ 0x80u];
            unsigned v = 0;
            const int clear = los_walk(a.occ, a.g, cx, cy, cz, tx, ty, tz, 1, 0, v);
            ++rays;
            visits += v;
            if (clear) {
                if constexpr (kWeighted) revealed += wt;
                else ++revealed;
                if (a.mark) atomicOr(&s_mark[l], 1u << b);
            }
        }
        __syncthreads();
        // the survivors of this lane's word: the atomic only where the plane lacks one of them
        if (a.mark && w >= 0) {
            const unsigned bits = s_mark[threadIdx.x];
            if (bits != 0u && (a.mark[w] & bits) != bits) __hip_atomic_fetch_or(a.mark + w, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
    for (int sh = 32; sh > 0; sh >>= 1) revealed += __shfl_xor(revealed, sh);
    if (lane == 0) s_wave[wave] = revealed;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long total = 0;
        for (int k = 0; k < TO_BLOCK / 64; ++k) total += s_wave[k];
        if (total != 0) __hip_atomic_fetch_add(a.gains + view, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (a.stats) { occ_count(a.stats, centres); occ_count(a.stats + 1, rays); occ_count(a.stats + 2, visits); }
}

// round `round` of a greedy selection: the largest gain among the candidates not taken, the lowest index on ties
__global__ void __launch_bounds__(TO_BLOCK)
k_view_volume_pick(const long long* __restrict__ gains, int* __restrict__ taken, long long n, long long min_gain, int round, int* __restrict__ order,
                   long long* __restrict__ picked_gain, int* __restrict__ stop) {
    __shared__ long long s_gain[TO_BLOCK];
    __shared__ long long s_idx[TO_BLOCK];
    if (*stop != 0) return;   // (uniform)
    long long best = -1, at = -1;
    for (long long i = threadIdx.x; i < n; i += TO_BLOCK)   // (ascending: the first of equal gains stays)
        if (!taken[i] && gains[i] > best) { best = gains[i]; at = i; }
    s_gain[threadIdx.x] = best;
    s_idx[threadIdx.x] = at;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TO_BLOCK; ++k)
            if (s_gain[k] > best || (s_gain[k] == best && s_idx[k] >= 0 && s_idx[k] < at)) { best = s_gain[k]; at = s_idx[k]; }
        if (at < 0 || best < min_gain) {
            *stop = 1;
        } else {
            order[round] = (int)at;
            picked_gain[round] = best;
            taken[at] = 1;
        }
    }
}

// K = (fx s cx; 0 fy cy; 0 0 1): the corner rays of the pixel rectangle widened by a pixel; false for any other K (no window then)
inline bool vol_corner_rays(const FrustumConsts& f, double* rx, double* ry) {
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(f.k[i])) return false;
    if (!(f.k[0] > 0.f) || !(f.k[4] > 0.f) || f.k[3] != 0.f || f.k[6] != 0.f || f.k[7] != 0.f || f.k[8] != 1.f) return false;
    if (!std::isfinite(f.wl) || !std::isfinite(f.hl)) return false;
    const double us[2] = {0.0, (double)f.wl + 1.0}, vs[2] = {0.0, (double)f.hl + 1.0};
    for (int k = 0; k < 4; ++k) {
        const double y = (vs[k >> 1] - (double)f.k[5]) / (double)f.k[4];
        ry[k] = y;
        rx[k] = (us[k & 1] - (double)f.k[2] - (double)f.k[1] * y) / (double)f.k[0];
    }
    return true;
}

}  // namespace

extern "C" int tohip_occ_unknown(const void* occupied, const void* free_grid, void* out, size_t grid_bytes, const tohip_occ_geom* geom,
                                 void* stream_) {
    OccGeom g;
    const int rc = occ_check(out, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!occupied || !free_grid || out == occupied || out == free_grid) return TOHIP_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    const OccMaskLaunch m = occ_mask_begin(out, g, st);
    if (m.rc != TOHIP_OK) return m.rc;
    k_occ_unknown<<<m.blocks, TO_BLOCK, 0, st>>>(occ_data(occupied), occ_data(free_grid), occ_data(out), g, m.n_words);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

namespace {

// what the weighted instantiation reads beyond tohip_view_volume's arguments; all null: the unweighted kernel
struct ViewWeights {
    const void* evidence;
    size_t evid_bytes;
    const uint16_t* table;
    const void* candidates;
};

// tohip_view_volume and tohip_view_information: one set of checks, one launch
int view_volume_launch(const void* occupied, const void* free_grid, const void* claimed, void* mark, size_t grid_bytes, const tohip_occ_geom* geom,
                       const ViewWeights* wt, const float* poses, const float* quats, int64_t n_views, const int32_t* view_index,
                       const tohip_camera* cam, float min_dist, float max_dist, int32_t window, int64_t* gains, const int32_t* stop, uint64_t* stats,
                       void* stream_) {
    OccGeom g;
    const int rc = occ_check(occupied, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (wt) {
        OccGeom ge;
        const int re = evid_check(wt->evidence, wt->evid_bytes, geom, ge);
        if (re != TOHIP_OK) return re;
        if (!wt->table || ((uintptr_t)wt->table & 1u) != 0 || !wt->candidates) return TOHIP_EINVAL;
        const void* others[4] = {occupied, free_grid, mark, wt->evidence};   // (free_grid is not read: it is here to be told apart)
        for (const void* o : others)
            if (wt->candidates == o) return TOHIP_EINVAL;
    }
    if (!free_grid || free_grid == occupied || !poses || !quats || !cam || !gains || n_views < 1 || n_views > 65535) return TOHIP_EINVAL;
    if (mark && (mark == occupied || mark == free_grid)) return TOHIP_EINVAL;
    if (mark && mark == claimed && n_views > 1 && !view_index) return TOHIP_EINVAL;   // two views' lanes would race on one word
    hipStream_t st = (hipStream_t)stream_;
    ViewVolumeArgs a;
    a.occ = occ_data(occupied);
    a.fre = occ_data(free_grid);
    a.claimed = claimed ? occ_data(claimed) : nullptr;
    a.mark = mark ? occ_data(mark) : nullptr;
    a.g = g;
    a.nbz = (g.nz + 1) / 2;
    a.poses = poses;
    a.quats = quats;
    a.n_views = (int)n_views;
    a.view_index = view_index;
    for (int i = 0; i < 9; ++i) a.f.k[i] = cam->K[i];
    a.f.wl = (float)((double)cam->img_width - 1.0);
    a.f.hl = (float)((double)cam->img_height - 1.0);
    a.f.dmin = min_dist;
    a.f.dmax = max_dist;
    for (int k = 0; k < 4; ++k) a.ray_x[k] = a.ray_y[k] = 0.0;
    a.window = (window != 0 && vol_corner_rays(a.f, a.ray_x, a.ray_y)) ? 1 : 0;
    a.gains = (unsigned long long*)gains;
    a.stop = stop;
    a.stats = (unsigned long long*)stats;
    a.cand = wt ? occ_data(wt->candidates) : nullptr;
    a.bytes = wt ? (const unsigned char*)wt->evidence + kEvidHdr : nullptr;
    a.table = wt ? wt->table : nullptr;
    const hipError_t e = hipMemsetAsync(gains, 0, sizeof(int64_t) * (size_t)n_views, st);
    if (e != hipSuccess) return (int)e;
    const int64_t slabs = ((int64_t)occ_words(g.nx, g.ny, g.nz) + kVolSlab - 1) / kVolSlab;
    const dim3 grid_dim((unsigned)(slabs < kVolMaxSlabBlocks ? slabs : kVolMaxSlabBlocks), view_index ? 1u : (unsigned)n_views);
    if (wt)
        k_view_volume<true><<<grid_dim, TO_BLOCK, 0, st>>>(a);
    else
        k_view_volume<false><<<grid_dim, TO_BLOCK, 0, st>>>(a);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

}  // namespace

extern "C" int tohip_view_volume(const void* occupied, const void* free_grid, const void* claimed, void* mark, size_t grid_bytes,
                                 const tohip_occ_geom* geom, const float* poses, const float* quats, int64_t n_views, const int32_t* view_index,
                                 const tohip_camera* cam, float min_dist, float max_dist, int32_t window, int64_t* gains, const int32_t* stop,
                                 uint64_t* stats, void* stream_) {
    return view_volume_launch(occupied, free_grid, claimed, mark, grid_bytes, geom, nullptr, poses, quats, n_views, view_index, cam, min_dist,
                              max_dist, window, gains, stop, stats, stream_);
}

extern "C" int tohip_evid_weight_plane(const void* evidence, size_t evid_bytes, const tohip_occ_geom* geom, const uint16_t* table, void* plane_out,
                                       size_t grid_bytes, int64_t* total_out, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    OccGeom g;
    int rc = evid_check(evidence, evid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    rc = occ_check(plane_out, grid_bytes, geom, g);
    if (rc != TOHIP_OK) return rc;
    if (!table || ((uintptr_t)table & 1u) != 0 || plane_out == evidence || ((uintptr_t)plane_out & 3u) != 0) return TOHIP_EINVAL;
    const long long n_words = (long long)occ_words(g.nx, g.ny, g.nz);
    k_evid_weight_plane<<<(unsigned)occ_list_blocks(g), TO_BLOCK, 0, (hipStream_t)stream_>>>(
        reinterpret_cast<const uint4*>((const char*)evidence + kEvidHdr), table, (unsigned*)plane_out, occ_data(plane_out), g, n_words,
        (unsigned long long*)total_out);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_view_information(const void* occupied, const void* free_grid, const void* claimed, void* mark, size_t grid_bytes,
                                      const tohip_occ_geom* geom, const void* evidence, size_t evid_bytes, const uint16_t* table,
                                      const void* candidates, const float* poses, const float* quats, int64_t n_views, const int32_t* view_index,
                                      const tohip_camera* cam, float min_dist, float max_dist, int32_t window, int64_t* gains, const int32_t* stop,
                                      uint64_t* stats, void* stream_, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    const ViewWeights wt = {evidence, evid_bytes, table, candidates};
    return view_volume_launch(occupied, free_grid, claimed, mark, grid_bytes, geom, &wt, poses, quats, n_views, view_index, cam, min_dist, max_dist,
                              window, gains, stop, stats, stream_);
}

extern "C" int tohip_view_volume_pick(const int64_t* gains, int32_t* taken, int64_t n_views, int64_t min_gain, int32_t round, int32_t* order,
                                      int64_t* picked_gain, int32_t* stop, void* stream_) {
    if (!gains || !taken || !order || !picked_gain || !stop || n_views < 1 || n_views > (int64_t)0x7fffffff || min_gain < 1 || round < 0)
        return TOHIP_EINVAL;
    k_view_volume_pick<<<1, TO_BLOCK, 0, (hipStream_t)stream_>>>((const long long*)gains, taken, (long long)n_views, (long long)min_gain, round,
                                                                 order, (long long*)picked_gain, stop);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
