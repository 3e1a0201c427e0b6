// posegraph_kernels.hip — pose-graph optimisation ("Pose graph"), for gfx950: Levenberg–Marquardt over the poses of a
// graph whose edges are relative (or absolute) pose measurements with 6 x 6 information matrices; each damped step solved by
// conjugate gradients with a block-Jacobi preconditioner.  Everything is f64 add, subtract, multiply, divide and compare in the ONE
// order synth.py states (pose_graph_*_ref), compiled with contraction off: the device gives the restatement's bits.
//
// THE ORDERS.  A 6-term product sum runs in ascending index from its first product.  A node's sums over its incident edges start at
//   0.0 and follow the host-built CSR list, ascending edge index.  A sum over nodes or edges is a halving tree over each block of 256
//   in LDS (pg_tree), then the block partials from 0.0 in ascending block order (pg_sum), re-done by whoever needs the scalar.
// THE SCALARS (kPgS words) live in three copies so that no block reads a word another block of the same launch writes: HOME (1) is
//   what linearise, gather and result read; k_pg_step reads HOME and writes copy 2; the first k_pg_spmv of a solve reads 2 and
//   writes 0, a later one reads HOME and writes 0; k_pg_update reads 0 and writes HOME.  Thread 0 of block 0 always copies, also in a
//   frozen launch.  Kernel boundaries are the only global synchronisation; there is no atomic, no spin wait, nothing read back.
// THE INVARIANT, for every array as for the scalars: NO BLOCK READS A WORD THAT ANOTHER BLOCK OF THE SAME LAUNCH WRITES.  A launch reads
//   other blocks' data only from arrays that an EARLIER launch finished: the partial arrays (cost, r.z, p.Ap) and the flag arrays
//   (small step, bad pivot) are written per block by one launch and summed by a later one; k_pg_spmv reads its neighbours' z and the
//   previous p and writes the other p buffer; k_pg_step, which resets the small-step flags, does not read them: k_pg_gather's first
//   thread, one launch earlier, has reduced them into the word behind the trial cost.
//
//   k_pg_linearize  one lane per edge, at the TRIAL nodes (current moved by the pending step x): the record (100 f64) into the edge
//                   buffer that is not current, and the block's partial of rho.
//   k_pg_gather     one lane per node: diagonal block (21) and gradient (6) over the CSR list into the node buffer that is not
//                   current; thread 0 of block 0 sums the cost partials into the trial-cost word and ANDs the small-step flags of
//                   the solve before into the word behind it.
//   k_pg_step       accept or reject (every block decides alike from HOME and the trial cost), lambda, statuses; per node: the
//                   accepted pose, L d L^T of the damped block, x = 0, r = 0 - g, z = M^-1 r, the r.z partial.
//   k_pg_spmv       beta and p = z + beta p on the fly (its own and its neighbours'), A p by node rows, the p.Ap partial.
//   k_pg_update     alpha, x, r, z, the r.z partial, the block's step-is-small flag.
//   k_pg_result     the scalars, the poses, chi^2 and the weights into one buffer: the caller's single read-back.
namespace {

#pragma clang fp contract(off)

constexpr int kPgEdge = TOHIP_POSEGRAPH_EDGE;   // f64 words of an edge's record
constexpr int kPgNode = 27;                     // D (21) and g (6)
constexpr int kPgS = TOHIP_POSEGRAPH_SCALARS;   // words of one copy of the scalars
constexpr long long kPgMax = 1ll << 22;         // nodes, and edges
// the record's words
constexpr int kPgRS = 6, kPgRW = 7, kPgRRho = 8, kPgHaa = 10, kPgHbb = 31, kPgHab = 52, kPgGa = 88, kPgGb = 94;
// the scalars' words (f64 unless named an integer)
constexpr int kPgLam = 0, kPgCost = 1, kPgCost0 = 2, kPgStatus = 3 /* int */, kPgIter = 4 /* int */, kPgAccepted = 5 /* int */, kPgCgTotal = 6 /* int */,
              kPgSel = 7 /* int */, kPgRz = 8, kPgRz0 = 9, kPgCgStop = 10 /* int */, kPgHave = 11 /* int */;
enum { kPgRunning = 0, kPgConverged = 1, kPgStalled = 2, kPgDegenerate = 3, kPgNonfinite = 4 };
// the workspace's regions (8-byte words), tohip_posegraph_layout's order
enum { kPgOffS = 0, kPgOffPose, kPgOffX, kPgOffEdge, kPgOffNode, kPgOffLdl, kPgOffR, kPgOffZ, kPgOffP, kPgOffAp, kPgOffCostPart, kPgOffRzPart,
       kPgOffPapPart, kPgOffSmallPart, kPgOffDegPart, kPgOffTrialCost, kPgOffTotal, kPgRegions };
static_assert(kPgRegions == TOHIP_POSEGRAPH_REGIONS, "the header's count");

struct PgLayout {
    long long off[kPgRegions];
};

inline PgLayout pg_layout(long long n, long long e) {
    const long long nbn = (n + TO_BLOCK - 1) / TO_BLOCK, nbe = (e + TO_BLOCK - 1) / TO_BLOCK;
    const long long size[kPgRegions - 1] = {3 * kPgS, 8 * n, 6 * n, 2 * e * kPgEdge, 2 * n * kPgNode, 21 * n, 6 * n, 6 * n, 12 * n, 6 * n,
                                            nbe, nbn, nbn, nbn, nbn, 2};   // (the last: the trial cost, and whether the pending step is small)
    PgLayout L;
    long long at = 0;
    for (int i = 0; i < kPgRegions - 1; ++i) {
        L.off[i] = at;
        at += size[i];
    }
    L.off[kPgOffTotal] = at;
    return L;
}

struct PgWork {   // the regions as pointers
    double *S, *pose, *x, *edge, *node, *ldl, *r, *z, *p, *ap, *costpart, *rzpart, *pappart, *trialcost;
    long long *smallpart, *degpart;
};

inline PgWork pg_work(void* work, const PgLayout& L) {
    double* w = reinterpret_cast<double*>(work);
    PgWork W;
    W.S = w + L.off[kPgOffS], W.pose = w + L.off[kPgOffPose], W.x = w + L.off[kPgOffX], W.edge = w + L.off[kPgOffEdge], W.node = w + L.off[kPgOffNode];
    W.ldl = w + L.off[kPgOffLdl], W.r = w + L.off[kPgOffR], W.z = w + L.off[kPgOffZ], W.p = w + L.off[kPgOffP], W.ap = w + L.off[kPgOffAp];
    W.costpart = w + L.off[kPgOffCostPart], W.rzpart = w + L.off[kPgOffRzPart], W.pappart = w + L.off[kPgOffPapPart];
    W.smallpart = reinterpret_cast<long long*>(w + L.off[kPgOffSmallPart]), W.degpart = reinterpret_cast<long long*>(w + L.off[kPgOffDegPart]);
    W.trialcost = w + L.off[kPgOffTrialCost];
    return W;
}

__device__ __forceinline__ long long pg_int(const double* S, int k) { return reinterpret_cast<const long long*>(S)[k]; }
__device__ __forceinline__ void pg_set_int(double* S, int k, long long v) { reinterpret_cast<long long*>(S)[k] = v; }

// the halving tree over the block's 256 values -> the partial, in every thread
__device__ __forceinline__ double pg_tree(double v, double* s) {
    const int t = threadIdx.x;
    __syncthreads();   // (s may still be read from an earlier use)
    s[t] = v;
    __syncthreads();
    for (int m = TO_BLOCK / 2; m >= 1; m >>= 1) {
        if (t < m) s[t] = s[t] + s[t + m];
        __syncthreads();
    }
    return s[0];
}

// the partials from 0.0 in ascending order, by thread 0, -> in every thread
__device__ __forceinline__ double pg_sum(const double* __restrict__ part, long long nb, double* s1) {
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (long long b = 0; b < nb; ++b) v = v + part[b];
        *s1 = v;
    }
    __syncthreads();
    return *s1;
}

__device__ __forceinline__ void pg_qmul(const double* p, const double* q, double* o) {   // the Hamilton product, k_scan_step's order
    o[0] = ((p[0] * q[0] - p[1] * q[1]) - p[2] * q[2]) - p[3] * q[3];
    o[1] = ((p[0] * q[1] + p[1] * q[0]) + p[2] * q[3]) - p[3] * q[2];
    o[2] = ((p[0] * q[2] - p[1] * q[3]) + p[2] * q[0]) + p[3] * q[1];
    o[3] = ((p[0] * q[3] + p[1] * q[2]) - p[2] * q[1]) + p[3] * q[0];
}

// a node's trial pose: t + dt, (1, dr / 2) (x) q
__device__ __forceinline__ void pg_trial(const double* __restrict__ pose, const double* __restrict__ x, long long i, double* t, double* q) {
    const double* P = pose + 8 * i;
    const double* X = x + 6 * i;
    const double h[4] = {1.0, 0.5 * X[3], 0.5 * X[4], 0.5 * X[5]};
    const double q0[4] = {P[3], P[4], P[5], P[6]};
    pg_qmul(h, q0, q);
    t[0] = P[0] + X[0], t[1] = P[1] + X[1], t[2] = P[2] + X[2];
}

__device__ __forceinline__ double pg_dot6(const double* a, int sa, const double* b, int sb) {   // sum_k a[k sa] b[k sb], ascending from the first
    double acc = a[0] * b[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) acc = acc + a[k * sa] * b[k * sb];
    return acc;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_pg_linearize(const int* __restrict__ ab, const double* __restrict__ meas, const double* __restrict__ omega, const int* __restrict__ free_mask,
               long long n_edges, double c2, int robust, const double* __restrict__ S, const double* __restrict__ pose, const double* __restrict__ x,
               double* __restrict__ edge, double* __restrict__ costpart) {
    __shared__ double s_tree[TO_BLOCK];
    if (pg_int(S, kPgStatus) != kPgRunning) return;   // (uniform: frozen)
    const long long k = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    double rho = 0.0;
    if (k < n_edges) {
        const int a = ab[2 * k], b = ab[2 * k + 1];
        double ta[3] = {0.0, 0.0, 0.0}, qa[4] = {1.0, 0.0, 0.0, 0.0}, tb[3], qb[4];   // (a = -1: the world frame)
        if (a >= 0) pg_trial(pose, x, a, ta, qa);
        pg_trial(pose, x, b, tb, qb);
        const double* Z = meas + 7 * k;
        double R[3][3], v[3], e[6];
        {
            const double w = qa[0], qx = qa[1], qy = qa[2], qz = qa[3];
            const double s = 2.0 / (((w * w + qx * qx) + qy * qy) + qz * qz);
            R[0][0] = 1.0 - s * (qy * qy + qz * qz), R[0][1] = s * (qx * qy - w * qz), R[0][2] = s * (qx * qz + w * qy);
            R[1][0] = s * (qx * qy + w * qz), R[1][1] = 1.0 - s * (qx * qx + qz * qz), R[1][2] = s * (qy * qz - w * qx);
            R[2][0] = s * (qx * qz - w * qy), R[2][1] = s * (qy * qz + w * qx), R[2][2] = 1.0 - s * (qx * qx + qy * qy);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = tb[i] - ta[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) e[i] = ((R[0][i] * v[0] + R[1][i] * v[1]) + R[2][i] * v[2]) - Z[i];
        {
            const double ca[4] = {qa[0], -qa[1], -qa[2], -qa[3]}, cz[4] = {Z[3], -Z[4], -Z[5], -Z[6]};
            double dq[4], eps[4];
            pg_qmul(ca, qb, dq);
            pg_qmul(dq, cz, eps);
#pragma unroll
            for (int i = 0; i < 3; ++i) e[3 + i] = (2.0 * eps[1 + i]) / eps[0];
        }
        double Ja[6][6], Jb[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) Ja[i][j] = Jb[i][j] = 0.0;
        {
            const double h[3] = {0.5 * e[3], 0.5 * e[4], 0.5 * e[5]};
            const double G[3][3] = {{1.0 + h[0] * h[0], h[0] * h[1] + h[2], h[0] * h[2] - h[1]},
                                    {h[1] * h[0] - h[2], 1.0 + h[1] * h[1], h[1] * h[2] + h[0]},
                                    {h[2] * h[0] + h[1], h[2] * h[1] - h[0], 1.0 + h[2] * h[2]}};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double gr = (G[i][0] * R[j][0] + G[i][1] * R[j][1]) + G[i][2] * R[j][2];
                    Jb[i][j] = R[j][i], Ja[i][j] = -R[j][i];
                    Jb[3 + i][3 + j] = gr, Ja[3 + i][3 + j] = -gr;
                }
                Ja[i][3] = R[1][i] * v[2] - R[2][i] * v[1];
                Ja[i][4] = R[2][i] * v[0] - R[0][i] * v[2];
                Ja[i][5] = R[0][i] * v[1] - R[1][i] * v[0];
            }
        }
        double Om[6][6];
        {
            const double* O = omega + 21 * k;
            int m = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) Om[i][j] = Om[j][i] = O[m++];
        }
        double u[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) u[i] = pg_dot6(Om[i], 1, e, 1);
        const double s = pg_dot6(e, 1, u, 1);
        double w = 1.0;
        rho = s;
        if (robust) {
            const double f = c2 / (c2 + s);
            w = f * f;
            rho = (c2 * s) / (c2 + s);
        }
        const int ma = a >= 0 ? free_mask[a] : 0, mb = free_mask[b];
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                Ja[r][c] = ((ma >> c) & 1) ? Ja[r][c] : 0.0;
                Jb[r][c] = ((mb >> c) & 1) ? Jb[r][c] : 0.0;
            }
        double Ma[6][6], Mb[6][6], uw[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double Wi[6];   // (W = w Omega, one row at a time)
#pragma unroll
            for (int j = 0; j < 6; ++j) Wi[j] = w * Om[i][j];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                Ma[i][j] = pg_dot6(Wi, 1, &Ja[0][j], 6);
                Mb[i][j] = pg_dot6(Wi, 1, &Jb[0][j], 6);
            }
            uw[i] = pg_dot6(Wi, 1, e, 1);
        }
        const long long sel = pg_int(S, kPgSel);
        double* rec = edge + ((sel ^ 1) * n_edges + k) * kPgEdge;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            rec[i] = e[i];
            rec[kPgGa + i] = pg_dot6(&Ja[0][i], 6, uw, 1);
            rec[kPgGb + i] = pg_dot6(&Jb[0][i], 6, uw, 1);
        }
        rec[kPgRS] = s, rec[kPgRW] = w, rec[kPgRRho] = rho, rec[9] = 0.0;
        int m = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                rec[kPgHaa + m] = pg_dot6(&Ja[0][i], 6, &Ma[0][j], 6);
                rec[kPgHbb + m] = pg_dot6(&Jb[0][i], 6, &Mb[0][j], 6);
                ++m;
            }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) rec[kPgHab + 6 * i + j] = pg_dot6(&Ja[0][i], 6, &Mb[0][j], 6);
    }
    const double part = pg_tree(rho, s_tree);
    if (threadIdx.x == 0) costpart[blockIdx.x] = part;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_pg_gather(const int* __restrict__ row_ptr, const int* __restrict__ incident, const int* __restrict__ free_mask, long long n_nodes, long long n_edges,
            const double* __restrict__ S, const double* __restrict__ edge, double* __restrict__ node, const double* __restrict__ costpart,
            const long long* __restrict__ smallpart, double* __restrict__ trialcost) {
    if (pg_int(S, kPgStatus) != kPgRunning) return;   // (uniform: frozen)
    const long long other = pg_int(S, kPgSel) ^ 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long nbe = (n_edges + TO_BLOCK - 1) / TO_BLOCK;
        double c = 0.0;
        for (long long b = 0; b < nbe; ++b) c = c + costpart[b];
        trialcost[0] = c;
        const long long nbn = (n_nodes + TO_BLOCK - 1) / TO_BLOCK;
        long long small = 1;   // (the flags of the solve before this launch: k_pg_step, which resets them, reads this word instead)
        for (long long b = 0; b < nbn; ++b) small &= smallpart[b];
        pg_set_int(trialcost, 1, small);
    }
    const long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    double acc[kPgNode];
#pragma unroll
    for (int m = 0; m < kPgNode; ++m) acc[m] = 0.0;
    const double* E = edge + other * n_edges * kPgEdge;
    for (int at = row_ptr[i]; at < row_ptr[i + 1]; ++at) {
        const int code = incident[at];
        const double* rec = E + (long long)(code >> 1) * kPgEdge;
        const double* H = rec + ((code & 1) ? kPgHbb : kPgHaa);
        const double* G = rec + ((code & 1) ? kPgGb : kPgGa);
#pragma unroll
        for (int m = 0; m < 21; ++m) acc[m] = acc[m] + H[m];
#pragma unroll
        for (int m = 0; m < 6; ++m) acc[21 + m] = acc[21 + m] + G[m];
    }
    const int mask = free_mask[i];
    double* out = node + (other * n_nodes + i) * kPgNode;
    int m = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) {
            const bool free_rc = ((mask >> r) & 1) && ((mask >> c) & 1);
            out[m] = free_rc ? acc[m] : (r == c ? 1.0 : 0.0);
            ++m;
        }
        out[21 + r] = ((mask >> r) & 1) ? acc[21 + r] : 0.0;
    }
}

// the node's damped block from its D (21) -> A, symmetric
__device__ __forceinline__ void pg_damped(const double* __restrict__ D, double lam, int mask, double A[6][6]) {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = D[m++];
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if ((mask >> i) & 1) A[i][i] = A[i][i] + lam * A[i][i];
}

// z = (L d L^T)^-1 r: reg_solve's substitutions.  ldl: L's strict lower triangle row-major (15), then d (6)
__device__ __forceinline__ void pg_block_solve(const double* __restrict__ ldl, const double* r, double* z) {
    double L[6][6], y[6];
    int m = 0;
#pragma unroll
    for (int i = 1; i < 6; ++i)
#pragma unroll
        for (int k = 0; k < i; ++k) L[i][k] = ldl[m++];
    const double* d = ldl + 15;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * z[k];
        z[i] = v;
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_pg_step(const int* __restrict__ free_mask, long long n_nodes, double tol_t, double tol_r, const double* __restrict__ S_in, double* __restrict__ S_out,
          const double* __restrict__ trialcost, double* __restrict__ pose, double* __restrict__ x, const double* __restrict__ node,
          double* __restrict__ ldl, double* __restrict__ r_, double* __restrict__ z_, double* __restrict__ p0, double* __restrict__ rzpart,
          long long* __restrict__ smallpart, long long* __restrict__ degpart) {
    __shared__ double s_tree[TO_BLOCK];
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    double lam = S_in[kPgLam], cost_cur = S_in[kPgCost], cost0 = S_in[kPgCost0];
    long long status = pg_int(S_in, kPgStatus), iter = pg_int(S_in, kPgIter), accepted = pg_int(S_in, kPgAccepted), sel = pg_int(S_in, kPgSel),
              have = pg_int(S_in, kPgHave);
    bool accept = false, solve = false;
    if (status == kPgRunning) {
        const bool small = pg_int(trialcost, 1) != 0;   // (reduced by k_pg_gather: smallpart itself is only WRITTEN here)
        const double cost = trialcost[0];
        const bool first = iter == 0;
        iter += 1;
        if (!(cost < __builtin_inf())) {
            status = kPgNonfinite;
        } else if (first || cost < cost_cur) {
            accept = solve = true;
            cost_cur = cost;
            sel ^= 1;
            have = 1;
            if (first) {
                cost0 = cost;
            } else {
                accepted += 1;
                lam = lam / 8.0;
                lam = lam > 0x1p-30 ? lam : 0x1p-30;
                if (small) {
                    status = kPgConverged;
                    solve = false;
                }
            }
        } else {
            lam = lam * 8.0;
            solve = true;
            if (lam > 0x1p30) {
                status = kPgStalled;
                solve = false;
            }
        }
    }
    if (writer) {
        for (int k = 0; k < kPgS; ++k) S_out[k] = S_in[k];
        S_out[kPgLam] = lam, S_out[kPgCost] = cost_cur, S_out[kPgCost0] = cost0;
        pg_set_int(S_out, kPgStatus, status), pg_set_int(S_out, kPgIter, iter), pg_set_int(S_out, kPgAccepted, accepted), pg_set_int(S_out, kPgSel, sel);
        pg_set_int(S_out, kPgHave, have), pg_set_int(S_out, kPgCgStop, 0);
    }
    if (!accept && !solve) return;   // (uniform)
    const long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    double rz = 0.0;
    bool bad = false;
    if (i < n_nodes) {
        if (accept) {
            double t[3], q[4];
            pg_trial(pose, x, i, t, q);
            double* P = pose + 8 * i;
            P[0] = t[0], P[1] = t[1], P[2] = t[2], P[3] = q[0], P[4] = q[1], P[5] = q[2], P[6] = q[3];
        }
        if (solve) {
            const int mask = free_mask[i];
            const double* D = node + (sel * n_nodes + i) * kPgNode;
            double A[6][6], L[6][6], d[6];
            pg_damped(D, lam, mask, A);
#pragma unroll
            for (int k = 0; k < 6; ++k) x[6 * i + k] = 0.0, p0[6 * i + k] = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double v = A[j][j];
#pragma unroll
                for (int k = 0; k < j; ++k) v = v - L[j][k] * (L[j][k] * d[k]);
                bad = bad || !(v > 0.0) || !(v < __builtin_inf());
                d[j] = v;
#pragma unroll
                for (int ii = j + 1; ii < 6; ++ii) {
                    double u = A[ii][j];
#pragma unroll
                    for (int k = 0; k < j; ++k) u = u - L[ii][k] * (L[j][k] * d[k]);
                    L[ii][j] = u / v;
                }
            }
            double* F = ldl + 21 * i;
            int m = 0;
#pragma unroll
            for (int ii = 1; ii < 6; ++ii)
#pragma unroll
                for (int k = 0; k < ii; ++k) F[m++] = L[ii][k];
#pragma unroll
            for (int k = 0; k < 6; ++k) F[15 + k] = d[k];
            double r[6], z[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) r[k] = 0.0 - D[21 + k];
            pg_block_solve(F, r, z);
#pragma unroll
            for (int k = 0; k < 6; ++k) r_[6 * i + k] = r[k], z_[6 * i + k] = z[k];
            rz = pg_dot6(r, 1, z, 1);
        }
    }
    if (!solve) return;   // (uniform)
    const double part = pg_tree(rz, s_tree);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) {
        rzpart[blockIdx.x] = part;
        smallpart[blockIdx.x] = 1;
        degpart[blockIdx.x] = any_bad ? 1 : 0;
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_pg_spmv(const int* __restrict__ ab, const int* __restrict__ row_ptr, const int* __restrict__ incident, const int* __restrict__ free_mask,
          long long n_nodes, long long n_edges, int first, double tol2, const double* __restrict__ S_in, double* __restrict__ S_out,
          const double* __restrict__ edge, const double* __restrict__ node, const double* __restrict__ z_, const double* __restrict__ p_in,
          double* __restrict__ p_out, double* __restrict__ ap, const double* __restrict__ rzpart, double* __restrict__ pappart,
          const long long* __restrict__ degpart) {
    __shared__ double s_tree[TO_BLOCK];
    __shared__ double s_one;
    __shared__ long long s_deg;
    const long long nbn = (n_nodes + TO_BLOCK - 1) / TO_BLOCK;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    long long status = pg_int(S_in, kPgStatus), stop = pg_int(S_in, kPgCgStop);
    double rz_prev = S_in[kPgRz], rz0 = S_in[kPgRz0], beta = 0.0;
    bool run = status == kPgRunning && !stop;
    if (run && first) {
        if (threadIdx.x == 0) {
            long long deg = 0;
            for (long long b = 0; b < nbn; ++b) deg |= degpart[b];
            s_deg = deg;
        }
        __syncthreads();
        if (s_deg) {
            status = kPgDegenerate;
            run = false;
        }
    }
    if (run) {
        const double rz = pg_sum(rzpart, nbn, &s_one);
        if (first)
            rz0 = rz;
        else
            beta = rz / rz_prev;
        if (rz <= tol2 * rz0) {
            stop = 1;
            run = false;
        } else {
            rz_prev = rz;
        }
    }
    if (writer) {
        for (int k = 0; k < kPgS; ++k) S_out[k] = S_in[k];
        S_out[kPgRz] = rz_prev, S_out[kPgRz0] = rz0;
        pg_set_int(S_out, kPgStatus, status), pg_set_int(S_out, kPgCgStop, stop);
    }
    if (!run) return;   // (uniform)
    const long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    double pap = 0.0;
    if (i < n_nodes) {
        const long long sel = pg_int(S_in, kPgSel);
        const double lam = S_in[kPgLam];
        double p[6], y[6], A[6][6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            p[k] = z_[6 * i + k] + beta * p_in[6 * i + k];
            p_out[6 * i + k] = p[k];
        }
        pg_damped(node + (sel * n_nodes + i) * kPgNode, lam, free_mask[i], A);
#pragma unroll
        for (int r = 0; r < 6; ++r) y[r] = pg_dot6(A[r], 1, p, 1);
        const double* E = edge + sel * n_edges * kPgEdge;
        for (int at = row_ptr[i]; at < row_ptr[i + 1]; ++at) {
            const int code = incident[at], k = code >> 1, side = code & 1;
            const int a = ab[2 * k];
            if (a < 0) continue;   // (an absolute edge has no off-diagonal block)
            const long long j = side ? a : ab[2 * k + 1];
            double po[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) po[c] = z_[6 * j + c] + beta * p_in[6 * j + c];
            const double* B = E + (long long)k * kPgEdge + kPgHab;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double term = side ? pg_dot6(B + r, 6, po, 1) : pg_dot6(B + 6 * r, 1, po, 1);
                y[r] = y[r] + term;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) ap[6 * i + k] = y[k];
        pap = pg_dot6(p, 1, y, 1);
    }
    const double part = pg_tree(pap, s_tree);
    if (threadIdx.x == 0) pappart[blockIdx.x] = part;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_pg_update(long long n_nodes, double tol_t, double tol_r, const double* __restrict__ S_in, double* __restrict__ S_out, const double* __restrict__ ldl,
            const double* __restrict__ p, const double* __restrict__ ap, double* __restrict__ x, double* __restrict__ r_, double* __restrict__ z_,
            const double* __restrict__ pappart, double* __restrict__ rzpart, long long* __restrict__ smallpart) {
    __shared__ double s_tree[TO_BLOCK];
    __shared__ double s_one;
    const long long nbn = (n_nodes + TO_BLOCK - 1) / TO_BLOCK;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    long long stop = pg_int(S_in, kPgCgStop), total = pg_int(S_in, kPgCgTotal);
    bool run = pg_int(S_in, kPgStatus) == kPgRunning && !stop;
    double alpha = 0.0;
    if (run) {
        const double pap = pg_sum(pappart, nbn, &s_one);
        if (!(pap > 0.0)) {
            stop = 1;
            run = false;
        } else {
            alpha = S_in[kPgRz] / pap;
            total += 1;
        }
    }
    if (writer) {
        for (int k = 0; k < kPgS; ++k) S_out[k] = S_in[k];
        pg_set_int(S_out, kPgCgStop, stop), pg_set_int(S_out, kPgCgTotal, total);
    }
    if (!run) return;   // (uniform)
    const long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    double rz = 0.0;
    bool big = false;
    if (i < n_nodes) {
        double r[6], z[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double xv = x[6 * i + k] + alpha * p[6 * i + k], tol = k < 3 ? tol_t : tol_r;
            x[6 * i + k] = xv;
            big = big || !(xv <= tol && -xv <= tol);
            r[k] = r_[6 * i + k] - alpha * ap[6 * i + k];
        }
        pg_block_solve(ldl + 21 * i, r, z);
#pragma unroll
        for (int k = 0; k < 6; ++k) r_[6 * i + k] = r[k], z_[6 * i + k] = z[k];
        rz = pg_dot6(r, 1, z, 1);
    }
    const double part = pg_tree(rz, s_tree);
    const int any_big = __syncthreads_or(big ? 1 : 0);
    if (threadIdx.x == 0) {
        rzpart[blockIdx.x] = part;
        smallpart[blockIdx.x] = any_big ? 0 : 1;
    }
}

__global__ void __launch_bounds__(TO_BLOCK)
k_pg_start(const double* __restrict__ nodes, long long n_nodes, double* __restrict__ S, double* __restrict__ pose, double* __restrict__ x,
           long long* __restrict__ smallpart) {
    const long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    if (i == 0) {
        for (int k = 0; k < 3 * kPgS; ++k) S[k] = 0.0;
        S[kPgS + kPgLam] = 0x1p-10;   // (HOME is copy 1)
    }
    if (threadIdx.x == 0) smallpart[blockIdx.x] = 1;
    if (i >= n_nodes) return;
#pragma unroll
    for (int k = 0; k < 7; ++k) pose[8 * i + k] = nodes[7 * i + k];
    pose[8 * i + 7] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) x[6 * i + k] = 0.0;
}

__global__ void __launch_bounds__(TO_BLOCK)
k_pg_result(long long n_nodes, long long n_edges, const double* __restrict__ S, const double* __restrict__ pose, const double* __restrict__ edge,
            double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * TO_BLOCK + threadIdx.x;
    if (i < kPgS) out[i] = S[i];
    if (i < n_nodes) {
#pragma unroll
        for (int k = 0; k < 7; ++k) out[kPgS + 7 * i + k] = pose[8 * i + k];
    }
    if (i < n_edges) {
        const bool have = pg_int(S, kPgHave) != 0;
        const double* rec = edge + (pg_int(S, kPgSel) * n_edges + i) * kPgEdge;
        out[kPgS + 7 * n_nodes + i] = have ? rec[kPgRS] : 0.0;
        out[kPgS + 7 * n_nodes + n_edges + i] = have ? rec[kPgRW] : 0.0;
    }
}

struct PgGraph {   // the checked arguments of one graph
    const int *ab, *row_ptr, *incident, *free_mask;
    const double *meas, *omega;
    long long n, e, n_incident;
};

// two byte ranges share a byte
inline bool pg_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// sizes, nulls, alignment, the workspace's size, and that the workspace (the output) shares no byte with an input
inline int pg_check(PgGraph& G, const int32_t* ab, const double* meas, const double* omega, const int32_t* row_ptr, const int32_t* incident,
                    const int32_t* free_mask, int64_t n, int64_t e, int64_t n_incident, const void* work, size_t work_bytes, uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    if (n < 1 || n > kPgMax || e < 1 || e > kPgMax || n_incident < e || n_incident > 2 * e) return TOHIP_EINVAL;
    if (!ab || !meas || !omega || !row_ptr || !incident || !free_mask || !work) return TOHIP_EINVAL;
    if (!scan_aligned(ab, 4) || !scan_aligned(row_ptr, 4) || !scan_aligned(incident, 4) || !scan_aligned(free_mask, 4) || !scan_aligned(meas, 8) ||
        !scan_aligned(omega, 8) || !scan_aligned(work, 8))
        return TOHIP_EINVAL;
    if (work_bytes < (size_t)pg_layout(n, e).off[kPgOffTotal] * 8) return TOHIP_ENOSPC;
    const void* ins[6] = {ab, meas, omega, row_ptr, incident, free_mask};
    const size_t size[6] = {(size_t)e * 8, (size_t)e * 56, (size_t)e * 168, (size_t)(n + 1) * 4, (size_t)n_incident * 4, (size_t)n * 4};
    for (int i = 0; i < 6; ++i)
        if (pg_overlap(ins[i], size[i], work, work_bytes)) return TOHIP_EINVAL;
    G.ab = ab, G.meas = meas, G.omega = omega, G.row_ptr = row_ptr, G.incident = incident, G.free_mask = free_mask;
    G.n = n, G.e = e, G.n_incident = n_incident;
    return TOHIP_OK;
}

inline bool pg_tol_ok(double v) { return v >= 0.0 && std::isfinite(v); }

inline int pg_enqueue_linearize(const PgGraph& G, const PgWork& W, double c2, int robust, hipStream_t st) {
    k_pg_linearize<<<(unsigned)((G.e + TO_BLOCK - 1) / TO_BLOCK), TO_BLOCK, 0, st>>>(G.ab, G.meas, G.omega, G.free_mask, G.e, c2, robust, W.S + kPgS,
                                                                                      W.pose, W.x, W.edge, W.costpart);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

inline int pg_enqueue_gather(const PgGraph& G, const PgWork& W, hipStream_t st) {
    k_pg_gather<<<(unsigned)((G.n + TO_BLOCK - 1) / TO_BLOCK), TO_BLOCK, 0, st>>>(G.row_ptr, G.incident, G.free_mask, G.n, G.e, W.S + kPgS, W.edge, W.node,
                                                                                   W.costpart, W.smallpart, W.trialcost);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

inline int pg_enqueue_step(const PgGraph& G, const PgWork& W, int64_t cg_iterations, double tol2, double tol_t, double tol_r, hipStream_t st) {
    const unsigned grid = (unsigned)((G.n + TO_BLOCK - 1) / TO_BLOCK);
    double *S0 = W.S, *S1 = W.S + kPgS, *S2 = W.S + 2 * kPgS;
    k_pg_step<<<grid, TO_BLOCK, 0, st>>>(G.free_mask, G.n, tol_t, tol_r, S1, S2, W.trialcost, W.pose, W.x, W.node, W.ldl, W.r, W.z, W.p, W.rzpart,
                                         W.smallpart, W.degpart);
    TO_HIP_CHECK_LAUNCH();
    for (int64_t k = 0; k < cg_iterations; ++k) {
        double *p_in = W.p + (k & 1) * 6 * G.n, *p_out = W.p + ((k + 1) & 1) * 6 * G.n;
        k_pg_spmv<<<grid, TO_BLOCK, 0, st>>>(G.ab, G.row_ptr, G.incident, G.free_mask, G.n, G.e, k == 0 ? 1 : 0, tol2, k == 0 ? S2 : S1, S0, W.edge, W.node,
                                             W.z, p_in, p_out, W.ap, W.rzpart, W.pappart, W.degpart);
        TO_HIP_CHECK_LAUNCH();
        k_pg_update<<<grid, TO_BLOCK, 0, st>>>(G.n, tol_t, tol_r, S0, S1, W.ldl, p_out, W.ap, W.x, W.r, W.z, W.pappart, W.rzpart, W.smallpart);
        TO_HIP_CHECK_LAUNCH();
    }
    return TOHIP_OK;
}

}  // namespace

extern "C" size_t tohip_posegraph_workspace_bytes(int64_t n_nodes, int64_t n_edges, uint32_t flags) {
    if (flags != 0u || n_nodes < 1 || n_nodes > kPgMax || n_edges < 1 || n_edges > kPgMax) return 0;
    return (size_t)pg_layout(n_nodes, n_edges).off[kPgOffTotal] * 8;
}

extern "C" int tohip_posegraph_layout(int64_t n_nodes, int64_t n_edges, int64_t* offsets_host, uint32_t flags) {
    if (flags != 0u || n_nodes < 1 || n_nodes > kPgMax || n_edges < 1 || n_edges > kPgMax || !offsets_host) return TOHIP_EINVAL;
    const PgLayout L = pg_layout(n_nodes, n_edges);
    for (int i = 0; i < kPgRegions; ++i) offsets_host[i] = L.off[i];
    return TOHIP_OK;
}

extern "C" int tohip_posegraph_start(const double* nodes, int64_t n_nodes, int64_t n_edges, void* workspace, size_t workspace_bytes, void* stream_,
                                     uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    if (n_nodes < 1 || n_nodes > kPgMax || n_edges < 1 || n_edges > kPgMax || !nodes || !workspace || !scan_aligned(nodes, 8) ||
        !scan_aligned(workspace, 8))
        return TOHIP_EINVAL;
    const PgLayout L = pg_layout(n_nodes, n_edges);
    if (workspace_bytes < (size_t)L.off[kPgOffTotal] * 8) return TOHIP_ENOSPC;
    if (pg_overlap(nodes, (size_t)n_nodes * 56, workspace, workspace_bytes)) return TOHIP_EINVAL;
    const PgWork W = pg_work(workspace, L);
    k_pg_start<<<(unsigned)((n_nodes + TO_BLOCK - 1) / TO_BLOCK), TO_BLOCK, 0, (hipStream_t)stream_>>>(nodes, n_nodes, W.S, W.pose, W.x, W.smallpart);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}

extern "C" int tohip_posegraph_linearize(const int32_t* ab, const double* meas, const double* omega, const int32_t* row_ptr, const int32_t* incident,
                                         const int32_t* free_mask, int64_t n_nodes, int64_t n_edges, int64_t n_incident, double robust_c,
                                         void* workspace, size_t workspace_bytes, void* stream_, uint32_t flags) {
    PgGraph G;
    const int rc = pg_check(G, ab, meas, omega, row_ptr, incident, free_mask, n_nodes, n_edges, n_incident, workspace, workspace_bytes, flags);
    if (rc != TOHIP_OK) return rc;
    if (!pg_tol_ok(robust_c)) return TOHIP_EINVAL;
    const PgWork W = pg_work(workspace, pg_layout(n_nodes, n_edges));
    return pg_enqueue_linearize(G, W, robust_c * robust_c, robust_c > 0.0 ? 1 : 0, (hipStream_t)stream_);
}

extern "C" int tohip_posegraph_gather(const int32_t* ab, const double* meas, const double* omega, const int32_t* row_ptr, const int32_t* incident,
                                      const int32_t* free_mask, int64_t n_nodes, int64_t n_edges, int64_t n_incident, void* workspace,
                                      size_t workspace_bytes, void* stream_, uint32_t flags) {
    PgGraph G;
    const int rc = pg_check(G, ab, meas, omega, row_ptr, incident, free_mask, n_nodes, n_edges, n_incident, workspace, workspace_bytes, flags);
    if (rc != TOHIP_OK) return rc;
    return pg_enqueue_gather(G, pg_work(workspace, pg_layout(n_nodes, n_edges)), (hipStream_t)stream_);
}

extern "C" int tohip_posegraph_step(const int32_t* ab, const double* meas, const double* omega, const int32_t* row_ptr, const int32_t* incident,
                                    const int32_t* free_mask, int64_t n_nodes, int64_t n_edges, int64_t n_incident, int64_t cg_iterations,
                                    double cg_tol, double tol_t, double tol_r, void* workspace, size_t workspace_bytes, void* stream_, uint32_t flags) {
    PgGraph G;
    const int rc = pg_check(G, ab, meas, omega, row_ptr, incident, free_mask, n_nodes, n_edges, n_incident, workspace, workspace_bytes, flags);
    if (rc != TOHIP_OK) return rc;
    if (cg_iterations < 1 || cg_iterations > TOHIP_POSEGRAPH_MAX_CG || !pg_tol_ok(cg_tol) || !pg_tol_ok(tol_t) || !pg_tol_ok(tol_r)) return TOHIP_EINVAL;
    return pg_enqueue_step(G, pg_work(workspace, pg_layout(n_nodes, n_edges)), cg_iterations, cg_tol * cg_tol, tol_t, tol_r, (hipStream_t)stream_);
}

extern "C" int tohip_posegraph_optimize(const int32_t* ab, const double* meas, const double* omega, const int32_t* row_ptr, const int32_t* incident,
                                        const int32_t* free_mask, int64_t n_nodes, int64_t n_edges, int64_t n_incident, int64_t iterations,
                                        int64_t cg_iterations, double cg_tol, double robust_c, double tol_t, double tol_r, void* workspace,
                                        size_t workspace_bytes, void* stream_, uint32_t flags) {
    PgGraph G;
    int rc = pg_check(G, ab, meas, omega, row_ptr, incident, free_mask, n_nodes, n_edges, n_incident, workspace, workspace_bytes, flags);
    if (rc != TOHIP_OK) return rc;
    if (iterations < 1 || iterations > TOHIP_POSEGRAPH_MAX_ITERATIONS || cg_iterations < 1 || cg_iterations > TOHIP_POSEGRAPH_MAX_CG || !pg_tol_ok(cg_tol) ||
        !pg_tol_ok(robust_c) || !pg_tol_ok(tol_t) || !pg_tol_ok(tol_r))
        return TOHIP_EINVAL;
    const PgWork W = pg_work(workspace, pg_layout(n_nodes, n_edges));
    hipStream_t st = (hipStream_t)stream_;
    for (int64_t it = 0; it < iterations; ++it) {
        if ((rc = pg_enqueue_linearize(G, W, robust_c * robust_c, robust_c > 0.0 ? 1 : 0, st)) != TOHIP_OK) return rc;
        if ((rc = pg_enqueue_gather(G, W, st)) != TOHIP_OK) return rc;
        if ((rc = pg_enqueue_step(G, W, cg_iterations, cg_tol * cg_tol, tol_t, tol_r, st)) != TOHIP_OK) return rc;
    }
    return TOHIP_OK;
}

extern "C" int tohip_posegraph_result(int64_t n_nodes, int64_t n_edges, const void* workspace, size_t workspace_bytes, double* out, void* stream_,
                                      uint32_t flags) {
    if (flags != 0u) return TOHIP_EINVAL;   // (reserved)
    if (n_nodes < 1 || n_nodes > kPgMax || n_edges < 1 || n_edges > kPgMax || !workspace || !out || !scan_aligned(workspace, 8) || !scan_aligned(out, 8))
        return TOHIP_EINVAL;
    const PgLayout L = pg_layout(n_nodes, n_edges);
    if (workspace_bytes < (size_t)L.off[kPgOffTotal] * 8) return TOHIP_ENOSPC;
    if (pg_overlap(out, (size_t)(kPgS + 7 * n_nodes + 2 * n_edges) * 8, workspace, workspace_bytes)) return TOHIP_EINVAL;
    const PgWork W = pg_work(const_cast<void*>(workspace), L);
    const long long m = std::max<long long>(std::max<long long>(n_nodes, n_edges), kPgS);
    k_pg_result<<<(unsigned)((m + TO_BLOCK - 1) / TO_BLOCK), TO_BLOCK, 0, (hipStream_t)stream_>>>(n_nodes, n_edges, W.S + kPgS, W.pose, W.edge, out);
    TO_HIP_CHECK_LAUNCH();
    return TOHIP_OK;
}
