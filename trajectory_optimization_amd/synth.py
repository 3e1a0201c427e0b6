"""Seeded synthetic inputs for the BASELINE.json configurations.

One definition shared by the golden-fixture generator, the parity tests and
bench.py so that every leg sees bit-identical inputs.  numpy's PCG64 stream is
stable across numpy versions, so the inputs do not depend on the torch build.

Shapes follow the reference's input contract: cloud (N,3) f32 as produced by
its PointCloud2 ingest (/root/reference/src/trajectory_optimization.py:62-63),
waypoint positions (W,3) f32 and wxyz quaternions (W,4) f32
(/root/reference/src/trajectory_optimization.py:66-80), intrinsics as returned
by load_intrinsics (/root/reference/src/tools.py:320-325).
"""
import math

import numpy as np

# /root/reference/src/tools.py:320-325
IMG_WIDTH = 1232.0
IMG_HEIGHT = 1616.0
K_INTRINS = np.array([[758.03967, 0.0, 621.46572],
                      [0.0, 761.62359, 756.86402],
                      [0.0, 0.0, 1.0]], dtype=np.float32)

# body -> optical frame (camera +Z along body +X, +X to the right, +Y down), wxyz
Q_OPTICAL = np.array([0.5, -0.5, 0.5, -0.5], dtype=np.float64)


def quat_mul(a, b):
    """Hamilton product, wxyz, broadcasting over leading dims (float64)."""
    aw, ax, ay, az = np.moveaxis(np.asarray(a, dtype=np.float64), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b, dtype=np.float64), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def make_cloud(n_points, seed=0, extent=(40.0, 40.0, 4.0)):
    """Uniform slab `rand(N,3)*extent - extent/2` metres, f32."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(extent, dtype=np.float64)
    pts = rng.random((n_points, 3)) * ext - ext / 2.0
    return pts.astype(np.float32)


def make_path(n_wps, optical=True, jitter_seed=None, scale=1.0):
    """Smooth curve t=scale*(-10+20s, 3 sin 6s, 0), yaw 0.5 cos 6s, wxyz quats.

    With `optical` the yaw rotation is composed with the body->optical
    rotation so the camera +Z axis looks along the path.  `jitter_seed`
    adds a small random roll/pitch and a non-unit scale to the quaternions
    (exercises the F.normalize step of to_camera_frame).
    """
    if n_wps == 1:
        s = np.zeros(1)
    else:
        s = np.arange(n_wps, dtype=np.float64) / (n_wps - 1)
    pos = scale * np.stack([-10.0 + 20.0 * s, 3.0 * np.sin(6.0 * s), np.zeros_like(s)], axis=1)
    yaw = 0.5 * np.cos(6.0 * s)
    q = np.stack([np.cos(yaw / 2), np.zeros_like(s), np.zeros_like(s), np.sin(yaw / 2)], axis=1)
    if optical:
        q = quat_mul(q, Q_OPTICAL[None, :])
    if jitter_seed is not None:
        rng = np.random.default_rng(jitter_seed)
        dq = np.concatenate([np.ones((n_wps, 1)), 0.05 * rng.standard_normal((n_wps, 3))], axis=1)
        q = quat_mul(q, dq) * (0.5 + rng.random((n_wps, 1)))
    return pos.astype(np.float32), q.astype(np.float32)


def candidate_grid(xs, ys, z, n_headings):
    """Candidate views for a view selection: positions xs x ys at height z, n_headings headings 2 pi j / n_headings + 0.1 at each;
    quaternion r_z(heading) (x) Q_OPTICAL (the camera looks along the heading); candidate index = (ix * len(ys) + iy) * n_headings + j.
    -> (poses (M,3) f32, wxyz quats (M,4) f32)."""
    poses, quats = [], []
    for x in xs:
        for y in ys:
            for j in range(n_headings):
                a = 2.0 * np.pi * j / n_headings + 0.1
                poses.append([x, y, z])
                quats.append(quat_mul(np.array([np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)]), Q_OPTICAL))
    return np.asarray(poses, dtype=np.float32), np.asarray(quats, dtype=np.float32)


def bundled_candidate_grid(points, path, g=6, n_headings=4):
    """The candidate grid over a scanned cloud: x in linspace(min_x + 3, max_x - 3, g), y likewise, z = the mean z of `path`."""
    lo, hi = points.min(axis=0).astype(np.float64), points.max(axis=0).astype(np.float64)
    return candidate_grid(np.linspace(lo[0] + 3, hi[0] - 3, g), np.linspace(lo[1] + 3, hi[1] - 3, g),
                          float(np.asarray(path)[:, 2].astype(np.float64).mean()), n_headings)


def camera_rig(n_cams=5):
    """Fixed extrinsics of a multi-camera rig: yaw offsets 0, +-72, +-144 deg
    about the body z axis, shared K (BASELINE.json config 5). Returns wxyz
    quaternions (C,4) f32 rotating rig->body and zero lever arms (C,3)."""
    offs = np.deg2rad(np.array([0.0, 72.0, -72.0, 144.0, -144.0][:n_cams]))
    q = np.stack([np.cos(offs / 2), np.zeros_like(offs), np.zeros_like(offs), np.sin(offs / 2)], axis=1)
    return q.astype(np.float32), np.zeros((n_cams, 3), dtype=np.float32)


def with_duplicate_rows(base, dup, seed):
    """`base` (n,3) plus copies of its rows `dup` (and of dup[:len(dup)//6] once more), all rows then shuffled (PCG64(seed)): a cloud
    with exact duplicate rows whose copies sit before and after their originals.  -> (points, source row of each point)."""
    src = np.concatenate([np.arange(len(base)), np.asarray(dup), np.asarray(dup)[:len(dup) // 6]])
    order = np.random.default_rng(seed).permutation(len(src))
    src = src[order]
    return base[src].astype(np.float32), src


# ---- tools.plan_tour restated in numpy: what tour_kernels.hip must give, element for element ------------------------
TOUR_INF = 1 << 62
TOUR_MAX_LEN = 1 << 40


def tour_edge_lengths(P):
    """w (n,n) int64: llrint(|P_i - P_j| 2^20) in f64, the differences taken lower index minus higher; -1 where an end is not finite
    or the length exceeds 2^40."""
    P = np.asarray(P, dtype=np.float32)
    n = len(P)
    lo, hi = np.minimum.outer(np.arange(n), np.arange(n)), np.maximum.outer(np.arange(n), np.arange(n))
    fin = np.isfinite(P).all(axis=1)
    Pd = np.where(fin[:, None], P, 0).astype(np.float64)
    d = Pd[lo] - Pd[hi]
    L = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * 1048576.0
    w = np.rint(np.minimum(L, float(1 << 42))).astype(np.int64)
    w[(w > TOUR_MAX_LEN) | ~fin[lo] | ~fin[hi]] = -1
    return w


def tour_two_opt_changes(D, t, closed):
    """(m,m) int64: entry (i, j), 1 <= i < j <= m - 1, is what reversing t[i..j] adds to the length; 0 elsewhere."""
    m = len(t)
    out = np.zeros((m, m), dtype=np.int64)
    if m < 3:
        return out
    t = np.asarray(t)
    tn = np.append(t, t[0])
    i, j = np.triu_indices(m, 1)
    keep = i >= 1
    i, j = i[keep], j[keep]
    has_next = np.full(len(i), True) if closed else j + 1 < m
    d = D[tn[i - 1], tn[j]] - D[tn[i - 1], tn[i]]
    d = d + np.where(has_next, D[tn[i], tn[j + 1]] - D[tn[j], tn[j + 1]], 0)
    out[i, j] = d
    return out


def tour_plan(P, blocked=None, closed=False, max_moves=None, via_D=None):
    """The whole definition: P (n,3) f32 nodes (node 0 the start), blocked (n,n) bool or None (the pairs whose segment query found a
    point; symmetric) -> dict(order, m, unreachable, length_fixed, nn_length_fixed, moves, converged, D, nxt, w, walk).  Floyd-Warshall
    is vectorised per k and 2-opt per move, all in int64.  via_D (n or more rows, n or more columns, int64; None: no roadmap): the
    roadmap's route lengths between the tour nodes — the initial leg is min(direct, via) and the result gains via_flag (n,n) bool,
    True where via < direct strictly."""
    P = np.asarray(P, dtype=np.float32)
    n = len(P)
    max_moves = 4 * n if max_moves is None else int(max_moves)
    w = tour_edge_lengths(P)
    opened = w >= 0
    if blocked is not None:
        opened &= ~np.asarray(blocked, dtype=bool)
    np.fill_diagonal(opened, False)
    D = np.where(opened, w, TOUR_INF).astype(np.int64)
    via_flag = None
    if via_D is not None:
        via = np.asarray(via_D, dtype=np.int64)[:n, :n]
        via_flag = via < D
        np.fill_diagonal(via_flag, False)
        D = np.where(via_flag, via, D)
        opened = D < TOUR_INF
        np.fill_diagonal(opened, False)
    np.fill_diagonal(D, 0)
    nxt = np.where(opened, np.arange(n)[None, :], -1).astype(np.int32)
    for k in range(n):
        a, b = D[:, k:k + 1], D[k:k + 1, :]
        s = a + b   # (below 2^63: both terms are at most 2^62)
        better = (a < TOUR_INF) & (b < TOUR_INF) & (s < D)
        D = np.where(better, s, D)
        nxt = np.where(better, nxt[:, k:k + 1], nxt)
    reach = D[0] < TOUR_INF
    m = int(reach.sum())
    t, left = [0], reach.copy()
    left[0] = False
    nn = 0
    while len(t) < m:
        row = np.where(left, D[t[-1]], np.iinfo(np.int64).max)
        j = int(np.argmin(row))   # the first minimum: ties to the lowest j
        nn += int(row[j])
        t.append(j)
        left[j] = False
    if closed and m > 1:
        nn += int(D[t[-1], 0])
    length, moves = nn, 0
    while True:
        ch = tour_two_opt_changes(D, t, closed)
        best = int(ch.min())
        if best >= 0:
            converged = True
            break
        if moves >= max_moves:
            converged = False
            break
        i, j = np.unravel_index(int(np.argmin(ch)), ch.shape)   # row-major first minimum: lowest i, then lowest j
        t[i:j + 1] = t[i:j + 1][::-1]
        length += best
        moves += 1
    order = np.full(n, -1, dtype=np.int32)
    order[:m] = t
    out = dict(order=order, m=m, unreachable=~reach, length_fixed=length, nn_length_fixed=nn, moves=moves, converged=converged, D=D,
               nxt=nxt, w=w, walk=tour_walk(t, nxt, closed))
    if via_flag is not None:
        out["via_flag"] = via_flag
    return out


def tour_walk(order, nxt, closed):
    """The order with the pass-through nodes inserted: u, nxt[u][v], ..., v for consecutive u, v (and back to node 0 when closed)."""
    stops = [int(v) for v in order] + ([int(order[0])] if closed and len(order) > 1 else [])
    walk = [stops[0]]
    for v in stops[1:]:
        u = walk[-1]
        while u != v:
            u = int(nxt[u][v])
            walk.append(u)
    return walk


# ---- the free-space roadmap restated in numpy: what roadmap_kernels.hip must give, element for element ---------------
ROADMAP_MAX_NODES = 16384
ROADMAP_MAX_K = 32
ROADMAP_MAX_SOURCES = 256


def roadmap_lattice(lo, hi, spacing):
    """Free-space node candidates: the lattice lo + spacing (a, b, c) inside the box [lo, hi] (both ends included up to rounding),
    x the slowest index -> (M,3) f32.  Plain numpy; whether a node or an edge is free is the roadmap's business."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    h = float(spacing)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(h) and h > 0.0 and (hi >= lo).all()):
        raise ValueError(f"roadmap_lattice needs finite lo <= hi and a finite spacing > 0, got {lo}, {hi}, {spacing!r}")
    axes = [lo[a] + h * np.arange(int(np.floor((hi[a] - lo[a]) / h + 1e-9)) + 1) for a in range(3)]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    return g.astype(np.float32)


def roadmap_knn_ref(Q, k, max_edge=None):
    """nbr (M,k) int32, length_fixed (M,k) int64: for each node the k others with the smallest (d2, j), ties to the lower j, ascending
    — d2 in f64 without contraction, the differences taken lower index minus higher; both ends finite; d2 <= (double)(float)max_edge^2
    when max_edge is given; -1 in both arrays where no candidate fills the slot.  length = rint(min(sqrt(d2) 2^20, 2^42))."""
    Q = np.asarray(Q, dtype=np.float32)
    M = len(Q)
    fin = np.isfinite(Q).all(axis=1)
    Qd = np.where(fin[:, None], Q, 0).astype(np.float64)
    idx = np.arange(M)
    lo, hi = np.minimum.outer(idx, idx), np.maximum.outer(idx, idx)
    d = Qd[lo] - Qd[hi]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    ok = fin[:, None] & fin[None, :] & (idx[:, None] != idx[None, :])
    if max_edge is not None:
        ok &= d2 <= np.float64(np.float32(max_edge)) ** 2
    key = np.where(ok, d2, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]   # stable: equal keys keep the ascending j
    got = np.take_along_axis(ok, order, axis=1)
    nbr = np.full((M, k), -1, dtype=np.int32)
    length = np.full((M, k), -1, dtype=np.int64)
    kk = order.shape[1]
    L = np.rint(np.minimum(np.sqrt(np.take_along_axis(d2, order, axis=1)) * 1048576.0, float(1 << 42))).astype(np.int64)
    nbr[:, :kk] = np.where(got, order, -1)
    length[:, :kk] = np.where(got, L, -1)
    return nbr, length


def roadmap_edges(nbr, length, open_):
    """The directed relaxations (u, v, L) of a roadmap: both directions of every open slot (a pair named in both lists appears twice in
    each direction: harmless)."""
    nbr, length = np.asarray(nbr), np.asarray(length, dtype=np.int64)
    M = nbr.shape[0]
    ok = np.asarray(open_).astype(bool) & (nbr >= 0) & (nbr < M) & (length >= 0) & (length <= TOUR_MAX_LEN)
    i, s = np.nonzero(ok)
    j = nbr[i, s].astype(np.int64)
    L = length[i, s]
    return np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([L, L])


def roadmap_routes_ref(nbr, length, open_, sources):
    """D (S,M) int64, pred (S,M) int32 over the undirected graph of the open slots: Bellman-Ford sweeps in int64 until nothing moves
    (the fixed point is the shortest-route table whatever the order), INF = 2^62 where no route exists, D[s][src[s]] = 0; pred[s][v] =
    the lowest u with {u, v} open and D[s][u] + len == D[s][v], -1 for the source and the unreachable."""
    M = np.asarray(nbr).shape[0]
    src = np.asarray(sources, dtype=np.int64).reshape(-1)
    S = len(src)
    u, v, L = roadmap_edges(nbr, length, open_)
    D = np.full((S, M), TOUR_INF, dtype=np.int64)
    D[np.arange(S), src] = 0
    pred = np.full((S, M), -1, dtype=np.int32)
    if len(u) == 0:
        return D, pred
    o = np.argsort(v, kind="stable")
    u, v, L = u[o], v[o], L[o]
    heads, starts = np.unique(v, return_index=True)
    for _ in range(M + 1):
        cand = np.where(D[:, u] < TOUR_INF, D[:, u] + L[None, :], TOUR_INF)
        best = np.minimum.reduceat(cand, starts, axis=1)
        new = np.minimum(D[:, heads], best)
        if (new == D[:, heads]).all():
            break
        D[:, heads] = new
    else:
        raise RuntimeError("roadmap_routes_ref did not converge")
    hit = (D[:, u] < TOUR_INF) & (D[:, u] + L[None, :] == D[:, v]) & (v[None, :] != src[:, None])
    cu = np.where(hit, u[None, :], np.iinfo(np.int64).max)
    lowest = np.minimum.reduceat(cu, starts, axis=1)
    pred[:, heads] = np.where(lowest < M, lowest, -1).astype(np.int32)
    return D, pred


def roadmap_tight_walk(D_row, edges, src, dst):
    """src, ..., dst over tight edges only — (u, v, L) of roadmap_edges with D[u] + L == D[v] — by a depth-first search back from dst
    that takes the lowest u first and enters no node twice: every edge of a shortest route is tight, so it ends at src whenever
    D[dst] is finite, zero-length edges between coincident nodes or not.  None when dst is not reached."""
    src, dst = int(src), int(dst)
    D_row = np.asarray(D_row, dtype=np.int64)
    if D_row[dst] >= TOUR_INF:
        return None
    u, v, L = edges
    tight = (D_row[u] < TOUR_INF) & (D_row[u] + L == D_row[v])
    u, v = u[tight], v[tight]
    o = np.lexsort((u, v))
    u, v = u[o], v[o]
    first, last = np.searchsorted(v, np.arange(len(D_row))), np.searchsorted(v, np.arange(len(D_row)), side="right")
    parent, stack = {dst: None}, [dst]
    while stack:
        x = stack.pop()
        if x == src:
            walk = [src]
            while parent[walk[-1]] is not None:
                walk.append(parent[walk[-1]])
            return walk
        for w in u[first[x]:last[x]][::-1].tolist():   # pushed in descending order: the lowest comes off first
            if w not in parent:
                parent[w] = x
                stack.append(w)
    return None


def roadmap_walk(pred_row, src, dst, tight=None):
    """src, ..., dst along one source's predecessors, or None when dst is not reached.  Coincident nodes are joined by zero-length
    edges, and the lowest-predecessor rule can then point two of them at each other: a chain that comes back to a node it has
    visited is replaced by roadmap_tight_walk over (D_row, edges) = tight() — a route of the same length; without `tight` it
    raises."""
    src, dst = int(src), int(dst)
    walk, seen = [dst], {dst}
    while walk[-1] != src:
        p = int(pred_row[walk[-1]])
        if p < 0:
            return None
        if p in seen:
            if tight is None:
                raise ValueError("the predecessors run in a circle: coincident nodes joined by zero-length edges")
            return roadmap_tight_walk(*tight(), src, dst)
        walk.append(p)
        seen.add(p)
    return walk[::-1]

def roadmap_join(head, via):
    """[head; via] as the planners build it: a via row that coincides with a head row is made non-finite (such a node has no edge,
    and no zero-length edge ties it to its twin) -> (len(head) + len(via), 3) f32."""
    head, via = np.asarray(head, dtype=np.float32).reshape(-1, 3), np.array(via, dtype=np.float32).reshape(-1, 3)
    twin = (via[:, None, :] == head[None, :, :]).all(axis=2).any(axis=1)
    via[twin] = np.nan
    return np.concatenate([head, via])


def doorway_scene():
    """A wall with a doorway and a sealed box: dict(points (N,3) f32: the plane x = 0, y in [-4, 4], z in [0, 3] at 0.05 m spacing
    with a gap at |y| < 0.5, and a closed cubic shell of half side 0.4 m around node 7; radius 0.3; nodes (8,3) f32: the start and
    three views at x ~ -2, three views at x ~ +2 (all at y >= 2: every straight leg across the wall hits it) and a view inside the
    shell; left / right / enclosed: those nodes' indices; lattice (663,3) f32: roadmap_lattice at 0.5 m over the box [-3, 3] x
    [-4, 4] x [0.5, 1.5], which holds nodes inside the gap and no way round the wall's ends)."""
    g = np.arange(-80, 81) * 0.05
    z = np.arange(0, 61) * 0.05
    yy, zz = np.meshgrid(g[np.abs(g) >= 0.5 - 1e-9], z, indexing="ij")
    wall = np.stack([np.zeros(yy.size), yy.ravel(), zz.ravel()], axis=1)
    c = np.array([2.25, -2.25, 1.25])
    t = np.arange(-8, 9) * 0.05
    a, b = [m.ravel() for m in np.meshgrid(t, t, indexing="ij")]
    faces = []
    for axis in range(3):
        for side in (-0.4, 0.4):
            f = np.empty((a.size, 3))
            f[:, axis] = side
            f[:, (axis + 1) % 3] = a
            f[:, (axis + 2) % 3] = b
            faces.append(c + f)
    nodes = np.float32([[-2.0, 3.0, 1.0], [-2.1, 2.2, 1.2], [-2.2, 3.6, 0.8], [-1.9, 2.7, 1.4],
                        [2.1, 2.3, 1.1], [1.9, 3.4, 0.9], [2.2, 2.8, 1.3], [2.25, -2.25, 1.25]])
    return dict(points=np.concatenate([wall] + faces).astype(np.float32), radius=0.3, nodes=nodes, left=[0, 1, 2, 3], right=[4, 5, 6],
                enclosed=7, lattice=roadmap_lattice((-3.0, -4.0, 0.5), (3.0, 4.0, 1.5), 0.5))


# ---- tools.refine_path restated in numpy: what path_kernels.hip must give, element for element ------------------------
PATH_MAX_NODES = 1024
PATH_MAX_ROWS = 4096


def path_chord_lengths(P):
    """w (L,L) int64, read at [i, j] with i < j: rint(min(|P_i - P_j| 2^20, 2^42)) in f64, the differences lower index minus higher
    (the tour's length without its limit: an input leg is open however long it is)."""
    Pd = np.asarray(P, dtype=np.float32).astype(np.float64)
    d = Pd[:, None, :] - Pd[None, :, :]
    L = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * 1048576.0
    return np.rint(np.minimum(L, float(1 << 42))).astype(np.int64)


def path_spacing_fixed(spacing):
    """H: rint((double)(float)spacing 2^20), at least 1 and held at 2^42; 0 for no spacing."""
    if spacing is None or float(np.float32(spacing)) == 0.0:
        return 0
    return max(1, int(np.rint(min(float(np.float32(spacing)) * 1048576.0, float(1 << 42)))))


def _unit_quat(q):
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    return [w / n, x / n, y / n, z / n]


def path_refine_ref(P, keep, open_band, window, spacing, quats=None, max_rows=PATH_MAX_ROWS):
    """The whole definition: P (L,3) f32 in walking order, keep (L,) or None, open_band (L,W), window W, spacing h or None ->
    dict(status, m, R, length_fixed, input_length_fixed, n_open, D, pred, corner, corners, row_node, poses, quats): int64 for the
    search, f64 for rows and quaternions.  With status bit 0 only the header fields are there (m = R = 0); with bit 1 (R > max_rows)
    row_node / poses / quats are None."""
    P = np.asarray(P, dtype=np.float32)
    L, W = len(P), int(window)
    kept = np.zeros(L, dtype=bool) if keep is None else np.asarray(keep).astype(bool).copy()
    kept[0] = kept[-1] = True
    bad = not np.isfinite(P).all()
    if quats is not None:
        quats = np.asarray(quats, dtype=np.float32)
        qk = quats[kept]
        bad = bad or bool((~np.isfinite(qk).all(axis=1) | (qk == 0).all(axis=1)).any())
    if bad:
        return dict(status=1, m=0, R=0, length_fixed=0, input_length_fixed=0, n_open=0)
    w = path_chord_lengths(P)
    band = np.asarray(open_band).reshape(L, W) != 0
    idx = np.arange(L)
    last = np.maximum.accumulate(np.where(kept, idx, -1))   # the largest kept node <= i
    nxt = np.minimum.accumulate(np.where(kept, idx, L)[::-1])[::-1]   # the smallest kept node >= i
    D, pred, n_open = np.zeros(L, dtype=np.int64), np.full(L, -1, dtype=np.int32), 0
    for j in range(1, L):
        i = np.arange(max(j - W, last[j - 1]), j)
        wi = w[i, j]
        op = (wi <= TOUR_MAX_LEN) & band[i, j - i - 1]
        n_open += int(op[:-1].sum())
        op[-1] = True   # the input leg
        key = np.where(op, D[i] + wi, np.iinfo(np.int64).max)
        k = int(np.argmin(key))   # the first minimum: the lowest i
        D[j], pred[j] = key[k], i[k]
    corners = [L - 1]
    while corners[-1] != 0:
        corners.append(int(pred[corners[-1]]))
    corners = corners[::-1]
    m = len(corners) - 1
    corner = np.full(L, -1, dtype=np.int32)
    corner[:m + 1] = corners
    H = path_spacing_fixed(spacing)
    wq = [int(w[a, b]) for a, b in zip(corners, corners[1:])]
    nq = [max(1, (x + H - 1) // H) if H else 1 for x in wq]
    R = 1 + sum(nq)
    out = dict(status=0, m=m, R=R, length_fixed=int(D[-1]), input_length_fixed=int(w[idx[:-1], idx[1:]].sum()), n_open=n_open, D=D,
               pred=pred, corner=corner, corners=np.asarray(corners, dtype=np.int64), row_node=None, poses=None, quats=None)
    if R > max_rows:
        out["status"] = 2
        return out
    Pd = P.astype(np.float64)
    poses, row_node = np.empty((R, 3), dtype=np.float32), np.full(R, -1, dtype=np.int32)
    qrows = np.empty((R, 4), dtype=np.float32) if quats is not None else None
    pre = np.concatenate([[0], np.cumsum(wq)]).astype(np.int64)   # the corner legs' lengths before corner q
    pos = {c: q for q, c in enumerate(corners)}
    r = 0
    for q, (a, b) in enumerate(zip(corners, corners[1:])):
        n = nq[q]
        f = np.arange(n, dtype=np.float64) / float(n)
        poses[r:r + n] = (Pd[a] + (Pd[b] - Pd[a]) * f[:, None]).astype(np.float32)
        poses[r] = P[a]
        row_node[r] = a
        if quats is not None:
            ka, kb = int(last[a]), int(nxt[a + 1])
            S = float(pre[pos[kb]] - pre[pos[ka]])
            qa, qb = _unit_quat(quats[ka]), _unit_quat(quats[kb])
            dot = ((qa[0] * qb[0] + qa[1] * qb[1]) + qa[2] * qb[2]) + qa[3] * qb[3]
            sg = -1.0 if dot < 0.0 else 1.0
            for t in range(n):
                if t == 0 and kept[a]:
                    qrows[r] = _unit_quat(quats[a])
                    continue
                s = float(pre[q] - pre[pos[ka]]) + float(wq[q]) * float(t) / float(n)
                u = s / S if S > 0.0 else 0.0
                o = [(1.0 - u) * x + u * (sg * y) for x, y in zip(qa, qb)]
                nn = math.sqrt(((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3])
                qrows[r + t] = [x / nn for x in o]
        r += n
    poses[r], row_node[r] = P[L - 1], L - 1
    if quats is not None:
        qrows[r] = _unit_quat(quats[L - 1])
    out.update(poses=poses, row_node=row_node, quats=qrows)
    return out


# ---- tools.propose_views restated in numpy: what propose_kernels.hip must give, element for element ------------------
VIEW_MAX_POSITIONS = 65536
VIEW_SECTORS = (8, 16, 32, 64, 128)
VIEW_MAX_PER_POSITION = 8
VIEW_MAX_WEIGHT = 32768


def propose_tables(S):
    """The two host-made tables of a proposal with S sectors -> (bounds (2, S/4 - 1) f32: row 0 c_k = (float)cos(2 pi k / S), row 1
    s_k = (float)sin(2 pi k / S) for k = 1 .. S/4 - 1, computed in f64; quats (S, 4) f32 wxyz: heading h looks along the centre of
    sector h, r_z((h + 1/2) 2 pi / S) (x) Q_OPTICAL, candidate_grid's convention)."""
    if S not in VIEW_SECTORS:
        raise ValueError(f"sectors must be one of {VIEW_SECTORS}, got {S!r}")
    ang = 2.0 * np.pi * np.arange(1, S // 4, dtype=np.float64) / S
    bounds = np.stack([np.cos(ang), np.sin(ang)]).astype(np.float32)
    mid = (np.arange(S, dtype=np.float64) + 0.5) * (2.0 * np.pi / S)
    rz = np.stack([np.cos(mid / 2), np.zeros(S), np.zeros(S), np.sin(mid / 2)], axis=1)
    return bounds, quat_mul(rz, Q_OPTICAL[None, :]).astype(np.float32)


def propose_sectors(dx, dy, S, bounds):
    """The sector of each (dx, dy) f32 pair: q S/4 + the COUNT of boundaries k with fl(b c_k) >= fl(a s_k); -1 where dx = dy = 0 (or
    a NaN) gives no quadrant.  f32, operation for operation."""
    dx, dy = np.asarray(dx, dtype=np.float32), np.asarray(dy, dtype=np.float32)
    c, s = np.asarray(bounds[0], dtype=np.float32), np.asarray(bounds[1], dtype=np.float32)
    quad = [(dx > 0) & (dy >= 0), (dx <= 0) & (dy > 0), (dx < 0) & (dy <= 0), (dx >= 0) & (dy < 0)]
    a = np.select(quad, [dx, dy, -dx, -dy], default=np.float32(0)).astype(np.float32)
    b = np.select(quad, [dy, -dx, -dy, dx], default=np.float32(0)).astype(np.float32)
    q = np.select(quad, [0, 1, 2, 3], default=-1)
    with np.errstate(all="ignore"):
        count = ((b[:, None] * c[None, :]) >= (a[:, None] * s[None, :])).sum(axis=1)
    return np.where(q >= 0, q * (S // 4) + count, -1).astype(np.int64)


def propose_hist_ref(points, positions, open, weights, S, min_dist, max_dist, tan_v):
    """hist (M, S) int64 of the pair test (propose_kernels.hip's header), in numpy f32 operation for operation: points (N,3),
    positions (M,3), open (M,) (zero = closed), weights (N,) integers in the points' row order or None (every point weighs 1)."""
    f32 = np.float32
    P, T = np.asarray(points, dtype=f32).reshape(-1, 3), np.asarray(positions, dtype=f32).reshape(-1, 3)
    op = np.asarray(open).reshape(-1) != 0
    w = np.ones(len(P), dtype=np.int64) if weights is None else np.asarray(weights).astype(np.int64).reshape(-1)
    bounds, _ = propose_tables(S)
    fin = np.isfinite(P).all(axis=1)
    X, Y, Z, w = P[fin, 0], P[fin, 1], P[fin, 2], w[fin]
    mn, mx, tv = f32(min_dist), f32(max_dist), f32(tan_v)
    hist = np.zeros((len(T), S), dtype=np.int64)
    with np.errstate(all="ignore"):
        min2, max2, tv2 = mn * mn, mx * mx, tv * tv
        for c in range(len(T)):
            t = T[c]
            if not op[c] or not np.isfinite(t).all():
                continue
            dx, dy, dz = X - t[0], Y - t[1], Z - t[2]
            hh, zz = dx * dx + dy * dy, dz * dz
            r2 = hh + zz
            g = (r2 >= min2) & (r2 <= max2) & (zz <= tv2 * hh)
            sec = propose_sectors(dx[g], dy[g], S, bounds)
            ok = sec >= 0
            # (float64 weights in bincount: the sums are integers below 2^53, so they are exact)
            hist[c] = np.bincount(sec[ok], weights=w[g][ok].astype(np.float64), minlength=S).astype(np.int64)
    return hist


def propose_headings_ref(hist, hw, n_per, sep=None, min_score=0):
    """(heading (M, n_per) int32, score (M, n_per) int64) of hist (M, S) int64: circular window sums over |j| <= hw, then n_per
    rounds of the argmax over the unsuppressed headings with score >= max(min_score, 1), ties to the lowest h, suppressing every h
    within sep (circular; default 2 hw) of the winner; -1 / 0 in the slots no round fills."""
    hist = np.asarray(hist, dtype=np.int64)
    M, S = hist.shape
    sep = 2 * hw if sep is None else sep
    win = np.zeros_like(hist)
    for j in range(-hw, hw + 1):
        win += np.roll(hist, -j, axis=1)   # win[h] += hist[(h + j) mod S]
    heading = np.full((M, n_per), -1, dtype=np.int32)
    score = np.zeros((M, n_per), dtype=np.int64)
    thr = max(int(min_score), 1)
    hs = np.arange(S)
    for c in range(M):
        free = win[c] >= thr
        for r in range(n_per):
            if not free.any():
                break
            best = int(win[c][free].max())
            h = int(np.flatnonzero(free & (win[c] == best))[0])
            heading[c, r], score[c, r] = h, best
            d = np.abs(hs - h)
            free &= np.minimum(d, S - d) > sep
    return heading, score


# ---- the occupancy grid and the line-of-sight walk restated in numpy: what occupancy_kernels.hip must give, bit for bit --
OCC_MAX_DIM = 2048
OCC_MAX_VOXELS = 1 << 31
LOS_MAX_SKIP = 8192


def occ_fixed(points, origin, resolution):
    """Fixed-point grid coordinates of world points -> (q (N,3) int64 in 1/256 voxel, ok (N,) bool): per axis g = fl(fl(p - origin) /
    r) in f32, in range iff -2048 <= g < 4096 (false for NaN and inf), q = floor(g * 256) (exact); q = 0 on an axis out of range."""
    f32 = np.float32
    P = np.asarray(points, dtype=f32).reshape(-1, 3)
    o, r = np.asarray(origin, dtype=f32).reshape(3), f32(resolution)
    with np.errstate(all="ignore"):
        g = ((P - o[None, :]).astype(f32) / r).astype(f32)
        ok = (g >= f32(-2048)) & (g < f32(4096))
        q = np.floor(np.where(ok, g, f32(0)) * f32(256)).astype(np.int64)
    return q, ok.all(axis=1)


def occupancy_ref(points, origin, resolution, dims, occ=None):
    """insert(points) -> (occ (nx,ny,nz) bool, skipped): a row in range whose voxel q >> 8 lies inside dims sets that voxel; every
    other row is counted.  occ: the grid so far (not modified) or None for an empty one."""
    dims = tuple(int(d) for d in dims)
    out = np.zeros(dims, dtype=bool) if occ is None else np.array(occ, dtype=bool)
    q, ok = occ_fixed(points, origin, resolution)
    v = q >> 8
    inside = ok & ((v >= 0) & (v < np.asarray(dims)[None, :])).all(axis=1)
    out[v[inside, 0], v[inside, 1], v[inside, 2]] = True
    return out, int((~inside).sum())


def walk_fixed(A, B, visit):
    """The walk from A to B, (R,3) integer fixed-point triples (both in range), vectorised over the rays still walking — the one
    restatement of the kernels' step block.  v = A >> 8, e = B >> 8, n = the distance to the next face ((v+1) 256 - A going up, A - v
    256 going down); sum |e - v| steps, each along the axis — among those with v_a != e_a — of the smallest n_a / m_a (n_a m_b < n_b
    m_a in int64, ties to the lowest axis).  At every round visit(idx, vi, last) gets the rays still walking, their voxels and which
    of them stand on their end voxel; it returns the rays that walk on as a bool array, or None for all.  A ray on its end voxel
    stops whatever visit says."""
    A, B = np.asarray(A, dtype=np.int64).reshape(-1, 3), np.asarray(B, dtype=np.int64).reshape(-1, 3)
    D = B - A
    s, m = np.sign(D), np.abs(D)
    e = B >> 8
    v = A >> 8
    n = np.where(s > 0, (v + 1) * 256 - A, A - v * 256)
    idx = np.arange(len(A))
    while len(idx):
        vi = v[idx]
        last = (vi == e[idx]).all(axis=1)
        go = visit(idx, vi, last)
        idx = idx[~last if go is None else go & ~last]
        if not len(idx):
            break
        act, ni, mi = v[idx] != e[idx], n[idx], m[idx]
        best = np.full(len(idx), -1, dtype=np.int64)
        nb, mb = np.zeros(len(idx), dtype=np.int64), np.ones(len(idx), dtype=np.int64)
        for a in range(3):
            take = act[:, a] & ((best < 0) | (ni[:, a] * mb < nb * mi[:, a]))
            best = np.where(take, a, best)
            nb, mb = np.where(take, ni[:, a], nb), np.where(take, mi[:, a], mb)
        v[idx, best] += s[idx, best]
        n[idx, best] += 256


def los_fixed(A, B, occ, skip=(1, 1), trace=False):
    """walk_fixed from A to B through occ (nx,ny,nz) bool -> blocked (R,) bool: a visited voxel is tested iff cheb(v, v0) >= skip[0]
    and cheb(v, e) > skip[1]; blocked iff a tested voxel inside dims is occupied, and the ray stops there.  trace: every ray walks to
    its end and (blocked, visited) is returned, visited[r] the list of ray r's voxels v0 .. e."""
    A, B = np.asarray(A, dtype=np.int64).reshape(-1, 3), np.asarray(B, dtype=np.int64).reshape(-1, 3)
    occ = np.asarray(occ, dtype=bool)
    dims = np.asarray(occ.shape, dtype=np.int64)
    ss, es = int(skip[0]), int(skip[1])
    v0, e = A >> 8, B >> 8
    blocked = np.zeros(len(A), dtype=bool)
    visited = [[] for _ in range(len(A))] if trace else None

    def visit(idx, vi, last):
        if trace:
            for k, r in enumerate(idx):
                visited[r].append(tuple(int(c) for c in vi[k]))
        tested = (np.abs(vi - v0[idx]).max(axis=1) >= ss) & (np.abs(vi - e[idx]).max(axis=1) > es)
        t = tested & ((vi >= 0) & (vi < dims[None, :])).all(axis=1)
        hit = np.zeros(len(idx), dtype=bool)
        hit[t] = occ[vi[t, 0], vi[t, 1], vi[t, 2]]
        blocked[idx[hit]] = True
        return None if trace else ~hit

    walk_fixed(A, B, visit)
    return (blocked, visited) if trace else blocked


def los_ref(a, b, origin, resolution, occ, skip=(1, 1)):
    """line_of_sight(a, b) of world points (R,3) -> (R,) uint8: 1 clear, 0 blocked, 2 an endpoint out of range."""
    qa, oka = occ_fixed(a, origin, resolution)
    qb, okb = occ_fixed(b, origin, resolution)
    ok = oka & okb
    out = np.full(len(qa), 2, dtype=np.uint8)
    out[ok] = 1 - los_fixed(qa[ok], qb[ok], occ, skip).astype(np.uint8)
    return out


# ---- free-space carving, the three-state map, frontiers and the ordered listing restated in numpy ("Free space and
# frontiers"): what frontier_kernels.hip must give, bit for bit.  int64 throughout. --------------------------------------------------
CARVE_MAX_RANGE = 6144 * 256


def carve_clip(A, B, R):
    """The truncation rule on fixed-point triples (N,3) int64 -> (B' (N,3), hit (N,) bool): L = isqrt(D . D); with R > 0 and L > R,
    B' = A + sign(D) floor(|D| R / L) per axis and the ray is no hit; otherwise B' = B and it is."""
    A, B = np.asarray(A, dtype=np.int64).reshape(-1, 3), np.asarray(B, dtype=np.int64).reshape(-1, 3)
    D = B - A
    L = np.array([math.isqrt(int(d)) for d in (D * D).sum(axis=1)], dtype=np.int64)
    R = int(R)
    cut = (L > R) if R > 0 else np.zeros(len(A), dtype=bool)
    Bc = A + np.sign(D) * (np.abs(D) * R // np.maximum(L, 1)[:, None])
    return np.where(cut[:, None], Bc, B), ~cut


def carve_fixed(A, B, hit, free):
    """walk_fixed from A to B (fixed-point triples, in range), setting free[v] for every visited voxel inside dims except the last
    voxel of a ray with hit[i]; free (nx,ny,nz) bool is modified in place.  -> the number of voxels visited (v_0 ... v_T of every
    ray).  tests/test_frontier_cpu.py checks it against los_fixed(trace=True)."""
    hit = np.asarray(hit, dtype=bool).reshape(-1)
    dims = np.asarray(free.shape, dtype=np.int64)
    visits = [0]

    def visit(idx, vi, last):
        visits[0] += len(idx)
        mark = ~(last & hit[idx]) & ((vi >= 0) & (vi < dims[None, :])).all(axis=1)
        free[vi[mark, 0], vi[mark, 1], vi[mark, 2]] = True

    walk_fixed(A, B, visit)
    return visits[0]


def carve_range(max_range, resolution):
    """max_range in metres -> R in 1/256 voxel: floor(float64(max_range) / float64(f32 resolution) * 256); None -> 0 (no limit)."""
    if max_range is None:
        return 0
    return int(math.floor(float(max_range) / float(np.float32(resolution)) * 256.0))


def carve_ref(origins, points, origin, resolution, dims, max_range=None, free=None, R=None):
    """carve(origins, points, max_range) -> (free (nx,ny,nz) bool, skipped, flags (N,) uint8: 0 hit, 1 truncated, 2 skipped,
    visits).  origins: (3,) / (1,3) shared or (N,3).  free: the plane so far (not modified) or None.  R: the fixed-point range
    itself instead of max_range."""
    dims = tuple(int(d) for d in dims)
    out = np.zeros(dims, dtype=bool) if free is None else np.array(free, dtype=bool)
    P = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    O = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    if len(O) == 1:
        O = np.broadcast_to(O, P.shape)
    qa, oka = occ_fixed(O, origin, resolution)
    qb, okb = occ_fixed(P, origin, resolution)
    ok = oka & okb
    R = carve_range(max_range, resolution) if R is None else int(R)
    flags = np.full(len(P), 2, dtype=np.uint8)
    Bc, hit = carve_clip(qa[ok], qb[ok], R)
    flags[ok] = np.where(hit, 0, 1)
    visits = carve_fixed(qa[ok], Bc, hit, out)
    return out, int((~ok).sum()), flags, visits


def state_ref(positions, origin, resolution, occ, free):
    """(M,3) world positions -> (M,) uint8: 2 occupied, 1 free, 0 unknown, 3 out of range or outside dims."""
    occ, free = np.asarray(occ, dtype=bool), np.asarray(free, dtype=bool)
    q, ok = occ_fixed(positions, origin, resolution)
    v = q >> 8
    inside = ok & ((v >= 0) & (v < np.asarray(occ.shape)[None, :])).all(axis=1)
    out = np.full(len(q), 3, dtype=np.uint8)
    vi = v[inside]
    out[inside] = np.where(occ[vi[:, 0], vi[:, 1], vi[:, 2]], 2, free[vi[:, 0], vi[:, 1], vi[:, 2]].astype(np.uint8))
    return out


def frontier_ref(occ, free, min_unknown=1):
    """The frontier mask (nx,ny,nz) bool: state 1 and at least min_unknown of the six face neighbours inside dims in state 0."""
    occ, free = np.asarray(occ, dtype=bool), np.asarray(free, dtype=bool)
    unknown = ~occ & ~free
    cnt = np.zeros(occ.shape, dtype=np.int64)
    for ax in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        cnt[tuple(lo)] += unknown[tuple(hi)]
        cnt[tuple(hi)] += unknown[tuple(lo)]
    return free & ~occ & (cnt >= int(min_unknown))


def occ_export_ref(grid, origin, resolution):
    """export() of a grid (nx,ny,nz) bool -> (ijk (F,3) int32, centres (F,3) f32) in ascending (word, bit) order: word = ((z >> 1)
    nby + (y >> 2)) nbx + (x >> 2), bit = x & 3 | (y & 3) << 2 | (z & 1) << 4; centre = fl(origin + fl(fl(i + 0.5) r)) in f32."""
    g = np.asarray(grid, dtype=bool)
    return occ_export_sparse(np.argwhere(g), g.shape, origin, resolution)


def occ_export_sparse(ijk, dims, origin, resolution):
    """occ_export_ref of the grid of `dims` whose set voxels are the rows of ijk (M,3) — distinct and inside dims — without the dense
    grid: the rows sorted by the same (word, bit) key, and their centres.  For grids too large to hold as a bool array."""
    nbx, nby = (int(dims[0]) + 3) // 4, (int(dims[1]) + 3) // 4
    ijk = np.asarray(ijk, dtype=np.int64).reshape(-1, 3)
    x, y, z = ijk[:, 0], ijk[:, 1], ijk[:, 2]
    key = ((((z >> 1) * nby + (y >> 2)) * nbx + (x >> 2)) << 5) | (x & 3) | ((y & 3) << 2) | ((z & 1) << 4)
    ijk = ijk[np.argsort(key, kind="stable")]
    f32 = np.float32
    o, r = np.asarray(origin, dtype=f32).reshape(3), f32(resolution)
    centres = (o[None, :] + ((ijk.astype(f32) + f32(0.5)) * r).astype(f32)).astype(f32)
    return ijk.astype(np.int32), centres


# ---- the unknown volume a view reveals and the greedy choice by it restated in numpy ("Unknown volume"): what
# volume_kernels.hip must give, bit for bit.  int64 throughout. -------------------------------------------------------------------------
def unknown_ref(occ, free):
    """SpaceMap.unknown() -> (nx,ny,nz) bool: the voxels of state 0, neither occupied nor free."""
    return ~np.asarray(occ, dtype=bool) & ~np.asarray(free, dtype=bool)


def voxel_centres(dims, origin, resolution):
    """The centre of every voxel of a grid -> (nx,ny,nz,3) f32: fl(origin + fl(fl(i + 0.5) r)) per axis, export()'s rule."""
    f32 = np.float32
    o, r = np.asarray(origin, dtype=f32).reshape(3), f32(resolution)
    ax = [(o[a] + ((np.arange(int(dims[a])).astype(f32) + f32(0.5)) * r).astype(f32)).astype(f32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).astype(f32)


def _seen_candidates(cand, t, origin, resolution, occ):
    """The voxels of the mask cand (nx,ny,nz) bool that the walk from t sees -> (nx,ny,nz) bool: los_fixed from the camera position t
    to the voxel's centre with skip (1, 0) finds no occupied voxel.  A position t out of range, or a centre out of range, sees nothing."""
    seen = np.zeros(occ.shape, dtype=bool)
    qa, oka = occ_fixed(np.asarray(t, dtype=np.float32).reshape(1, 3), origin, resolution)
    ijk = np.argwhere(cand)
    if not oka[0] or not len(ijk):
        return seen
    c = voxel_centres(occ.shape, origin, resolution)[ijk[:, 0], ijk[:, 1], ijk[:, 2]]
    qb, okb = occ_fixed(c, origin, resolution)
    clear = np.zeros(len(ijk), dtype=bool)
    clear[okb] = ~los_fixed(np.broadcast_to(qa, qb[okb].shape), qb[okb], occ, (1, 0))
    ijk = ijk[clear]
    seen[ijk[:, 0], ijk[:, 1], ijk[:, 2]] = True
    return seen


def view_volume_ref(kept, t, origin, resolution, occ, free, claimed=None):
    """The voxels one view reveals -> (gain, revealed (nx,ny,nz) bool).  kept: (nx,ny,nz) bool, the cull's verdict on every voxel's
    centre — an input, so the f32 cull is not re-derived here.  A voxel is revealed iff its state is 0, it is not set in claimed,
    kept holds it and los_fixed from the camera position t to its centre with skip (1, 0) finds no occupied voxel: the camera's own
    voxel and the target are not tested, unknown voxels do not block.  A position t out of range, or a centre out of range,
    reveals nothing."""
    occ, free = np.asarray(occ, dtype=bool), np.asarray(free, dtype=bool)
    cand = unknown_ref(occ, free) & np.asarray(kept, dtype=bool)
    if claimed is not None:
        cand &= ~np.asarray(claimed, dtype=bool)
    revealed = _seen_candidates(cand, t, origin, resolution, occ)
    return int(revealed.sum()), revealed


def information_weights_ref(values_int8, table):
    """The weight of every voxel -> (nx,ny,nz) int64: table[L + 128], the table (256,) read as unsigned 16-bit."""
    L = np.asarray(values_int8).astype(np.int64)
    W = np.asarray(table).astype(np.int64).reshape(256)
    assert L.min() >= -128 and L.max() <= 127 and W.min() >= 0 and W.max() <= 65535
    return W[L + 128]


def view_information_ref(kept, t, origin, resolution, values_int8, occ, table, claimed=None):
    """The information one view gains -> (gain, informed (nx,ny,nz) bool).  values_int8: the map's evidence values (nx,ny,nz), -128
    never observed; table: (256,) weights indexed by L + 128; occ: the occupied plane the walk tests (the map's: L > threshold).  A
    voxel is a candidate iff its weight is positive, whatever its state; it is informed iff it is not set in claimed, kept holds it
    and the walk of view_volume_ref sees it — the target voxel is not tested, so an occupied candidate can be informed.  gain = the sum
    of the informed voxels' weights, int64."""
    occ = np.asarray(occ, dtype=bool)
    weights = information_weights_ref(values_int8, table)
    cand = (weights > 0) & np.asarray(kept, dtype=bool)
    if claimed is not None:
        cand &= ~np.asarray(claimed, dtype=bool)
    informed = _seen_candidates(cand, t, origin, resolution, occ)
    return int(weights[informed].sum()), informed


def volume_select_ref(revealed_sets, k, min_gain=1, claimed=None):
    """The greedy selection over per-view revealed masks (M, nx,ny,nz) bool, each computed WITHOUT a claimed plane -> (order list,
    gains list, revealed mask).  Round after round the view not yet taken with the most voxels outside the claimed mask wins, the
    lowest index on ties; below min_gain the selection stops; otherwise its voxels join the mask.  (A voxel's line of sight does not
    depend on the claimed plane, so masking afterwards equals scoring against it.)"""
    sets = np.asarray(revealed_sets, dtype=bool)
    mask = np.zeros(sets.shape[1:], dtype=bool) if claimed is None else np.array(claimed, dtype=bool)
    taken, order, gains = np.zeros(len(sets), dtype=bool), [], []
    for _ in range(min(int(k), len(sets))):
        g = np.array([-1 if taken[i] else int((sets[i] & ~mask).sum()) for i in range(len(sets))], dtype=np.int64)
        best = int(np.argmax(g))   # (the first of equal gains)
        if g[best] < int(min_gain):
            break
        taken[best] = True
        order.append(best)
        gains.append(int(g[best]))
        mask |= sets[best]
    return order, gains, mask


def information_select_ref(informed_sets, weights, k, min_gain=1, claimed=None):
    """volume_select_ref with a weight per voxel: the greedy selection over per-view informed masks (M, nx,ny,nz) bool, each computed
    WITHOUT a claimed plane, and weights (nx,ny,nz) int64 -> (order list, gains list, claimed mask).  A view's gain is the sum of the
    weights of its voxels outside the mask; the lowest index wins a tie; below min_gain the selection stops."""
    sets, weights = np.asarray(informed_sets, dtype=bool), np.asarray(weights, dtype=np.int64)
    mask = np.zeros(sets.shape[1:], dtype=bool) if claimed is None else np.array(claimed, dtype=bool)
    taken, order, gains = np.zeros(len(sets), dtype=bool), [], []
    for _ in range(min(int(k), len(sets))):
        g = np.array([-1 if taken[i] else int(weights[sets[i] & ~mask].sum()) for i in range(len(sets))], dtype=np.int64)
        best = int(np.argmax(g))   # (the first of equal gains)
        if g[best] < int(min_gain):
            break
        taken[best] = True
        order.append(best)
        gains.append(int(g[best]))
        mask |= sets[best]
    return order, gains, mask


# ---- ray casts and depth scans restated in numpy ("Ray casts and depth scans"): what raycast_kernels.hip must give, bit
# for bit.  Visitors of walk_fixed in int64; the f32 ray arithmetic operation by operation. ------------------------------------------
SCAN_MAX_SIDE = 8192
SCAN_MAX_VIEWS = 65535


def cast_fixed(A, B, occ, skip=(1, 0), marks=None, plane=None):
    """The cast of A -> B, (R,3) fixed-point triples (both in range), through occ (nx,ny,nz) bool: walk_fixed, stopped at the HIT,
    the first visited voxel that los_fixed would call occupied (cheb(v, v0) >= skip[0], cheb(v, e) > skip[1], inside dims, set).
    -> dict(hit (R,) bool, voxel (R,3) int64 the hit voxel, steps (R,3) int64 the steps taken per axis when the walk stood on it, last
    (R,) int64 the axis of the last of them (-1: none), visits (R,) int64 the voxels looked at: those with cheb(v, e) > skip[1] up to
    and including the hit).  marks (R,) int64 with plane (nx,ny,nz) bool: instead of casting, the first marks[i] looked-at voxels of
    ray i that lie inside dims are set in plane (the walk in front of a known hit), and nothing is tested."""
    A, B = np.asarray(A, dtype=np.int64).reshape(-1, 3), np.asarray(B, dtype=np.int64).reshape(-1, 3)
    occ = np.asarray(occ, dtype=bool)
    dims = np.asarray(occ.shape, dtype=np.int64)
    ss, es = int(skip[0]), int(skip[1])
    R = len(A)
    v0, e = A >> 8, B >> 8
    out = dict(hit=np.zeros(R, dtype=bool), voxel=np.zeros((R, 3), dtype=np.int64), steps=np.zeros((R, 3), dtype=np.int64),
               last=np.full(R, -1, dtype=np.int64), visits=np.zeros(R, dtype=np.int64))
    prev, axis = v0.copy(), np.full(R, -1, dtype=np.int64)
    left = None if marks is None else np.array(marks, dtype=np.int64)

    def visit(idx, vi, last):
        moved = vi != prev[idx]
        axis[idx] = np.where(moved.any(axis=1), moved.argmax(axis=1), axis[idx])
        prev[idx] = vi
        seen = np.abs(vi - e[idx]).max(axis=1) > es
        inside = ((vi >= 0) & (vi < dims[None, :])).all(axis=1)
        if left is not None:
            seen &= left[idx] > 0
            left[idx[seen]] -= 1
            m = seen & inside
            plane[vi[m, 0], vi[m, 1], vi[m, 2]] = True
            return seen
        out["visits"][idx[seen]] += 1
        t = seen & (np.abs(vi - v0[idx]).max(axis=1) >= ss) & inside
        hit = np.zeros(len(idx), dtype=bool)
        hit[t] = occ[vi[t, 0], vi[t, 1], vi[t, 2]]
        r = idx[hit]
        out["hit"][r], out["voxel"][r], out["steps"][r], out["last"][r] = True, vi[hit], np.abs(vi[hit] - v0[r]), axis[r]
        return seen & ~hit   # (the distance to e only falls: a voxel not looked at ends the walk)

    walk_fixed(A, B, visit)
    return out


def cast_entry(A, B, steps, last=None):
    """The entry parameter of the voxel reached from A (towards B) by steps (R,3) per axis -> (num, den) int64, the exact rational:
    with last (R,) — the axis of the last step, -1 for none — the crossing parameter n / m of that step, n = n0 + 256 (k - 1) the
    distance to the face before the step added 256; without it the maximum over the axes with k > 0 of (n0_a + 256 (k_a - 1)) / m_a
    by integer cross-multiplication, the lowest axis kept on ties (equal rationals: the same f32 quotient).  0/1 with no step."""
    A, B = np.asarray(A, dtype=np.int64).reshape(-1, 3), np.asarray(B, dtype=np.int64).reshape(-1, 3)
    k = np.asarray(steps, dtype=np.int64).reshape(-1, 3)
    D = B - A
    s, m = np.sign(D), np.abs(D)
    v = A >> 8
    n = np.where(s > 0, (v + 1) * 256 - A, A - v * 256) + 256 * (k - 1)
    num, den = np.zeros(len(A), dtype=np.int64), np.ones(len(A), dtype=np.int64)
    if last is not None:
        last = np.asarray(last, dtype=np.int64).reshape(-1)
        has, a = last >= 0, np.maximum(last, 0)
        rows = np.arange(len(A))
        return np.where(has, n[rows, a], num), np.where(has, m[rows, a], den)
    for a in range(3):
        take = (k[:, a] > 0) & (n[:, a] * den > num * m[:, a])
        num, den = np.where(take, n[:, a], num), np.where(take, m[:, a], den)
    return num, den


def cast_lam(num, den):
    """lam = fl(f32(num) / f32(den)): both are exact in f32 (< 2^24) and the division is correctly rounded."""
    return (np.asarray(num).astype(np.float32) / np.asarray(den).astype(np.float32)).astype(np.float32)


def cast_ref(a, b, origin, resolution, occ, skip=(1, 0)):
    """OccupancyGrid.cast(a, b, skip) of world points (R,3) -> (voxel (R,) int32: i + nx (j + ny k) of the hit, -1 clear, -2 an
    endpoint out of range; lam (R,) f32: the entry parameter, 1 clear, NaN out of range; visits: the voxels looked at)."""
    occ = np.asarray(occ, dtype=bool)
    qa, oka = occ_fixed(a, origin, resolution)
    qb, okb = occ_fixed(b, origin, resolution)
    ok = oka & okb
    voxel, lam = np.full(len(qa), -2, dtype=np.int32), np.full(len(qa), np.nan, dtype=np.float32)
    c = cast_fixed(qa[ok], qb[ok], occ, skip)
    num, den = cast_entry(qa[ok], qb[ok], c["steps"])
    v = c["voxel"]
    voxel[ok] = np.where(c["hit"], v[:, 0] + occ.shape[0] * (v[:, 1] + occ.shape[1] * v[:, 2]), -1)
    lam[ok] = np.where(c["hit"], cast_lam(num, den), np.float32(1))
    return voxel, lam, int(c["visits"].sum())


def exact_pose_ref(quats):
    """exact_pose(normalize = 1) of quaternions (V,4) wxyz in f32, operation by operation: ss = ((w w + x x) + y y) + z z, n =
    max(sqrt(ss), 1e-12), q / n."""
    f32 = np.float32
    q = np.asarray(quats, dtype=f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ss = (q[:, 0] * q[:, 0]).astype(f32)
        for a in (1, 2, 3):
            ss = (ss + (q[:, a] * q[:, a]).astype(f32)).astype(f32)
        nn = np.sqrt(ss).astype(f32)
        nn = np.where(nn < f32(1e-12), f32(1e-12), nn).astype(f32)
        return (q / nn[:, None]).astype(f32)


def scan_rays_ref(poses, quats, K, img_width, img_height, max_dist):
    """The far point of every pixel's ray -> (V, H, W, 3) f32, every operation rounded in f32 and none fused: dc = ((x - cx) / fx,
    (y - cy) / fy, 1), Fc = (dc.x D, dc.y D, D), B = rot(q, Fc) + t with q = exact_pose_ref(quats) and rot = q (0, Fc) conj(q) as two
    Hamilton products in exact_to_cam's order of terms."""
    f32 = np.float32
    K = np.asarray(K, dtype=f32).reshape(9)
    W, H, D = int(img_width), int(img_height), f32(max_dist)
    t = np.asarray(poses, dtype=f32).reshape(-1, 3)
    q = exact_pose_ref(quats)
    with np.errstate(all="ignore"):
        dx = ((np.arange(W).astype(f32) - K[2]).astype(f32) / K[0]).astype(f32)
        dy = ((np.arange(H).astype(f32) - K[5]).astype(f32) / K[4]).astype(f32)
        shape = (len(t), H, W)
        bx = np.broadcast_to((dx * D).astype(f32)[None, None, :], shape)
        by = np.broadcast_to((dy * D).astype(f32)[None, :, None], shape)
        bz = np.broadcast_to(D, shape)
        bw = np.zeros(shape, dtype=f32)
        aw, ax, ay, az = (q[:, i][:, None, None] for i in range(4))
        cw, cx, cy, cz = aw, -ax, -ay, -az
        ow = aw * bw - ax * bx - ay * by - az * bz
        ox = aw * bx + ax * bw + ay * bz - az * by
        oy = aw * by - ax * bz + ay * bw + az * bx
        oz = aw * bz + ax * by - ay * bx + az * bw
        r = [ow * cx + ox * cw + oy * cz - oz * cy, ow * cy - ox * cz + oy * cw + oz * cx, ow * cz + ox * cy - oy * cx + oz * cw]
        out = np.stack([r[a] + t[:, a][:, None, None] for a in range(3)], axis=-1)
    assert out.dtype == f32
    return out


def depth_scan_ref(poses, quats, K, img_width, img_height, min_dist, max_dist, origin, resolution, occ):
    """depth_scan of the grid occ (nx,ny,nz) bool -> dict(voxel (V,H,W) int32, depth (V,H,W) f32, flags (V,H,W) uint8, points
    (V,H,W,3) f32, far (V,H,W,3) f32, hit_plane and pass_plane (nx,ny,nz) bool, rays, visits): per pixel the cast t -> B with skip
    (1, 0); flags 0 a return, 1 none within max_dist, 2 skipped (t or B out of range), 3 a hit with !(depth > min_dist); depth =
    fl(lam D), +inf for flag 1, NaN for flag 2; points: the hit voxel's centre (flag 0), B (flag 1), NaN otherwise.  hit_plane: the
    flag-0 hit voxels; pass_plane: the voxels inside dims that a ray of flag 0 or 1 looked at before its hit."""
    f32 = np.float32
    occ = np.asarray(occ, dtype=bool)
    nx, ny, _ = occ.shape
    far = scan_rays_ref(poses, quats, K, img_width, img_height, max_dist)
    V, H, W, _ = far.shape
    t = np.asarray(poses, dtype=f32).reshape(-1, 3)
    qa, oka = occ_fixed(np.repeat(t, H * W, axis=0), origin, resolution)
    qb, okb = occ_fixed(far.reshape(-1, 3), origin, resolution)
    ok = oka & okb
    n = len(qa)
    voxel, depth = np.full(n, -2, dtype=np.int32), np.full(n, np.nan, dtype=f32)
    flags, points = np.full(n, 2, dtype=np.uint8), np.full((n, 3), np.nan, dtype=f32)
    A, B = qa[ok], qb[ok]
    c = cast_fixed(A, B, occ, (1, 0))
    num, den = cast_entry(A, B, c["steps"])
    hit, v = c["hit"], c["voxel"]
    dep = (cast_lam(num, den) * f32(max_dist)).astype(f32)
    fl = np.where(hit, np.where(dep > f32(min_dist), 0, 3), 1).astype(np.uint8)
    voxel[ok] = np.where(hit, v[:, 0] + nx * (v[:, 1] + ny * v[:, 2]), -1)
    depth[ok] = np.where(hit, dep, f32(np.inf))
    flags[ok] = fl
    o, r = np.asarray(origin, dtype=f32).reshape(3), f32(resolution)
    centre = (o[None, :] + ((v.astype(f32) + f32(0.5)) * r).astype(f32)).astype(f32)
    p = np.full((len(A), 3), np.nan, dtype=f32)
    p[fl == 0], p[fl == 1] = centre[fl == 0], far.reshape(-1, 3)[ok][fl == 1]
    points[ok] = p
    hit_plane, pass_plane = np.zeros(occ.shape, dtype=bool), np.zeros(occ.shape, dtype=bool)
    h = v[fl == 0]
    hit_plane[h[:, 0], h[:, 1], h[:, 2]] = True
    cast_fixed(A, B, occ, (1, 0), marks=np.where(fl == 3, 0, c["visits"] - hit), plane=pass_plane)
    return dict(voxel=voxel.reshape(V, H, W), depth=depth.reshape(V, H, W), flags=flags.reshape(V, H, W), points=points.reshape(V, H, W, 3),
                far=far, hit_plane=hit_plane, pass_plane=pass_plane, rays=int(ok.sum()), visits=int(c["visits"].sum()))


def box_room(doorway=False, step=0.02):
    """A scanned room for the exploration tests and the sample: the six faces of the box [0, 2] x [0, 2] x [0, 1] sampled every `step`
    metres, face after face (edges and corners appear once per face) -> (N,3) f32; doorway: the wall x = 2 is left open for y in
    (0.75, 1.25), z in (0.01, 0.75)."""
    s, z = np.arange(int(round(2.0 / step)) + 1) * step, np.arange(int(round(1.0 / step)) + 1) * step
    faces = []
    for x in (0.0, 2.0):
        Y, Z = np.meshgrid(s, z, indexing="ij")
        faces.append(np.stack([np.full(Y.size, x), Y.ravel(), Z.ravel()], axis=1))
    for y in (0.0, 2.0):
        X, Z = np.meshgrid(s, z, indexing="ij")
        faces.append(np.stack([X.ravel(), np.full(X.size, y), Z.ravel()], axis=1))
    for h in (0.0, 1.0):
        X, Y = np.meshgrid(s, s, indexing="ij")
        faces.append(np.stack([X.ravel(), Y.ravel(), np.full(X.size, h)], axis=1))
    P = np.concatenate(faces)
    if doorway:
        P = P[~((P[:, 0] == 2.0) & (P[:, 1] > 0.75) & (P[:, 1] < 1.25) & (P[:, 2] > 0.01) & (P[:, 2] < 0.75))]
    return P.astype(np.float32)


def doorway_beams(origin, far=6.0):
    """No-return beams through box_room's doorway, as a scanner reports them: far points `far` metres out along 9 x 7 directions
    from origin through the opening -> (63,3) f32."""
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    T = np.array([[2.0, y, z] for y in np.linspace(0.8, 1.2, 9) for z in np.linspace(0.1, 0.7, 7)])
    d = T - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (o + far * d).astype(np.float32)


# ---- the clearance field restated in numpy ("Clearance field"): what field_kernels.hip must give, bit for bit.  int64
# throughout. ------------------------------------------------------------------------------------------------------------------------
FIELD_SENTINEL = 65535
FIELD_MAX_D = 254
FIELD_UNKNOWN = ("free", "obstacle")


def field_obstacles(occ, free=None, unknown="free"):
    """The obstacle mask (nx,ny,nz) bool: the occupied voxels and, with unknown='obstacle', also those of state 0 (neither bit)."""
    occ = np.asarray(occ, dtype=bool)
    if unknown not in FIELD_UNKNOWN:
        raise ValueError(f"unknown must be 'free' or 'obstacle', got {unknown!r}")
    if unknown == "free":
        return occ.copy()
    if free is None:
        raise ValueError("unknown='obstacle' needs the free plane")
    return occ | ~np.asarray(free, dtype=bool)


def _field_axis_cost(k, metric):
    k = abs(int(k))
    return (max(k - 1, 0) if metric == "gap" else k) ** 2


def field_ref(occ, free=None, D=8, unknown="free", metric="gap"):
    """The field (nx,ny,nz) int64 by three windowed passes of truncated min-plus — x, then y, then z; per-axis cost max(|k| - 1, 0)^2
    (metric='centre': k^2, the squared distance between voxel centres, for the cross-check against scipy); window +-(D + 1); values
    above D^2 dropped after each pass -> min over the obstacles of gap2 where that is <= D^2, else 65535."""
    D = int(D)
    if not 1 <= D <= FIELD_MAX_D:
        raise ValueError(f"D must be an integer in [1, {FIELD_MAX_D}], got {D}")
    big = np.int64(1) << 40
    f = np.where(field_obstacles(occ, free, unknown), np.int64(0), big)
    for ax in range(3):
        n = f.shape[ax]
        out = f.copy()   # (offset 0 costs 0)
        for k in range(1, min(D + 1, n - 1) + 1):
            c = _field_axis_cost(k, metric)
            if c > D * D:
                break
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, n - k), slice(k, n)
            lo, hi = tuple(lo), tuple(hi)
            out[lo] = np.minimum(out[lo], f[hi] + c)
            out[hi] = np.minimum(out[hi], f[lo] + c)
        f = np.where(out <= D * D, out, big)
    return np.where(f <= D * D, f, FIELD_SENTINEL).astype(np.int64)


def field_brute(occ, free=None, D=8, unknown="free", metric="gap"):
    """The field by its definition: the minimum of gap2(v, u) over all obstacles u, for small grids (memory: voxels x obstacles)."""
    D = int(D)
    obs = field_obstacles(occ, free, unknown)
    V = np.argwhere(np.ones(obs.shape, dtype=bool)).astype(np.int64)
    U = np.argwhere(obs).astype(np.int64)
    out = np.full(len(V), FIELD_SENTINEL, dtype=np.int64)
    if len(U):
        for lo in range(0, len(V), 1024):
            d = np.abs(V[lo:lo + 1024, None, :] - U[None, :, :])
            if metric == "gap":
                d = np.maximum(d - 1, 0)
            g2 = (d * d).sum(axis=2).min(axis=1)
            out[lo:lo + 1024] = np.where(g2 <= D * D, g2, FIELD_SENTINEL)
    return out.reshape(obs.shape)


def field_max_dist_voxels(max_dist, resolution):
    """max_dist in metres -> D in voxels: ceil(float64(max_dist) / float64(f32 resolution)) (not range-checked)."""
    return int(math.ceil(float(max_dist) / float(np.float32(resolution))))


def field_need2(radius, resolution):
    """The squared gap, in voxels, that certifies `radius` metres: ceil((float64(radius) / float64(f32 resolution) + 1/64)^2).  The
    1/64 voxel covers the 1/256-voxel quantisation of a leg's endpoints (at most sqrt(3)/256 voxel off the true segment) and the f32
    rounding of the fixed-point coordinates."""
    return int(math.ceil((float(radius) / float(np.float32(resolution)) + 1.0 / 64.0) ** 2))


def field_positions_ref(positions, origin, resolution, field):
    """(M,3) world positions -> (M,) int32: the voxel's value, 65535 in range but outside dims, -1 out of range."""
    field = np.asarray(field)
    q, ok = occ_fixed(positions, origin, resolution)
    v = q >> 8
    inside = ok & ((v >= 0) & (v < np.asarray(field.shape)[None, :])).all(axis=1)
    out = np.where(ok, FIELD_SENTINEL, -1).astype(np.int32)
    out[inside] = field[v[inside, 0], v[inside, 1], v[inside, 2]]
    return out


def field_segments_ref(a, b, origin, resolution, field):
    """The segment query (E,3), (E,3) world points -> (d2 (E,) int32, vox (E,) int32), on top of walk_fixed: the minimum of the field
    over the visited voxels v_0 ... v_T inside dims (65535: none inside, or all hold 65535; -1: an endpoint out of range) and the
    linear index (k ny + j) nx + i of the first visited voxel that attains it (-1 with 65535 or -1).  Vectorised over the legs: a
    visitor that keeps a strictly smaller value, so the first voxel in walk order wins (tests/test_map_at_size_cpu.py restates it
    voxel by voxel over los_fixed's trace)."""
    field = np.asarray(field)
    nx, ny, nz = field.shape
    dims = np.asarray(field.shape, dtype=np.int64)
    qa, oka = occ_fixed(a, origin, resolution)
    qb, okb = occ_fixed(b, origin, resolution)
    ok = oka & okb
    best, arg = np.full(int(ok.sum()), FIELD_SENTINEL, dtype=np.int64), np.full(int(ok.sum()), -1, dtype=np.int64)

    def visit(idx, vi, last):
        inside = ((vi >= 0) & (vi < dims[None, :])).all(axis=1)
        r, v = idx[inside], vi[inside]
        val = field[v[:, 0], v[:, 1], v[:, 2]].astype(np.int64)
        less = val < best[r]
        best[r[less]], arg[r[less]] = val[less], ((v[:, 2] * ny + v[:, 1]) * nx + v[:, 0])[less]

    walk_fixed(qa[ok], qb[ok], visit)
    d2, vox = np.full(len(qa), -1, dtype=np.int32), np.full(len(qa), -1, dtype=np.int32)
    d2[ok], vox[ok] = best, arg
    return d2, vox


def field_metres(d2, resolution):
    """d2 (any shape) -> f32 metres: fl(fl(sqrt((float) d2)) r); +inf for 65535, NaN for -1."""
    d2 = np.asarray(d2, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        m = (np.sqrt(np.maximum(d2, 0).astype(np.float32)).astype(np.float32) * np.float32(resolution)).astype(np.float32)
    m = np.where(d2 == FIELD_SENTINEL, np.float32(np.inf), m)
    return np.where(d2 < 0, np.float32(np.nan), m).astype(np.float32)


def field_edges_ref(d2, vox, need2, resolution):
    """ClearanceField.edges from a segment query's answer -> (d f32, idx int32): an open leg (d2 >= need2) +inf / -1, a blocked one
    metres / vox, a leg with an endpoint out of range 0 / -2."""
    d2, vox = np.asarray(d2, dtype=np.int64), np.asarray(vox, dtype=np.int64)
    open_ = d2 >= int(need2)
    d = np.where(d2 < 0, np.float32(0), np.where(open_, np.float32(np.inf), field_metres(d2, resolution))).astype(np.float32)
    idx = np.where(d2 < 0, -2, np.where(open_, -1, vox)).astype(np.int32)
    return d, idx


def field_nodes_ref(field, need2, stride=1, state=None):
    """The node mask (nx,ny,nz) bool: field >= need2, every index i with i % stride == stride // 2 and, where state (nx,ny,nz) is
    given, state == 1 (free)."""
    field = np.asarray(field)
    stride = int(stride)
    m = field >= int(need2)
    for ax, n in enumerate(field.shape):
        sel = (np.arange(n) % stride) == stride // 2
        shape = [1, 1, 1]
        shape[ax] = n
        m = m & sel.reshape(shape)
    if state is not None:
        m = m & (np.asarray(state) == 1)
    return m


FIELD_ROOM = dict(origin=(-0.5, -0.5, -0.5), resolution=0.1, dims=(40, 30, 20))   # box_room and 1.5 m beyond its doorway


def field_room_legs(n=2000, seed=11):
    """Seeded random legs for the field's guarantee over box_room(doorway=True): both ends uniform in [0.05, 2.95] x [0.05, 1.95] x
    [0.05, 0.95], every other leg no longer than 0.5 m per axis (short legs are the ones a planner asks) -> (a, b) (n,3) f32."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([0.05, 0.05, 0.05]), np.array([2.95, 1.95, 0.95])
    a = rng.uniform(lo, hi, (n, 3))
    b = rng.uniform(lo, hi, (n, 3))
    short = np.clip(a + rng.uniform(-0.5, 0.5, (n, 3)), lo, hi)
    b[::2] = short[::2]
    return a.astype(np.float32), b.astype(np.float32)


def segment_point_distance(a, b, P, chunk=64):
    """min over the rows of P of the f64 distance from the point to the segment a[e] -> b[e] -> (E,) f64."""
    a, b, P = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(P, dtype=np.float64)
    out = np.empty(len(a))
    for lo in range(0, len(a), chunk):
        A, D = a[lo:lo + chunk, None, :], (b[lo:lo + chunk] - a[lo:lo + chunk])[:, None, :]
        dd = (D * D).sum(axis=2)
        t = np.clip(((P[None] - A) * D).sum(axis=2) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
        out[lo:lo + chunk] = np.sqrt((((A + t[..., None] * D) - P[None]) ** 2).sum(axis=2).min(axis=1))
    return out


def doorway_outside_scan(origin, n=24000, far=6.0):
    """A second message for box_room(doorway=True), taken from `origin` outside the wall x = 2 (origin[0] > 2): n beams on a Fibonacci
    sphere; a beam that meets the wall x = 2 (y in [0, 2], z in [0, 1], not the opening) returns that point, every other beam —
    into the open, or through the doorway — reports a far point `far` metres out, as a scanner does without a return -> (n,3) f32."""
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    rad = np.sqrt(1.0 - z * z)
    d = np.stack([rad * np.cos(phi), rad * np.sin(phi), z], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d[:, 0] < 0, (2.0 - o[0]) / d[:, 0], np.inf)
    hit = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d
    wall = np.isfinite(t) & (hit[:, 1] >= 0) & (hit[:, 1] <= 2) & (hit[:, 2] >= 0) & (hit[:, 2] <= 1)
    wall &= ~((hit[:, 1] > 0.75) & (hit[:, 1] < 1.25) & (hit[:, 2] > 0.01) & (hit[:, 2] < 0.75))
    hit[:, 0] = 2.0
    return np.where(wall[:, None], hit, o + far * d).astype(np.float32)


FIELD_DOORWAY = dict(origin=(-0.5, -0.5, -0.5), resolution=0.05, dims=(80, 60, 40))


def doorway_messages():
    """box_room(doorway=True) scanned as two messages -> [(scanner (3,) f32, rows (N,3) f32, max_range or None), ...]: the room from
    inside — the cone through the opening has no return and stays unknown — then doorway_outside_scan from 0.4 m beyond the door with
    a range of 1.4 m, which carves that cone and a ball of free space outside.  Beyond that ball nothing is known."""
    s1, s2 = np.float32([1.03, 0.97, 0.52]), np.float32([2.4, 1.0, 0.5])
    return [(s1, box_room(doorway=True), None), (s2, doorway_outside_scan(s2), 1.4)]


# ---- the travel field restated in numpy ("Travel field"): what travel_kernels.hip must give, bit for bit.  int64
# throughout, dense (nx,ny,nz) arrays, -1 = unreachable. ---------------------------------------------------------------------------
TRAVEL_WEIGHTS = (64, 91, 111)          # face, edge, corner moves, in 1/64 voxel edge: round(64 sqrt(k))
TRAVEL_MAX_LIMIT = (1 << 31) - 1
TRAVEL_MOVES = tuple((m % 3 - 1, (m // 3) % 3 - 1, m // 9 - 1) for m in range(27))   # move m = (dz+1) 9 + (dy+1) 3 + (dx+1) -> (dx, dy, dz)


def travel_limit(max_dist, resolution):
    """max_dist in metres (None: no truncation) -> the largest cost kept: min(floor(float64(max_dist) / float64(f32 resolution) 64),
    2^31 - 1)."""
    if max_dist is None:
        return TRAVEL_MAX_LIMIT
    return int(min(math.floor(float(max_dist) / float(np.float32(resolution)) * 64.0), TRAVEL_MAX_LIMIT))


def travel_traversable_ref(field, need2, state=None):
    """The traversable set T (nx,ny,nz) bool: field >= need2 and, where state is given, state == 1 — field_nodes_ref at stride 1."""
    return field_nodes_ref(field, need2, 1, state)


def _travel_shift(a, d, fill):
    """out[v] = a[v + d] where v + d lies inside, else fill."""
    out = np.full_like(a, fill)
    src, dst = [], []
    for n, k in zip(a.shape, d):
        src.append(slice(max(k, 0), n + min(k, 0)))
        dst.append(slice(max(-k, 0), n + min(-k, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def travel_allowed_ref(T):
    """{move m: (nx,ny,nz) bool} for the 26 moves: the move from v is allowed iff every voxel of the box spanned by v and v + d is in
    T (2, 4 or 8 voxels) — no corner is cut."""
    T = np.asarray(T, dtype=bool)
    out = {}
    for m, (dx, dy, dz) in enumerate(TRAVEL_MOVES):
        if m == 13:
            continue
        ok = T.copy()
        for ex in {0, dx}:
            for ey in {0, dy}:
                for ez in {0, dz}:
                    ok &= _travel_shift(T, (ex, ey, ez), False)
        out[m] = ok
    return out


def travel_seeds_ref(sources, origin, resolution, T):
    """(S,3) source positions -> (seeded (S,) uint8, voxels (S,3) int64): seeded iff the position is in range, its voxel lies
    inside dims and in T; there is no snapping."""
    T = np.asarray(T, dtype=bool)
    q, ok = occ_fixed(sources, origin, resolution)
    v = q >> 8
    inside = ok & ((v >= 0) & (v < np.asarray(T.shape)[None, :])).all(axis=1)
    seeded = np.zeros(len(v), dtype=np.uint8)
    seeded[inside] = T[v[inside, 0], v[inside, 1], v[inside, 2]]
    return seeded, v


def travel_ref(T, seeds, limit=TRAVEL_MAX_LIMIT):
    """The travel field (nx,ny,nz) int64 by Bellman-Ford: cost 0 at the voxels `seeds` (K,3) that lie in T, then sweeps of 26 shifted
    minima under the move masks until nothing changes; a value above limit is never stored (a prefix of a shortest path is shorter:
    what is stored is the untruncated distance).  -1 = unreachable."""
    T = np.asarray(T, dtype=bool)
    big = np.int64(1) << 40
    cost = np.full(T.shape, big, dtype=np.int64)
    for x, y, z in np.asarray(seeds, dtype=np.int64).reshape(-1, 3):
        if 0 <= x < T.shape[0] and 0 <= y < T.shape[1] and 0 <= z < T.shape[2] and T[x, y, z]:
            cost[x, y, z] = 0
    allowed = travel_allowed_ref(T)
    weights = {m: TRAVEL_WEIGHTS[sum(1 for k in d if k) - 1] for m, d in enumerate(TRAVEL_MOVES) if m != 13}
    while True:
        before = cost.copy()
        for m, ok in allowed.items():
            cand = _travel_shift(cost, TRAVEL_MOVES[m], big) + weights[m]
            cost = np.where(ok & (cand <= limit) & (cand < cost), cand, cost)
        if np.array_equal(cost, before):
            break
    return np.where(cost <= limit, cost, -1).astype(np.int64)


def travel_metres(cost, resolution):
    """cost codes (any shape) -> f32 metres: fl(fl((float) cost / 64) r); +inf for -1, NaN for -2."""
    c = np.asarray(cost, dtype=np.int64)
    m = ((np.maximum(c, 0).astype(np.float32) * np.float32(1.0 / 64.0)).astype(np.float32) * np.float32(resolution)).astype(np.float32)
    m = np.where(c == -1, np.float32(np.inf), m)
    return np.where(c == -2, np.float32(np.nan), m).astype(np.float32)


def travel_positions_ref(positions, origin, resolution, cost):
    """(M,3) world positions -> (M,) int64: the voxel's cost, -1 unreachable, -2 out of range or outside dims."""
    cost = np.asarray(cost, dtype=np.int64)
    q, ok = occ_fixed(positions, origin, resolution)
    v = q >> 8
    inside = ok & ((v >= 0) & (v < np.asarray(cost.shape)[None, :])).all(axis=1)
    out = np.full(len(v), -2, dtype=np.int64)
    out[inside] = cost[v[inside, 0], v[inside, 1], v[inside, 2]]
    return out


def travel_paths_ref(goals, origin, resolution, cost, T):
    """One path per goal position, by the path rule -> a list of (L,3) f32 arrays of voxel centres from the goal's voxel to its
    source (L = 0: the goal is unreachable, out of range or outside dims): the predecessor of v is the allowed neighbour u with
    cost[u] + w == cost[v], the lowest move number on ties."""
    cost, T = np.asarray(cost, dtype=np.int64), np.asarray(T, dtype=bool)
    f32 = np.float32
    o, r = np.asarray(origin, dtype=f32).reshape(3), f32(resolution)
    codes = travel_positions_ref(goals, origin, resolution, cost)
    q, _ = occ_fixed(goals, origin, resolution)
    inside = lambda p: all(0 <= p[a] < T.shape[a] for a in range(3))   # noqa: E731
    out = []
    for e, code in enumerate(codes):
        rows = []
        if code >= 0:
            v = tuple(int(k) for k in q[e] >> 8)
            while True:
                rows.append((o + ((np.asarray(v, dtype=f32) + f32(0.5)).astype(f32) * r).astype(f32)).astype(f32))
                if cost[v] == 0:
                    break
                for m, d in enumerate(TRAVEL_MOVES):
                    u = (v[0] + d[0], v[1] + d[1], v[2] + d[2])
                    if m == 13 or not inside(u) or cost[u] < 0:
                        continue
                    w = TRAVEL_WEIGHTS[sum(1 for k in d if k) - 1]
                    box = [(v[0] + ex, v[1] + ey, v[2] + ez) for ex in {0, d[0]} for ey in {0, d[1]} for ez in {0, d[2]}]
                    if cost[u] + w == cost[v] and all(T[b] for b in box):
                        v = u
                        break
                else:
                    raise AssertionError(f"no predecessor at {v}: not a travel field")
        out.append(np.asarray(rows, dtype=f32).reshape(-1, 3))
    return out


# ---- weighted travel fields ("Weighted travel fields"): a layer kappa (nx,ny,nz) of factors in [16, 255], 16 neutral.
TRAVEL_KAPPA_NEUTRAL, TRAVEL_KAPPA_MAX = 16, 255
TRAVEL_MAX_STEP = (111 * 2 * TRAVEL_KAPPA_MAX + 16) >> 5   # 1769


def travel_step(w, ka, kb):
    """The weighted cost of a move of weight w (64, 91 or 111) between voxels of factors ka and kb: (w (ka + kb) + 16) >> 5 —
    symmetric, an integer, >= w for factors >= 16 and exactly w at 16.  Integers or int64 arrays."""
    return (w * (ka + kb) + 16) >> 5


def travel_weighted_ref(T, seeds, kappa, limit=TRAVEL_MAX_LIMIT):
    """travel_ref with the layer kappa (nx,ny,nz): the move m from u to v costs travel_step(w_m, kappa[u], kappa[v]).  The same
    sweeps, the same truncation, -1 = unreachable."""
    T = np.asarray(T, dtype=bool)
    kappa = np.asarray(kappa, dtype=np.int64)
    assert kappa.shape == T.shape and kappa.min(initial=TRAVEL_KAPPA_NEUTRAL) >= TRAVEL_KAPPA_NEUTRAL and \
        kappa.max(initial=TRAVEL_KAPPA_NEUTRAL) <= TRAVEL_KAPPA_MAX
    big = np.int64(1) << 40
    cost = np.full(T.shape, big, dtype=np.int64)
    for x, y, z in np.asarray(seeds, dtype=np.int64).reshape(-1, 3):
        if 0 <= x < T.shape[0] and 0 <= y < T.shape[1] and 0 <= z < T.shape[2] and T[x, y, z]:
            cost[x, y, z] = 0
    allowed = travel_allowed_ref(T)
    steps = {m: travel_step(TRAVEL_WEIGHTS[sum(1 for k in d if k) - 1], kappa, _travel_shift(kappa, d, TRAVEL_KAPPA_NEUTRAL))
             for m, d in enumerate(TRAVEL_MOVES) if m != 13}
    while True:
        before = cost.copy()
        for m, ok in allowed.items():
            cand = _travel_shift(cost, TRAVEL_MOVES[m], big) + steps[m]
            cost = np.where(ok & (cand <= limit) & (cand < cost), cand, cost)
        if np.array_equal(cost, before):
            break
    return np.where(cost <= limit, cost, -1).astype(np.int64)


def travel_weighted_paths_ref(goals, origin, resolution, cost, T, kappa):
    """travel_paths_ref under the layer kappa: the predecessor of v is the allowed neighbour u with cost[u] + travel_step(w, kappa[v],
    kappa[u]) == cost[v], the lowest move number on ties."""
    cost, T, kappa = np.asarray(cost, dtype=np.int64), np.asarray(T, dtype=bool), np.asarray(kappa, dtype=np.int64)
    f32 = np.float32
    o, r = np.asarray(origin, dtype=f32).reshape(3), f32(resolution)
    codes = travel_positions_ref(goals, origin, resolution, cost)
    q, _ = occ_fixed(goals, origin, resolution)
    inside = lambda p: all(0 <= p[a] < T.shape[a] for a in range(3))   # noqa: E731
    out = []
    for e, code in enumerate(codes):
        rows = []
        if code >= 0:
            v = tuple(int(k) for k in q[e] >> 8)
            while True:
                rows.append((o + ((np.asarray(v, dtype=f32) + f32(0.5)).astype(f32) * r).astype(f32)).astype(f32))
                if cost[v] == 0:
                    break
                for m, d in enumerate(TRAVEL_MOVES):
                    u = (v[0] + d[0], v[1] + d[1], v[2] + d[2])
                    if m == 13 or not inside(u) or cost[u] < 0:
                        continue
                    step = travel_step(TRAVEL_WEIGHTS[sum(1 for k in d if k) - 1], int(kappa[v]), int(kappa[u]))
                    box = [(v[0] + ex, v[1] + ey, v[2] + ez) for ex in {0, d[0]} for ey in {0, d[1]} for ez in {0, d[2]}]
                    if cost[u] + step == cost[v] and all(T[b] for b in box):
                        v = u
                        break
                else:
                    raise AssertionError(f"no predecessor at {v}: not a weighted travel field")
        out.append(np.asarray(rows, dtype=f32).reshape(-1, 3))
    return out


def travel_weights_lut(radius, soft_radius, resolution, D, gain=4.0):
    """The default table of tools.travel_weights -> (D^2 + 1,) uint8, indexed by the clearance field's squared gap d2 in voxels:
    kappa(d2) = 16 + 16 gain max(0, (soft - g) / (soft - radius))^2 with g = sqrt(d2) f64(f32 resolution), computed in float64, then
    np.rint and clipped to [16, 255].  Neutral at and beyond soft_radius, steepest at radius."""
    d2 = np.arange(int(D) * int(D) + 1, dtype=np.float64)
    g = np.sqrt(d2) * float(np.float32(resolution))
    t = np.maximum(0.0, (float(soft_radius) - g) / (float(soft_radius) - float(radius)))
    return np.clip(np.rint(16.0 + 16.0 * float(gain) * t * t), TRAVEL_KAPPA_NEUTRAL, TRAVEL_KAPPA_MAX).astype(np.uint8)


def travel_weights_ref(field, lut, state=None, unknown_add=0):
    """k_travel_weights restated: kappa[v] = lut[min(field[v], len(lut) - 1)] over a clearance field (nx,ny,nz); where `state`
    (state_ref's codes per voxel: 0 unknown, 1 free, 2 occupied) is given, + unknown_add at the unknown voxels, saturating at 255.
    -> (nx,ny,nz) uint8."""
    lut = np.asarray(lut, dtype=np.int64).reshape(-1)
    k = lut[np.minimum(np.asarray(field, dtype=np.int64), len(lut) - 1)]
    if state is not None:
        k = np.where(np.asarray(state) == 0, np.minimum(k + int(unknown_add), TRAVEL_KAPPA_MAX), k)
    return k.astype(np.uint8)


def travel_weight_fixed(travel_weight, resolution):
    """select_views_volume's travel_weight (revealed voxels per metre travelled) -> the pick's integer m = round(travel_weight r 2^20 /
    64): gain 2^20 - m cost is then gain - travel_weight metres, in units of 2^-20 voxel."""
    return int(round(float(travel_weight) * float(np.float32(resolution)) * (1 << 20) / 64.0))


def view_pick_travel_ref(gains, taken, cost, m, min_gain=1):
    """One round of the pick that prices the trip -> the winner's index or -1 (stop): among the candidates with taken == 0, gain >=
    min_gain and cost >= 0 the largest gain 2^20 - m cost (Python integers), the lowest index on ties."""
    best, at = None, -1
    for i, (g, t, c) in enumerate(zip(np.asarray(gains).tolist(), np.asarray(taken).tolist(), np.asarray(cost).tolist())):
        if t or g < min_gain or c < 0:
            continue
        score = g * (1 << 20) - int(m) * c
        if best is None or score > best:
            best, at = score, i
    return at


TRAVEL_MAX_FIELDS = 256


def travel_batch_ref(T, seeds_per_field, limit=TRAVEL_MAX_LIMIT):
    """B travel fields over one T -> (B,nx,ny,nz) int64: field b is travel_ref from seeds_per_field[b] (a (K,3) list of voxels, K >=
    0) — a loop over the single field, which is the batch's whole definition."""
    T = np.asarray(T, dtype=bool)
    return np.stack([travel_ref(T, np.asarray(s, dtype=np.int64).reshape(-1, 3), limit) for s in seeds_per_field]).reshape((-1,) + T.shape)


def travel_matrix_ref(positions, origin, resolution, T, limit=TRAVEL_MAX_LIMIT):
    """The map-distance matrix of (M,3) positions -> (cost (M,M) int64, seeded (M,) uint8): cost[i][j] is the cost, in the field
    seeded at position i alone, of position j's voxel (travel_positions_ref's codes: -1 unreachable — a whole row where i is not
    seeded — and -2 in the columns out of range or outside dims)."""
    seeded, vox = travel_seeds_ref(positions, origin, resolution, T)
    fields = travel_batch_ref(T, [vox[i:i + 1] if seeded[i] else [] for i in range(len(vox))], limit)
    cost = np.stack([travel_positions_ref(positions, origin, resolution, f) for f in fields]) if len(vox) else np.zeros((0, 0), dtype=np.int64)
    return cost.astype(np.int64), seeded


def assign_greedy_ref(cost, min_cost=0):
    """The greedy assignment of rows to columns -> (col_of_row (R,) int32, row_of_col (C,) int32), -1 where nothing was assigned: the
    candidates are the pairs with cost[r][c] >= min_cost (>= 0: negative entries mean none); the smallest (cost, r, c) whose row is
    unassigned and whose column is unclaimed is assigned, until none is left."""
    cost = np.asarray(cost, dtype=np.int64)
    R, C = cost.shape
    col_of_row, row_of_col = np.full(R, -1, dtype=np.int32), np.full(C, -1, dtype=np.int32)
    while True:
        best = None
        for r in range(R):
            if col_of_row[r] >= 0:
                continue
            for c in range(C):
                if row_of_col[c] < 0 and cost[r, c] >= min_cost and (best is None or (int(cost[r, c]), r, c) < best):
                    best = (int(cost[r, c]), r, c)
        if best is None:
            return col_of_row, row_of_col
        col_of_row[best[1]], row_of_col[best[2]] = best[2], best[1]


def assign_min_cost_fixed(min_cost, resolution):
    """assign_frontiers' min_cost in metres -> the integer bound in 1/64 voxel edge: ceil(float64(min_cost) / float64(f32 r) 64)."""
    return int(math.ceil(float(min_cost) / float(np.float32(resolution)) * 64.0))


def tour_travel_units(cost, resolution):
    """Travel costs (1/64 voxel edge; any shape) -> the tour's unit, 2^-20 m: round_half_even(float64(cost) (float64(f32 r) 2^14)) —
    one correctly rounded f64 product (the scale by 2^14 is exact); the codes -1 and -2 become TOUR_INF."""
    c = np.asarray(cost, dtype=np.int64)
    scale = float(np.float32(resolution)) * 16384.0
    return np.where(c < 0, np.int64(TOUR_INF), np.rint(np.maximum(c, 0).astype(np.float64) * scale).astype(np.int64))


# ---- connected components restated in numpy ("Connected components"): what components_kernels.hip must give, bit for
# bit.  Dense (nx,ny,nz) arrays, the linear index of voxel (x, y, z) is v = (z ny + y) nx + x, -1 = a clear voxel. ----------------------
COMPONENT_CONNECTIVITIES = (6, 18, 26)


def components_offsets(connectivity):
    """The neighbour offsets (dx, dy, dz) of a connectivity: those that differ on 1 (6), <= 2 (18) or <= 3 (26) axes."""
    if connectivity not in COMPONENT_CONNECTIVITIES:
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for m, d in enumerate(TRAVEL_MOVES) if m != 13 and sum(1 for k in d if k) <= most]


def components_ref(plane, connectivity=26):
    """Connected components of a bool plane (nx,ny,nz) -> (ids (nx,ny,nz) int64, -1 where clear; roots (C,) int64 ascending): every
    set voxel starts with its own linear index; rounds of shifted minima over the connectivity's offsets, each followed by pointer
    jumping (a label is the index of a voxel of the same component, whose label is no larger), until nothing changes.  The root of a
    component is its lowest linear index, the id its root's rank."""
    plane = np.asarray(plane, dtype=bool)
    nx, ny, nz = plane.shape
    big = np.int64(1) << 40
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    lin = ((z * ny + y) * nx + x).astype(np.int64)
    lab = np.where(plane, lin, big)
    offsets = components_offsets(connectivity)
    order = lin[plane]                         # a set voxel's linear index, in the dense array's own order
    flat = np.full(nx * ny * nz, big, dtype=np.int64)
    while True:
        before = lab
        for d in offsets:
            lab = np.where(plane, np.minimum(lab, _travel_shift(lab, d, big)), big)
        while True:                            # label <- the label of the voxel it names
            flat[order] = lab[plane]
            nxt = flat[lab[plane]]
            if np.array_equal(nxt, lab[plane]):
                break
            lab[plane] = nxt
        if np.array_equal(lab, before):
            break
    roots = np.unique(lab[plane])
    ids = np.full(plane.shape, -1, dtype=np.int64)
    ids[plane] = np.searchsorted(roots, lab[plane])
    return ids, roots.astype(np.int64)


def components_stats_ref(ids, origin, resolution):
    """Per component of an id volume (nx,ny,nz), -1 clear -> dict(sizes (C,) int64, sums (C,3) int64 of i, j, k, bbox (C,2,3) int32
    minimum and maximum per axis, centroids (C,3) f32 = fl(origin + (sum / size + 0.5) r) computed in float64 from the f32 origin and
    resolution, then cast)."""
    ids = np.asarray(ids, dtype=np.int64)
    C = int(ids.max()) + 1 if ids.size and ids.max() >= 0 else 0
    ijk = np.argwhere(ids >= 0).astype(np.int64)
    of = ids[ids >= 0]
    sizes = np.zeros(C, dtype=np.int64)
    sums = np.zeros((C, 3), dtype=np.int64)
    bbox = np.empty((C, 2, 3), dtype=np.int32)
    bbox[:, 0], bbox[:, 1] = np.iinfo(np.int32).max, -1
    np.add.at(sizes, of, 1)
    np.add.at(sums, of, ijk)
    np.minimum.at(bbox[:, 0], of, ijk.astype(np.int32))
    np.maximum.at(bbox[:, 1], of, ijk.astype(np.int32))
    o = np.asarray(origin, dtype=np.float32).astype(np.float64).reshape(1, 3)
    r = float(np.float32(resolution))
    centroids = (o + (sums.astype(np.float64) / np.maximum(sizes, 1)[:, None].astype(np.float64) + 0.5) * r).astype(np.float32)
    return dict(sizes=sizes, sums=sums, bbox=bbox, centroids=centroids)


def components_min_ref(ids, values, sentinel=0xFFFFFFFF):
    """Per component the smallest entry of values (nx,ny,nz) that is not the sentinel, and the lowest linear index v = (z ny + y) nx +
    x among the voxels that attain it -> (value (C,) int64, voxel (C,) int64); -1 / -1 where every voxel holds the sentinel."""
    ids, values = np.asarray(ids, dtype=np.int64), np.asarray(values, dtype=np.int64)
    nx, ny, nz = ids.shape
    C = int(ids.max()) + 1 if ids.size and ids.max() >= 0 else 0
    big = np.int64(1) << 40
    value = np.full(C, big, dtype=np.int64)
    voxel = np.full(C, big, dtype=np.int64)
    ok = (ids >= 0) & (values != sentinel)
    ijk = np.argwhere(ok)
    lin = (ijk[:, 2] * ny + ijk[:, 1]) * nx + ijk[:, 0]
    of, val = ids[ok], values[ok]
    np.minimum.at(value, of, val)
    hit = val == value[of]
    np.minimum.at(voxel, of[hit], lin[hit])
    none = value == big
    return np.where(none, -1, value), np.where(none, -1, voxel)


def components_positions_ref(positions, origin, resolution, ids):
    """(M,3) world positions -> (M,) int64: the voxel's id, -1 clear, -2 out of range or outside dims."""
    return travel_positions_ref(positions, origin, resolution, ids)


def frontier_clusters_ref(sizes, cost=None, min_size=1):
    """The rows of frontier_clusters -> the component ids in row order (K,) int64: the components with size >= min_size; with cost
    (C,) int64 (-1 unreachable) the reachable ones first, by ascending cost, then descending size, then ascending id; without it by
    descending size, then ascending id."""
    sizes = [int(s) for s in np.asarray(sizes).tolist()]
    keep = [i for i, s in enumerate(sizes) if s >= min_size]
    if cost is None:
        return np.asarray(sorted(keep, key=lambda i: (-sizes[i], i)), dtype=np.int64)
    cost = [int(c) for c in np.asarray(cost).tolist()]
    return np.asarray(sorted(keep, key=lambda i: (cost[i] < 0, max(cost[i], 0), -sizes[i], i)), dtype=np.int64)


# ---- the evidence map restated in numpy ("Evidence map"): what evidence_kernels.hip must give, bit for bit.  int64
# throughout, dense (nx,ny,nz) arrays. --------------------------------------------------------------------------------------------------
EVID_UNKNOWN = -128
EVID_HEADER = 256
EVID_DEFAULTS = dict(hit=17, miss=8, lmin=-40, lmax=70, threshold=0)
EVID_SCENE = dict(origin=(-0.2, -0.2, -0.2), resolution=0.1, dims=(24, 24, 14), scanner=(0.5, 1.0, 0.5), step=0.04,
                  pillar=((1.0, 0.8, 0.0), (1.3, 1.2, 0.7)), leg=((0.5, 1.0, 0.35), (1.8, 1.0, 0.35)))


def evidence_params(params=None):
    """{hit, miss, lmin, lmax, threshold} (missing keys: EVID_DEFAULTS; None: all defaults) -> the five integers in that order."""
    p = dict(EVID_DEFAULTS, **(params or {}))
    return tuple(int(p[k]) for k in ("hit", "miss", "lmin", "lmax", "threshold"))


def evidence_fold_ref(L, H, M, params=None):
    """One scan folded into the values L (nx,ny,nz) integers (-128: never observed; not modified) -> (L' int64, counts (4,) int64).  H,
    M: the scan's hit and pass planes (nx,ny,nz) bool.  base = (L == -128 ? 0 : L); with the H bit L' = min(base + hit, lmax);
    otherwise with the M bit L' = max(base - miss, lmin); otherwise L' = L.  counts: voxels updated, voxels newly known (they left
    -128), occupied (L > threshold) voxels that appeared, occupied voxels that vanished."""
    hit, miss, lmin, lmax, thr = evidence_params(params)
    L = np.asarray(L, dtype=np.int64)
    H, M = np.asarray(H, dtype=bool), np.asarray(M, dtype=bool)
    base = np.where(L == EVID_UNKNOWN, 0, L)
    out = np.where(H, np.minimum(base + hit, lmax), np.where(M, np.maximum(base - miss, lmin), L))
    touched = H | M
    counts = np.array([touched.sum(), (touched & (L == EVID_UNKNOWN)).sum(), ((out > thr) & ~(L > thr)).sum(), ((L > thr) & ~(out > thr)).sum()],
                      dtype=np.int64)
    return out, counts


def evidence_planes_ref(L, threshold=0):
    """The derived planes of the values L -> (occupied, free) (nx,ny,nz) bool: L > threshold; L != -128 and L <= threshold."""
    L = np.asarray(L, dtype=np.int64)
    return L > int(threshold), (L != EVID_UNKNOWN) & (L <= int(threshold))


def _evidence_bricks(dims):
    nx, ny, nz = (int(d) for d in dims)
    return (nx + 3) // 4, (ny + 3) // 4, (nz + 1) // 2


def evidence_brick_order(L):
    """The byte image of the evidence buffer holding the values L (nx,ny,nz) -> (256 + 32 words,) uint8: a zero header, then the int8
    value of voxel (x, y, z) at byte 32 w + b, w = ((z >> 1) nby + (y >> 2)) nbx + (x >> 2), b = x & 3 | (y & 3) << 2 | (z & 1) << 4;
    the pad voxels (outside dims) hold -128."""
    L = np.asarray(L, dtype=np.int64)
    nx, ny, nz = L.shape
    nbx, nby, nbz = _evidence_bricks(L.shape)
    pad = np.full((4 * nbx, 4 * nby, 2 * nbz), EVID_UNKNOWN, dtype=np.int64)
    pad[:nx, :ny, :nz] = L
    # (bx, x&3, by, y&3, bz, z&1) -> (bz, by, bx, z&1, y&3, x&3): the last three are the bit, most significant first
    img = pad.reshape(nbx, 4, nby, 4, nbz, 2).transpose(4, 2, 0, 5, 3, 1).reshape(-1)
    return np.concatenate([np.zeros(EVID_HEADER, dtype=np.uint8), img.astype(np.int8).view(np.uint8)])


def evidence_from_brick_order(image, dims):
    """The inverse of evidence_brick_order -> (values (nx,ny,nz) int64, pads: the values of the pad voxels, int64)."""
    nx, ny, nz = (int(d) for d in dims)
    nbx, nby, nbz = _evidence_bricks(dims)
    v = np.asarray(image, dtype=np.uint8)[EVID_HEADER:].view(np.int8).astype(np.int64)
    full = v.reshape(nbz, nby, nbx, 2, 4, 4).transpose(2, 5, 1, 4, 0, 3).reshape(4 * nbx, 4 * nby, 2 * nbz)
    inside = np.zeros(full.shape, dtype=bool)
    inside[:nx, :ny, :nz] = True
    return full[:nx, :ny, :nz].copy(), full[~inside]


def evidence_scan_ref(L, scanner, points, origin, resolution, dims, params=None, max_range=None):
    """EvidenceMap.integrate restated -> (L', counts, skipped, H, M): the pass plane M is carve_ref of the scan into an empty plane, the
    hit plane H is occupancy_ref of the rows whose ray was not truncated (flags != 1) into an empty grid, then one evidence_fold_ref.
    skipped: the rays carve skipped."""
    P = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    M, skipped, flags, _ = carve_ref(scanner, P, origin, resolution, dims, max_range=max_range)
    H, _ = occupancy_ref(P if max_range is None else P[flags != 1], origin, resolution, dims)
    out, counts = evidence_fold_ref(L, H, M, params)
    return out, counts, skipped, H, M


# ---- re-framing and merging maps restated in numpy ("Re-framing and merging maps"): what reframe_kernels.hip must give,
# bit for bit.  Slices of dense (nx,ny,nz) arrays. -----------------------------------------------------------------------------------
def shifted_window(src, dst_dims, shift, empty):
    """The source values of a destination box -> an array of shape dst_dims: voxel v holds src[v + shift] where v + shift lies inside
    src's shape, `empty` elsewhere."""
    src = np.asarray(src)
    out = np.full(tuple(int(d) for d in dst_dims), empty, dtype=src.dtype)
    to, frm = [], []
    for nd, ns, s in zip(out.shape, src.shape, (int(v) for v in shift)):
        lo, hi = max(0, -s), min(nd, ns - s)   # 0 <= v < nd and 0 <= v + s < ns
        if hi <= lo:
            return out
        to.append(slice(lo, hi))
        frm.append(slice(lo + s, hi + s))
    out[tuple(to)] = src[tuple(frm)]
    return out


def occ_transfer_ref(bits, dst_bits, shift, mode):
    """tohip_occ_transfer restated -> (new (dst's shape) bool, count).  bits: the source plane, dst_bits: the destination before (not
    modified; only its shape matters to 'copy'), shift: three integers — destination voxel v takes source voxel v + shift.  mode
    'copy': new = the source bits, count = the bits set afterwards; 'or': new = dst | source, count = the bits that were not set."""
    dst = np.asarray(dst_bits, dtype=bool)
    S = shifted_window(np.asarray(bits, dtype=bool), dst.shape, shift, False)
    if mode == "copy":
        return S, int(S.sum())
    if mode != "or":
        raise ValueError(f"mode must be 'copy' or 'or', got {mode!r}")
    return dst | S, int((S & ~dst).sum())


def evidence_combine_ref(S, L_dst, mode, params=None):
    """The transfer and resample entries' combine of sampled source values S with the destination's D = L_dst (not modified) -> (L'
    int64, counts (4,) int64).  'copy': L' = S, counted against an empty destination.  'add': S == -128 leaves D, else clamp((D == -128
    ? 0 : D) + S, lmin, lmax).  'confident': the larger of D and clamp(S) under the key (|L|, L), -128 below everything.  counts:
    values that changed, voxels newly known, occupied (L > threshold) voxels that appeared, that vanished."""
    _, _, lmin, lmax, thr = evidence_params(params)
    D = np.asarray(L_dst, dtype=np.int64)
    known = S != EVID_UNKNOWN
    if mode == "copy":
        D, out = np.full(D.shape, EVID_UNKNOWN, dtype=np.int64), S
    elif mode == "add":
        out = np.where(known, np.clip(np.where(D == EVID_UNKNOWN, 0, D) + S, lmin, lmax), D)
    elif mode == "confident":
        C = np.where(known, np.clip(S, lmin, lmax), EVID_UNKNOWN)
        key = lambda L: np.where(L == EVID_UNKNOWN, -1, 2 * np.abs(L) + (L > 0))   # noqa: E731
        out = np.where(key(C) > key(D), C, D)
    else:
        raise ValueError(f"mode must be 'copy', 'add' or 'confident', got {mode!r}")
    counts = np.array([(out != D).sum(), ((D == EVID_UNKNOWN) & (out != EVID_UNKNOWN)).sum(), ((out > thr) & ~(D > thr)).sum(),
                       ((D > thr) & ~(out > thr)).sum()], dtype=np.int64)
    return out, counts


def evidence_transfer_ref(L_src, L_dst, shift, mode, params=None):
    """tohip_evid_transfer restated -> (L' (dst's shape) int64, counts (4,) int64).  S = the source values (-128 outside the source), D
    = L_dst (not modified).  'copy': L' = S, counted against an empty destination.  'add': S == -128 leaves D, else clamp((D == -128 ?
    0 : D) + S, lmin, lmax).  'confident': the larger of D and clamp(S) under the key (|L|, L), -128 below everything.  counts: values
    that changed, voxels newly known, occupied (L > threshold) voxels that appeared, that vanished."""
    S = shifted_window(np.asarray(L_src, dtype=np.int64), np.shape(L_dst), shift, EVID_UNKNOWN)
    return evidence_combine_ref(S, L_dst, mode, params)


# ---- resampling maps restated in numpy ("Resampling maps"): what resample_kernels.hip must give, bit for bit, from the
# same twelve integers (ops.resample_affine).  Dense (nx,ny,nz) arrays, int64 throughout. ---------------------------------------------
RESAMPLE_FRAC_BITS = 20
RESAMPLE_MAX_M, RESAMPLE_MAX_T = 1 << 21, 1 << 40
RESAMPLE_EVID_RULES = ("nearest", "cover")
RESAMPLE_OCC_RULES = ("nearest", "any", "all")


def resample_nearest(affine, dst_dims):
    """The twelve integers (M row major, then T) -> n (3, nx, ny, nz) int64, the nearest source voxel of every voxel of dst_dims: u_a =
    M[a][0] (2 i + 1) + M[a][1] (2 j + 1) + M[a][2] (2 k + 1) + T[a], n_a = u_a >> 20 (numpy's >> of a negative int64 is arithmetic)."""
    a = np.asarray(affine, dtype=np.int64).reshape(12)
    if (np.abs(a[:9]) > RESAMPLE_MAX_M).any() or (np.abs(a[9:]) > RESAMPLE_MAX_T).any():
        raise ValueError("the affine map exceeds |M| <= 2^21, |T| <= 2^40")
    M, T = a[:9].reshape(3, 3), a[9:]
    i, j, k = np.ix_(*(2 * np.arange(int(d), dtype=np.int64) + 1 for d in dst_dims))   # (open grids: the sums broadcast)
    return np.stack([(M[r, 0] * i + M[r, 1] * j + M[r, 2] * k + T[r]) >> RESAMPLE_FRAC_BITS for r in range(3)])


def _resample_take(src, n, empty):
    """src at the voxels n (3, ...) where they lie inside src's shape, `empty` elsewhere."""
    inside = np.ones(n.shape[1:], dtype=bool)
    for a in range(3):
        inside &= (n[a] >= 0) & (n[a] < src.shape[a])
    c = [np.clip(n[a], 0, src.shape[a] - 1) for a in range(3)]
    return np.where(inside, src[c[0], c[1], c[2]], empty)


_RESAMPLE_TAPS = [np.array((dx, dy, dz), dtype=np.int64).reshape(3, 1, 1, 1) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def evid_sample_ref(L_src, affine, dst_dims, rule="nearest", threshold=0):
    """The sampled source values S (dst_dims, int64).  'nearest': the value of n, -128 outside the source.  'cover': the maximum over
    the 27 source voxels around n of the key free < unknown < occupied — 128 + L for L <= threshold, 256 for -128 and outside the
    source, 640 + L above the threshold — decoded again."""
    L = np.asarray(L_src, dtype=np.int64)
    n = resample_nearest(affine, dst_dims)
    if rule == "nearest":
        return _resample_take(L, n, EVID_UNKNOWN)
    if rule != "cover":
        raise ValueError(f"rule must be 'nearest' or 'cover', got {rule!r}")
    key = np.where(L == EVID_UNKNOWN, 256, np.where(L > threshold, 640 + L, 128 + L))
    best = np.zeros(n.shape[1:], dtype=np.int64)
    for tap in _RESAMPLE_TAPS:
        best = np.maximum(best, _resample_take(key, n + tap, 256))
    return np.where(best > 512, best - 640, np.where(best == 256, EVID_UNKNOWN, best - 128))


def evid_resample_ref(L_src, L_dst, affine, rule, mode, params=None):
    """tohip_evid_resample restated -> (L' (dst's shape) int64, counts (4,) int64): evid_sample_ref's S under the parameters'
    threshold, combined with L_dst (not modified) as the transfer does (evidence_combine_ref)."""
    S = evid_sample_ref(L_src, affine, np.shape(L_dst), rule, evidence_params(params)[4])
    return evidence_combine_ref(S, L_dst, mode, params)


def occ_resample_ref(bits, dst_bits, affine, rule, mode):
    """tohip_occ_resample restated -> (new (dst's shape) bool, count).  rule 'nearest': the bit of n; 'any': the OR of the 27 bits
    around n; 'all': their AND, a voxel outside the source counting 0.  mode 'copy' / 'or' and the count as occ_transfer_ref."""
    src, dst = np.asarray(bits, dtype=bool), np.asarray(dst_bits, dtype=bool)
    n = resample_nearest(affine, dst.shape)
    if rule == "nearest":
        S = _resample_take(src, n, False)
    elif rule in ("any", "all"):
        S = np.full(dst.shape, rule == "all")
        for tap in _RESAMPLE_TAPS:
            t = _resample_take(src, n + tap, False)
            S = (S | t) if rule == "any" else (S & t)
    else:
        raise ValueError(f"rule must be 'nearest', 'any' or 'all', got {rule!r}")
    if mode == "copy":
        return S, int(S.sum())
    if mode != "or":
        raise ValueError(f"mode must be 'copy' or 'or', got {mode!r}")
    return dst | S, int((S & ~dst).sum())


# ---- coarsening maps restated in numpy ("Coarsening maps"): what coarsen_kernels.hip must give, bit for bit, from the
# factor and the integer offset (ops.coarsen_offset).  Dense (nx,ny,nz) arrays, int64 throughout. -------------------------------------
COARSEN_MAX_FACTOR = 8
COARSEN_MAX_OFFSET = 1 << 20
COARSEN_EVID_RULES = ("cover", "max")
COARSEN_OCC_RULES = ("any", "all")


def coarsen_children(src, dst_dims, factor, offset, empty):
    """The children of every voxel of dst_dims -> (nx, ny, nz, f^3): those of d are src[f d + offset + e], e in [0, f)^3, `empty`
    where that lies outside src's shape."""
    f = int(factor)
    if not 2 <= f <= COARSEN_MAX_FACTOR or any(abs(int(o)) > COARSEN_MAX_OFFSET for o in offset):
        raise ValueError(f"factor must lie in [2, {COARSEN_MAX_FACTOR}] and the offset within 2^20, got {factor!r} and {tuple(offset)!r}")
    d = tuple(int(n) for n in dst_dims)
    win = shifted_window(src, tuple(f * n for n in d), offset, empty)
    return win.reshape(d[0], f, d[1], f, d[2], f).transpose(0, 2, 4, 1, 3, 5).reshape(*d, f ** 3)


def evid_coarsen_sample_ref(L_src, dst_dims, factor, offset, rule="cover", threshold=0):
    """The source values S (dst_dims, int64) of the coarse voxels.  'cover': the maximum over the f^3 children of evid_sample_ref's key
    free < unknown < occupied (a child outside the source is unknown), decoded again.  'max': the largest child as a signed byte."""
    C = coarsen_children(np.asarray(L_src, dtype=np.int64), dst_dims, factor, offset, EVID_UNKNOWN)
    if rule == "max":
        return C.max(axis=-1)
    if rule != "cover":
        raise ValueError(f"rule must be 'cover' or 'max', got {rule!r}")
    best = np.where(C == EVID_UNKNOWN, 256, np.where(C > threshold, 640 + C, 128 + C)).max(axis=-1)
    return np.where(best > 512, best - 640, np.where(best == 256, EVID_UNKNOWN, best - 128))


def evid_coarsen_ref(L_src, L_dst, factor, offset, rule, mode, params=None):
    """tohip_evid_coarsen restated -> (L' (dst's shape) int64, counts (4,) int64): evid_coarsen_sample_ref's S under the parameters'
    threshold, combined with L_dst (not modified) as the transfer does (evidence_combine_ref)."""
    S = evid_coarsen_sample_ref(L_src, np.shape(L_dst), factor, offset, rule, evidence_params(params)[4])
    return evidence_combine_ref(S, L_dst, mode, params)


def occ_coarsen_ref(bits, dst_bits, factor, offset, rule, mode, veto=None):
    """tohip_occ_coarsen restated -> (new (dst's shape) bool, count).  rule 'any': the OR of the f^3 child bits, and with a veto plane
    (the source's shape; 'any' only) that OR and not the OR of the veto's children; 'all': their AND, a child outside the source
    counting 0.  mode 'copy' / 'or' and the count as occ_transfer_ref."""
    src, dst = np.asarray(bits, dtype=bool), np.asarray(dst_bits, dtype=bool)
    if rule not in COARSEN_OCC_RULES:
        raise ValueError(f"rule must be 'any' or 'all', got {rule!r}")
    C = coarsen_children(src, dst.shape, factor, offset, False)
    S = C.any(axis=-1) if rule == "any" else C.all(axis=-1)
    if veto is not None:
        if rule != "any" or np.shape(veto) != src.shape:
            raise ValueError("a veto plane goes with rule 'any' and has the source's shape")
        S = S & ~coarsen_children(np.asarray(veto, dtype=bool), dst.shape, factor, offset, False).any(axis=-1)
    if mode == "copy":
        return S, int(S.sum())
    if mode != "or":
        raise ValueError(f"mode must be 'copy' or 'or', got {mode!r}")
    return dst | S, int((S & ~dst).sum())


def pillar_scan(room, origin, lo, hi):
    """The scan `room` (N,3) taken from `origin` with the axis-aligned box [lo, hi] in the way -> (N,3) f32: a ray origin -> room[i]
    that enters the box (the slab method in f64; the origin lies outside it) returns its entry point instead."""
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    P = np.asarray(room, dtype=np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    d = P - o
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    par = d == 0   # a ray parallel to a slab: inside it for every t, or never
    inside = (o >= lo) & (o <= hi)
    near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    t_in, t_out = near.max(axis=1), far.min(axis=1)
    meets = (t_in <= t_out) & (t_in > 0.0) & (t_in < 1.0)
    return np.where(meets[:, None], o + np.where(meets, t_in, 0.0)[:, None] * d, P).astype(np.float32)


# ---- the ground layer ("Ground layer") -------------------------------------------------------------------------------
GROUND_MAX_HEADROOM = 64
GROUND_MAX_STEP = 4
GROUND_MAX_DROP = 2048
GROUND_UNKNOWN = FIELD_UNKNOWN


def ground_headroom_voxels(headroom, resolution):
    """headroom in metres -> H in voxels: ceil(float64(headroom) / float64(f32 resolution)), field_max_dist_voxels' rule."""
    return field_max_dist_voxels(headroom, resolution)


def _ground_up(a, k, fill):
    """out[x, y, z] = a[x, y, z + k] where z + k lies inside, else fill."""
    out = np.full_like(a, fill)
    n = a.shape[2]
    if abs(k) < n:
        out[:, :, max(-k, 0):n + min(-k, 0)] = a[:, :, max(k, 0):n + min(k, 0)]
    return out


def ground_ref(occ, free=None, headroom=4, step=1, unknown="free"):
    """The ground layer of a map -> {support, ground, floor, obstacles, drive}, five (nx,ny,nz) bool arrays, from the five rules.
    clear: not occupied (and, with unknown='obstacle', known free; outside dims clear under 'free' only).  support: occupied with H
    clear voxels above.  ground: a support voxel whose eight lateral neighbour columns lie inside dims and hold either a support
    voxel within +-step levels or an occupied voxel in the H levels above (a wall).  floor: the ground voxels and what is stacked
    solid under them.  obstacles: occupied and not floor (and, with 'obstacle', every unknown voxel).  drive: the non-occupied
    voxels with a ground voxel 1 .. step + 1 levels below."""
    occ = np.asarray(occ, dtype=bool)
    H, s = int(headroom), int(step)
    if unknown not in GROUND_UNKNOWN:
        raise ValueError(f"unknown must be 'free' or 'obstacle', got {unknown!r}")
    if unknown == "obstacle" and free is None:
        raise ValueError("unknown='obstacle' needs the free plane")
    if not 1 <= H <= GROUND_MAX_HEADROOM or not 0 <= s <= GROUND_MAX_STEP or s + 1 > H:
        raise ValueError(f"headroom must lie in [1, {GROUND_MAX_HEADROOM}] and step in [0, min({GROUND_MAX_STEP}, headroom - 1)], got {H}, {s}")
    known = unknown == "obstacle"
    clear = ~occ & np.asarray(free, dtype=bool) if known else ~occ
    support = occ.copy()
    for k in range(1, H + 1):
        support &= _ground_up(clear, k, not known)
    near = np.zeros_like(occ)    # a support voxel of this column within +-step levels
    for k in range(-s, s + 1):
        near |= _ground_up(support, k, False)
    wall = np.zeros_like(occ)    # an occupied voxel of this column in the H levels above
    for k in range(1, H + 1):
        wall |= _ground_up(occ, k, False)
    fine = near | wall
    ground = support.copy()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            if dx or dy:
                ground &= _travel_shift(fine, (dx, dy, 0), False)
    floor = np.zeros_like(occ)
    for z in range(occ.shape[2] - 1, -1, -1):
        above = floor[:, :, z + 1] if z + 1 < occ.shape[2] else False
        floor[:, :, z] = occ[:, :, z] & (ground[:, :, z] | above)
    obstacles = occ & ~floor
    if known:
        obstacles |= ~occ & ~np.asarray(free, dtype=bool)
    drive = np.zeros_like(occ)
    for k in range(1, s + 2):
        drive |= _ground_up(ground, -k, False)
    drive &= ~occ
    return {"support": support, "ground": ground, "floor": floor, "obstacles": obstacles, "drive": drive}


def ground_snap_ref(positions, origin, resolution, ground, drive, max_drop):
    """(M,3) positions -> (standing (M,3) f32, drop (M,) int32): from the position's voxel (x, y, z) down, the first k in 0 .. max_drop
    with drive[x, y, z - k] and ground[x, y, z - k - 1]; standing is that voxel's centre fl(origin + fl(fl(i + 0.5) r)), drop is k.
    -1: no such voxel; -2: out of range or outside dims; standing is NaN for both."""
    ground, drive = np.asarray(ground, dtype=bool), np.asarray(drive, dtype=bool)
    f32 = np.float32
    o, r = np.asarray(origin, dtype=f32).reshape(3), f32(resolution)
    q, ok = occ_fixed(positions, origin, resolution)
    v = q >> 8
    inside = ok & ((v >= 0) & (v < np.asarray(ground.shape)[None, :])).all(axis=1)
    standing = np.full((len(v), 3), np.nan, dtype=f32)
    drop = np.where(inside, -1, -2).astype(np.int32)
    for i in np.flatnonzero(inside):
        x, y, z = (int(c) for c in v[i])
        for k in range(0, int(max_drop) + 1):
            zz = z - k
            if zz < 1:
                break
            if drive[x, y, zz] and ground[x, y, zz - 1]:
                at = np.asarray((x, y, zz), dtype=f32)
                standing[i] = (o + ((at + f32(0.5)).astype(f32) * r).astype(f32)).astype(f32)
                drop[i] = k
                break
    return standing, drop


def ground_pack(bits):
    """A dense (nx,ny,nz) bool array -> the brick words (uint32, x fastest over the bricks) an occupancy plane holds after its
    header: a word is 4 x 4 x 2 voxels, bit x&3 | (y&3)<<2 | (z&1)<<4; pad bits 0."""
    bits = np.asarray(bits, dtype=bool)
    nx, ny, nz = bits.shape
    nbx, nby, nbz = (nx + 3) // 4, (ny + 3) // 4, (nz + 1) // 2
    pad = np.zeros((4 * nbx, 4 * nby, 2 * nbz), dtype=np.uint32)
    pad[:nx, :ny, :nz] = bits
    b = pad.reshape(nbx, 4, nby, 4, nbz, 2)
    sh = (np.arange(4)[:, None, None] + 4 * np.arange(4)[None, :, None] + 16 * np.arange(2)[None, None, :]).astype(np.uint32)
    words = (b << sh[None, :, None, :, None, :]).sum(axis=(1, 3, 5), dtype=np.uint64).astype(np.uint32)   # (nbx, nby, nbz)
    return np.ascontiguousarray(words.transpose(2, 1, 0)).reshape(-1)


# ---- scan matching restated in numpy ("Scan matching"): what scanmatch_kernels.hip must give, bit for bit -----------
SCAN_MAX_WINDOW = (16, 16, 4)
SCAN_MAX_ROTATIONS = 256
SCAN_MAX_POINTS = 1 << 22
SCAN_MAX_CANDIDATES = 1 << 22


def scan_rotation(quat):
    """A quaternion (4,) wxyz -> R (3,3) f32: normalised in f64, the rotation matrix of p -> q p conj(q) in f64, rounded once."""
    q = np.asarray(quat, dtype=np.float64).reshape(4)
    w, x, y, z = q / np.sqrt((q * q).sum())
    R = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                  [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                  [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]], dtype=np.float64)
    return R.astype(np.float32)


def scan_voxels_ref(points, R, t, origin, resolution):
    """Sensor-frame points (N,3) under the pose (R (3,3), t (3,)) -> (voxel (N,3) int64, ok (N,) bool): per axis a the world coordinate
    fl(fl(fl(fl(R_a0 p_x) + fl(R_a1 p_y)) + fl(R_a2 p_z)) + t_a) in f32, then occ_fixed's rule and q >> 8.  ok: in range on every axis
    (false for NaN and inf): the points that take part."""
    f32 = np.float32
    P = np.asarray(points, dtype=f32).reshape(-1, 3)
    R, t = np.asarray(R, dtype=f32).reshape(3, 3), np.asarray(t, dtype=f32).reshape(3)
    with np.errstate(all="ignore"):
        cols = []
        for a in range(3):
            s = ((R[a, 0] * P[:, 0]).astype(f32) + (R[a, 1] * P[:, 1]).astype(f32)).astype(f32)
            s = (s + (R[a, 2] * P[:, 2]).astype(f32)).astype(f32)
            cols.append((s + t[a]).astype(f32))
        W = np.stack(cols, axis=1)
    q, ok = occ_fixed(W, origin, resolution)
    return q >> 8, ok


def scan_values_ref(L, floor=None, unknown_value=0):
    """The value volume of the log-odds L (nx,ny,nz): max(L, floor) where L != -128 (floor None or -127: no floor), unknown_value where
    it is -128 -> int64."""
    L = np.asarray(L, dtype=np.int64)
    fl = -127 if floor is None else int(floor)
    if not -127 <= fl <= 0 or not -127 <= int(unknown_value) <= 0:
        raise ValueError(f"floor and unknown_value must lie in [-127, 0], got {floor!r}, {unknown_value!r}")
    return np.where(L == EVID_UNKNOWN, int(unknown_value), np.maximum(L, fl))


def scan_table_ref(L, floor=None, unknown_value=0):
    """The score table of the values L -> the byte image (256 + 32 words,) uint8: a zero header, then 128 + value per voxel in brick
    order, 128 + unknown_value in the pad voxels."""
    L = np.asarray(L, dtype=np.int64)
    img = evidence_brick_order(L)   # (pads -128)
    vals = scan_values_ref(img[EVID_HEADER:].view(np.int8).astype(np.int64), floor, unknown_value)
    return np.concatenate([np.zeros(EVID_HEADER, dtype=np.uint8), (vals + 128).astype(np.uint8)])


def scan_score_ref(L, origin, resolution, points, R, t, shift=(0, 0, 0), floor=None, unknown_value=0):
    """One candidate, point by point -> (score, used, inside, known): used = the points in range; inside = those whose voxel + shift
    lies inside dims; known = those with L != -128 there; score = the sum over the used points of the value of voxel + shift
    (unknown_value outside dims)."""
    L = np.asarray(L, dtype=np.int64)
    V = scan_values_ref(L, floor, unknown_value)
    v, ok = scan_voxels_ref(points, R, t, origin, resolution)
    v = v[ok] + np.asarray(shift, dtype=np.int64).reshape(1, 3)
    ins = ((v >= 0) & (v < np.asarray(L.shape)[None, :])).all(axis=1)
    vi = v[ins]
    known = L[vi[:, 0], vi[:, 1], vi[:, 2]] != EVID_UNKNOWN
    score = int(V[vi[:, 0], vi[:, 1], vi[:, 2]].sum()) + int(unknown_value) * int((~ins).sum())
    return score, int(ok.sum()), int(ins.sum()), int(known.sum())


def scan_correlate_ref(L, origin, resolution, points, Rs, t, window, floor=None, unknown_value=0, chunk=2048):
    """Every candidate of a search window -> (scores (K, 2wz+1, 2wy+1, 2wx+1) int32, used (K,) int32): rotations Rs (K,3,3), one
    translation t, shifts |dx| <= wx, |dy| <= wy, |dz| <= wz.  The value volume is padded with unknown_value by twice the window; a
    point whose base voxel lies farther than the window from dims sees unknown_value at every shift; the others read their window
    of the padded volume."""
    L = np.asarray(L, dtype=np.int64)
    w = np.asarray([int(c) for c in window], dtype=np.int64)
    if (w < 0).any() or (w > np.asarray(SCAN_MAX_WINDOW)).any():
        raise ValueError(f"window must lie in [0, {SCAN_MAX_WINDOW}] per axis, got {tuple(window)!r}")
    Rs = np.asarray(Rs, dtype=np.float32).reshape(-1, 3, 3)
    dims = np.asarray(L.shape, dtype=np.int64)
    V = scan_values_ref(L, floor, unknown_value)
    pad = np.full(tuple(dims + 4 * w), int(unknown_value), dtype=np.int64)
    pad[2 * w[0]:2 * w[0] + dims[0], 2 * w[1]:2 * w[1] + dims[1], 2 * w[2]:2 * w[2] + dims[2]] = V
    views = np.lib.stride_tricks.sliding_window_view(pad, tuple(2 * w + 1))   # [x0, y0, z0, i, j, k] = pad[x0 + i, y0 + j, z0 + k]
    scores = np.zeros((len(Rs),) + tuple(2 * w[::-1] + 1), dtype=np.int64)
    used = np.zeros(len(Rs), dtype=np.int32)
    for k, R in enumerate(Rs):
        v, ok = scan_voxels_ref(points, R, t, origin, resolution)
        v = v[ok]
        used[k] = len(v)
        near = ((v >= -w) & (v < dims + w)).all(axis=1)
        acc = np.full(tuple(2 * w + 1), int(unknown_value) * int((~near).sum()), dtype=np.int64)
        b = v[near] + w   # the window's first voxel v - w in the padded volume: v - w + 2 w
        for i in range(0, len(b), chunk):
            c = b[i:i + chunk]
            acc += views[c[:, 0], c[:, 1], c[:, 2]].sum(axis=0)
        scores[k] = acc.transpose(2, 1, 0)
    return scores.astype(np.int32), used


def scan_best_ref(scores):
    """The best candidate of scores (K, nzw, nyw, nxw) -> int32[8]: flat index, k, dx, dy, dz, score, ties, 0 under the key (score,
    then smaller dx^2 + dy^2 + dz^2, then lower flat index); ties counts the candidates whose score equals the best."""
    s = np.asarray(scores, dtype=np.int64)
    K, nzw, nyw, nxw = s.shape
    dz, dy, dx = np.meshgrid(np.arange(nzw) - nzw // 2, np.arange(nyw) - nyw // 2, np.arange(nxw) - nxw // 2, indexing="ij")
    d2 = np.broadcast_to(dx * dx + dy * dy + dz * dz, s.shape).reshape(-1)
    flat = s.reshape(-1)
    top = flat.max()
    cand = np.flatnonzero(flat == top)
    i = int(cand[np.argmin(d2[cand])])   # (argmin: the first of equals, the lower index)
    return np.array([i, i // (nzw * nyw * nxw), dx.reshape(-1)[i % dx.size], dy.reshape(-1)[i % dx.size], dz.reshape(-1)[i % dx.size], top,
                     len(cand), 0], dtype=np.int32)


# ---- relocalisation restated in numpy ("Relocalisation"): what scansearch_kernels.hip must give, bit for bit ----------
RELOC_MAX_LEVELS = 6
RELOC_MAX_WINDOW = (2048, 2048, 4)
RELOC_MAX_CAPACITY = 1 << 24
RELOC_RECORD = 11 + RELOC_MAX_LEVELS + 1   # int64 words: flat, k, dx, dy, dz, score, ties, status, incumbent, evaluated, H, nodes[0 .. 6]
RELOC_NO_INCUMBENT = -(1 << 31)            # the incumbent before the first descent (all there is with H = 0)


def scan_levels_ref(L, H, floor=None, unknown_value=0):
    """The level tables of the log-odds L (nx,ny,nz) as dense volumes -> [T_0, ..., T_H], each (nx,ny,nz) int64 of bytes: T_0 = 128 +
    value; T_h(x, y, z) = max over 0 <= i, j < 2^h of T_0'(x + i, y + j, z), T_0' being T_0 continued by 128 + unknown_value outside
    dims — built as the four-way maximum of T_{h-1} at stride 2^(h-1)."""
    if not 0 <= int(H) <= RELOC_MAX_LEVELS:
        raise ValueError(f"levels must lie in [0, {RELOC_MAX_LEVELS}], got {H!r}")
    T = [scan_values_ref(L, floor, unknown_value) + 128]
    nx, ny, nz = T[0].shape
    u = 128 + int(unknown_value)
    for h in range(1, int(H) + 1):
        s = 1 << (h - 1)
        pad = np.full((nx + s, ny + s, nz), u, dtype=np.int64)
        pad[:nx, :ny] = T[-1]
        T.append(np.maximum(np.maximum(pad[:nx, :ny], pad[s:, :ny]), np.maximum(pad[:nx, s:], pad[s:, s:])))
    return T


def scan_level_bytes_ref(T, unknown_value=0):
    """The byte image of one level table T (nx,ny,nz) of bytes -> (256 + 32 words,) uint8: a zero header, then brick order with 128 +
    unknown_value in the pad voxels."""
    T = np.asarray(T, dtype=np.int64)
    nx, ny, nz = T.shape
    nbx, nby, nbz = _evidence_bricks(T.shape)
    pad = np.full((4 * nbx, 4 * nby, 2 * nbz), 128 + int(unknown_value), dtype=np.int64)
    pad[:nx, :ny, :nz] = T
    img = pad.reshape(nbx, 4, nby, 4, nbz, 2).transpose(4, 2, 0, 5, 3, 1).reshape(-1)
    return np.concatenate([np.zeros(EVID_HEADER, dtype=np.uint8), img.astype(np.uint8)])


def scan_lookup_ref(Th, h, u, X, Y, Z):
    """B_h at integer arrays X, Y, Z (any shape): u where Z is outside [0, nz) or X outside [-(2^h - 1), nx) or Y outside [-(2^h - 1),
    ny); otherwise Th[max(X, 0), max(Y, 0), Z], raised to u where X < 0 or Y < 0."""
    nx, ny, nz = Th.shape
    b = (1 << h) - 1
    ins = (Z >= 0) & (Z < nz) & (X >= -b) & (X < nx) & (Y >= -b) & (Y < ny)
    c = Th[np.clip(X, 0, nx - 1), np.clip(Y, 0, ny - 1), np.clip(Z, 0, nz - 1)]
    c = np.where((X < 0) | (Y < 0), np.maximum(c, u), c)
    return np.where(ins, c, u)


def _reloc_bounds(Th, h, u, voxels, nodes, cells=1 << 22):
    """The bounds of nodes (M,4) int64 (k, sx, sy, sz) at level h; voxels[k]: the (n_k,3) voxels in range under rotation k.  A node whose
    k names no rotation gets RELOC_NO_INCUMBENT."""
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1, 4)
    out = np.full(len(nodes), RELOC_NO_INCUMBENT, dtype=np.int64)
    for k in np.unique(nodes[:, 0]):
        if not 0 <= k < len(voxels):
            continue
        rows = np.flatnonzero(nodes[:, 0] == k)
        v = voxels[k]
        if len(v) == 0:
            out[rows] = 0
            continue
        step = max(1, cells // len(v))
        for i in range(0, len(rows), step):
            r = rows[i:i + step]
            s = nodes[r, 1:]
            vals = scan_lookup_ref(Th, h, u, v[None, :, 0] + s[:, None, 0], v[None, :, 1] + s[:, None, 1], v[None, :, 2] + s[:, None, 2])
            out[r] = vals.sum(axis=1) - 128 * len(v)
    return out


def _reloc_voxels(points, Rs, t, origin, resolution):
    Rs = np.asarray(Rs, dtype=np.float32).reshape(-1, 3, 3)
    vox = []
    for R in Rs:
        v, ok = scan_voxels_ref(points, R, t, origin, resolution)
        vox.append(v[ok])
    return vox


def scan_bound_ref(L, origin, resolution, points, Rs, t, nodes, level, floor=None, unknown_value=0):
    """Explicit nodes (M,4) integers (k, sx, sy, sz) of one level -> (bounds (M,) int32, used (K,) int32): the bound of a node is the sum
    over the points in range under rotation k of B_level(voxel_k(p) + (sx, sy, sz)), less 128 x their number."""
    T = scan_levels_ref(L, level, floor, unknown_value)[int(level)]
    vox = _reloc_voxels(points, Rs, t, origin, resolution)
    b = _reloc_bounds(T, int(level), 128 + int(unknown_value), vox, nodes)
    return b.astype(np.int32), np.asarray([len(v) for v in vox], dtype=np.int32)


def _reloc_order(nodes, bounds):
    """The index of the best node: the largest bound, then the lowest (k, sz, sy, sx)."""
    top = np.flatnonzero(bounds == bounds.max())
    n = nodes[top]
    return int(top[np.lexsort((n[:, 1], n[:, 2], n[:, 3], n[:, 0]))[0]])


def _reloc_children(nodes, half, wx, wy):
    kids = []
    for j in range(4):
        c = nodes.copy()
        c[:, 1] += (j & 1) * half
        c[:, 2] += (j >> 1) * half
        kids.append(c[(c[:, 1] <= wx) & (c[:, 2] <= wy)])
    return np.concatenate(kids, axis=0)


def scan_search_ref(L, origin, resolution, points, Rs, t, window, levels, floor=None, unknown_value=0, capacity=1 << 22, lists=None):
    """The branch-and-bound search as DESIGN.md 10 "Relocalisation" defines it -> the record, (18,) int64: flat index, k, dx, dy, dz,
    score, ties, status, incumbent, evaluated, H, nodes[0 .. H] (the rest 0).  The top level holds every node with sx in {-wx, -wx +
    2^H, ...} <= wx, sy likewise, every sz and every rotation; for h = H .. 1: the node with the largest bound (then the lowest (k, sz,
    sy, sx)) is followed greedily to a leaf, the incumbent becomes max(incumbent, the leaf's score), every node whose bound is below
    the incumbent is dropped, the rest are replaced by their children; at level 0 the maximum of the key (score, smaller |s|^2, lower
    flat index) and the number of survivors with the best score.  A level of more than `capacity` nodes stops the search: status =
    count << 3 | (level + 1), flat index -1, nodes[level] = count.  lists: a dict that receives {level: the nodes (m,4) of every list
    that was bounded}, for tests that ask how a list is made up."""
    wx, wy, wz = (int(c) for c in window)
    H = int(levels)
    if not (0 <= wx <= RELOC_MAX_WINDOW[0] and 0 <= wy <= RELOC_MAX_WINDOW[1] and 0 <= wz <= RELOC_MAX_WINDOW[2]):
        raise ValueError(f"window must lie in [0, {RELOC_MAX_WINDOW}] per axis, got {tuple(window)!r}")
    T = scan_levels_ref(L, H, floor, unknown_value)
    u = 128 + int(unknown_value)
    vox = _reloc_voxels(points, Rs, t, origin, resolution)
    K = len(vox)
    rec = np.zeros(RELOC_RECORD, dtype=np.int64)
    rec[8], rec[10] = RELOC_NO_INCUMBENT, H
    step = 1 << H
    k, sz, sy, sx = np.meshgrid(np.arange(K), np.arange(-wz, wz + 1), np.arange(-wy, wy + 1, step), np.arange(-wx, wx + 1, step), indexing="ij")
    nodes = np.stack([k.reshape(-1), sx.reshape(-1), sy.reshape(-1), sz.reshape(-1)], axis=1).astype(np.int64)

    def overflow(level, count):
        rec[0], rec[7], rec[11 + level] = -1, (count << 3) | (level + 1), count
        return rec

    if len(nodes) > capacity:
        return overflow(H, len(nodes))
    bounds = _reloc_bounds(T[H], H, u, vox, nodes)
    rec[9] = len(nodes)
    if lists is not None:
        lists[H] = nodes
    for h in range(H, 0, -1):
        rec[11 + h] = len(nodes)
        at = nodes[_reloc_order(nodes, bounds)][None, :]
        for lev in range(h - 1, -1, -1):
            kids = _reloc_children(at, 1 << lev, wx, wy)
            kb = _reloc_bounds(T[lev], lev, u, vox, kids)
            rec[9] += len(kids)
            i = _reloc_order(kids, kb)
            at, leaf = kids[i][None, :], int(kb[i])
        rec[8] = max(int(rec[8]), leaf)
        nodes = _reloc_children(nodes[bounds >= rec[8]], 1 << (h - 1), wx, wy)
        if len(nodes) > capacity:
            return overflow(h - 1, len(nodes))
        bounds = _reloc_bounds(T[h - 1], h - 1, u, vox, nodes)
        rec[9] += len(nodes)
        if lists is not None:
            lists[h - 1] = nodes
    rec[11] = len(nodes)
    nxw, nyw, nzw = 2 * wx + 1, 2 * wy + 1, 2 * wz + 1
    top = np.flatnonzero(bounds == bounds.max())
    n = nodes[top]
    flat = ((n[:, 0] * nzw + n[:, 3] + wz) * nyw + n[:, 2] + wy) * nxw + n[:, 1] + wx
    d2 = (n[:, 1:] ** 2).sum(axis=1)
    i = np.lexsort((flat, d2))[0]
    rec[:8] = (flat[i], n[i, 0], n[i, 1], n[i, 2], n[i, 3], bounds.max(), len(top), 0)
    return rec


def scan_exhaustive_ref(L, origin, resolution, points, Rs, t, window, floor=None, unknown_value=0):
    """The exhaustive answer over a window of any size -> (7,) int64: flat index, k, dx, dy, dz, score, ties under scan matching's key.
    Per rotation the points in range are grouped by voxel, and each distinct voxel adds its count times the slice of the value volume
    its window covers (unknown_value outside dims) to the window's scores."""
    wx, wy, wz = (int(c) for c in window)
    V = scan_values_ref(L, floor, unknown_value)
    nx, ny, nz = V.shape
    un = int(unknown_value)
    vox = _reloc_voxels(points, Rs, t, origin, resolution)
    scores = np.zeros((len(vox), 2 * wz + 1, 2 * wy + 1, 2 * wx + 1), dtype=np.int64)
    for k, v in enumerate(vox):
        acc = np.full((2 * wx + 1, 2 * wy + 1, 2 * wz + 1), un * len(v), dtype=np.int64)
        if len(v):
            uniq, cnt = np.unique(v, axis=0, return_counts=True)
            for (x, y, z), c in zip(uniq, cnt):
                lo = np.maximum([x - wx, y - wy, z - wz], 0)
                hi = np.minimum([x + wx + 1, y + wy + 1, z + wz + 1], [nx, ny, nz])
                if (lo >= hi).any():
                    continue
                a = lo - np.asarray([x - wx, y - wy, z - wz])
                e = a + (hi - lo)
                acc[a[0]:e[0], a[1]:e[1], a[2]:e[2]] += int(c) * (V[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] - un)
        scores[k] = acc.transpose(2, 1, 0)
    flat = scores.reshape(-1)
    top = np.flatnonzero(flat == flat.max())
    S = scores[0].size
    s = top % S
    dz, rem = s // ((2 * wy + 1) * (2 * wx + 1)) - wz, s % ((2 * wy + 1) * (2 * wx + 1))
    dy, dx = rem // (2 * wx + 1) - wy, rem % (2 * wx + 1) - wx
    i = np.lexsort((top, dx * dx + dy * dy + dz * dz))[0]
    return np.asarray([top[i], top[i] // S, dx[i], dy[i], dz[i], flat.max(), len(top)], dtype=np.int64)


def reloc_default_levels(window):
    """The smallest H <= 6 with ceil((2wx+1) / 2^H) ceil((2wy+1) / 2^H) <= 256 (6 where none is)."""
    wx, wy = int(window[0]), int(window[1])
    for H in range(RELOC_MAX_LEVELS + 1):
        if -(-(2 * wx + 1) // (1 << H)) * -(-(2 * wy + 1) // (1 << H)) <= 256:
            return H
    return RELOC_MAX_LEVELS


def reloc_full_window(voxel, dims):
    """The window centred on the prior's voxel (clamped into dims) that reaches every voxel of dims: wx = max(i_x, nx - 1 - i_x), wy
    likewise, wz = 0."""
    i = [min(max(int(v), 0), int(d) - 1) for v, d in zip(voxel, dims)]
    return (max(i[0], int(dims[0]) - 1 - i[0]), max(i[1], int(dims[1]) - 1 - i[1]), 0)


# ---- scan registration restated in numpy and Python floats ("Scan registration"): what scanreg_kernels.hip must give,
# ---- bit for bit.  The normal equations are integers; the step is f64 add, multiply, divide and compare in one fixed order.
SCANREG_RECORD = 32          # int64 words of a pose's record: H's upper triangle (21), J^T e (6), e^2, used, inside, 0, 0
SCANREG_STATE = 64           # 8-byte words of a pose's state
SCANREG_STATUS = ("RUNNING", "CONVERGED", "STALLED", "DEGENERATE", "EMPTY")
SCANREG_MAX_ITERATIONS = 256
SCANREG_LAMBDA0 = 2.0 ** -10
SCANREG_LAMBDA_MIN, SCANREG_LAMBDA_MAX = 2.0 ** -30, 2.0 ** 30
SCANREG_TOL_T, SCANREG_TOL_R = 1.0 / 256.0, 1.0e-4
# the state's words: f64 unless named an integer
SR_T, SR_Q, SR_LAMBDA, SR_DELTA, SR_STATUS, SR_ITER, SR_ACCEPTED, SR_TRIAL_T, SR_TRIAL_Q, SR_RECORD = 0, 3, 7, 8, 14, 15, 16, 17, 20, 24
SCANREG_DOF = "xyzrpw"       # translation x y z, rotation about the world's x (roll), y (pitch), z (yaw)


def scan_dof_mask(dof):
    """A string over `x y z r p w` (each at most once, at least one), or a 6-bit mask in [1, 63] -> the mask: bit i frees degree of
    freedom i of (x, y, z, roll, pitch, yaw)."""
    if isinstance(dof, str):
        if not dof or len(set(dof)) != len(dof) or any(c not in SCANREG_DOF for c in dof):
            raise ValueError(f"dof must name each of 'x y z r p w' at most once and one at least, got {dof!r}")
        return sum(1 << SCANREG_DOF.index(c) for c in dof)
    if isinstance(dof, (int, np.integer)) and not isinstance(dof, bool) and 1 <= int(dof) <= 63:
        return int(dof)
    raise ValueError(f"dof must be a string over 'xyzrpw' or a mask in [1, 63], got {dof!r}")


def scan_fixed_ref(points, R, t, origin, resolution):
    """Sensor-frame points (N,3) under the pose (R, t) -> (q (N,3) int64 in 1/256 voxel, ok (N,)): scan_voxels_ref's world coordinate,
    then occ_fixed."""
    f32 = np.float32
    P = np.asarray(points, dtype=f32).reshape(-1, 3)
    R, t = np.asarray(R, dtype=f32).reshape(3, 3), np.asarray(t, dtype=f32).reshape(3)
    with np.errstate(all="ignore"):
        cols = []
        for a in range(3):
            s = ((R[a, 0] * P[:, 0]).astype(f32) + (R[a, 1] * P[:, 1]).astype(f32)).astype(f32)
            s = (s + (R[a, 2] * P[:, 2]).astype(f32)).astype(f32)
            cols.append((s + t[a]).astype(f32))
        W = np.stack(cols, axis=1)
    return occ_fixed(W, origin, resolution)


def scan_corners_ref(T, q, unknown_value=0):
    """Fixed-point positions q (n,3) int64 over the dense table T (nx,ny,nz) of bytes -> (V (2,2,2,n) int64, w [axis] (2,n), all_inside
    (n,)): the eight table bytes around each position on the lattice of voxel CENTRES, 128 + unknown_value outside dims."""
    c = q - 128
    b, f = c >> 8, c & 255
    w = [np.stack([256 - f[:, k], f[:, k]]) for k in range(3)]
    dims = np.asarray(T.shape, dtype=np.int64)
    V = np.empty((2, 2, 2, len(q)), dtype=np.int64)
    all_in = np.ones(len(q), dtype=bool)
    for i in range(2):
        for j in range(2):
            for k in range(2):
                v = b + np.asarray((i, j, k), dtype=np.int64)
                ok = ((v >= 0) & (v < dims)).all(axis=1)
                vc = np.clip(v, 0, dims - 1)
                V[i, j, k] = np.where(ok, T[vc[:, 0], vc[:, 1], vc[:, 2]], 128 + int(unknown_value))
                all_in &= ok
    return V, w, all_in


def scan_rows_ref(T, q, qt, unknown_value=0):
    """The rows of the normal equations at positions q (n,3) with the pose's own fixed-point translation qt (3,) -> (J (n,6) int64,
    e (n,) int64, all_inside (n,)), straight from the definitions: M24, G16, e, g, the lever arm a and j = (a x g + 2^11) >> 12."""
    V, w, all_in = scan_corners_ref(T, q, unknown_value)
    M24 = sum(V[i, j, k] * w[0][i] * w[1][j] * w[2][k] for i in range(2) for j in range(2) for k in range(2))
    Gx = sum(w[1][j] * w[2][k] * (V[1, j, k] - V[0, j, k]) for j in range(2) for k in range(2))
    Gy = sum(w[0][i] * w[2][k] * (V[i, 1, k] - V[i, 0, k]) for i in range(2) for k in range(2))
    Gz = sum(w[0][i] * w[1][j] * (V[i, j, 1] - V[i, j, 0]) for i in range(2) for j in range(2))
    e = (255 * (1 << 24) - M24 + (1 << 11)) >> 12
    g = (np.stack([Gx, Gy, Gz], axis=1) + 128) >> 8
    a = (q - np.asarray(qt, dtype=np.int64).reshape(1, 3) + 32) >> 6
    cr = np.stack([a[:, 1] * g[:, 2] - a[:, 2] * g[:, 1], a[:, 2] * g[:, 0] - a[:, 0] * g[:, 2], a[:, 0] * g[:, 1] - a[:, 1] * g[:, 0]], axis=1)
    return np.concatenate([g, (cr + (1 << 11)) >> 12], axis=1), e, all_in


def scan_normal_ref(L, origin, resolution, points, poses12, floor=None, unknown_value=0, chunk=1 << 16):
    """The records of B poses -> (B, 32) int64: [0:21] the upper triangle of H = sum J J^T, row-major, [21:27] sum J e, [27] sum e^2,
    [28] used, [29] inside (all eight corners inside dims), [30:32] 0.  poses12 (B,12) f32: R row-major, then t.  A pose whose t is
    out of range has an all-zero record.  At most 2^22 points: every sum stays below 2^62 and int64 holds it."""
    P = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    if not 1 <= len(P) <= SCAN_MAX_POINTS:
        raise ValueError(f"1 .. 2^22 points, got {len(P)}")
    poses12 = np.asarray(poses12, dtype=np.float32).reshape(-1, 12)
    T = scan_values_ref(L, floor, unknown_value) + 128
    iu = np.triu_indices(6)
    out = np.zeros((len(poses12), SCANREG_RECORD), dtype=np.int64)
    for b, pose in enumerate(poses12):
        qt, t_ok = occ_fixed(pose[9:12], origin, resolution)
        if not t_ok[0]:
            continue
        q, ok = scan_fixed_ref(P, pose[:9], pose[9:12], origin, resolution)
        q = q[ok]
        for i in range(0, len(q), chunk):
            J, e, all_in = scan_rows_ref(T, q[i:i + chunk], qt[0], unknown_value)
            out[b, :21] += (J[:, iu[0]] * J[:, iu[1]]).sum(axis=0)
            out[b, 21:27] += (J * e[:, None]).sum(axis=0)
            out[b, 27] += (e * e).sum()
            out[b, 29] += int(all_in.sum())
        out[b, 28] = len(q)
    return out


def scan_pose12_ref(t, q):
    """The f64 state pose (t (3,) metres, q (4,) wxyz UNNORMALISED) -> the 12 f32 the kernels take: R of q with s = 2 / (q . q), in
    this operation order, then t; each rounded once."""
    w, x, y, z = (float(v) for v in q)
    s = 2.0 / (((w * w + x * x) + y * y) + z * z)
    R = [1.0 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y),
         s * (x * y + w * z), 1.0 - s * (x * x + z * z), s * (y * z - w * x),
         s * (x * z - w * y), s * (y * z + w * x), 1.0 - s * (x * x + y * y)]
    return np.asarray(R + [float(v) for v in t], dtype=np.float64).astype(np.float32)


def scan_register_init_ref(poses, quats):
    """B starting poses (B,3) and quaternions (B,4), host numbers -> (state (B,64) int64 — f64 words by their bits —, poses12 (B,12)
    f32): the current and the trial pose are the start, lambda = 2^-10, everything else 0."""
    t = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(quats, dtype=np.float64).reshape(-1, 4)
    st = np.zeros((len(t), SCANREG_STATE), dtype=np.float64)
    st[:, SR_T:SR_T + 3] = st[:, SR_TRIAL_T:SR_TRIAL_T + 3] = t
    st[:, SR_Q:SR_Q + 4] = st[:, SR_TRIAL_Q:SR_TRIAL_Q + 4] = q
    st[:, SR_LAMBDA] = SCANREG_LAMBDA0
    return st.view(np.int64), np.stack([scan_pose12_ref(a, b) for a, b in zip(t, q)])


def scan_solve_ref(record, lam, mask):
    """One damped Gauss-Newton solve from a record (32 ints) -> delta (6 floats: voxels, radians) or None where a pivot is <= 0 or not
    finite.  A = S H S and rhs = S b / 4096 with S = diag(1/256 x3, 4 x3); a locked degree of freedom has its row and column cleared,
    1 on the diagonal and rhs 0; A_ii += lam A_ii; LDL^T without pivoting, columns left to right, each sum in ascending k."""
    S = (1.0 / 256.0,) * 3 + (4.0,) * 3
    A = [[0.0] * 6 for _ in range(6)]
    rhs = [0.0] * 6
    n = 0
    for i in range(6):
        for j in range(i, 6):
            free = (mask >> i) & 1 and (mask >> j) & 1
            v = float(int(record[n])) * S[i] * S[j] if free else (1.0 if i == j else 0.0)
            A[i][j] = A[j][i] = v
            n += 1
        rhs[i] = float(int(record[21 + i])) * S[i] * (1.0 / 4096.0) if (mask >> i) & 1 else 0.0
    for i in range(6):
        if (mask >> i) & 1:
            A[i][i] = A[i][i] + lam * A[i][i]
    Lm = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        v = A[j][j]
        for k in range(j):
            v = v - Lm[j][k] * (Lm[j][k] * d[k])
        if not (v > 0.0) or not v < math.inf:
            return None
        d[j] = v
        for i in range(j + 1, 6):
            u = A[i][j]
            for k in range(j):
                u = u - Lm[i][k] * (Lm[j][k] * d[k])
            Lm[i][j] = u / v
    y = [0.0] * 6
    for i in range(6):
        v = rhs[i]
        for k in range(i):
            v = v - Lm[i][k] * y[k]
        y[i] = v
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i] / d[i]
        for k in range(i + 1, 6):
            v = v - Lm[k][i] * x[k]
        x[i] = v
    return x


def scan_step_ref(records, state, resolution, dof=63, tol_t=SCANREG_TOL_T, tol_r=SCANREG_TOL_R):
    """One step of every pose: records (B,32) int64 at the trial poses and state (B,64) int64 -> (the next state, poses12 (B,12) f32 or
    None rows where a pose wrote none): what k_scan_step does, in Python floats (IEEE binary64, no fused operation)."""
    mask = scan_dof_mask(dof)
    r = float(np.float32(resolution))
    tol_t, tol_r = float(tol_t), float(tol_r)
    state = np.array(state, dtype=np.int64).reshape(-1, SCANREG_STATE)
    records = np.asarray(records, dtype=np.int64).reshape(-1, SCANREG_RECORD)
    F = state.view(np.float64)
    poses12 = [None] * len(state)
    for b in range(len(state)):
        I, D = state[b], F[b]
        if I[SR_STATUS] != 0:
            continue
        first = I[SR_ITER] == 0
        I[SR_ITER] += 1
        rec = records[b]
        if rec[28] == 0:
            I[SR_STATUS] = 4
            continue
        cur = I[SR_RECORD:SR_RECORD + 32]
        if first or (rec[28] == cur[28] and rec[27] < cur[27]):
            D[SR_T:SR_T + 3] = D[SR_TRIAL_T:SR_TRIAL_T + 3]
            D[SR_Q:SR_Q + 4] = D[SR_TRIAL_Q:SR_TRIAL_Q + 4]
            cur[:] = rec
            if not first:
                I[SR_ACCEPTED] += 1
                lam = float(D[SR_LAMBDA]) / 8.0
                D[SR_LAMBDA] = lam if lam > SCANREG_LAMBDA_MIN else SCANREG_LAMBDA_MIN
                d = [float(v) for v in D[SR_DELTA:SR_DELTA + 6]]
                if all(v <= tol_t and -v <= tol_t for v in d[:3]) and all(v <= tol_r and -v <= tol_r for v in d[3:]):
                    I[SR_STATUS] = 1
                    continue
        else:
            lam = float(D[SR_LAMBDA]) * 8.0
            D[SR_LAMBDA] = lam
            if lam > SCANREG_LAMBDA_MAX:
                I[SR_STATUS] = 2
                continue
        x = scan_solve_ref([int(v) for v in cur], float(D[SR_LAMBDA]), mask)
        if x is None:
            I[SR_STATUS] = 3
            continue
        D[SR_DELTA:SR_DELTA + 6] = x
        t = [float(D[SR_T + a]) + r * x[a] for a in range(3)]
        qw, qx, qy, qz = (float(v) for v in D[SR_Q:SR_Q + 4])
        hx, hy, hz = 0.5 * x[3], 0.5 * x[4], 0.5 * x[5]
        q = [((qw - hx * qx) - hy * qy) - hz * qz,
             ((qx + hx * qw) + hy * qz) - hz * qy,
             ((qy - hx * qz) + hy * qw) + hz * qx,
             ((qz + hx * qy) - hy * qx) + hz * qw]
        D[SR_TRIAL_T:SR_TRIAL_T + 3] = t
        D[SR_TRIAL_Q:SR_TRIAL_Q + 4] = q
        poses12[b] = scan_pose12_ref(t, q)
    return state, poses12


def scan_register_ref(L, origin, resolution, points, poses, quats, iterations=30, dof=63, tol_t=SCANREG_TOL_T, tol_r=SCANREG_TOL_R, floor=None,
                      unknown_value=0):
    """`iterations` rounds of normal + step from the starting poses -> the state (B,64) int64: what ScanMatcher.register leaves on the
    device, bit for bit.  A frozen pose's record is not evaluated."""
    if not 1 <= int(iterations) <= SCANREG_MAX_ITERATIONS:
        raise ValueError(f"1 .. {SCANREG_MAX_ITERATIONS} iterations, got {iterations!r}")
    state, poses12 = scan_register_init_ref(poses, quats)
    for _ in range(int(iterations)):
        live = np.flatnonzero(state[:, SR_STATUS] == 0)
        if len(live) == 0:
            break
        records = np.zeros((len(state), SCANREG_RECORD), dtype=np.int64)
        records[live] = scan_normal_ref(L, origin, resolution, points, poses12[live], floor, unknown_value)
        state, new = scan_step_ref(records, state, resolution, dof, tol_t, tol_r)
        for b, row in enumerate(new):
            if row is not None:
                poses12[b] = row
    return state



# ---- pose-graph optimisation restated in numpy ("Pose graph"): what posegraph_kernels.hip must give, bit for bit.  All
# ---- of it is f64 add, subtract, multiply, divide and compare, elementwise over the edges or the nodes, in ONE order:
#   a product of two 6 x 6 blocks, and a block times a vector, sums its six terms in ascending index, left to right, from the first
#     product (no leading zero);
#   a node's sums over its incident edges start at 0.0 and add the edges in ascending edge index (pose_graph_incidence);
#   a sum over the nodes (a dot product: the node's six products left to right first) or over the edges (the cost) is a halving tree
#     over each block of 256 (v[i] += v[i + m], m = 128, 64 .. 1; the last block padded with 0.0), then the block partials from 0.0 in
#     ascending block order (pose_graph_tree_sum).
POSEGRAPH_EDGE = 100         # f64 words of an edge's record
# the record's words: e (6), s = e^T Omega e, the IRLS weight w, rho(s), 0, then with W = w Omega the upper triangles of Ja^T W Ja and
# Jb^T W Jb (21 each, row-major), Ja^T W Jb (36, row-major), Ja^T W e and Jb^T W e (6 each)
PG_E, PG_S, PG_W, PG_RHO, PG_HAA, PG_HBB, PG_HAB, PG_GA, PG_GB = 0, 6, 7, 8, 10, 31, 52, 88, 94
POSEGRAPH_STATUS = ("RUNNING", "CONVERGED", "STALLED", "DEGENERATE", "NONFINITE")
POSEGRAPH_LAMBDA0 = 2.0 ** -10
POSEGRAPH_BLOCK = 256
POSEGRAPH_MAX_NODES = POSEGRAPH_MAX_EDGES = 1 << 22
_PG_TRIU = [(i, j) for i in range(6) for j in range(i, 6)]


def pose_graph_tree_sum(v):
    """The one order of a sum over nodes or edges -> a Python float: halving trees over blocks of 256, then the partials ascending."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    nb = max(1, -(-len(v) // POSEGRAPH_BLOCK))
    w = np.zeros(nb * POSEGRAPH_BLOCK, dtype=np.float64)
    w[:len(v)] = v
    w = w.reshape(nb, POSEGRAPH_BLOCK)
    m = POSEGRAPH_BLOCK // 2
    with np.errstate(all="ignore"):
        while m >= 1:
            w[:, :m] = w[:, :m] + w[:, m:2 * m]
            m //= 2
        total = 0.0
        for b in range(nb):
            total = total + float(w[b, 0])
    return total


def pose_graph_incidence(ab, n):
    """Edges (E,2) int32, a = -1 an absolute edge -> (row_ptr (n+1,) int32, incident int32): node i's entries are
    incident[row_ptr[i]:row_ptr[i+1]], each 2 edge + side (side 0: the node is the edge's a, 1: its b), in ascending edge index."""
    ab = np.asarray(ab, dtype=np.int64).reshape(-1, 2)
    node = ab.reshape(-1)                                   # entry 2 k + side
    code = np.arange(len(node), dtype=np.int64)
    keep = node >= 0
    node, code = node[keep], code[keep]
    order = np.argsort(node, kind="stable")                 # (stable: ascending code, so ascending edge, within a node)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(row_ptr, node + 1, 1)
    return np.cumsum(row_ptr).astype(np.int32), code[order].astype(np.int32)


def _pg_qmul(p, q):
    """The Hamilton product p (x) q of two quaternions given as 4 arrays each, in k_scan_step's operation order."""
    pw, px, py, pz = p
    qw, qx, qy, qz = q
    return (((pw * qw - px * qx) - py * qy) - pz * qz,
            ((pw * qx + px * qw) + py * qz) - pz * qy,
            ((pw * qy - px * qz) + py * qw) + pz * qx,
            ((pw * qz + px * qy) - py * qx) + pz * qw)


def _pg_rot(q):
    """R of an unnormalised quaternion, s = 2 / (q . q): scan_pose12_ref's rule, as 3 x 3 arrays in f64."""
    w, x, y, z = q
    s = 2.0 / (((w * w + x * x) + y * y) + z * z)
    return [[1.0 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
            [s * (x * y + w * z), 1.0 - s * (x * x + z * z), s * (y * z - w * x)],
            [s * (x * z - w * y), s * (y * z + w * x), 1.0 - s * (x * x + y * y)]]


def pose_graph_perturb_ref(t, q, x):
    """Nodes (N,3), (N,4) moved by x (N,6): t + dt and (1, dr / 2) (x) q, k_scan_step's perturbation -> (t, q)."""
    t, q, x = (np.asarray(v, dtype=np.float64) for v in (t, q, x))
    with np.errstate(all="ignore"):
        nq = _pg_qmul((1.0, 0.5 * x[:, 3], 0.5 * x[:, 4], 0.5 * x[:, 5]), (q[:, 0], q[:, 1], q[:, 2], q[:, 3]))
        return t + x[:, :3], np.stack(nq, axis=1)


def _pg_edges(t, q, ab, zt, zq):
    """-> (e [6], R [3][3] of node a, v [3] = t_b - t_a), arrays over the edges.  An absolute edge (a = -1) is an edge from the world
    frame, t = 0 and q = (1, 0, 0, 0): then d_t = t_b and d_q = q_b exactly."""
    t, q = np.asarray(t, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64).reshape(-1, 4)
    ab = np.asarray(ab, dtype=np.int64).reshape(-1, 2)
    zt, zq = np.asarray(zt, dtype=np.float64).reshape(-1, 3), np.asarray(zq, dtype=np.float64).reshape(-1, 4)
    a, b = ab[:, 0], ab[:, 1]
    world = a < 0
    ta = np.where(world[:, None], 0.0, t[np.maximum(a, 0)])
    qa = np.where(world[:, None], np.asarray([1.0, 0.0, 0.0, 0.0]), q[np.maximum(a, 0)])
    tb, qb = t[b], q[b]
    R = _pg_rot(qa.T)
    v = [tb[:, k] - ta[:, k] for k in range(3)]
    e = [((R[0][i] * v[0] + R[1][i] * v[1]) + R[2][i] * v[2]) - zt[:, i] for i in range(3)]
    dq = _pg_qmul((qa[:, 0], -qa[:, 1], -qa[:, 2], -qa[:, 3]), qb.T)
    eps = _pg_qmul(dq, (zq[:, 0], -zq[:, 1], -zq[:, 2], -zq[:, 3]))
    e += [(2.0 * eps[k]) / eps[0] for k in (1, 2, 3)]
    return e, R, v


def pose_graph_residual_ref(t, q, ab, zt, zq):
    """The residuals (E,6) of the edges at the nodes (t (N,3), q (N,4) wxyz, not normalised): e_t = R_a^T (t_b - t_a) - z_t and the
    Gibbs vector e_r = 2 vec(eps) / w(eps) of eps = conj(q_a) (x) q_b (x) conj(z_q).  w(eps) = 0 gives a non-finite entry."""
    with np.errstate(all="ignore"):
        return np.stack(_pg_edges(t, q, ab, zt, zq)[0], axis=1)


def _pg_jacobians(e, R, v):
    """The exact first derivatives of e in (dt, dr) of node a and of node b -> (Ja, Jb) as 6 x 6 lists of arrays (a Python 0.0 where
    the entry is structurally zero).  With G = I - [e_r / 2]x + (e_r / 2)(e_r / 2)^T:
        Jb = [[R^T, 0], [0, G R^T]],   Ja = [[-R^T, R^T [v]x], [0, -G R^T]]."""
    h = [0.5 * e[3], 0.5 * e[4], 0.5 * e[5]]
    G = [[1.0 + h[0] * h[0], h[0] * h[1] + h[2], h[0] * h[2] - h[1]],
         [h[1] * h[0] - h[2], 1.0 + h[1] * h[1], h[1] * h[2] + h[0]],
         [h[2] * h[0] + h[1], h[2] * h[1] - h[0], 1.0 + h[2] * h[2]]]
    GR = [[(G[i][0] * R[j][0] + G[i][1] * R[j][1]) + G[i][2] * R[j][2] for j in range(3)] for i in range(3)]
    Ja = [[0.0] * 6 for _ in range(6)]
    Jb = [[0.0] * 6 for _ in range(6)]
    for i in range(3):
        for j in range(3):
            Jb[i][j] = R[j][i]
            Ja[i][j] = -R[j][i]
            Jb[3 + i][3 + j] = GR[i][j]
            Ja[3 + i][3 + j] = -GR[i][j]
        Ja[i][3] = R[1][i] * v[2] - R[2][i] * v[1]
        Ja[i][4] = R[2][i] * v[0] - R[0][i] * v[2]
        Ja[i][5] = R[0][i] * v[1] - R[1][i] * v[0]
    return Ja, Jb


def pose_graph_jacobians_ref(t, q, ab, zt, zq):
    """-> (Ja (E,6,6), Jb (E,6,6)), unmasked: what pose_graph_linearize_ref multiplies out.  Ja of an absolute edge is the derivative
    in the world frame's own motion, which nothing uses."""
    with np.errstate(all="ignore"):
        e, R, v = _pg_edges(t, q, ab, zt, zq)
        Ja, Jb = _pg_jacobians(e, R, v)
    E = len(e[0])
    full = lambda J: np.stack([np.stack([np.broadcast_to(np.asarray(J[i][j], dtype=np.float64), (E,)) for j in range(6)], axis=1)   # noqa: E731
                               for i in range(6)], axis=1)
    return full(Ja), full(Jb)


def pose_graph_omega_full(omega):
    """(E,21) upper triangles, row-major -> (E,6,6) symmetric."""
    omega = np.asarray(omega, dtype=np.float64).reshape(-1, 21)
    O = np.zeros((len(omega), 6, 6))
    for n, (i, j) in enumerate(_PG_TRIU):
        O[:, i, j] = O[:, j, i] = omega[:, n]
    return O


def pose_graph_free_masks(n, fixed=(), dof=63):
    """-> (n,) int32: a node's free degrees of freedom, scan_dof_mask(dof), 0 for a fixed node."""
    m = np.full(n, scan_dof_mask(dof), dtype=np.int32)
    m[np.asarray(list(fixed), dtype=np.int64)] = 0
    return m


def _pg_dot6(A, x):
    """sum_k A[k] x[k], ascending k from the first product."""
    acc = A[0] * x[0]
    for k in range(1, 6):
        acc = acc + A[k] * x[k]
    return acc


def pose_graph_linearize_ref(t, q, ab, zt, zq, omega, free_mask, robust=None):
    """The edge records (E,100) at the nodes: e, s = e^T Omega e (u = Omega e first, each row ascending; then e . u), the weight
    w (1.0, or (c^2 / (c^2 + s))^2 with robust=c), rho(s) (s, or c^2 s / (c^2 + s)), and with W = w Omega and the columns of Ja and Jb
    of LOCKED degrees of freedom (free_mask; every one of the world frame's) set to 0.0: M_a = W Ja, M_b = W Jb, u_w = W e, then
    Ja^T M_a and Jb^T M_b (upper triangles), Ja^T M_b, Ja^T u_w and Jb^T u_w."""
    ab = np.asarray(ab, dtype=np.int64).reshape(-1, 2)
    free_mask = np.asarray(free_mask, dtype=np.int64)
    E = len(ab)
    rec = np.zeros((E, POSEGRAPH_EDGE), dtype=np.float64)
    if E == 0:
        return rec
    with np.errstate(all="ignore"):
        e, R, v = _pg_edges(t, q, ab, zt, zq)
        Ja, Jb = _pg_jacobians(e, R, v)
        O = pose_graph_omega_full(omega)
        Om = [[O[:, i, j] for j in range(6)] for i in range(6)]
        u = [_pg_dot6(Om[i], e) for i in range(6)]
        s = _pg_dot6(e, u)
        if robust is None:
            w, rho = np.ones(E), s
        else:
            c2 = float(robust) * float(robust)
            f = c2 / (c2 + s)
            w, rho = f * f, (c2 * s) / (c2 + s)
        ma = np.where(ab[:, 0] >= 0, free_mask[np.maximum(ab[:, 0], 0)], 0)
        mb = free_mask[ab[:, 1]]
        zero = np.zeros(E)
        for J, m in ((Ja, ma), (Jb, mb)):
            for c in range(6):
                on = ((m >> c) & 1).astype(bool)
                for r in range(6):
                    J[r][c] = np.where(on, J[r][c], zero)
        W = [[w * Om[i][j] for j in range(6)] for i in range(6)]
        col = lambda J, j: [J[k][j] for k in range(6)]                                     # noqa: E731
        Ma = [[_pg_dot6(W[i], col(Ja, j)) for j in range(6)] for i in range(6)]
        Mb = [[_pg_dot6(W[i], col(Jb, j)) for j in range(6)] for i in range(6)]
        uw = [_pg_dot6(W[i], e) for i in range(6)]
        for k in range(6):
            rec[:, PG_E + k] = e[k]
            rec[:, PG_GA + k] = _pg_dot6(col(Ja, k), uw)
            rec[:, PG_GB + k] = _pg_dot6(col(Jb, k), uw)
        rec[:, PG_S], rec[:, PG_W], rec[:, PG_RHO] = s, w, rho
        for n, (i, j) in enumerate(_PG_TRIU):
            rec[:, PG_HAA + n] = _pg_dot6(col(Ja, i), col(Ma, j))
            rec[:, PG_HBB + n] = _pg_dot6(col(Jb, i), col(Mb, j))
        for i in range(6):
            for j in range(6):
                rec[:, PG_HAB + 6 * i + j] = _pg_dot6(col(Ja, i), col(Mb, j))
    return rec


def pose_graph_gather_ref(rec, ab, n, free_mask):
    """-> (D (n,21), the upper triangle of each node's diagonal block of H; g (n,6); cost): a node's sums over its incident edges from
    0.0 in ascending edge index (Ja^T W Ja and Ja^T W e where it is the edge's a, Jb^T W Jb and Jb^T W e where it is its b); then a
    locked degree of freedom's row and column are 0.0 with 1.0 on the diagonal, and its g is 0.0.  cost: the tree sum of rho."""
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, POSEGRAPH_EDGE)
    row_ptr, inc = pose_graph_incidence(ab, n)
    free_mask = np.asarray(free_mask, dtype=np.int64)
    D, g = np.zeros((n, 21)), np.zeros((n, 6))
    deg = np.diff(row_ptr)
    with np.errstate(all="ignore"):
        for s in range(int(deg.max()) if n else 0):
            nodes = np.flatnonzero(deg > s)
            code = inc[row_ptr[nodes] + s].astype(np.int64)
            k, side = code >> 1, (code & 1).astype(bool)
            D[nodes] = D[nodes] + np.where(side[:, None], rec[k, PG_HBB:PG_HBB + 21], rec[k, PG_HAA:PG_HAA + 21])
            g[nodes] = g[nodes] + np.where(side[:, None], rec[k, PG_GB:PG_GB + 6], rec[k, PG_GA:PG_GA + 6])
    for m, (i, j) in enumerate(_PG_TRIU):
        locked = (((free_mask >> i) & 1) == 0) | (((free_mask >> j) & 1) == 0)
        D[locked, m] = 1.0 if i == j else 0.0
    for i in range(6):
        g[((free_mask >> i) & 1) == 0, i] = 0.0
    return D, g, pose_graph_tree_sum(rec[:, PG_RHO])


def pose_graph_factor_ref(D, lam, free_mask):
    """Each node's damped block, A_ii += lam A_ii on its free degrees of freedom, factored L d L^T in scan_solve_ref's order ->
    (L (n,6,6) strictly lower, d (n,6), ok (n,) bool: every pivot > 0 and finite)."""
    D = np.asarray(D, dtype=np.float64).reshape(-1, 21)
    free_mask = np.asarray(free_mask, dtype=np.int64)
    n = len(D)
    A = [[None] * 6 for _ in range(6)]
    for m, (i, j) in enumerate(_PG_TRIU):
        A[i][j] = A[j][i] = D[:, m]
    with np.errstate(all="ignore"):
        for i in range(6):
            A[i][i] = np.where((free_mask >> i) & 1, A[i][i] + lam * A[i][i], A[i][i])
        L, d, ok = np.zeros((n, 6, 6)), np.zeros((n, 6)), np.ones(n, dtype=bool)
        for j in range(6):
            v = A[j][j]
            for k in range(j):
                v = v - L[:, j, k] * (L[:, j, k] * d[:, k])
            ok &= (v > 0.0) & (v < math.inf)
            d[:, j] = v
            for i in range(j + 1, 6):
                u = A[i][j]
                for k in range(j):
                    u = u - L[:, i, k] * (L[:, j, k] * d[:, k])
                L[:, i, j] = u / v
    return L, d, ok


def pose_graph_block_solve_ref(L, d, r):
    """z = (L d L^T)^-1 r per node, scan_solve_ref's forward and back substitution."""
    n = len(r)
    y, z = np.zeros((n, 6)), np.zeros((n, 6))
    with np.errstate(all="ignore"):
        for i in range(6):
            v = r[:, i]
            for k in range(i):
                v = v - L[:, i, k] * y[:, k]
            y[:, i] = v
        for i in range(5, -1, -1):
            v = y[:, i] / d[:, i]
            for k in range(i + 1, 6):
                v = v - L[:, k, i] * z[:, k]
            z[:, i] = v
    return z


def _pg_node_dot(a, b):
    """sum over the nodes of a_i . b_i: six products left to right, then the tree."""
    acc = a[:, 0] * b[:, 0]
    for k in range(1, 6):
        acc = acc + a[:, k] * b[:, k]
    return pose_graph_tree_sum(acc)


def pose_graph_matvec_plan(D, rec, ab, lam, free_mask):
    """-> matvec(p (n,6)) -> (n,6), (H + lam diag H) p by node rows: the node's own damped block first (row r: sum_c A[r][c] p[c],
    ascending c), then its incident edges in ascending edge index, each adding B p_other (B = Ja^T W Jb where the node is a, its
    transpose where it is b; the six terms ascending, summed before they are added; an absolute edge has no such block).  What does
    not depend on p is laid out once."""
    n = len(D)
    ab = np.asarray(ab, dtype=np.int64).reshape(-1, 2)
    free_mask = np.asarray(free_mask, dtype=np.int64)
    row_ptr, inc = pose_graph_incidence(ab, n)
    deg = np.diff(row_ptr)
    A = [[None] * 6 for _ in range(6)]
    for m, (i, j) in enumerate(_PG_TRIU):
        A[i][j] = A[j][i] = D[:, m]
    with np.errstate(all="ignore"):
        for i in range(6):
            A[i][i] = np.where((free_mask >> i) & 1, A[i][i] + lam * A[i][i], A[i][i])
    slots = []
    for s in range(int(deg.max()) if n else 0):
        nodes = np.flatnonzero(deg > s)
        code = inc[row_ptr[nodes] + s].astype(np.int64)
        k, side = code >> 1, (code & 1).astype(bool)
        keep = ab[k, 0] >= 0
        nodes, k, side = nodes[keep], k[keep], side[keep]
        B = rec[k, PG_HAB:PG_HAB + 36].reshape(-1, 6, 6)
        rows = [[np.where(side, B[:, c, r], B[:, r, c]) for c in range(6)] for r in range(6)]
        slots.append((nodes, np.where(side, ab[k, 0], ab[k, 1]), rows))

    def matvec(p):
        out = np.zeros((n, 6))
        with np.errstate(all="ignore"):
            pc = [p[:, c] for c in range(6)]
            for r in range(6):
                out[:, r] = _pg_dot6(A[r], pc)
            for nodes, other, rows in slots:
                po = [p[other, c] for c in range(6)]
                for r in range(6):
                    out[nodes, r] = out[nodes, r] + _pg_dot6(rows[r], po)
        return out
    return matvec


def pose_graph_matvec_ref(D, rec, ab, lam, free_mask, p):
    """(H + lam diag H) p -> (n,6): pose_graph_matvec_plan's product, once."""
    return pose_graph_matvec_plan(D, rec, ab, lam, free_mask)(np.asarray(p, dtype=np.float64))


def pose_graph_cg_ref(D, g, rec, ab, lam, free_mask, cg_iterations, cg_tol=1e-8, tol_t=0.0, tol_r=0.0):
    """One damped solve (H + lam diag H) x = -g by preconditioned conjugate gradients from x = 0, the preconditioner the L d L^T of each
    damped diagonal block -> dict(x (n,6), iterations, degenerate, small).  r = 0.0 - g, z = M^-1 r, then per iteration: rz = r . z
    (rz0 the first); stop if rz <= cg_tol^2 rz0; beta = 0.0 the first time, rz / the previous rz after; p = z + beta p (p = 0 before);
    Ap; pAp = p . Ap; stop, keeping x, unless pAp > 0; alpha = rz / pAp; x = x + alpha p; r = r - alpha Ap; z = M^-1 r.  small: every
    |x| within tol_t (translation) and tol_r (rotation).  degenerate: a block pivot <= 0 or not finite: nothing is solved."""
    n = len(D)
    g = np.asarray(g, dtype=np.float64).reshape(n, 6)
    L, d, ok = pose_graph_factor_ref(D, lam, free_mask)
    x = np.zeros((n, 6))
    out = dict(x=x, iterations=0, degenerate=not bool(ok.all()), small=True)
    if out["degenerate"]:
        return out
    tol2 = float(cg_tol) * float(cg_tol)
    tol = np.asarray([tol_t] * 3 + [tol_r] * 3, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = 0.0 - g
        z = pose_graph_block_solve_ref(L, d, r)
        p = np.zeros((n, 6))
        rz_prev = rz0 = 0.0
        matvec = pose_graph_matvec_plan(D, rec, ab, lam, free_mask)
        for k in range(int(cg_iterations)):
            rz = _pg_node_dot(r, z)
            if k == 0:
                rz0, beta = rz, 0.0
            else:
                beta = rz / rz_prev
            if rz <= tol2 * rz0:
                break
            rz_prev = rz
            p = z + beta * p
            Ap = matvec(p)
            pAp = _pg_node_dot(p, Ap)
            if not pAp > 0.0:
                break
            alpha = rz / pAp
            x = x + alpha * p
            r = r - alpha * Ap
            z = pose_graph_block_solve_ref(L, d, r)
            out["iterations"] += 1
            out["small"] = bool(((x <= tol) & (-x <= tol)).all())
    out["x"] = x
    return out


def pose_graph_start_ref(t, q):
    """The optimiser's state at its start, a dict: the current nodes t, q; the pending step x = 0; lam = 2^-10; status RUNNING (0);
    iterations, accepted, cg_iterations 0; cost and initial_cost 0.0; small True; rec, D, g None until the first acceptance."""
    t = np.array(t, dtype=np.float64).reshape(-1, 3)
    q = np.array(q, dtype=np.float64).reshape(-1, 4)
    return dict(t=t, q=q, x=np.zeros((len(t), 6)), lam=POSEGRAPH_LAMBDA0, status=0, iterations=0, accepted=0, cg_iterations=0, cost=0.0,
                initial_cost=0.0, small=True, rec=None, D=None, g=None)


def pose_graph_step_ref(state, ab, zt, zq, omega, free_mask, cg_iterations, cg_tol=1e-8, robust=None, tol_t=1e-5, tol_r=1e-6):
    """One outer iteration, in place: linearise at the TRIAL nodes (the current ones moved by x), gather, then k_scan_step's state
    machine — a non-finite trial cost: NONFINITE; the first trial, or one whose cost is strictly lower: accepted (the trial becomes
    current; after the first: accepted + 1, lam = max(lam / 8, 2^-30), CONVERGED if the step was small); otherwise lam = 8 lam,
    STALLED past 2^30 — and the next damped solve by pose_graph_cg_ref (DEGENERATE from it).  A state that is not RUNNING is left."""
    st = state
    if st["status"] != 0:
        return st
    n = len(st["t"])
    first = st["iterations"] == 0
    st["iterations"] += 1
    tt, tq = pose_graph_perturb_ref(st["t"], st["q"], st["x"])
    rec = pose_graph_linearize_ref(tt, tq, ab, zt, zq, omega, free_mask, robust)
    D, g, cost = pose_graph_gather_ref(rec, ab, n, free_mask)
    if not cost < math.inf:
        st["status"] = 4
        return st
    if first or cost < st["cost"]:
        st.update(t=tt, q=tq, rec=rec, D=D, g=g, cost=cost)
        if first:
            st["initial_cost"] = cost
        else:
            st["accepted"] += 1
            lam = st["lam"] / 8.0
            st["lam"] = lam if lam > SCANREG_LAMBDA_MIN else SCANREG_LAMBDA_MIN
            if st["small"]:
                st["status"] = 1
                return st
    else:
        st["lam"] = st["lam"] * 8.0
        if st["lam"] > SCANREG_LAMBDA_MAX:
            st["status"] = 2
            return st
    cg = pose_graph_cg_ref(st["D"], st["g"], st["rec"], ab, st["lam"], free_mask, cg_iterations, cg_tol, tol_t, tol_r)
    st["x"] = cg["x"]                        # (all zero where the solve is degenerate: the kernels clear x before they factor)
    if cg["degenerate"]:
        st["status"] = 3
        return st
    st["small"] = cg["small"]
    st["cg_iterations"] += cg["iterations"]
    return st


def pose_graph_default_cg(n):
    return min(6 * int(n), 1000)


def pose_graph_optimize_ref(t, q, ab, zt, zq, omega, fixed=(), iterations=30, cg_iterations=None, cg_tol=1e-8, dof=63, robust=None, tol_t=1e-5,
                            tol_r=1e-6, snapshots=()):
    """`iterations` outer iterations from the starting nodes -> the state (pose_graph_start_ref's dict; chi2 = rec[:, 6] and weights =
    rec[:, 7] at the result).  With snapshots, a tuple of iteration counts: {count: a copy of the state after that many}, the last
    included, from one run."""
    import copy
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    free_mask = pose_graph_free_masks(len(t), fixed, dof)
    cg_iterations = pose_graph_default_cg(len(t)) if cg_iterations is None else int(cg_iterations)
    st = pose_graph_start_ref(t, q)
    shots = {}
    for it in range(1, int(iterations) + 1):
        pose_graph_step_ref(st, ab, zt, zq, omega, free_mask, cg_iterations, cg_tol, robust, tol_t, tol_r)
        if it in snapshots:
            shots[it] = copy.deepcopy(st)
    return shots if snapshots else st


def pose_graph_dense_ref(t, q, ab, zt, zq, omega, fixed=(), iterations=30, dof=63, robust=None, tol_t=1e-5, tol_r=1e-6):
    """The same Levenberg-Marquardt on a dense H, assembled with numpy's matrix products from pose_graph_jacobians_ref and solved with
    np.linalg.solve: the independent check of the block-sparse path (no fixed order, no conjugate gradients) -> dict(t, q, cost,
    initial_cost, iterations, accepted, status, lam)."""
    t = np.array(t, dtype=np.float64).reshape(-1, 3)
    q = np.array(q, dtype=np.float64).reshape(-1, 4)
    ab = np.asarray(ab, dtype=np.int64).reshape(-1, 2)
    n = len(t)
    free = np.concatenate([[(int(m) >> i) & 1 for i in range(6)] for m in pose_graph_free_masks(n, fixed, dof)]).astype(bool)
    O = pose_graph_omega_full(omega)

    def evaluate(t, q):
        e = pose_graph_residual_ref(t, q, ab, zt, zq)
        Ja, Jb = pose_graph_jacobians_ref(t, q, ab, zt, zq)
        s = np.einsum("ki,kij,kj->k", e, O, e)
        if robust is None:
            w, rho = np.ones(len(s)), s
        else:
            c2 = float(robust) ** 2
            w, rho = (c2 / (c2 + s)) ** 2, c2 * s / (c2 + s)
        H, g = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
        W = w[:, None, None] * O
        JW = {side: np.einsum("kji,kjl->kil", J, W) for side, J in ((0, Ja), (1, Jb))}             # J^T W per edge
        for k, (a, b) in enumerate(ab):
            blocks = [(b, 1, Jb[k])] + ([(a, 0, Ja[k])] if a >= 0 else [])
            for i, si, _ in blocks:
                g[6 * i:6 * i + 6] += JW[si][k] @ e[k]
                for j, _, Jj in blocks:
                    H[6 * i:6 * i + 6, 6 * j:6 * j + 6] += JW[si][k] @ Jj
        return float(rho.sum()), H, g

    lam, status, accepted, x = POSEGRAPH_LAMBDA0, 0, 0, np.zeros(6 * n)
    cost = initial = 0.0
    H = g = None
    done = 0
    for it in range(int(iterations)):
        done += 1
        tt, tq = pose_graph_perturb_ref(t, q, x.reshape(n, 6))
        c, Ht, gt = evaluate(tt, tq)
        if not np.isfinite(c):
            status = 4
            break
        if it == 0 or c < cost:
            t, q, cost, H, g = tt, tq, c, Ht, gt
            if it == 0:
                initial = c
            else:
                accepted += 1
                lam = max(lam / 8.0, SCANREG_LAMBDA_MIN)
                xs = np.abs(x.reshape(n, 6))
                if (xs[:, :3] <= tol_t).all() and (xs[:, 3:] <= tol_r).all():
                    status = 1
                    break
        else:
            lam *= 8.0
            if lam > SCANREG_LAMBDA_MAX:
                status = 2
                break
        A = H + lam * np.diag(np.diag(H))
        x = np.zeros(6 * n)
        sub = A[np.ix_(free, free)]
        try:
            x[free] = np.linalg.solve(sub, -g[free])
        except np.linalg.LinAlgError:
            status = 3
            break
    return dict(t=t, q=q, cost=cost, initial_cost=initial, iterations=done, accepted=accepted, status=status, lam=lam)


def _quat_mul_np(p, q):
    return np.stack(_pg_qmul(tuple(np.asarray(p, dtype=np.float64).T), tuple(np.asarray(q, dtype=np.float64).T)), axis=-1)


def pose_graph_relative_ref(ta, qa, tb, qb):
    """The relative pose of b seen from a in an edge's convention: (R_a^T (t_b - t_a), conj(q_a) (x) q_b normalised)."""
    qa, qb = np.asarray(qa, dtype=np.float64), np.asarray(qb, dtype=np.float64)
    R = np.asarray(_pg_rot(tuple(qa.T)))
    if R.ndim == 3:
        R = np.moveaxis(R, -1, 0)
    d = np.asarray(tb, dtype=np.float64) - np.asarray(ta, dtype=np.float64)
    dt = np.einsum("...ji,...j->...i", R, d)
    dq = _quat_mul_np(qa * np.asarray([1.0, -1.0, -1.0, -1.0]), qb)
    return dt, dq / np.sqrt((dq * dq).sum(axis=-1, keepdims=True))


def pose_graph_loop(n, laps=1, sigma_t=0.02, sigma_r=0.01, closures=4, seed=0, radius=5.0):
    """A ground-truth loop with drifting odometry and closure edges -> dict(truth_t (N,3), truth_q (N,4), t (N,3), q (N,4): the
    dead-reckoned start; ab (E,2) int32, zt (E,3), zq (E,4), omega (E,21), n_odometry): N = n laps nodes on a circle of `radius` in the
    plane z = 0, heading along the tangent, with a gentle roll and pitch so that all six degrees of freedom are exercised; N - 1 odometry
    edges, each the true relative pose with Gaussian noise (sigma_t metres, sigma_r radians per axis) AND a constant bias of sigma_t / 2 in
    x and sigma_r / 2 in yaw, the drift; `closures` edges of the true relative pose with a fifth of the noise, between node i and node
    i + n (laps - 1) (the same place on the last lap; with laps = 1 between the start's and the end's neighbourhoods).  Omega is
    diag(1 / sigma^2) of each edge's own noise.  Node 0 is exact: fix it."""
    rng = np.random.default_rng(seed)
    N = int(n) * int(laps)
    ang = 2.0 * np.pi * np.arange(N) / n
    truth_t = np.stack([radius * np.cos(ang), radius * np.sin(ang), 0.2 * np.sin(2.0 * ang)], axis=1)
    yaw, roll, pitch = ang + np.pi / 2.0, 0.05 * np.sin(ang), 0.05 * np.cos(ang)
    qz = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], axis=1)
    qy = np.stack([np.cos(pitch / 2), 0 * yaw, np.sin(pitch / 2), 0 * yaw], axis=1)
    qx = np.stack([np.cos(roll / 2), np.sin(roll / 2), 0 * yaw, 0 * yaw], axis=1)
    truth_q = _quat_mul_np(qz, _quat_mul_np(qy, qx))

    def noisy(a, b, st, sr, bias):
        dt, dq = pose_graph_relative_ref(truth_t[a], truth_q[a], truth_t[b], truth_q[b])
        m = len(a)
        dt = dt + st * rng.standard_normal((m, 3)) + bias * np.asarray([0.5 * st, 0.0, 0.0])
        h = 0.5 * (sr * rng.standard_normal((m, 3)) + bias * np.asarray([0.0, 0.0, 0.5 * sr]))
        dq = _quat_mul_np(np.concatenate([np.ones((m, 1)), h], axis=1), dq)
        om = np.zeros((m, 21))
        for k, (i, j) in enumerate(_PG_TRIU):
            if i == j:
                om[:, k] = 1.0 / (st * st) if i < 3 else 1.0 / (sr * sr)
        return dt, dq, om

    a = np.arange(N - 1)
    ot, oq, oo = noisy(a, a + 1, sigma_t, sigma_r, 1.0)
    if laps > 1:
        ca = (np.arange(closures) * n) // max(closures, 1) + n // (2 * max(closures, 1))
        cb = ca + n * (laps - 1)
    else:
        ca = np.arange(closures)
        cb = N - 1 - np.arange(closures)
    ct, cq, co = noisy(ca, cb, sigma_t / 5.0, sigma_r / 5.0, 0.0)
    t, q = np.zeros((N, 3)), np.zeros((N, 4))
    t[0], q[0] = truth_t[0], truth_q[0]
    for i in range(N - 1):                                   # dead reckoning: t_b = t_a + R_a z_t, q_b = q_a (x) z_q
        R = np.asarray(_pg_rot(tuple(q[i])))
        t[i + 1] = t[i] + R @ ot[i]
        q[i + 1] = _quat_mul_np(q[i], oq[i])
    return dict(truth_t=truth_t, truth_q=truth_q, t=t, q=q, ab=np.concatenate([np.stack([a, a + 1], axis=1), np.stack([ca, cb], axis=1)]).astype(np.int32),
                zt=np.concatenate([ot, ct]), zq=np.concatenate([oq, cq]), omega=np.concatenate([oo, co]), n_odometry=N - 1)


# ---- the particle filter restated in numpy ("Particle filter"): what particle_kernels.hip must give, bit for bit ------
MCL_MAX_N = 1 << 20
MCL_CLAMP = (1 << 24) - 1
MCL_FLOOR = -(1 << 40)
MCL_MAX_SIGMA_Q8 = 1 << 24
MCL_TURN = 16384
MCL_RECORD = 16
MCL_RECORD_FIELDS = ("s1", "s2", "sum_x", "sum_y", "sum_z", "sum_cos", "sum_sin", "best", "best_score", "best_known", "best_used", "verdict",
                     "n_eff_bits", "max_log_weight", "n", "zero")
MCL_GAUSS_WORD, MCL_EXP2_WORD, MCL_TABLE_WORDS = 32768, 33796, 34052
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_ref(counter, key, rounds=10):
    """Philox4x32 (Salmon et al. 2011): counter = four 32-bit words, key = two, each a number or an array (broadcast) -> (..., 4)
    uint32.  Multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _M32 for v in key]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0, k1 = k
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _mcl_words(n, step, stream, seed):
    """The four words of particles 0 .. n - 1 -> (n, 4) int64: key (seed's low and high 32 bits), counter (i, 0, step, stream)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_ref((np.arange(n), 0, int(step) & 0xFFFFFFFF, stream), (seed & 0xFFFFFFFF, seed >> 32)).astype(np.int64)


def _norm_ppf(p):
    """The standard normal's quantile by bisection on erfc, in f64 (no scipy)."""
    lo, hi = -9.0, 9.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(-mid / math.sqrt(2.0)) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def mcl_trig_table():
    """TRIG (16384, 2) int32: round(32768 cos), round(32768 sin) of 2 pi h / 16384."""
    a = 2.0 * np.pi * np.arange(MCL_TURN, dtype=np.float64) / MCL_TURN
    return np.stack([np.rint(32768.0 * np.cos(a)), np.rint(32768.0 * np.sin(a))], axis=1).astype(np.int32)


def mcl_gauss_table():
    """GAUSS (1025,) int32: round(4096 Phi^-1((i + 0.5) / 1025)), a Q12 standard normal at 1025 knots."""
    return np.array([int(round(4096.0 * _norm_ppf((i + 0.5) / 1025.0))) for i in range(1025)], dtype=np.int32)


def mcl_exp2_table():
    """EXP2 (256,) int32: round(2^20 2^(-j / 256))."""
    return np.rint(2.0 ** 20 * 2.0 ** (-np.arange(256, dtype=np.float64) / 256.0)).astype(np.int32)


_MCL_TABLES = {}


def mcl_tables_ref():
    """-> (TRIG, GAUSS, EXP2), built once."""
    if not _MCL_TABLES:
        _MCL_TABLES["t"] = (mcl_trig_table(), mcl_gauss_table(), mcl_exp2_table())
    return _MCL_TABLES["t"]


def mcl_table_words_ref():
    """The tables as the one int32 buffer the kernels take: TRIG at word 0, GAUSS at 32768, EXP2 at 33796; 34052 words."""
    trig, gauss, exp2 = mcl_tables_ref()
    words = np.zeros(MCL_TABLE_WORDS, dtype=np.int32)
    words[:2 * MCL_TURN] = trig.reshape(-1)
    words[MCL_GAUSS_WORD:MCL_GAUSS_WORD + 1025] = gauss
    words[MCL_EXP2_WORD:MCL_EXP2_WORD + 256] = exp2
    return words


def mcl_sigma_q8(sigma):
    """sigma in state units -> round(256 sigma), an int in [0, 2^24]."""
    q = np.rint(256.0 * np.asarray(sigma, dtype=np.float64)).astype(np.int64)
    if (q < 0).any() or (q > MCL_MAX_SIGMA_Q8).any():
        raise ValueError(f"sigma must lie in [0, 65536] state units, got {sigma!r}")
    return q


def mcl_gauss_ref(u):
    """32-bit words -> the Q12 standard normal g: i = u >> 22, f = (u >> 6) & 0xFFFF, (GAUSS[i] (65536 - f) + GAUSS[i + 1] f) >> 16."""
    gauss = mcl_tables_ref()[1].astype(np.int64)
    u = np.asarray(u, dtype=np.int64)
    i, f = u >> 22, (u >> 6) & 0xFFFF
    return (gauss[i] * (65536 - f) + gauss[i + 1] * f) >> 16


def mcl_noise_ref(u, sigma_q8):
    """noise(u, sigma) = (g sigma_q8 + 2^19) >> 20, state units (arithmetic shift)."""
    return (mcl_gauss_ref(u) * np.asarray(sigma_q8, dtype=np.int64) + (1 << 19)) >> 20


def mcl_seed_gaussian_ref(n, prior, sigma_q8, seed=0, step=0):
    """-> state (n, 4) int32: clamp(prior_a + noise(word_a, sigma_a)) for x, y, z; (prior_h + noise) mod 16384.  Stream 0."""
    u = _mcl_words(n, step, 0, seed)
    s = np.asarray(prior, dtype=np.int64).reshape(1, 4) + mcl_noise_ref(u, np.asarray(sigma_q8, dtype=np.int64).reshape(1, 4))
    s[:, :3] = np.clip(s[:, :3], -MCL_CLAMP, MCL_CLAMP)
    s[:, 3] %= MCL_TURN
    return s.astype(np.int32)


def mcl_seed_positions_ref(n, positions, origin, resolution, jitter=True, seed=0, step=0):
    """-> state (n, 4) int32: particle i takes row word0 mod M of the world positions (M, 3): the voxel it lies in (occ_fixed's rule),
    at 1/256 offsets word1 >> 24, (word1 >> 16) & 255, word2 >> 24 (128 each without jitter); heading word3 >> 18.  Stream 3."""
    P = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    u = _mcl_words(n, step, 3, seed)
    q, _ = occ_fixed(P[u[:, 0] % P.shape[0]], origin, resolution)
    j = np.stack([u[:, 1] >> 24, (u[:, 1] >> 16) & 0xFF, u[:, 2] >> 24], axis=1) if jitter else np.full((n, 3), 128, dtype=np.int64)
    return np.concatenate([(q >> 8) * 256 + j, (u[:, 3] >> 18)[:, None]], axis=1).astype(np.int32)


def mcl_predict_ref(state, delta, sigma_q8, seed=0, step=1):
    """One motion update -> the new state (n, 4) int32.  n_a = delta_a + noise(word_a, sigma_a); (c, s) = TRIG[h]; X += (c n_x - s n_y +
    2^14) >> 15, Y += (s n_x + c n_y + 2^14) >> 15, Z += n_z, clamped; h = (h + n_h) mod 16384.  Stream 1."""
    s = np.asarray(state, dtype=np.int64).copy()
    u = _mcl_words(s.shape[0], step, 1, seed)
    nz = np.asarray(delta, dtype=np.int64).reshape(1, 4) + mcl_noise_ref(u, np.asarray(sigma_q8, dtype=np.int64).reshape(1, 4))
    trig = mcl_tables_ref()[0].astype(np.int64)[s[:, 3] % MCL_TURN]
    c, sn = trig[:, 0], trig[:, 1]
    s[:, 0] += (c * nz[:, 0] - sn * nz[:, 1] + (1 << 14)) >> 15
    s[:, 1] += (sn * nz[:, 0] + c * nz[:, 1] + (1 << 14)) >> 15
    s[:, 2] += nz[:, 2]
    s[:, :3] = np.clip(s[:, :3], -MCL_CLAMP, MCL_CLAMP)
    s[:, 3] = (s[:, 3] % MCL_TURN + nz[:, 3]) % MCL_TURN
    return s.astype(np.int32)


def mcl_poses_ref(state, origin, resolution, attitude=None):
    """-> (n, 12) f32, scan matching's pose of each particle: R = Rz(h) A in f32 — c32 = f32(c) 2^-15; row 0 fl(fl(c32 A_0j) - fl(s32
    A_1j)), row 1 fl(fl(s32 A_0j) + fl(c32 A_1j)), row 2 A_2j — and t_a = fl(fl(f32(X_a) f32(resolution / 256)) + origin_a)."""
    f32 = np.float32
    s = np.asarray(state, dtype=np.int64)
    A = np.eye(3, dtype=f32) if attitude is None else np.asarray(attitude, dtype=f32).reshape(3, 3)
    trig = mcl_tables_ref()[0][s[:, 3] % MCL_TURN].astype(f32) * f32(2.0 ** -15)
    c, sn = trig[:, 0:1], trig[:, 1:2]
    r0 = ((c * A[0][None, :]).astype(f32) - (sn * A[1][None, :]).astype(f32)).astype(f32)
    r1 = ((sn * A[0][None, :]).astype(f32) + (c * A[1][None, :]).astype(f32)).astype(f32)
    r2 = np.broadcast_to(A[2][None, :], r0.shape)
    r256 = f32(f32(resolution) / f32(256.0))
    t = ((s[:, :3].astype(f32) * r256).astype(f32) + np.asarray(origin, dtype=f32).reshape(1, 3)).astype(f32)
    return np.ascontiguousarray(np.concatenate([r0, r1, r2, t], axis=1), dtype=f32)


def mcl_weigh_ref(L, origin, resolution, points, state, attitude=None, floor=None, unknown_value=0, chunk=128):
    """-> (score, used, known), each (n,) int32: scan matching's score, used and known of the scan at every particle's pose (zero
    shift), by scan_score_ref's rules, `chunk` particles at a time."""
    f32 = np.float32
    L = np.asarray(L, dtype=np.int64)
    V = scan_values_ref(L, floor, unknown_value)
    P = np.asarray(points, dtype=f32).reshape(-1, 3)
    T = mcl_poses_ref(state, origin, resolution, attitude)
    n = T.shape[0]
    score, used, known = (np.zeros(n, dtype=np.int64) for _ in range(3))
    dims = np.asarray(L.shape)
    for a in range(0, n, chunk):
        Tc = T[a:a + chunk]
        with np.errstate(all="ignore"):
            cols = []
            for ax in range(3):
                w = ((Tc[:, 3 * ax, None] * P[None, :, 0]).astype(f32) + (Tc[:, 3 * ax + 1, None] * P[None, :, 1]).astype(f32)).astype(f32)
                w = (w + (Tc[:, 3 * ax + 2, None] * P[None, :, 2]).astype(f32)).astype(f32)
                cols.append((w + Tc[:, 9 + ax, None]).astype(f32))
            W = np.stack(cols, axis=2)
        q, ok = occ_fixed(W.reshape(-1, 3), origin, resolution)
        v = (q >> 8).reshape(W.shape)
        ok = ok.reshape(W.shape[:2])
        ins = ok & ((v >= 0) & (v < dims[None, None, :])).all(axis=2)
        vc = np.where(ins[:, :, None], v, 0)
        Lp = L[vc[:, :, 0], vc[:, :, 1], vc[:, :, 2]]
        kn = ins & (Lp != EVID_UNKNOWN)
        val = np.where(ins, V[vc[:, :, 0], vc[:, :, 1], vc[:, :, 2]], int(unknown_value))
        score[a:a + chunk] = np.where(ok, val, 0).sum(axis=1)
        used[a:a + chunk] = ok.sum(axis=1)
        known[a:a + chunk] = kn.sum(axis=1)
    return score.astype(np.int32), used.astype(np.int32), known.astype(np.int32)


def mcl_weight_ref(log_weight):
    """Normalised log-weights (<= 0) -> w int64: d = -log_weight, EXP2[(d & 0xFFFF) >> 8] >> (d >> 16) where d >> 16 <= 20, else 0."""
    d = -np.asarray(log_weight, dtype=np.int64)
    q = d >> 16
    e = mcl_tables_ref()[2].astype(np.int64)[(d & 0xFFFF) >> 8]
    return np.where(q <= 20, e >> np.minimum(q, 20), 0)


def mcl_n_eff(s1, s2):
    """f64(S1) f64(S1) / f64(S2): one conversion each, one multiply, one divide."""
    return float(int(s1)) * float(int(s1)) / float(int(s2))


def mcl_weights_ref(state, log_weight, score=None, beta_q=256, threshold=0.0, used=None, known=None):
    """One weight update -> (log_weight (n,) int64, w (n,) int64, record (16,) int64): log_weight += score beta_q (score None: nothing
    added), the maximum subtracted, the floor -2^40 applied, the weights, and the record MCL_RECORD_FIELDS names.  The integer sums
    wrap modulo 2^64 as the device's do."""
    s = np.asarray(state, dtype=np.int64)
    lw = np.asarray(log_weight, dtype=np.int64).copy()
    if score is not None:
        lw = lw + np.asarray(score, dtype=np.int64) * int(beta_q)
    m = int(lw.max())
    lw = np.maximum(lw - m, MCL_FLOOR)
    w = mcl_weight_ref(lw)
    trig = mcl_tables_ref()[0].astype(np.int64)[s[:, 3] % MCL_TURN]
    with np.errstate(over="ignore"):
        sums = [w.sum(), (w * w).sum(), (w * s[:, 0]).sum(), (w * s[:, 1]).sum(), (w * s[:, 2]).sum(), (w * trig[:, 0]).sum(), (w * trig[:, 1]).sum()]
    best = int(np.flatnonzero(lw == 0)[0])
    n_eff = mcl_n_eff(sums[0], sums[1])
    pick = lambda a: 0 if a is None else int(np.asarray(a)[best])   # noqa: E731
    rec = [int(v) for v in sums] + [best, pick(score), pick(known), pick(used), int(n_eff < float(threshold)),
                                    int(np.float64(n_eff).view(np.int64)), m, s.shape[0], 0]
    return lw, w, np.array(rec, dtype=np.int64)


def mcl_ancestors_ref(w, r):
    """The systematic resample -> ancestors (n,) int64: t_j = (j S1 + r) div n, a_j = the least i with C_i > t_j, C the inclusive prefix
    sum of w; r in [0, S1)."""
    w = np.asarray(w, dtype=np.uint64)
    n = w.shape[0]
    C = np.cumsum(w, dtype=np.uint64)
    s1 = int(C[-1])
    if not 0 <= int(r) < s1 or n * s1 + s1 >= 1 << 64:
        raise ValueError("r must lie in [0, S1) and n S1 fit 64 bits")
    t = (np.arange(n, dtype=np.uint64) * np.uint64(s1) + np.uint64(int(r))) // np.uint64(n)
    return np.searchsorted(C, t, side="right").astype(np.int64)


def mcl_resample_ref(state, log_weight, w, threshold, seed=0, step=0):
    """-> (state, log_weight, ancestors (n,) int32, verdict): resample iff n_eff < threshold, with r = (word0 2^32 + word1) mod S1 of the
    words of counter (0, 0, step, 2); otherwise the state and the log-weights as they are and the identity."""
    s, lw, w = np.asarray(state, dtype=np.int32), np.asarray(log_weight, dtype=np.int64), np.asarray(w, dtype=np.int64)
    s1, s2 = int(w.sum()), int((w * w).sum())
    if not mcl_n_eff(s1, s2) < float(threshold):
        return s.copy(), lw.copy(), np.arange(s.shape[0], dtype=np.int32), 0
    u = _mcl_words(1, step, 2, seed)[0]
    a = mcl_ancestors_ref(w, ((int(u[0]) << 32) + int(u[1])) % s1)
    return s[a].copy(), np.zeros_like(lw), a.astype(np.int32), 1


def mcl_estimate_ref(record, origin, resolution):
    """The record -> dict: mean position (world, f64: origin + resolution (sum / S1) / 256), mean heading (radians, atan2 of the two
    sums), n_eff, best index."""
    rec = dict(zip(MCL_RECORD_FIELDS, (int(v) for v in record)))
    mean = np.array([rec["sum_x"], rec["sum_y"], rec["sum_z"]], dtype=np.float64) / float(rec["s1"])
    return dict(state=mean, position=np.asarray(origin, dtype=np.float64) + float(resolution) * mean / 256.0,
                yaw=math.atan2(float(rec["sum_sin"]), float(rec["sum_cos"])), n_eff=mcl_n_eff(rec["s1"], rec["s2"]), best=rec["best"])


def mcl_state_units(pose, yaw, origin, resolution):
    """A world position (3,) and a heading in radians -> the four state integers: round(256 (p - origin) / resolution), round(16384 yaw
    / 2 pi) mod 16384, in f64."""
    p = np.rint(256.0 * (np.asarray(pose, dtype=np.float64).reshape(3) - np.asarray(origin, dtype=np.float64).reshape(3)) / float(resolution))
    return [int(v) for v in p] + [int(round(MCL_TURN * float(yaw) / (2.0 * math.pi))) % MCL_TURN]


def mcl_filter_ref(L, origin, resolution, scans, deltas, sigmas_q8, prior, prior_sigma_q8, n, seed=0, beta_q=256, ratio=0.5, floor=None,
                   unknown_value=0, attitude=None):
    """The whole loop restated: seed_gaussian at step 0, then per scan predict (step k + 1) -> weigh -> weights -> resample.  deltas
    (K, 4) in state units, sigmas_q8 (4,) -> a list of dicts: state and log_weight after the update, record, ancestors, score."""
    state = mcl_seed_gaussian_ref(n, prior, prior_sigma_q8, seed, 0)
    lw = np.zeros(n, dtype=np.int64)
    out = []
    for k, pts in enumerate(scans):
        step = k + 1
        state = mcl_predict_ref(state, deltas[k], sigmas_q8, seed, step)
        score, used, known = mcl_weigh_ref(L, origin, resolution, pts, state, attitude, floor, unknown_value)
        lw, w, rec = mcl_weights_ref(state, lw, score, beta_q, ratio * n, used, known)
        weighed = state
        state, lw, anc, verdict = mcl_resample_ref(state, lw, w, ratio * n, seed, step)
        assert verdict == rec[11]
        out.append(dict(state=state, log_weight=lw, record=rec, ancestors=anc, score=score, weighed_state=weighed, weights=w))
    return out
