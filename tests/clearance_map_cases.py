"""The clearance term asked of the map, restated in numpy (no GPU, no library): float32 op by op, brute force over every obstacle
voxel, the 64-bit key and its tie rule, the float64 finish — and the grids and queries the CPU and GPU tests share.

An obstacle voxel (x, y, z) is the point fl(o_a + fl(fl(i_a + 0.5) r)) per axis; its index is lin = (z ny + y) nx + x.  The winner of a
query is the smallest key (float bits of d2) << 32 | lin over d2 < fl(r r)."""
import numpy as np

f32, f64 = np.float32, np.float64

# case 1's grid: partial bricks on every far face (bricks are 4 x 4 x 2), an origin that is no multiple of the resolution
DIMS, RES, ORIGIN = (13, 10, 7), 0.1, (0.23, -0.41, 0.07)
RADII = (0.04, 0.25, 1.0)


def centres(ijk, origin=ORIGIN, res=RES):
    """(n, 3) integer voxels -> (n, 3) float32 centres, export's arithmetic."""
    ijk = np.asarray(ijk).reshape(-1, 3)
    o, r = np.asarray(origin, f32), f32(res)
    return (o[None, :] + ((ijk.astype(f32) + f32(0.5)) * r).astype(f32)).astype(f32)


def linear(ijk, dims=DIMS):
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    return (ijk[:, 2] * dims[1] + ijk[:, 1]) * dims[0] + ijk[:, 0]


def obstacles(occupied, free=None, origin=ORIGIN, res=RES):
    """occupied, free: bool (nx, ny, nz) arrays -> (lin (n,) ascending, C (n, 3) f32): the obstacle voxels — occupied, and with a
    free plane those of neither bit as well."""
    mask = np.asarray(occupied, bool) if free is None else (np.asarray(occupied, bool) | ~np.asarray(free, bool))
    ijk = np.argwhere(mask)
    lin = linear(ijk, mask.shape)
    order = np.argsort(lin)
    return lin[order], centres(ijk[order], origin, res)


def point_d2(t, C):
    t = np.asarray(t, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (t[0] - C[:, 0]).astype(f32), (t[1] - C[:, 1]).astype(f32), (t[2] - C[:, 2]).astype(f32)
        return ((dx * dx + dy * dy).astype(f32) + dz * dz).astype(f32)


def segment_d2(a, b, C):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = (b - a).astype(f32)
        ee = f32(f32(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        inv = f32(1.0) / ee if ee > 0 else f32(0.0)
        ux, uy, uz = (C[:, 0] - a[0]).astype(f32), (C[:, 1] - a[1]).astype(f32), (C[:, 2] - a[2]).astype(f32)
        dot = ((ux * e[0] + uy * e[1]).astype(f32) + uz * e[2]).astype(f32)
        s = np.fmin(np.fmax((dot * inv).astype(f32), f32(0.0)), f32(1.0)).astype(f32)
        qx, qy, qz = (ux - s * e[0]).astype(f32), (uy - s * e[1]).astype(f32), (uz - s * e[2]).astype(f32)
        return ((qx * qx + qy * qy).astype(f32) + qz * qz).astype(f32)


def winner(d2, lin, r):
    """-> (row of the winner in lin / C, or -1; its d2): the smallest key over d2 < fl(r r)."""
    r2 = f32(r) * f32(r)
    hit = np.flatnonzero(d2 < r2)
    if hit.size == 0:
        return -1, f32(np.inf)
    key = (d2[hit].view(np.uint32).astype(np.uint64) << np.uint64(32)) | lin[hit].astype(np.uint64)
    k = int(hit[int(np.argmin(key))])
    return k, d2[k]


def query_points(lin, C, q, r, w=0.0):
    """The point query -> dict(d (n,) f32, idx (n,) int32 linear indices, term (n,) f64, grad (n, 3) f32, value f32)."""
    q = np.asarray(q, f32).reshape(-1, 3)
    n = len(q)
    d, idx, term, grad = np.full(n, np.inf, f32), np.full(n, -1, np.int32), np.zeros(n, f64), np.zeros((n, 3), f32)
    r64, w64 = f64(f32(r)), f64(f32(w))
    for i, t in enumerate(q):
        if not np.isfinite(t).all() or len(lin) == 0:
            continue
        k, d2 = winner(point_d2(t, C), lin, r)
        if k < 0:
            continue
        dd = np.sqrt(f64(d2))
        h = r64 - dd
        d[i], idx[i], term[i] = f32(dd), lin[k], h * h
        if dd > 0.0:
            c = -2.0 * w64 * h
            grad[i] = (c * (t.astype(f64) - C[k].astype(f64)) / dd).astype(f32)
    return dict(d=d, idx=idx, term=term, grad=grad, value=f32(w64 * _sum(term)))


def _sum(terms):
    s = f64(0.0)
    for t in terms:
        s = s + t
    return s


def query_segments(lin, C, poses, r, w=0.0, n_traj=1):
    """The segment query of n_traj trajectories laid end to end -> dict(d, idx, s (n_traj (W-1),), term (n_traj W,) f64, grad
    (n_traj W, 3) f32, value (n_traj,) f32)."""
    P = np.asarray(poses, f32).reshape(-1, 3)
    W = len(P) // n_traj
    ns = n_traj * (W - 1)
    d, idx, s = np.full(ns, np.inf, f32), np.full(ns, -1, np.int32), np.zeros(ns, f32)
    term, part = np.zeros(n_traj * W, f64), np.zeros((ns, 6), f64)
    r64, w64 = f64(f32(r)), f64(f32(w))
    for seg in range(ns):
        row = seg // (W - 1) * W + seg % (W - 1)
        a, b = P[row], P[row + 1]
        if not (np.isfinite(a).all() and np.isfinite(b).all()) or len(lin) == 0:
            continue
        k, d2 = winner(segment_d2(a, b, C), lin, r)
        if k < 0:
            continue
        dd = np.sqrt(f64(d2))
        a64, e, u = a.astype(f64), b.astype(f64) - a.astype(f64), C[k].astype(f64) - a.astype(f64)
        ee = (f64(0.0) + e[0] * e[0]) + e[1] * e[1] + e[2] * e[2]
        dot = (f64(0.0) + u[0] * e[0]) + u[1] * e[1] + u[2] * e[2]
        t = min(max(dot / ee, 0.0), 1.0) if ee > 0.0 else 0.0
        v = t * e - u
        h = r64 - dd
        d[seg], idx[seg], s[seg], term[row] = f32(dd), lin[k], f32(t), h * h
        vv = (f64(0.0) + v[0] * v[0]) + v[1] * v[1] + v[2] * v[2]
        if vv > 0.0:
            c = -2.0 * w64 * h / np.sqrt(vv)
            part[seg, :3], part[seg, 3:] = c * (1.0 - t) * v, c * t * v
    grad = np.zeros((n_traj * W, 3), f32)
    for row in range(n_traj * W):
        wp = row % W
        seg = row // W * (W - 1) + wp
        gb = part[seg - 1, 3:] if wp > 0 else np.zeros(3)
        ga = part[seg, :3] if wp < W - 1 else np.zeros(3)
        grad[row] = (gb + ga).astype(f32)
    value = np.array([f32(w64 * _sum(term[b * W:(b + 1) * W])) for b in range(n_traj)], f32)
    return dict(d=d, idx=idx, s=s, term=term, grad=grad, value=value)


def window(lo, hi, r, origin, res, dims):
    """The bricks a query's window covers, restated for PLACING obstacles (no result depends on it): per axis [first, first + n)."""
    out = []
    for a, per in ((0, 4), (1, 4), (2, 2)):
        nb = (dims[a] + per - 1) // per
        o, rr = f32(origin[a]), f32(res)
        v0 = (f32(lo[a]) - f32(r) - o) / rr - f32(1.0)
        v1 = (f32(hi[a]) + f32(r) - o) / rr + f32(1.0)
        b0 = int(min(max(np.floor(v0 / f32(per)), 0), nb))
        b1 = int(min(max(np.floor(v1 / f32(per)) + 1, 0), nb))
        out.append((b0, max(b1 - b0, 0)))
    return out


# ---- the hand-computed case: a waypoint on the corner shared by eight occupied voxels ---------------------------------------------
HAND = dict(dims=(3, 3, 3), res=1.0, origin=(0.0, 0.0, 0.0), t=(1.0, 1.0, 1.0), r=1.0, w=2.0)


def hand_grid():
    occ = np.zeros(HAND["dims"], bool)
    occ[:2, :2, :2] = True
    return occ


# ---- case 1: about 40 occupied voxels in 13 x 10 x 7 -------------------------------------------------------------------------------
BLOCK = (3, 3, 5)       # the 2 x 2 x 2 occupied block whose shared corner and faces give the ties (chosen so that they are exact: below)
BOUNDARY = (12, 5, 3)   # an occupied voxel on the far x face
LONE = (9, 3, 5)        # an occupied voxel with no other within 0.3 m: the strict '<' at r = 0.04 and 0.25


def case1_voxels():
    rng = np.random.default_rng(7)
    vox = {(12, 0, 0), (0, 9, 0), (0, 0, 6), (12, 9, 6), BOUNDARY, LONE, (12, 9, 0), (6, 9, 2), (5, 4, 6), (12, 2, 6), (3, 8, 6), (0, 0, 0)}
    vox |= {(BLOCK[0] + i, BLOCK[1] + j, BLOCK[2] + k) for i in (0, 1) for j in (0, 1) for k in (0, 1)}
    while len(vox) < 40:
        v = tuple(int(c) for c in rng.integers(0, DIMS))
        if max(abs(v[a] - LONE[a]) for a in range(3)) > 3:
            vox.add(v)
    return np.array(sorted(vox), np.int64)


def dense(vox, dims=DIMS):
    m = np.zeros(dims, bool)
    m[tuple(np.asarray(vox).T)] = True
    return m


def at_exactly(c, r):
    """A query at distance exactly fl(r) from the centre c along one axis: t with fl(t_a - c_a) == +-fl(r) in float32, or None."""
    for a in range(3):
        for sign in (1.0, -1.0):
            t = c.copy()
            t[a] = f32(c[a] + f32(sign) * f32(r))
            if f32(t[a] - c[a]) == f32(sign) * f32(r):
                return t
    return None


def case1_points(r):
    """The point queries of case 1 for radius r -> (names, (n, 3) f32)."""
    vox = case1_voxels()
    C = centres(vox)
    by = {tuple(v): c for v, c in zip(vox.tolist(), C)}
    lo, hi = by[BLOCK], by[(BLOCK[0] + 1, BLOCK[1] + 1, BLOCK[2] + 1)]
    corner = ((lo + hi) * f32(0.5)).astype(f32)
    face = np.array([corner[0], lo[1], lo[2]], f32)
    exact = at_exactly(by[LONE], r)
    assert exact is not None, r
    q = [("interior", (0.71, 0.03, 0.36)), ("corner", corner), ("face", face), ("own centre", by[(6, 9, 2)]), ("exactly r", exact),
         ("outside dims", by[BOUNDARY] + np.array([0.08, 0.0, 0.0], f32)), ("1e6", (1e6, 0.0, 0.0)), ("1e30", (0.5, -1e30, 0.2)),
         ("nan", (0.5, np.nan, 0.2)), ("inf", (np.inf, 0.0, 0.2)), ("interior 2", (1.02, 0.31, 0.58)), ("below", (0.3, -0.38, 0.01))]
    return [n for n, _ in q], np.array([np.asarray(p, f32) for _, p in q], f32)


def case1_paths(r):
    """Two sets of n_traj = 2 trajectories of W = 4 waypoints, (8, 3) f32 each.  Set 0: a degenerate segment D -> D, and the last
    waypoint of trajectory 0 (D) and the first of trajectory 1 (E) straddling the LONE voxel — a segment D -> E would pass through its
    centre — then a waypoint outside dims.  Set 1: a waypoint 1e6 m away, a NaN row and one 1e30 m away."""
    c = centres([LONE])[0]
    off = np.array([max(1.5 * r, 0.06), 0.0, 0.0], f32)
    D, E = (c - off).astype(f32), (c + off).astype(f32)
    out = centres([BOUNDARY])[0] + np.array([0.08, 0.02, 0.0], f32)
    s0 = np.array([(0.71, 0.03, 0.36), (0.6, 0.1, 0.3), D, D, E, out, (1.02, 0.31, 0.58), (0.8, 0.4, 0.2)], f32)
    s1 = np.array([(0.4, -0.2, 0.3), (1e6, 0.0, 0.0), (0.9, 0.2, 0.5), (np.nan, 0.2, 0.3),
                   (0.3, -0.3, 0.1), (0.5, 0.0, 0.6), (0.5, 1e30, 0.6), (1.2, 0.4, 0.65)], f32)
    return [s0, s1]
