"""numpy restatement of the nearest-depth sphere splat of trajectory_optimization_amd/csrc/render_kernels.hip
(TEST INFRASTRUCTURE ONLY).  The reference's renderer is pytorch3d pulsar (/root/reference/src/tools.py:147-172),
third-party CUDA absent from the tree and the image: PARITY UNPINNED — this pins the build's own specification."""
import numpy as np


def render_points(verts, K, height, width, radius=0.03, znear=1.0, zfar=10.0, background=1.0):
    v = np.asarray(verts, np.float32)
    fx, cx, fy, cy = (np.float32(K[0][0]), np.float32(K[0][2]), np.float32(K[1][1]), np.float32(K[1][2]))
    H, W = int(height), int(width)
    zbuf = np.full((H, W), np.inf, np.float32)
    owner = np.full((H, W), -1, np.int64)
    # the rows inside the depth range with finite X and Y, in index order: a row outside it (a NaN depth included) splats nothing, and
    # neither does one whose projection is not finite (the kernels' `u + rho >= 0 && u - rho <= width` is false for it)
    with np.errstate(invalid="ignore"):
        live = (v[:, 2] >= np.float32(znear)) & (v[:, 2] <= np.float32(zfar)) & np.isfinite(v[:, 0]) & np.isfinite(v[:, 1])
    for i in np.flatnonzero(live):
        X, Y, Z = v[i]
        with np.errstate(over="ignore"):
            u, w_ = fx * X / Z + cx, fy * Y / Z + cy
        rho = fx * np.float32(radius) / Z
        if not (np.isfinite(u) and np.isfinite(w_)):   # (fx X overflowed)
            continue
        j0, j1 = max(0, int(np.floor(u - rho - np.float32(0.5)))), min(W - 1, int(np.ceil(u + rho - np.float32(0.5))))
        i0, i1 = max(0, int(np.floor(w_ - rho - np.float32(0.5)))), min(H - 1, int(np.ceil(w_ + rho - np.float32(0.5))))
        if j1 < j0 or i1 < i0:
            continue
        pj = np.arange(j0, j1 + 1, dtype=np.float32) + np.float32(0.5) - u
        pi = np.arange(i0, i1 + 1, dtype=np.float32) + np.float32(0.5) - w_
        inside = (pj[None, :] * pj[None, :] + pi[:, None] * pi[:, None]) <= rho * rho
        zb = zbuf[i0:i1 + 1, j0:j1 + 1]
        ow = owner[i0:i1 + 1, j0:j1 + 1]
        win = inside & ((Z < zb) | ((Z == zb) & (i < ow)))
        zb[win] = Z
        ow[win] = i
    img = np.full((H, W, 3), background, np.float32)
    hit = owner >= 0
    if hit.any():   # (an empty cloud has no minimum)
        lo, hi = v.min(), v.max()
        img[hit] = (v[owner[hit]] - lo) / (hi - lo)
    return img, owner


def render_points_blend(verts, K, height, width, radius=0.03, znear=1.0, zfar=10.0, gamma=0.1, background=1.0):
    """The soft blend stated in render_kernels.hip (`gamma`): per pixel (sum_i w_i c_i + w_bg c_bg) / (sum_i w_i + w_bg) over the discs
    covering the pixel centre, w_i = (1 - distance to the disc centre / rho_i) exp((zn_i - zn_front) / gamma), zn = (zfar - Z) /
    (zfar - znear), w_bg = exp((0 - zn_front) / gamma); sums in float64, no fixed point.  A pixel whose weights all vanish takes the
    front sphere's colour.  PARITY UNPINNED (pulsar is absent): this restates the build's own text."""
    v = np.asarray(verts, np.float32)
    _, owner = render_points(v, K, height, width, radius, znear, zfar, background)
    fx, cx, fy, cy = (np.float32(K[0][0]), np.float32(K[0][2]), np.float32(K[1][1]), np.float32(K[1][2]))
    H, W = int(height), int(width)
    lo, hi = v.min(), v.max()
    col = ((v - lo) / (hi - lo)).astype(np.float64)
    zfront = np.where(owner >= 0, v[np.maximum(owner, 0), 2], np.float32(zfar)).astype(np.float64)
    rng = float(zfar) - float(znear)
    acc = np.zeros((H, W, 4), np.float64)
    for i, (X, Y, Z) in enumerate(v):
        if not (Z >= znear and Z <= zfar):
            continue
        u, w_ = fx * X / Z + cx, fy * Y / Z + cy
        rho = fx * np.float32(radius) / Z
        j0, j1 = max(0, int(np.floor(u - rho - np.float32(0.5)))), min(W - 1, int(np.ceil(u + rho - np.float32(0.5))))
        i0, i1 = max(0, int(np.floor(w_ - rho - np.float32(0.5)))), min(H - 1, int(np.ceil(w_ + rho - np.float32(0.5))))
        if j1 < j0 or i1 < i0:
            continue
        pj = np.arange(j0, j1 + 1, dtype=np.float32) + np.float32(0.5) - u
        pi = np.arange(i0, i1 + 1, dtype=np.float32) + np.float32(0.5) - w_
        q2 = pj[None, :] * pj[None, :] + pi[:, None] * pi[:, None]
        inside = q2 <= rho * rho
        d = np.maximum(np.float32(1.0) - np.sqrt(q2) / rho, np.float32(0.0)).astype(np.float64)
        t = (zfront[i0:i1 + 1, j0:j1 + 1] - float(Z)) / rng / float(gamma)
        wgt = np.where(inside, d * np.exp(np.minimum(t, 0.0)), 0.0)
        acc[i0:i1 + 1, j0:j1 + 1, 0] += wgt
        acc[i0:i1 + 1, j0:j1 + 1, 1:] += wgt[..., None] * col[i]
    wbg = np.exp((zfront - float(zfar)) / rng / float(gamma))
    Wt = acc[..., 0] + wbg
    img = np.full((H, W, 3), background, np.float64)
    hit = owner >= 0
    ok = hit & (Wt > 0)
    img[ok] = (acc[..., 1:][ok] + (wbg[ok] * background)[:, None]) / Wt[ok][:, None]
    dead = hit & ~(Wt > 0)
    img[dead] = col[owner[dead]]
    return img.astype(np.float32)
