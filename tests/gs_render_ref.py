"""CPU restatement of the Gaussian rasterizer (``orv_amd.gs_render``, include/orv_mi355.h ``orv_gs_*``), written from the arithmetic contract
of DESIGN.md §12 in numpy, at a chosen precision (fp32: the contract itself, operation by operation; fp64: the yardstick the kernel's and the
fp32 run's rounding are measured against).  Besides the four planes and ``radii`` it reports per-pixel contributor counts and the FRAGILE
pixels: those where a discrete decision of a live entry sits within ``delta`` of its threshold, so that a last-bit difference may take the
other branch.  Depths are compared as fp32 at either precision, exact depth ties go by Gaussian index, and neither is fragile.
"""
from __future__ import annotations

import numpy as np

TILE = 16
NEAR = 0.01
DELTA = 1e-4
BIG = 1.0e9


def _trunc(v):
    """float -> int toward zero of max(v, -1e9) then min(., 1e9), both NaN-dropping (fmax / fmin): the defined range is untouched, and a NaN
    becomes -1e9 as in the kernel.  NaN inputs are outside the contract; this only keeps both sides defined and equal."""
    return np.fmin(np.fmax(v, -BIG), BIG).astype(np.int64)


def _rects(px, py, r, gx, gy, dt):
    """Clamped tile rectangle (x0, y0, x1, y1) of centres (px, py) and integer radii r."""
    fr = r.astype(dt)
    s, f = dt(16.0), dt(15.0)
    x0 = np.clip(_trunc((px - fr) / s), 0, gx)
    y0 = np.clip(_trunc((py - fr) / s), 0, gy)
    x1 = np.clip(_trunc((px + fr + f) / s), 0, gx)
    y1 = np.clip(_trunc((py + fr + f) / s), 0, gy)
    return np.stack([x0, y0, x1, y1], axis=1)


def _canon(rect):
    """An empty rectangle is (0, 0, 0, 0) whatever its corners."""
    empty = (rect[:, 2] <= rect[:, 0]) | (rect[:, 3] <= rect[:, 1])
    return np.where(empty[:, None], 0, rect)


def preprocess(means, scales, rots, H, W, tanfovx, tanfovy, scale_modifier, view, proj, dtype=np.float32, delta=DELTA):
    """Steps 1-7 per Gaussian.  -> dict(px, py, conic [N,3], z, radii, rect, visible, lam3, rect_unstable)."""
    dt = dtype
    m, s, q = (np.asarray(a, dtype=np.float64).astype(dt) for a in (means, scales, rots))
    V, P = np.asarray(view).astype(dt), np.asarray(proj).astype(dt)
    tfx, tfy, sm = dt(tanfovx), dt(tanfovy), dt(scale_modifier)
    N = m.shape[0]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(all="ignore"):
        tx0 = x * V[0, 0] + y * V[1, 0] + z * V[2, 0] + V[3, 0]
        ty0 = x * V[0, 1] + y * V[1, 1] + z * V[2, 1] + V[3, 1]
        tz = x * V[0, 2] + y * V[1, 2] + z * V[2, 2] + V[3, 2]
        front = tz > dt(NEAR)
        hx = x * P[0, 0] + y * P[1, 0] + z * P[2, 0] + P[3, 0]
        hy = x * P[0, 1] + y * P[1, 1] + z * P[2, 1] + P[3, 1]
        hw = x * P[0, 3] + y * P[1, 3] + z * P[2, 3] + P[3, 3]
        w = dt(1.0) / (hw + dt(1e-7))
        px = ((hx * w + dt(1.0)) * dt(W) - dt(1.0)) / dt(2.0)
        py = ((hy * w + dt(1.0)) * dt(H) - dt(1.0)) / dt(2.0)
        qn = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        qr, qx, qy, qz = (q[:, k] / qn for k in range(4))
        one, two = dt(1.0), dt(2.0)
        R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - qr * qz), two * (qx * qz + qr * qy)],
             [two * (qx * qy + qr * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qr * qx)],
             [two * (qx * qz - qr * qy), two * (qy * qz + qr * qx), one - two * (qx * qx + qy * qy)]]
        sc = [sm * s[:, k] for k in range(3)]
        M = [[R[r][c] * sc[c] for c in range(3)] for r in range(3)]
        S3 = [[M[r][0] * M[c][0] + M[r][1] * M[c][1] + M[r][2] * M[c][2] for c in range(3)] for r in range(3)]
        limx, limy = dt(1.3) * tfx, dt(1.3) * tfy
        tx = np.minimum(limx, np.maximum(-limx, tx0 / tz)) * tz
        ty = np.minimum(limy, np.maximum(-limy, ty0 / tz)) * tz
        fx, fy = dt(W) / (two * tfx), dt(H) / (two * tfy)
        j00, j02, j11, j12 = fx / tz, -(fx * tx) / (tz * tz), fy / tz, -(fy * ty) / (tz * tz)
        T0 = [j00 * V[c, 0] + j02 * V[c, 2] for c in range(3)]            # T = J Rw, Rw[r][c] = V[c][r]
        T1 = [j11 * V[c, 1] + j12 * V[c, 2] for c in range(3)]
        U0 = [T0[0] * S3[0][c] + T0[1] * S3[1][c] + T0[2] * S3[2][c] for c in range(3)]
        U1 = [T1[0] * S3[0][c] + T1[1] * S3[1][c] + T1[2] * S3[2][c] for c in range(3)]
        va = U0[0] * T0[0] + U0[1] * T0[1] + U0[2] * T0[2] + dt(0.3)
        vb = U0[0] * T1[0] + U0[1] * T1[1] + U0[2] * T1[2]
        vc = U1[0] * T1[0] + U1[1] * T1[1] + U1[2] * T1[2] + dt(0.3)
        det = va * vc - vb * vb
        ok = front & (det != 0)
        conic = np.stack([vc / det, -vb / det, va / det], axis=1)
        mid = (va + vc) / two
        lam = mid + np.sqrt(np.maximum(dt(0.1), mid * mid - det))
        lam3 = dt(3.0) * np.sqrt(lam)
        r = _trunc(np.ceil(lam3))
        rect = _canon(_rects(px, py, r, gx, gy, dt))
        # a rectangle is unstable if it changes when the centre moves by +-delta or 3 sqrt(lambda) by +-delta before the ceil
        d = dt(delta)
        unstable = np.zeros(N, dtype=bool)
        for ppx, ppy, rr in ((px - d, py, r), (px + d, py, r), (px, py - d, r), (px, py + d, r),
                             (px, py, _trunc(np.ceil(lam3 - d))), (px, py, _trunc(np.ceil(lam3 + d)))):
            unstable |= np.any(_canon(_rects(ppx, ppy, rr, gx, gy, dt)) != rect, axis=1)
    rect = np.where(ok[:, None], rect, 0)
    visible = ok & (rect[:, 2] > rect[:, 0])
    return dict(px=px, py=py, conic=conic, z=tz, radii=np.where(visible, r, 0).astype(np.int32), rect=rect.astype(np.int64), visible=visible,
                lam3=lam3, front=front, rect_unstable=unstable & ok)


def rasterize(means, opacities, scales, rots, colors, feats, H, W, tanfovx, tanfovy, bg, scale_modifier, view, proj, dtype=np.float32,
              delta=DELTA):
    """-> dict(color [3,H,W], feat [F,H,W], depth [1,H,W], alpha [1,H,W], radii [N], count [H,W], fragile [H,W], fragile_by {threshold: [H,W]},
    pre = preprocess(...))."""
    dt = dtype
    pre = preprocess(means, scales, rots, H, W, tanfovx, tanfovy, scale_modifier, view, proj, dt, delta)
    N = np.asarray(means).shape[0]
    op = np.asarray(opacities, dtype=np.float64).reshape(-1).astype(dt)
    col = np.asarray(colors, dtype=np.float64).reshape(N, 3).astype(dt)
    F = 0 if feats is None else np.asarray(feats).shape[1]
    ft = np.zeros((N, 0), dt) if F == 0 else np.asarray(feats, dtype=np.float64).astype(dt)
    bgc = np.asarray(bg, dtype=np.float64).astype(dt)
    X, Y = np.meshgrid(np.arange(W).astype(dt), np.arange(H).astype(dt))
    T = np.ones((H, W), dt)
    C, Fm, D = np.zeros((3, H, W), dt), np.zeros((F, H, W), dt), np.zeros((H, W), dt)
    done = np.zeros((H, W), bool)
    causes = {k: np.zeros((H, W), bool) for k in ("power", "alpha", "stop", "near_tie", "rect")}     # fragile pixels by threshold
    count = np.zeros((H, W), np.int32)
    last = np.full((H, W), np.nan)
    half, cap, amin, tmin = dt(-0.5), dt(0.99), dt(1.0) / dt(255.0), dt(0.0001)
    px, py, conic, z = pre["px"], pre["py"], pre["conic"], pre["z"]

    def power_of(g, xs, ys):
        dx, dy = px[g] - X[ys, xs], py[g] - Y[ys, xs]
        return half * (conic[g, 0] * dx * dx + conic[g, 2] * dy * dy) - conic[g, 1] * dx * dy

    vis = np.nonzero(pre["visible"])[0]
    order = vis[np.lexsort((vis, z[vis].astype(np.float32)))]       # ascending fp32 depth, ties by ascending index
    with np.errstate(all="ignore"):
        for g in order:
            x0, y0, x1, y1 = pre["rect"][g]
            xs, ys = slice(x0 * TILE, min(x1 * TILE, W)), slice(y0 * TILE, min(y1 * TILE, H))
            live = ~done[ys, xs]
            if not live.any():
                continue
            power = power_of(g, xs, ys)
            f_pow = live & (np.abs(power) < 1e-6)
            ok = live & (power <= 0)
            alpha = np.minimum(cap, op[g] * np.exp(power))
            f_alpha = ok & (np.abs(255.0 * alpha.astype(np.float64) - 1.0) < delta)
            ok &= alpha >= amin
            Tn = T[ys, xs] * (dt(1.0) - alpha)
            f_stop = ok & (np.abs(1e4 * Tn.astype(np.float64) - 1.0) < delta)
            zg = float(z[g])
            lz = last[ys, xs]
            f_tie = ok & (lz != zg) & (np.abs(lz - zg) < 1e-6 * np.maximum(np.abs(lz), abs(zg)))
            last[ys, xs] = np.where(ok, zg, lz)
            stop = ok & (Tn < tmin)
            add = ok & ~stop
            wgt = np.where(add, alpha * T[ys, xs], dt(0.0))
            for c in range(3):
                C[c, ys, xs] += wgt * col[g, c]
            for c in range(F):
                if ft[g, c] != 0:
                    Fm[c, ys, xs] += wgt * ft[g, c]
            D[ys, xs] += wgt * z[g]
            T[ys, xs] = np.where(add, Tn, T[ys, xs])
            done[ys, xs] |= stop
            count[ys, xs] += add
            for k, f in (("power", f_pow), ("alpha", f_alpha), ("stop", f_stop), ("near_tie", f_tie)):
                causes[k][ys, xs] |= f
        # a Gaussian whose rectangle is unstable may enter or leave a tile's list: every pixel it would contribute to is fragile
        whole = (slice(0, W), slice(0, H))
        for g in np.nonzero(pre["rect_unstable"])[0]:
            power = power_of(g, *whole)
            causes["rect"] |= (power <= 0) & (op[g].astype(np.float64) * np.exp(power.astype(np.float64)) >= (1.0 - delta) / 255.0)
    fragile = np.logical_or.reduce(list(causes.values()))
    color = C + T[None] * bgc[:, None, None]
    return dict(color=color, feat=Fm, depth=D[None], alpha=(dt(1.0) - T)[None], radii=pre["radii"], count=count, fragile=fragile, fragile_by=causes, pre=pre)
