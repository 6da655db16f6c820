"""numpy restatement of the control-preparation contract, written from the contract and not from the kernel: every
product and sum is an array operation of its own, so in float32 each one is rounded to fp32 exactly once, in the contract's order.
``dt=np.float64`` evaluates the same formulas in fp64 (the variant compared with the fp64 torch chain).

A plan is a list of one or two stages ``(rh, rw, top, left, ch, cw)``: resize to (rh, rw), crop [top:top+ch, left:left+cw]."""
import colorsys

import numpy as np


def axis_taps(n, o, dt=np.float32):
    """Antialiased-bilinear taps of ``n`` inputs -> ``o`` outputs: (j [o, K] tap indices, valid [o, K], w [o, K] normalised weights)."""
    scale = dt(n) / dt(o)
    support = scale if scale >= 1 else dt(1)
    inv = dt(1) / scale if scale >= 1 else dt(1)
    i = np.arange(o).astype(dt)
    c = scale * (i + dt(0.5))
    lo = np.maximum(((c - support) + dt(0.5)).astype(np.int64), 0)            # astype truncates toward zero, like int()
    hi = np.minimum(((c + support) + dt(0.5)).astype(np.int64), n)
    K = int((hi - lo).max())
    j = lo[:, None] + np.arange(K)[None, :]
    valid = j < hi[:, None]
    w = np.maximum(dt(0), dt(1) - np.abs(((j.astype(dt) - c[:, None]) + dt(0.5)) * inv)).astype(dt)
    total = np.zeros(o, dtype=dt)
    for k in range(K):                                                         # summed in tap order
        total = np.where(valid[:, k], total + w[:, k], total)
    w = (w / total[:, None]).astype(dt)
    return np.minimum(j, n - 1), valid, w


def resize_last_axis(x, o, dt=np.float32):
    j, valid, w = axis_taps(x.shape[-1], o, dt)
    out = np.zeros(x.shape[:-1] + (o,), dtype=dt)
    for k in range(j.shape[1]):                                                # the sum in tap order of x[j] * w[j]
        out = np.where(valid[:, k], out + x[..., j[:, k]] * w[:, k], out)
    return out.astype(dt)


def resize_bilinear(x, oh, ow, dt=np.float32):
    """x [..., h, w]: the horizontal pass first (rounded to ``dt``), then the vertical pass."""
    x = resize_last_axis(x.astype(dt), ow, dt)
    return np.swapaxes(resize_last_axis(np.swapaxes(x, -1, -2), oh, dt), -1, -2)


def nearest_index(n, o):
    scale = np.float32(n) / np.float32(o)
    return np.minimum(np.floor(np.arange(o).astype(np.float32) * scale).astype(np.int64), n - 1)


def resize_nearest(x, oh, ow):
    return x[..., nearest_index(x.shape[-2], oh), :][..., nearest_index(x.shape[-1], ow)]


def apply_plan(x, stages, mode, dt=np.float32):
    for rh, rw, top, left, ch, cw in stages:
        x = resize_bilinear(x, rh, rw, dt) if mode == "bilinear" else resize_nearest(x, rh, rw)
        x = x[..., top:top + ch, left:left + cw]
    return x


def _gather(x, index):
    return x if index is None else x[np.asarray(index).reshape(-1)]


def depths(x, stages, index=None, dt=np.float32):
    """fp32 [N, h, w] -> [n_out, 1, H, W]: min(max(resized, 0.01), 0.4) * 2.5."""
    y = apply_plan(_gather(np.asarray(x), index).astype(dt), stages, "bilinear", dt)
    with np.errstate(invalid="ignore"):
        y = np.where(y < dt(0.01), dt(0.01), np.where(y > dt(0.4), dt(0.4), y))   # a NaN stays a NaN
    return (y * dt(2.5)).astype(dt)[:, None]


def palette60():
    colors = [tuple(int(c * 255) for c in colorsys.hsv_to_rgb(i / 60, 0.75, 0.95)) for i in range(60)]
    colors[59] = (0, 0, 0)
    return np.array(colors, dtype=np.float32)


def labels(ids, stages, index=None):
    """uint8 ids [N, h, w] -> fp32 [n_out, 3, H, W]: nearest resize of the ids, then palette[id] / 255."""
    y = apply_plan(_gather(np.asarray(ids), index), stages, "nearest")
    return np.moveaxis((palette60() / np.float32(255))[y], -1, 1).astype(np.float32)


def frames(x, stages, index=None, normalize=True, dt=np.float32):
    """uint8 [N, h, w, 3] -> [n_out, 3, H, W]: x / 255, antialiased bilinear plan, then (x - 0.5) / 0.5."""
    y = np.moveaxis(_gather(np.asarray(x), index), -1, 1).astype(dt) / dt(255)
    y = apply_plan(y.astype(dt), stages, "bilinear", dt)
    if normalize:
        y = (y - dt(0.5)) / dt(0.5)
    return y.astype(dt)
