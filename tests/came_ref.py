"""CPU restatement of the fused CAME optimizer (``orv_amd.optim.FusedCAME``, include/orv_mi355.h ``orv_came_*``), written from the rule in
DESIGN.md 4.3.4 and not from the kernels.  Not a test.

The rule restates ``came_pytorch``'s ``CAME.step`` FROM MEMORY: the package cannot be installed where this project is developed, so nothing
here was compared against it (UNPINNED, like the diffusers leaves of oracle/leaf.py and the Prodigy rule of tests/prodigy_ref.py).  One
parameter group; ``RMS(p)``, which ``came_pytorch`` stores and never reads, is not kept.

    g = gradient x clip coefficient ;  q = g g + eps1
    parameter of two or more dimensions (factored over the last two, every leading index a matrix of its own):
        r = b2 r + (1-b2) mean(q, -1) ;  c = b2 c + (1-b2) mean(q, -2) ;  u = (g rsqrt(r / mean(r, -1))[..., :, None]) rsqrt(c)[..., None, :]
    otherwise:   v = b2 v + (1-b2) q ;  u = g rsqrt(v)
    k = max(1, sqrt(mean(u u over the whole parameter)) / clip_threshold) ;  u = u / k
    m = b1 m + (1-b1) u ;  s = (u - m)^2 + eps2                                                       (the new m)
    factored:    Rr = b3 Rr + (1-b3) mean(s, -1) ;  Cc = b3 Cc + (1-b3) mean(s, -2) ;  out = (m rsqrt(Rr / mean(Rr, -1))[..., :, None]) rsqrt(Cc)[..., None, :]
    otherwise:   out = m
    w = w - (wd lr) w  (wd != 0) ;  w = w - lr out

All state starts at zero; there is no bias correction and no step count.  ``dtype`` chooses the evaluation: ``torch.float32`` rounds every
operation separately (the hyper-parameters enter as fp32: the C ABI takes floats), ``torch.float64`` is the yardstick: the same inputs, the
same fp32-rounded hyper-parameters, everything in double.

Two closed forms from zero state (``rank_one_step`` / ``unfactored_step``): a rank-one gradient g_ij = a_i b_j moves every weight of a matrix
by -lr (1-b1) / (b1 sqrt(1-b3)) sign(g), whatever b2 and clip_threshold are; an unfactored parameter moves by -lr (1-b1) clip_threshold sign(g)
whenever 1 / sqrt(1-b2) > clip_threshold."""
import math

import torch

SEG = 2048
DEFAULTS = dict(eps=(1e-30, 1e-16), clip_threshold=1.0, betas=(0.9, 0.999, 0.9999), weight_decay=0.0)
REFERENCE_BETAS = (0.9, 0.95, 0.98)          # the reference's yaml: beta1 / beta2 / beta3
STATS = ("r", "c", "res_r", "res_c", "v")
NAMES = {"r": "exp_avg_sq_row", "c": "exp_avg_sq_col", "res_r": "exp_avg_res_row", "res_c": "exp_avg_res_col", "v": "exp_avg_sq"}


def f32(x) -> float:
    """A Python float rounded to fp32 (what a ``float`` argument of the C ABI holds)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def is_factored(shape) -> bool:
    return len(shape) >= 2


def new_state(shape, dtype=torch.float64):
    """Zero state shaped as ``came_pytorch`` keeps it."""
    shape = tuple(shape)
    z = lambda s: torch.zeros(s, dtype=dtype)
    st = {"exp_avg": z(shape)}
    if is_factored(shape):
        st.update(exp_avg_sq_row=z(shape[:-1]), exp_avg_sq_col=z(shape[:-2] + shape[-1:]),
                  exp_avg_res_row=z(shape[:-1]), exp_avg_res_col=z(shape[:-2] + shape[-1:]))
    else:
        st["exp_avg_sq"] = z(shape)
    return st


def _approx(x, row, col):
    """(x rsqrt(row / mean(row, -1))[..., :, None]) rsqrt(col)[..., None, :]"""
    rf = (row / row.mean(dim=-1, keepdim=True)).rsqrt()
    return (x * rf.unsqueeze(-1)) * col.rsqrt().unsqueeze(-2)


def param_step(w, g, st, dtype, lr, clip=1.0, **hyper):
    """One step of one parameter: ``w`` the weight and ``st`` (``new_state``) in ``dtype``, ``g`` the raw gradient.  ``st`` is updated in
    place -> (new weight, k, RMS of u before the division), all in ``dtype``."""
    h = dict(DEFAULTS, **hyper)
    T = lambda x: torch.tensor(f32(x), dtype=dtype)
    one = torch.ones((), dtype=dtype)
    b1, b2, b3 = (T(b) for b in h["betas"])
    eps1, eps2 = (T(e) for e in h["eps"])
    gr = g.to(dtype) * T(clip)
    q = gr * gr + eps1
    fact = is_factored(w.shape)
    if fact:
        st["exp_avg_sq_row"] = b2 * st["exp_avg_sq_row"] + (one - b2) * q.mean(dim=-1)
        st["exp_avg_sq_col"] = b2 * st["exp_avg_sq_col"] + (one - b2) * q.mean(dim=-2)
        u = _approx(gr, st["exp_avg_sq_row"], st["exp_avg_sq_col"])
    else:
        st["exp_avg_sq"] = b2 * st["exp_avg_sq"] + (one - b2) * q
        u = gr * st["exp_avg_sq"].rsqrt()
    rms = (u * u).mean().sqrt()
    k = torch.clamp(rms / T(h["clip_threshold"]), min=1.0)
    u = u / k
    m = b1 * st["exp_avg"] + (one - b1) * u
    st["exp_avg"] = m
    if fact:
        s = (u - m) ** 2 + eps2
        st["exp_avg_res_row"] = b3 * st["exp_avg_res_row"] + (one - b3) * s.mean(dim=-1)
        st["exp_avg_res_col"] = b3 * st["exp_avg_res_col"] + (one - b3) * s.mean(dim=-2)
        out = _approx(m, st["exp_avg_res_row"], st["exp_avg_res_col"])
    else:
        out = m
    if h["weight_decay"] != 0:
        w = w - (T(h["weight_decay"]) * T(lr)) * w
    return w - T(lr) * out, k, rms


def rank_one_step(lr, betas):
    """|delta w| of every element of a matrix after one step from zero state on a rank-one gradient without zeros."""
    b1, _, b3 = (f32(b) for b in betas)
    return f32(lr) * (1 - b1) / (b1 * math.sqrt(1 - b3))


def unfactored_step(lr, betas, clip_threshold):
    """|delta w| of every element of an unfactored parameter after one step from zero state; holds when 1 / sqrt(1-b2) > clip_threshold."""
    b1, b2, _ = (f32(b) for b in betas)
    assert 1 / math.sqrt(1 - b2) > clip_threshold
    return f32(lr) * (1 - b1) * f32(clip_threshold)


# ---- flat layout: where a parameter's statistics live, and one step over segments ----
def layout(shapes):
    """Per parameter (B, R, C, row0, col0, v0) - the offsets of its statistics in the flat arrays r / res_r (B R values), c / res_c (B C) and
    v (unfactored parameters only, each padded to 2048) - and the totals (n_rows, n_cols, n_v)."""
    rows = cols = nv = 0
    out = []
    for shape in shapes:
        numel = 1
        for d in shape:
            numel *= int(d)
        if is_factored(shape):
            R, C = int(shape[-2]), int(shape[-1])
            B = numel // (R * C)
            out.append((B, R, C, rows, cols, nv))
            rows, cols = rows + B * R, cols + B * C
        else:
            out.append((1, 0, 0, rows, cols, nv))
            nv += (numel + SEG - 1) // SEG * SEG
    return out, (rows, cols, nv)


def zero_stats(shapes, dtype=torch.float32):
    _, (rows, cols, nv) = layout(shapes)
    return dict(r=torch.zeros(rows, dtype=dtype), c=torch.zeros(cols, dtype=dtype), res_r=torch.zeros(rows, dtype=dtype),
                res_c=torch.zeros(cols, dtype=dtype), v=torch.zeros(nv, dtype=dtype))


def state_of(shape, lay, m_seg, stats, dtype):
    """The ``came_pytorch``-shaped state of one parameter from the flat arrays."""
    B, R, C, row0, col0, v0 = lay
    shape = tuple(shape)
    numel = m_seg.numel()
    st = {"exp_avg": m_seg.to(dtype).view(shape)}
    if R:
        lead = shape[:-2]
        st["exp_avg_sq_row"] = stats["r"][row0:row0 + B * R].to(dtype).view(lead + (R,))
        st["exp_avg_sq_col"] = stats["c"][col0:col0 + B * C].to(dtype).view(lead + (C,))
        st["exp_avg_res_row"] = stats["res_r"][row0:row0 + B * R].to(dtype).view(lead + (R,))
        st["exp_avg_res_col"] = stats["res_c"][col0:col0 + B * C].to(dtype).view(lead + (C,))
    else:
        st["exp_avg_sq"] = stats["v"][v0:v0 + numel].to(dtype).view(shape)
    return st


def flat_step(w, g, m, stats, shapes, seg_start, seg_active, dtype, lr, clip=1.0, **hyper):
    """One step on flat buffers (``w`` the weights - fp32 masters or bf16 values -, ``g`` bf16, ``m`` and ``stats`` fp32; segment i holds a
    parameter of ``shapes[i]``) evaluated in ``dtype`` -> (w, m, stats) as new tensors in ``dtype``, and per segment k and the RMS of u (None
    for an inactive one).  Inactive segments and padding keep everything."""
    lays, _ = layout(shapes)
    starts = [int(x) for x in seg_start.tolist()]
    w2, m2 = w.to(dtype).clone(), m.to(dtype).clone()
    stats2 = {k: stats[k].to(dtype).clone() for k in STATS}
    ks, rmss = [], []
    for i, (shape, lay) in enumerate(zip(shapes, lays)):
        if not int(seg_active[i]):
            ks.append(None); rmss.append(None)
            continue
        shape = tuple(shape)
        B, R, C, row0, col0, v0 = lay
        numel = 1
        for d in shape:
            numel *= int(d)
        a = starts[i]
        st = state_of(shape, lay, m[a:a + numel], stats, dtype)
        wn, k, rms = param_step(w[a:a + numel].to(dtype).view(shape), g[a:a + numel].view(shape), st, dtype, lr, clip=clip, **hyper)
        w2[a:a + numel], m2[a:a + numel] = wn.reshape(-1), st["exp_avg"].reshape(-1)
        if R:
            stats2["r"][row0:row0 + B * R] = st["exp_avg_sq_row"].reshape(-1)
            stats2["c"][col0:col0 + B * C] = st["exp_avg_sq_col"].reshape(-1)
            stats2["res_r"][row0:row0 + B * R] = st["exp_avg_res_row"].reshape(-1)
            stats2["res_c"][col0:col0 + B * C] = st["exp_avg_res_col"].reshape(-1)
        else:
            stats2["v"][v0:v0 + numel] = st["exp_avg_sq"].reshape(-1)
        ks.append(float(k)); rmss.append(float(rms))
    return w2, m2, stats2, ks, rmss


def came_step(p, g, m, stats, seg_start, seg_active, geom, sizes, scratch, lr, betas, eps=(1e-30, 1e-16), clip_threshold=1.0,
              weight_decay=0.0, clip_coef=None, lo=None, mode=0, which=None):
    """Stand-in for ``orv_amd.ops.came_step`` on CPU tensors (fp32 arithmetic), in place, for CPU tests of the optimizer's host logic.  The
    shapes are read from the geometry table ([B, R, C], or [numel] where R == 0): the rule only looks at the last two dimensions."""
    import adamw_ref
    assert which is None and mode in (0, 1) and p.numel() % SEG == 0 and scratch.numel() >= sizes["n_scratch"]
    table = geom.view(-1, 12).tolist()
    shapes = [(row[0], row[1], row[2]) if row[1] else (row[10],) for row in table]
    full = {k: (stats.get(k) if stats.get(k) is not None else torch.zeros(0)) for k in STATS}
    w = adamw_ref.rebuild(p, lo) if mode == 1 else p.float()
    clip = float(clip_coef) if clip_coef is not None else 1.0
    w2, m2, stats2, ks, rmss = flat_step(w, g, m, full, shapes, seg_start, seg_active, torch.float32, lr, clip=clip, betas=betas, eps=eps,
                                         clip_threshold=clip_threshold, weight_decay=weight_decay)
    if mode == 1:
        p2, lo2 = adamw_ref.split(w2)
        lo.copy_(lo2)
    else:
        p2 = w2.to(torch.bfloat16)
    p.copy_(p2)
    m.copy_(m2)
    for k in STATS:
        if stats.get(k) is not None:
            stats[k].copy_(stats2[k])
    tail = scratch[scratch.numel() - 2 * len(table):].view(-1, 2)
    for i, (k, rms) in enumerate(zip(ks, rmss)):
        if k is not None:
            tail[i, 0], tail[i, 1] = k, rms
