"""Explicit float64 restatements of the hand-written backward kernels (CPU only; nothing here imports the GPU library).

Every function states the adjoint as formulas, not through autograd: ``tests/test_backward_ref_host.py`` checks each against
``torch.autograd`` in float64, and the GPU tests compare the kernels with them.  Inputs are the (bf16- or fp32-representable)
values the kernel reads; ``dtype`` selects the precision the formulas are evaluated in (float64: the reference; float32: the
yardstick for what plain fp32 evaluation of the same formulas loses).  Results come back as a dict of tensors of that dtype.

For every output that is a sum over rows, ``abs_<name>`` is the same sum over |term|: the scale an fp32 accumulation error is
measured against.
"""
import math

import torch

LOG2E = 1.4426950408889634


def _c(t, dtype):
    return None if t is None else t.to(dtype)


def group_of_rows(seq, n_text, per_group):
    """Token group of every sequence position: 0 for the text rows, 1 + i for the i-th block of ``per_group`` video rows
    (``per_group`` <= 0: all video rows are group 1)."""
    s = torch.arange(seq)
    gsz = per_group if per_group > 0 else max(seq - n_text, 1)
    return torch.where(s < n_text, torch.zeros_like(s), 1 + (s - n_text) // gsz)


def n_groups(seq, n_text, per_group):
    """Number of table entries the kernels address (the text entry included, also when it has no rows)."""
    vid = seq - n_text
    gsz = per_group if per_group > 0 else vid
    return 1 + (-(-vid // gsz) if gsz > 0 else 0)


def mapped_rows(n_rows, xmap):
    """Row of the mapped buffer that dense row r reads / writes: (r // rows) * bstride + off + r % rows."""
    r = torch.arange(n_rows)
    if xmap is None:
        return r
    rows, bstride, off = xmap
    return (r // rows) * bstride + off + r % rows


def ln_mod_bwd(dy, x, dres, gamma, beta, scale_tab, groups, eps, xmap=None, dtype=torch.float64):
    """Adjoint of y = (xh * gamma + beta) * (1 + scale[b, g]) + shift[b, g], xh = LayerNorm(x) without affine.

    ``dy`` [batch * seq, D] is dense; ``x``, ``dres`` and the returned ``dx`` live in the mapped buffer (rows the map does not
    reach are NaN in ``dx``).  ``scale_tab`` [batch, G, D] or None; ``groups`` = (seq, n_text, per_group)."""
    seq, n_text, per_group = groups
    dy = _c(dy, dtype)
    R, D = dy.shape
    batch = R // seq
    xr = mapped_rows(R, xmap)
    xs = _c(x, dtype)[xr]
    gam = torch.ones(D, dtype=dtype) if gamma is None else _c(gamma, dtype)
    bet = torch.zeros(D, dtype=dtype) if beta is None else _c(beta, dtype)
    G = n_groups(seq, n_text, per_group)
    grp = group_of_rows(seq, n_text, per_group).repeat(batch)
    bidx = torch.arange(R) // seq
    osc = torch.ones(R, D, dtype=dtype) if scale_tab is None else 1 + _c(scale_tab, dtype)[bidx, grp]
    mu = xs.mean(1, keepdim=True)
    xc = xs - mu
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    xh = xc * rstd
    dxh = dy * osc * gam
    dxs = rstd * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    if dres is not None:
        dxs = dxs + _c(dres, dtype)[xr]
    dx = torch.full(x.shape, float("nan"), dtype=dtype)
    dx[xr] = dxs
    t_gamma, t_beta = osc * dy * xh, osc * dy
    t_scale, t_shift = dy * (xh * gam + bet), dy
    flat = bidx * G + grp

    def by_group(t):
        return torch.zeros(batch * G, D, dtype=dtype).index_add_(0, flat, t).view(batch, G, D)

    return {"dx": dx, "rows": xr, "dgamma": t_gamma.sum(0), "abs_dgamma": t_gamma.abs().sum(0), "dbeta": t_beta.sum(0),
            "abs_dbeta": t_beta.abs().sum(0), "dscale": by_group(t_scale), "abs_dscale": by_group(t_scale.abs()),
            "dshift": by_group(t_shift), "abs_dshift": by_group(t_shift.abs()),
            "group_rows": torch.bincount(flat, minlength=batch * G).view(batch, G)}


def gated_bwd(dout, y, gate_tab, groups, dtype=torch.float64):
    """Adjoint of out = x + gate[b, g] * y on the y branch: dy = gate * dout, dgate[b, g] = sum over the group's rows of dout * y."""
    seq, n_text, per_group = groups
    dout, y, gate = _c(dout, dtype), _c(y, dtype), _c(gate_tab, dtype)
    R, D = dout.shape
    batch = R // seq
    G = gate.shape[1]
    grp = group_of_rows(seq, n_text, per_group).repeat(batch)
    bidx = torch.arange(R) // seq
    flat = bidx * G + grp
    t = dout * y
    z = lambda: torch.zeros(batch * G, D, dtype=dtype)
    return {"dy": gate[bidx, grp] * dout, "dgate": z().index_add_(0, flat, t).view(batch, G, D),
            "abs_dgate": z().index_add_(0, flat, t.abs()).view(batch, G, D),
            "group_rows": torch.bincount(flat, minlength=batch * G).view(batch, G)}


def small_linear_bwd(dy, x, W, dtype=torch.float64):
    """Adjoint of y = x W^T + b for a few rows: dW = dy^T x, db = column sums of dy, dx = dy W (None without W)."""
    dy, x, W = _c(dy, dtype), _c(x, dtype), _c(W, dtype)
    out = {"dW": dy.t() @ x, "db": dy.sum(0), "abs_db": dy.abs().sum(0), "dx": None, "abs_dx": None}
    if W is not None:
        out["dx"], out["abs_dx"] = dy @ W, dy.abs() @ W.abs()
    return out


def rope_apply(z, rope, n_text):
    """Rotary embedding on positions >= n_text of z [..., S, 64]: pairs (2i, 2i + 1), y = z cos + rot(z) sin."""
    if rope is None:
        return z
    cos, sin = (r.to(z.dtype) for r in rope)
    zv = z[..., n_text:, :]
    rot = torch.stack([-zv[..., 1::2], zv[..., 0::2]], dim=-1).flatten(-2)
    return torch.cat([z[..., :n_text, :], zv * cos + rot * sin], dim=-2)


def _rope_adjoint(d, rope, n_text):
    if rope is None:
        return d
    cos, sin = (r.to(d.dtype) for r in rope)
    dv = d[..., n_text:, :]
    ev, od = dv[..., 0::2], dv[..., 1::2]
    back = torch.stack([ev * cos[:, 0::2] + od * sin[:, 1::2], od * cos[:, 1::2] - ev * sin[:, 0::2]], dim=-1).flatten(-2)
    return torch.cat([d[..., :n_text, :], back], dim=-2)


def qkv_prep_bwd(raw, dq, dk, gq, gk, rope, n_text, eps, dtype=torch.float64):
    """Adjoint of q = RoPE(LayerNorm64(raw_q) * gq + bq) (and the same for k) given dq, dk.

    ``raw`` [B, S, 3, H, 64] (the packed projection output), ``dq`` / ``dk`` [B, S, H, 64]; ``rope`` = (cos, sin) [S - n_text, 64]
    or None.  Returns the gradients of the raw q and k thirds and of the four norm vectors."""
    raw = _c(raw, dtype)
    out = {}
    for i, (name, d, gam) in enumerate((("q", dq, gq), ("k", dk, gk))):
        xs = raw[:, :, i].transpose(1, 2)                               # [B, H, S, 64]
        dz = _rope_adjoint(_c(d, dtype).transpose(1, 2), rope, n_text)
        gam = torch.ones(64, dtype=dtype) if gam is None else _c(gam, dtype)
        xc = xs - xs.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
        xh = xc * rstd
        dxh = dz * gam
        dx = rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))
        out["draw_" + name] = dx.transpose(1, 2)
        tg = (dz * xh).reshape(-1, 64)
        tb = dz.reshape(-1, 64)
        out["dg" + name], out["abs_dg" + name] = tg.sum(0), tg.abs().sum(0)
        out["db" + name], out["abs_db" + name] = tb.sum(0), tb.abs().sum(0)
    return out


def attention_bwd(q_stored, k, v, do, scale, dtype=torch.float64):
    """Softmax attention and its adjoint, per head: all operands [B, H, S, 64].

    ``q_stored`` is what the kernel reads (q already multiplied by scale * log2 e); it is divided back here and the gradients
    are with respect to that un-premultiplied q.  ``lse`` is the natural-log row sum of exp(scale * q k^T)."""
    q = _c(q_stored, dtype) / (scale * LOG2E)
    k, v, do = _c(k, dtype), _c(v, dtype), _c(do, dtype)
    s = scale * (q @ k.transpose(-1, -2))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    out = p @ v
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (do * out).sum(-1, keepdim=True))
    return {"out": out, "lse": (m + torch.log(l)).squeeze(-1), "dq": scale * (ds @ k), "dk": scale * (ds.transpose(-1, -2) @ q),
            "dv": p.transpose(-1, -2) @ do}


def mod_tables_bwd(dtab, cond_v, cond_t, Ws, text, dtype=torch.float64):
    """Adjoint of the AdaLN tables out[t][b][1 + f] = W_t[:width] cond_v[b * T + f] + bias, out[t][b][0] = W_t[width:] cond_t[b] + bias.

    ``dtab`` [n_tab, B, 1 + T, width]; ``Ws`` a list of [width * (1 + text), E].  Returns gW [n_tab, ntot, E], gb [n_tab, ntot] and the
    conditioning gradients summed over the tables."""
    dtab, cond_v, cond_t = _c(dtab, dtype), _c(cond_v, dtype), _c(cond_t, dtype)
    n_tab, B, G, width = dtab.shape
    gW, gb, agb = [], [], []
    dcv, acv = torch.zeros_like(cond_v), torch.zeros_like(cond_v)
    dct = act = None
    if text:
        dct, act = torch.zeros_like(cond_t), torch.zeros_like(cond_t)
    for t in range(n_tab):
        W = _c(Ws[t], dtype)
        dv = dtab[t][:, 1:].reshape(B * (G - 1), width)
        w, b, ab = [dv.t() @ cond_v], [dv.sum(0)], [dv.abs().sum(0)]
        dcv += dv @ W[:width]
        acv += dv.abs() @ W[:width].abs()
        if text:
            dt = dtab[t][:, 0]
            w.append(dt.t() @ cond_t), b.append(dt.sum(0)), ab.append(dt.abs().sum(0))
            dct += dt @ W[width:]
            act += dt.abs() @ W[width:].abs()
        gW.append(torch.cat(w)), gb.append(torch.cat(b)), agb.append(torch.cat(ab))
    return {"gW": torch.stack(gW), "gb": torch.stack(gb), "abs_gb": torch.stack(agb), "d_cond_v": dcv, "abs_d_cond_v": acv,
            "d_cond_t": dct, "abs_d_cond_t": act}
