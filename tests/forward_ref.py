"""Explicit float64 restatements of the small forward kernels of the DiT trunk (``orv_amd/csrc/norm.hip``, ``embed.hip``), CPU only:
nothing here imports the GPU library.  ``tests/test_forward_ref_host.py`` checks each against an independent source
(``torch.nn.functional``, ``oracle/leaf.py``), ``tests/test_gpu_forward_edges.py`` compares the kernels with them.

Every function takes the operands of the ``orv_amd.ops`` wrapper of the same name as CPU tensors (bf16 activations / weights, fp32
tables) and evaluates the formulas of the kernel headers in ``dtype``: float64 is the reference, float32 the yardstick for what a
plain fp32 evaluation of the same formulas loses (the ``A`` of the GPU module's bounds).  Scalars the wrappers pass as C floats
(eps, q_premul, the scheduler coefficients) are rounded to float32 first: that is the value the kernel receives.

Three operations round an intermediate to bf16 inside (the conditioning of the modulation tables, the staged input of
``skinny_linear`` after ``act_in``, the normalised q / k before RoPE).  A correct fp32 kernel may land on the other side of a rounding
boundary there, and only there.  These restatements therefore
  * evaluate the intermediate in float64 AND float32, whatever ``dtype`` is,
  * take ``window`` = 16 x the largest |float32 - float64| of that intermediate on the call's own inputs,
  * round the float64 value (``round_bf16_ties``) and continue from it in ``dtype`` (so the float32 evaluation never differs from the
    float64 one by a flipped rounding, only by arithmetic),
  * return the mask of the elements within ``window`` of a boundary, and the bound term those elements add to each output.

The case tables of the GPU module live here, so that the host module can check the inputs (the tie cap) without a GPU.
"""
import math

import torch

BF = torch.bfloat16
F32, F64 = torch.float32, torch.float64
LOG2E = 1.4426950408889634


def rb(g, *shape, mul=1.0, add=0.0):
    """bf16-representable random values, as bf16."""
    return (torch.randn(*shape, generator=g) * mul + add).to(BF)


def ru(g, *shape, lo=-1.0, hi=1.0):
    """bf16-representable uniform values: the inputs of the operations that round an intermediate.  The share of elements near a
    rounding boundary grows with max|v| * density(v = 0); a uniform input keeps it about three times below a normal one's."""
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(BF)


def _f32(v):
    """A Python float as the C float the wrapper passes."""
    return float(torch.tensor(float(v), dtype=F32))


def _c(t, dtype):
    return None if t is None else t.to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# bf16 rounding with a tie mask
# ---------------------------------------------------------------------------------------------------------------------------
def ulp_bf16(v64):
    """Spacing of the bf16 grid in the binade of ``v64`` (8 significant bits; the subnormal spacing below 2^-126)."""
    _, e = torch.frexp(v64.double().abs())
    return torch.ldexp(torch.ones_like(v64, dtype=F64), (e - 1).clamp_min(-126) - 7)


def round_bf16_ties(v64, window):
    """-> (bf16 round-to-nearest-even of ``v64`` as float64, mask of the elements within ``window`` (absolute) of a rounding
    boundary, i.e. of the midpoint between two neighbouring bf16 values)."""
    v64 = v64.double()
    u = ulp_bf16(v64)
    q = v64 / u                                     # exact: u is a power of two
    r = torch.round(q) * u                          # torch.round rounds halves to even
    dist = (q - torch.floor(q) - 0.5).abs() * u
    return r, dist <= window


def round_bf16(v64):
    return round_bf16_ties(v64, 0.0)[0]


def _rounded_mid(mid_fn, window_rows=None):
    """The shared treatment of an inner bf16 rounding: ``mid_fn(dtype)`` evaluates the intermediate; -> (rounded float64, mask, window)."""
    m64, m32 = mid_fn(F64), mid_fn(F32).double()
    d = (m32 - m64).abs()
    if window_rows is not None:
        d = d[window_rows]
    window = 16.0 * (d.max().item() if d.numel() else 0.0)
    r, mask = round_bf16_ties(m64, window)
    return r, mask, window


# ---------------------------------------------------------------------------------------------------------------------------
# index helpers
# ---------------------------------------------------------------------------------------------------------------------------
def group_of_rows(seq, n_text, per_group):
    """``orv_group_of`` of every sequence position: 0 for the text rows, 1 + i for the i-th block of ``per_group`` video rows
    (``per_group`` <= 0: every video row is group 1)."""
    s = torch.arange(seq)
    vid = 1 + (s - n_text) // per_group if per_group > 0 else torch.ones_like(s)
    return torch.where(s < n_text, torch.zeros_like(s), vid)


def n_groups(seq, n_text, per_group):
    return int(group_of_rows(seq, n_text, per_group).max()) + 1


def mapped_rows(n_rows, rmap):
    """Row of the mapped buffer that dense row r addresses: (r // rows) * bstride + off + r % rows; ``rmap`` = (rows, bstride, off)."""
    r = torch.arange(n_rows)
    if rmap is None:
        return r
    rows, bstride, off = rmap
    return (r // rows) * bstride + off + r % rows


def pack_p16(rows, D):
    """Element offset of (r, d) in the packed P16 layout, [rows, D] int64: chunk c = d // 8 of row r is 16-byte slot
    (c & 3) * 16 + (r & 15) of block (r >> 4, c >> 2); blocks are 1 KiB (512 elements), row-block-major."""
    r = torch.arange(rows)[:, None]
    d = torch.arange(D)[None, :]
    c = d >> 3
    block = (r >> 4) * (D >> 5) + (c >> 2)
    slot = (c & 3) * 16 + (r & 15)
    return block * 512 + slot * 8 + (d & 7)


def vt_position(s):
    """Position of key ``s`` on the key axis of V^T: bits 2 and 3 exchanged."""
    return (s & ~12) | ((s & 4) << 1) | ((s & 8) >> 1)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm-modulate
# ---------------------------------------------------------------------------------------------------------------------------
def layernorm_modulate(x, gamma, beta, scale, shift, grp, batch, D, eps, xmap=None, dtype=F64):
    """y[r] = (LN(x[map(r)]) * gamma + beta) * (1 + scale[b, g]) + shift[b, g]; every factor optional.

    ``x`` [rows of the (mapped) buffer, >= D]; ``scale`` / ``shift`` [batch, G, D] (any view); ``grp`` = (seq, n_text, per_group).
    Two-pass statistics, biased variance.  -> [batch * seq, D] in ``dtype``, not rounded."""
    seq, n_text, per_group = grp
    R = batch * seq
    xs = x[mapped_rows(R, xmap)][:, :D].to(dtype)
    mu = xs.sum(1, keepdim=True) / D
    xc = xs - mu
    var = (xc * xc).sum(1, keepdim=True) / D
    y = xc / torch.sqrt(var + _f32(eps))
    if gamma is not None:
        y = y * gamma.to(dtype)
    if beta is not None:
        y = y + beta.to(dtype)
    if scale is not None:
        b = torch.arange(R) // seq
        g = group_of_rows(seq, n_text, per_group).repeat(batch)
        y = y * (1 + scale.to(dtype)[b, g]) + shift.to(dtype)[b, g]
    return y


# ---------------------------------------------------------------------------------------------------------------------------
# qkv_prep
# ---------------------------------------------------------------------------------------------------------------------------
def qkv_prep(src, gq, bq, gk, bk, rope, B, S, H, n_text, eps, q_premul=1.0, dtype=F64):
    """``src`` [B * S, 3 * H * 64] bf16 (q | k | v thirds, head-major).  Per head: LayerNorm(64) of q and k with optional gamma / beta;
    on rows >= n_text (``rope`` = (cos, sin) [S - n_text, 64] fp32) the normalised value is rounded to bf16 and rotated,
    out[2i] = a cos[2i] - c sin[2i], out[2i + 1] = c cos[2i + 1] + a sin[2i + 1] with (a, c) the rounded pair; q is then multiplied
    by ``q_premul`` (once, before the output rounding).  V^T [B, H, 64, s_pad]: key s at ``(s & ~15) | vt_position(s & 15)``, zero padded.

    -> dict: q, k [B, S, H, 64] in ``dtype`` (not rounded); v [B, S, H, 64] bf16 and vT bf16 (bit copies);
       tie_q, tie_k: the bound term of the issue for the flagged pairs, 2^-8 (|a cos| + |c sin|) (times q_premul for q);
       flip_q, flip_k: what a flipped rounding of the flagged elements can move each output by, |cos| ulp(a) + |sin| ulp(c);
       tie_frac: share of the rounded elements that are flagged."""
    x = src.view(B, S, 3, H, 64)
    pm = _f32(q_premul)
    out = {}
    flagged = total = 0
    for which, name, gam, bet in ((0, "q", gq, bq), (1, "k", gk, bk)):
        def normed(dt, which=which, gam=gam, bet=bet):
            xs = x[:, :, which].to(dt)
            mu = xs.sum(-1, keepdim=True) / 64
            xc = xs - mu
            var = (xc * xc).sum(-1, keepdim=True) / 64
            y = xc / torch.sqrt(var + _f32(eps))
            if gam is not None:
                y = y * gam.to(dt)
            if bet is not None:
                y = y + bet.to(dt)
            return y
        y = normed(dtype)
        tie = torch.zeros(B, S, H, 64, dtype=F64)
        flip = torch.zeros(B, S, H, 64, dtype=F64)
        if rope is not None and n_text < S:
            r64, mask, _ = _rounded_mid(normed, (slice(None), slice(n_text, S)))
            r64, mask = r64[:, n_text:], mask[:, n_text:]
            cos, sin = (t[:S - n_text].double()[None, :, None, :] for t in rope)
            a, c = r64[..., 0::2], r64[..., 1::2]
            ma, mc = mask[..., 0::2], mask[..., 1::2]
            ua, uc = ulp_bf16(a) * ma, ulp_bf16(c) * mc
            pair = (ma | mc).double()
            cd, sd, ad, cc = cos.to(dtype), sin.to(dtype), a.to(dtype), c.to(dtype)
            rot = torch.empty(r64.shape, dtype=dtype)
            rot[..., 0::2] = ad * cd[..., 0::2] - cc * sd[..., 0::2]
            rot[..., 1::2] = cc * cd[..., 1::2] + ad * sd[..., 1::2]
            y = torch.cat([y[:, :n_text], rot], dim=1)
            t = tie[:, n_text:]
            t[..., 0::2] = pair * 2.0 ** -8 * ((a * cos[..., 0::2]).abs() + (c * sin[..., 0::2]).abs())
            t[..., 1::2] = pair * 2.0 ** -8 * ((c * cos[..., 1::2]).abs() + (a * sin[..., 1::2]).abs())
            f = flip[:, n_text:]
            f[..., 0::2] = cos[..., 0::2].abs() * ua + sin[..., 0::2].abs() * uc
            f[..., 1::2] = cos[..., 1::2].abs() * uc + sin[..., 1::2].abs() * ua
            flagged += int(mask.sum())
            total += mask.numel()
        if which == 0:
            y, tie, flip = y * pm, tie * abs(pm), flip * abs(pm)
        out[name], out["tie_" + name], out["flip_" + name] = y, tie, flip
    out["tie_frac"] = flagged / total if total else 0.0
    v = x[:, :, 2].contiguous()
    s_pad = (S + 63) // 64 * 64
    vT = torch.zeros(B, H, 64, s_pad, dtype=BF)
    s = torch.arange(S)
    vT[..., (s & ~15) | vt_position(s & 15)] = v.permute(0, 2, 3, 1)
    out["v"], out["vT"] = v, vT
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# activations, written out (the host module compares them with torch.nn.functional)
# ---------------------------------------------------------------------------------------------------------------------------
def silu(v):
    return v / (1 + torch.exp(-v))


def gelu_tanh(v):
    return 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v * v * v)))


ACT = {None: lambda v: v, "silu": silu, "gelu_tanh": gelu_tanh}
ACT_SLOPE = {None: 1.0, "silu": 1.1, "gelu_tanh": 1.13}       # upper bounds of |d act / dv| (1.0998 and 1.1289)


# ---------------------------------------------------------------------------------------------------------------------------
# modulation tables
# ---------------------------------------------------------------------------------------------------------------------------
def modulation_tables(temb, action_emb, Ws, bs, B, T, E, width, text, dtype=F64):
    """out[tab, b, 1 + t] = W_tab[:width] . c_v[b, t] + bias_tab[:width],  c_v = bf16(silu(bf16(temb[b] + a[b, t])))  (no ``a``: T == 1
    and c_v = bf16(silu(temb[b])));  out[tab, b, 0] = W_tab[width:] . bf16(silu(temb[b])) + bias_tab[width:] if ``text``, else 0.

    ``Ws`` list of [width * (1 + text), E] bf16; ``bs`` None or a list whose entries may be None.
    -> dict: out [n_tab, B, 1 + T, width] in ``dtype``; abs_terms (sum |w c| + |bias|); tie (sum over the flagged c_k of |w_k| ulp(c_k));
       tie_frac."""
    def cond(dt):
        t = temb.to(dt)
        if action_emb is None:
            cv = t[:, None, :]
        else:
            # the add is performed in the model dtype: exact in float32 and float64 alike, then rounded to bf16
            cv = round_bf16(temb.double()[:, None, :] + action_emb.double()).to(dt)
        return silu(torch.cat([t[:, None, :], cv], dim=1))          # [B, 1 + T, E]: row 0 is the text conditioning
    c64, mask, _ = _rounded_mid(cond)
    cu = ulp_bf16(c64) * mask
    n_tab = len(Ws)
    out = torch.zeros(n_tab, B, 1 + T, width, dtype=dtype)
    abs_terms = torch.zeros(n_tab, B, 1 + T, width, dtype=F64)
    tie = torch.zeros(n_tab, B, 1 + T, width, dtype=F64)
    for i, W in enumerate(Ws):
        bias = None if bs is None else bs[i]
        for lo, rows in ((0, slice(1, None)),) + (((width, slice(0, 1)),) if text else ()):
            Wd = W[lo:lo + width]
            o = c64[:, rows].to(dtype) @ Wd.to(dtype).t()
            a = c64[:, rows].abs() @ Wd.double().abs().t()
            if bias is not None:
                o = o + bias[lo:lo + width].to(dtype)
                a = a + bias[lo:lo + width].double().abs()
            out[i, :, rows], abs_terms[i, :, rows] = o, a
            tie[i, :, rows] = cu[:, rows] @ Wd.double().abs().t()
    used = mask if text else mask[:, 1:]
    return {"out": out, "abs_terms": abs_terms, "tie": tie, "tie_frac": used.double().mean().item(), "cond": c64}


# ---------------------------------------------------------------------------------------------------------------------------
# skinny_linear
# ---------------------------------------------------------------------------------------------------------------------------
def skinny_linear(x, W, bias=None, xb=None, xb_rep=1, act_in=None, act_out=None, dtype=F64):
    """out[m] = act_out(W . bf16(act_in(bf16(x[m] + xb[m // xb_rep]))) + bias);  x [M, K], W [N, K], xb [ceil(M / xb_rep), K] bf16.

    -> dict: out [M, N] in ``dtype`` (not rounded); pre (the value before act_out); abs_terms (sum |w x| + |bias|); tie (already
       multiplied by the slope bound of act_out); a_act (max |act_out in float32 - in float64| on the float64 pre-activation); tie_frac."""
    M, K = x.shape
    s = x.double()
    if xb is not None:
        s = round_bf16(s + xb.double()[torch.arange(M) // xb_rep])      # model-dtype add: exact, then one rounding
    st64, mask, _ = _rounded_mid(lambda dt: ACT[act_in](s.to(dt)))
    su = ulp_bf16(st64) * mask
    pre = st64.to(dtype) @ W.to(dtype).t()
    abs_terms = st64.abs() @ W.double().abs().t()
    if bias is not None:
        pre = pre + bias.to(dtype)
        abs_terms = abs_terms + bias.double().abs()
    tie = (su @ W.double().abs().t()) * ACT_SLOPE[act_out]
    pre64 = pre.double() if dtype == F64 else None
    a_act = 0.0
    if act_out is not None and pre64 is not None:
        a_act = (ACT[act_out](pre64.float()).double() - ACT[act_out](pre64)).abs().max().item()
    return {"out": ACT[act_out](pre), "pre": pre, "abs_terms": abs_terms, "tie": tie, "a_act": a_act,
            "tie_frac": mask.double().mean().item()}


# ---------------------------------------------------------------------------------------------------------------------------
# timestep embedding, scheduler step, row kernels
# ---------------------------------------------------------------------------------------------------------------------------
def timestep_embedding(t, dim, flip_sin_to_cos=True, freq_shift=0.0, dtype=F64):
    """emb[b] = [sin(t_b f_k) | cos(t_b f_k)], f_k = exp(-ln(10000) k / (dim // 2 - freq_shift)); halves exchanged when
    ``flip_sin_to_cos``; an odd ``dim`` has a zero last column.  ``t`` fp32 [batch]."""
    half = dim // 2
    k = torch.arange(half, dtype=dtype)
    f = torch.exp(-math.log(10000.0) * k / (half - _f32(freq_shift)))
    a = t.to(dtype)[:, None] * f[None, :]
    first, second = (torch.cos(a), torch.sin(a)) if flip_sin_to_cos else (torch.sin(a), torch.cos(a))
    out = torch.zeros(t.numel(), dim, dtype=dtype)
    out[:, :half], out[:, half:2 * half] = first, second
    return out


def sched_step(x, v_c, v_u, guidance_scale, old_x0, noise, sa, sb, m3, m4, cx, cd, cn, dtype=F64):
    """v = v_u + gs (v_c - v_u) (no v_u: v_c);  x0 = sa x - sb v;  d = m3 x0 - m4 old_x0 (no old_x0: x0);  x' = cx x + cd d + cn noise.

    -> dict: x (not rounded), x0, abs_x0 (sum of the |terms| of x0 written out over x, v_c, v_u), n_x0 (their number)."""
    sa, sb, m3, m4, cx, cd, cn, gs = (_f32(c) for c in (sa, sb, m3, m4, cx, cd, cn, guidance_scale))
    xv, v = x.to(dtype).flatten(), v_c.to(dtype).flatten()
    abs_v, n = v.double().abs(), 2
    if v_u is not None:
        u = v_u.to(dtype).flatten()
        abs_v, n = u.double().abs() * (1 + abs(gs)) + abs(gs) * v.double().abs(), 4
        v = u + gs * (v - u)
    x0 = sa * xv - sb * v
    d = x0 if old_x0 is None else m3 * x0 - m4 * old_x0.to(dtype).flatten()
    r = cx * xv + cd * d
    if noise is not None:
        r = r + cn * noise.to(dtype).flatten()
    return {"x": r, "x0": x0, "abs_x0": abs(sa) * xv.double().abs() + abs(sb) * abs_v, "n_x0": n}


def add_rows(a, amap, b, M, D):
    """out[m] = bf16(a[amap(m)] + b[m]): one fp32 add of two bf16 values, rounded once.  -> bf16 [M, D]"""
    return (a[mapped_rows(M, amap)][:, :D].float() + b[:M, :D].float()).to(BF)


def gather_rows(src, idx, D):
    return src[idx.long()][:, :D]


def scatter_gated_rows(x, y, idx, gate, seq, n_text, D, dtype=F64):
    """x[idx[r]] += gate[idx[r] // seq] * y[r] for the rows whose target is a video row (idx[r] % seq >= n_text); ``idx`` distinct.
    ``gate`` [batch, D] fp32.  -> (x' [rows, D] in ``dtype``, not rounded; bool mask of the rows that were updated)"""
    il = idx.long()
    out = x[:, :D].to(dtype).clone()
    vid = (il % seq) >= n_text
    out[il[vid]] += gate.to(dtype)[il[vid] // seq] * y[:, :D].to(dtype)[vid]
    touched = torch.zeros(x.shape[0], dtype=torch.bool)
    touched[il[vid]] = True
    return out, touched


# ---------------------------------------------------------------------------------------------------------------------------
# case tables (shared by the host and the GPU module) and their inputs
# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm-modulate, rows-per-wave kernel (full form, no row map, D <= 2048): name -> (D, batch, seq, n_text, per_group, wide table)
# "wide": scale / shift are the [..., D:2D] / [..., :D] slices of a 6 D-wide table (mod_b, mod_g larger than the dense strides).
LN_ROWS_CASES = {
    "d8_r1": (8, 3, 25, 3, 5, True),               # ln_mod_rows_kernel<1>, R = 1, one active lane
    "d512_r1": (512, 3, 25, 3, 5, False),          # <1>, chunk group exactly full
    "d520_r1": (520, 3, 25, 3, 5, True),           # <2>, one lane in the second group
    "d1024_r1": (1024, 3, 25, 3, 5, False),        # <2>, both groups full
    "d1032_r1": (1032, 3, 25, 3, 5, True),         # ch = 3 -> <4>
    "d2048_r1": (2048, 3, 25, 3, 5, True),         # <4>, all four groups full
    "d8_r2": (8, 3, 683, 7, 97, False),            # <1>, R = 2 over 2049 rows: rows (682, 683) straddle the batch, (6, 7) the text / video
    "d520_r2": (520, 3, 683, 7, 97, True),         # <2>, R = 2, ragged last wave (row 2048 alone)
    "d1032_r2": (1032, 3, 683, 7, 97, False),      # <4>, R = 2
    "d64_r4": (64, 71, 131, 7, 31, True),          # <1>, R = 4 over 9301 rows: group change, batch boundary and last row inside a wave's rows
}
# packed output (ln_mod_rows_kernel<CH, PACKED>): name -> (D, batch, seq, n_text, per_group, wide)
LN_PACKED_CASES = {
    "d32_75": (32, 3, 25, 3, 5, True),             # <1, true>: 4 live lanes, 60 clamped lanes re-store the last chunk; ragged 16-row block
    "d1920_75": (1920, 3, 25, 3, 5, True),         # <4, true>: the model width
    "d2048_75": (2048, 3, 25, 3, 5, False),        # <4, true>: the widest packed form
    "d32_2049": (32, 3, 683, 7, 97, False),        # <1, true>, R = 2
    "d1920_2049": (1920, 3, 683, 7, 97, True),     # <4, true>, R = 2
    "d2048_2049": (2048, 3, 683, 7, 97, True),     # <4, true>, R = 2
}
# one-row kernel, full form with a table, 37 rows (the last workgroup has one live wave): D -> instantiation
LN_ONE_ROW_WIDTHS = {
    2056: "ln_mod_kernel<6, true>: ch = 5, one lane in the fifth group",
    3072: "ln_mod_kernel<6, true>: six groups full",
    3080: "ln_mod_kernel<8, true>: ch = 7",
    4096: "ln_mod_kernel<8, true>: the maximum",
}
LN_ONE_ROW_GRP = (1, 37, 5, 8)                      # batch, seq, n_text, per_group
# one-row kernel, partial forms (ln_mod_kernel<CH, false>, CH by LN_PARTIAL_WIDTHS below): name -> (gamma, beta, table)
LN_PARTIAL_FORMS = {
    "gamma_beta": (True, True, False),             # norm_final
    "gamma": (True, False, False),
    "beta": (False, True, False),
    "table": (False, False, True),
    "nothing": (False, False, False),
}
# widths of the partial-form cases: D -> the CH of ln_mod_kernel<CH, false> (and of <CH, true> for the full form behind a row map)
LN_PARTIAL_WIDTHS = {
    128: 1,                                        # ln_mod_kernel<1, ..>: 16 live lanes
    520: 2,                                        # ln_mod_kernel<2, ..>: one lane in the second chunk group
    1024: 2,                                       # ln_mod_kernel<2, ..>: both groups full
    1920: 4,                                       # ln_mod_kernel<4, ..>: the model width
}
LN_PARTIAL_GEOM = (2, 32, 5, 8)                     # batch, video rows, text rows of the joint buffer, per_group of the table form


def ln_inputs(D, batch, seq, n_text, per_group, wide, seed, rows_x=None, ldx=None):
    g = torch.Generator().manual_seed(seed)
    G = n_groups(seq, n_text, per_group)
    x = rb(g, rows_x or batch * seq, ldx or D, mul=2.0, add=0.3)
    tab = torch.randn(batch, G, 6 * D if wide else 2 * D, generator=g) * 0.5
    return {"x": x, "gamma": rb(g, D, add=1.0, mul=0.3), "beta": rb(g, D, mul=0.5), "tab": tab, "shift": tab[..., :D],
            "scale": tab[..., D:2 * D], "mod_b": tab.stride(0), "mod_g": tab.stride(1)}


# qkv_prep: (S, H, form, factors, rope).  B = 2 everywhere: batch 1's rows sit directly after batch 0's last row.  Every case runs with
# q_premul = 1 and 0.125 log2(e).  form: in place / out of place (src=), with / without V^T; factors: all four, biases null, all null;
# rope: n_text = 0, 5, S - 1, S (the tables are never read: a one-row dummy).  One kernel (qkv_prep_kernel); the comments name the path.
QKV_CASES = [
    (1, 1, "inplace_vt", "all", "nt0"),            # one live row, 63 clamped ones; V^T tile with 63 zero keys
    (8, 1, "inplace", "nobias", "ntS"),            # the shipped form; rope tables present but no row reads them
    (15, 1, "from_vt", "none", "nt5"),             # out of place + V^T: the v third copied by the LDS staging loop
    (16, 1, "from", "all", "ntS-1"),               # out of place without V^T: the early-return copy loop; one rope row
    (17, 1, "inplace_vt", "nobias", "nt5"),        # first row of the second wave
    (63, 1, "inplace", "none", "nt0"),
    (64, 1, "from_vt", "all", "ntS"),              # exactly one tile
    (65, 1, "from", "nobias", "nt0"),              # second tile with one row
    (129, 1, "inplace_vt", "none", "ntS-1"),       # three tiles
    (65, 3, "inplace_vt", "all", "nt5"),           # H = 3: head offsets inside the row, every form
    (65, 3, "inplace", "all", "nt5"),
    (65, 3, "from_vt", "nobias", "nt5"),
    (65, 3, "from", "none", "nt5"),
    (129, 1, "inplace", "all", "nt0"),             # the shipped form with every row rotated
]
QKV_PREMULS = (1.0, 0.125 * LOG2E)


def qkv_n_text(S, rope):
    return {"nt0": 0, "nt5": 5, "ntS-1": S - 1, "ntS": S}[rope]


def qkv_inputs(case, seed):
    S, H, form, factors, rope = case
    B = 2
    g = torch.Generator().manual_seed(seed)
    nt = qkv_n_text(S, rope)
    src = ru(g, B * S, 3 * H * 64, lo=-2.5, hi=3.0)
    f = {"gq": rb(g, 64, add=1.0, mul=0.3), "bq": rb(g, 64, mul=0.3), "gk": rb(g, 64, add=1.0, mul=0.3), "bk": rb(g, 64, mul=0.3)}
    if factors == "nobias":
        f["bq"] = f["bk"] = None
    elif factors == "none":
        f = dict.fromkeys(f)
    ang = torch.rand(max(S - nt, 1), 64, generator=g) * 6.0
    amp = 0.5 + torch.rand(max(S - nt, 1), 64, generator=g)          # cos / sin per element, not per pair: a swapped index shows
    return {"src": src, "rope": ((amp * ang.cos()).float(), (amp * ang.sin()).float()), "n_text": nt, "B": B, **f}


# modulation tables: (B, T, E, width, text, action_emb, bias).  bias: "all", "tab1" (the second table's bias pointer is null), "none" (no
# pointer array).  width 544 = 17 blocks is ragged against both grids; widths 32 and 96 leave LDS-kernel waves without a block.
MOD_CASES = [
    (1, 1, 64, 32, True, False, "all"),            # mod_tables_kernel<4>, B T = 1, no action embedding
    (4, 8, 64, 96, True, True, "tab1"),            # <4>, B T = 32: one full row tile
    (33, 1, 64, 544, False, False, "all"),         # <4>, B T = 33: second video tile; text off: row 0 stays zero
    (3, 11, 128, 32, True, True, "all"),           # mod_tables_kernel<8>, B T = 33
    (4, 8, 128, 544, True, True, "none"),          # <8>, no bias at all
    (1, 1, 128, 96, False, True, "all"),           # <8>, B T = 1
    (33, 1, 256, 544, True, True, "all"),          # mod_tables_kernel<16>, B = 33 with text: second text tile
    (2, 16, 256, 96, False, True, "tab1"),         # <16>, B T = 32
    (1, 1, 256, 32, True, True, "all"),            # <16>, B T = 1
    (11, 3, 512, 544, True, True, "all"),          # mod_tables_lds_kernel, B T = 33, 17 blocks: waves with 3 and 2 blocks
    (33, 1, 512, 96, True, True, "tab1"),          # lds kernel, second text tile, wave 3 without a block
    (1, 1, 512, 32, False, True, "all"),           # lds kernel, three waves without a block
    (32, 1, 512, 32, True, False, "none"),         # lds kernel, B T = 32, no action embedding (T = 1), no bias
]
MOD_CHILD_CASE = (11, 3, 512, 544, True, True, "all")       # once more with ORV_MOD_TABLES_LDS=0: mod_tables_kernel<32>
MOD_NTAB = 2


def mod_inputs(case, seed):
    B, T, E, width, text, with_act, bias = case
    if not with_act:
        T = 1
    g = torch.Generator().manual_seed(seed)
    rows = width * (2 if text else 1)
    Ws = [rb(g, rows, E, mul=0.05) for _ in range(MOD_NTAB)]
    bs = [rb(g, rows) for _ in range(MOD_NTAB)]
    if bias == "tab1":
        bs[1] = None
    return {"temb": ru(g, B, E, lo=-2.0, hi=2.0), "act": ru(g, B, T, E, lo=-0.5, hi=0.5) if with_act else None, "Ws": Ws, "bs": None if bias == "none" else bs,
            "B": B, "T": T, "E": E, "width": width, "text": text}


# skinny_linear: name -> dict(M, N, K, + options).  out: "bf16" / "f32"; ldo_pad: ldo = N + ldo_pad; omap: (rows, bstride, off)
SKINNY_CASES = {
    "1x1x8": dict(M=1, N=1, K=8),                                   # one output, one chunk, one live lane
    "16x5x64": dict(M=16, N=5, K=64),                               # a full 16-row block, 8 live lanes
    "17x28x28": dict(M=17, N=28, K=28),                             # second block with one row; K % 8 != 0: scalar tail only
    "3x9x4": dict(M=3, N=9, K=4),                                   # the smallest K the launcher accepts
    "5x7x60": dict(M=5, N=7, K=60),                                 # scalar tail at its upper end (K <= 64)
    "33x40x520": dict(M=33, N=40, K=520),                           # three row blocks; chunk 64 wraps to lane 0
    "3x8x2056": dict(M=3, N=8, K=2056),                             # 65 792 bytes of LDS: the hipFuncSetAttribute path
    "3x8x5120": dict(M=3, N=8, K=5120),                             # 160 KiB: the limit the launcher advertises
    "xb_rep17": dict(M=34, N=9, K=64, xb_rep=17, act_in="silu"),    # block 1 (rows 16..31) straddles the xb boundary at row 17
    "f32_omap": dict(M=10, N=24, K=72, out="f32", ldo_pad=8, omap=(5, 6, 1), xb_rep=5, act_in="silu"),   # the AdaLN table form
    "f32_act": dict(M=7, N=12, K=40, out="f32", act_out="gelu_tanh"),
    "bf16_ldo": dict(M=19, N=12, K=40, ldo_pad=8),                  # bf16 output with ldo = N + 8
    "no_bias": dict(M=19, N=12, K=40, bias=False),
}
for _ai in (None, "silu", "gelu_tanh"):
    for _ao in (None, "silu", "gelu_tanh"):
        SKINNY_CASES[f"act_{_ai}_{_ao}"] = dict(M=16, N=5, K=64, act_in=_ai, act_out=_ao)      # apply_act on both sides
# npw = 2 (every case above ends at one column per wave): two columns per wave, and the last wave leaves its loop at n >= N after one
SKINNY_CASES["16x2051x8"] = dict(M=16, N=2051, K=8)


def skinny_inputs(name, seed):
    c = SKINNY_CASES[name]
    M, N, K = c["M"], c["N"], c["K"]
    g = torch.Generator().manual_seed(seed)
    rep = c.get("xb_rep")
    return {"x": ru(g, M, K, lo=-2.0, hi=2.0), "W": rb(g, N, K, mul=1.0 / math.sqrt(K)), "bias": rb(g, N) if c.get("bias", True) else None,
            "xb": ru(g, -(-M // rep), K, lo=-0.5, hi=0.5) if rep else None, "xb_rep": rep or 1, "act_in": c.get("act_in"), "act_out": c.get("act_out")}


# timestep embedding
TS_DIMS = (2, 6, 7, 512)                  # one frequency; three; odd (zero last column); the model's
TS_VALUES = (0.0, 0.5, 19.0, 999.0)

# sched_step: (n, coefficient set, v_u, old_x0, noise, want_x0).  Coefficient sets (``sched_coefficients``): 0-5 DDIM, 6-11 DPM, each
# first / middle / last step of a 3-step then a 50-step schedule.  old_x0 is dropped where the schedule has no finite m3 / m4.
SCHED_NS = (1, 255, 257)                  # one thread; one block short of full; one element in the second block
SCHED_CASES = [(SCHED_NS[i % 3], (5 * i) % 12, bool(i & 1), bool(i & 2), bool(i & 4), bool(i & 8)) for i in range(16)]


def sched_coefficients():
    """-> 12 dicts (sa, sb, m3, m4, cx, cd, cn) from ``oracle.leaf``'s schedulers."""
    from oracle import leaf
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
              set_alpha_to_one=True, prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=3.0,
              timestep_spacing="trailing")
    out = []
    for dpm in (False, True):
        for steps in (3, 50):
            s = (leaf.CogVideoXDPMScheduler if dpm else leaf.CogVideoXDDIMScheduler)(**kw)
            s.set_timesteps(steps)
            ts = s.timesteps.tolist()
            for i in (0, steps // 2, steps - 1):
                t = ts[i]
                prev = t - 1000 // steps
                a_t = s.alphas_cumprod[t]
                a_p = s.alphas_cumprod[prev] if prev >= 0 else s.final_alpha_cumprod
                c = {"sa": float(a_t ** 0.5), "sb": float((1 - a_t) ** 0.5), "m3": None, "m4": None, "cn": 0.0, "t": t, "steps": steps,
                     "dpm": dpm, "t_back": ts[i - 1] if i else None}
                if dpm:
                    m1, m2, mn, m3, m4 = s.coefficients(a_t, a_p, s.alphas_cumprod[ts[i - 1]] if i else None)
                    c.update(cx=float(m1), cd=-float(m2), cn=float(mn))
                    if m3 is not None and math.isfinite(float(m3)) and math.isfinite(float(m4)):
                        c.update(m3=float(m3), m4=float(m4))
                else:
                    A = ((1 - a_p) / (1 - a_t)) ** 0.5
                    c.update(cx=float(A), cd=float(a_p ** 0.5 - a_t ** 0.5 * A))
                out.append(c)
    return out


ROW_DS = (8, 136)                         # one chunk per row; 17 chunks: a 256-thread block ends inside a row


# Seeds of the cases that round an intermediate, chosen (from the reference alone) so that the tie cap of the host module holds with a
# margin: at most 1.4 % of the rounded elements lie within the window of a rounding boundary.
QKV_SEEDS = [101, 110, 121, 133, 141, 150, 160, 170, 181, 193, 201, 211, 223, 233]
MOD_SEEDS = [201, 212, 225, 231, 243, 250, 260, 270, 284, 294, 302, 311, 320]
MOD_CHILD_SEED = MOD_SEEDS[MOD_CASES.index(MOD_CHILD_CASE)]
SKINNY_SEEDS = dict(zip(SKINNY_CASES, [300, 310, 320, 330, 340, 350, 360, 370, 388, 399, 400, 410, 420, 430, 440, 450, 465, 470, 484, 496, 507,
                                       516, 520]))


def tie_cases():
    """Every case whose restatement rounds an intermediate: (family, id, thunk -> restatement dict).  The seeds are fixed here, so the
    host module checks the tie cap on exactly the inputs the GPU module runs."""
    items = []
    for i, c in enumerate(QKV_CASES):
        for pm in QKV_PREMULS:
            items.append(("qkv_prep", f"{i}-{pm:.3f}", lambda i=i, c=c, pm=pm: qkv_reference(c, qkv_inputs(c, QKV_SEEDS[i]), pm)))
    for i, c in enumerate(MOD_CASES):
        items.append(("mod_tables", str(i), lambda i=i, c=c: mod_reference(mod_inputs(c, MOD_SEEDS[i]))))
    for i, name in enumerate(SKINNY_CASES):
        items.append(("skinny_linear", name, lambda i=i, name=name: skinny_reference(skinny_inputs(name, SKINNY_SEEDS[name]))))
    return items


def qkv_reference(case, inp, q_premul, dtype=F64):
    S, H = case[0], case[1]
    rope = inp["rope"] if inp["n_text"] < S else None           # n_text = S: the dummy tables are never read
    return qkv_prep(inp["src"], inp["gq"], inp["bq"], inp["gk"], inp["bk"], rope, inp["B"], S, H, inp["n_text"], 1e-6, q_premul, dtype)


def mod_reference(inp, dtype=F64):
    return modulation_tables(inp["temb"], inp["act"], inp["Ws"], inp["bs"], inp["B"], inp["T"], inp["E"], inp["width"], inp["text"], dtype)


def skinny_reference(inp, dtype=F64):
    return skinny_linear(inp["x"], inp["W"], inp["bias"], inp["xb"], inp["xb_rep"], inp["act_in"], inp["act_out"], dtype)
