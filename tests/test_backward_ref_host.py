"""The float64 restatements of ``tests/backward_ref.py`` against ``torch.autograd`` in float64 through the plain forward op
(``F.layer_norm`` + modulate, gate * y, ``F.linear``, LayerNorm(64) + the rotation of ``leaf.apply_rotary_emb``, softmax attention,
the AdaLN linears).  Agreement to 1e-9 of max|ref|: this is the only check of the reference the GPU tests measure the kernels against."""
import math

import pytest
import torch
import torch.nn.functional as F

import backward_ref as ref

F64 = torch.float64


def same(got, want, what=""):
    err = (got - want).abs().max().item()
    assert err <= 1e-9 * max(want.abs().max().item(), 1e-300), (what, err, want.abs().max().item())


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


@pytest.mark.parametrize("batch,seq,n_text,per_group,D", [(2, 11, 3, 4, 16), (1, 9, 0, 3, 24), (2, 7, 2, 0, 8)])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("mod", [True, False])
@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("mapped", [True, False])
def test_ln_mod_bwd_matches_autograd(batch, seq, n_text, per_group, D, affine, mod, res, mapped):
    g = torch.Generator().manual_seed(seq * 100 + D)
    R = batch * seq
    xmap = (seq, seq + 5, 2) if mapped else None
    rows = ref.mapped_rows(R, xmap)
    x = (rnd(g, batch * (seq + 5) + 2 if mapped else R, D) * 2 + 0.3).requires_grad_()
    gamma, beta = (rnd(g, D).requires_grad_(), rnd(g, D).requires_grad_()) if affine else (None, None)
    G = ref.n_groups(seq, n_text, per_group)
    scale, shift = (rnd(g, batch, G, D).requires_grad_(), rnd(g, batch, G, D).requires_grad_()) if mod else (None, None)
    dy = rnd(g, R, D)
    dres = rnd(g, *x.shape) if res else None
    grp = ref.group_of_rows(seq, n_text, per_group).repeat(batch)
    b = torch.arange(R) // seq
    y = F.layer_norm(x[rows], (D,), gamma, beta, 1e-5)
    if mod:
        y = y * (1 + scale[b, grp]) + shift[b, grp]
    y.backward(dy)
    got = ref.ln_mod_bwd(dy, x.detach(), dres, None if gamma is None else gamma.detach(), None if beta is None else beta.detach(),
                         None if scale is None else scale.detach(), (seq, n_text, per_group), 1e-5, xmap)
    want_dx = x.grad[rows] + (dres[rows] if res else 0)
    same(got["dx"][rows], want_dx, "dx")
    untouched = torch.ones(x.shape[0], dtype=torch.bool)
    untouched[rows] = False
    assert torch.isnan(got["dx"][untouched]).all() and torch.equal(got["rows"], rows)
    if affine:
        same(got["dgamma"], gamma.grad, "dgamma"), same(got["dbeta"], beta.grad, "dbeta")
    if mod:
        same(got["dscale"], scale.grad, "dscale"), same(got["dshift"], shift.grad, "dshift")
    for k in ("dgamma", "dbeta", "dscale", "dshift"):
        assert (got["abs_" + k] >= got[k].abs() * (1 - 1e-12)).all()
    assert int(got["group_rows"].sum()) == R


@pytest.mark.parametrize("batch,seq,n_text,per_group,D", [(2, 11, 3, 4, 16), (3, 10, 0, 5, 8)])
def test_gated_bwd_matches_autograd(batch, seq, n_text, per_group, D):
    g = torch.Generator().manual_seed(seq)
    R = batch * seq
    G = ref.n_groups(seq, n_text, per_group)
    yb, dout = rnd(g, R, D).requires_grad_(), rnd(g, R, D)
    gate = rnd(g, batch, G, D).requires_grad_()
    grp = ref.group_of_rows(seq, n_text, per_group).repeat(batch)
    (gate[torch.arange(R) // seq, grp] * yb).backward(dout)
    got = ref.gated_bwd(dout, yb.detach(), gate.detach(), (seq, n_text, per_group))
    same(got["dy"], yb.grad, "dy"), same(got["dgate"], gate.grad, "dgate")
    assert (got["abs_dgate"] >= got["dgate"].abs() * (1 - 1e-12)).all()
    if n_text == 0:
        assert (got["group_rows"][:, 0] == 0).all() and (got["dgate"][:, 0] == 0).all()


@pytest.mark.parametrize("R,N,K", [(3, 5, 7), (9, 4, 6)])
@pytest.mark.parametrize("with_w", [True, False])
def test_small_linear_bwd_matches_autograd(R, N, K, with_w):
    g = torch.Generator().manual_seed(R)
    x, W, b = rnd(g, R, K).requires_grad_(), rnd(g, N, K).requires_grad_(), rnd(g, N).requires_grad_()
    dy = rnd(g, R, N)
    F.linear(x, W, b).backward(dy)
    got = ref.small_linear_bwd(dy, x.detach(), W.detach() if with_w else None)
    same(got["dW"], W.grad, "dW"), same(got["db"], b.grad, "db")
    if with_w:
        same(got["dx"], x.grad, "dx")
        assert (got["abs_dx"] >= got["dx"].abs() * (1 - 1e-12)).all()
    else:
        assert got["dx"] is None and got["abs_dx"] is None


def _rotary64(x, rope):
    """``oracle.leaf.apply_rotary_emb`` without its cast to float32 (that cast alone costs 1e-7): the same three lines in the dtype
    of ``x``; ``test_rotary64_is_the_oracle_rotation`` holds the two together."""
    cos, sin = rope[0][None, None], rope[1][None, None]
    xr, xi = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    rot = torch.stack([-xi, xr], dim=-1).flatten(3)
    return x * cos + rot * sin


def test_rotary64_is_the_oracle_rotation():
    from oracle import leaf
    g = torch.Generator().manual_seed(4)
    x = rnd(g, 2, 3, 5, 64)
    ang = torch.rand(5, 32, generator=g, dtype=F64) * 6.28
    rope = (ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous())
    want = leaf.apply_rotary_emb(x, rope)                               # evaluated in float32 inside
    assert (_rotary64(x, rope) - want).abs().max().item() <= 4 * 2.0 ** -24 * want.abs().max().item()
    same(ref.rope_apply(x, rope, 0), _rotary64(x, rope), "rope_apply")
    same(ref.rope_apply(x, (rope[0][2:], rope[1][2:]), 2)[:, :, 2:], _rotary64(x[:, :, 2:], (rope[0][2:], rope[1][2:])), "rope_apply n_text")
    assert torch.equal(ref.rope_apply(x, (rope[0][2:], rope[1][2:]), 2)[:, :, :2], x[:, :, :2])


def _qk_forward(raw, gq, bq, gk, bk, rope, n_text, eps):
    x = raw.permute(2, 0, 3, 1, 4)                                    # [3, B, H, S, 64]
    out = []
    for xs, gam, bet in ((x[0], gq, bq), (x[1], gk, bk)):
        z = F.layer_norm(xs, (64,), gam, bet, eps)
        if rope is not None:
            z = torch.cat([z[:, :, :n_text], _rotary64(z[:, :, n_text:], rope)], dim=2)
        out.append(z)
    return out[0], out[1], x[2]


@pytest.mark.parametrize("B,S,H,n_text,use_rope,affine", [(2, 9, 2, 3, True, True), (1, 5, 1, 0, False, True), (1, 6, 3, 0, True, False),
                                                          (2, 5, 1, 4, True, True)])
def test_qkv_prep_bwd_matches_autograd(B, S, H, n_text, use_rope, affine):
    g = torch.Generator().manual_seed(S)
    raw = (rnd(g, B, S, 3, H, 64) * 1.5).requires_grad_()
    gq, bq, gk, bk = ((rnd(g, 64) * 0.5 + 1).requires_grad_() if affine else None for _ in range(4))
    rope = None
    if use_rope:
        ang = torch.rand(S - n_text, 32, generator=g, dtype=F64) * 6.28
        rope = (ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous())
    qq, kk, _ = _qk_forward(raw, gq, bq, gk, bk, rope, n_text, 1e-6)
    dq, dk = rnd(g, B, S, H, 64), rnd(g, B, S, H, 64)
    ((qq * dq.transpose(1, 2)).sum() + (kk * dk.transpose(1, 2)).sum()).backward()
    det = lambda t: None if t is None else t.detach()
    got = ref.qkv_prep_bwd(raw.detach(), dq, dk, det(gq), det(gk), rope, n_text, 1e-6)
    same(got["draw_q"], raw.grad[:, :, 0], "draw_q"), same(got["draw_k"], raw.grad[:, :, 1], "draw_k")
    assert raw.grad[:, :, 2].abs().max().item() == 0
    if affine:
        for name, p in (("dgq", gq), ("dbq", bq), ("dgk", gk), ("dbk", bk)):
            same(got[name], p.grad, name)
            assert (got["abs_" + name] >= got[name].abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("B,H,S", [(2, 2, 7), (1, 3, 70)])
def test_attention_bwd_matches_autograd(B, H, S):
    g = torch.Generator().manual_seed(S)
    scale = 0.125
    q, k, v = (rnd(g, B, H, S, 64).requires_grad_() for _ in range(3))
    do = rnd(g, B, H, S, 64)
    sc = scale * (q @ k.transpose(-1, -2))
    o = torch.softmax(sc, dim=-1) @ v
    o.backward(do)
    got = ref.attention_bwd(q.detach() * (scale * ref.LOG2E), k.detach(), v.detach(), do, scale)
    same(got["out"], o.detach(), "out"), same(got["lse"], torch.logsumexp(sc.detach(), dim=-1), "lse")
    same(got["dq"], q.grad, "dq"), same(got["dk"], k.grad, "dk"), same(got["dv"], v.grad, "dv")


@pytest.mark.parametrize("n_tab,B,T,E,width,text", [(2, 2, 3, 8, 6, True), (1, 3, 1, 4, 5, False)])
def test_mod_tables_bwd_matches_autograd(n_tab, B, T, E, width, text):
    g = torch.Generator().manual_seed(B * 10 + T)
    ntot = width * (2 if text else 1)
    Ws = [rnd(g, ntot, E).requires_grad_() for _ in range(n_tab)]
    bs = [rnd(g, ntot).requires_grad_() for _ in range(n_tab)]
    cond_v, cond_t = rnd(g, B * T, E).requires_grad_(), rnd(g, B, E).requires_grad_()
    dtab = rnd(g, n_tab, B, 1 + T, width)
    loss = 0
    for t in range(n_tab):
        vid = F.linear(cond_v, Ws[t][:width], bs[t][:width]).view(B, T, width)
        loss = loss + (vid * dtab[t][:, 1:]).sum()
        if text:
            loss = loss + (F.linear(cond_t, Ws[t][width:], bs[t][width:]) * dtab[t][:, 0]).sum()
    loss.backward()
    got = ref.mod_tables_bwd(dtab, cond_v.detach(), cond_t.detach(), [w.detach() for w in Ws], text)
    for t in range(n_tab):
        same(got["gW"][t], Ws[t].grad, "gW"), same(got["gb"][t], bs[t].grad, "gb")
    same(got["d_cond_v"], cond_v.grad, "d_cond_v")
    if text:
        same(got["d_cond_t"], cond_t.grad, "d_cond_t")
    else:
        assert got["d_cond_t"] is None


def test_float32_evaluation_is_a_yardstick_not_the_reference():
    """``dtype=torch.float32`` evaluates the same formulas in fp32: close to, and distinct from, the float64 result."""
    g = torch.Generator().manual_seed(0)
    dy, x = rnd(g, 12, 64).to(torch.bfloat16), rnd(g, 12, 64).to(torch.bfloat16)
    a = ref.ln_mod_bwd(dy, x, None, None, None, None, (12, 0, 0), 1e-5)
    b = ref.ln_mod_bwd(dy, x, None, None, None, None, (12, 0, 0), 1e-5, dtype=torch.float32)
    assert a["dx"].dtype == F64 and b["dx"].dtype == torch.float32
    err = (a["dx"] - b["dx"].double()).abs().max().item()
    assert 0 < err < 1e-4 * a["dx"].abs().max().item()
    assert math.isclose(ref.LOG2E, 1 / math.log(2), rel_tol=1e-15)
