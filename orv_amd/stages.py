"""Forward stages that the inference path (``CogVideoXTransformer3DModelTraj._forward_inference``) and the training path
(``training.forward_train``) share: everything ahead of the transformer blocks (``embed``) and everything after them (``head``).

``embed`` runs in one of two modes.  ``keep=None`` is the no-grad path, captured into a HIP graph by ``GraphedTransformer``: nothing in it
may sync with the host or allocate beyond what it returns.  With a ``keep`` object it stores the activations ``training.backward`` reads
as attributes of that object.  The two modes issue the same kernels on the same operands with ONE exception, ``mlp2`` below.
"""
from __future__ import annotations

import dataclasses
from types import SimpleNamespace
from typing import Optional

import torch

from . import ops

BF16 = torch.bfloat16


@dataclasses.dataclass
class Shapes:
    """Sizes of one forward.  ``B`` counts clips after the views are folded into the batch ((b0 v) f ...), ``P`` the spatial tokens of one
    latent frame, ``Nv = Tq * P`` the video tokens, ``S = Nt + Nv`` the rows of one clip in the joint buffer, ``M = B * S``."""
    B: int
    b0: int
    nv: int
    T: int
    Hh: int
    Ww: int
    C: int
    p: int
    pt: Optional[int]
    Tq: int
    P: int
    Nv: int
    Nt: int
    S: int
    M: int
    D: int
    heads: int
    E: int
    mod_text: bool
    # known after the action stage of ``embed``: action frames, modulation groups (text + frames), video tokens per action frame
    Ta: Optional[int] = None
    G: Optional[int] = None
    per_group: Optional[int] = None


def shapes(hidden_states, encoder_hidden_states, num_views, config) -> Shapes:
    c = config
    bb, vf, C, Hh, Ww = hidden_states.shape
    B, T = bb * num_views, vf // num_views                                          # :756-758
    mod_text = bool(c.modulate_encoder_hidden_states)
    Nt = encoder_hidden_states.shape[1] if mod_text else 0
    Tq = T // (c.patch_size_t or 1)
    P = (Hh // c.patch_size) * (Ww // c.patch_size)
    Nv = Tq * P
    S = Nt + Nv
    return Shapes(B=B, b0=bb, nv=num_views, T=T, Hh=Hh, Ww=Ww, C=C, p=c.patch_size, pt=c.patch_size_t, Tq=Tq, P=P, Nv=Nv, Nt=Nt, S=S,
                  M=B * S, D=c.num_attention_heads * c.attention_head_dim, heads=c.num_attention_heads, E=c.time_embed_dim,
                  mod_text=mod_text)


_ACT = {"silu": torch.nn.functional.silu, "gelu_tanh": lambda u: torch.nn.functional.gelu(u, approximate="tanh")}


def mlp2(x, lin1, lin2, act, keep=False):
    """Linear - activation - Linear of the conditioning branch (time, ofs, ActionEmbed, ActionRecon) -> (y, u, h).

    THE one place where the inference and the training arithmetic differ.  Fused (``keep=False``): ``orv_skinny_linear`` applies the
    activation to its fp32 accumulator and rounds once; u and h are None.  Saving (``keep=True``): the backward needs the pre-activation,
    so it is rounded to bf16 (u), activated by torch in fp32 and rounded again (h).  Each path is bounded against the oracle on its own."""
    if not keep:
        return ops.skinny_linear(ops.skinny_linear(x, lin1.weight, lin1.bias, act_out=act), lin2.weight, lin2.bias), None, None
    u = ops.skinny_linear(x, lin1.weight, lin1.bias)
    h = _ACT[act](u.float()).to(BF16)
    return ops.skinny_linear(h, lin2.weight, lin2.bias), u, h


def pad_k(a, w):
    """A [M, K] and W [N, ...] of a GEMM whose K is not a multiple of 64 (only tiny test configs) get zero-padded."""
    w, K = w.reshape(w.shape[0], -1), a.shape[1]
    if K % 64:
        pad = 64 - K % 64
        a, w = torch.nn.functional.pad(a, (0, pad)), torch.nn.functional.pad(w, (0, pad))
    return a.contiguous(), w.contiguous()


def mv_index(b, v, f, Nt, P, S, dev):
    """The token permutation '(b v) (f s) -> (b f) (v s)' (text '(b v) n -> (b f) (v n)') of the multiview blocks as an int32 row index
    into the joint [(b v), S, D] buffer."""
    bi = torch.arange(b, device=dev).view(b, 1, 1, 1)
    fi = torch.arange(f, device=dev).view(1, f, 1, 1)
    vi = torch.arange(v, device=dev).view(1, 1, v, 1)
    txt = ((bi * v + vi) * S + torch.arange(Nt, device=dev).view(1, 1, 1, Nt)).expand(b, f, v, Nt)
    vid = (bi * v + vi) * S + Nt + fi * P + torch.arange(P, device=dev).view(1, 1, 1, P)
    return torch.cat([txt.reshape(b, f, v * Nt), vid.reshape(b, f, v * P)], dim=2).to(torch.int32).contiguous().view(-1)


def mv_layout(b, v, f, Nt, P, S, dev):
    """Row index and sizes of the regrouped buffer: ``Sm`` rows per (clip, frame), ``R`` rows in all, ``s_pad`` = Sm padded to 64."""
    Sm = v * (Nt + P)
    return dict(idx=mv_index(b, v, f, Nt, P, S, dev), Sm=Sm, R=b * f * Sm, s_pad=(Sm + 63) // 64 * 64)


def _actions_saving(model, sh, actions, pad, want_recon, keep):
    """``ActionEmbed`` / ``ActionRecon`` (components.py) through ``mlp2`` in saving mode.  The mask is not cached on the device here."""
    ae, b0, E = model.action_embed, sh.b0, sh.E
    dev = actions.device
    xa = torch.cat([torch.zeros_like(actions[:, :1]), actions], dim=1)
    xa = xa.reshape(b0, (actions.shape[1] + 1) // ae.compress_ratio, -1)
    if ae.patch_size_t > 1:
        xa = xa.reshape(b0, xa.shape[1] // ae.patch_size_t, -1)
    Ta = xa.shape[1]
    keep.ae_in = xa.reshape(b0 * Ta, -1).to(BF16).contiguous()
    emb, keep.ae_u, keep.ae_h = mlp2(keep.ae_in, ae.mlp[0], ae.mlp[3], "gelu_tanh", keep=True)
    emb = emb.view(b0, Ta, E)
    is_mask = ae.forced_mask.to(dev, torch.bool) if ae.forced_mask is not None else torch.rand(b0, device=dev) < 0.1
    if ae.mask:
        emb = torch.where(is_mask[:, None, None], ae.mask_embed.weight[None].to(emb.dtype), emb)
    keep.is_mask = is_mask
    if sh.nv > 1:                                                                    # :815-816
        emb = emb.repeat_interleave(sh.nv, dim=0)
    action_emb, recon = emb.contiguous(), None
    if want_recon:                                                                   # :822-825, components.py:92-104
        ar = model.action_recon
        keep.has_recon, keep.ar_pad = True, pad
        keep.ar_in = action_emb.reshape(sh.B * Ta, E)
        y, keep.ar_u, keep.ar_h = mlp2(keep.ar_in, ar.mlp[0], ar.mlp[2], "gelu_tanh", keep=True)
        y = y.view(sh.B, Ta, -1)
        if ar.compress_ratio > 1:
            y = y.reshape(sh.B, int(Ta * ar.compress_ratio), y.shape[-1] // ar.compress_ratio)
        recon = y[:, 1 + pad:].contiguous()
    return action_emb, is_mask, recon


def embed(model, sh, x, hidden_states, encoder_hidden_states, controls, timestep, ofs=None, image_rotary_emb=None,
          image_rotary_emb_view=None, keep=None):
    """Everything ahead of the blocks: conditioning embeddings, the tokens of the joint buffer ``x`` [M, D] (the caller's), the action
    stage, visual guidance, the modulation tables of every norm and the multiview regrouping.  ``sh`` gains ``Ta, G, per_group``."""
    c = model.config
    dev = hidden_states.device
    saving = keep is not None
    B, T, Hh, Ww, p, pt, P, Nv, Nt, S, D, E, nv = sh.B, sh.T, sh.Hh, sh.Ww, sh.p, sh.pt, sh.P, sh.Nv, sh.Nt, sh.S, sh.D, sh.E, sh.nv
    if nv > 1:                                                                       # :756-758
        hidden_states = hidden_states.reshape(B, T, *hidden_states.shape[2:])
        encoder_hidden_states = encoder_hidden_states.repeat_interleave(nv, dim=0)

    # 1. time (+ofs) embedding  (:762-775)
    tvec = torch.as_tensor(timestep, device=dev).reshape(-1).to(torch.float32)
    if tvec.numel() == 1 and sh.b0 > 1:
        tvec = tvec.expand(sh.b0)
    te, oe = model.time_embedding, model.ofs_embedding
    t_emb = ops.timestep_embedding(tvec.contiguous(), D, c.flip_sin_to_cos, c.freq_shift)
    temb, te_u1, te_h1 = mlp2(t_emb, te.linear_1, te.linear_2, "silu", saving)
    if saving:
        keep.t_emb, keep.te_u1, keep.te_h1, keep.has_ofs = t_emb, te_u1, te_h1, oe is not None
    if oe is not None:
        ovec = torch.as_tensor(ofs, device=dev).reshape(-1).to(torch.float32)
        o_emb = ops.timestep_embedding(ovec.contiguous(), c.ofs_embed_dim, c.flip_sin_to_cos, c.freq_shift)
        o_out, oe_u1, oe_h1 = mlp2(o_emb, oe.linear_1, oe.linear_2, "silu", saving)
        temb = temb + o_out              # [B,E] + [1,E]; tiny glue add in the model dtype as at :775
        if saving:
            keep.o_emb, keep.oe_u1, keep.oe_h1 = o_emb, oe_u1, oe_h1
    if nv > 1:                           # multiviews share the same noise level (:777-779)
        temb = temb.repeat_interleave(nv, dim=0).contiguous()

    # 2. patch embedding straight into the joint [B,S,D] buffer (:788-794)
    pe = model.patch_embed
    tokens = ops.patchify(hidden_states.to(BF16), None, p, pt)
    a2, w2 = pad_k(tokens.view(B * Nv, -1), pe.proj.weight)
    cpos = pos = pe.video_pos_table(T, Hh, Ww, dev)
    pos_mod = Nv
    if nv > 1:
        # :797-800 adds pos_embedding_v[view, spatial] to every frame: folded into the patch-embed epilogue as one table
        # of n_view*Nv rows (row = view*Nv + frame*P + s), built once per shape.
        pos, pos_mod = model._view_pos_table(pos, nv, T, P, dev), nv * Nv
    vmap = ops.rowmap(Nv, S, Nt)
    ops.gemm(a2, w2, pe.proj.bias, x, B * Nv, D, a2.shape[1], epilogue=2 if pos is not None else 0, R=pos, r_mod=pos_mod, ldr=D, cmap=vmap)
    text2d = None
    if sh.mod_text:
        text2d = encoder_hidden_states.to(BF16).reshape(B * Nt, -1).contiguous()
        a2, w2 = pad_k(text2d, pe.text_proj.weight)
        ops.gemm(a2, w2, pe.text_proj.bias, x, B * Nt, D, a2.shape[1], cmap=ops.rowmap(Nt, S, 0))

    # 3. action embedding (:805-825): the modules in the fused mode, their linears through mlp2 in the saving mode
    action_emb = is_mask = recon = None
    actions = controls.get('actions', None)
    if saving:
        keep.temb, keep.tokens, keep.text2d, keep.has_actions, keep.has_recon = temb, tokens, text2d, actions is not None, False
    if actions is not None:
        actions = actions.to(device=dev)
        res = (actions.size(1) + 1) % 4
        pad = 4 - res if res > 0 else 0
        if pad:
            actions = torch.cat([actions.new_zeros((actions.shape[0], pad, actions.shape[2])), actions], dim=1)
        want_recon = model.training and c.recon_action and model.action_recon is not None
        if saving:
            action_emb, is_mask, recon = _actions_saving(model, sh, actions, pad, want_recon, keep)
        else:
            action_emb, is_mask = model.action_embed(actions)
            if nv > 1:                   # multiviews share the same actions (:815-816)
                action_emb = action_emb.repeat_interleave(nv, dim=0)
            action_emb = action_emb.contiguous()
            if want_recon:
                recon = model.action_recon(action_emb)
                if pad > 0:
                    recon = recon[:, pad:]

    # 3b. occupancy-derived visual guidance (:828-858): each control map goes through the SAME patch-embed (+ the frame position table
    #     only, never the view table), initial_combine_linear(hidden.repeat(1,1,K) + cat(controls)) is added to the video rows.  The
    #     reference also runs text_proj for every control map and throws the result away (:833,:842) - not reproduced.
    ctoks, ctrl_tokens, comb = [], [], None
    if c.visual_guidance:
        for key in ('depths', 'labels'):
            cm = controls.get(key, None)
            if cm is None:
                continue
            if nv > 1:
                cm = cm.reshape(cm.shape[0] * nv, cm.shape[1] // nv, *cm.shape[2:])
            tk = ops.patchify(cm.to(device=dev, dtype=BF16), None, p, pt)
            a2c, w2c = pad_k(tk.view(B * Nv, -1), pe.proj.weight)
            ctok = torch.empty(B * Nv, D, dtype=BF16, device=dev)
            ops.gemm(a2c, w2c, pe.proj.bias, ctok, B * Nv, D, a2c.shape[1], epilogue=2 if cpos is not None else 0, R=cpos, r_mod=Nv, ldr=D)
            ctoks.append(ctok)
            ctrl_tokens.append(tk.view(B * Nv, -1))
    if ctoks:
        assert len(ctoks) == model.num_control_keys, \
            f'Mismatched number of controls: {len(ctoks)=} but {model.num_control_keys=}.'
        K2 = model.num_control_keys * D
        comb = torch.empty(B * Nv, K2, dtype=BF16, device=dev)
        for jx, ctok in enumerate(ctoks):
            ops.add_rows(x, vmap, ctok, comb, jx * D, B * Nv, D, ldo=K2)
        icl = model.initial_combine_linear
        ops.gemm(comb, icl.weight, icl.bias, x, B * Nv, D, K2, epilogue=2, R=x, ldr=D, cmap=vmap)

    # 4. modulation tables for every norm, fp32 [B, G, 3D]: group 0 = text rows, 1.. = frames (:117-145)
    Ta = action_emb.shape[1] if action_emb is not None else 1
    if Nv % Ta:
        raise ValueError(f"{Nv} video tokens cannot be split over {Ta} action frames")
    sh.Ta, sh.G, sh.per_group = Ta, 1 + Ta, Nv // Ta if action_emb is not None else 0
    L = c.num_layers
    ptr = model._pointer_tables(dev)
    mod = ops.modulation_tables(temb, action_emb, ptr["w_blk"], ptr["b_blk"], 2 * L, B, Ta, E, 3 * D, sh.mod_text)
    modf = ops.modulation_tables(temb, action_emb, ptr["w_out"], ptr["b_out"], 1, B, Ta, E, 2 * D, False)[0]

    as_f32 = lambda tabs: None if tabs is None else tuple(r.to(device=dev, dtype=torch.float32).contiguous() for r in tabs)
    rope, rope_view, mv = as_f32(image_rotary_emb), None, None
    if c.multiview:                                                                  # :273-348
        if Nv % T:
            raise ValueError(f"{Nv} video tokens cannot be split over {T} frames for the multiview blocks")
        # the fused mode takes the index from the model's per-shape cache (with its workspace buffers), the saving mode builds it
        lay = (mv_layout if saving else model._mv_state)(sh.b0, nv, T, Nt, Nv // T, S, dev)
        wmv, bmv = model._mv_pointer_tables(dev)
        mv = SimpleNamespace(idx=lay["idx"], Sm=lay["Sm"], R=lay["R"], s_pad=lay["s_pad"], n_text=nv * Nt, ws=lay,
                             mod=ops.modulation_tables(temb, None, wmv, bmv, L, B, 1, E, 3 * D, sh.mod_text),      # [L, B, 2, 3D]
                             grp0=ops.groups(S, Nt, 0))
        rope_view = as_f32(image_rotary_emb_view)
    if saving:
        keep.action_emb, keep.ctrl_tokens, keep.comb, keep.mod, keep.modf = action_emb, ctrl_tokens, comb, mod, modf
        keep.rope, keep.rope_view = rope, rope_view
    return SimpleNamespace(temb=temb, action_emb=action_emb, is_action_mask=is_mask, actions_recon=recon, mod=mod, modf=modf,
                           grp=ops.groups(S, Nt, sh.per_group), rope=rope, rope_view=rope_view, vmap=vmap, mv=mv)


def head(model, sh, x, vis, vis2, modf):
    """Everything after the blocks: norm_final -> norm_out -> proj_out (output columns zero-padded to 64) -> unpatchify -> view unfold,
    on the caller's ``vis`` / ``vis2`` [B * Nv, D].  norm_final is row-wise, so the 2B (:916) and 5B (:911-913) branches are the same
    arithmetic on the video rows; they are read in place from the joint buffer.  Returns (output, fo_pad)."""
    c = model.config
    B, Nv, D = sh.B, sh.Nv, sh.D
    gv = ops.groups(Nv, 0, sh.per_group)
    ops.layernorm_modulate(x, vis, model.norm_final.weight, model.norm_final.bias, None, None, 0, 0, gv, B, D, c.norm_eps,
                           xmap=ops.rowmap(Nv, sh.S, sh.Nt))
    no = model.norm_out
    ops.layernorm_modulate(vis, vis2, no.norm.weight, no.norm.bias, modf[..., D:], modf[..., :D], sh.G * 2 * D, 2 * D, gv, B, D, c.norm_eps)
    fo = model.proj_out.weight.shape[0]
    fo_pad = (fo + 63) // 64 * 64
    wo, bo = model.proj_out.weight, model.proj_out.bias
    if fo_pad != fo:                          # CogVideoX1.5 (p_t = 2): 128 -> fits; tiny test configs: zero-padded columns
        wo = torch.nn.functional.pad(wo, (0, 0, 0, fo_pad - fo)).contiguous()
        bo = torch.nn.functional.pad(bo, (0, fo_pad - fo)).contiguous() if bo is not None else None
    out_tok = torch.empty(B * Nv, fo_pad, dtype=BF16, device=x.device)
    ops.gemm(vis2, wo, bo, out_tok, B * Nv, fo_pad, D)
    if fo_pad != fo:
        out_tok = out_tok[:, :fo].contiguous()
    output = ops.unpatchify(out_tok, B, sh.T, fo // (sh.p * sh.p * (sh.pt or 1)), sh.Hh, sh.Ww, sh.p, sh.pt)
    if sh.nv > 1:                                                                    # :941
        output = output.reshape(sh.b0, sh.nv * sh.T, *output.shape[2:])
    return output, fo_pad
