"""``stages.embed`` in its two modes (``keep=None``: the no-grad launches; ``keep`` object: what ``training.backward`` reads) on the tiny goldens.

The token stage does not depend on the conditioning branch, so the filled token buffers of the two modes must be bit-identical; the
modulation tables differ by the documented rounding of ``stages.mlp2`` (each path is bounded against the oracle elsewhere) and are compared
by shape only."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_golden  # noqa: E402

BF = torch.bfloat16
ALWAYS = ["t_emb", "te_u1", "te_h1", "has_ofs", "temb", "tokens", "text2d", "has_actions", "has_recon", "action_emb", "ctrl_tokens", "comb",
          "mod", "modf", "rope", "rope_view"]
OFS, ACTIONS, RECON = ["o_emb", "oe_u1", "oe_h1"], ["ae_in", "ae_u", "ae_h", "is_mask"], ["ar_pad", "ar_in", "ar_u", "ar_h"]


def fields(s):
    return tuple(getattr(s, f) for f, _ in s._fields_)


@pytest.mark.parametrize("name", ["fwd_cond", "fwd_pt2_ofs", "fwd_multiview", "fwd_train_recon"])
def test_embed_modes_fill_the_same_tokens_and_keep_what_backward_reads(name):
    from orv_amd import stages
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    dev = torch.device("cuda:0")
    cfg, extra, ins, w, outs = load_golden(name)
    m = CogVideoXTransformer3DModelTraj(**cfg)
    m.load_state_dict(w, strict=True)
    m = m.to(dev, BF).train(extra["training"])
    ctrl = {}
    if "actions" in ins:
        ctrl["actions"] = ins["actions"].to(dev)
        m.action_embed.forced_mask = torch.tensor(extra["mask"])
    for key in ("depths", "labels"):
        if key in ins:
            ctrl[key] = ins[key].to(dev, BF)
    rope = (ins["rope_cos"].to(dev), ins["rope_sin"].to(dev)) if "rope_cos" in ins else None
    ofs = None if extra["ofs"] is None else torch.full((1,), float(extra["ofs"]), device=dev)
    hs, eh, ts = ins["hidden_states"].to(dev, BF), ins["encoder_hidden_states"].to(dev, BF), ins["timestep"].to(dev)

    def run(keep):
        sh = stages.shapes(hs, eh, extra["num_views"], m.config)
        x = torch.empty(sh.M, sh.D, dtype=BF, device=dev)
        with torch.no_grad():
            return sh, x, stages.embed(m, sh, x, hs, eh, ctrl, ts, ofs, rope, keep=keep)

    run(None)                                   # builds the per-shape caches (position and pointer tables, multiview workspace)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    sh0, x0, st0 = run(None)
    assert sorted(vars(st0)) == sorted(["temb", "action_emb", "is_action_mask", "actions_recon", "mod", "modf", "grp", "rope", "rope_view",
                                        "vmap", "mv"])
    mask0, shapes0 = st0.is_action_mask, (st0.mod.shape, st0.modf.shape, None if st0.mv is None else st0.mv.mod.shape)
    grp0, mv0 = fields(st0.grp), None if st0.mv is None else (st0.mv.idx, st0.mv.Sm, st0.mv.R, st0.mv.s_pad)
    with_record = torch.cuda.memory_allocated()
    del st0
    # nothing outlives the record the fused mode returns: no saved activations, no new cache entries - what is left is the caller's token
    # buffer (the allocator hands out multiples of 512 bytes) and at most the mask
    assert torch.cuda.memory_allocated() - held <= -(-x0.numel() * 2 // 512) * 512 + 512
    assert torch.cuda.memory_allocated() < with_record

    keep = SimpleNamespace()
    sh1, x1, st1 = run(keep)
    assert torch.equal(x1, x0)
    assert sh1 == sh0 and None not in (sh1.Ta, sh1.G, sh1.per_group)
    assert (mask0 is None) == (st1.is_action_mask is None) and (mask0 is None or torch.equal(st1.is_action_mask, mask0))
    assert fields(st1.grp) == grp0
    assert (st1.mod.shape, st1.modf.shape, None if st1.mv is None else st1.mv.mod.shape) == shapes0
    assert (st1.mv is None) == (mv0 is None) == (not cfg.get("multiview", False))
    if mv0 is not None:
        assert torch.equal(st1.mv.idx, mv0[0]) and (st1.mv.Sm, st1.mv.R, st1.mv.s_pad) == mv0[1:]

    want = ALWAYS + (OFS if keep.has_ofs else []) + (ACTIONS if keep.has_actions else []) + (RECON if keep.has_recon else [])
    assert sorted(vars(keep)) == sorted(want)
    assert keep.has_ofs == (extra["ofs"] is not None) and keep.has_actions == ("actions" in ins)
    assert keep.has_recon == bool(extra["training"] and cfg.get("recon_action", False) and "actions" in ins)
    assert (keep.text2d is not None) == sh1.mod_text and len(keep.ctrl_tokens) == sum(k in ins for k in ("depths", "labels"))
    assert (keep.comb is not None) == bool(keep.ctrl_tokens) and keep.mod is st1.mod and keep.modf is st1.modf
    tensors = [getattr(keep, k) for k in want if k.endswith(("_u", "_u1", "_h", "_h1", "_in", "_emb")) or k in ("tokens", "temb")]
    assert all(t is None or (torch.is_tensor(t) and t.is_cuda) for t in tensors) and keep.tokens is not None and keep.te_u1 is not None
