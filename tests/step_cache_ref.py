"""Reference for the first-block step cache, written from the contract, not from the kernels.

* ``probe_ref`` / ``store_ref`` / ``apply_ref``: numpy restatements of the three kernels.  Arrays are float32 holding bf16-representable
  values (``to_np`` of a torch bf16 tensor is exact); ``bf16_rne`` rounds a float32 array to the nearest bf16, ties to even, on its bits.
* ``oracle_states`` / ``oracle_head`` / ``cached_forward_ref``: a skipped forward assembled from the oracle's pieces in fp32:
  ``head(F_B + (X_A - F_A))``.
"""
import numpy as np
import torch

from oracle import dit


# ---- the kernels ----
def bf16_rne(a):
    """float32 array -> float32 array of the nearest bf16 values, ties to even; NaN stays NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).copy()
    out[np.isnan(a)] = np.nan
    return out


def to_np(t):
    return t.detach().float().cpu().numpy()


def video_rows(x, Nt):
    """x float32 [B, S, D] -> its video rows [B, Nv, D]."""
    return x[:, Nt:, :]


def probe_ref(x, e, p, Nt):
    """x [B, S, D] after iteration 0, e / p [B, Nv, D] -> (f, c, sums float64 [B, 2])."""
    f = video_rows(x, Nt).astype(np.float32).copy()
    c = bf16_rne(f - e.astype(np.float32))                                  # one fp32 subtraction, one rounding
    num = np.abs(c - p.astype(np.float32)).astype(np.float64)               # fp32 subtraction, abs, widened
    den = np.abs(p.astype(np.float32)).astype(np.float64)
    B = x.shape[0]
    sums = np.stack([num.reshape(B, -1).sum(axis=1, dtype=np.float64), den.reshape(B, -1).sum(axis=1, dtype=np.float64)], axis=1)
    return f, c, sums


def store_ref(x, f, c, Nt):
    """x [B, S, D] after the last iteration -> (t, p)."""
    return bf16_rne(video_rows(x, Nt).astype(np.float32) - f.astype(np.float32)), c.copy()


def apply_ref(x, t, Nt):
    """-> x with its video rows replaced by bf16(x + t); the text rows are the input's."""
    out = x.astype(np.float32).copy()
    out[:, Nt:, :] = bf16_rne(video_rows(x, Nt).astype(np.float32) + t.astype(np.float32))
    return out


def same_bits(a, b):
    """Equal as float32 bit patterns (both arrays hold bf16-representable values, so this is equality of the bf16 bits)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- a cached forward from the oracle's pieces ----
def oracle_states(w, cfg, ins, extra, hidden_states=None, timestep=None):
    """The oracle forward of a ``fwd_*`` golden (optionally on other latents / timesteps) -> (sample, inter, temb): ``inter`` holds
    ``block{i}`` = [text | video] rows after iteration i and ``action_emb``; ``temb`` is what the head's AdaLayerNorm takes."""
    cfgf = {**dit.DEFAULT_CONFIG, **cfg}
    hs = ins["hidden_states"] if hidden_states is None else hidden_states
    ts = ins["timestep"] if timestep is None else timestep
    nv = extra["num_views"]
    out, _, _, inter = dit.dit_forward(w, cfg, hs, ins["encoder_hidden_states"], ts, actions=ins.get("actions"),
                                       is_mask=torch.tensor(extra["mask"]) if "actions" in ins else None, num_views=nv,
                                       return_intermediates=True)
    temb = dit.time_embedding(w, cfgf, ts, hs.dtype)
    assert not cfgf["ofs_embed_dim"], "the goldens used here carry no ofs embedding"
    if nv > 1:
        temb = temb.repeat_interleave(nv, dim=0)
    return out, inter, temb


def oracle_head(w, cfg, vis, temb, action_emb, hidden_shape, num_views):
    """norm_final -> norm_out -> proj_out -> unpatchify -> view unfold on video rows ``vis`` [B, Nv, D] (the 2B branch)."""
    cfgf = {**dit.DEFAULT_CONFIG, **cfg}
    bb, vf, _, h, wd = hidden_shape
    b, t = bb * num_views, vf // num_views
    v = dit._ln(w, "norm_final", vis, cfgf["norm_eps"])
    v = dit.ada_layernorm_out(w, cfgf, v, temb, action_emb)
    v = dit._lin(w, "proj_out", v)
    out = dit.unpatchify(v, b, t, h, wd, cfgf["patch_size"], cfgf["patch_size_t"])
    if num_views > 1:
        out = out.reshape(bb, num_views * out.shape[1], *out.shape[2:])
    return out


def cached_forward_ref(w, cfg, ins, extra, hidden_b, timestep_b):
    """Call A = the golden's inputs (computed), call B = (hidden_b, timestep_b) skipped -> (head(F_B + (X_A - F_A)), uncached B)."""
    L = {**dit.DEFAULT_CONFIG, **cfg}["num_layers"]
    nt = ins["encoder_hidden_states"].shape[1]
    _, ia, _ = oracle_states(w, cfg, ins, extra)
    out_b, ib, temb_b = oracle_states(w, cfg, ins, extra, hidden_b, timestep_b)
    fa, xa, fb = ia["block0"][:, nt:], ia[f"block{L - 1}"][:, nt:], ib["block0"][:, nt:]
    # the head is the oracle's own: on B's uncached last state it must give B's uncached output
    chk = oracle_head(w, cfg, ib[f"block{L - 1}"][:, nt:], temb_b, ib.get("action_emb"), hidden_b.shape, extra["num_views"])
    assert torch.allclose(chk, out_b, atol=1e-5, rtol=1e-5), "oracle_head drifted from dit_forward's tail"
    return oracle_head(w, cfg, fb + (xa - fa), temb_b, ib.get("action_emb"), hidden_b.shape, extra["num_views"]), out_b
