"""MI355X-native mirror of ``orv.models.cogvideox_control`` (/root/reference/orv/models/cogvideox_control.py).

Same class names, constructor kwargs, ``forward`` / ``__call__`` signatures, ``.config`` attribute access and
``state_dict`` keys as the reference, with no diffusers dependency.  The ``nn.Module`` tree below is a
*parameter container*: every ``nn.Linear`` / ``nn.LayerNorm`` / ``nn.Conv2d`` exists so checkpoints load under the
reference's key names; none of their torch ``forward`` methods is ever called.  All arithmetic of the transformer
forward (reference lines :715-948) runs in the hand-written HIP kernels of liborv_mi355.so through ``orv_amd.ops``:

    time/ofs embedding   orv_timestep_embedding + orv_skinny_linear            (:762-775)
    patch embed          orv_patchify + orv_gemm_bf16 (pos-embed add fused)    (:788)
    action embedding     orv_skinny_linear x2                                  (:805-820, components.py:47-71)
    AdaLN tables         orv_skinny_linear (SiLU + split-linear trick fused)   (:117-130, :172)
    per block            orv_layernorm_modulate -> orv_gemm_bf16(QKV + qk LayerNorm epilogue) -> orv_attention_fwd
                         -> orv_gemm_bf16(out-proj, gated residual) -> orv_layernorm_modulate
                         -> orv_gemm_bf16(FFN1, GELU) -> orv_gemm_bf16(FFN2, gated residual)   (:394-445)
    head                 orv_layernorm_modulate x2 -> orv_gemm_bf16 -> orv_unpatchify          (:909-936)

The text and video streams live in ONE joint activation buffer [B, S = n_text + n_video, D] (text rows first, the order
of the reference's torch.cat at :222,:437), so no concat/split copies exist; per-frame modulation and gates are looked
up by token group inside the kernels instead of materialising ``repeat_interleave`` ([B, 3000, 1920] x 3 per norm).

There is no CPU / eager fallback: tensors must live on an MI355X and the model must be bf16.
"""
from __future__ import annotations

import fnmatch
import json
import math
import os
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import torch
from torch import nn

from . import _state, lora as _lora, ops, stages, training as _training
from .components import ActionEmbed, ActionRecon, Transformer3DModelTrajOutput
from .embeddings import sincos_3d
from .schedulers import CogVideoXDDIMScheduler, CogVideoXDPMScheduler, retrieve_timesteps

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634


class FrozenConfig(dict):
    """Attribute + mapping access, like diffusers' FrozenDict (``model.config.patch_size`` / ``dict(model.config)``)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


# ------------------------------------------------------------------------------------------------------------------
# parameter containers (names == reference / diffusers attribute names == checkpoint keys)
# ------------------------------------------------------------------------------------------------------------------
class _NoForward(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(f"{type(self).__name__} is a parameter container; the arithmetic runs in liborv_mi355.so")


class CogVideoXLayerNormZero(_NoForward):
    """:41-58. ``linear`` is [6D, E] when text is modulated too, else [3D, E]."""

    def __init__(self, conditioning_dim: int, embedding_dim: int, elementwise_affine: bool = True, eps: float = 1e-5,
                 bias: bool = True, modulate_encoder_hidden_states: Optional[bool] = False) -> None:
        super().__init__()
        self.modulate_encoder_hidden_states = modulate_encoder_hidden_states
        self.silu = nn.SiLU()
        self.linear = nn.Linear(conditioning_dim, (6 if modulate_encoder_hidden_states else 3) * embedding_dim, bias=bias)
        self.norm = nn.LayerNorm(embedding_dim, eps=eps, elementwise_affine=elementwise_affine)


class AdaLayerNorm(_NoForward):
    """:153-197 as built at :572-578 (chunk_dim=1; linear output order is (shift, scale))."""

    def __init__(self, embedding_dim: int, output_dim: int, norm_elementwise_affine: bool = False,
                 norm_eps: float = 1e-5, chunk_dim: int = 0):
        super().__init__()
        self.chunk_dim, self.emb = chunk_dim, None
        self.silu = nn.SiLU()
        self.linear = nn.Linear(embedding_dim, output_dim)
        self.norm = nn.LayerNorm(output_dim // 2, norm_eps, norm_elementwise_affine)


class Attention(_NoForward):
    """diffusers ``Attention`` as configured at :382-391 (self-attention, bias, qk LayerNorm eps 1e-6)."""

    def __init__(self, query_dim: int, heads: int, dim_head: int, bias: bool, out_bias: bool, qk_norm: bool = True,
                 eps: float = 1e-6):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.dim_head, self.eps = heads, dim_head, eps
        self.to_q = nn.Linear(query_dim, inner, bias=bias)
        self.to_k = nn.Linear(query_dim, inner, bias=bias)
        self.to_v = nn.Linear(query_dim, inner, bias=bias)
        self.norm_q = nn.LayerNorm(dim_head, eps=eps) if qk_norm else None
        self.norm_k = nn.LayerNorm(dim_head, eps=eps) if qk_norm else None
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim, bias=out_bias), nn.Dropout(0.0)])
        self._packed = None
        self._bound = None

    def score_bound(self, scale: float, rope: bool = True):
        """Guaranteed upper bound of |q' . k'| in log2 units, q' = norm_q(q) * scale * log2 e and k' = norm_k(k) as the
        projection epilogue / ``orv_qkv_prep`` produce them.  A LayerNorm output over 64 channels is gamma * xhat + beta with
        ||xhat||_2 <= 8, so (round 6, per channel instead of the product of per-vector maxima - VERDICT r5 weak #2)

            |q' . k'| <= 64 max_c |gamma_q,c gamma_k,c| + 8 ||gamma_q * beta_k|| + 8 ||gamma_k * beta_q|| + |beta_q . beta_k|

        ``rope=True`` (the safe default): RoPE rotates each channel PAIR of q and of k by its own angle, which mixes the two channels of
        a pair - the same four terms with per-pair quantities (max |gamma| of the pair, ||beta|| of the pair; the last term becomes
        sum_p ||beta_q,p|| ||beta_k,p||), valid for any rotation including none.  2 % margin for the bf16 rounding of q' and k'.
        Feeds the fixed-shift softmax of ``orv_attention_fwd_bounded``; cached per weight version (one host read per model)."""
        if self.norm_q is None or self.norm_k is None:
            return None
        key = self._bound_key(scale, rope)
        if self._bound is None or self._bound[0] != key:
            prime_score_bounds([self], scale, rope=rope)
        return self._bound[1]

    def score_bound_dev(self, scale: float, rope: bool = True):
        """``score_bound`` as a one-element fp32 DEVICE tensor (``prime_score_bounds(..., on_device=True)``): the training
        forward hands it to ``orv_attention_fwd_bounded_dev`` - the bound changes with every optimizer step and must not cost a
        blocking device -> host read per step."""
        if self.norm_q is None or self.norm_k is None:
            return None
        key = self._bound_key(scale, rope)
        bd = getattr(self, "_bound_dev", None)
        if bd is None or bd[0] != key:
            prime_score_bounds([self], scale, on_device=True, rope=rope)
        return self._bound_dev[1]

    def _bound_key(self, scale, rope=True):
        ps = (self.norm_q.weight, self.norm_q.bias, self.norm_k.weight, self.norm_k.bias)
        return tuple((w.data_ptr(), w._version) for w in ps) + (_state.weights_epoch[0], float(scale), bool(rope))

    def packed_qkv(self):
        """[3*inner, query_dim] weight and [3*inner] bias for the single fused QKV GEMM (cached per weight version)."""
        ws = (self.to_q.weight, self.to_k.weight, self.to_v.weight)
        key = tuple((w.data_ptr(), w._version) for w in ws) + (_state.weights_epoch[0],)
        if self._packed is None or self._packed[0] != key:
            w = torch.cat([x.detach() for x in ws], dim=0).contiguous()
            b = None
            if self.to_q.bias is not None:
                b = torch.cat([self.to_q.bias.detach(), self.to_k.bias.detach(), self.to_v.bias.detach()]).contiguous()
            self._packed = (key, w, b)
        return self._packed[1], self._packed[2]


def score_bound_terms(gq, bq, gk, bk, rope: bool = True):
    """The bound of ``Attention.score_bound`` before the scale, for stacks ``[n, 64]`` of qk-LayerNorm parameters (fp32) -> ``[n]``."""
    if rope:
        pair = lambda t: t.reshape(t.shape[0], -1, 2)
        gq, gk = pair(gq.abs()).amax(-1), pair(gk.abs()).amax(-1)
        bq, bk = pair(bq).norm(dim=-1), pair(bk).norm(dim=-1)
        const = (bq * bk).sum(dim=1)
    else:
        const = (bq * bk).sum(dim=1).abs()
    rt = 8.0                             # ||xhat||_2 <= sqrt(64)
    return rt * rt * (gq * gk).abs().amax(dim=1) + rt * (gq * bk).norm(dim=1) + rt * (gk * bq).norm(dim=1) + const


def prime_score_bounds(attns, scale: float, on_device: bool = False, rope: bool = True) -> None:
    """``Attention.score_bound`` for many modules with ONE device -> host copy (a model has 30-84 of them): stale entries are
    recomputed together on the device and read back once.  ``on_device=True`` (training, where the bound changes with every
    optimizer step): NO host copy at all - every module gets a one-element view of the device vector (``score_bound_dev``)."""
    if on_device:
        todo = [a for a in attns if a.norm_q is not None and a.norm_k is not None
                and (getattr(a, "_bound_dev", None) is None or a._bound_dev[0] != a._bound_key(scale, rope))]
    else:
        todo = [a for a in attns if a.norm_q is not None and a.norm_k is not None and (a._bound is None or a._bound[0] != a._bound_key(scale, rope))]
    if not todo:
        return
    if todo[0].dim_head != 64:
        raise ValueError("score bound: the attention kernels are built for 64 channels per head")
    with torch.no_grad():
        gq = torch.stack([a.norm_q.weight.detach().float() for a in todo])
        bq = torch.stack([a.norm_q.bias.detach().float() for a in todo])
        gk = torch.stack([a.norm_k.weight.detach().float() for a in todo])
        bk = torch.stack([a.norm_k.bias.detach().float() for a in todo])
        vals = (1.02 * float(scale) * LOG2E * score_bound_terms(gq, bq, gk, bk, rope)).contiguous()
        if on_device:
            for i, a in enumerate(todo):
                a._bound_dev = (a._bound_key(scale, rope), vals[i:i + 1])
            return
        vals = vals.tolist()
    for a, v in zip(todo, vals):
        a._bound = (a._bound_key(scale, rope), float(v))


class _GELUProj(_NoForward):
    def __init__(self, dim_in, dim_out, bias=True):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out, bias=bias)


class FeedForward(_NoForward):
    """diffusers ``FeedForward(dim, activation_fn='gelu-approximate', final_dropout=True)``: keys net.0.proj / net.2."""

    def __init__(self, dim: int, dropout: float = 0.0, activation_fn: str = "gelu-approximate", inner_dim=None,
                 bias: bool = True):
        super().__init__()
        if activation_fn != "gelu-approximate":
            raise NotImplementedError(f"activation_fn={activation_fn}: the fused GEMM epilogue implements GELU(tanh)")
        inner_dim = inner_dim or 4 * dim
        self.net = nn.ModuleList([_GELUProj(dim, inner_dim, bias), nn.Dropout(dropout),
                                  nn.Linear(inner_dim, dim, bias=bias), nn.Dropout(dropout)])


class CogVideoXBlock(_NoForward):
    """:351-445."""

    def __init__(self, dim: int, num_attention_heads: int, attention_head_dim: int, time_embed_dim: int,
                 dropout: float = 0.0, activation_fn: str = "gelu-approximate", attention_bias: bool = False,
                 qk_norm: bool = True, norm_elementwise_affine: bool = True, norm_eps: float = 1e-5,
                 attention_out_bias: bool = True, modulate_encoder_hidden_states: Optional[bool] = False, **kwargs):
        super().__init__()
        mk = dict(modulate_encoder_hidden_states=modulate_encoder_hidden_states)
        self.norm1 = CogVideoXLayerNormZero(time_embed_dim, dim, norm_elementwise_affine, norm_eps, bias=True, **mk)
        self.attn1 = Attention(dim, num_attention_heads, attention_head_dim, attention_bias, attention_out_bias, qk_norm)
        self.norm2 = CogVideoXLayerNormZero(time_embed_dim, dim, norm_elementwise_affine, norm_eps, bias=True, **mk)
        self.ff = FeedForward(dim, dropout=dropout, activation_fn=activation_fn)
        self.modulate_encoder_hidden_states = modulate_encoder_hidden_states


class MVBlock(_NoForward):
    """:273-348 (multiview cross-view attention).  Parameter container; the arithmetic is
    ``CogVideoXTransformer3DModelTraj._mv_block`` (gather -> QKV GEMM -> attention -> out/proj GEMMs -> gated scatter)."""

    def __init__(self, dim, num_attention_heads, attention_head_dim, time_embed_dim, attention_bias=False, qk_norm=True,
                 norm_elementwise_affine=True, norm_eps=1e-5, attention_out_bias=True,
                 modulate_encoder_hidden_states=False):
        super().__init__()
        self.norm1 = CogVideoXLayerNormZero(time_embed_dim, dim, norm_elementwise_affine, norm_eps, bias=True,
                                            modulate_encoder_hidden_states=modulate_encoder_hidden_states)
        self.attn1 = Attention(dim, num_attention_heads, attention_head_dim, attention_bias, attention_out_bias, qk_norm)
        self.cam_encoder = nn.Linear(12, dim)
        self.proj_out = nn.Linear(dim, dim)
        for p in (*self.cam_encoder.parameters(), *self.proj_out.parameters()):
            p.data.zero_()


class CogVideoXPatchEmbed(_NoForward):
    """diffusers ``CogVideoXPatchEmbed`` as built at :531-547: ``proj`` (Conv2d k=s=p, or Linear for patch_size_t),
    ``text_proj`` and the non-persistent sin-cos table."""

    def __init__(self, patch_size=2, patch_size_t=None, in_channels=16, embed_dim=1920, text_embed_dim=4096, bias=True,
                 sample_width=90, sample_height=60, sample_frames=49, temporal_compression_ratio=4,
                 max_text_seq_length=226, spatial_interpolation_scale=1.875, temporal_interpolation_scale=1.0,
                 use_positional_embeddings=True, use_learned_positional_embeddings=True):
        super().__init__()
        self.patch_size, self.patch_size_t, self.embed_dim = patch_size, patch_size_t, embed_dim
        self.sample_height, self.sample_width, self.sample_frames = sample_height, sample_width, sample_frames
        self.temporal_compression_ratio, self.max_text_seq_length = temporal_compression_ratio, max_text_seq_length
        self.spatial_interpolation_scale = spatial_interpolation_scale
        self.temporal_interpolation_scale = temporal_interpolation_scale
        self.use_positional_embeddings = use_positional_embeddings
        self.use_learned_positional_embeddings = use_learned_positional_embeddings
        if patch_size_t is None:
            self.proj = nn.Conv2d(in_channels, embed_dim, kernel_size=(patch_size, patch_size), stride=patch_size, bias=bias)
        else:
            self.proj = nn.Linear(in_channels * patch_size * patch_size * patch_size_t, embed_dim)
        self.text_proj = nn.Linear(text_embed_dim, embed_dim)
        if use_positional_embeddings or use_learned_positional_embeddings:
            self.register_buffer("pos_embedding", self._joint_table(sample_height, sample_width, sample_frames),
                                 persistent=use_learned_positional_embeddings)
        self._video_tables: Dict[Any, torch.Tensor] = {}

    def _video_table(self, height, width, pre_frames) -> torch.Tensor:
        p = self.patch_size
        frames = (pre_frames - 1) // self.temporal_compression_ratio + 1
        return sincos_3d(self.embed_dim, width // p, height // p, frames, self.spatial_interpolation_scale,
                         self.temporal_interpolation_scale)

    def _joint_table(self, height, width, pre_frames) -> torch.Tensor:
        vid = self._video_table(height, width, pre_frames)
        joint = torch.zeros(1, self.max_text_seq_length + vid.shape[0], self.embed_dim, dtype=torch.float32)
        joint[0, self.max_text_seq_length:] = vid
        return joint

    def video_pos_table(self, latent_frames, height, width, device) -> Optional[torch.Tensor]:
        """bf16 [T*h*w, D] rows of the table that patch-embed adds to the video tokens (None for RoPE models)."""
        if not (self.use_positional_embeddings or self.use_learned_positional_embeddings):
            return None
        pre = (latent_frames - 1) * self.temporal_compression_ratio + 1
        key = (latent_frames, height, width, str(device))
        if key not in self._video_tables:
            if (height, width, pre) == (self.sample_height, self.sample_width, self.sample_frames):
                tab = self.pos_embedding[0, self.max_text_seq_length:]
            else:
                if self.use_learned_positional_embeddings:
                    raise ValueError("learned positional embeddings need the trained sample size")
                tab = self._video_table(height, width, pre)
            self._video_tables[key] = tab.to(device=device, dtype=BF16).contiguous()
        return self._video_tables[key]


class TimestepEmbedding(_NoForward):
    def __init__(self, in_channels, time_embed_dim, act_fn="silu"):
        super().__init__()
        if act_fn != "silu":
            raise NotImplementedError("timestep_activation_fn must be 'silu'")
        self.linear_1 = nn.Linear(in_channels, time_embed_dim)
        self.act = nn.SiLU()
        self.linear_2 = nn.Linear(time_embed_dim, time_embed_dim)


_CONFIG_DEFAULTS = dict(
    num_attention_heads=30, attention_head_dim=64, in_channels=16, out_channels=16, flip_sin_to_cos=True, freq_shift=0,
    time_embed_dim=512, ofs_embed_dim=None, text_embed_dim=4096, num_layers=30, dropout=0.0, attention_bias=True,
    sample_width=90, sample_height=60, sample_frames=49, patch_size=2, patch_size_t=None, temporal_compression_ratio=4,
    max_text_seq_length=226, activation_fn="gelu-approximate", timestep_activation_fn="silu",
    norm_elementwise_affine=True, norm_eps=1e-5, spatial_interpolation_scale=1.875, temporal_interpolation_scale=1.0,
    use_rotary_positional_embeddings=False, use_learned_positional_embeddings=False, patch_bias=True,
    loaded_pretrained_model_name_or_path=None, modulate_encoder_hidden_states=False, num_control_blocks=12,
    recon_action=False, visual_guidance=False, num_control_keys=2, multiview=False, max_n_view=3, from_t2v=False)


class CogVideoXTransformer3DModelTraj(nn.Module, _lora.LoraMixin):
    """Trajectory/occupancy-conditioned CogVideoX 3-D DiT (:448-1087)."""

    config_name = "config.json"

    # the reference's registered signature (:452-494): same names, order and defaults, positional use included
    def __init__(self, num_attention_heads: int = 30, attention_head_dim: int = 64, in_channels: int = 16,
                 out_channels: Optional[int] = 16, flip_sin_to_cos: bool = True, freq_shift: int = 0, time_embed_dim: int = 512,
                 ofs_embed_dim: Optional[int] = None, text_embed_dim: int = 4096, num_layers: int = 30, dropout: float = 0.0,
                 attention_bias: bool = True, sample_width: int = 90, sample_height: int = 60, sample_frames: int = 49,
                 patch_size: int = 2, patch_size_t: Optional[int] = None, temporal_compression_ratio: int = 4,
                 max_text_seq_length: int = 226, activation_fn: str = "gelu-approximate", timestep_activation_fn: str = "silu",
                 norm_elementwise_affine: bool = True, norm_eps: float = 1e-5, spatial_interpolation_scale: float = 1.875,
                 temporal_interpolation_scale: float = 1.0, use_rotary_positional_embeddings: bool = False,
                 use_learned_positional_embeddings: bool = False, patch_bias: bool = True,
                 loaded_pretrained_model_name_or_path: Optional[str] = None, modulate_encoder_hidden_states: bool = False,
                 num_control_blocks: int = 12, recon_action: bool = False, visual_guidance: bool = False,
                 num_control_keys: int = 2, multiview: bool = False, max_n_view: int = 3, from_t2v: bool = False, **kwargs):
        given = {k: v for k, v in locals().items() if k in _CONFIG_DEFAULTS}
        super().__init__()
        unknown = {k: v for k, v in kwargs.items() if not k.startswith("_")}
        cfg = {**_CONFIG_DEFAULTS, **given}
        self._extra_config = unknown
        self.config = FrozenConfig(cfg)
        c = self.config
        inner = c.num_attention_heads * c.attention_head_dim
        if c.attention_head_dim != 64:
            raise NotImplementedError("the attention kernels are built for head_dim 64 (every CogVideoX/ORV config)")
        self.inner_dim = inner
        self.patch_embed = CogVideoXPatchEmbed(
            patch_size=c.patch_size, patch_size_t=c.patch_size_t, in_channels=c.in_channels, embed_dim=inner,
            text_embed_dim=c.text_embed_dim, bias=c.patch_bias, sample_width=c.sample_width,
            sample_height=c.sample_height, sample_frames=c.sample_frames,
            temporal_compression_ratio=c.temporal_compression_ratio, max_text_seq_length=c.max_text_seq_length,
            spatial_interpolation_scale=c.spatial_interpolation_scale,
            temporal_interpolation_scale=c.temporal_interpolation_scale,
            use_positional_embeddings=not c.use_rotary_positional_embeddings,
            use_learned_positional_embeddings=c.use_learned_positional_embeddings)
        self.embedding_dropout = nn.Dropout(c.dropout)
        self.time_embedding = TimestepEmbedding(inner, c.time_embed_dim, c.timestep_activation_fn)
        self.ofs_embedding = None
        if c.ofs_embed_dim:
            if c.ofs_embed_dim != c.time_embed_dim:
                raise ValueError("ofs_embed_dim must equal time_embed_dim (the embeddings are summed, :775)")
            self.ofs_embedding = TimestepEmbedding(c.ofs_embed_dim, c.ofs_embed_dim, c.timestep_activation_fn)
        if fnmatch.fnmatch(str(c.loaded_pretrained_model_name_or_path), 'THUDM*CogVideoX*'):
            if not c.modulate_encoder_hidden_states:
                raise RuntimeError(f"You're trying to load {c.loaded_pretrained_model_name_or_path} but"
                                   "set modulate_encoder_hidden_states to False!")
        blk = dict(dim=inner, num_attention_heads=c.num_attention_heads, attention_head_dim=c.attention_head_dim,
                   time_embed_dim=c.time_embed_dim, attention_bias=c.attention_bias,
                   norm_elementwise_affine=c.norm_elementwise_affine, norm_eps=c.norm_eps,
                   modulate_encoder_hidden_states=c.modulate_encoder_hidden_states)
        self.transformer_blocks = nn.ModuleList(
            [CogVideoXBlock(dropout=c.dropout, activation_fn=c.activation_fn, **blk) for _ in range(c.num_layers)])
        self.norm_final = nn.LayerNorm(inner, c.norm_eps, c.norm_elementwise_affine)
        self.norm_out = AdaLayerNorm(embedding_dim=c.time_embed_dim, output_dim=2 * inner,
                                     norm_elementwise_affine=c.norm_elementwise_affine, norm_eps=c.norm_eps, chunk_dim=1)
        self.proj_out = nn.Linear(inner, c.patch_size * c.patch_size * (c.patch_size_t or 1) * c.out_channels)
        # NB the reference passes mask=self.training inside __init__, i.e. always True (:581-582)
        self.action_embed = ActionEmbed(state_dim=7, hidden_size=c.time_embed_dim, compress_ratio=4,
                                        patch_size_t=c.patch_size_t, mask=True)
        self.action_recon = ActionRecon(7, c.time_embed_dim, 4) if c.recon_action else None
        if c.visual_guidance:
            if c.num_control_blocks > c.num_layers:
                raise ValueError("num_tracking_blocks must be less than or equal to num_layers")
            self.num_control_keys = c.num_control_keys
            self.initial_combine_linear = nn.Linear(inner * c.num_control_keys, inner)
        if c.multiview:
            self.register_buffer("pos_embedding_v", sincos_3d(
                inner, c.sample_width // c.patch_size, c.sample_height // c.patch_size, c.max_n_view,
                c.spatial_interpolation_scale, 1.0)[None], persistent=False)
            self.mv_blocks = nn.ModuleList([MVBlock(**blk) for _ in range(c.num_layers)])
        self.gradient_checkpointing = False
        self._ws: Dict[Any, Dict[str, torch.Tensor]] = {}
        self._mxfp8 = False         # MXFP8 inference mode of the block GEMMs (enable_mxfp8)
        self._mx_gen = 0            # bumped by every enable_mxfp8 call: part of GraphedTransformer's key
        self._step_cache = None     # first-block step cache (enable_step_cache); None: off
        self._sc_gen = 0            # bumped by every enable_step_cache call: part of GraphedTransformer's key
        self._mx_cache = None       # per block: (weight key, quantised QKV / out / FFN1 / FFN2 weights)
        self._lora_init()           # LoRA adapters of the attention projections (orv_amd/lora.py)
        self._set_zeros()
        self._set_trainable_parameters()

    # ---- reference housekeeping (:625-656) ----
    def _set_zeros(self):
        if self.config.from_t2v:
            self.patch_embed.proj.weight.data[:, -16:, ...].zero_()
        if hasattr(self, 'initial_combine_linear'):
            self.initial_combine_linear.weight.data.zero_()
            self.initial_combine_linear.bias.data.zero_()

    def _set_trainable_parameters(self):
        # Data-parallel bookkeeping hint (orv_amd.optim.FusedAdamW): the six big weights of a block are the gradients that are FINAL when the
        # hand-written backward leaves the block (training.backward's grad_hook) - biases / LayerNorm affines are converted at the very end,
        # the AdaLN linears close with the modulation tables.  Tagged, they are laid out first and contiguously in the optimizer's flat
        # gradient buffer, so a block's early gradients leave as ONE 88-MB all-reduce during the backward (xGMI rings are per-link bound:
        # few, large messages) instead of two early + two late pieces.
        for blk in self.transformer_blocks:
            for lin in (blk.attn1.to_q, blk.attn1.to_k, blk.attn1.to_v, blk.attn1.to_out[0], blk.ff.net[0].proj, blk.ff.net[2]):
                lin.weight._orv_grad_early = True
        if self.config.multiview:
            for p in self.parameters():
                p.requires_grad_(False)
            for p in self.mv_blocks.parameters():
                p.requires_grad_(True)
        else:
            for p in self.parameters():
                p.requires_grad_(True)

    def enable_gradient_checkpointing(self):
        """Block-level activation recompute, as the reference's ``torch.utils.checkpoint`` per block (:867-899): the training
        forward keeps only every block's input and the backward rebuilds a block's activations right before using them
        (orv_amd/training.py ``run_block`` / ``sv.recompute``).  Gradients are bit-identical to the run that keeps everything;
        peak memory drops by ~0.9 GB per block at B = 4, the step gains one forward."""
        self.gradient_checkpointing = True

    def disable_gradient_checkpointing(self):
        self.gradient_checkpointing = False

    # ---- MXFP8 inference mode ----
    def enable_mxfp8(self, enabled: bool = True):
        """Opt-in MXFP8 inference: the four GEMMs of every transformer block (QKV, out-projection, FFN1, FFN2; :232-234, 263, 439-440) run
        on the block-scaled MFMA with MXFP8 activations and weights (include/orv_mi355.h "MXFP8").  The embeddings, modulation tables,
        attention, qk LayerNorm, the head (norm_final / norm_out / proj_out) and the multiview blocks stay bf16.  The weights are quantised
        here (on the first forward when the model is not yet a bf16 model on the GPU) and again whenever a block weight changes (in-place
        edits, moves, replaced Parameters).  Inference only: a forward in training mode or with gradients raises RuntimeError.
        ``enable_mxfp8(False)`` returns to the bf16 path bit for bit and frees the quantised weights.  Returns ``self``."""
        if enabled and self._lora_runtime() is not None:
            raise RuntimeError("MXFP8 mode runs fused adapters only: fuse_lora() (the fused weights are quantised), disable_adapters() or "
                               "delete_adapter() before enable_mxfp8()")
        self._mxfp8 = bool(enabled)
        self._mx_gen += 1
        self._mx_cache = None
        if self._mxfp8 and len(self.transformer_blocks):
            w = self.transformer_blocks[0].ff.net[2].weight
            if w.is_cuda and w.dtype == BF16:
                self._mxfp8_weights()
        return self

    @property
    def mxfp8_enabled(self) -> bool:
        return self._mxfp8

    def _mxfp8_weights(self):
        """Per block {"qkv", "out", "ff1", "ff2": (q, s)} of the MXFP8 weights.  A block is re-quantised (into the same storage) when one of
        its weights changed since - in-place edits bump ``_version``, moves change ``data_ptr``, a replaced Parameter changes identity, fused
        optimizer steps move the weights epoch: the rules of ``GraphedTransformer._weights_version``."""
        blocks = self.transformer_blocks
        if self._mx_cache is None or len(self._mx_cache) != len(blocks):
            self._mx_cache = [None] * len(blocks)
        out = []
        for i, blk in enumerate(blocks):
            at, ff = blk.attn1, blk.ff
            ws = (at.to_q.weight, at.to_k.weight, at.to_v.weight, at.to_out[0].weight, ff.net[0].proj.weight, ff.net[2].weight)
            key = tuple((id(w), w._version, w.data_ptr(), str(w.device)) for w in ws) + (_state.weights_epoch[0],)
            ent = self._mx_cache[i]
            if ent is None or ent[0] != key:
                for w in ws:
                    if w.shape[0] % 128 or w.shape[1] % 128:
                        raise ValueError(f"MXFP8 mode needs block GEMM widths that are multiples of 128 (got a {tuple(w.shape)} weight)")
                old = ent[1] if ent is not None else {}
                new = {}
                for name, w in (("qkv", torch.cat([x.detach() for x in ws[:3]], dim=0)), ("out", ws[3]), ("ff1", ws[4]), ("ff2", ws[5])):
                    w = w.detach().contiguous()
                    q, sc = old.get(name, (None, None))
                    if q is None or q.shape != w.shape or q.device != w.device:
                        q, sc = None, None
                    new[name] = ops.mxfp8_quantize(w, q=q, s=sc)
                ent = self._mx_cache[i] = (key, new)
            out.append(ent[1])
        return out

    def _mx_block(self, blk, wq, ws, m1, m2, mb, mg, grp, B, S, Nt, rope, scale):
        """One transformer block (:394-445) with its four GEMMs on MXFP8: LayerNorm-modulate writes the MXFP8 A operand of QKV and FFN1;
        QKV writes the raw projection, which ``orv_qkv_prep`` normalises (+ RoPE) in place; attention writes row-major bf16 and the
        hidden state of the FeedForward is row-major bf16, both quantised for the GEMM that follows."""
        c = self.config
        D, heads = self.inner_dim, c.num_attention_heads
        M = B * S
        x, qkv, att, hbuf, s_pad = ws["x"], ws["qkv"], ws["att"], ws["h"], ws["s_pad"]
        at, f0, f2 = blk.attn1, blk.ff.net[0].proj, blk.ff.net[2]
        FF = f0.weight.shape[0]
        need = M * max(D, FF)
        if ws.get("mx_q") is None or ws["mx_q"].numel() < need:
            ws["mx_q"] = torch.empty(need, dtype=torch.uint8, device=x.device)
            ws["mx_s"] = torch.empty(need // 32, dtype=torch.uint8, device=x.device)
        aq, asc = ws["mx_q"], ws["mx_s"]
        qd, sd = aq[:M * D].view(M, D), asc[:M * D // 32].view(M, D // 32)
        qf, sf = aq[:M * FF].view(M, FF), asc[:M * FF // 32].view(M, FF // 32)
        ops.layernorm_modulate_mxfp8(x, qd, sd, blk.norm1.norm.weight, blk.norm1.norm.bias, m1[..., D:2 * D], m1[..., :D], mb, mg, grp, B,
                                     D, c.norm_eps)
        _, bqkv = at.packed_qkv()
        ops.gemm_mxfp8(qd, sd, *wq["qkv"], bqkv, qkv, M, 3 * D, D)
        nq, nk = at.norm_q, at.norm_k
        ops.qkv_prep(qkv, None, nq.weight, nq.bias, nk.weight, nk.bias, rope, B, S, heads, Nt, s_pad, at.eps, q_premul=scale * LOG2E)
        bound = at.score_bound(scale, rope is not None)
        ops.attention_fwd(qkv, None, att, B, S, heads, s_pad, 1.0 / LOG2E, score_bound=bound, ws=ws["attn_ws"])
        ops.mxfp8_quantize(att, M, D, qd, sd, ldx=D)
        ops.gemm_mxfp8(qd, sd, *wq["out"], at.to_out[0].bias, x, M, D, D, epilogue=2, R=x, ldr=D, gate=m1[..., 2 * D:], gate_b=mb,
                       gate_g=mg, grp=grp)
        ops.layernorm_modulate_mxfp8(x, qd, sd, blk.norm2.norm.weight, blk.norm2.norm.bias, m2[..., D:2 * D], m2[..., :D], mb, mg, grp, B,
                                     D, c.norm_eps)
        ops.gemm_mxfp8(qd, sd, *wq["ff1"], f0.bias, hbuf, M, FF, D, epilogue=1)
        ops.mxfp8_quantize(hbuf, M, FF, qf, sf, ldx=FF)
        ops.gemm_mxfp8(qf, sf, *wq["ff2"], f2.bias, x, M, D, FF, epilogue=2, R=x, ldr=D, gate=m2[..., 2 * D:], gate_b=mb, gate_g=mg, grp=grp)

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    # ---- config / checkpoint surface (:950-1087; diffusers ModelMixin subset) ----
    @classmethod
    def from_config(cls, config, **kwargs):
        cfg = {k: v for k, v in dict(config).items() if not k.startswith("_")}
        cfg.update(kwargs)
        return cls(**cfg)

    @classmethod
    def load_config(cls, path, subfolder: Optional[str] = None, **_):
        d = os.path.join(path, subfolder) if subfolder and os.path.isdir(os.path.join(path, subfolder)) else path
        with open(os.path.join(d, cls.config_name), "r", encoding="utf-8") as f:
            return json.load(f)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder: Optional[str] = None, torch_dtype=None,
                        revision=None, variant=None, **kwargs):
        """Loads an ORV checkpoint directly, or converts: a vanilla CogVideoX transformer (2B: T2V->I2V channel doubling with
        the new half zeroed, :1016-1030), or an ORV checkpoint into a model with EXTRA modules requested through kwargs
        (``multiview=True``, ``recon_action=True``, ``visual_guidance=True`` - the train script's finetune flow,
        train...sft.py:276-283): the reference's strict load fails there, is caught (:970) and answered by
        ``from_config(base.config, **kwargs)`` + ``load_state_dict(strict=False)`` + the ``mv_blocks`` copy (:1043-1050).
        Without kwargs a same-class checkpoint with missing / unexpected keys is a RuntimeError (:955-967)."""
        from .checkpoint import load_state_dict_dir
        path = str(pretrained_model_name_or_path)
        d = os.path.join(path, subfolder) if subfolder and os.path.isdir(os.path.join(path, subfolder)) else path
        config = cls.load_config(path, subfolder=subfolder)
        state = load_state_dict_dir(d)
        same_class = config.get("_class_name") == cls.__name__
        cfg = {k: v for k, v in config.items() if not k.startswith("_")}
        model = None
        if same_class:
            # :954-968 - load as this class with the caller's overrides applied; any missing / unexpected / mismatched key is
            # an error there, which the reference catches (:970) and answers with the conversion path below
            try:
                cand = cls(**{**cfg, **kwargs})
                missing, unexpected = cand.load_state_dict(state, strict=False)   # size mismatches raise RuntimeError
                msg = ""
                if missing:
                    msg += f"Some weights of {cls.__name__} are not found in pretrained weights: {missing}. "
                if unexpected:
                    msg += f"Some weights may be lost in {cls.__name__}: {unexpected}. "
                if msg:
                    raise RuntimeError(msg)
                model = cand
            except RuntimeError as e:
                if not kwargs:           # nothing to convert to: the checkpoint itself is inconsistent with its config
                    raise
                cls._last_load_fallback = str(e)
        if model is None:
            # :974-1050 - conversion: build from the CHECKPOINT's config plus the caller's kwargs, load what matches
            # (strict=False; a shape mismatch still raises, as torch does), widen a T2V patch embedding, seed mv_blocks
            kwargs = dict(kwargs)
            if fnmatch.fnmatch(path, 'THUDM*CogVideoX*'):
                for k in ("sample_height", "sample_width", "sample_frames"):
                    cfg[k] = kwargs.pop(k)
            if fnmatch.fnmatch(path, 'THUDM*CogVideoX*-2b*'):
                assert cfg['in_channels'] == 16, f'Wrong `in_channels` in config of {path}!'
                cfg['in_channels'] = 32
                model = cls(**{**cfg, **kwargs, "from_t2v": True})
                state = dict(state)
                w = state.pop('patch_embed.proj.weight')
                model.load_state_dict(state, strict=False)
                model.patch_embed.proj.weight.data[:, :16, ...].copy_(w)
            else:
                model = cls(**{**cfg, **kwargs})
                model.load_state_dict(state, strict=False)
            # a checkpoint that is not multiview itself seeds every mv_block from the 3-D attention block beside it (:1043-1050)
            if model.config.multiview and not ('multiview' in path or config.get("multiview", False)):
                for i in range(len(model.mv_blocks)):
                    model.mv_blocks[i].load_state_dict(model.transformer_blocks[i].state_dict(), strict=False)
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        model._set_trainable_parameters()
        return model

    def save_pretrained(self, save_directory, is_main_process: bool = True, save_function: Optional[Callable] = None,
                        safe_serialization: bool = True, variant: Optional[str] = None,
                        max_shard_size: Union[int, str] = "5GB", push_to_hub: bool = False, state_dict=None, **kwargs):
        """``state_dict``: the tensors to write in place of ``self.state_dict()`` (same keys; orv_amd.train_state passes the copies its
        snapshot took, so that the file holds the weights of the save and not of whenever the writer gets to them)."""
        from .checkpoint import save_state_dict_dir
        if not is_main_process:
            return
        os.makedirs(save_directory, exist_ok=True)
        save_state_dict_dir(self.state_dict() if state_dict is None else state_dict, save_directory, max_shard_size=max_shard_size)
        cfg = {**dict(self.config), "_class_name": "CogVideoXTransformer3DModelTraj", "_diffusers_version": "0.32.0.dev0"}
        with open(os.path.join(save_directory, self.config_name), "w", encoding="utf-8") as f:
            json.dump(cfg, f, indent=2)

    @staticmethod
    def compute_action_loss(x, x_recon, loss_weight: dict, mask: Optional[torch.Tensor] = None):
        """:690-713 (tiny [B,16,7] tensors; plain torch)."""
        import torch.nn.functional as F
        if mask is None:
            mask = torch.ones((x.size(0),), device=x.device).bool()
        rot_loss = 1 - torch.cos(x_recon[mask, ..., 3:6] - x[mask, ..., 3:6]).mean()
        x_recon[..., -1] = torch.sigmoid(x_recon[..., -1])
        pos_loss = F.smooth_l1_loss(x_recon[mask, ..., :3], x[mask, ..., :3])
        grip_loss = F.smooth_l1_loss(x_recon[mask, ..., -1], x[mask, ..., -1])
        return (rot_loss * loss_weight['rot_loss'], pos_loss * loss_weight['pos_loss'],
                grip_loss * loss_weight['grip_loss'])

    # ---- the hot path ----
    def _workspace(self, B, S, Nv, dev):
        c = self.config
        D, H = self.inner_dim, c.num_attention_heads
        key = (B, S, Nv, str(dev))
        if key not in self._ws:
            s_pad = (S + 63) // 64 * 64
            M = B * S
            e = lambda *shape, dt=BF16: torch.empty(*shape, dtype=dt, device=dev)
            # attention workspace: partial results of the key-split last round (orv_attention_fwd_bounded_ws); None when the shape's
            # grid has no small last round (B = 1, B = 2, the 5B widths)
            nb = ops.attention_ws_bytes(B, S, H)
            # att and h carry orv_packed_rows(M) row slots: on the packed path (below) they hold the P16 layout, else rows [0, M) row-major
            Mp = ops.packed_rows(M)
            self._ws = {key: dict(x=e(M, D), xn=e(Mp, D), qkv=e(M, 3 * D), att=e(Mp, D), h=e(Mp, 4 * D), vis=e(B * Nv, D),
                                  vis2=e(B * Nv, D), s_pad=s_pad,
                                  attn_ws=torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None)}
        ws = self._ws[key]
        # the packed-operand plan is derived from the library's tile chooser: valid for the orv_gemm_force_tile epoch it was made in
        # (a tile pinned later left a stale plan asking the d8 kernel for a shape the pin excludes)
        ep = ops.lib().orv_gemm_force_epoch()
        if ws.get("packed_epoch") != ep:
            FF = self.transformer_blocks[0].ff.net[0].proj.weight.shape[0] if len(self.transformer_blocks) else 4 * D
            ws["packed"], ws["packed_epoch"] = self._packed_plan(B * S, D, FF), ep
        return ws

    def softmax_kernel_census(self, rope: bool = False) -> Dict[str, Any]:
        """Which attention-softmax form every block's CURRENT weights select: ``layers_static`` (fixed-shift kernel: the qk-LayerNorm
        bound stays below ``orv_attention_static_limit``) / ``layers_online`` (running max), and the largest bound.  A trained checkpoint
        whose norm_q / norm_k gains push a layer's bound past the limit moves that layer - and only that layer - onto the online kernel."""
        scale = 1.0 / math.sqrt(self.config.attention_head_dim)
        ats = [b.attn1 for b in self.transformer_blocks]
        prime_score_bounds(ats, scale, rope=rope)
        lim = float(ops.lib().orv_attention_static_limit(1))
        bounds = [a.score_bound(scale, rope) for a in ats]
        static = sum(1 for b in bounds if b is not None and 0.0 < b <= lim)
        return {"layers_static": static, "layers_online": len(ats) - static, "static_limit_log2": lim,
                "max_bound_log2": round(max((b for b in bounds if b is not None), default=float("nan")), 2)}

    @staticmethod
    def _packed_plan(M, D, FF=None):
        """Which GEMMs of a block take their A operand in the packed P16 layout (round 5, csrc/gemm_d8.hip: A straight to registers, twice
        the bytes in flight of the LDS-staged kernel; bit-identical results).  The producer must be an MFMA kernel that writes the layout for
        free - FFN2's A is FFN1's GELU epilogue (cogvideox_control.py:439 -> :440), the out-projection's A is the attention output (:256-263) -
        and the d8 kernel must be the better choice for the shape: exactly where the row-major cost model picks the 256 x 192 t8 tile
        (same tile count; B = 1 and other single-round shapes keep their smaller row-major tiles).  ``ORV_GEMM_PACKED=0``: A/B switch."""
        plan = {"ffn": False, "out": False, "qkv": False, "ffn1": False}
        FF = FF or 4 * D                      # FeedForward inner dimension as built (``ff.net[0].proj.weight.shape[0]``)
        if os.environ.get("ORV_GEMM_PACKED", "1") == "0":
            return plan
        t8_192 = "gemm_t8_kernel<192, 2>"
        # FeedForward pair: wherever FFN1 can write the packed hidden state (the t8 kernel's 256-wide GELU epilogue) and a d8 tile takes
        # FFN2 - measured better at B = 4 (256 x 192 tiles: -0.7 % in the model), B = 2 and B = 1 (256 x 128 tiles against the single-round
        # simple kernels: 0.203 -> 0.180 ms and 0.118 -> 0.093 ms standalone, profiles/r5_gemm_d8_b1.txt)
        if (ops.gemm_kernel_name(M, D, FF, 2, a_packed=True) is not None
                and ops.gemm_kernel_name(M, FF, D, 1, c_packed=True) is not None):
            plan["ffn"] = True
        # out-projection (K = D: 30 K-tiles, epilogue-heavy): where the row-major model picks the 256 x 192 t8 tile (B = 4: -6 %) and where the
        # 256 x 128 d8 tiles fit ONE round of the CUs (B = 1: 0.037 -> 0.033 ms); in between (B = 2: 390 tiles) the row-major kernel wins
        kn_out = ops.gemm_kernel_name(M, D, D, 2, a_packed=True)
        if kn_out is not None:
            one_round = D % 128 == 0 and -(-M // 256) * (D // 128) <= _num_cus()
            want_out = os.environ.get("ORV_PACKED_OUT", "auto")
            # round 6: measured again with the 192-row d8 tiles (gemm_d8r192_kernel: 510 tiles of 192 x 128 at two clips) - the row-major kernel
            # still wins there (0.0603 vs 0.0610 ms, step 22.41 vs 22.50 ms, profiles/r6_gemm_d8_r192.txt); ORV_PACKED_OUT = 0 / 1 force it
            if want_out == "1" or (want_out == "auto" and (ops.gemm_kernel_name(M, D, D, 2) == t8_192 or one_round)):
                plan["out"] = True
        # the LayerNorm outputs (A of q | k | v and of FFN1): the producer is a row-per-wave VALU kernel whose packed store scatters 16-byte
        # pieces - a loss at B = 4 and B = 2 (profiles/r5_model_ab_packed_ln.txt, r5_packed_qkv_b1.txt: +2.7 % / +1.2 % per step).  At ONE clip the
        # q | k and v launches are single, latency-bound rounds (255 tiles each) and ONE d8 launch for q | k | v is shorter than the pair
        # (0.0871 -> 0.0792 ms, step -1.3 %): "auto" takes the packed path exactly there.  ORV_PACKED_QKV / ORV_PACKED_FFN1 = 0 / 1 force them.
        if D <= 2048 and D % 192 == 0:
            want = os.environ.get("ORV_PACKED_QKV", _PACKED_QKV_DEFAULT)
            single_round = -(-M // 192) * (2 * D // 256) <= _num_cus()
            kn_qkv = ops.gemm_kernel_name(M, 3 * D, D, 4, a_packed=True)
            if (want == "1" or (want == "auto" and single_round)) and kn_qkv is not None:
                plan["qkv"] = True
            if (plan["ffn"] and os.environ.get("ORV_PACKED_FFN1", _PACKED_FFN1_DEFAULT) == "1"
                    and ops.gemm_kernel_name(M, FF, D, 1, a_packed=True, c_packed=True) is not None):
                plan["ffn1"] = True
        return plan

    def _view_pos_table(self, pos, n_view, T, P, dev):
        key = ("posv", n_view, T, P, str(dev))
        if key not in self._ws:
            D = self.inner_dim
            pv = self.pos_embedding_v.to(device=dev, dtype=torch.float32).reshape(self.config.max_n_view, -1, D)[:n_view]
            if pv.shape[1] != P:
                raise ValueError(f"pos_embedding_v is built for {pv.shape[1]} spatial tokens, got {P} (:679-688)")
            base = pos.float().reshape(1, T, P, D) if pos is not None else 0.0
            # the reference rounds to bf16 after each of the two adds; one table keeps a single rounding in the epilogue
            tab = (base + pv.to(BF16).float()[:, None]).reshape(n_view * T * P, D)
            self._ws[key] = tab.to(BF16).contiguous()
        return self._ws[key]

    def _pointer_tables(self, dev):
        """Device arrays of weight/bias pointers of every AdaLN linear (norm1, norm2 of each block; norm_out), built once."""
        lins = [n.linear for blk in self.transformer_blocks for n in (blk.norm1, blk.norm2)]
        key = (str(dev),) + tuple(l.weight.data_ptr() for l in lins) + (self.norm_out.linear.weight.data_ptr(),)
        if getattr(self, "_ptr_tables", None) is None or self._ptr_tables[0] != key:
            def arr(ts):
                return torch.tensor([0 if t is None else t.data_ptr() for t in ts], dtype=torch.int64, device=dev)
            no = self.norm_out.linear
            self._ptr_tables = (key, dict(w_blk=arr([l.weight for l in lins]), b_blk=arr([l.bias for l in lins]),
                                          w_out=arr([no.weight]), b_out=arr([no.bias])))
        return self._ptr_tables[1]

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor,
                controls_or_guidances: Dict[str, torch.Tensor], timestep: Union[int, float, torch.LongTensor],
                timestep_cond: Optional[torch.Tensor] = None, ofs: Optional[Union[int, float, torch.LongTensor]] = None,
                image_rotary_emb: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                attention_kwargs: Optional[Dict[str, Any]] = None, return_dict: bool = True, num_views: int = 1,
                image_rotary_emb_view: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        c = self.config
        if self._mxfp8 and (self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()))):
            raise RuntimeError("MXFP8 mode is inference-only: call model.eval() and run under torch.no_grad() (or "
                               "requires_grad_(False)), or turn it off with enable_mxfp8(False) before training")
        if self._step_cache is not None:
            from .step_cache import SUPPORTED as _SC_SUPPORTED
            if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                raise RuntimeError(f"step cache: this forward records gradients; {_SC_SUPPORTED} - or disable_step_cache()")
            if _chains() > 1:
                raise RuntimeError(f"step cache: ORV_CHAINS = {_chains()}; {_SC_SUPPORTED} (the segments stay single-stream)")
        if not hidden_states.is_cuda:
            raise RuntimeError("orv_amd runs on MI355X only: move the model and its inputs to the GPU (no CPU fallback)")
        # attention_kwargs["scale"] multiplies the active adapter's coefficient for this call (:729-741); ignored without an adapter
        lora_rt = self._lora_runtime((attention_kwargs or {}).get("scale", 1.0)) if self._lora_active is not None else None
        if lora_rt is not None and self._mxfp8:
            raise RuntimeError("MXFP8 mode runs fused adapters only: fuse_lora(), disable_adapters() or enable_mxfp8(False)")
        if self.dtype != BF16:
            raise RuntimeError(f"orv_amd kernels are bf16: call model.to(torch.bfloat16) (got {self.dtype}).  The reference's "
                               "`--dtype float16` (inference_control_to_video.py:198-203) is not provided - its default and every shipped "
                               "config is bfloat16; run with `--dtype bfloat16`")
        if num_views > 1 and not c.multiview:
            raise ValueError("num_views > 1 needs a multiview=True model (pos_embedding_v / mv_blocks, :592-606)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            # training step (train_cogvideox_control_to_video_sft.py:1051-1093): forward that saves activations, with the
            # hand-written backward attached to autograd as one node
            if self._lora_fused is not None:
                raise RuntimeError("an adapter is fused into the weights: unfuse_lora() before a forward that records gradients")
            out, mask, recon = _training.forward_with_grad(self, hidden_states, encoder_hidden_states, controls_or_guidances, timestep,
                                                 ofs, image_rotary_emb, num_views, image_rotary_emb_view, lora=lora_rt)
            if not return_dict:
                return (out, mask, recon)
            return Transformer3DModelTrajOutput(sample=out, is_action_mask=mask, actions_recon=recon)
        with torch.no_grad():
            return self._forward_inference(hidden_states, encoder_hidden_states, controls_or_guidances, timestep, ofs,
                                           image_rotary_emb, return_dict, num_views, image_rotary_emb_view, lora=lora_rt)

    # ---- multiview (:273-348, :797-800) ----
    def _mv_state(self, b, v, f, Nt, P, S, dev):
        """Per-shape cache of the multiview regrouping: ``stages.mv_layout`` (row index, sizes) plus the workspace of ``_mv_block``."""
        key = ("mv", b, v, f, Nt, P, str(dev))
        if key not in self._ws:
            D = self.inner_dim
            lay = stages.mv_layout(b, v, f, Nt, P, S, dev)
            e = lambda *shape: torch.empty(*shape, dtype=BF16, device=dev)
            self._ws[key] = dict(lay, xm=e(lay["R"], D), qkv=e(lay["R"], 3 * D), att=e(lay["R"], D))
        return self._ws[key]

    def _mv_pointer_tables(self, dev):
        lins = [blk.norm1.linear for blk in self.mv_blocks]
        key = (str(dev),) + tuple(l.weight.data_ptr() for l in lins)
        if getattr(self, "_mv_ptr_tables", None) is None or self._mv_ptr_tables[0] != key:
            arr = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=dev)
            self._mv_ptr_tables = (key, arr([l.weight for l in lins]), arr([l.bias for l in lins]))
        return self._mv_ptr_tables[1:]

    @staticmethod
    def _qkv_projection(at, xn, qkv, rope, B, S, heads, n_text, s_pad, scale, raw=None, a_packed=False):
        """to_q / to_k / to_v + norm_q / norm_k (+ RoPE) (:232-254): q', k', v into ``qkv``; the attention kernel reads all three
        in place (V through transposing LDS reads: no V^T copy).  Without RoPE the qk LayerNorm and the softmax pre-multiplier
        (scale * log2 e, one rounding) ride in the GEMM epilogue; with RoPE the projection is followed by ``orv_qkv_prep``.
        ``raw`` (training) receives the un-normalised projection for the LayerNorm adjoint."""
        D = heads * 64
        M = B * S
        wqkv, bqkv = at.packed_qkv()
        nq, nk = at.norm_q, at.norm_k
        if rope is None and _FUSE_QKNORM:
            ops.gemm(xn, wqkv, bqkv, qkv, M, 3 * D, D, epilogue=4, Y=raw,
                     qknorm=(nq.weight, nq.bias, nk.weight, nk.bias, at.eps, scale * LOG2E, heads), a_packed=a_packed)
        else:
            dst = qkv if raw is None else raw
            ops.gemm(xn, wqkv, bqkv, dst, M, 3 * D, D, a_packed=a_packed)
            ops.qkv_prep(qkv, None, nq.weight, nq.bias, nk.weight, nk.bias, rope, B, S, heads, n_text, s_pad, at.eps,
                         q_premul=scale * LOG2E, src=raw)

    def _mv_block(self, blk, mv, m, x, xn, grp0, Bv, S, Nt, n_view, n_frame, rope_view=None):
        """MVBlock.forward (:313-348): AdaLN (no action term) -> tokens of all views of one frame attend jointly ->
        to_out, proj_out -> rearranged back and added with gate_msa.  m: this block's fp32 table [Bv, 2, 3D]."""
        c = self.config
        D, heads = self.inner_dim, c.num_attention_heads
        at = blk.attn1
        ops.layernorm_modulate(x, xn, blk.norm1.norm.weight, blk.norm1.norm.bias, m[..., D:2 * D], m[..., :D],
                               2 * 3 * D, 3 * D, grp0, Bv, D, c.norm_eps)
        R, Sm, s_pad = mv["R"], mv["Sm"], mv["s_pad"]
        ops.gather_rows(xn, mv["idx"], mv["xm"], R, D)
        scale = 1.0 / math.sqrt(c.attention_head_dim)
        self._qkv_projection(at, mv["xm"], mv["qkv"], rope_view, R // Sm, Sm, heads, n_view * Nt, s_pad, scale)
        ops.attention_fwd(mv["qkv"], None, mv["att"], R // Sm, Sm, heads, s_pad, 1.0 / LOG2E, score_bound=at.score_bound(scale, rope_view is not None))
        ops.gemm(mv["att"], at.to_out[0].weight, at.to_out[0].bias, mv["xm"], R, D, D)
        ops.gemm(mv["xm"], blk.proj_out.weight, blk.proj_out.bias, mv["att"], R, D, D)
        # '(b f) (v s) d -> (b v) (f s) d' + gated residual on the video rows only (the text output of attn1 is dropped)
        ops.scatter_gated_rows(mv["att"], mv["idx"], m[:, 1, 2 * D:], 2 * 3 * D, x, R, D, S, Nt)

    def _base_attention(self, blk, ws, packed, m1, mb, mg, grp, B, S, Nt, rope, scale):
        """norm1 -> q | k | v -> attention -> gated out-projection residual of one block (:394-437), packed operands where the plan says so."""
        c = self.config
        D, heads = self.inner_dim, c.num_attention_heads
        M = B * S
        x, xn, qkv, att, s_pad = ws["x"], ws["xn"], ws["qkv"], ws["att"], ws["s_pad"]
        at = blk.attn1
        ops.layernorm_modulate(x, xn, blk.norm1.norm.weight, blk.norm1.norm.bias, m1[..., D:2 * D], m1[..., :D],
                               mb, mg, grp, B, D, c.norm_eps, out_packed=packed["qkv"])
        self._qkv_projection(at, xn, qkv, rope, B, S, heads, Nt, s_pad, scale, a_packed=packed["qkv"])
        bound = at.score_bound(scale, rope is not None)
        # packed path: the attention kernel writes its output, the FFN1 GELU epilogue the hidden state, in the P16 layout the d8 GEMM reads
        att_p = packed["out"] and ws["attn_ws"] is None and ops.attention_packed_ok(bound, 1.0 / LOG2E)
        if att_p:
            ops.attention_fwd(qkv, None, att, B, S, heads, s_pad, 1.0 / LOG2E, score_bound=bound, out_packed=True)
        else:
            ops.attention_fwd(qkv, None, att, B, S, heads, s_pad, 1.0 / LOG2E, score_bound=bound, ws=ws["attn_ws"])
        ops.gemm(att, at.to_out[0].weight, at.to_out[0].bias, x, M, D, D, epilogue=2, R=x, ldr=D,
                 gate=m1[..., 2 * D:], gate_b=mb, gate_g=mg, grp=grp, a_packed=att_p)

    def _lora_attention(self, blk, lbw, lora, ws, m1, mb, mg, grp, B, S, Nt, rope, scale):
        """The same with an active LoRA adapter (orv_amd/lora.py): row-major operands throughout; the rank updates are added to the raw
        q | k | v projection before ``orv_qkv_prep`` and to the residual stream before the unchanged out-projection launch."""
        c = self.config
        D, heads = self.inner_dim, c.num_attention_heads
        M = B * S
        x, xn, qkv, att, s_pad = ws["x"], ws["xn"], ws["qkv"], ws["att"], ws["s_pad"]
        at = blk.attn1
        need = M * 3 * lora.rp
        if ws.get("lora_t") is None or ws["lora_t"].numel() < need:
            ws["lora_t"] = torch.empty(need, dtype=BF16, device=x.device)
        T = ws["lora_t"]
        ops.layernorm_modulate(x, xn, blk.norm1.norm.weight, blk.norm1.norm.bias, m1[..., D:2 * D], m1[..., :D], mb, mg, grp, B, D, c.norm_eps)
        if lbw.nT:
            _lora.qkv_projection(at, lbw, lora, xn, qkv, T[:M * lbw.nT * lora.rp].view(M, lbw.nT * lora.rp), rope, B, S, heads, Nt, s_pad, scale)
        else:
            self._qkv_projection(at, xn, qkv, rope, B, S, heads, Nt, s_pad, scale)
        bound = at.score_bound(scale, rope is not None)
        ops.attention_fwd(qkv, None, att, B, S, heads, s_pad, 1.0 / LOG2E, score_bound=bound, ws=ws["attn_ws"])
        if lbw.out_params is not None:
            _lora.out_update(lbw, lora, att, T[:M * lora.rp].view(M, lora.rp), x, x, M, D, m1[..., 2 * D:], mb, mg, grp)
        ops.gemm(att, at.to_out[0].weight, at.to_out[0].bias, x, M, D, D, epilogue=2, R=x, ldr=D, gate=m1[..., 2 * D:], gate_b=mb, gate_g=mg,
                 grp=grp)

    def _forward_inference(self, hidden_states, encoder_hidden_states, controls_or_guidances, timestep, ofs,
                           image_rotary_emb, return_dict, num_views=1, image_rotary_emb_view=None, lora=None):
        """Workspace lookup -> ``stages.embed`` -> score-bound priming -> blocks -> ``stages.head``.  With the
        step cache on (section 20) the block loop is cut behind iteration 0 and behind the last iteration: ``StepCache.run``."""
        ctx = self._inference_front(hidden_states, encoder_hidden_states, controls_or_guidances, timestep, ofs, image_rotary_emb,
                                    return_dict, num_views, image_rotary_emb_view, lora)
        if self._step_cache is not None:
            return self._step_cache.run(self, ctx)
        self._run_blocks(ctx, 0, len(self.transformer_blocks))
        return self._inference_head(ctx)

    def _inference_front(self, hidden_states, encoder_hidden_states, controls_or_guidances, timestep, ofs, image_rotary_emb, return_dict,
                         num_views, image_rotary_emb_view, lora):
        """Everything ahead of the block loop -> the forward's context: shapes, workspace, the embed stage's outputs, block operands."""
        c = self.config
        sh = stages.shapes(hidden_states, encoder_hidden_states, num_views, c)
        ws = self._workspace(sh.B, sh.S, sh.Nv, hidden_states.device)
        st = stages.embed(self, sh, ws["x"], hidden_states, encoder_hidden_states, controls_or_guidances, timestep, ofs, image_rotary_emb,
                          image_rotary_emb_view)
        scale = 1.0 / math.sqrt(c.attention_head_dim)
        prime_score_bounds([b.attn1 for b in self.transformer_blocks], scale, rope=st.rope is not None)
        if st.mv is not None:
            prime_score_bounds([b.attn1 for b in self.mv_blocks], scale, rope=st.rope_view is not None)
        from types import SimpleNamespace
        return SimpleNamespace(sh=sh, ws=ws, st=st, x=ws["x"], scale=scale, lora=lora, num_views=num_views, return_dict=return_dict,
                               mxw=self._mxfp8_weights() if self._mxfp8 else None)

    def _run_blocks(self, ctx, i0, i1):
        """Iterations [i0, i1) of the block loop (:861-907 -> :394-445) on the joint buffer of ``ctx``."""
        c = self.config
        sh, ws, st, lora, mxw, scale = ctx.sh, ctx.ws, ctx.st, ctx.lora, ctx.mxw, ctx.scale
        B, S, Nt, D, M, T = sh.B, sh.S, sh.Nt, sh.D, sh.M, sh.T
        x, xn, hbuf, packed = ws["x"], ws["xn"], ws["h"], ws["packed"]
        mod, grp, rope, mv = st.mod, st.grp, st.rope, st.mv
        mb, mg = sh.G * 3 * D, 3 * D
        for i in range(i0, i1):
            blk = self.transformer_blocks[i]
            if mv is not None:
                self._mv_block(self.mv_blocks[i], mv.ws, mv.mod[i], x, xn, mv.grp0, B, S, Nt, ctx.num_views, T, st.rope_view)
            m1, m2 = mod[2 * i], mod[2 * i + 1]
            if mxw is not None:
                self._mx_block(blk, mxw[i], ws, m1, m2, mb, mg, grp, B, S, Nt, rope, scale)
                continue
            lbw = lora.block(i) if lora is not None else None
            if lbw is not None:
                self._lora_attention(blk, lbw, lora, ws, m1, mb, mg, grp, B, S, Nt, rope, scale)
            else:
                self._base_attention(blk, ws, packed, m1, mb, mg, grp, B, S, Nt, rope, scale)
            ops.layernorm_modulate(x, xn, blk.norm2.norm.weight, blk.norm2.norm.bias, m2[..., D:2 * D], m2[..., :D],
                                   mb, mg, grp, B, D, c.norm_eps, out_packed=packed["ffn1"])
            f0, f2 = blk.ff.net[0].proj, blk.ff.net[2]
            ops.gemm(xn, f0.weight, f0.bias, hbuf, M, f0.weight.shape[0], D, epilogue=1, a_packed=packed["ffn1"], c_packed=packed["ffn"])
            ops.gemm(hbuf, f2.weight, f2.bias, x, M, D, f0.weight.shape[0], epilogue=2, R=x, ldr=D,
                     gate=m2[..., 2 * D:], gate_b=mb, gate_g=mg, grp=grp, a_packed=packed["ffn"])

    def _inference_head(self, ctx):
        st = ctx.st
        output, _ = stages.head(self, ctx.sh, ctx.x, ctx.ws["vis"], ctx.ws["vis2"], st.modf)
        if not ctx.return_dict:
            return (output, st.is_action_mask, st.actions_recon)
        return Transformer3DModelTrajOutput(sample=output, is_action_mask=st.is_action_mask, actions_recon=st.actions_recon)

    # ---- first-block step cache (orv_amd/step_cache.py) ----
    def enable_step_cache(self, threshold, max_consecutive_skips=None):
        """Turn the opt-in, lossy first-block step cache on -> its ``StepCache``.  Every inference forward then runs the embedding and
        the first block, and skips the remaining blocks when the first block's residual moved by less than ``threshold`` (relative L1,
        largest over the clips) since the last computed forward; ``max_consecutive_skips`` caps runs of skipped forwards."""
        from . import step_cache as _sc
        if len(self.transformer_blocks) < 2:
            raise ValueError(f"step cache: num_layers = {len(self.transformer_blocks)}; {_sc.SUPPORTED}")
        self._sc_gen += 1
        self._step_cache = _sc.StepCache(threshold, max_consecutive_skips, generation=self._sc_gen)
        return self._step_cache

    def disable_step_cache(self):
        self._step_cache = None
        return self


# ------------------------------------------------------------------------------------------------------------------
# sampler pipeline (:1090-1489)
# ------------------------------------------------------------------------------------------------------------------
_FUSE_QKNORM = os.environ.get("ORV_FUSED_QKNORM", "1") != "0"      # A/B switch: 0 = projection + orv_qkv_prep


def _chains() -> int:
    """ORV_CHAINS=n (default 1): GraphedTransformer cuts a batch into n chains on n streams (see ``GraphedTransformer._forward``)."""
    try:
        return max(1, int(os.environ.get("ORV_CHAINS", "1")))
    except ValueError:
        return 1


_PACKED_QKV_DEFAULT, _PACKED_FFN1_DEFAULT = "auto", "0"


def _num_cus() -> int:
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count if torch.cuda.is_available() else 256


class _NotCapturable(TypeError):
    """A call argument of a kind ``GraphedTransformer`` cannot hold in static buffers: the caller falls back to eager launches."""


class GraphedTransformer:
    """One denoise step's transformer forward replayed from a HIP graph (``torch.cuda.CUDAGraph`` over the library's
    launches on the capture stream): ~330 kernel launches become one submission, which matters when the step is short
    (B=1: ~17 ms of kernels).

    A captured graph bakes in the ADDRESS of every tensor it touched, so the wrapper owns static copies of ALL tensor
    inputs (latents, prompt embeddings, timestep, ofs, rotary tables, every control tensor) and refreshes them with
    ``copy_`` before each replay; callers may pass fresh tensors on every call.  The cache key is the inputs' shapes /
    dtypes / structure plus the non-tensor arguments, the model's weights epoch (fused optimizer steps) and the sum of the
    parameters' ``_version`` counters (``load_state_dict`` / in-place edits), so stale weights are never replayed.  The
    first call per key runs eagerly (builds pointer tables / workspaces / position tables), the second is captured, later
    ones replay.  At most ``max_entries`` graphs are kept (least recently used is dropped with its workspace)."""

    def __init__(self, transformer, max_entries: int = 4):
        from collections import OrderedDict
        self.tr = transformer
        self.max_entries = max_entries
        self._state = OrderedDict()
        _state.watch_parameter_registration()

    @staticmethod
    def _flatten(kw):
        """(tensor leaves in a fixed order, structure descriptor) of the call's keyword arguments."""
        leaves, desc = [], []
        for k in sorted(kw):
            v = kw[k]
            if torch.is_tensor(v):
                leaves.append(v); desc.append((k, "t", tuple(v.shape), str(v.dtype)))
            elif isinstance(v, (tuple, list)) and v and all(torch.is_tensor(x) for x in v):
                leaves.extend(v); desc.append((k, "seq", tuple((tuple(x.shape), str(x.dtype)) for x in v)))
            elif isinstance(v, dict):
                sub = []
                for kk in sorted(v):
                    vv = v[kk]
                    if torch.is_tensor(vv):
                        leaves.append(vv); sub.append((kk, tuple(vv.shape), str(vv.dtype)))
                    elif vv is None:
                        sub.append((kk, None))
                    else:
                        raise _NotCapturable(f"GraphedTransformer: unsupported entry {k}[{kk!r}] of type {type(vv).__name__}")
                desc.append((k, "dict", tuple(sub)))
            elif v is None or isinstance(v, (bool, int, float, str)):
                desc.append((k, "v", v))
            else:
                raise _NotCapturable(f"GraphedTransformer: unsupported argument {k} of type {type(v).__name__}")
        return leaves, tuple(desc)

    @staticmethod
    def _rebuild(kw, static):
        """kw with every tensor leaf replaced by the matching static buffer (same traversal order as ``_flatten``)."""
        it = iter(static)
        out = {}
        for k in sorted(kw):
            v = kw[k]
            if torch.is_tensor(v):
                out[k] = next(it)
            elif isinstance(v, (tuple, list)) and v and all(torch.is_tensor(x) for x in v):
                out[k] = tuple(next(it) for _ in v)
            elif isinstance(v, dict):
                out[k] = {kk: (next(it) if torch.is_tensor(vv) else vv) for kk, vv in sorted(v.items())}
            else:
                out[k] = v
        return out

    def _weights_version(self):
        """In-place edits bump ``_version``; storage moves (``p.data = ...``: FusedAdamW's flat layout, ``.to()``) change
        ``data_ptr``; a parameter REPLACED by another object (``m.weight = nn.Parameter(...)``, ``load_state_dict(assign=True)``),
        added or removed goes through ``Module.register_parameter`` / ``__delattr__``: the process-wide registration hook
        (``_state.param_epoch``) and the parameter count tell, and the cached parameter list is re-collected then (the
        old list kept the replaced objects, whose identity, version and storage never change again, and the graph replayed the
        old weights).  The per-call cost is one pass over the cached list - no module walk on the B = 1 path the graph exists
        to speed up; every data_ptr enters the key (a sampled subset missed moves of the unsampled ones)."""
        ps = getattr(self, "_plist", None)
        self._vcalls = getattr(self, "_vcalls", 0) + 1
        if ps is not None and self._pepoch == _state.param_epoch[0]:
            # structural fingerprint: edits that bypass register_parameter / register_module - ``del m.weight``, ``del blocks[k:]``,
            # writes into ``_parameters`` / ``_modules`` - change the live counts of the cached module list; a full re-walk every 64th call
            # catches what keeps the counts (a same-size swap inside ``_modules``).  ~600 dict lengths per call, no generator walk.
            fp = (sum(len(m._parameters) for m in self._mlist), sum(len(m._modules) for m in self._mlist))
            if fp != self._mfp or (self._vcalls & 63) == 0 and [id(m) for m in self.tr.modules()] != self._mids:
                ps = None
        if ps is None or self._pepoch != _state.param_epoch[0]:
            self._mlist = list(self.tr.modules())
            self._mids = [id(m) for m in self._mlist]
            self._mfp = (sum(len(m._parameters) for m in self._mlist), sum(len(m._modules) for m in self._mlist))
            ps = self._plist = list(self.tr.parameters())
            self._pepoch = _state.param_epoch[0]
        return (len(ps), len(self._mlist), sum(p._version for p in ps), hash(tuple(p.data_ptr() for p in ps)), hash(tuple(map(id, ps))))

    # ---- batch chains (experiment, ORV_CHAINS=n): the clips of a batch are independent until the sampler's update, so the batch can be cut
    # into n chains that run the SAME forward on n streams inside the captured graph.  Every kernel of the path is persistent / fills the
    # chip on its own, so two chains do not co-run in steady state - but the ramp and the tail of every launch (first loads of a cold
    # pipeline, the last tile's epilogue, a last round that does not fill its slots) overlap with the neighbouring launch of the other
    # chain instead of leaving the CUs idle behind the in-order barrier of a single stream.  Results are bit-identical to the uncut call
    # (every kernel is deterministic and batch independent); the action-mask draw is made ONCE for the whole batch, before the fork, so the
    # global RNG stream advances exactly as in the uncut call.
    def _chain_parts(self, kw, n):
        hs = kw["hidden_states"]
        B = hs.shape[0]
        if n <= 1 or B % n or B < n:
            return None
        b = B // n

        def cut(v, i):
            return v[i * b:(i + 1) * b] if (torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B) else v
        parts = []
        for i in range(n):
            d = {}
            for k, v in kw.items():
                if k in ("hidden_states", "encoder_hidden_states", "timestep"):
                    d[k] = cut(v, i)
                elif k == "controls_or_guidances" and isinstance(v, dict):
                    d[k] = {kk: cut(vv, i) for kk, vv in v.items()}
                else:
                    d[k] = v
            parts.append(d)
        return parts

    def _forward(self, kw, st, concurrent):
        """``self.tr(**kw)``, cut into ``ORV_CHAINS`` batch chains when that is enabled and the batch divides; ``concurrent``: the chains
        run on side streams (inside a capture), else one after the other on the current stream (the eager warm-up call)."""
        n = _chains()
        parts = self._chain_parts(kw, n) if n > 1 else None
        if parts is None:
            out = self.tr(**kw)
            st["ws"] = self.tr._ws
            return out
        tr = self.tr
        B = kw["hidden_states"].shape[0]
        b = B // n
        dev = kw["hidden_states"].device
        ae = getattr(tr, "action_embed", None)
        ctl = kw.get("controls_or_guidances") or {}
        full_mask = saved_mask = None
        if ae is not None and ctl.get("actions", None) is not None:
            saved_mask = ae.forced_mask
            if saved_mask is not None:
                if saved_mask.device != dev or saved_mask.dtype != torch.bool:      # once, like ActionEmbed.forward: no H2D copy per call
                    saved_mask = ae.forced_mask = saved_mask.to(device=dev, dtype=torch.bool)
                full_mask = saved_mask
            else:
                full_mask = torch.rand(B, device=dev) < 0.1          # the draw ActionEmbed.forward would make for the whole batch
        chain_ws = st.setdefault("chain_ws", [dict() for _ in range(n)])
        saved_ws = tr._ws
        cur = torch.cuda.current_stream(dev)
        side = []
        if concurrent:
            side = getattr(self, "_side", None)
            if side is None or len(side) < n - 1 or side[0].device != dev:
                side = self._side = [torch.cuda.Stream(device=dev) for _ in range(n - 1)]
            fork = torch.cuda.Event()
            fork.record(cur)
        outs = []
        try:
            for i, pkw in enumerate(parts):
                tr._ws = chain_ws[i]
                if full_mask is not None:
                    ae.forced_mask = full_mask[i * b:(i + 1) * b]
                if concurrent and i:
                    side[i - 1].wait_event(fork)
                    with torch.cuda.stream(side[i - 1]):
                        outs.append(tr(**pkw))
                else:
                    outs.append(tr(**pkw))
                chain_ws[i] = tr._ws
        finally:
            tr._ws = saved_ws
            if full_mask is not None:
                ae.forced_mask = saved_mask
        if concurrent:
            for s in side[:n - 1]:
                cur.wait_stream(s)
        st["ws"] = chain_ws
        cat = lambda j: (None if outs[0][j] is None else torch.cat([o[j] for o in outs], dim=0))
        sample, mask, recon = cat(0), cat(1), cat(2)
        if isinstance(outs[0], tuple):
            return (sample, mask, recon) if len(outs[0]) == 3 else (sample,) + tuple(outs[0][1:])
        return Transformer3DModelTrajOutput(sample=sample, is_action_mask=mask, actions_recon=recon)

    def __call__(self, hidden_states, encoder_hidden_states, timestep, **kw):
        kw = dict(kw, hidden_states=hidden_states, encoder_hidden_states=encoder_hidden_states, timestep=timestep)
        akw = kw.pop("attention_kwargs", None)
        leaves, desc = self._flatten(kw)
        # adapter state: generation (add / set / delete / enable / fuse), active name and this call's scale; in-place edits of adapter
        # values move the parameters' _version sum / the weights epoch like any other weight
        lkey = self.tr._lora_key((akw or {}).get("scale", 1.0)) if getattr(self.tr, "_lora_active", None) is not None else None
        if akw is not None:
            if any(torch.is_tensor(v) for v in akw.values()):
                raise _NotCapturable("GraphedTransformer: tensor entries in attention_kwargs")
            kw["attention_kwargs"] = akw
        # MXFP8 state: a graph captured in one mode never replays in the other, nor after a re-enable (new quantised weights)
        mx = (self.tr._mx_gen,) if getattr(self.tr, "_mxfp8", False) else None
        base = (desc, _state.weights_epoch[0], self._weights_version(), self.tr.training, _chains(), mx, lkey)
        sc = getattr(self.tr, "_step_cache", None)
        if sc is None:
            return self._replay(base, kw, leaves, self._forward, self.max_entries)
        return self._call_segments(base, kw, leaves, sc)

    def _call_segments(self, base, kw, leaves, sc):
        """A forward with the step cache on: three entries per call shape - front (embed, iteration 0, probe),
        tail (iterations 1 .. L-1, store, head) and skip (apply, head) - with the one host read of the step between front and the rest.
        The front entry keeps the forward's context (modulation tables, row maps, RoPE tables, workspace) alive for the other two, which
        are captured only against a CAPTURED front: its tensors have fixed addresses then."""
        limit = 3 * self.max_entries
        gen = sc.generation

        def front(kw_, st, concurrent):
            sc._segment = "front"
            try:
                self._forward(kw_, st, concurrent)
            finally:
                sc._segment = None
            st["ctx"] = sc._ctx
            return None
        self._replay(base + (gen, "front"), kw, leaves, front, limit)
        fst = self._state[base + (gen, "front")]
        sc.adopt(fst["ctx"])
        skip = sc.decide_now()
        run = lambda kw_, st, concurrent: sc.segment(self.tr, skip)
        if "graph" not in fst:
            with torch.no_grad():
                return run(None, None, False)
        key = base + (gen, "skip" if skip else "tail")
        if key in self._state and self._state[key].get("front") is not fst:     # captured against a front entry that is gone
            del self._state[key]
        out = self._replay(key, {}, [], run, limit)
        self._state[key]["front"] = fst
        if base + (gen, "front") in self._state:
            self._state.move_to_end(base + (gen, "front"))                       # never dropped ahead of its tail / skip entries
        return out

    def _replay(self, key, kw, leaves, forward, limit):
        """``forward(kw, st, concurrent)`` under the entry ``key``: eager on the first call, captured on the second, replayed from then on."""
        st = self._state.get(key)
        if st is None:                       # eager warm-up call
            st = self._state[key] = {"calls": 1}
            while len(self._state) > limit:
                self._state.popitem(last=False)
            with torch.no_grad():
                return forward(kw, st, False)
        self._state.move_to_end(key)
        if st.get("eager_only"):             # a capture of this key failed before: plain launches from now on
            with torch.no_grad():
                return forward(kw, st, False)
        if "graph" not in st:
            st["static"] = [t.clone() for t in leaves]
            skw = self._rebuild(kw, st["static"])
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            try:
                # thread_local: another thread's CUDA calls (a DataLoader pin_memory thread during in-training validation,
                # base_train.yaml pin_memory / 8 workers) must not invalidate this capture
                with torch.no_grad(), torch.cuda.graph(g, capture_error_mode="thread_local"):
                    st["out"] = forward(skw, st, True)                   # st["ws"]: the captured launches point into these workspaces -
            except _NotCapturable:
                raise
            except Exception as e:           # out of memory in the private pool, a syncing op, a foreign capture-unsafe call
                for k in ("static", "out", "ws", "chain_ws"):
                    st.pop(k, None)
                st["eager_only"] = True
                import warnings
                warnings.warn(f"orv_amd: HIP-graph capture of the transformer forward failed ({type(e).__name__}: {e}); this call "
                              "shape runs with eager launches from now on (set ORV_HIP_GRAPH=0 or pipe.enable_hip_graph(False) to "
                              "skip the attempt)", RuntimeWarning)
                torch.cuda.synchronize()
                with torch.no_grad():
                    return forward(kw, st, False)
            st["graph"] = g                                              # kept alive even if the model later swaps in another one
            st["lora"] = getattr(self.tr, "_lora_cached_operands", lambda: None)()   # the adapter operand copies the captured launches read
        else:
            for dst, src in zip(st["static"], leaves):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
        st["graph"].replay()
        return st["out"]


class CogVideoXPipelineOutput:
    def __init__(self, frames):
        self.frames = frames


class ChannelsLastFrames:
    """Marks a bf16 [B, 1, H, W, 8] tensor as reference frames already laid out for ``vae.encode_channels_last`` (what
    ``orv_frames_handoff`` writes for a rollout's next chunk), so that ``prepare_latents`` encodes it as it is."""

    def __init__(self, data):
        self.data = data


class CogVideoXImageToVideoPipelineTraj:
    """The reference's I2V pipeline (:1090-1489) with the call surface its entry points use
    (/root/reference/orv/pipeline/inference_control_to_video.py:71-146, evaluation_control_to_video.py:245-349):
    ``from_pretrained`` / ``save_pretrained`` / ``to`` / ``__call__(image=<PIL | tensor>, prompt=<str>, negative_prompt=...,
    output_type='pil' | 'latent' | 'pt' | 'np')`` / ``.scheduler`` / ``.vae`` / ``.text_encoder`` / ``.transformer``.

    Built here (MI355X): ``prepare_latents`` (:1115-1225), the denoise loop (:1402-1473) and - SURVEY §8(f) rank 1 - the VAE
    (``orv_amd.vae.AutoencoderKLCogVideoX``, parity unpinned) and the T5 text encoder (``orv_amd.t5.T5EncoderModel``); the tokenizer
    is outside this build.  The pipeline DELEGATES to whatever
    ``vae`` / ``text_encoder`` / ``tokenizer`` objects it holds with exactly the calls the reference and its diffusers base
    class make (``vae.encode(x).latent_dist.sample(generator)``, ``vae.decode(z).sample``, ``tokenizer(prompt,
    padding='max_length', ...)``, ``text_encoder(ids)[0]``), so diffusers' own ``AutoencoderKLCogVideoX`` and transformers'
    ``T5EncoderModel`` drop in as well.  Without them, pass pre-encoded latents / ``prompt_embeds`` and
    ``output_type='latent'`` (what the reference's dataset cache provides)."""

    config_name = "model_index.json"

    def __init__(self, tokenizer=None, text_encoder=None, vae=None, transformer: CogVideoXTransformer3DModelTraj = None,
                 scheduler: Union[CogVideoXDDIMScheduler, CogVideoXDPMScheduler] = None):
        if not isinstance(transformer, CogVideoXTransformer3DModelTraj):
            raise ValueError("The transformer in this pipeline must be of type CogVideoXTransformer3DModelTraj")
        self.tokenizer, self.text_encoder, self.vae = tokenizer, text_encoder, vae
        self.transformer, self.scheduler = transformer, scheduler
        vcfg = getattr(vae, "config", None)
        self.vae_scale_factor_spatial = 2 ** (len(vcfg.block_out_channels) - 1) if vcfg is not None else 8
        self.vae_scale_factor_temporal = getattr(vcfg, "temporal_compression_ratio", 4) if vcfg is not None else 4
        self.vae_scaling_factor_image = getattr(vcfg, "scaling_factor", 1.15258426) if vcfg is not None else 1.15258426
        self._guidance_scale, self._interrupt, self._num_timesteps = 1.0, False, 0
        self._graphed: Optional[GraphedTransformer] = None
        self._graph_mode: Optional[bool] = None      # None: automatic (see transformer_forward); True / False: enable_hip_graph()
        self._step_cache_policy = (1, 1)             # (compute_first, compute_last) of enable_step_cache()
        self._step_cache_report: List[tuple] = []
        from .components import VideoProcessor
        self.video_processor = VideoProcessor(vae_latent_channels=getattr(vcfg, "latent_channels", 16) if vcfg is not None else 16,
                                              vae_scale_factor=self.vae_scale_factor_spatial)          # :1110-1113

    guidance_scale = property(lambda self: self._guidance_scale)
    interrupt = property(lambda self: self._interrupt)
    num_timesteps = property(lambda self: self._num_timesteps)

    @property
    def invert_scale_latents(self) -> bool:
        """Read at call time like the reference (:1186): its entry points overwrite ``pipe.vae`` config AFTER construction
        (inference_control_to_video.py:108)."""
        vcfg = getattr(self.vae, "config", None)
        if vcfg is None:
            return False
        try:
            return bool(vcfg["invert_scale_latents"] if isinstance(vcfg, dict) else getattr(vcfg, "invert_scale_latents", False))
        except KeyError:
            return False

    # ---- construction / persistence (diffusers DiffusionPipeline subset the entry points use) ----
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, transformer=None, scheduler=None, vae=None, text_encoder=None,
                        tokenizer=None, torch_dtype=None, **_unused):
        """Reads ``model_index.json`` of a pipeline directory (the layout ``save_pretrained`` and the reference's final export
        write, train...sft.py:1184-1199): ``transformer/`` through ``CogVideoXTransformer3DModelTraj.from_pretrained`` (ORV
        or vanilla CogVideoX weights), ``scheduler/scheduler_config.json`` into this package's scheduler of the recorded
        class.  Components passed as keyword arguments win (inference_control_to_video.py:80-84 passes ``transformer=``).
        A ``vae/`` folder is loaded into ``orv_amd.vae.AutoencoderKLCogVideoX`` (diffusers' key names); a T5 under
        ``text_encoder/`` + ``tokenizer/`` is loaded through ``transformers`` when that package is importable; without it
        ``text_encoder/`` goes into ``orv_amd.t5.T5EncoderModel`` and the tokenizer has to be supplied."""
        path = str(pretrained_model_name_or_path)
        index = {}
        ipath = os.path.join(path, cls.config_name)
        if os.path.exists(ipath):
            with open(ipath, "r", encoding="utf-8") as f:
                index = json.load(f)
        if transformer is None:
            if not os.path.isdir(os.path.join(path, "transformer")):
                raise OSError(f"{path} has no transformer/ folder: pass transformer=")
            transformer = CogVideoXTransformer3DModelTraj.from_pretrained(path, subfolder="transformer", torch_dtype=torch_dtype)
        if scheduler is None:
            spath = os.path.join(path, "scheduler", "scheduler_config.json")
            if os.path.exists(spath):
                with open(spath, "r", encoding="utf-8") as f:
                    scfg = json.load(f)
                name = scfg.get("_class_name") or (index.get("scheduler") or [None, "CogVideoXDDIMScheduler"])[1]
                sched_cls = {"CogVideoXDDIMScheduler": CogVideoXDDIMScheduler, "CogVideoXDPMScheduler": CogVideoXDPMScheduler}.get(name)
                if sched_cls is None:
                    raise ValueError(f"scheduler class {name} is not a CogVideoX scheduler")
                scheduler = sched_cls.from_config(scfg)
            else:
                raise OSError(f"{path} has no scheduler/scheduler_config.json: pass scheduler=")
        if vae is None and os.path.exists(os.path.join(path, "vae", "config.json")):
            from .vae import AutoencoderKLCogVideoX            # the MI355X VAE (parity unpinned)
            vae = AutoencoderKLCogVideoX.from_pretrained(path, subfolder="vae", torch_dtype=torch_dtype)
        if text_encoder is None and os.path.isdir(os.path.join(path, "text_encoder")):
            try:
                from transformers import T5EncoderModel
            except Exception:            # package absent: the encoder of this library (orv_amd.t5, transformers' checkpoint layout)
                from .t5 import T5EncoderModel
                try:
                    text_encoder = T5EncoderModel.from_pretrained(path, subfolder="text_encoder", torch_dtype=torch_dtype)
                except Exception:        # absent / foreign weights or an unsupported config: None, as in the branch below
                    text_encoder = None
            else:
                try:
                    text_encoder = T5EncoderModel.from_pretrained(path, subfolder="text_encoder", torch_dtype=torch_dtype)
                except Exception:        # absent weights: stays None, prompt= then asks for prompt_embeds
                    text_encoder = None
        if tokenizer is None and os.path.isdir(os.path.join(path, "tokenizer")):
            try:
                from transformers import T5Tokenizer
                tokenizer = T5Tokenizer.from_pretrained(path, subfolder="tokenizer")
            except Exception:
                tokenizer = None
        pipe = cls(tokenizer=tokenizer, text_encoder=text_encoder, vae=vae, transformer=transformer, scheduler=scheduler)
        if torch_dtype is not None:
            pipe.to(dtype=torch_dtype)
        return pipe

    def save_pretrained(self, save_directory, safe_serialization: bool = True, max_shard_size: Union[int, str] = "5GB", **kw):
        """``model_index.json`` + ``transformer/`` + ``scheduler/scheduler_config.json``; ``vae`` / ``text_encoder`` /
        ``tokenizer`` are written by their own ``save_pretrained`` when they have one."""
        os.makedirs(save_directory, exist_ok=True)
        index = {"_class_name": type(self).__name__, "_diffusers_version": "0.32.0.dev0",
                 "transformer": ["orv_amd", type(self.transformer).__name__],
                 "scheduler": ["orv_amd", type(self.scheduler).__name__]}
        self.transformer.save_pretrained(os.path.join(save_directory, "transformer"), safe_serialization=safe_serialization,
                                         max_shard_size=max_shard_size)
        os.makedirs(os.path.join(save_directory, "scheduler"), exist_ok=True)
        with open(os.path.join(save_directory, "scheduler", "scheduler_config.json"), "w", encoding="utf-8") as f:
            json.dump({**dict(self.scheduler.config), "_class_name": type(self.scheduler).__name__,
                       "_diffusers_version": "0.32.0.dev0"}, f, indent=2)
        for name in ("vae", "text_encoder", "tokenizer"):
            obj = getattr(self, name)
            if obj is not None and hasattr(obj, "save_pretrained"):
                obj.save_pretrained(os.path.join(save_directory, name))
                index[name] = [type(obj).__module__.split(".")[0], type(obj).__name__]
        with open(os.path.join(save_directory, self.config_name), "w", encoding="utf-8") as f:
            json.dump(index, f, indent=2)

    # memory management of the reference's entry points: one MI355X holds every component (288 GB), nothing is offloaded
    def enable_model_cpu_offload(self, *a, **k):
        return self

    def enable_sequential_cpu_offload(self, *a, **k):
        return self

    def maybe_free_model_hooks(self):
        return None

    def progress_bar(self, iterable=None, total=None):
        try:
            from tqdm.auto import tqdm
            return tqdm(iterable, total=total, disable=getattr(self, "_progress_bar_disabled", True))
        except Exception:                # pragma: no cover
            import contextlib
            return contextlib.nullcontext()

    def set_progress_bar_config(self, **kw):
        self._progress_bar_disabled = bool(kw.get("disable", False))

    # ---- text side: delegate to the attached T5 (diffusers CogVideoXPipeline.encode_prompt / _get_t5_prompt_embeds) ----
    def _get_t5_prompt_embeds(self, prompt, num_videos_per_prompt=1, max_sequence_length=226, device=None, dtype=None):
        if self.tokenizer is None or self.text_encoder is None:
            raise NotImplementedError("prompt= needs the pipeline's `tokenizer` and `text_encoder` (T5) objects: attach a tokenizer "
                                      "(transformers' T5Tokenizer or any callable of its call shape; not built here) and "
                                      "text_encoder=orv_amd.t5.T5EncoderModel.from_pretrained(path, subfolder='text_encoder'), or pass "
                                      "prompt_embeds (the reference's dataset caches them, dataset.py:1056-1059)")
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        text_inputs = self.tokenizer(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                                     add_special_tokens=True, return_tensors="pt")
        ids = text_inputs.input_ids if hasattr(text_inputs, "input_ids") else text_inputs["input_ids"]
        enc_dev = getattr(self.text_encoder, "device", device)
        embeds = self.text_encoder(ids.to(enc_dev))[0].to(dtype=dtype, device=device)
        b, seq, _ = embeds.shape
        return embeds.repeat(1, num_videos_per_prompt, 1).view(b * num_videos_per_prompt, seq, -1)

    def encode_prompt(self, prompt, negative_prompt=None, do_classifier_free_guidance: bool = True,
                      num_videos_per_prompt: int = 1, prompt_embeds=None, negative_prompt_embeds=None,
                      max_sequence_length: int = 226, device=None, dtype=None):
        device = device or self._execution_device
        dtype = dtype or self.transformer.dtype
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt) if prompt is not None else prompt_embeds.shape[0]
        if prompt_embeds is None:
            prompt_embeds = self._get_t5_prompt_embeds(prompt, num_videos_per_prompt, max_sequence_length, device, dtype)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            negative_prompt = negative_prompt or ""
            negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
            if prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            if batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            negative_prompt_embeds = self._get_t5_prompt_embeds(negative_prompt, num_videos_per_prompt, max_sequence_length,
                                                                device, dtype)
        return prompt_embeds, negative_prompt_embeds

    def check_inputs(self, image, prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs,
                     prompt_embeds=None, negative_prompt_embeds=None):
        """diffusers ``CogVideoXImageToVideoPipeline.check_inputs`` (called at :1261-1270)."""
        import PIL.Image
        if not torch.is_tensor(image) and not isinstance(image, PIL.Image.Image) and not isinstance(image, list):
            raise ValueError("`image` has to be of type `torch.Tensor` or `PIL.Image.Image` or `List[PIL.Image.Image]` but is"
                             f" {type(image)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        allowed = {"latents", "prompt_embeds", "negative_prompt_embeds"}
        if callback_on_step_end_tensor_inputs is not None and not all(k in allowed for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {sorted(allowed)}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None and prompt_embeds.shape != negative_prompt_embeds.shape:
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                             f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds`"
                             f" {negative_prompt_embeds.shape}.")

    def decode_latents(self, latents: torch.Tensor) -> torch.Tensor:
        """Hands the latents to the attached VAE exactly as the base diffusers pipeline does (``[B,F,C,h,w] -> [B,C,F,h,w]``,
        divided by the VAE scaling factor, ``vae.decode(...).sample``)."""
        if self.vae is None or not hasattr(self.vae, "decode"):
            raise NotImplementedError("VAE decode needs the pipeline's `vae` object (orv_amd.vae.AutoencoderKLCogVideoX or "
                                      "diffusers' class): attach one or use output_type='latent'")
        z = latents.permute(0, 2, 1, 3, 4) / self.vae_scaling_factor_image
        out = self.vae.decode(z)
        return getattr(out, "sample", out)

    # ---- LoRA (diffusers ``CogVideoXLoraLoaderMixin`` subset; the adapters live on the transformer, orv_amd/lora.py) ----
    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, adapter_name: Optional[str] = None, **kwargs):
        """Loads ``pytorch_lora_weights.safetensors`` (directory, file or state dict with ``transformer.``-prefixed keys) into the
        transformer and makes it the active adapter."""
        self.transformer.load_lora_adapter(pretrained_model_name_or_path_or_dict, adapter_name=adapter_name or "default",
                                           prefix="transformer")
        self.transformer.set_adapter(adapter_name or "default")

    def unload_lora_weights(self):
        tr = self.transformer
        tr.unfuse_lora()
        for name in list(tr._lora_adapters):
            tr.delete_adapter(name)

    def fuse_lora(self, lora_scale: float = 1.0, **kwargs):
        self.transformer.fuse_lora(lora_scale=lora_scale)

    def unfuse_lora(self, **kwargs):
        self.transformer.unfuse_lora()

    @classmethod
    def save_lora_weights(cls, save_directory, transformer_lora_layers: Dict[str, torch.Tensor] = None, is_main_process: bool = True,
                          transformer_lora_adapter_metadata: Optional[Dict[str, Any]] = None, **kwargs):
        """Writes ``transformer_lora_layers`` (``transformer.get_adapter_state_dict()``: keys without a prefix) as
        ``pytorch_lora_weights.safetensors`` with ``transformer.``-prefixed keys; ``transformer_lora_adapter_metadata`` (``r``,
        ``lora_alpha``, ``use_rslora``) goes into the file's ``lora_adapter_metadata`` entry."""
        from safetensors.torch import save_file
        if not transformer_lora_layers:
            raise ValueError("You must pass `transformer_lora_layers`.")
        if not is_main_process:
            return
        os.makedirs(save_directory, exist_ok=True)
        sd = {(k if k.startswith("transformer.") else "transformer." + k): v.detach().to("cpu").contiguous()
              for k, v in transformer_lora_layers.items()}
        meta = {"format": "pt"}
        if transformer_lora_adapter_metadata:
            meta["lora_adapter_metadata"] = json.dumps(dict(transformer_lora_adapter_metadata), sort_keys=True)
        save_file(sd, os.path.join(save_directory, _lora.LORA_WEIGHT_NAME), metadata=meta)

    def enable_hip_graph(self, enabled: bool = True):
        """Force (``True``) or forbid (``False``) replaying the transformer forward of each denoise step from a HIP graph (see
        ``GraphedTransformer``).  Without this call the choice is automatic: ``__call__`` - the surface the reference's entry points
        use unchanged, inference_control_to_video.py:122-146 - replays from a graph whenever it can (below)."""
        self._graph_mode = bool(enabled)
        self._graphed = GraphedTransformer(self.transformer) if enabled else None
        return self

    def enable_step_cache(self, threshold, *, max_consecutive_skips=None, compute_first: int = 1, compute_last: int = 1):
        """Turn the opt-in, lossy first-block step cache of the transformer on for this pipeline's denoise loops (DESIGN.md section 20;
        ``CogVideoXTransformer3DModelTraj.enable_step_cache``) -> its ``StepCache``.  Every call (and every chunk of a ``rollout``) starts
        cold; its first ``compute_first`` (>= 1) and last ``compute_last`` (>= 0) steps are computed whatever their distance."""
        for name, v, lo in (("compute_first", compute_first, 1), ("compute_last", compute_last, 0)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"step cache: {name} = {v!r}; supported: an integer >= {lo}")
        sc = self.transformer.enable_step_cache(threshold, max_consecutive_skips)
        self._step_cache_policy = (compute_first, compute_last)
        self._step_cache_report = []
        return sc

    def disable_step_cache(self):
        self.transformer.disable_step_cache()
        self._step_cache_report = []
        return self

    @property
    def step_cache_report(self):
        """(timestep, max distance, skipped, reason) per step of the last call with the step cache on; empty with the cache off."""
        return list(self._step_cache_report)

    def transformer_forward(self, **kw):
        """One transformer forward of the denoise loop (the call at cogvideox_control.py:1415-1425), the way ``__call__`` makes it.
        Default = HIP-graph replay (bit-identical to the eager launches - tests/test_gpu_model.py - and ~1 ms per B = 4 step / ~2.5 ms per
        B = 1 step faster: no launch gaps): on a GPU, outside autograd, unless ``enable_hip_graph(False)`` or ``ORV_HIP_GRAPH=0`` said no.
        The first call per (shapes, weight version) runs eagerly, the second is captured, later ones replay; arguments the graph
        cannot hold in static buffers (``_NotCapturable``) and CPU tensors take the eager launches."""
        tr = self.transformer
        use = self._graph_mode
        if use is None:
            use = (os.environ.get("ORV_HIP_GRAPH", "1") != "0" and kw["hidden_states"].is_cuda and not torch.is_grad_enabled()
                   and not tr.training)
        if use:
            if self._graphed is None or self._graphed.tr is not tr:
                self._graphed = GraphedTransformer(tr)
            try:
                return self._graphed(**kw)
            except _NotCapturable:
                pass
        return tr(**kw)

    def to(self, device=None, dtype=None):
        """``pipe.to(device, dtype=dtype)`` (inference_control_to_video.py:95): every attached torch module follows."""
        if isinstance(device, torch.dtype):
            device, dtype = None, device
        self.transformer.to(device=device, dtype=dtype)
        for obj in (self.vae, self.text_encoder):
            if obj is not None and hasattr(obj, "to"):
                obj.to(device=device, dtype=dtype)
        return self

    @property
    def _execution_device(self):
        return self.transformer.device

    def _scale(self):
        return 1 / self.vae_scaling_factor_image if self.invert_scale_latents else self.vae_scaling_factor_image

    def _image_latents(self, image, batch_size, num_channels_latents, num_views, dtype, device, generator):
        ch = image.size(1)
        image = image.to(device=device, dtype=dtype)
        if image.ndim == 4:
            # RGB reference frames [(b v f), 3, H, W]: encoded by the ATTACHED vae exactly as :1150-1167 (one clip at a time,
            # `retrieve_latents(vae.encode(x), generator)` = latent_dist.sample(generator))
            if ch != 3:
                raise RuntimeError(f'Invalid input channels {image.shape=}!')
            if self.vae is None or not hasattr(self.vae, "encode"):
                raise NotImplementedError("RGB reference frames need a `vae` object with .encode() (SURVEY §8(f) next row is "
                                          "not built here): attach one or pass pre-encoded latents")
            img = image.reshape(batch_size * num_views, -1, *image.shape[1:]).permute(0, 2, 1, 3, 4)     # [(b v), C, f, H, W]
            gens = generator if isinstance(generator, list) else [generator] * img.shape[0]
            lats = [_retrieve_latents(self.vae.encode(img[i].unsqueeze(0)), gens[i if isinstance(generator, list) else 0])
                    for i in range(img.shape[0])]
            image_latents = torch.cat(lats, dim=0).to(dtype).permute(0, 2, 1, 3, 4)                      # [(b v), f, C, h, w]
            image_latents = image_latents.reshape(batch_size, -1, *image_latents.shape[2:])              # [b, (v f), C, h, w]
            image_latents = self._scale() * image_latents
        elif ch == num_channels_latents * 2:
            eps = _randn(tuple(image.shape[:1]) + (num_channels_latents,) + tuple(image.shape[2:]), generator, device, dtype)
            image_latents = ops.gaussian_sample(image, eps.float(), self._scale())         # fused sample+scale+permute
        elif ch == num_channels_latents:
            image_latents = (self._scale() * image).permute(0, 2, 1, 3, 4)
        else:
            raise RuntimeError(f'Invalid input channels {image.shape=} while {num_channels_latents=}!')
        return image_latents

    def prepare_latents(self, image: torch.Tensor, batch_size: int = 1, num_channels_latents: int = 16,
                        num_frames: int = 13, num_views: int = 1, height: int = 60, width: int = 90,
                        dtype: Optional[torch.dtype] = None, device: Optional[torch.device] = None,
                        generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None):
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(
                f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        pt = self.transformer.config.patch_size_t
        t_lat = (num_frames - 1) // self.vae_scale_factor_temporal + 1
        shape = (batch_size, num_views * t_lat, num_channels_latents, height // self.vae_scale_factor_spatial,
                 width // self.vae_scale_factor_spatial)
        if pt is not None:
            shape = shape[:1] + (shape[1] + shape[1] % pt,) + shape[2:]
        if isinstance(image, ChannelsLastFrames):
            from .vae import DiagonalGaussianDistribution
            # reference frames a rollout handed over on the device, already in the encoder's layout [b, f, H, W, 8]: the same moments as
            # vae.encode gives on the same pixels (its own first step is this layout), sampled clip by clip as below
            h = image.data
            if num_views != 1 or h.shape[0] != batch_size:
                raise RuntimeError(f'Invalid channels-last image input: {tuple(h.shape)=} for {batch_size=} and {num_views=}!')
            gens = generator if isinstance(generator, list) else [generator] * batch_size
            lats = [DiagonalGaussianDistribution(self.vae.encode_channels_last(h[i:i + 1], dtype=dtype)).sample(gens[i]) for i in range(batch_size)]
            image_latents = self._scale() * torch.cat(lats, dim=0).to(dtype).permute(0, 2, 1, 3, 4)       # [b, f, C, h, w]
        elif image.ndim not in (4, 5):
            raise RuntimeError(f'Invalid dimensions of image input: {image.shape=}')
        else:
            image_latents = self._image_latents(image, batch_size, num_channels_latents, num_views, dtype, device, generator)
        b, vf = image_latents.shape[:2]
        image_latents = image_latents.reshape(b, num_views, vf // num_views, *image_latents.shape[2:])
        f_img = image_latents.size(2)
        if f_img > t_lat:
            raise RuntimeError(f'Invalid input image_frames={f_img} while num_frames={t_lat}!')
        pad = torch.zeros((batch_size, num_views, t_lat - f_img) + tuple(shape[2:]), device=device, dtype=dtype)
        image_latents = torch.cat([image_latents, pad], dim=2)
        if pt is not None:
            first = image_latents[:, :, : image_latents.size(1) % pt, ...]
            image_latents = torch.cat([first, image_latents], dim=2)
        image_latents = image_latents.flatten(1, 2).contiguous()
        if latents is None:
            latents = _randn(shape, generator, device, dtype)
        else:
            latents = latents.to(device)
        return latents * self.scheduler.init_noise_sigma, image_latents

    @torch.no_grad()
    def __call__(self, image, prompt=None, negative_prompt=None, height: Optional[int] = None,
                 width: Optional[int] = None, num_views: int = 1, num_frames: int = 49, num_inference_steps: int = 50,
                 timesteps: Optional[List[int]] = None, guidance_scale: float = 6, use_dynamic_cfg: bool = False,
                 num_videos_per_prompt: int = 1, eta: float = 0.0, generator=None, latents=None, prompt_embeds=None,
                 negative_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True,
                 attention_kwargs=None, callback_on_step_end=None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 226,
                 controls_or_guidances: Dict[str, torch.Tensor] = {}):
        call = self._prepare_call(image, prompt, negative_prompt, height, width, num_views, num_frames, num_inference_steps, timesteps,
                                  guidance_scale, use_dynamic_cfg, num_videos_per_prompt, eta, generator, latents, prompt_embeds,
                                  negative_prompt_embeds, output_type, return_dict, attention_kwargs, callback_on_step_end,
                                  callback_on_step_end_tensor_inputs, max_sequence_length, controls_or_guidances)
        image = self.video_processor.preprocess(image, height=height, width=width).to(device=call.device, dtype=call.dtype)   # :1366
        video = self._generate(image, call, decode=output_type != "latent")
        if output_type != "latent":                                                  # :1477-1479
            video = self.video_processor.postprocess_video(video=video, output_type=output_type)
        self.maybe_free_model_hooks()
        if not return_dict:
            return (video,)
        return CogVideoXPipelineOutput(frames=video)

    @torch.no_grad()
    def _prepare_call(self, image, prompt=None, negative_prompt=None, height: Optional[int] = None,
                 width: Optional[int] = None, num_views: int = 1, num_frames: int = 49, num_inference_steps: int = 50,
                 timesteps: Optional[List[int]] = None, guidance_scale: float = 6, use_dynamic_cfg: bool = False,
                 num_videos_per_prompt: int = 1, eta: float = 0.0, generator=None, latents=None, prompt_embeds=None,
                 negative_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True,
                 attention_kwargs=None, callback_on_step_end=None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 226,
                 controls_or_guidances: Dict[str, torch.Tensor] = {}):
        """The part of ``__call__`` in front of ``video_processor.preprocess`` (:1261-1364): input checks, prompt embeddings, timesteps,
        the frame count's padding and the occupancy controls.  -> the call's state, which ``_generate`` consumes."""
        tr, sched = self.transformer, self.scheduler
        self.check_inputs(image, prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds,
                          negative_prompt_embeds)
        self._guidance_scale, self._interrupt = guidance_scale, False
        device = self._execution_device
        dtype = tr.dtype
        do_cfg = guidance_scale > 1.0
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(        # :1290-1299 (T5 only when prompt= is used)
            prompt=prompt, negative_prompt=negative_prompt, do_classifier_free_guidance=do_cfg,
            num_videos_per_prompt=num_videos_per_prompt, prompt_embeds=prompt_embeds,
            negative_prompt_embeds=negative_prompt_embeds, max_sequence_length=max_sequence_length, device=device, dtype=dtype)
        batch_size = prompt_embeds.shape[0] // (num_videos_per_prompt if prompt is not None else 1)
        prompt_embeds = prompt_embeds.to(device=device, dtype=dtype)
        if do_cfg:
            prompt_embeds = torch.cat([negative_prompt_embeds.to(device=device, dtype=dtype), prompt_embeds], dim=0)
        timesteps, num_inference_steps = retrieve_timesteps(sched, num_inference_steps, device, timesteps)
        self._num_timesteps = len(timesteps)
        ts_host = timesteps.tolist()
        latent_frames = (num_frames - 1) // self.vae_scale_factor_temporal + 1
        in_ch = tr.config.in_channels
        latent_channels = in_ch // 2 if in_ch != 16 else in_ch
        pt = tr.config.patch_size_t
        controls = dict(controls_or_guidances)
        if pt is not None and latent_frames % pt != 0:
            add = pt - latent_frames % pt
            num_frames += add * self.vae_scale_factor_temporal
            if controls.get('actions', None) is not None:
                a = controls['actions']
                controls['actions'] = torch.cat(
                    [a, torch.zeros((a.size(0), add * self.vae_scale_factor_temporal, a.size(2)), dtype=a.dtype,
                                    device=a.device)], dim=1)
        # occupancy controls given as un-sampled VAE moments [B, 2C, F, H, W] are sampled, scaled and doubled along the
        # channel axis exactly as :1332-1364 (global RNG, like the reference's `.sample()` without a generator)
        for key in ('depths', 'labels'):
            cm = controls.get(key, None)
            if cm is not None and cm.ndim == 5 and cm.size(1) == latent_channels * 2:
                cm = cm.to(device=device, dtype=dtype)
                eps = torch.randn((cm.shape[0], latent_channels) + tuple(cm.shape[2:]), device=device, dtype=dtype)
                lat = ops.gaussian_sample(cm, eps.float(), self._scale())
                controls[key] = torch.cat([lat, lat], dim=2)
        from types import SimpleNamespace
        return SimpleNamespace(device=device, dtype=dtype, do_cfg=do_cfg, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                               batch_size=batch_size * num_videos_per_prompt, ts_host=ts_host, num_inference_steps=num_inference_steps,
                               latent_channels=latent_channels, num_frames=num_frames, num_views=num_views, height=height, width=width,
                               controls=controls, generator=generator, latents=latents, guidance_scale=guidance_scale,
                               use_dynamic_cfg=use_dynamic_cfg, attention_kwargs=attention_kwargs, callback_on_step_end=callback_on_step_end,
                               callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs)

    @torch.no_grad()
    def _generate(self, image, call, decode: bool = True):
        """The part of ``__call__`` behind ``video_processor.preprocess`` (:1367-1479): ``image`` is the preprocessed reference image on the
        device (RGB in [-1, 1], latents or moments; ``ChannelsLastFrames`` for a frame handed over on the device) -> the decoded
        video [B, 3, F, H, W] on the device, or with ``decode=False`` the latents.  The generator is consumed in this order: image
        latents, initial noise, DPM noise."""
        tr, sched = self.transformer, self.scheduler
        device, dtype, do_cfg, prompt_embeds, negative_prompt_embeds = call.device, call.dtype, call.do_cfg, call.prompt_embeds, call.negative_prompt_embeds
        ts_host, num_inference_steps, latent_channels, num_frames, num_views = call.ts_host, call.num_inference_steps, call.latent_channels, call.num_frames, call.num_views
        height, width, controls, generator, latents, guidance_scale = call.height, call.width, call.controls, call.generator, call.latents, call.guidance_scale
        use_dynamic_cfg, attention_kwargs, callback_on_step_end = call.use_dynamic_cfg, call.attention_kwargs, call.callback_on_step_end
        callback_on_step_end_tensor_inputs, pt = call.callback_on_step_end_tensor_inputs, tr.config.patch_size_t
        latents, image_latents = self.prepare_latents(image, call.batch_size, latent_channels,
                                                      num_frames, num_views, height, width, dtype, device, generator,
                                                      latents)
        image_rotary_emb = None
        if tr.config.use_rotary_positional_embeddings:
            from .utils import prepare_rotary_positional_embeddings
            # the reference's inherited helper uses the transformer's sample size as the RoPE base grid
            image_rotary_emb = prepare_rotary_positional_embeddings(
                height, width, latents.size(1), self.vae_scale_factor_spatial, tr.config.patch_size, pt,
                tr.config.attention_head_dim, device,
                base_height=tr.config.sample_height * self.vae_scale_factor_spatial,
                base_width=tr.config.sample_width * self.vae_scale_factor_spatial)
        ofs_emb = None if tr.config.ofs_embed_dim is None else latents.new_full((1,), fill_value=2.0)
        is_dpm = isinstance(sched, CogVideoXDPMScheduler)
        old_x0 = None
        sc = getattr(tr, "_step_cache", None)
        if sc is not None:                   # every call - every chunk of a rollout - starts cold
            sc.reset()
            self._step_cache_report = []
            first, last = self._step_cache_policy
        for i, t in enumerate(ts_host):
            if self._interrupt:
                continue
            if sc is not None and (i < first or i >= len(ts_host) - last):
                sc.force_compute()
            # channel-concat [latents | image_latents] (:1409-1413)
            x_in = torch.cat([latents] * 2) if do_cfg else latents
            img_in = torch.cat([image_latents] * 2) if do_cfg else image_latents
            model_in = torch.cat([x_in, img_in], dim=2)
            tvec = torch.full((model_in.shape[0],), t, device=device, dtype=torch.int64)
            noise_pred = self.transformer_forward(hidden_states=model_in, encoder_hidden_states=prompt_embeds, timestep=tvec, ofs=ofs_emb,
                             image_rotary_emb=image_rotary_emb, attention_kwargs=attention_kwargs,
                             controls_or_guidances=controls, return_dict=False, num_views=num_views)[0]
            if sc is not None:
                rec = sc.history[-1]
                self._step_cache_report.append((t, rec.max_distance, rec.skipped, rec.reason))
            gs = guidance_scale
            if use_dynamic_cfg:
                gs = 1 + guidance_scale * ((1 - math.cos(math.pi * ((num_inference_steps - t) / num_inference_steps) ** 5.0)) / 2)
                self._guidance_scale = gs
            v_u = v_c = noise_pred
            if do_cfg:
                v_u, v_c = noise_pred.chunk(2)
            kw = dict(model_output_uncond=v_u.contiguous() if do_cfg else None, guidance_scale=gs)
            if not is_dpm:
                latents = sched.step(v_c.contiguous(), t, latents, return_dict=False, **kw)[0]
            else:
                latents, old_x0 = sched.step(v_c.contiguous(), old_x0, t, ts_host[i - 1] if i > 0 else None, latents,
                                             generator=generator, **kw)
            if callback_on_step_end is not None:
                avail = {"latents": latents, "prompt_embeds": prompt_embeds,
                         "negative_prompt_embeds": negative_prompt_embeds}
                cb = callback_on_step_end(self, i, t, {k: avail[k] for k in callback_on_step_end_tensor_inputs})
                latents = cb.pop("latents", latents)
                prompt_embeds = cb.pop("prompt_embeds", prompt_embeds)
        b, vf = latents.shape[:2]
        latents = latents.reshape(b * num_views, vf // num_views, *latents.shape[2:])
        return self.decode_latents(latents) if decode else latents

    def rollout(self, image, plan, controls_for_slice, **kw):
        """A cascaded long-video rollout (``orv_amd.rollout.rollout``): one call of this pipeline per slice of ``plan``, the frame handed
        from chunk to chunk and the stitched uint8 episode kept on the device."""
        from .rollout import rollout
        return rollout(self, image, plan, controls_for_slice, **kw)


def _retrieve_latents(encoder_output, generator=None):
    """diffusers ``retrieve_latents`` (sample_mode='sample')."""
    if hasattr(encoder_output, "latent_dist"):
        return encoder_output.latent_dist.sample(generator)
    if hasattr(encoder_output, "latents"):
        return encoder_output.latents
    raise AttributeError("Could not access latents of provided encoder_output")


def _randn(shape, generator, device, dtype):
    """diffusers ``randn_tensor``: a CPU generator draws on the CPU in the target dtype, then the result is copied."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    if isinstance(generator, list):
        return torch.cat([_randn((1,) + tuple(shape[1:]), g, device, dtype) for g in generator], dim=0)
    if generator is not None and generator.device.type == "cpu" and device.type != "cpu":
        return torch.randn(tuple(shape), generator=generator, device="cpu", dtype=dtype).to(device)
    return torch.randn(tuple(shape), generator=generator, device=device, dtype=dtype)
