"""T5 v1.1 text encoder on liborv_mi355.so: the ``text_encoder`` of the CogVideoX pipelines.

The reference encodes prompts with transformers' ``T5EncoderModel`` called as ``text_encoder(ids)[0]``
(/root/reference/orv/models/text_encoder.py:34, from the pipeline at /root/reference/orv/models/cogvideox_control.py:1290-1299).  This
class has that call surface, transformers' module / checkpoint names and transformers' arithmetic (``T5Stack`` in eval mode with no
attention mask: RMS LayerNorm, unscaled attention with a relative-position bias, gated-GELU FFN, no biases); the arithmetic runs in the
HIP kernels (``orv_gather_rows``, ``orv_t5_rmsnorm``, ``orv_gemm_bf16``, ``orv_t5_attention_fwd``, ``orv_geglu``).  Inference only.  The
tokenizer is not part of it.  Nothing here imports ``transformers``."""
from __future__ import annotations

import json
import math
import os
from typing import Optional

import torch
import torch.nn as nn

from .cogvideox_control import FrozenConfig, _NoForward

BF16 = torch.bfloat16
CONFIG_NAME = "config.json"
WEIGHTS_NAME = "model.safetensors"
INDEX_NAME = "model.safetensors.index.json"
SUPPORTED = ("feed_forward_proj 'gated-gelu' (T5 v1.1), d_kv 64, d_model / num_heads * d_kv / d_ff multiples of 64, bfloat16 weights on the "
             "GPU, sequences of at most 512 tokens, no attention mask")

_DEFAULTS = {"vocab_size": 32128, "d_model": 4096, "d_kv": 64, "d_ff": 10240, "num_layers": 24, "num_heads": 64,
             "relative_attention_num_buckets": 32, "relative_attention_max_distance": 128, "dropout_rate": 0.1,
             "layer_norm_epsilon": 1e-6, "initializer_factor": 1.0, "feed_forward_proj": "gated-gelu", "is_encoder_decoder": False,
             "use_cache": False, "tie_word_embeddings": False, "model_type": "t5", "architectures": ["T5EncoderModel"]}


def relative_position_bucket(rel: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """T5's bidirectional bucket of ``rel = key position - query position``.  Evaluated on the HOST with transformers' own fp32 torch
    expression: at distances 16, 32 and 64 the logarithm lands exactly on an integer, which a device ``logf`` need not reproduce."""
    nb = num_buckets // 2
    out = (rel > 0).long() * nb
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).long()
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(n < max_exact, n, large)


def build_bias_rel(table: torch.Tensor, S: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """``relative_attention_bias.weight`` [num_buckets, H] -> fp32 [H, 2S - 1] on the table's device; entry ``j - i + S - 1`` is the bias of
    query i and key j (the operand of ``orv_t5_attention_fwd``).  The bias depends on ``j - i`` only, so the [H, S, S] tensor never exists."""
    bucket = relative_position_bucket(torch.arange(-(S - 1), S), num_buckets, max_distance)
    return table.detach().float()[bucket.to(table.device)].t().contiguous()


class T5EncoderOutput(tuple):
    """``out.last_hidden_state`` and ``out[0]`` are the same tensor (transformers' ``BaseModelOutput`` as the pipelines use it)."""

    def __new__(cls, last_hidden_state):
        return super().__new__(cls, (last_hidden_state,))

    last_hidden_state = property(lambda self: tuple.__getitem__(self, 0))


class _Weight(_NoForward):
    def __init__(self, *shape):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(*shape), requires_grad=False)


class _T5Attention(_NoForward):
    def __init__(self, cfg, has_bias):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        self.q, self.k, self.v = _Weight(inner, cfg.d_model), _Weight(inner, cfg.d_model), _Weight(inner, cfg.d_model)
        self.o = _Weight(cfg.d_model, inner)
        if has_bias:
            self.relative_attention_bias = _Weight(cfg.relative_attention_num_buckets, cfg.num_heads)


class _T5LayerSelfAttention(_NoForward):
    def __init__(self, cfg, has_bias):
        super().__init__()
        self.SelfAttention = _T5Attention(cfg, has_bias)
        self.layer_norm = _Weight(cfg.d_model)


class _T5DenseGatedActDense(_NoForward):
    def __init__(self, cfg):
        super().__init__()
        self.wi_0, self.wi_1, self.wo = _Weight(cfg.d_ff, cfg.d_model), _Weight(cfg.d_ff, cfg.d_model), _Weight(cfg.d_model, cfg.d_ff)


class _T5LayerFF(_NoForward):
    def __init__(self, cfg):
        super().__init__()
        self.DenseReluDense = _T5DenseGatedActDense(cfg)
        self.layer_norm = _Weight(cfg.d_model)


class _T5Block(_NoForward):
    def __init__(self, cfg, has_bias):
        super().__init__()
        self.layer = nn.ModuleList([_T5LayerSelfAttention(cfg, has_bias), _T5LayerFF(cfg)])


class _T5Stack(_NoForward):
    def __init__(self, cfg, embed):
        super().__init__()
        self.embed_tokens = embed
        self.block = nn.ModuleList([_T5Block(cfg, i == 0) for i in range(cfg.num_layers)])
        self.final_layer_norm = _Weight(cfg.d_model)


def _stacked(cache: dict, key, params):
    """One contiguous [sum rows, K] weight holding ``params`` one under the other (ONE GEMM for q | k | v and for wi_0 | wi_1).  The
    parameters are then re-pointed at row slices of that buffer, so there is one copy of the weights and every later in-place change
    (``load_state_dict``, ``copy_``) lands in the GEMM operand; a parameter that was replaced or moved (``.to()``) no longer points into
    the buffer and the stack is rebuilt from the current values."""
    buf = cache.get(key)
    off, ok = 0, buf is not None
    for p in params:
        ok = ok and p.data_ptr() == buf.data_ptr() + off * buf.element_size() and p.dtype == buf.dtype and p.device == buf.device
        off += p.numel()
    if not ok:
        buf = torch.cat([p.detach() for p in params], dim=0).contiguous()
        r = 0
        for p in params:
            p.data = buf[r:r + p.shape[0]]
            r += p.shape[0]
        cache[key] = buf
    return buf


class T5EncoderModel(nn.Module):
    """``T5EncoderModel(config_dict)`` / ``.from_pretrained(path, subfolder=None, torch_dtype=None)`` / ``.save_pretrained(dir)`` /
    ``model(input_ids)[0]``.  ``state_dict()`` carries transformers' keys.  Refused (``ValueError`` naming the supported set): any
    ``feed_forward_proj`` but ``gated-gelu``, ``d_kv != 64``, widths that are not multiples of 64; at call time CPU tensors, weights that
    are not bfloat16, sequences above the attention kernel's maximum, and an attention mask that masks anything."""

    config_name = CONFIG_NAME

    def __init__(self, config=None, **kwargs):
        super().__init__()
        cfg = FrozenConfig({**_DEFAULTS, **{k: v for k, v in dict(config or {}).items()}, **kwargs})
        if cfg.feed_forward_proj != "gated-gelu":
            raise ValueError(f"orv_amd.t5: feed_forward_proj={cfg.feed_forward_proj!r} is not built; supported: {SUPPORTED}")
        if cfg.d_kv != 64:
            raise ValueError(f"orv_amd.t5: d_kv={cfg.d_kv} is not built (the attention kernel has head_dim 64); supported: {SUPPORTED}")
        for name, val in (("d_model", cfg.d_model), ("num_heads * d_kv", cfg.num_heads * cfg.d_kv), ("d_ff", cfg.d_ff)):
            if val <= 0 or val % 64:
                raise ValueError(f"orv_amd.t5: {name}={val} is not a multiple of 64; supported: {SUPPORTED}")
        if cfg.num_layers < 1 or cfg.vocab_size < 1:
            raise ValueError("orv_amd.t5: num_layers and vocab_size must be positive")
        self.config = cfg
        self._stacks, self._ws, self._bias = {}, {}, {}
        self.shared = _Weight(cfg.vocab_size, cfg.d_model)
        self.encoder = _T5Stack(cfg, self.shared)            # encoder.embed_tokens IS shared (one Parameter under both names)
        self.requires_grad_(False).eval()

    def _apply(self, fn, *args, **kwargs):
        for cache in (self._stacks, self._ws, self._bias):    # .to(): the stacked operands and workspaces belong to the old placement
            cache.clear()
        return super()._apply(fn, *args, **kwargs)

    # ---- surface ----
    @property
    def dtype(self):
        return self.shared.weight.dtype

    @property
    def device(self):
        return self.shared.weight.device

    def get_input_embeddings(self):
        return self.shared

    def train(self, mode: bool = True):
        return super().train(False)                           # inference only: there is no dropout path

    @classmethod
    def from_config(cls, config, **kwargs):
        return cls(config, **kwargs)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder: Optional[str] = None, torch_dtype=None, **_unused):
        """``config.json`` + ``model.safetensors`` (or ``model.safetensors.index.json`` + shards) in transformers' layout.  Either or both
        of ``shared.weight`` / ``encoder.embed_tokens.weight`` may be present; ``decoder.*`` / ``lm_head.*`` (a full T5 checkpoint) are
        skipped as transformers' encoder class does; any other missing or unexpected key is a ``RuntimeError``."""
        from .checkpoint import load_state_dict_dir
        path = str(pretrained_model_name_or_path)
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, cls.config_name), "r", encoding="utf-8") as f:
            cfg = json.load(f)
        state = {k: v for k, v in load_state_dict_dir(d, weights_name=WEIGHTS_NAME, index_name=INDEX_NAME, pattern="model*.safetensors").items()
                 if not (k.startswith("decoder.") or k.startswith("lm_head."))}
        model = cls({k: v for k, v in cfg.items() if not k.startswith("_")})
        some = next(iter(state.values()), None)
        if torch_dtype is not None or (some is not None and some.is_floating_point()):
            model.to(torch_dtype if torch_dtype is not None else some.dtype)      # before the copy: no fp32 detour of a bf16 checkpoint
        a, b = "shared.weight", "encoder.embed_tokens.weight"
        if a in state and b not in state:
            state[b] = state[a]
        elif b in state and a not in state:
            state[a] = state[b]
        missing, unexpected = model.load_state_dict(state, strict=False)      # a shape mismatch raises RuntimeError itself
        if missing or unexpected:
            raise RuntimeError(f"T5EncoderModel checkpoint mismatch under {d}: missing {list(missing)[:5]}, unexpected {list(unexpected)[:5]}")
        return model

    def save_pretrained(self, save_directory, max_shard_size="5GB", **_unused):
        """Writes ``config.json`` and ``model.safetensors`` (sharded above ``max_shard_size``); the tied embedding is stored once, as
        ``shared.weight``, like transformers does."""
        from .checkpoint import save_state_dict_dir
        os.makedirs(save_directory, exist_ok=True)
        state = {k: v.detach().cpu().clone() for k, v in self.state_dict().items() if k != "encoder.embed_tokens.weight"}
        save_state_dict_dir(state, save_directory, max_shard_size=max_shard_size, weights_name=WEIGHTS_NAME, index_name=INDEX_NAME)
        with open(os.path.join(save_directory, self.config_name), "w", encoding="utf-8") as f:
            json.dump({**dict(self.config), "torch_dtype": str(self.dtype).replace("torch.", "")}, f, indent=2)

    # ---- caches ----
    def _workspace(self, B, S, dev):
        key = (B, S, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) > 8:
                self._ws.clear()
            c = self.config
            M, D, inner, F = B * S, c.d_model, c.num_heads * c.d_kv, c.d_ff
            e = lambda *shape: torch.empty(*shape, dtype=BF16, device=dev)
            ws = {"idx": torch.empty(M, dtype=torch.int32, device=dev), "x": e(M, D), "h": e(M, D), "qkv": e(M, 3 * inner),
                  "att": e(M, inner), "ff": e(M, 2 * F), "gg": e(M, F)}
            self._ws[key] = ws
        return ws

    def _bias_rel(self, S, dev):
        table = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        key, version = (S, str(dev)), (table.data_ptr(), table._version)
        hit = self._bias.get(key)
        if hit is None or hit[0] != version:                  # in-place edits move `_version`, a replaced tensor moves `data_ptr`
            if len(self._bias) > 8:
                self._bias.clear()
            c = self.config
            hit = (version, build_bias_rel(table, S, c.relative_attention_num_buckets, c.relative_attention_max_distance))
            self._bias[key] = hit
        return hit[1]

    # ---- forward ----
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, return_dict: bool = True, **_unused):
        from . import ops
        c = self.config
        if input_ids is None or input_ids.dim() != 2:
            raise ValueError("orv_amd.t5: input_ids must be a [batch, sequence] integer tensor")
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            raise ValueError("orv_amd.t5: masked keys are out of scope: attention_mask must be None or all ones (the CogVideoX path passes "
                             "none, so padding tokens are attended, /root/reference/orv/models/text_encoder.py:34)")
        dev = self.device
        if dev.type != "cuda" or not input_ids.is_cuda:
            raise ValueError(f"orv_amd.t5: the encoder and input_ids must live on the GPU (model on {dev}, input_ids on {input_ids.device}); "
                             f"there is no CPU path; supported: {SUPPORTED}")
        if self.dtype != BF16:
            raise ValueError(f"orv_amd.t5: weights are {self.dtype}; supported: {SUPPORTED}")
        B, S = input_ids.shape
        if S < 1 or S > ops.t5_attention_max_seq():
            raise ValueError(f"orv_amd.t5: sequence length {S} is outside 1..{ops.t5_attention_max_seq()}; supported: {SUPPORTED}")
        if bool(((input_ids < 0) | (input_ids >= c.vocab_size)).any()):       # the one host read of a forward: the gather follows the ids
            raise ValueError(f"orv_amd.t5: input_ids outside [0, {c.vocab_size})")
        M, D, H, F, eps = B * S, c.d_model, c.num_heads, c.d_ff, float(c.layer_norm_epsilon)
        inner = H * c.d_kv
        ws = self._workspace(B, S, dev)
        bias = self._bias_rel(S, dev)
        x, h, qkv, att, ff, gg = ws["x"], ws["h"], ws["qkv"], ws["att"], ws["ff"], ws["gg"]
        ws["idx"].copy_(input_ids.reshape(-1))
        ops.gather_rows(self.shared.weight, ws["idx"], x, M, D)
        for i, blk in enumerate(self.encoder.block):
            sa, ffn = blk.layer[0], blk.layer[1]
            at, dd = sa.SelfAttention, ffn.DenseReluDense
            wqkv = _stacked(self._stacks, (i, "qkv"), (at.q.weight, at.k.weight, at.v.weight))
            wi = _stacked(self._stacks, (i, "wi"), (dd.wi_0.weight, dd.wi_1.weight))
            ops.t5_rmsnorm(x, sa.layer_norm.weight, h, M, D, eps)
            ops.gemm(h, wqkv, None, qkv, M, 3 * inner, D)
            ops.t5_attention_fwd(qkv, bias, att, B, S, H)
            ops.gemm(att, at.o.weight, None, x, M, D, inner, epilogue=2, R=x, ldr=D)
            ops.t5_rmsnorm(x, ffn.layer_norm.weight, h, M, D, eps)
            ops.gemm(h, wi, None, ff, M, 2 * F, D)
            ops.geglu(ff, gg, M, F)
            ops.gemm(gg, dd.wo.weight, None, x, M, D, F, epilogue=2, R=x, ldr=D)
        out = torch.empty(B, S, D, dtype=BF16, device=dev)
        ops.t5_rmsnorm(x, self.encoder.final_layer_norm.weight, out, M, D, eps)
        return T5EncoderOutput(out) if return_dict else (out,)
