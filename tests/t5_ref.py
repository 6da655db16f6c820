"""Plain-torch restatement of the T5 v1.1 encoder (transformers' ``T5Stack`` in eval mode, ``attention_mask=None``): the reference of the
T5 tests.  Works on a transformers-format state dict; imports neither ``orv_amd`` nor ``transformers``.  ``dtype=torch.bfloat16`` runs the
same graph with transformers' bf16 rounding points (the accuracy yardstick of the GPU tests)."""
import math

import torch


def tiny_config(d_model=128, num_heads=2, d_ff=128, num_layers=2, vocab_size=64, d_kv=64):
    """A T5 v1.1 encoder config with transformers' field names."""
    return {"architectures": ["T5EncoderModel"], "model_type": "t5", "d_model": d_model, "d_kv": d_kv, "num_heads": num_heads, "d_ff": d_ff,
            "num_layers": num_layers, "vocab_size": vocab_size, "feed_forward_proj": "gated-gelu", "relative_attention_num_buckets": 32,
            "relative_attention_max_distance": 128, "layer_norm_epsilon": 1e-6, "tie_word_embeddings": False, "dropout_rate": 0.1,
            "is_encoder_decoder": False, "use_cache": False}


def relative_position_bucket(rel, num_buckets=32, max_distance=128):
    """T5's bidirectional bucket of ``rel = key position - query position`` (an integer tensor)."""
    nb = num_buckets // 2
    out = (rel > 0).long() * nb
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).long()
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(n < max_exact, n, large)


def position_bias(table, S, num_buckets=32, max_distance=128):
    """[H, S, S]: bias[h, i, j] = table[bucket(j - i), h] (table is relative_attention_bias.weight, [num_buckets, H])."""
    pos = torch.arange(S, device=table.device)
    bucket = relative_position_bucket(pos[None, :] - pos[:, None], num_buckets, max_distance)
    return table[bucket].permute(2, 0, 1)


def rms(x, w, eps):
    y = x * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)          # fp32
    if w.dtype in (torch.float16, torch.bfloat16):
        y = y.to(w.dtype)
    return w * y


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def encode(state, cfg, ids, dtype=torch.float32):
    """last_hidden_state [B, S, d_model] in ``dtype``."""
    w = {k: v.to(dtype) for k, v in state.items()}
    H, dk, eps = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"]
    B, S = ids.shape
    x = w["shared.weight"][ids]
    bias = position_bias(w["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], S,
                         cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"])
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        h = rms(x, w[p + "0.layer_norm.weight"], eps)
        q, k, v = ((h @ w[p + f"0.SelfAttention.{n}.weight"].T).view(B, S, H, dk).transpose(1, 2) for n in "qkv")
        s = q @ k.transpose(-1, -2) + bias                                       # no 1 / sqrt(d) scale
        a = torch.softmax(s.float(), dim=-1).to(s.dtype)
        x = x + (a @ v).transpose(1, 2).reshape(B, S, H * dk) @ w[p + "0.SelfAttention.o.weight"].T
        h = rms(x, w[p + "1.layer_norm.weight"], eps)
        g = gelu_new(h @ w[p + "1.DenseReluDense.wi_0.weight"].T) * (h @ w[p + "1.DenseReluDense.wi_1.weight"].T)
        x = x + g @ w[p + "1.DenseReluDense.wo.weight"].T
    return rms(x, w["encoder.final_layer_norm.weight"], eps)


def state_keys(cfg):
    """transformers' T5EncoderModel.state_dict() key order."""
    keys = ["shared.weight", "encoder.embed_tokens.weight"]
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        keys += [p + f"0.SelfAttention.{n}.weight" for n in "qkvo"]
        if i == 0:
            keys.append(p + "0.SelfAttention.relative_attention_bias.weight")
        keys.append(p + "0.layer_norm.weight")
        keys += [p + f"1.DenseReluDense.{n}.weight" for n in ("wi_0", "wi_1", "wo")]
        keys.append(p + "1.layer_norm.weight")
    keys.append("encoder.final_layer_norm.weight")
    return keys


def make_state(cfg, seed=0):
    """Seeded weights, fp32 tensors holding bf16-representable values: q ~ N(0, (2 (d_model d_kv)^-0.5)^2) (score std about 2),
    k / v / o / wi ~ N(0, 1 / d_model), wo ~ N(0, 1 / d_ff), norm gains 1 + 0.1 N(0, 1), embedding and bias table N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    D, dk, H, dff = cfg["d_model"], cfg["d_kv"], cfg["num_heads"], cfg["d_ff"]
    inner = H * dk
    r = lambda *shape: torch.randn(*shape, generator=g)
    st = {}
    for key in state_keys(cfg):
        leaf = key.split(".")[-2]
        if key == "shared.weight":
            t = r(cfg["vocab_size"], D)
        elif key == "encoder.embed_tokens.weight":
            t = st["shared.weight"].clone()
        elif leaf == "q":
            t = r(inner, D) * (2.0 * (D * dk) ** -0.5)
        elif leaf in ("k", "v"):
            t = r(inner, D) * D ** -0.5
        elif leaf == "o":
            t = r(D, inner) * D ** -0.5
        elif leaf in ("wi_0", "wi_1"):
            t = r(dff, D) * D ** -0.5
        elif leaf == "wo":
            t = r(D, dff) * dff ** -0.5
        elif leaf == "relative_attention_bias":
            t = r(cfg["relative_attention_num_buckets"], H)
        else:                                                                     # layer_norm / final_layer_norm
            t = 1.0 + 0.1 * r(D)
        st[key] = t.bfloat16().float()
    return st


def make_ids(cfg, B, S, seed=1):
    return torch.randint(0, cfg["vocab_size"], (B, S), generator=torch.Generator().manual_seed(seed))


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def load_tiny():
    """tests/golden/t5_tiny.safetensors (tools/make_t5_golden.py) -> (config, state_dict key order, weights fp32, input_ids, transformers'
    fp32 output)."""
    import json
    import os
    from safetensors import safe_open
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_tiny.safetensors")
    with safe_open(path, framework="pt") as f:
        meta = f.metadata()
        keys = json.loads(meta["keys"])
        state = {k: f.get_tensor("w." + k).float() for k in keys}
        return json.loads(meta["config"]), keys, state, f.get_tensor("input_ids"), f.get_tensor("output")
