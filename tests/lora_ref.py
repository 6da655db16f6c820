"""Reference helpers for the LoRA tests: random adapters, their state-dict form, and the merged weights W + c B A the fp32 oracle
(oracle/dit.py, unmodified) is run on."""
import math

import torch

TARGETS = ("to_q", "to_k", "to_v", "to_out.0")
FILE_NAME = "pytorch_lora_weights.safetensors"


def coefficient(r, lora_alpha, scale=1.0, use_rslora=False):
    return scale * lora_alpha / (math.sqrt(r) if use_rslora else r)


def sigma_for(r):
    """Standard deviation of the test adapters' A and B: the merged update c B A has entries ~ c sigma^2 sqrt(r), so sigma shrinks with
    r^(1/4) to keep the update (and the oracle's merged-vs-base separation, >= 1e-1 on both golden configs) at the r = 8, sigma = 0.2 size."""
    return 0.2 * (8.0 / r) ** 0.25


def module_names(num_layers, targets=TARGETS):
    return [f"transformer_blocks.{i}.attn1.{t}" for i in range(num_layers) for t in targets]


def random_adapter(cfg, r, sigma, seed=0, targets=TARGETS):
    """{module name: (A [r, D], B [D, r])}, both ~ N(0, sigma) rounded to bf16 (kept as fp32 tensors): nonzero B, so that no dA is zero."""
    D = cfg["num_attention_heads"] * cfg["attention_head_dim"]
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in module_names(cfg["num_layers"], targets):
        A = (sigma * torch.randn(r, D, generator=g)).to(torch.bfloat16).float()
        B = (sigma * torch.randn(D, r, generator=g)).to(torch.bfloat16).float()
        out[name] = (A, B)
    return out


def adapter_state_dict(adapter, prefix="transformer."):
    sd = {}
    for name, (A, B) in adapter.items():
        sd[f"{prefix}{name}.lora_A.weight"] = A.to(torch.bfloat16)
        sd[f"{prefix}{name}.lora_B.weight"] = B.to(torch.bfloat16)
    return sd


def merged_weights(w, adapter, c):
    """The oracle's state dict with W_eff = W + c B A (fp32; A and B may be autograd leaves)."""
    out = dict(w)
    for name, (A, B) in adapter.items():
        out[name + ".weight"] = w[name + ".weight"] + c * (B @ A)
    return out


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def oracle_forward(dit, cfg, extra, ins, sd):
    rope = (ins["rope_cos"], ins["rope_sin"]) if "rope_cos" in ins else None
    mask = torch.tensor(extra["mask"]) if "actions" in ins else None
    return dit.dit_forward(sd, cfg, ins["hidden_states"], ins["encoder_hidden_states"], ins["timestep"], actions=ins.get("actions"),
                           is_mask=mask, image_rotary_emb=rope)[0]


def model_inputs(extra, ins, dev):
    """(args, kwargs) of the HIP model's forward for a golden fixture."""
    bf = torch.bfloat16
    ctrl = {"actions": ins["actions"].to(dev)} if "actions" in ins else {}
    rope = (ins["rope_cos"].to(dev), ins["rope_sin"].to(dev)) if "rope_cos" in ins else None
    return ((ins["hidden_states"].to(dev, bf), ins["encoder_hidden_states"].to(dev, bf), ctrl, ins["timestep"].to(dev)),
            dict(image_rotary_emb=rope, return_dict=False))


def build_model(cls, cfg, extra, ins, w, dev=None):
    m = cls(**cfg)
    m.load_state_dict(w, strict=True)
    m = m.to(torch.bfloat16)
    if dev is not None:
        m = m.to(dev)
    if "actions" in ins:
        m.action_embed.forced_mask = torch.tensor(extra["mask"])
    return m.eval()


def load_adapter(model, adapter, r, lora_alpha, name="default", use_rslora=False):
    """Put a ``random_adapter`` into the model through the public surface: add_adapter fixes r and alpha, the loader copies the tensors."""
    model.add_adapter(r=r, lora_alpha=lora_alpha, use_rslora=use_rslora, adapter_name=name)
    model.load_lora_adapter(adapter_state_dict(adapter), adapter_name=name)
    return model
