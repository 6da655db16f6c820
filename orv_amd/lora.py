"""LoRA adapters on the four attention linears of ``transformer_blocks[i].attn1`` (to_q, to_k, to_v, to_out[0]).

The reference's forward carries the diffusers LoRA plumbing (``scale_lora_layers`` / ``attention_kwargs["scale"]``,
cogvideox_control.py:729-741, :938-940) and its train script a LoRA branch (train...sft.py:489-491); here the adapter arithmetic

    y = x W^T + b + c (x A^T) B^T,   A [r, in], B [out, r] bf16,   c = scale * lora_alpha / r   (/ sqrt(r) with use_rslora)

runs in HIP: the down-projection T = x A^T, the rank update, dT = c dY B and dx += dT A are ``orv_gemm_bf16`` launches on operands whose
rank is zero-padded to a multiple of 64 (cached copies; the padding is no parameter and stays zero, c is folded into the copy of B), and
the adapter weight gradients dB = c dY^T T, dA = dT^T X come from ``orv_gemm_tn_skinny_bf16``.

``LoraMixin`` is the host surface of ``CogVideoXTransformer3DModelTraj`` (peft / diffusers names; neither package is needed).  The adapter
tensors are ``nn.Parameter``s held by a child module that ``parameters()`` / ``.to()`` see and ``state_dict()`` / ``load_state_dict()`` /
``save_pretrained`` do not: a checkpoint of an adapted model is the base model's.
"""
from __future__ import annotations

import json
import math
import os
from collections import OrderedDict
from typing import Any, Dict, List, Optional

import torch
from torch import nn

from . import _state, ops

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634
TARGETS = ("to_q", "to_k", "to_v", "to_out.0")
LORA_WEIGHT_NAME = "pytorch_lora_weights.safetensors"
MAX_RANK = 128
_SUPPORTED = ("LoRA adapters are supported on the attention projections transformer_blocks[i].attn1.{to_q, to_k, to_v, to_out.0} only, "
              "with 1 <= r <= 128, lora_dropout = 0, no DoRA and one active adapter at a time")
_CONFIG_KEYS = ("r", "lora_alpha", "target_modules", "init_lora_weights", "use_rslora", "lora_dropout", "use_dora")


def _target_of(name: str) -> Optional[str]:
    """'to_q' / ... / 'to_out.0' for a target-module entry ('to_q', 'attn1.to_q', ...), None for anything else."""
    name = str(name)
    for t in TARGETS:
        if name == t or name.endswith("." + t):
            head = name[:-len(t)].rstrip(".")
            if head in ("", "attn1") or head.endswith(".attn1"):
                if "mv_blocks" in head:
                    return None
                return t
    return None


def parse_config(adapter_config=None, **kw) -> Dict[str, Any]:
    """peft ``LoraConfig`` fields from a duck-typed object / dict and keywords -> a validated plain dict."""
    cfg = dict(r=8, lora_alpha=8, target_modules=None, init_lora_weights=True, use_rslora=False, lora_dropout=0.0, use_dora=False)
    given = set()
    if adapter_config is not None:
        for k in _CONFIG_KEYS:
            if isinstance(adapter_config, dict):
                if k in adapter_config:
                    cfg[k] = adapter_config[k]; given.add(k)
            elif hasattr(adapter_config, k):
                cfg[k] = getattr(adapter_config, k); given.add(k)
    for k, v in kw.items():
        if k not in _CONFIG_KEYS:
            raise TypeError(f"add_adapter: unknown LoRA config field {k!r} (known: {', '.join(_CONFIG_KEYS)})")
        cfg[k] = v; given.add(k)
    r = cfg["r"]
    if not isinstance(r, int) or isinstance(r, bool) or not 1 <= r <= MAX_RANK:
        raise ValueError(f"LoRA rank r={r!r} is out of range: {_SUPPORTED}")
    if "lora_alpha" not in given:
        cfg["lora_alpha"] = r
    if cfg["lora_dropout"]:
        raise ValueError(f"lora_dropout={cfg['lora_dropout']} is not supported: {_SUPPORTED}")
    if cfg["use_dora"]:
        raise ValueError(f"use_dora (DoRA) is not supported: {_SUPPORTED}")
    tm = cfg["target_modules"]
    if tm is None:
        tm = list(TARGETS)
    if isinstance(tm, str):
        tm = [tm]
    targets = []
    for name in tm:
        t = _target_of(name)
        if t is None:
            raise ValueError(f"target module {name!r} is not supported (FeedForward and mv_blocks targets are out of scope): {_SUPPORTED}")
        if t not in targets:
            targets.append(t)
    if not targets:
        raise ValueError(f"target_modules is empty: {_SUPPORTED}")
    cfg["target_modules"] = [t for t in TARGETS if t in targets]
    cfg["lora_alpha"] = float(cfg["lora_alpha"])
    cfg["use_rslora"] = bool(cfg["use_rslora"])
    return cfg


class _AdapterStore(nn.Module):
    """Holds the adapter Parameters: visible to ``parameters()`` / ``.to()``, absent from ``state_dict()`` / ``load_state_dict()``."""

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        return destination if destination is not None else OrderedDict()

    def _load_from_state_dict(self, *args, **kwargs):
        return

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("_AdapterStore is a parameter container")


class _Adapter:
    def __init__(self, name, cfg):
        self.name = name
        self.r, self.lora_alpha, self.use_rslora = cfg["r"], cfg["lora_alpha"], cfg["use_rslora"]
        self.targets = list(cfg["target_modules"])
        self.rp = (self.r + 63) // 64 * 64           # rank as the GEMMs see it (zero padded)
        self.r16 = (self.r + 15) // 16 * 16          # rank as the skinny weight-gradient kernel sees it
        self.params: Dict[str, tuple] = {}           # "transformer_blocks.{i}.attn1.{target}" -> (A, B)
        self.cache: Dict[Any, Any] = {}

    def coefficient(self, scale=1.0):
        return float(scale) * self.lora_alpha / (math.sqrt(self.r) if self.use_rslora else self.r)

    def pname(self, module, which):
        return f"{self.name}__{module.replace('.', '__')}__{which}"


class _BlockWeights:
    """Padded operand copies of one block's adapter for one coefficient c (see ``LoraRuntime.block``)."""
    pass


class LoraRuntime:
    """The active adapter at one coefficient: per-block padded GEMM operands, cached per (parameter versions, weights epoch, c)."""

    def __init__(self, adapter: _Adapter, c: float):
        self.ad, self.c = adapter, c
        self.rp, self.r, self.r16 = adapter.rp, adapter.r, adapter.r16
        self.held = []       # every operand set handed out: a captured graph keeps its runtime, and with it these addresses, alive

    def block(self, i: int, train: bool = False) -> Optional[_BlockWeights]:
        ad = self.ad
        mods = [(t, ad.params.get(f"transformer_blocks.{i}.attn1.{t}")) for t in ad.targets]
        mods = [(t, ab) for t, ab in mods if ab is not None]
        if not mods:
            return None
        key = (i, self.c, bool(train), _state.weights_epoch[0]) + tuple((p.data_ptr(), p._version) for _, ab in mods for p in ab)
        hit = ad.cache.get((i, bool(train)))
        if hit is not None and hit[0] == key:
            self.held.append(hit[1])
            return hit[1]
        rp, r, c = self.rp, self.r, self.c
        bw = _BlockWeights()
        dev = mods[0][1][0].device
        D = mods[0][1][0].shape[1]

        def pad_a(A):                  # [r, D] -> [rp, D]
            out = torch.zeros(rp, A.shape[1], dtype=BF16, device=dev)
            out[:r] = A.detach()
            return out

        def pad_cb(B):                 # [out, r] -> bf16(c B) [out, rp]
            out = torch.zeros(B.shape[0], rp, dtype=BF16, device=dev)
            out[:, :r] = (B.detach().float() * c).to(BF16)
            return out
        qkv = [(j, t) for j, t in enumerate(TARGETS[:3]) if any(t == m for m, _ in mods)]
        byname = dict(mods)
        bw.qkv = [j for j, _ in qkv]
        bw.nT = len(qkv)
        bw.qkv_params = [byname[t] for _, t in qkv]
        if qkv:
            bw.Acat = torch.cat([pad_a(byname[t][0]) for _, t in qkv], dim=0).contiguous()            # [nT rp, D]
            bw.cB = [pad_cb(byname[t][1]) for _, t in qkv]                                             # [D, rp] each
            if train:
                bw.AcatT = bw.Acat.t().contiguous()                                                    # [D, nT rp]
                bw.cBT = [b.t().contiguous() for b in bw.cB]                                           # [rp, D] each
        bw.out_params = byname.get("to_out.0")
        if bw.out_params is not None:
            bw.oA = pad_a(bw.out_params[0])
            bw.ocB = pad_cb(bw.out_params[1])
            if train:
                bw.oAT = bw.oA.t().contiguous()
                bw.ocBT = bw.ocB.t().contiguous()
        bw.D = D
        ad.cache[(i, bool(train))] = (key, bw)
        self.held.append(bw)
        return bw


# ---- block arithmetic (HIP launches) -----------------------------------------------------------------------------------------------
def qkv_projection(at, bw, rt, xn, qkv, T, rope, B, S, heads, n_text, s_pad, scale, raw=None):
    """to_q / to_k / to_v with the adapter's rank update, then norm_q / norm_k (+ RoPE): the plain projection (epilogue 0) into the raw
    buffer, T = xn Acat^T, raw[:, third j] += T_j (c B_j)^T (epilogue 2, R == C), ``orv_qkv_prep``.  The qk LayerNorm is nonlinear: the
    fused epilogue 4 cannot be used while an adapter is active."""
    D = heads * 64
    M = B * S
    rp = rt.rp
    wqkv, bqkv = at.packed_qkv()
    nq, nk = at.norm_q, at.norm_k
    dst = qkv if raw is None else raw
    ops.gemm(xn, wqkv, bqkv, dst, M, 3 * D, D)
    if bw.nT:
        W = bw.nT * rp
        ops.gemm(xn, bw.Acat, None, T, M, W, D)
        for slot, j in enumerate(bw.qkv):
            cj = dst[:, j * D:]
            ops.gemm(T[:, slot * rp:], bw.cB[slot], None, cj, M, D, rp, epilogue=2, R=cj, lda=W, ldc=3 * D, ldr=3 * D)
    ops.qkv_prep(qkv, None, nq.weight, nq.bias, nk.weight, nk.bias, rope, B, S, heads, n_text, s_pad, at.eps,
                 q_premul=scale * LOG2E, src=raw)


def out_update(bw, rt, att, To, x_in, x_out, M, D, gate, gate_b, gate_g, grp, Y=None):
    """x_out = x_in + gate * c (att A^T) B^T - the adapter's share of the gated out-projection residual, run BEFORE the unchanged base launch."""
    rp = rt.rp
    ops.gemm(att, bw.oA, None, To, M, rp, D)
    ops.gemm(To, bw.ocB, None, x_out, M, D, rp, epilogue=2, R=x_in, ldr=D, gate=gate, gate_b=gate_b, gate_g=gate_g, grp=grp, Y=Y, ldy=D)


def _grad_dest(param, grads, rows, cols, dev):
    """(destination [rows, cols] bf16, ld, accumulate, finish()) of an adapter weight gradient whose kernel shape (rank rounded up to 16)
    may exceed the parameter's: the optimizer's segment / a fresh tensor directly when the shapes agree, else a temporary + slice copy."""
    exact = tuple(param.shape) == (rows, cols)
    if id(param) in grads:
        g = grads[id(param)]
        if exact and g.is_contiguous() and g.data_ptr() % 16 == 0:
            return g, True, (lambda t: None)
        tmp = torch.empty(rows, cols, dtype=BF16, device=dev)
        return tmp, False, (lambda t: g.add_(t[:param.shape[0], :param.shape[1]]))
    g = _state.grad_view(param)
    if g is None:
        g = torch.empty_like(param, dtype=BF16)
    grads[id(param)] = g
    if exact and g.is_contiguous() and g.data_ptr() % 16 == 0:
        return g, False, (lambda t: None)
    tmp = torch.empty(rows, cols, dtype=BF16, device=dev)
    return tmp, False, (lambda t: g.copy_(t[:param.shape[0], :param.shape[1]]))


def linear_backward(rt, params, dY, ldy, T, ldt, X, ldx, cBT, dT, lddt, M, D_out, D_in, grads):
    """Adjoint of one adapted linear's low-rank branch, given dY [M, D_out] (row stride ldy), the saved T = X A^T [M, rp] (stride ldt) and
    the layer input X [M, D_in]: dT = dY (c B) into ``dT`` (stride lddt), dB = c dY^T T and dA = dT^T X by the skinny kernel.  The caller
    adds dT A into its dX (one GEMM for all of a block's q / k / v adapters)."""
    A, Bp = params
    rp, r16 = rt.rp, rt.r16
    dev = dY.device
    ops.gemm(dY, cBT, None, dT, M, rp, D_out, lda=ldy, ldc=lddt)
    if Bp.requires_grad:
        dst, acc, fin = _grad_dest(Bp, grads, D_out, r16, dev)
        ops.gemm_tn_skinny(dY, T, dst, M, D_out, r16, alpha=rt.c, accumulate=acc, ldu=ldy, ldv=ldt, ldc=r16)
        fin(dst)
    if A.requires_grad:
        dst, acc, fin = _grad_dest(A, grads, r16, D_in, dev)
        ops.gemm_tn_skinny(dT, X, dst, M, r16, D_in, alpha=1.0, accumulate=acc, ldu=lddt, ldv=ldx, ldc=D_in)
        fin(dst)


# ---- host surface ----------------------------------------------------------------------------------------------------------------------
class LoraMixin:
    """peft / diffusers adapter surface of ``CogVideoXTransformer3DModelTraj``."""

    def _lora_init(self):
        self._lora_adapters: Dict[str, _Adapter] = OrderedDict()
        self._lora_active: Optional[str] = None
        self._lora_enabled = True
        self._lora_fused = None          # (adapter name, lora_scale, {module name: original bf16 weight}) while fused
        self._lora_gen = 0               # bumped by every structural change: part of GraphedTransformer's key

    # -- queries --
    @property
    def active_adapter(self) -> Optional[str]:
        return self._lora_active

    def active_adapters(self) -> List[str]:
        return [self._lora_active] if self._lora_active is not None else []

    def _lora_runtime(self, scale: float = 1.0) -> Optional[LoraRuntime]:
        """The adapter the forward has to run, or None (no adapter, disabled, deleted, fused: today's code path)."""
        if self._lora_active is None or not self._lora_enabled or self._lora_fused is not None:
            return None
        ad = self._lora_adapters[self._lora_active]
        return LoraRuntime(ad, ad.coefficient(scale))

    def _lora_cached_operands(self):
        """The padded operand copies of the active adapter that the last forward read (``LoraRuntime.block``'s cache), or None without
        an adapter on the forward path: a captured graph keeps them alive after the cache entries are replaced."""
        if self._lora_runtime() is None:
            return None
        return [bw for _, bw in self._lora_adapters[self._lora_active].cache.values()]

    def _lora_key(self, scale: float = 1.0):
        return (self._lora_gen, self._lora_active, self._lora_enabled, self._lora_fused is not None and self._lora_fused[:2], float(scale))

    def _lora_linear(self, module_name: str) -> nn.Linear:
        parts = module_name.split(".")          # transformer_blocks.{i}.attn1.{to_q | to_out.0}
        at = self.transformer_blocks[int(parts[1])].attn1
        return at.to_out[0] if parts[3] == "to_out" else getattr(at, parts[3])

    # -- construction --
    def add_adapter(self, adapter_config=None, adapter_name: str = "default", **kw):
        """peft ``add_adapter``: ``adapter_config`` is any object or dict with ``r``, ``lora_alpha``, ``target_modules``,
        ``init_lora_weights``, ``use_rslora``, ``lora_dropout``, ``use_dora`` (the same names work as keywords).  A is initialised with
        ``kaiming_uniform_(a=sqrt(5))``, B with zeros (``init_lora_weights=False``: B ~ N(0, 0.02) as peft's test mode); every base parameter
        is frozen, the adapter tensors are the only trainable parameters.  The new adapter becomes the active one."""
        cfg = parse_config(adapter_config, **kw)
        if adapter_name in self._lora_adapters:
            raise ValueError(f"adapter {adapter_name!r} already exists: delete_adapter({adapter_name!r}) first")
        if self._lora_fused is not None:
            raise RuntimeError("an adapter is fused into the weights: unfuse_lora() before adding another one")
        if "__" in adapter_name or "." in adapter_name:
            raise ValueError("adapter names may not contain '.' or '__'")
        if getattr(self, "_mxfp8", False):
            raise RuntimeError("MXFP8 mode runs fused adapters only: enable_mxfp8(False) first, or add the adapter and fuse_lora() before "
                               "enable_mxfp8()")
        ad = _Adapter(adapter_name, cfg)
        if not hasattr(self, "_lora_store"):
            self._lora_base_requires_grad = [(p, p.requires_grad) for p in self.parameters()]     # given back by the last delete_adapter
            self._lora_store = _AdapterStore()
        ref = self.transformer_blocks[0].attn1.to_q.weight if len(self.transformer_blocks) else None
        for i, blk in enumerate(self.transformer_blocks):
            for t in ad.targets:
                name = f"transformer_blocks.{i}.attn1.{t}"
                lin = self._lora_linear(name)
                A = torch.empty(ad.r, lin.in_features, dtype=torch.float32)
                nn.init.kaiming_uniform_(A, a=math.sqrt(5))
                B = torch.zeros(lin.out_features, ad.r, dtype=torch.float32)
                if cfg["init_lora_weights"] is False:
                    nn.init.normal_(B, std=0.02)
                pa = nn.Parameter(A.to(device=ref.device, dtype=ref.dtype))
                pb = nn.Parameter(B.to(device=ref.device, dtype=ref.dtype))
                self._lora_store.register_parameter(ad.pname(name, "A"), pa)
                self._lora_store.register_parameter(ad.pname(name, "B"), pb)
                ad.params[name] = (pa, pb)
        self._lora_adapters[adapter_name] = ad
        self._lora_active = adapter_name
        self._lora_enabled = True
        self._lora_gen += 1
        self._lora_freeze()
        return self

    def _lora_freeze(self):
        own = {id(p) for ad in self._lora_adapters.values() for ab in ad.params.values() for p in ab}
        for p in self.parameters():
            if id(p) not in own:
                p.requires_grad_(False)
        for name, ad in self._lora_adapters.items():
            for ab in ad.params.values():
                for p in ab:
                    p.requires_grad_(name == self._lora_active)

    def set_adapter(self, adapter_name):
        if isinstance(adapter_name, (list, tuple)):
            if len(adapter_name) != 1:
                raise ValueError(f"set_adapter: more than one active adapter at a time is not supported: {_SUPPORTED}")
            adapter_name = adapter_name[0]
        if adapter_name not in self._lora_adapters:
            raise ValueError(f"set_adapter: no adapter named {adapter_name!r} (have: {list(self._lora_adapters)})")
        if self._lora_fused is not None:
            raise RuntimeError("an adapter is fused into the weights: unfuse_lora() before switching")
        self._lora_active = adapter_name
        self._lora_gen += 1
        self._lora_freeze()

    def disable_adapters(self):
        self._lora_enabled = False
        self._lora_gen += 1

    def enable_adapters(self):
        if getattr(self, "_mxfp8", False) and self._lora_active is not None and self._lora_fused is None:
            raise RuntimeError("MXFP8 mode runs fused adapters only: fuse_lora() or enable_mxfp8(False) first")
        self._lora_enabled = True
        self._lora_gen += 1

    def delete_adapter(self, adapter_name: str):
        if adapter_name not in self._lora_adapters:
            raise ValueError(f"delete_adapter: no adapter named {adapter_name!r}")
        if self._lora_fused is not None and self._lora_fused[0] == adapter_name:
            raise RuntimeError(f"adapter {adapter_name!r} is fused into the weights: unfuse_lora() first")
        ad = self._lora_adapters.pop(adapter_name)
        for name in ad.params:
            for which in ("A", "B"):
                delattr(self._lora_store, ad.pname(name, which))
        _state.param_epoch[0] += 1
        if self._lora_active == adapter_name:
            self._lora_active = next(iter(self._lora_adapters), None)
        self._lora_gen += 1
        if not self._lora_adapters:
            del self._lora_store
            for p, flag in self.__dict__.pop("_lora_base_requires_grad"):       # trainable again as before the first add_adapter
                p.requires_grad_(flag)
        else:
            self._lora_freeze()

    # -- (de)serialisation --
    def get_adapter_state_dict(self, adapter_name: str = "default") -> Dict[str, torch.Tensor]:
        """peft-style keys without a prefix: ``transformer_blocks.{i}.attn1.{to_q|to_k|to_v|to_out.0}.lora_{A|B}.weight``."""
        if adapter_name not in self._lora_adapters:
            raise ValueError(f"no adapter named {adapter_name!r}")
        sd = OrderedDict()
        for name, (A, B) in self._lora_adapters[adapter_name].params.items():
            sd[f"{name}.lora_A.weight"] = A.detach()
            sd[f"{name}.lora_B.weight"] = B.detach()
        return sd

    def save_lora_adapter(self, save_directory, adapter_name: str = "default", prefix: str = "transformer", state_dict=None):
        """``state_dict``: the tensors to write in place of ``get_adapter_state_dict(adapter_name)`` (same keys; orv_amd.train_state passes
        the copies its snapshot took)."""
        from safetensors.torch import save_file
        ad = self._lora_adapters.get(adapter_name)
        if ad is None:
            raise ValueError(f"no adapter named {adapter_name!r}")
        os.makedirs(save_directory, exist_ok=True)
        pre = prefix + "." if prefix else ""
        own = self.get_adapter_state_dict(adapter_name) if state_dict is None else state_dict
        sd = {pre + k: v.detach().to("cpu").contiguous() for k, v in own.items()}
        meta = {"format": "pt", "lora_adapter_metadata": json.dumps(
            {"r": ad.r, "lora_alpha": ad.lora_alpha, "use_rslora": ad.use_rslora, "target_modules": ad.targets}, sort_keys=True)}
        path = os.path.join(save_directory, LORA_WEIGHT_NAME)
        save_file(sd, path, metadata=meta)
        return path

    def load_lora_adapter(self, path_or_state_dict, adapter_name: str = "default", prefix: Optional[str] = "transformer"):
        """Loads ``pytorch_lora_weights.safetensors`` (a directory, the file, or a state dict).  ``lora_alpha`` comes from the file's
        ``lora_adapter_metadata`` entry when present, else from per-module ``.alpha`` scalars, else it equals the rank.  Into an existing
        adapter of the same geometry the tensors are copied in place (``_version``-keyed caches and graphs see it)."""
        sd, meta = read_lora_file(path_or_state_dict)
        pre = prefix + "." if prefix else ""
        mods: Dict[str, Dict[str, torch.Tensor]] = {}
        alphas = {}
        for k, v in sd.items():
            k2 = k[len(pre):] if pre and k.startswith(pre) else k
            for suf, slot in ((".lora_A.weight", "A"), (".lora_B.weight", "B"), (".lora_A.default.weight", "A"), (".lora_B.default.weight", "B")):
                if k2.endswith(suf):
                    mods.setdefault(k2[:-len(suf)], {})[slot] = v
                    break
            else:
                if k2.endswith(".alpha"):
                    alphas[k2[:-len(".alpha")]] = float(v)
                else:
                    raise ValueError(f"load_lora_adapter: unexpected key {k!r}: {_SUPPORTED}")
        if not mods:
            raise ValueError("load_lora_adapter: no lora_A / lora_B tensors found")
        L = len(self.transformer_blocks)
        targets, r = [], None
        for name, ab in mods.items():
            parts = name.split(".")
            t = ".".join(parts[3:])
            ok = (len(parts) >= 4 and parts[0] == "transformer_blocks" and parts[1].isdigit() and int(parts[1]) < L and parts[2] == "attn1"
                  and t in TARGETS)
            if not ok:
                raise ValueError(f"load_lora_adapter: {name!r} is not an adapted module of this model: {_SUPPORTED}")
            if "A" not in ab or "B" not in ab:
                raise ValueError(f"load_lora_adapter: {name!r} needs both lora_A and lora_B")
            lin = self._lora_linear(name)
            ra = ab["A"].shape[0]
            if tuple(ab["A"].shape) != (ra, lin.in_features) or tuple(ab["B"].shape) != (lin.out_features, ra):
                raise ValueError(f"load_lora_adapter: {name!r} has shapes {tuple(ab['A'].shape)} / {tuple(ab['B'].shape)}")
            if r is None:
                r = ra
            elif r != ra:
                raise ValueError("load_lora_adapter: one rank per adapter (rank patterns are not supported)")
            if t not in targets:
                targets.append(t)
        for t in targets:
            for i in range(L):
                if f"transformer_blocks.{i}.attn1.{t}" not in mods:
                    raise ValueError(f"load_lora_adapter: transformer_blocks.{i}.attn1.{t} is missing (every block carries the same targets)")
        alpha, rslora = float(r), False
        if alphas:
            vals = set(alphas.values())
            if len(vals) != 1:
                raise ValueError("load_lora_adapter: per-module alphas differ (alpha patterns are not supported)")
            alpha = vals.pop()
        if meta and meta.get("lora_adapter_metadata"):
            m = json.loads(meta["lora_adapter_metadata"])
            alpha, rslora = float(m.get("lora_alpha", alpha)), bool(m.get("use_rslora", False))
            if int(m.get("r", r)) != r:
                raise ValueError(f"load_lora_adapter: metadata rank {m.get('r')} does not match the tensors' rank {r}")
        ad = self._lora_adapters.get(adapter_name)
        if ad is not None and (ad.r != r or set(ad.targets) != set(targets)):
            raise ValueError(f"adapter {adapter_name!r} exists with another geometry: delete_adapter({adapter_name!r}) first")
        if ad is None:
            self.add_adapter(dict(r=r, lora_alpha=alpha, use_rslora=rslora, target_modules=targets), adapter_name=adapter_name)
            ad = self._lora_adapters[adapter_name]
        else:
            if self._lora_fused is not None:
                raise RuntimeError("an adapter is fused into the weights: unfuse_lora() before loading")
            if alphas or (meta and meta.get("lora_adapter_metadata")):       # a file that states no alpha keeps the adapter's own
                ad.lora_alpha, ad.use_rslora = alpha, rslora
            self._lora_gen += 1
        with torch.no_grad():
            for name, ab in mods.items():
                A, B = ad.params[name]
                A.copy_(ab["A"].to(device=A.device, dtype=A.dtype))
                B.copy_(ab["B"].to(device=B.device, dtype=B.dtype))
        return self

    # -- merging --
    def fuse_lora(self, lora_scale: float = 1.0, adapter_name: Optional[str] = None):
        """W <- bf16(fp32(W) + c B A) for every adapted linear (fp32 arithmetic, in-place ``copy_``).  The original weights are kept, so
        ``unfuse_lora()`` restores them bit for bit.  While fused the adapter path is off: the forward is the default path."""
        if self._lora_fused is not None:
            raise RuntimeError("an adapter is already fused: unfuse_lora() first")
        name = adapter_name or self._lora_active
        if name is None or name not in self._lora_adapters:
            raise ValueError("fuse_lora: no adapter to fuse")
        ad = self._lora_adapters[name]
        c = ad.coefficient(lora_scale)
        saved = {}
        with torch.no_grad():
            for mod, (A, B) in ad.params.items():
                w = self._lora_linear(mod).weight
                saved[mod] = w.detach().clone()
                w.copy_((w.float() + c * (B.float() @ A.float())).to(w.dtype))
        self._lora_fused = (name, float(lora_scale), saved)
        self._lora_gen += 1
        return self

    def unfuse_lora(self):
        if self._lora_fused is None:
            return self
        with torch.no_grad():
            for mod, w0 in self._lora_fused[2].items():
                w = self._lora_linear(mod).weight
                w.copy_(w0.to(device=w.device, dtype=w.dtype))
        self._lora_fused = None
        self._lora_gen += 1
        return self


def read_lora_file(path_or_state_dict):
    """-> (state dict, metadata or None) of a LoRA file / directory / state dict."""
    if isinstance(path_or_state_dict, dict):
        return dict(path_or_state_dict), None
    from safetensors import safe_open
    path = str(path_or_state_dict)
    if os.path.isdir(path):
        path = os.path.join(path, LORA_WEIGHT_NAME)
    sd = {}
    with safe_open(path, framework="pt") as f:
        meta = f.metadata()
        for k in f.keys():
            sd[k] = f.get_tensor(k)
    return sd, meta
