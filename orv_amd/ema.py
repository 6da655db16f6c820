"""Exponential moving average (EMA) of the trainable weights, kept on the flat buffers of the fused optimizers.

Diffusion fine-tuning samples from an average of the weights, usually through ``diffusers.training_utils.EMAModel`` (the module the
reference's train script imports its helpers from).  That class keeps its shadow in the parameters' dtype, and the parameters here are bf16:
at ``decay = 0.9999`` one update moves the shadow by ``1e-4 (s - p)``, far below half a bf16 grid step of ``s``, so a bf16 shadow never
moves (tests/test_ema_host.py shows the stall).  ``FusedEMA`` therefore keeps

* ONE fp32 shadow buffer in the segment layout of the optimizer's flat parameter buffer (``offs``, segments padded to 2048, padding zero):
  +4 bytes per trainable parameter;
* as its input the exact fp32 master ``p | lo`` where the optimizer keeps one (``param_precision="split_fp32"``, ``FusedProdigy``), the
  bf16 weight otherwise

and updates it with one streaming launch per step (``orv_ema_update``, orv_amd/csrc/optim_ema.hip):

    s <- s - fp32(1 - decay) * (s - theta)              three fp32 operations, each rounded on its own

Method names and semantics follow ``EMAModel`` (``get_decay``, ``step``, ``store``, ``copy_to``, ``restore``, ``state_dict`` keys), restated
from memory and NOT pinned: diffusers is not available to compare against.  Differences: the constructor takes the fused optimizer, not a
parameter list; ``step()`` takes no arguments; ``store`` / ``copy_to`` / ``restore`` act on the optimizer's own parameters.

There is no data-parallel collective: the shadow is a function of (weights, step count) only, the weights are identical on every rank after
each optimizer step, so the ranks' shadows agree by construction.
"""
from __future__ import annotations

import contextlib
import struct
from typing import Dict

import torch

from . import _state, ops
from .optim import FusedAdamW

_INIT_CHUNK = 64 * 1024 * 1024      # elements per piece of the one-time shadow initialisation (bounds its int32 temporaries to 2 x 256 MB)


def _f32(x: float) -> float:
    """The fp32 value nearest to the host double ``x`` (what the C ABI's ``float`` argument receives), as a Python float."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


class FusedEMA:
    def __init__(self, optimizer, decay: float = 0.9999, min_decay: float = 0.0, update_after_step: int = 0, use_ema_warmup: bool = False,
                 inv_gamma: float = 1.0, power: float = 2 / 3):
        if not isinstance(optimizer, FusedAdamW):
            raise TypeError(f"FusedEMA: optimizer is a {type(optimizer).__name__}; the shadow lives in the flat layout of FusedAdamW / "
                            "FusedProdigy / FusedCAME (construct one of them over the trainable parameters first)")
        if not optimizer.params:
            raise ValueError("FusedEMA: the optimizer owns no trainable parameter")
        if not 0.0 <= float(decay) <= 1.0 or not 0.0 <= float(min_decay) <= 1.0:
            raise ValueError(f"FusedEMA: decay={decay}, min_decay={min_decay} must lie in [0, 1]")
        if not float(inv_gamma) > 0:
            raise ValueError(f"FusedEMA: inv_gamma={inv_gamma} must be greater than 0")
        self.optimizer = optimizer
        self.decay, self.min_decay = float(decay), float(min_decay)
        self.update_after_step, self.use_ema_warmup = int(update_after_step), bool(use_ema_warmup)
        self.inv_gamma, self.power = float(inv_gamma), float(power)
        self.optimization_step = 0
        self.cur_decay_value = None          # the decay of the last step(), for logging (EMAModel's attribute)
        self._stash = None                   # (p copy, lo copy or None) between store() and restore()
        if optimizer._flat is None:
            optimizer._build()
        f = self._buffers()
        if "lo" in f:
            optimizer._drop_stale_param_lo()
        # one-time initialisation, exact (signed zeros included): shadow bits = the master's, (p_bits << 16) + sign_extend(lo)
        n = f["p"].numel()
        self.shadow = torch.empty(n, dtype=torch.float32, device=f["p"].device)
        for a in range(0, n, _INIT_CHUNK):
            b = min(n, a + _INIT_CHUNK)
            bits = f["p"][a:b].float().view(torch.int32)          # bf16 -> fp32 is exact: the pattern shifted up by 16
            if "lo" in f:
                bits += f["lo"][a:b].to(torch.int32)
            self.shadow[a:b] = bits.view(torch.float32)

    def _buffers(self):
        f = self.optimizer._flat
        if getattr(self, "_p_buffer", None) is None:
            self._p_buffer = f["p"]
        elif f is None or f["p"] is not self._p_buffer:
            raise RuntimeError("FusedEMA: the optimizer's flat parameter buffer was rebuilt; the shadow's layout belongs to the old one")
        return f

    # ---- the decay schedule (host float64) ----
    def get_decay(self, optimization_step: int) -> float:
        step = max(0, int(optimization_step) - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            value = 1.0 - (1.0 + step / self.inv_gamma) ** -self.power
        else:
            value = (1.0 + step) / (10.0 + step)
        return max(min(value, self.decay), self.min_decay)

    # ---- the update ----
    @torch.no_grad()
    def step(self):
        """Call after ``optimizer.step()``: one launch over the whole flat buffer."""
        if self._stash is not None:
            raise RuntimeError("FusedEMA.step: the averaged weights are swapped in (store() without restore()): the optimizer would have "
                               "updated the average itself and restore() would then discard that update - call restore() before training on")
        f = self._buffers()
        if "lo" in f:
            self.optimizer._drop_stale_param_lo()
        self.optimization_step += 1
        d = self.get_decay(self.optimization_step)
        self.cur_decay_value = d
        ops.ema_update(self.shadow, f["p"], f.get("lo"), _f32(1.0 - d))

    # ---- the weight swap for evaluation ----
    def _swap_in(self, keep: bool):
        f = self._buffers()
        lo = f.get("lo")
        if keep:
            if lo is not None:
                self.optimizer._drop_stale_param_lo()
            stash = (torch.empty_like(f["p"]), None if lo is None else torch.empty_like(lo))
            ops.ema_swap_in(f["p"], self.shadow, lo, stash_p=stash[0], stash_lo=stash[1], zero_lo=False)
            self._stash = stash
        else:
            # outside a store() / restore() pair the written value becomes the weight for good: its master is that value, lo = 0
            ops.ema_swap_in(f["p"], self.shadow, lo, zero_lo=lo is not None and self._stash is None)
        _state.bump_weights_epoch()

    def _refuse_second_store(self):
        if self._stash is not None:
            raise RuntimeError("FusedEMA.store: a stash is already held (store() without restore()): a second store() would keep the "
                               "swapped-in averages and lose the training weights - call restore() first")

    @torch.no_grad()
    def store(self):
        """Stash the training weights (``p``, and ``lo`` where the optimizer keeps masters) for ``restore()``."""
        self._refuse_second_store()
        f = self._buffers()
        if "lo" in f:
            self.optimizer._drop_stale_param_lo()
        self._stash = (f["p"].clone(), f["lo"].clone() if "lo" in f else None)
        _state.bump_weights_epoch()

    @torch.no_grad()
    def copy_to(self):
        """Write ``bf16_rne(shadow)`` into the optimizer's parameters (the model reads them in place).  Outside a ``store()`` / ``restore()``
        pair the low halves are zeroed too, so that the master equals the written value."""
        self._swap_in(keep=False)

    @torch.no_grad()
    def restore(self):
        """Put the stashed training weights back, bit for bit, and free the stash."""
        if self._stash is None:
            raise RuntimeError("FusedEMA.restore: nothing is stashed (call store() first)")
        f = self._buffers()
        f["p"].copy_(self._stash[0])
        if self._stash[1] is not None:
            f["lo"].copy_(self._stash[1])
        self._stash = None
        _state.bump_weights_epoch()

    @contextlib.contextmanager
    def average_parameters(self):
        """``store()`` + ``copy_to()`` going in (ONE launch), ``restore()`` going out."""
        self._refuse_second_store()
        with torch.no_grad():
            self._swap_in(keep=True)
        try:
            yield self
        finally:
            self.restore()

    def save_pretrained(self, model, directory, **kwargs):
        """``model.save_pretrained(directory)`` on the averaged weights; the training weights are back afterwards."""
        with self.average_parameters():
            model.save_pretrained(directory, **kwargs)

    # ---- views and checkpoints ----
    def shadow_tensors(self) -> Dict[torch.nn.Parameter, torch.Tensor]:
        """``{parameter: fp32 view of its shadow}`` (shaped like the parameter, aliasing the flat shadow buffer)."""
        f = self._buffers()
        return {p: self.shadow[o:o + p.numel()].view(p.shape) for p, o in zip(self.optimizer.params, f["offs"])}

    def state_dict(self):
        """``EMAModel``'s keys - ``shadow_params`` is the list of fp32 shadows in ``optimizer.params`` order (views, not copies) - plus
        ``shapes``, the parameter shapes in that order, so that a different flat order is refused on load."""
        return {"decay": self.decay, "min_decay": self.min_decay, "optimization_step": self.optimization_step,
                "update_after_step": self.update_after_step, "use_ema_warmup": self.use_ema_warmup, "inv_gamma": self.inv_gamma,
                "power": self.power, "shadow_params": list(self.shadow_tensors().values()),
                "shapes": [list(p.shape) for p in self.optimizer.params]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        shapes = [list(p.shape) for p in self.optimizer.params]
        shadows = sd.get("shadow_params")
        have = [list(s) for s in sd["shapes"]] if sd.get("shapes") is not None else (None if shadows is None else [list(t.shape) for t in shadows])
        if have is not None and have != shapes:
            if sorted(have) == sorted(shapes):
                raise ValueError("FusedEMA.load_state_dict: same parameters, another flat-buffer ORDER - the shadows are stored by position in "
                                 "optimizer.params and cannot be mapped; build the optimizer over the parameters in the order that wrote the "
                                 "checkpoint")
            raise ValueError("FusedEMA.load_state_dict: the checkpoint was written for a different set of trainable parameters "
                             f"({len(have)} shadows vs {len(shapes)} here, or different shapes)")
        for key, cast in (("decay", float), ("min_decay", float), ("optimization_step", int), ("update_after_step", int),
                          ("use_ema_warmup", bool), ("inv_gamma", float), ("power", float)):
            if sd.get(key) is not None:
                setattr(self, key, cast(sd[key]))
        if shadows is not None:
            if self._stash is not None:
                raise RuntimeError("FusedEMA.load_state_dict: the averaged weights are swapped in (store() without restore())")
            for dst, src in zip(self.shadow_tensors().values(), shadows):
                dst.copy_(src)
