"""Opt-in first-block step cache of the denoise loop.

Every forward runs the embedding stage and iteration 0 of the block loop.  The first block's residual ``c = F - E`` is compared with the
one of the last COMPUTED forward (``p``); if it moved by less than ``threshold`` (relative L1, the largest over the clips), iterations
1 .. L-1 are skipped and the residual they produced last time (``t = X - F``) is added instead.  The mode is lossy.  The rule is restated
from memory of diffusers' ``FirstBlockCacheConfig`` and ParaAttention's "FBCache"; neither is installed where this was written, so it is
not pinned against them, and it deviates knowingly in one place: the distance is taken per clip and the LARGEST decides, where diffusers
takes one mean over the whole batch.

``decide`` is the whole decision, on the host, from the two sums per clip the probe kernel leaves.  ``StepCache`` owns the device state
and cuts ``CogVideoXTransformer3DModelTraj._forward_inference`` at two seams (after iteration 0, after the last iteration) into three
segments - front, tail, skip - which ``GraphedTransformer`` captures as three graphs.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops

REASONS = ("first", "shape", "forced", "cap", "threshold")
SUPPORTED = ("supported: an inference forward (eval / no_grad) of a model with num_layers >= 2, threshold >= 0 (inf allowed), "
             "max_consecutive_skips None or >= 0, ORV_CHAINS unset or 1")


def check_threshold(threshold) -> float:
    try:
        th = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"step cache: threshold = {threshold!r} is not a number; {SUPPORTED}") from None
    if math.isnan(th) or th < 0:
        raise ValueError(f"step cache: threshold = {threshold!r}; {SUPPORTED}")
    return th


def check_cap(max_consecutive_skips) -> Optional[int]:
    if max_consecutive_skips is None:
        return None
    if isinstance(max_consecutive_skips, bool) or int(max_consecutive_skips) != max_consecutive_skips or max_consecutive_skips < 0:
        raise ValueError(f"step cache: max_consecutive_skips = {max_consecutive_skips!r}; {SUPPORTED}")
    return int(max_consecutive_skips)


def distances(sums: Sequence[Sequence[float]]) -> List[float]:
    """``d_b = num_b / den_b`` as Python floats; ``den_b == 0`` gives ``inf`` (NaN where ``num_b`` is NaN)."""
    out = []
    for num, den in sums:
        num, den = float(num), float(den)
        if den == 0.0:
            out.append(float("nan") if math.isnan(num) else float("inf"))
        else:
            out.append(num / den)
    return out


def decide(sums, threshold: float, state: str = "valid", forced: bool = False, consecutive_skips: int = 0,
           max_consecutive_skips: Optional[int] = None) -> Tuple[bool, str, Optional[float], Optional[List[float]]]:
    """-> (skip, reason, max distance, per-clip distances).  ``sums``: (num_b, den_b) per clip; ``state``: 'valid' (the stored residuals
    belong to this shape), 'first' (nothing stored since the last reset) or 'shape' (stored for another shape).  Skip iff the state is
    valid, the call is not forced, the cap is not reached and ``max_b d_b < threshold`` - a comparison a NaN fails, so NaN computes.
    Without a valid state the sums were taken against no residual and no distance is reported."""
    if state not in ("valid", "first", "shape"):
        raise ValueError(f"step cache: state = {state!r}; supported: 'valid', 'first', 'shape'")
    if state != "valid":
        return False, state, None, None
    d = distances(sums)
    dmax = float("nan") if any(math.isnan(v) for v in d) else max(d)
    if forced:
        return False, "forced", dmax, d
    if max_consecutive_skips is not None and consecutive_skips >= max_consecutive_skips:
        return False, "cap", dmax, d
    return bool(dmax < threshold), "threshold", dmax, d


class StepCache:
    """State of the step cache of one model: ``first_output`` (F), ``first_residual`` (p) and ``tail_residual`` (t), bf16 [B, Nv, D] of the
    shape in use, ``history`` (one record per forward: ``max_distance``, ``distances``, ``skipped``, ``reason``), ``reset()`` and
    ``force_compute()``.  ``threshold`` and ``max_consecutive_skips`` may be changed between forwards."""

    def __init__(self, threshold, max_consecutive_skips=None, generation: int = 0):
        self._threshold = check_threshold(threshold)
        self._cap = check_cap(max_consecutive_skips)
        self.generation = generation
        self.history: List[SimpleNamespace] = []
        self._bufs = {}
        self._key = None            # the shape in use
        self._valid_key = None      # the shape the stored residuals belong to
        self._ever = False          # something was stored since the last reset
        self._forced = False
        self._consecutive = 0
        self._segment = None        # 'front' while GraphedTransformer drives the segments itself
        self._ctx = None

    threshold = property(lambda self: self._threshold)
    max_consecutive_skips = property(lambda self: self._cap)

    @threshold.setter
    def threshold(self, value):
        self._threshold = check_threshold(value)

    @max_consecutive_skips.setter
    def max_consecutive_skips(self, value):
        self._cap = check_cap(value)

    def reset(self):
        """Forget the stored residuals and the history: the next forward computes (reason ``first``)."""
        self._valid_key, self._ever, self._forced, self._consecutive = None, False, False, 0
        self.history = []

    def force_compute(self):
        """The next forward computes whatever the distance (reason ``forced``)."""
        self._forced = True

    def _buf(self, name):
        return None if self._key is None else self._bufs[self._key][name]

    first_output = property(lambda self: self._buf("f"))
    first_residual = property(lambda self: self._buf("p"))
    tail_residual = property(lambda self: self._buf("t"))

    def _buffers(self, B, Nv, D, dev):
        key = (B, Nv, D, str(dev))
        if key not in self._bufs:
            z = lambda: torch.zeros(B, Nv, D, dtype=torch.bfloat16, device=dev)
            self._bufs[key] = dict(e=z(), f=z(), c=z(), p=z(), t=z(), sums=torch.zeros(B, 2, dtype=torch.float64, device=dev),
                                   scratch=torch.zeros(ops.step_cache_scratch(B, Nv, D), dtype=torch.float64, device=dev))
        self._key = key
        return self._bufs[key]

    def adopt(self, ctx):
        """Make ``ctx`` (of a front segment captured earlier, now replayed from its graph) the context of the next segment."""
        sh = ctx.sh
        self._ctx, self._key = ctx, (sh.B, sh.Nv, sh.D, str(ctx.x.device))

    # ---- the three segments; ctx: what ``_inference_front`` left (shapes, workspace, embed stage outputs, adapter / MXFP8 operands) ----
    def front(self, model, ctx):
        """The rest of the front segment behind ``stages.embed``: snapshot of E, iteration 0, probe."""
        sh = ctx.sh
        b = self._buffers(sh.B, sh.Nv, sh.D, ctx.x.device)
        b["e"].copy_(ctx.x.view(sh.B, sh.S, sh.D)[:, sh.Nt:])
        model._run_blocks(ctx, 0, 1)
        ops.step_cache_probe(ctx.x, b["e"], b["p"], b["f"], b["c"], b["sums"], sh.B, sh.Nt, sh.Nv, sh.D, scratch=b["scratch"])
        self._ctx = ctx

    def decide_now(self) -> bool:
        """The one host read of a step: the [B, 2] sums of the front segment -> skip or compute; writes the history record."""
        key = self._key
        state = "valid" if self._valid_key == key else ("shape" if self._ever else "first")
        sums = self._bufs[key]["sums"].cpu().tolist() if state == "valid" else None
        skip, reason, dmax, d = decide(sums, self._threshold, state, self._forced, self._consecutive, self._cap)
        self._forced = False
        self._consecutive = self._consecutive + 1 if skip else 0
        if not skip:
            self._valid_key, self._ever = key, True
        self.history.append(SimpleNamespace(max_distance=dmax, distances=d, skipped=skip, reason=reason))
        return skip

    def segment(self, model, skip: bool):
        """The tail segment (iterations 1 .. L-1, store, head) or the skip segment (apply, head) on the context of the last front."""
        ctx = self._ctx
        sh = ctx.sh
        b = self._bufs[(sh.B, sh.Nv, sh.D, str(ctx.x.device))]
        if skip:
            ops.step_cache_apply(ctx.x, b["t"], sh.B, sh.Nt, sh.Nv, sh.D)
        else:
            model._run_blocks(ctx, 1, len(model.transformer_blocks))
            ops.step_cache_store(ctx.x, b["f"], b["c"], b["t"], b["p"], sh.B, sh.Nt, sh.Nv, sh.D)
        return model._inference_head(ctx)

    def run(self, model, ctx):
        """One forward: front, and - unless ``GraphedTransformer`` drives the segments - the decision and the segment it selects."""
        self.front(model, ctx)
        if self._segment == "front":
            return None
        return self.segment(model, self.decide_now())
