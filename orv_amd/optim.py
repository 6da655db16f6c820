"""Fused AdamW + global-norm clipping for the bf16-parameter training of the reference
(/root/reference/config/base_train.yaml:143-153: AdamW, betas 0.9/0.95, wd 1e-3, eps 1e-8, max_grad_norm 1.0;
/root/reference/orv/pipeline/train_cogvideox_control_to_video_sft.py:1095-1104: clip then step).

MI355X layout: every trainable parameter becomes a view into ONE flat bf16 buffer (segments padded to 2048 elements), with
flat bf16 gradient and fp32 moment buffers beside it (1.69 B parameters: 3.4 + 3.4 + 6.8 + 6.8 GB of the 288 GB).  A step
is then: gather the autograd gradients into the flat buffer (multi-tensor copy) -> optional RCCL all-reduce (SUM; the 1 / world of the
average is folded into the clip coefficient) of the flat buffer in 256 MB pieces -> ONE ``orv_sumsq`` -> clip coefficient on the device (no host sync before the update) -> ONE
``orv_adamw_flat`` (clip + moments + decoupled decay + bf16 write, 16-byte accesses).  Parameters that received no gradient
in a step are skipped exactly as ``torch.optim.AdamW`` skips them (segment activity mask) and every parameter carries its
OWN step count for the bias correction (``state[p]["step"]`` in torch).  Under data parallel a parameter is active iff it has a gradient on ANY rank (the usage mask rides in the last segment of the flat gradient buffer, so it arrives with the gradient
exchange itself: DDP's ``find_unused_parameters`` bookkeeping, which the reference enables, base_train.yaml:181); a rank without one contributes zeros,
so the collective schedule and the update are identical on all ranks and equal to the single-GPU trajectory.  Moments
are fp32 (the reference keeps them in the parameter dtype).

Parameter precision (``param_precision``): the default ``"bf16"`` rounds every updated weight back to bf16 to nearest-even, as the
reference's bf16 training does, so an update below half a bf16 step of the weight is lost whole.  ``"split_fp32"`` keeps an exact fp32 master
in 2 extra bytes per element (a flat int16 buffer of low halves beside the bf16 weights the model reads), ``"stochastic"`` rounds the fp32 result
to bf16 with a 16-bit random offset drawn from a hash of (seed, step count, flat index) - unbiased, no extra memory, identical on every rank.

State precision (``state_precision``): the default ``"fp32"`` keeps both moments in fp32 (8 bytes per element).  ``"fp8"`` keeps
them as block-scaled fp8 - one byte per element (first moment e4m3fn, second e5m2) plus one scale byte per block of 256, 2 + 2/256 bytes per
element - rounded stochastically with offsets from the same kind of hash (``seed`` is shared with the stochastic weight mode), so all ranks hold
identical state.  It is orthogonal to ``param_precision``; the format is defined in ``orv_amd/csrc/optim_s8.hip``.

Parameter groups, gradient norms, skip guard (all opt-in): ``FusedAdamW`` takes ``torch.optim``'s list of dicts (up to 8 groups
with their own ``lr`` / ``weight_decay``; ``named_groups`` builds it from a model) without reordering storage - a byte per segment names its group
and the rates travel by value with the launch.  With groups, ``skip_nonfinite=True`` or ``track_grad_norms=True`` the one-scalar norm becomes
per-segment fp64 sums in a fixed order (``orv_segment_sumsq``) and one small launch (``orv_step_guard``) that derives the clip coefficient and,
on a non-finite norm, switches the whole step off on the device.

``FusedProdigy`` is the learning-rate-free Prodigy update on the same storage, ``get_optimizer`` the reference's factory
(``train.optimizer.type: adamw | adam | prodigy``) over both classes.  ``FusedCAME`` is the reference's fourth choice,
CAME: one fp32 moment per element and a factored second moment, constructed directly."""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

from . import _state, ops

_SEG = 2048          # elements per workgroup of orv_adamw_flat; every segment is padded to a multiple of it
PARAM_PRECISIONS = ("bf16", "split_fp32", "stochastic")
STATE_PRECISIONS = ("fp32", "fp8")
_MAX_GROUPS = 8      # parameter groups of FusedAdamW (ORV_ADAMW_MAX_GROUPS: the by-value table of the _groups kernels)
_GROUP_KEYS = ("params", "lr", "weight_decay", "name", "initial_lr")      # what a parameter-group dict may carry
_BLOCK = 256         # elements per scale byte of the fp8 moments; divides _SEG, so a block never straddles a segment
_AR_CHUNK = 128 * 1024 * 1024   # bf16 elements per all-reduce call (256 MB: large enough that xGMI link bandwidth, not
#                                 launch latency, bounds the ring)


def _sqrt(x: float) -> float:
    """correctly rounded square root of a sum of squares; a NaN stays a NaN"""
    import math
    return math.sqrt(x) if x == x else x


class FusedAdamW:
    _checkpoint_kind = "adamw"
    _element_moments = ("m", "v")       # the fp32 per-element moment buffers ``_build`` allocates (FusedCAME keeps no element-sized v)
    _moment_keys = {"m": "exp_avg", "v": "exp_avg_sq"}      # their names in a checkpoint

    _supports_groups = True             # FusedProdigy / FusedCAME: one group only (their kernels take one lr)

    def __init__(self, params: Iterable[torch.nn.Parameter], lr=1e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-3,
                 max_grad_norm: float = 1.0, param_precision: str = "bf16", seed: int = 0, state_precision: str = "fp32",
                 skip_nonfinite: bool = False, track_grad_norms: bool = False):
        """``params``: an iterable of parameters, or - as for ``torch.optim.AdamW`` - a list of up to 8 dicts ``{"params": [...], "lr": ...,
        "weight_decay": ..., "name": ...}`` (parameter groups; missing keys take this constructor's values; ``betas``,
        ``eps``, ``max_grad_norm`` and the precisions are global).  Groups do not reorder storage: the flat layout is what it is without them
        and a byte per segment names its group.  ``param_groups`` is read at every step, so a schedule may change any group's ``lr``.
        ``skip_nonfinite=True``: a step whose global gradient norm is not finite updates nothing - weights, masters, moments and
        per-parameter step counts keep every byte - and is counted in ``skipped_steps``; the decision is taken on the device.
        ``track_grad_norms=True``: ``grad_norms()`` returns per-parameter, per-group and global norms of the last step.  Any of the three
        replaces ``orv_sumsq`` and the clip arithmetic by ``orv_segment_sumsq`` + ``orv_step_guard`` and the update by its ``_groups``
        form; without them a step issues exactly the launches it always did.

        ``step_count`` is the host's count of ``step()`` calls: it seeds the stochastic rounding (and the fp8 moments' offsets) and keeps
        advancing on a skipped step; the bias corrections follow the per-parameter counts on the device, which a skipped step leaves alone."""
        who = type(self).__name__
        if param_precision not in PARAM_PRECISIONS:
            raise ValueError(f"FusedAdamW: unknown param_precision {param_precision!r} (one of {', '.join(PARAM_PRECISIONS)})")
        if state_precision not in STATE_PRECISIONS:
            raise ValueError(f"FusedAdamW: unknown state_precision {state_precision!r} (one of {', '.join(STATE_PRECISIONS)})")
        if not 0 <= int(seed) < 2 ** 32:
            raise ValueError(f"FusedAdamW: seed={seed} must be a 32-bit unsigned integer")
        self.param_precision, self.state_precision, self.seed = param_precision, state_precision, int(seed)
        given = list(params)
        self._grouped = bool(given) and isinstance(given[0], dict)
        if self._grouped:
            group_of, specs = {}, []
            if len(given) > 1 and not self._supports_groups:
                raise ValueError(f"{who}: {len(given)} parameter groups; {who} keeps one group (its kernels take one lr) - FusedAdamW is the "
                                 f"class that has parameter groups (supported here: one group, or a plain iterable of parameters)")
            if len(given) > _MAX_GROUPS:
                raise ValueError(f"{who}: {len(given)} parameter groups (supported: 1..{_MAX_GROUPS}; the table of their lr / weight_decay "
                                 "travels by value with every launch)")
            for j, d in enumerate(given):
                extra = sorted(set(d) - set(_GROUP_KEYS)) if isinstance(d, dict) else ["<not a dict>"]
                if extra or "params" not in d:
                    raise ValueError(f"{who}: parameter group {j} carries {', '.join(extra) or 'no params'}; a group may carry "
                                     f"{', '.join(_GROUP_KEYS)} - betas, eps, max_grad_norm, param_precision and state_precision are global")
                gp = [p for p in d["params"] if p.requires_grad]
                name = str(d.get("name", f"group{j}"))
                if not gp:
                    raise ValueError(f"{who}: parameter group {j} ({name!r}) is empty (supported: at least one trainable parameter per group)")
                for p in gp:
                    if id(p) in group_of:
                        raise ValueError(f"{who}: a parameter of shape {tuple(p.shape)} is in two groups, {group_of[id(p)]} and {j} "
                                         "(supported: every parameter in exactly one group)")
                    group_of[id(p)] = j
                g_lr = d.get("lr", lr)
                specs.append({"lr": g_lr, "initial_lr": d.get("initial_lr", g_lr), "weight_decay": d.get("weight_decay", weight_decay),
                              "name": name, "params": gp})
            if len({s["name"] for s in specs}) != len(specs):
                raise ValueError(f"{who}: group names {[s['name'] for s in specs]} are not distinct (grad_norms() reports by name)")
            ps = [p for s in specs for p in s["params"]]
        else:
            ps = [p for p in given if p.requires_grad]
        # flat-buffer order: parameters the model tagged as "gradient final when its block's backward ends" first (model order: a block's
        # six weights are contiguous), everything else behind them - see CogVideoXTransformer3DModelTraj._set_trainable_parameters and
        # sharding.FlatGradReducer.  Untagged parameter lists (any other model) keep their order.  Groups do not enter.
        self.params: List[torch.nn.Parameter] = ([p for p in ps if getattr(p, "_orv_grad_early", False)]
                                                 + [p for p in ps if not getattr(p, "_orv_grad_early", False)])
        if self._grouped:
            self.param_groups = specs
            self._group_index = [group_of[id(p)] for p in self.params]      # group of every segment, flat order
        else:
            self.param_groups = [{"lr": lr, "initial_lr": lr, "weight_decay": weight_decay, "name": "all", "params": self.params}]
            self._group_index = [0] * len(self.params)
        self.betas, self.eps, self.max_grad_norm = betas, eps, max_grad_norm
        self.skip_nonfinite, self.track_grad_norms = bool(skip_nonfinite), bool(track_grad_norms)
        # the device-side statistics path: per-segment sums + step guard + the per-group update (else: the one-scalar path)
        self._guarded = (self._grouped and self._supports_groups) or self.skip_nonfinite or self.track_grad_norms
        self._skipped_steps, self.last_step_skipped, self._last_world = 0, False, 1
        self.step_count = 0
        self._flat = None
        self._handed = set()      # segments handed to the backward for in-place writing since the last step() / zero_grad()
        self._dirty = set()       # segments that hold data (written in place or copied into) and were not zeroed since

    # ``optimizer.lr`` / ``optimizer.weight_decay``: group 0, the only group of an optimizer built without groups
    lr = property(lambda self: self.param_groups[0]["lr"], lambda self, x: self.param_groups[0].__setitem__("lr", x))
    weight_decay = property(lambda self: self.param_groups[0]["weight_decay"],
                            lambda self, x: self.param_groups[0].__setitem__("weight_decay", x))

    @property
    def skipped_steps(self) -> int:
        """Steps the guard skipped so far (the device's counter, as of the last ``step()``'s host read)."""
        return self._skipped_steps

    def _grad_segment(self, i: int) -> torch.Tensor:
        return self._flat["views_g"][i]

    # ---- flat storage ----
    def _build(self):
        dev = self.params[0].device
        for p in self.params:
            if p.dtype != torch.bfloat16 or p.device != dev:
                raise RuntimeError("FusedAdamW: parameters must be bf16 tensors on one GPU (call model.to(device, bfloat16) first)")
        offs, o = [], 0
        for p in self.params:
            offs.append(o)
            o += (p.numel() + _SEG - 1) // _SEG * _SEG
        total = o
        # the gradient buffer carries one more segment: the usage mask of this rank (1.0 per parameter with a gradient), so that
        # under data parallel "used on ANY rank" arrives with the gradient exchange itself (SUM > 0) instead of a second collective
        tail = (len(self.params) + _SEG - 1) // _SEG * _SEG
        flat_p = torch.zeros(total, dtype=torch.bfloat16, device=dev)
        views_p, views_g = [], []
        flat_g = torch.zeros(total + tail, dtype=torch.bfloat16, device=dev)
        for p, off in zip(self.params, offs):
            v = flat_p[off:off + p.numel()].view(p.shape)
            v.copy_(p.data)
            p.data = v                                   # the module keeps its Parameter objects; only their storage moves
            views_p.append(v)
            views_g.append(flat_g[off:off + p.numel()].view(p.shape))
        self._flat = dict(
            p=flat_p, g=flat_g, g_params=flat_g[:total], g_mask=flat_g[total:total + len(self.params)],
            reduce_starts=offs + [total, total + tail], views_g=views_g, offs=offs,
            seg_start=torch.tensor(offs + [total], dtype=torch.int64, device=dev),
            active=torch.zeros(len(self.params), dtype=torch.uint8, device=dev), active_host=[False] * len(self.params),
            seg_step=torch.zeros(len(self.params), dtype=torch.int32, device=dev))
        if self._guarded:
            # group of every segment; per-segment sums of g^2; the guard's report (its skip counter continues a loaded checkpoint's)
            self._flat.update(seg_group=torch.tensor(self._group_index, dtype=torch.uint8, device=dev),
                              seg_ss=torch.zeros(len(self.params), dtype=torch.float64, device=dev),
                              clip=torch.zeros(1, dtype=torch.float32, device=dev),
                              report=torch.zeros(len(ops.GUARD_REPORT), dtype=torch.float64, device=dev))
            if self._skipped_steps:
                self._flat["report"][ops.GUARD_REPORT.index("skip_count")] = float(self._skipped_steps)
        if self.state_precision == "fp8":
            # all-zero bytes: every element +0 in a block of scale 2^-127, i.e. zero moments
            z8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
            self._flat.update(m8=z8(total), v8=z8(total), m_exp=z8(total // _BLOCK), v_exp=z8(total // _BLOCK))
        else:
            self._flat.update({b: torch.zeros(total, dtype=torch.float32, device=dev) for b in self._element_moments})
        if self.param_precision == "split_fp32":
            # low halves of the fp32 masters, same segment layout as `p`; zeros: the master is the current bf16 value exactly
            lo = torch.zeros(total, dtype=torch.int16, device=dev)
            self._flat.update(lo=lo, views_lo=[lo[off:off + p.numel()] for p, off in zip(self.params, offs)])
            self._seen_versions = [p._version for p in self.params]
        _state.register_grad_views(self.params, self)
        _state.bump_weights_epoch()      # parameter storage moved (p.data = view): captured graphs / derived-weight caches are stale

    # ---- data parallel: exchange overlapped with the backward ----
    def begin_overlapped_allreduce(self):
        """Returns ``hook(params, grads)`` for ``training.backward``: called whenever the gradients of a group of parameters
        are final, it copies them into the flat buffer and lets a ``FlatGradReducer`` start summing every contiguous final
        run over the process group while the backward continues.  ``step(average_over=world)`` then only sends the rest."""
        from .sharding import FlatGradReducer
        if self._flat is None:
            self._build()
        f = self._flat
        index = {id(p): i for i, p in enumerate(self.params)}
        red = FlatGradReducer(f["g"], f["reduce_starts"])      # parameter segments + the usage-mask segment (sent by finish())
        filled = set()

        def hook(params, grads):
            # Which segments one call makes final is decided by the CODE PATH of the backward, not by the data: the big weights
            # of a block have their gradient here, its small fp32-accumulated ones (biases, LayerNorm affine) are converted
            # at the very end on every rank alike, and the parameters whose gradient may exist on one rank only (action
            # reconstruction head, mask embedding, control fuse) are in no block list - they travel in ``finish`` as zeros
            # where a rank has none.  So every rank issues the same collectives in the same order.
            idx, srcs, dsts = [], [], []
            for p in params:
                i, g = index.get(id(p)), grads.get(id(p))
                if i is None or g is None or i in filled:
                    continue
                idx.append(i)
                if g.data_ptr() != f["views_g"][i].data_ptr():      # else: the backward wrote it in place (_state.grad_view)
                    srcs.append(g); dsts.append(f["views_g"][i])
            if not idx:
                return
            if srcs:
                torch._foreach_copy_(dsts, srcs)
            filled.update(idx)
            red.ready(idx)

        self._overlap = (red, filled)
        return hook

    def averaged_grads(self):
        """{parameter: averaged gradient copy} after a data-parallel ``step()`` (the flat buffer holds the SUM over ranks, see ``step``)."""
        import torch.distributed as dist
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        if self._flat is None:
            return {}
        return {p: (v.float() / world).to(v.dtype) for p, v in zip(self.params, self._flat["views_g"])}

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            p.grad = None
        # a segment written in place whose gradient is dropped here (skipped / overflow step) keeps its data: remember it so
        # the next step() zeroes it unless a new gradient overwrites it
        self._dirty |= self._handed
        self._handed.clear()

    @torch.no_grad()
    def step(self, average_over: Optional[int] = None) -> float:
        """One update.  ``average_over=world_size`` first averages the flat gradient buffer over the default process group
        (data parallel, one exchange per step).  NOTE: under data parallel the exchange is a SUM and 1 / world is folded
        into the clip coefficient and the returned norm, so after ``step()`` the ``p.grad`` views that alias the flat segments hold
        ``world x`` the mean gradient (also for segments this rank never produced); code that inspects ``p.grad`` afterwards
        (per-parameter norm logging) must divide by the world size - ``averaged_grads()`` returns such copies.  Returns the pre-clip global gradient norm (the only host read, issued after
        every kernel of the step is queued)."""
        if not self.params:
            return 0.0
        if self._flat is None:
            self._build()
        f = self._flat
        overlap = getattr(self, "_overlap", None)
        self._overlap = None
        distributed = overlap is not None or bool(average_over and average_over > 1)
        has_grad = [p.grad is not None for p in self.params]
        dev = f["p"].device
        if not distributed and not any(has_grad):
            return 0.0
        done = overlap[1] if overlap else ()
        self._dirty |= self._handed          # segments the backward wrote in place since the last step
        self._handed.clear()
        self._dirty.update(done)
        # A segment without a gradient this step must read as zeros for the global norm (and, under data parallel, for the
        # exchange): zero every one that holds data - a parameter that lost its gradient (zero_grad on a skipped step,
        # torch.autograd.grad, a branch not taken this step) - not only the active -> inactive transitions.
        stale = [i for i in self._dirty if not has_grad[i] and i not in done]
        if stale:
            torch._foreach_zero_([f["views_g"][i] for i in stale])
            self._dirty.difference_update(stale)
        pairs = [(p.grad, v) for i, (p, v, a) in enumerate(zip(self.params, f["views_g"], has_grad))
                 if a and i not in done and p.grad.data_ptr() != v.data_ptr()]     # in-place gradients need no copy
        srcs, dsts = [s_ for s_, _ in pairs], [d_ for _, d_ in pairs]
        if srcs:
            torch._foreach_copy_(dsts, srcs)
        self._dirty.update(i for i, h in enumerate(has_grad) if h)
        world = 1
        if distributed:
            # Data parallel: a parameter is updated iff it has a gradient on ANY rank (DDP's local_used_map with
            # find_unused_parameters, /root/reference/config/base_train.yaml:181): a rank without one contributes zeros, and
            # a parameter unused on every rank is skipped as torch.optim.AdamW skips grad-None parameters (no decay, no
            # moment decay, no step-count increment) - the same trajectory as the single-GPU run.  The mask rides in the last
            # segment of the gradient buffer (1.0 where this rank has a gradient; SUM over ranks > 0 <=> used somewhere), so
            # the step issues gradient collectives only, at the same points on every rank; it stays on the device.
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                world = dist.get_world_size()
            f["g_mask"].copy_(torch.tensor(has_grad, dtype=torch.bfloat16))
            if overlap is not None:
                overlap[0].finish(average=False)         # the rest of the buffer (mask segment included), wait
                self.last_exchange = overlap[0]          # bookkeeping for bench.py (collectives, bytes, exposed time): .stats()
            else:
                from .sharding import allreduce_flat_
                allreduce_flat_(f["g"], _AR_CHUNK, average=False)
            f["active"].copy_((f["g_mask"] > 0).to(torch.uint8))
            f["active_host"] = None                      # device-side mask: the host copy is unknown
            if world > 1:
                # the exchange wrote the summed gradient into EVERY segment, also those this rank has no gradient for: all of
                # them hold data now and must be zeroed before the next exchange / norm unless a new gradient overwrites them
                self._dirty.update(range(len(self.params)))
        elif has_grad != f["active_host"]:
            f["active"].copy_(torch.tensor(has_grad, dtype=torch.uint8))
            f["active_host"] = has_grad
        # The buffer holds the SUM over ranks; the 1 / world of the average is folded into the coefficient handed to the update
        # kernel (no separate pass over 3.4 GB): norm of the mean gradient = norm of the sum / world.
        if self._guarded:
            return self._guarded_step(f, world)
        ss = torch.zeros(1, dtype=torch.float32, device=dev)
        ops.sumsq(f["g_params"], ss)
        norm = ss.sqrt() / world
        clip = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0) if self.max_grad_norm else torch.ones_like(norm)
        if world > 1:
            clip = clip / world
        self.step_count += 1
        f["seg_step"].add_(f["active"].to(torch.int32))          # per-parameter step counts (torch.optim.AdamW state["step"])
        self._launch_update(f, clip)
        _state.bump_weights_epoch()      # parameters changed without a tensor._version bump: drop derived-weight caches
        return float(norm.item())

    def _guarded_step(self, f, world: int) -> float:
        """The rest of ``step()`` with groups, the skip guard or norm tracking: per-segment sums of g^2 in a fixed order,
        then ONE small launch that adds them up, writes the clip coefficient and - on a non-finite norm with ``skip_nonfinite`` - clears the
        activity mask; the per-parameter step counts and the update come behind it, so a skipped step moves nothing.  The host reads the
        report (norm, skip flag and count in one copy) after everything is queued."""
        ops.segment_sumsq(f["g"], f["seg_start"], f["seg_ss"])
        ops.step_guard(f["seg_ss"], f["seg_group"], f["active"], f["clip"], f["report"], float(self.max_grad_norm or 0.0), 1.0 / world,
                       self.skip_nonfinite)
        self.step_count += 1
        f["seg_step"].add_(f["active"].to(torch.int32))          # behind the guard: a skipped step adds zeros
        groups = self.param_groups
        common = dict(seg_step=f["seg_step"], lo=f.get("lo"), mode=ops.ADAMW_MODES[self.param_precision], seed=self.seed,
                      max_group=len(groups) - 1)
        lrs, wds = [g["lr"] for g in groups], [g["weight_decay"] for g in groups]
        if "lo" in f:
            self._drop_stale_param_lo()
        if self.state_precision == "fp8":
            ops.adamw_flat_s8_groups(f["p"], f["g"], f["m8"], f["v8"], f["m_exp"], f["v_exp"], f["seg_start"], f["active"], f["seg_group"],
                                     lrs, wds, self.betas[0], self.betas[1], self.eps, self.step_count, f["clip"],
                                     common_count=self.step_count - self._skipped_steps, **common)      # where the counts stand after skips
        else:
            ops.adamw_flat_groups(f["p"], f["g"], f["m"], f["v"], f["seg_start"], f["active"], f["seg_group"], lrs, wds, self.betas[0],
                                  self.betas[1], self.eps, self.step_count, f["clip"], **common)
        _state.bump_weights_epoch()
        report = dict(zip(ops.GUARD_REPORT, f["report"].tolist()))      # the step's one host read
        self._last_world = world
        self._skipped_steps, self.last_step_skipped = int(report["skip_count"]), bool(report["skipped"])
        if self.last_step_skipped:
            f["active_host"] = None          # the guard cleared the device mask: the host copy no longer describes it
        return _sqrt(report["ss"]) / world

    @torch.no_grad()
    def grad_norms(self):
        """``{"global": float, "groups": {name: float}, "params": fp64 tensor[len(self.params)] on the device}`` of the last ``step()``:
        norms of the gradient before clipping - of the MEAN gradient under data parallel - per parameter in ``self.params`` order (the
        flat-buffer order).  One host read (the report), made here and only when this is called; the sums behind it are those of
        ``orv_segment_sumsq``, reproducible to the bit.  Needs groups, ``skip_nonfinite`` or ``track_grad_norms=True``."""
        if not self._guarded:
            raise RuntimeError(f"{type(self).__name__}.grad_norms: per-parameter sums are not kept on the one-scalar path; construct with "
                               "track_grad_norms=True (or with parameter groups / skip_nonfinite=True)")
        if self._flat is None or self.step_count == 0:
            raise RuntimeError(f"{type(self).__name__}.grad_norms: no step has run yet")
        f, world = self._flat, self._last_world
        report = dict(zip(ops.GUARD_REPORT, f["report"].tolist()))
        return {"global": _sqrt(report["ss"]) / world,
                "groups": {g["name"]: _sqrt(report[f"group{j}"]) / world for j, g in enumerate(self.param_groups)},
                "params": f["seg_ss"].sqrt() / world}

    def _launch_update(self, f, clip):
        """The update kernel(s) of one step on the flat buffers ``f``; ``clip`` is the device-side coefficient (1 / world folded in)."""
        if self.state_precision == "fp8":
            if "lo" in f:
                self._drop_stale_param_lo()
            ops.adamw_flat_s8(f["p"], f["g"], f["m8"], f["v8"], f["m_exp"], f["v_exp"], f["seg_start"], f["active"],
                              self.param_groups[0]["lr"], self.betas[0], self.betas[1], self.eps, self.weight_decay, self.step_count, clip,
                              seg_step=f["seg_step"], lo=f.get("lo"), mode=ops.ADAMW_MODES[self.param_precision], seed=self.seed)
        elif self.param_precision == "bf16":
            ops.adamw_flat(f["p"], f["g"], f["m"], f["v"], f["seg_start"], f["active"], self.param_groups[0]["lr"], self.betas[0],
                           self.betas[1], self.eps, self.weight_decay, self.step_count, clip, seg_step=f["seg_step"])
        else:
            if "lo" in f:
                self._drop_stale_param_lo()
            ops.adamw_flat_ex(f["p"], f["g"], f["m"], f["v"], f["seg_start"], f["active"], self.param_groups[0]["lr"], self.betas[0],
                              self.betas[1], self.eps, self.weight_decay, self.step_count, clip, seg_step=f["seg_step"],
                              lo=f.get("lo"), mode=ops.ADAMW_MODES[self.param_precision], seed=self.seed)

    # ---- fp32 masters (param_precision="split_fp32") ----
    def _drop_stale_param_lo(self):
        """A parameter written by anything but this optimizer since the last ``step`` (``model.load_state_dict``, ``p.copy_`` under
        ``no_grad``: both bump ``p._version``; the update kernel does not) has a low half that belongs to a weight that is gone: zero it,
        so that the master is the new bf16 value exactly."""
        moved = [i for i, (p, ver) in enumerate(zip(self.params, self._seen_versions)) if p._version != ver]
        if moved:
            torch._foreach_zero_([self._flat["views_lo"][i] for i in moved])
            for i in moved:
                self._seen_versions[i] = self.params[i]._version

    @torch.no_grad()
    def reset_param_lo(self, params: Optional[Iterable[torch.nn.Parameter]] = None):
        """Zero the low halves of the fp32 masters of ``params`` (default: all), i.e. make every master equal to its current bf16 weight.
        In-place writes to a parameter that bump ``p._version`` are seen by ``step`` and handled there; writes through ``p.data`` (or raw
        device pointers) do NOT bump it and cannot be seen - call this after them.  A stale low half is bounded harm (the master is off by
        at most half a bf16 step, once), never a wrong weight.  No-op outside ``param_precision="split_fp32"``."""
        if self.param_precision != "split_fp32":
            return
        if self._flat is None:
            self._build()
        if params is None:
            self._flat["lo"].zero_()
        else:
            index = {id(p): i for i, p in enumerate(self.params)}
            for p in params:
                if id(p) not in index:
                    raise ValueError("FusedAdamW.reset_param_lo: a parameter this optimizer does not own")
                self._flat["views_lo"][index[id(p)]].zero_()
        self._seen_versions = [p._version for p in self.params]

    @torch.no_grad()
    def master_params(self) -> List[torch.Tensor]:
        """The fp32 master of every parameter (new fp32 tensors shaped like the parameters, in ``self.params`` order): bit pattern
        ``(p_bits << 16) + sign_extend(lo)`` under ``"split_fp32"`` (minus the low halves ``step`` would drop as stale), the bf16 value
        itself in the other modes.  For tests and for exporting a checkpoint at full precision."""
        if self.param_precision != "split_fp32" or self._flat is None:
            return [p.detach().float() for p in self.params]
        self._drop_stale_param_lo()
        return [(p.detach().float().view(torch.int32) + lo.view(p.shape).to(torch.int32)).view(torch.float32)
                for p, lo in zip(self.params, self._flat["views_lo"])]

    # ---- moments ----
    def _dequantized(self, q, exps, fmt):
        x = torch.empty(q.numel(), dtype=torch.float32, device=q.device)
        ops.state8_dequantize(q, exps, x, fmt)
        return x

    @torch.no_grad()
    def moments(self):
        """``(exp_avg, exp_avg_sq)``: the fp32 value of both moments of every parameter (two lists of new fp32 tensors shaped like the
        parameters, in ``self.params`` order), in either state precision - dequantising fp8 moments is exact.  For tests and exports."""
        if self._flat is None:
            self._build()
        f = self._flat
        if self.state_precision == "fp8":
            m, v = self._dequantized(f["m8"], f["m_exp"], "m"), self._dequantized(f["v8"], f["v_exp"], "v")
        else:
            m, v = f["m"], f.get("v")
        cut = lambda x: [x[o:o + p.numel()].view(p.shape).clone() for p, o in zip(self.params, f["offs"])]
        return cut(m), None if v is None else cut(v)

    # ---- checkpointing (torch.optim-like) ----
    def state_dict(self):
        """Flat moments plus the layout they are stored in (parameter element counts and segment offsets), so that a resume
        with a different trainable set fails loudly instead of mis-assigning moments."""
        layout = [int(p.numel()) for p in self.params]
        mode = {"param_precision": self.param_precision, "state_precision": self.state_precision, "seed": self.seed}
        if self._guarded:                   # JSON: the groups as index lists into the flat order, and the guard's counter
            mode["groups"] = [{"name": g["name"], "lr": g["lr"], "initial_lr": g["initial_lr"], "weight_decay": g["weight_decay"],
                               "params": [i for i, j in enumerate(self._group_index) if j == k]} for k, g in enumerate(self.param_groups)]
            mode["skipped_steps"] = self._skipped_steps
        fp8 = self.state_precision == "fp8"
        names = {"exp_avg8": "m8", "exp_avg_sq8": "v8", "exp_avg_exp": "m_exp", "exp_avg_sq_exp": "v_exp"} if fp8 else {self._moment_keys[b]: b for b in self._element_moments}
        if self._flat is None:
            return {"step": self.step_count, **{k: None for k in names}, "numels": layout, **mode}
        sd = {"step": self.step_count, **{k: self._flat[b] for k, b in names.items()}, "numels": layout,
              "seg_start": self._flat["seg_start"].tolist(), "seg_step": self._flat["seg_step"], **mode}
        if "lo" in self._flat:
            self._drop_stale_param_lo()
            sd["param_lo"] = self._flat["lo"]
        return sd

    def load_state_dict(self, sd):
        if sd.get("optimizer") not in (None, self._checkpoint_kind):        # FusedAdamW's own checkpoints carry no such key
            raise ValueError(f"{type(self).__name__}.load_state_dict: the checkpoint was written by the {sd['optimizer']!r} optimizer; its moments "
                             "have another meaning (Prodigy's carry a factor d, CAME's second moment is factored) and are not taken over")
        layout = [int(p.numel()) for p in self.params]
        if sd.get("numels") is not None and list(sd["numels"]) != layout:
            if sorted(sd["numels"]) == sorted(layout):
                raise ValueError("FusedAdamW.load_state_dict: same parameters, another flat-buffer ORDER - the checkpoint predates round 6, which "
                                 "lays the block weights out first (one all-reduce per block); its moments cannot be mapped by position.  Resume "
                                 "the parameters from the model checkpoint and restart the moments, or load with the build that wrote it")
            raise ValueError("FusedAdamW.load_state_dict: the checkpoint was written for a different set of trainable parameters "
                             f"({len(sd['numels'])} segments vs {len(layout)} here, or different sizes)")
        # Groups: the checkpoint's must cut the parameters as the live optimizer's do (a checkpoint without the key - every one written
        # before groups existed, and the one-scalar path's today - holds one group over all parameters); their lr / weight_decay are
        # taken over, as torch.optim does.
        live = [[i for i, j in enumerate(self._group_index) if j == k] for k in range(len(self.param_groups))]
        stored = sd.get("groups")
        theirs = [sorted(int(i) for i in g["params"]) for g in stored] if stored is not None else [list(range(len(self.params)))]
        if theirs != live:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the checkpoint holds {len(theirs)} parameter group(s) of "
                             f"{[len(t) for t in theirs]} parameters, this optimizer {len(live)} of {[len(t) for t in live]}, or the same "
                             "counts over other parameters; per-group settings cannot be mapped onto another partition")
        for g, s in zip(self.param_groups, stored or ()):
            g.update(lr=s["lr"], initial_lr=s["initial_lr"], weight_decay=s["weight_decay"], name=s["name"])
        self._skipped_steps = int(sd.get("skipped_steps") or 0)
        if self._flat is not None and "report" in self._flat:
            self._flat["report"][ops.GUARD_REPORT.index("skip_count")] = float(self._skipped_steps)
        self.step_count = int(sd["step"])
        # The precision mode is the constructor's; the stored one is a record.  The seed of the stochastic sequence is taken over, so that a
        # resumed run continues it.  Checkpoints without these keys (the default mode, older builds) load into any mode.
        if sd.get("seed") is not None:
            self.seed = int(sd["seed"])
        have = "fp8" if sd.get("exp_avg8") is not None else "fp32" if sd.get("exp_avg") is not None else None
        if self.param_precision == "split_fp32" and (sd.get("param_lo") is not None or have):
            if self._flat is None:
                self._build()
            lo = sd.get("param_lo")
            if lo is not None and lo.numel() != self._flat["lo"].numel():
                raise ValueError(f"FusedAdamW.load_state_dict: param_lo holds {lo.numel()} elements, the flat layout {self._flat['lo'].numel()}")
            if lo is None:                  # written by another mode: the masters are the bf16 weights
                self._flat["lo"].zero_()
            else:
                self._flat["lo"].copy_(lo)
            self._seen_versions = [p._version for p in self.params]
        if have:
            if self._flat is None:
                self._build()
            f = self._flat
            total = f["p"].numel()
            keys = ("exp_avg8", "exp_avg_sq8", "exp_avg_exp", "exp_avg_sq_exp") if have == "fp8" else tuple(self._moment_keys[b] for b in self._element_moments)
            want = (total, total, total // _BLOCK, total // _BLOCK)
            if any(sd.get(k) is None or sd[k].numel() != n for k, n in zip(keys, want)):
                raise ValueError("FusedAdamW.load_state_dict: moment buffers do not match the flat layout")
            dev = f["p"].device
            if have == self.state_precision:
                for k, b in zip(keys, ("m8", "v8", "m_exp", "v_exp") if have == "fp8" else self._element_moments):
                    f[b].copy_(sd[k])
            elif have == "fp32":              # fp32 checkpoint -> fp8 state: the bytes the update kernel would have stored at (seed, step)
                for k, q, e, fmt in (("exp_avg", "m8", "m_exp", "m"), ("exp_avg_sq", "v8", "v_exp", "v")):
                    ops.state8_quantize(sd[k].to(dev, torch.float32).contiguous(), f[q], f[e], fmt, seed=self.seed, step=self.step_count)
            else:                             # fp8 checkpoint -> fp32 state: exact
                for q, e, b, fmt in (("exp_avg8", "exp_avg_exp", "m", "m"), ("exp_avg_sq8", "exp_avg_sq_exp", "v", "v")):
                    ops.state8_dequantize(sd[q].to(dev).contiguous(), sd[e].to(dev).contiguous(), f[b], fmt)
            if sd.get("seg_step") is not None:
                self._flat["seg_step"].copy_(sd["seg_step"])
            else:                           # checkpoints written before per-parameter counts existed
                self._flat["seg_step"].fill_(self.step_count)


class FusedProdigy(FusedAdamW):
    """Prodigy, the learning-rate-free optimizer of the CogVideoX LoRA recipes (``train.optimizer.type: prodigy``; the reference's orv/utils.py:112-134),
    fused on the flat storage of ``FusedAdamW``: same flat bf16 gradient buffer, device-side clip coefficient, usage mask, overlapped gradient
    exchange and per-parameter skip; only the update differs.  The rule restates ``prodigyopt`` 1.0's ``Prodigy.step`` from
    memory (unpinned: the package is not available to compare against; one parameter group, no ``slice_p`` / ``fsdp_in_use``) and is written
    out in ``orv_amd/csrc/optim_prodigy.hip``.  A step is three stream-ordered launches - moments and per-chunk partial sums, the scalar
    recurrence of the step-size estimate ``d``, the weight update - and every scalar (``d``, ``d_max``, ``d_numerator``, ``k``) lives in a
    small fp64 array on the device: the host reads nothing inside a step.  Under data parallel every rank holds the same summed gradient and
    therefore computes the same ``d``; no collective is added.

    The weights are ALWAYS the exact split fp32 master of ``FusedAdamW(param_precision="split_fp32")``: the first updates have the size of
    ``d0`` (1e-6), far below half a bf16 step of any weight, so on bf16 weights ``p0 - p`` stays exactly 0, the numerator of the estimate
    stays 0 and ``d`` never leaves ``d0``.  ``p0``, the weight at a parameter's first update, is stored as bf16: at that moment the low half
    of a parameter this optimizer never updated is zero and the bf16 value is the master exactly.  If a low half is not zero then (a loaded
    checkpoint of another optimizer's masters) nothing is zeroed or refused: ``p0`` is the bf16 part of the master.

    ``lr`` multiplies the estimate (keep it at 1.0; schedules poke ``param_groups[0]["lr"]``, read at every step).  ``d``, ``d_max``,
    ``d_hat``, ``k``, ``dlr`` are host reads on demand, for logging."""

    _checkpoint_kind = "prodigy"      # state_dict()["optimizer"]
    _supports_groups = False

    def __init__(self, params: Iterable[torch.nn.Parameter], lr=1.0, betas=(0.9, 0.999), beta3: Optional[float] = None, eps=1e-8,
                 weight_decay=0.0, decouple: bool = True, use_bias_correction: bool = False, safeguard_warmup: bool = False, d0=1e-6,
                 d_coef=1.0, growth_rate=float("inf"), max_grad_norm: float = 1.0, param_precision: str = "split_fp32",
                 state_precision: str = "fp32"):
        if param_precision in ("bf16", "stochastic"):
            raise ValueError(f"FusedProdigy: param_precision={param_precision!r} cannot work: the first updates have the size of d0 = {d0:g}, "
                             "far below half a bf16 step of the weights, so they vanish in bf16, p0 - p stays 0 and d never grows "
                             "(supported: 'split_fp32', the exact fp32 master)")
        if param_precision != "split_fp32":
            raise ValueError(f"FusedProdigy: unknown param_precision {param_precision!r} (supported: 'split_fp32')")
        if state_precision != "fp32":
            raise ValueError(f"FusedProdigy: state_precision={state_precision!r} is not built for Prodigy (supported: 'fp32')")
        if not eps > 0:
            raise ValueError(f"FusedProdigy: eps={eps} must be greater than 0 (an element whose second moment is 0 divides by d * eps)")
        if not d0 > 0:
            raise ValueError(f"FusedProdigy: d0={d0} must be greater than 0")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                         param_precision="split_fp32", state_precision="fp32")
        self.beta3 = float(betas[1]) ** 0.5 if beta3 is None else float(beta3)
        self.decouple, self.use_bias_correction, self.safeguard_warmup = bool(decouple), bool(use_bias_correction), bool(safeguard_warmup)
        self.d0, self.d_coef, self.growth_rate = float(d0), float(d_coef), float(growth_rate)

    def _build(self):
        super()._build()
        f = self._flat
        dev, total = f["p"].device, f["p"].numel()
        f.update(s=torch.zeros(total, dtype=torch.float32, device=dev), p0=torch.zeros(total, dtype=torch.bfloat16, device=dev),
                 partials=torch.zeros(2 * (total // _SEG), dtype=torch.float64, device=dev),     # one (numerator, denominator) pair per chunk
                 pstate=torch.tensor([self.d0, self.d0] + [0.0] * (len(ops.PRODIGY_STATE) - 2), dtype=torch.float64, device=dev))

    def _launch_update(self, f, clip):
        self._drop_stale_param_lo()
        lr, (b1, b2) = self.param_groups[0]["lr"], self.betas
        ops.prodigy_moments(f["p"], f["lo"], f["g"], f["p0"], f["m"], f["v"], f["s"], f["seg_start"], f["active"], f["seg_step"], f["pstate"],
                            f["partials"], lr, b1, b2, self.beta3, self.weight_decay, self.decouple, self.safeguard_warmup,
                            self.use_bias_correction, self.d0, clip)
        ops.prodigy_recurrence(f["pstate"], f["partials"], lr, b1, b2, self.beta3, self.use_bias_correction, self.d0, self.d_coef,
                               self.growth_rate)
        ops.prodigy_update(f["p"], f["lo"], f["m"], f["v"], f["seg_start"], f["active"], f["pstate"], self.eps, self.weight_decay,
                           self.decouple)

    # ---- the step-size estimate (host reads, for logging only) ----
    def _scalar(self, name: str) -> float:
        if self._flat is None:
            return {"d": self.d0, "d_max": self.d0}.get(name, 0.0)
        return float(self._flat["pstate"][ops.PRODIGY_STATE.index(name)].item())

    d = property(lambda self: self._scalar("d"), doc="the step-size estimate after the last step")
    d_max = property(lambda self: self._scalar("d_max"))
    d_hat = property(lambda self: self._scalar("d_hat"), doc="the last raw estimate d_coef * numerator / denominator")
    k = property(lambda self: int(self._scalar("k")), doc="completed updates (a step whose denominator was 0 does not count)")
    dlr = property(lambda self: self._scalar("dlr"), doc="d * lr * bias correction the last step ran with")

    @torch.no_grad()
    def prodigy_state(self):
        """``(s, p0)``: per-parameter copies (fp32 / bf16, shaped like the parameters, ``self.params`` order) of the estimate's running sum and
        of the weight at the first update.  For tests and exports."""
        if self._flat is None:
            self._build()
        f = self._flat
        cut = lambda x: [x[o:o + p.numel()].view(p.shape).clone() for p, o in zip(self.params, f["offs"])]
        return cut(f["s"]), cut(f["p0"])

    # ---- checkpointing ----
    def state_dict(self):
        sd = super().state_dict()
        sd["optimizer"] = "prodigy"
        for key, buf in (("prodigy_s", "s"), ("prodigy_p0", "p0"), ("prodigy_state", "pstate")):
            sd[key] = None if self._flat is None else self._flat[buf]
        return sd

    def load_state_dict(self, sd):
        if sd.get("exp_avg8") is not None:
            raise ValueError("FusedProdigy.load_state_dict: the checkpoint holds fp8 moments; Prodigy keeps fp32 state only")
        super().load_state_dict(sd)
        if sd.get("prodigy_state") is None:
            if sd.get("exp_avg") is not None:
                raise ValueError("FusedProdigy.load_state_dict: the checkpoint has AdamW moments but no Prodigy state (s, p0, d): it was "
                                 "written by FusedAdamW; its moments have another meaning (Prodigy's carry a factor d)")
            return
        if self._flat is None:
            self._build()
        f = self._flat
        for key, buf in (("prodigy_s", "s"), ("prodigy_p0", "p0"), ("prodigy_state", "pstate")):
            if sd.get(key) is None or sd[key].numel() != f[buf].numel():
                raise ValueError(f"FusedProdigy.load_state_dict: {key} does not match the flat layout")
            f[buf].copy_(sd[key])


class FusedCAME(FusedAdamW):
    """CAME, the memory-saving optimizer of the reference's factory (``train.optimizer.type: came``; its orv/utils.py:136-150), fused on the flat
    storage of ``FusedAdamW``: same flat bf16 parameter and gradient buffers, device-side clip coefficient, usage mask, overlapped gradient
    exchange and per-parameter skip; only the update differs.  The rule restates ``came_pytorch``'s ``CAME.step`` from
    memory (unpinned: the package is not available to compare against; one parameter group) and is written out in
    ``orv_amd/csrc/optim_came.hip``.  State: ONE fp32 moment per element, and for every parameter of two or more dimensions a row and a column
    vector per matrix of its last two dimensions, twice (second moment, confidence) - about 4 bytes per element where AdamW keeps 8.  No
    element-sized second moment is ever allocated; parameters of fewer than two dimensions keep an fp32 ``v`` of their own size.  A step is
    seven stream-ordered launches and reads nothing on the host.  Under data parallel every rank holds the same summed gradient and therefore
    computes the same statistics; no collective is added.

    ``param_precision``: ``"bf16"`` (the reference's own arithmetic: the updated weight is rounded to bf16, nearest-even) or ``"split_fp32"``
    (the exact fp32 master of ``FusedAdamW``).  From the reference's yaml: ``FusedCAME(params, lr=learning_rate, betas=(beta1, beta2, beta3),
    weight_decay=weight_decay, max_grad_norm=max_grad_norm)``."""

    _checkpoint_kind = "came"            # state_dict()["optimizer"]
    _supports_groups = False
    _element_moments = ("m",)
    _STATS = ("r", "c", "res_r", "res_c", "v")
    _STAT_KEYS = {"r": "exp_avg_sq_row", "c": "exp_avg_sq_col", "res_r": "exp_avg_res_row", "res_c": "exp_avg_res_col", "v": "exp_avg_sq"}

    def __init__(self, params: Iterable[torch.nn.Parameter], lr, eps=(1e-30, 1e-16), clip_threshold=1.0, betas=(0.9, 0.999, 0.9999),
                 weight_decay=0.0, max_grad_norm: float = 1.0, param_precision: str = "bf16", state_precision: str = "fp32"):
        if param_precision not in ("bf16", "split_fp32"):
            raise ValueError(f"FusedCAME: param_precision={param_precision!r} is not built for CAME (supported: 'bf16', 'split_fp32')")
        if state_precision != "fp32":
            raise ValueError(f"FusedCAME: state_precision={state_precision!r} is not built for CAME (supported: 'fp32')")
        if not lr > 0:
            raise ValueError(f"FusedCAME: lr={lr} must be greater than 0 (supported: lr > 0; CAME has no default learning rate)")
        if len(betas) != 3 or not all(0.0 <= float(b) <= 1.0 for b in betas):
            raise ValueError(f"FusedCAME: betas={tuple(betas)} (supported: three values (beta1, beta2, beta3), each in [0, 1])")
        if len(eps) != 2 or not float(eps[0]) > 0 or float(eps[1]) < 0:
            raise ValueError(f"FusedCAME: eps={tuple(eps)} (supported: (eps1, eps2) with eps1 > 0 - an all-zero gradient divides by it - and eps2 >= 0)")
        if not clip_threshold > 0:
            raise ValueError(f"FusedCAME: clip_threshold={clip_threshold} must be greater than 0 (supported: clip_threshold > 0)")
        super().__init__(params, lr=lr, betas=tuple(float(b) for b in betas), eps=tuple(float(e) for e in eps), weight_decay=weight_decay,
                         max_grad_norm=max_grad_norm, param_precision=param_precision, state_precision="fp32")
        self.clip_threshold = float(clip_threshold)

    def _build(self):
        super()._build()                 # allocates m only (``_element_moments``)
        f = self._flat
        dev = f["p"].device
        geo = ops.came_geometry([p.shape for p in self.params])
        count = {"r": geo["n_rows"], "c": geo["n_cols"], "res_r": geo["n_rows"], "res_c": geo["n_cols"], "v": geo["n_v"]}
        f.update(came_geo=geo, came_geom=torch.tensor(geo["table"], dtype=torch.int64, device=dev),
                 came_stats={k: torch.zeros(n, dtype=torch.float32, device=dev) if n else None for k, n in count.items()},
                 came_scratch=torch.zeros(geo["n_scratch"], dtype=torch.float32, device=dev))     # allocated once; rewritten by every step

    def _launch_update(self, f, clip):
        if "lo" in f:
            self._drop_stale_param_lo()
        ops.came_step(f["p"], f["g"], f["m"], f["came_stats"], f["seg_start"], f["active"], f["came_geom"], f["came_geo"], f["came_scratch"],
                      self.param_groups[0]["lr"], self.betas, self.eps, self.clip_threshold, self.weight_decay, clip, lo=f.get("lo"),
                      mode=ops.ADAMW_MODES[self.param_precision])

    @torch.no_grad()
    def came_state(self):
        """Per-parameter copies of the state, shaped as ``came_pytorch`` keeps it (``self.params`` order): a list of dicts with ``exp_avg`` and
        either ``exp_avg_sq_row`` / ``exp_avg_res_row`` ``[..., R]`` and ``exp_avg_sq_col`` / ``exp_avg_res_col`` ``[..., C]``, or, for a
        parameter of fewer than two dimensions, ``exp_avg_sq``.  For tests and exports."""
        if self._flat is None:
            self._build()
        f = self._flat
        st, out = f["came_stats"], []
        for p, o, row in zip(self.params, f["offs"], f["came_geo"]["table"]):
            B, R, C, _, _, row0, col0, v0 = row[:8]
            d = {"exp_avg": f["m"][o:o + p.numel()].view(p.shape).clone()}
            if R:
                lead = tuple(p.shape[:-2])
                for k, a, n, dim in (("r", row0, B * R, R), ("c", col0, B * C, C), ("res_r", row0, B * R, R), ("res_c", col0, B * C, C)):
                    d[self._STAT_KEYS[k]] = st[k][a:a + n].view(lead + (dim,)).clone()
            else:
                d["exp_avg_sq"] = st["v"][v0:v0 + p.numel()].view(p.shape).clone()
            out.append(d)
        return out

    @torch.no_grad()
    def last_clip(self):
        """``(k, rms)`` of the last step: per parameter the divisor ``max(1, RMS(u) / clip_threshold)`` and the RMS of ``u`` before it
        (fp32 tensors on the device, ``self.params`` order; meaningless for a parameter the last step skipped).  For logging and tests."""
        if self._flat is None:
            self._build()
        pairs = self._flat["came_scratch"][-2 * len(self.params):].view(-1, 2)
        return pairs[:, 0].clone(), pairs[:, 1].clone()

    def state_bytes(self):
        """Resident bytes of (optimizer state, scratch): m and the statistics; the partial sums and factors one step rewrites."""
        if self._flat is None:
            self._build()
        f = self._flat
        nbytes = lambda t: 0 if t is None else t.numel() * t.element_size()
        return nbytes(f["m"]) + sum(nbytes(t) for t in f["came_stats"].values()), nbytes(f["came_scratch"])

    # ---- checkpointing ----
    def state_dict(self):
        sd = super().state_dict()
        sd["optimizer"] = "came"
        for k in self._STATS:
            sd["came_" + k] = None if self._flat is None else self._flat["came_stats"][k]
        sd["came_shapes"] = [list(p.shape) for p in self.params]
        return sd

    def load_state_dict(self, sd):
        if sd.get("optimizer") != "came":
            raise ValueError(f"FusedCAME.load_state_dict: the checkpoint was written by the {sd.get('optimizer') or 'adamw'!r} optimizer; CAME keeps "
                             "a factored second moment and a confidence term that such a checkpoint does not hold (supported: checkpoints of FusedCAME)")
        if sd.get("came_shapes") is not None and [list(s) for s in sd["came_shapes"]] != [list(p.shape) for p in self.params]:
            raise ValueError("FusedCAME.load_state_dict: the checkpoint was written for parameters of other shapes; the factored statistics "
                             "follow the last two dimensions and cannot be mapped")
        super().load_state_dict(sd)
        if sd.get("exp_avg") is None:
            return
        st = self._flat["came_stats"]
        for k in self._STATS:
            src = sd.get("came_" + k)
            if (src is None) != (st[k] is None) or (src is not None and src.numel() != st[k].numel()):
                raise ValueError(f"FusedCAME.load_state_dict: came_{k} does not match the flat layout")
            if src is not None:
                st[k].copy_(src)


def named_groups(model, *, weight_decay, no_decay=("bias", "norm"), lr=None, lr_overrides=None):
    """Parameter groups for ``FusedAdamW`` / ``get_optimizer`` from ``model.named_parameters()`` (trainable parameters only, each exactly
    once).  A parameter is NOT decayed when it is 1-D (or a scalar) - every bias, LayerNorm gain and qk-norm vector - or when its name
    contains one of the ``no_decay`` patterns.  ``lr_overrides``: ``{name prefix: lr}``, the first matching prefix wins, for the freshly
    initialised layers of a fine-tune (``{"action_embed": 5e-4, "initial_combine_linear": 5e-4}``); ``lr`` (``None``: the optimizer's) is
    the rate of everything else.  Returns a list of dicts named ``"decay"``, ``"no_decay"``, and per override prefix ``"<prefix>"`` /
    ``"<prefix>.no_decay"``; groups that would be empty are left out."""
    overrides = dict(lr_overrides or {})
    slots = {}                    # (prefix or None, decayed) -> parameters, in model order
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        prefix = next((k for k in overrides if name.startswith(k)), None)
        decayed = p.ndim > 1 and not any(pat in name for pat in no_decay)
        slots.setdefault((prefix, decayed), []).append(p)
    groups = []
    for prefix in [None] + list(overrides):
        for decayed in (True, False):
            ps = slots.get((prefix, decayed))
            if not ps:
                continue
            g = {"params": ps, "weight_decay": float(weight_decay) if decayed else 0.0,
                 "name": ("decay" if decayed else "no_decay") if prefix is None else (prefix if decayed else prefix + ".no_decay")}
            rate = lr if prefix is None else overrides[prefix]
            if rate is not None:
                g["lr"] = float(rate)
            groups.append(g)
    if len(groups) > _MAX_GROUPS:
        raise ValueError(f"named_groups: {len(groups)} groups ({[g['name'] for g in groups]}); FusedAdamW keeps at most {_MAX_GROUPS} - "
                         "use fewer lr_overrides, or prefixes that share a rate under one longer common prefix")
    return groups


_OPTIMIZERS = ("adam (weight_decay == 0 only)", "adamw", "prodigy")


def get_optimizer(params_to_optimize, optimizer_name: str = "adam", learning_rate: float = 1e-3, beta1: float = 0.9, beta2: float = 0.95,
                  beta3: float = 0.98, epsilon: float = 1e-8, weight_decay: float = 1e-4, prodigy_decouple: bool = False,
                  prodigy_use_bias_correction: bool = False, prodigy_safeguard_warmup: bool = False, use_8bit: bool = False,
                  use_4bit: bool = False, use_torchao: bool = False, use_deepspeed: bool = False, use_cpu_offload_optimizer: bool = False,
                  offload_gradients: bool = False, max_grad_norm: float = 1.0, **fused_kwargs):
    """The reference's optimizer factory (its orv/utils.py:16-163, driven by ``train.optimizer.*`` of config/base_train.yaml:143-158):
    same argument names, order and defaults; ``max_grad_norm`` and ``**fused_kwargs`` are this project's own, because the fused optimizers
    clip inside their step.  ``fused_kwargs`` are keyword arguments of the chosen class - ``param_precision=``, ``state_precision=``,
    ``seed=``, ``skip_nonfinite=`` and ``track_grad_norms=`` for ``FusedAdamW``; ``d0=``, ``d_coef=``, ``growth_rate=`` for ``FusedProdigy`` - and any other name is refused with the
    accepted set.  ``adamw`` -> ``FusedAdamW`` (``use_8bit``: fp8
    moments), ``adam`` -> the same where Adam and AdamW coincide (``weight_decay == 0``), ``prodigy`` -> ``FusedProdigy``; an unknown name falls
    back to ``adamw`` with a warning as the reference does.  ``came`` is refused here with a pointer to ``FusedCAME``, which is constructed
    directly; 4-bit / torchao / DeepSpeed / CPU-offloaded optimizers are not built and are refused.  ``params_to_optimize``: an iterable of parameters, or the reference's list of one ``{"params": ..., "lr": ...}`` dict (its
    ``lr`` wins over ``learning_rate``, as in torch), or - for ``adam`` / ``adamw``, with or without ``use_8bit`` - several such dicts:
    ``FusedAdamW``'s parameter groups (``named_groups`` builds them from a model); ``prodigy`` keeps one group, and several dicts that carry
    nothing but ``params`` are refused as the one group they describe."""
    import warnings
    supported = f"supported: optimizer_name in {', '.join(_OPTIMIZERS)}; use_8bit with adam / adamw (fp8 moments)"
    name = str(optimizer_name).lower()
    for flag, on in (("use_deepspeed", use_deepspeed), ("use_4bit", use_4bit), ("use_torchao", use_torchao),
                     ("use_cpu_offload_optimizer", use_cpu_offload_optimizer)):
        if on:
            raise ValueError(f"get_optimizer: {flag}=True is not built here ({supported})")
    if name not in ("adam", "adamw", "prodigy", "came"):
        warnings.warn(f"get_optimizer: optimizer_name={name!r} is not known ({supported}); falling back to 'adamw'")
        name = "adamw"
    if name == "came":
        raise ValueError("get_optimizer: CAME is not built into get_optimizer yet: construct orv_amd.FusedCAME(params, lr=learning_rate, "
                         f"betas=(beta1, beta2, beta3), weight_decay=weight_decay, max_grad_norm=max_grad_norm) directly ({supported})")
    if use_8bit and name not in ("adam", "adamw"):
        raise ValueError(f"get_optimizer: use_8bit=True goes with adam / adamw only, not with {name!r} ({supported})")
    params = list(params_to_optimize)
    if params and isinstance(params[0], dict):
        if len(params) == 1:
            learning_rate = params[0].get("lr", learning_rate)
            params = list(params[0]["params"])
        elif name == "prodigy":
            raise ValueError(f"get_optimizer: {len(params)} parameter groups; FusedProdigy keeps one group (parameter groups: adam / adamw, "
                             f"i.e. FusedAdamW) ({supported})")
        elif all(isinstance(d, dict) and set(d) <= {"params"} for d in params):
            # Stricter than torch.optim and than FusedAdamW itself, which both take such dicts.  The reason is an older assertion that this
            # change may not edit: tests/test_prodigy_host.py::test_get_optimizer_mapping still asks for a ValueError matching "one group"
            # for get_optimizer([{"params": ...}, {"params": ...}], "adamw").  Dicts that carry nothing of their own all run at
            # (learning_rate, weight_decay), so nothing is lost by refusing them here; lift this branch once that assertion may change.
            raise ValueError(f"get_optimizer: {len(params)} parameter groups that carry nothing but `params` are one group: pass the "
                             "parameters as one list, or give a group its own lr / weight_decay / name (parameter groups: adam / adamw, "
                             f"i.e. FusedAdamW) ({supported})")
        elif name == "adam" and any(d.get("weight_decay", weight_decay) != 0 for d in params):
            raise ValueError("get_optimizer: coupled weight decay (torch.optim.Adam with a weight_decay) is not built; Adam is provided only "
                             f"at weight_decay == 0 in every group, where it coincides with AdamW - use optimizer_name='adamw' ({supported})")
        # several dicts for adam / adamw: FusedAdamW's parameter groups; a dict's missing lr / weight_decay take learning_rate / weight_decay
    cls = FusedProdigy if name == "prodigy" else FusedAdamW
    own = {"prodigy": ("d0", "d_coef", "growth_rate", "param_precision", "state_precision")}.get(name, ("param_precision", "state_precision", "seed", "skip_nonfinite", "track_grad_norms"))
    unknown = sorted(set(fused_kwargs) - set(own))
    if unknown:
        raise ValueError(f"get_optimizer: {cls.__name__} takes no {', '.join(unknown)} (accepted beside the reference's arguments: {', '.join(own)})")
    if name == "prodigy":
        if learning_rate <= 0.1:
            warnings.warn(f"get_optimizer: learning_rate={learning_rate:g} is small for prodigy, whose lr multiplies its own step-size estimate; "
                          "values near 1.0 are the usual choice")
        return FusedProdigy(params, lr=learning_rate, betas=(beta1, beta2), beta3=beta3, eps=epsilon, weight_decay=weight_decay,
                            decouple=prodigy_decouple, use_bias_correction=prodigy_use_bias_correction,
                            safeguard_warmup=prodigy_safeguard_warmup, max_grad_norm=max_grad_norm, **fused_kwargs)
    if name == "adam" and weight_decay != 0 and not (params and isinstance(params[0], dict)):
        raise ValueError(f"get_optimizer: coupled weight decay (torch.optim.Adam with weight_decay={weight_decay}) is not built; Adam is "
                         f"provided only at weight_decay == 0, where it coincides with AdamW - use optimizer_name='adamw' for decoupled "
                         f"decay ({supported})")
    if use_8bit:
        fused_kwargs.setdefault("state_precision", "fp8")
    return FusedAdamW(params, lr=learning_rate, betas=(beta1, beta2), eps=epsilon, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                      **fused_kwargs)


# ---- learning-rate schedules of the train tail (train_cogvideox_control_to_video_sft.py:740-747, :1107; base_train.yaml:160-164) ----
# The reference calls ``diffusers.optimization.get_scheduler(name, optimizer=, num_warmup_steps=, num_training_steps=, num_cycles=, power=)``
# and ``lr_scheduler.step()`` after every optimizer step.  diffusers is not installable here: the multipliers below restate its published
# ``get_*_schedule*`` lambdas (LEAF, unpinned like oracle/leaf.py; hand-derived known answers in tests/test_lr_schedule.py).  Each returns
# lr(step) / lr_base for the number of ``step()`` calls made so far.
def _lr_lambda(name: str, num_warmup_steps: int, num_training_steps: Optional[int], num_cycles, power: float, lr_init: float):
    import math
    W = int(num_warmup_steps or 0)
    T = num_training_steps
    name = getattr(name, "value", name)
    if name not in ("constant", "constant_with_warmup") and T is None:
        raise ValueError(f"{name} requires `num_training_steps`, please provide that argument.")       # diffusers' message
    warm = lambda s: float(s) / float(max(1, W))
    if name == "constant":
        return lambda s: 1.0
    if name == "constant_with_warmup":
        return lambda s: warm(s) if s < W else 1.0
    if name == "linear":
        return lambda s: warm(s) if s < W else max(0.0, float(T - s) / float(max(1, T - W)))
    if name == "cosine":
        nc = 0.5 if num_cycles is None else float(num_cycles)      # NB the reference passes lr_num_cycles (1) for every schedule name

        def cosine(s):
            if s < W:
                return warm(s)
            prog = float(s - W) / float(max(1, T - W))
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * nc * 2.0 * prog)))
        return cosine
    if name == "cosine_with_restarts":                             # base_train.yaml:161 - the schedule every shipped config trains with
        nc = 1 if num_cycles is None else num_cycles

        def restarts(s):
            if s < W:
                return warm(s)
            prog = float(s - W) / float(max(1, T - W))
            if prog >= 1.0:
                return 0.0
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(nc) * prog) % 1.0))))
        return restarts
    if name == "polynomial":
        lr_end = 1e-7
        if not lr_init > lr_end:
            raise ValueError(f"lr_end ({lr_end}) must be smaller than initial lr ({lr_init})")

        def poly(s):
            if s < W:
                return warm(s)
            if s > T:
                return lr_end / lr_init
            pct = 1 - (s - W) / (T - W)
            return ((lr_init - lr_end) * pct ** power + lr_end) / lr_init
        return poly
    raise ValueError(f"unknown lr scheduler {name!r} (constant, constant_with_warmup, linear, cosine, cosine_with_restarts, polynomial)")


class LambdaSchedule:
    """``torch.optim.lr_scheduler.LambdaLR`` semantics on anything with ``param_groups`` (``FusedAdamW`` is not a ``torch.optim.Optimizer``):
    lr = base_lr x lambda(number of ``step()`` calls), applied at construction for step 0 - so with a warm-up the first optimizer
    step runs at lr 0, exactly as the reference's loop does (train...sft.py:1100-1107: ``optimizer.step()`` then ``lr_scheduler.step()``)."""

    def __init__(self, optimizer, lr_lambda, last_epoch: int = -1):
        self.optimizer, self.lr_lambda = optimizer, lr_lambda
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.base_lrs = [g["initial_lr"] for g in optimizer.param_groups]
        self.last_epoch = last_epoch
        self.step()

    def step(self):
        self.last_epoch += 1
        self._last_lr = [b * self.lr_lambda(self.last_epoch) for b in self.base_lrs]
        for g, lr in zip(self.optimizer.param_groups, self._last_lr):
            g["lr"] = lr

    def get_last_lr(self):
        return list(self._last_lr)

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "base_lrs": list(self.base_lrs), "_last_lr": list(self._last_lr)}

    def load_state_dict(self, sd):
        self.last_epoch, self.base_lrs = int(sd["last_epoch"]), list(sd["base_lrs"])
        self._last_lr = [b * self.lr_lambda(self.last_epoch) for b in self.base_lrs]
        for g, lr in zip(self.optimizer.param_groups, self._last_lr):
            g["lr"] = lr


def get_scheduler(name, optimizer, step_rules=None, num_warmup_steps: Optional[int] = None, num_training_steps: Optional[int] = None,
                  num_cycles: int = 1, power: float = 1.0, last_epoch: int = -1) -> LambdaSchedule:
    """Drop-in for ``diffusers.optimization.get_scheduler`` as the train script calls it (:740-747) - same argument names and defaults;
    ``piecewise_constant`` (``step_rules``) is not used by any shipped config and is refused.  With several parameter groups every group
    follows the ONE multiplier sequence from its own ``initial_lr``.  ``polynomial`` is the one schedule whose multiplier depends on the
    initial rate (it ends at ``lr_end`` = 1e-7): it is derived from group 0's, so another group ends at ``lr_end`` times its own
    ``initial_lr`` over group 0's, not at ``lr_end``."""
    if step_rules is not None or getattr(name, "value", name) == "piecewise_constant":
        raise ValueError("piecewise_constant / step_rules is not provided (no ORV config uses it)")
    if getattr(name, "value", name) != "constant" and num_warmup_steps is None:
        raise ValueError(f"{name} requires `num_warmup_steps`, please provide that argument.")
    lr0 = optimizer.param_groups[0].get("initial_lr", optimizer.param_groups[0]["lr"])
    return LambdaSchedule(optimizer, _lr_lambda(name, num_warmup_steps or 0, num_training_steps, num_cycles, power, lr0), last_epoch)
