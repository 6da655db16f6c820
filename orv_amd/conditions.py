"""Control encoding: the rendered depth and label maps of ``orv_amd.occupancy`` (or uint8 video frames) -> the VAE moments the denoise
and training paths start from.

Mirrors (behaviour, not code) the two halves the reference spreads over two files:
* preparation, ``orv/dataset/dataset.py:225-295`` and ``:852-888``: a per-frame torchvision loop of two resizes and two centre crops
  (antialiased bilinear for depth, nearest for labels), clamp and scale for depth, the 60-colour palette for labels;
* encoding, ``orv/dataset/encode_dataset.py:801-916``: depth repeated to 3 channels, one ``vae._encode`` per view, views joined along the
  frame axis.
Here the preparation is ONE kernel launch per tensor (``ops.cond_prepare``, ``csrc/conditions.hip``) that writes the bf16 channels-last
tensor the VAE encoder's first convolution reads, and the views are the batch dimension of one encode call.  The arithmetic contract is
DESIGN.md §15.  There is no CPU path: numpy arrays are uploaded, CPU tensors are refused.
"""
from __future__ import annotations

import colorsys
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

MAX_DOWNSCALE = 4           # per axis and stage: bounds the antialias filter at 10 taps
NUM_COLORS = 60


def generate_colors(n: int = NUM_COLORS):
    """``n`` RGB triples: ``int(c * 255)`` of ``colorsys.hsv_to_rgb(i / n, 0.75, 0.95)`` (``prepare_dataset.py:1458-1466``)."""
    return [tuple(int(c * 255) for c in colorsys.hsv_to_rgb(i / n, 0.75, 0.95)) for i in range(n)]


def palette60() -> np.ndarray:
    """The label palette, float32 [60, 3] in 0..255: ``generate_colors(60)`` with the last entry black (``dataset.py:243-245``)."""
    colors = generate_colors(NUM_COLORS)
    colors[-1] = (0, 0, 0)
    return np.array(colors, dtype=np.float32)


def _crop_offset(size: int, crop: int) -> int:
    return int(round((size - crop) / 2.0))          # torchvision's centre crop: Python's round, half to even


def _pair(v, name) -> Tuple[int, int]:
    v = tuple(int(s) for s in v)
    if len(v) != 2 or min(v) < 1:
        raise ValueError(f"orv_amd.conditions: `{name}` must be (height, width) of positive integers (got {v})")
    return v


@dataclass(frozen=True)
class Stage:
    """Resize ``in_size`` to ``resize``, then centre crop to ``crop`` at ``(top, left)``."""
    in_size: Tuple[int, int]
    resize: Tuple[int, int]
    crop: Tuple[int, int]
    top: int
    left: int

    def ints(self):
        return (*self.resize, self.top, self.left, *self.crop)


class ResizePlan:
    """One or two stages of (resize, centre crop) from ``source_size``; every size is (height, width).  ``stages`` lists
    ``(resize, crop)`` pairs.  A crop larger than its input (torchvision would pad) and a downscale beyond 4x per axis and stage are
    refused."""

    def __init__(self, source_size, stages: Sequence[Tuple[Tuple[int, int], Tuple[int, int]]]):
        self.source_size = _pair(source_size, "source_size")
        if len(stages) not in (1, 2):
            raise ValueError(f"orv_amd.conditions: a plan has 1 or 2 stages (got {len(stages)})")
        cur, built = self.source_size, []
        for k, (resize, crop) in enumerate(stages):
            resize, crop = _pair(resize, "resize"), _pair(crop, "crop")
            if crop[0] > resize[0] or crop[1] > resize[1]:
                raise ValueError(f"orv_amd.conditions: stage {k + 1} crops {crop} out of {resize}; supported: a crop no larger than its "
                                 "input (torchvision would pad; no shipped config does)")
            if cur[0] > MAX_DOWNSCALE * resize[0] or cur[1] > MAX_DOWNSCALE * resize[1]:
                raise ValueError(f"orv_amd.conditions: stage {k + 1} resizes {cur} to {resize}; supported: at most {MAX_DOWNSCALE}x "
                                 "downscale per axis and stage")
            built.append(Stage(cur, resize, crop, _crop_offset(resize[0], crop[0]), _crop_offset(resize[1], crop[1])))
            cur = crop
        self.stages = tuple(built)
        self.out_size = cur

    @staticmethod
    def new_size(ori_size, video_size) -> Tuple[int, int]:
        """``(new_h, new_w)`` of ``dataset.py:225-233``, with its truncations."""
        ori_h, ori_w = _pair(ori_size, "ori_size")
        vh, vw = _pair(video_size, "video_size")
        if vh % 8 or vw % 8:
            raise ValueError(f"orv_amd.conditions: video_size = {(vh, vw)}; supported: height and width multiples of 8 (the VAE's spatial factor)")
        if vw / vh < ori_w / ori_h:
            return vh, int(ori_w * (vh / ori_h))
        return int(ori_h * (vw / ori_w)), vw

    @classmethod
    def for_controls(cls, ori_size, video_size, source_size, render_size=None) -> "ResizePlan":
        """Depth and label maps (``dataset.py:277-295``): ``Resize(render_h)`` (shorter edge to ``render_h``, longer edge
        ``int(render_h * long / short)``) and ``CenterCrop(render_size)``, then ``Resize((new_h, new_w))`` and ``CenterCrop(video_size)``.
        ``render_size`` defaults to ``ori_size``; the reference's bridge override is ``render_size=(480, 640)``, ``ori_size=(256, 320)``."""
        new = cls.new_size(ori_size, video_size)
        render = _pair(ori_size if render_size is None else render_size, "render_size")
        h, w = _pair(source_size, "source_size")
        size = render[0]
        first = (size, int(size * w / h)) if h <= w else (int(size * h / w), size)
        return cls((h, w), [(first, render), (new, _pair(video_size, "video_size"))])

    @classmethod
    def for_frames(cls, ori_size, video_size, source_size=None) -> "ResizePlan":
        """Video frames and images (``dataset.py:255-275``): ``Resize((new_h, new_w))`` and ``CenterCrop(video_size)`` alone."""
        new = cls.new_size(ori_size, video_size)
        return cls(ori_size if source_size is None else source_size, [(new, _pair(video_size, "video_size"))])

    def __repr__(self):
        body = "; ".join(f"{s.in_size} -> resize {s.resize} -> crop {s.crop} at ({s.top}, {s.left})" for s in self.stages)
        return f"ResizePlan({body})"


def _device_input(x, name):
    if isinstance(x, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError(f"orv_amd.conditions: `{name}` is a numpy array and no GPU is available to upload it to; there is no CPU path")
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"orv_amd.conditions: `{name}` must be a numpy array or a GPU tensor (got {type(x).__name__})")
    return x


def _index(index, n_src, device):
    """-> (int32 [n_out] on the device or None, leading shape of the result)."""
    if index is None:
        return None, (1, n_src)
    if isinstance(index, torch.Tensor) and index.is_cuda:
        idx = index
    else:
        idx = torch.as_tensor(np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index))
    if idx.dim() not in (1, 2) or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"orv_amd.conditions: `index` must be int32 / int64 [n_out] or [V, F] (got {idx.dtype} {tuple(idx.shape)})")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_src):
        raise IndexError(f"orv_amd.conditions: `index` runs from {int(idx.min())} to {int(idx.max())}; supported: 0 to {n_src - 1} (the source has {n_src} frames)")
    lead = tuple(idx.shape) if idx.dim() == 2 else (1, idx.numel())
    return idx.to(device=device, dtype=torch.int32).reshape(-1).contiguous(), lead


def _check_plan(x, plan):
    if not isinstance(plan, ResizePlan):
        raise TypeError(f"orv_amd.conditions: `plan` must be a ResizePlan (got {type(plan).__name__})")
    if x.dim() >= 3 and tuple(x.shape[1:3]) != plan.source_size:
        raise ValueError(f"orv_amd.conditions: the plan starts from {plan.source_size} but the input frames are {tuple(x.shape[1:3])}")


def _prepare(x, plan, index, out, interp, post, palette=None):
    if out not in ("nchw", "vae"):
        raise ValueError(f"orv_amd.conditions: out = {out!r}; supported: 'nchw' (fp32 [N, C, H, W]) or 'vae' (bf16 [V, F, H, W, 8])")
    _check_plan(x, plan)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        idx, lead = _index(index, x.shape[0], x.device)
    else:
        idx, lead = None, None                       # ops.cond_prepare refuses the tensor below
    res = ops.cond_prepare(x, [s.ints() for s in plan.stages], interp, post, idx, palette, out)
    return res if out == "nchw" else res.view(*lead, *res.shape[1:])


def prepare_depths(x, plan: ResizePlan, index=None, out: str = "nchw"):
    """Depth fp32 [N, h, w] (numpy or GPU tensor) -> ``clamp(resized, 0.01, 0.4) * 2.5``: fp32 [n_out, 1, H, W] or bf16 [V, F, H, W, 8]
    (the depth in channels 0-2).  ``index`` [n_out] or [V, F] picks the source frame of every output frame."""
    return _prepare(_device_input(x, "depths"), plan, index, out, "bilinear", "depth")


def prepare_labels(x, plan: ResizePlan, index=None, out: str = "nchw"):
    """Label ids uint8 [N, h, w] below 60 -> ``palette60()[id] / 255`` after a nearest resize: fp32 [n_out, 3, H, W] or bf16 [V, F, H, W, 8]."""
    refusal = "orv_amd.conditions: label id {} is outside the palette; supported: ids 0 to 59 (the reference raises IndexError)"
    if isinstance(x, np.ndarray) and x.size and int(x.max()) >= NUM_COLORS:        # still on the host: checked before the upload
        raise IndexError(refusal.format(int(x.max())))
    host = isinstance(x, np.ndarray)
    x = _device_input(x, "labels")
    palette = None
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8:
        if not host and x.numel() and int(x.max()) >= NUM_COLORS:           # one device reduction, one host read
            raise IndexError(refusal.format(int(x.max())))
        palette = torch.from_numpy(palette60()).to(x.device)
    elif isinstance(x, torch.Tensor) and x.is_cuda:
        raise RuntimeError(f"orv_amd.conditions: label ids must be torch.uint8 [N, h, w] (got {x.dtype})")
    return _prepare(x, plan, index, out, "nearest", None, palette)


def prepare_frames(x, plan: ResizePlan, index=None, out: str = "nchw", normalize: bool = True):
    """Video frames uint8 [N, h, w, 3] -> ``x / 255``, antialiased bilinear resize, crop, then ``(x - 0.5) / 0.5`` unless
    ``normalize=False``: fp32 [n_out, 3, H, W] or bf16 [V, F, H, W, 8]."""
    x = _device_input(x, "frames")
    if isinstance(x, torch.Tensor) and x.is_cuda and not (x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3):
        raise RuntimeError(f"orv_amd.conditions: frames must be torch.uint8 [N, h, w, 3] (got {x.dtype} {tuple(x.shape)})")
    return _prepare(x, plan, index, out, "bilinear", "normalize" if normalize else None)


def _join_views(moments, dtype):
    """[V, 2C, F', h, w] -> [1, 2C, V * F', h, w]: 'v c f h w -> 1 c (v f) h w'."""
    V, C2, Fl, h, w = moments.shape
    return moments.permute(1, 0, 2, 3, 4).reshape(1, C2, V * Fl, h, w).contiguous().to(dtype)


def _ids(ids, limit, name):
    ids = [int(i) for i in ids]
    if not ids or min(ids) < 0 or max(ids) >= limit:
        raise IndexError(f"orv_amd.conditions: {name} = {ids}; supported: a non-empty list of ids from 0 to {limit - 1}")
    return ids


def encode_controls(vae, render, frame_ids, view_ids=(0,), control_keys=("depth", "label"), ori_size=(256, 320), video_size=(320, 480),
                    render_size=None, dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """``render`` = the dict (or ``np.load`` result) of ``OccupancyScene.render_trajectory``: ``semantics`` uint8 [n_frame, n_view, h, w],
    ``depths`` fp32 [n_frame * n_view, h, w], ``is_labeled``.  -> ``{"depths": [1, 32, V * F', H / 8, W / 8], "labels": ...}``: the VAE
    moments of the prepared maps, views joined along frames - what ``pipe(controls_or_guidances=...)`` takes; ``x[0].permute(1, 0, 2, 3)``
    is the form ``load_latent_controls`` returns.  ``labels`` is left out when ``is_labeled`` is false."""
    unknown = set(control_keys) - {"depth", "label"}
    if unknown:
        raise ValueError(f"orv_amd.conditions: control_keys = {tuple(control_keys)}; supported: 'depth', 'label'")
    semantics = render["semantics"]
    if semantics.ndim != 4:
        raise ValueError(f"orv_amd.conditions: `semantics` must be [n_frame, n_view, h, w] (got {tuple(semantics.shape)})")
    n_frame, n_view, h, w = semantics.shape
    frames, views = _ids(frame_ids, n_frame, "frame_ids"), _ids(view_ids, n_view, "view_ids")
    index = torch.tensor([[f * n_view + v for f in frames] for v in views], dtype=torch.int32)       # [V, F]: the (v f) order
    plan = ResizePlan.for_controls(ori_size, video_size, (h, w), render_size)
    out = {}
    if "depth" in control_keys:
        depths = render["depths"]
        if depths.ndim == 4:
            depths = depths.reshape(-1, *depths.shape[2:])
        if tuple(depths.shape) != (n_frame * n_view, h, w):
            raise ValueError(f"orv_amd.conditions: `depths` must be [n_frame * n_view, h, w] = {(n_frame * n_view, h, w)} (got {tuple(depths.shape)})")
        out["depths"] = _join_views(vae.encode_channels_last(prepare_depths(depths, plan, index, out="vae")), dtype)
    if "label" in control_keys and bool(render["is_labeled"]):
        ids = semantics.reshape(n_frame * n_view, h, w)
        out["labels"] = _join_views(vae.encode_channels_last(prepare_labels(ids, plan, index, out="vae")), dtype)
    return out


def encode_frames(vae, frames_uint8, ori_size=None, video_size=(320, 480), n_view: int = 1, frame_ids: Optional[Sequence[int]] = None,
                  normalize: bool = True, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Video or image moments (``encode_dataset.py:821-861``): uint8 [n_view * F, h, w, 3] with the views along frames (``(v f)``) ->
    [1, 32, n_view * F', H / 8, W / 8], each view encoded on its own.  ``frame_ids`` picks frames of every view; ``ori_size`` defaults
    to the frames' own size."""
    x = _device_input(frames_uint8, "frames")
    if x.dim() != 4 or x.shape[0] % n_view:
        raise ValueError(f"orv_amd.conditions: frames must be [n_view * F, h, w, 3] with n_view = {n_view} (got {tuple(x.shape)})")
    per_view = x.shape[0] // n_view
    ids = list(range(per_view)) if frame_ids is None else _ids(frame_ids, per_view, "frame_ids")
    index = torch.tensor([[v * per_view + f for f in ids] for v in range(n_view)], dtype=torch.int32)
    plan = ResizePlan.for_frames(tuple(x.shape[1:3]) if ori_size is None else ori_size, video_size, tuple(x.shape[1:3]))
    return _join_views(vae.encode_channels_last(prepare_frames(x, plan, index, out="vae", normalize=normalize)), dtype)
