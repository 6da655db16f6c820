"""Label-map compositing for ORV's conditioning chain, on the MI355X: a video segmenter's per-object masks to the 2-D label image.

The last non-network step of the reference's label preparation is ``postprocess_labels`` / ``_postprocess_labels``
(``orv/dataset/prepare_dataset.py:1377-1486``): the segmenter's logits are thresholded on the GPU (``:1275-1279``), copied to the host as
``[n, H, W]`` booleans, written to disk, reloaded by a 16-process pool and painted with ``2 n`` boolean-index stores per frame, largest
mask first, in an order frozen from the first frame (``:1412-1444``).  This module is that step over the HIP kernels of
``csrc/labelmap.hip``; the masks, or the logits themselves, stay on the device, and the ``index`` image goes on to
``occupancy.project_labels`` as it is.

* ``mask_stats`` - ``detections.area`` and ``sv.mask_to_xyxy`` (``:1406-1420``) per (frame, mask).
* ``paint_order`` - ``np.flip(np.argsort(area))`` (``:1420``) with the order among equal areas fixed.
* ``compose`` - the two paint loops (``:1412-1444``): the uint8 label image and its colour preview.
* ``postprocess_labels`` - the frame loop of ``_postprocess_labels`` over the dicts the per-frame ``.npz`` files hold.

Every output is an integer and equal bit for bit to what the reference's statements produce; the contract is in DESIGN.md §18.  Forward only.
"""
from __future__ import annotations

import numpy as np
import torch

from . import conditions, ops

NUM_COLORS = 60                                      # len(colors60) of the reference: a label's colour is palette[label % 60]
MAX_DIM = 65535
CHANNEL_ORDERS = ("bgr", "rgb")
SUPPORTED = ("supported: a CUDA tensor masks [F,n,H,W] or [n,H,W] of torch.bool, torch.uint8 (set where nonzero) or torch.float32 (logits, set "
             "where x > threshold) without requires_grad, whose inner [H,W] plane is contiguous, with 1 <= H, W < 65536 (the F and n strides "
             "are free); label_ids [n] of an integer type with values in [0, 255]; order = distinct mask numbers in [0, n), at most n of "
             f"them; channel_order in {CHANNEL_ORDERS}; palette uint8 [60, 3]; forward only")


def _refuse(what: str):
    raise NotImplementedError(f"orv_amd.labelmap: {what} ({SUPPORTED})")


def _check_masks(masks):
    """-> (masks as [F,n,H,W], whether a frame axis was added)."""
    if not isinstance(masks, torch.Tensor):
        _refuse(f"`masks` is a {type(masks).__name__}, not a tensor")
    if masks.dtype not in ops.LM_DTYPES:
        _refuse(f"`masks` is {masks.dtype}, not bool, uint8 or float32")
    if masks.dim() not in (3, 4):
        _refuse(f"`masks` has shape {tuple(masks.shape)}: not [F,n,H,W] or [n,H,W]")
    if masks.requires_grad:
        _refuse("`masks` has requires_grad=True and there is no backward pass: detach it")
    single = masks.dim() == 3
    if single:
        masks = masks[None]
    H, W = masks.shape[2:]
    if H * W == 0:
        _refuse(f"`masks` has shape {tuple(masks.shape)}: H * W == 0")
    if H > MAX_DIM or W > MAX_DIM:
        _refuse(f"`masks` has planes of {H} x {W}: H or W >= 65536")
    if masks.numel() and ((W > 1 and masks.stride(3) != 1) or (H > 1 and masks.stride(2) != W)):
        _refuse(f"the inner [H,W] plane of `masks` is not contiguous (strides {masks.stride()}): copy it with .contiguous()")
    if not masks.is_cuda:                                              # last, so that every other refusal can be met without a device
        _refuse(f"`masks` is not a CUDA tensor (it is on {masks.device}); there is no CPU path")
    return masks, single


def _host_ints(v, name):
    if isinstance(v, torch.Tensor):
        if v.dtype.is_floating_point or v.is_complex() or v.dtype == torch.bool:
            _refuse(f"`{name}` is {v.dtype}, not an integer type")
        v = v.detach().cpu().numpy()
    v = np.asarray(v)
    if v.size == 0:
        v = v.astype(np.int64)
    if v.dtype.kind not in "iu":
        _refuse(f"`{name}` is {v.dtype}, not an integer type")
    if v.ndim != 1:
        _refuse(f"`{name}` has shape {v.shape}, not one dimension")
    return v.astype(np.int64)


def _check_label_ids(label_ids, n):
    ids = _host_ints(label_ids, "label_ids")
    if len(ids) != n:
        _refuse(f"`label_ids` holds {len(ids)} values for n = {n} masks")
    if len(ids) and (ids.min() < 0 or ids.max() > 255):
        _refuse(f"`label_ids` holds values outside [0, 255] (min {ids.min()}, max {ids.max()})")
    return ids


def _check_order(order, n):
    order = _host_ints(order, "order")
    if len(order) > n:
        _refuse(f"`order` names {len(order)} masks, more than n = {n}")
    if len(order) and (order.min() < 0 or order.max() >= n):
        _refuse(f"`order` holds a mask number outside [0, n = {n}) (min {order.min()}, max {order.max()})")
    if len(np.unique(order)) != len(order):
        _refuse("`order` names a mask twice")
    return order


def _check_palette(palette, channel_order):
    if channel_order not in CHANNEL_ORDERS:
        _refuse(f"channel_order = {channel_order!r}")
    if palette is None:
        palette = conditions.palette60().astype(np.uint8)             # exact: generate_colors yields ints in 0..255, the last entry black
    else:
        if isinstance(palette, torch.Tensor):
            palette = palette.detach().cpu().numpy()
        palette = np.asarray(palette)
        if palette.dtype != np.uint8 or palette.shape != (NUM_COLORS, 3):
            _refuse(f"`palette` is {palette.dtype} {list(palette.shape)}, not uint8 [60, 3] of (r, g, b)")
    return palette[:, ::-1] if channel_order == "bgr" else palette   # the reference stores color.as_bgr()


@torch.no_grad()
def mask_stats(masks, threshold=0.0):
    """``masks`` [F,n,H,W] (or [n,H,W]: one frame, and the results lose the frame axis) -> ``(area int64 [F,n], xyxy int64 [F,n,4])`` on the
    device: the count of set pixels (``detections.area`` when masks are given) and ``x_min, y_min, x_max, y_max``, inclusive, over them
    (``sv.mask_to_xyxy``); an empty mask gives zeros."""
    masks, single = _check_masks(masks)
    area, xyxy = ops.lm_mask_stats(masks, threshold)
    return (area[0], xyxy[0]) if single else (area, xyxy)


def paint_order(area0):
    """The areas of one frame's masks [n] -> the paint order, numpy int64 [n]: ``np.flip(np.argsort(area0))`` with the sort stable, so the
    largest mask is painted first and the smallest wins a pixel; among equal areas the larger mask number is painted first and the smaller
    one wins (the reference's sort leaves that order open; the vote of ``voxelize`` breaks ties the same way)."""
    if isinstance(area0, torch.Tensor):
        area0 = area0.detach().cpu().numpy()
    area0 = np.asarray(area0)
    if area0.ndim != 1:
        raise ValueError(f"orv_amd.labelmap: `area0` has shape {area0.shape}; expected the [n] areas of one frame")
    return np.flip(np.argsort(area0, kind="stable")).astype(np.int64)


@torch.no_grad()
def compose(masks, label_ids, order=None, threshold=0.0, channel_order="bgr", palette=None):
    """``masks`` [F,n,H,W] (or [n,H,W]: one frame, and the images lose the frame axis), ``label_ids`` [n] in [0, 255] ->
    ``(index uint8 [F,H,W], color uint8 [F,H,W,3], order int64 [m])``, the images on the device and the order on the host.

    ``index`` starts at 255 and ``color`` at 0; for ``j`` in ``order``, in sequence, where mask ``j`` is set ``index = label_ids[j]`` and
    ``color = palette[label_ids[j] % 60]`` written as (b, g, r), or (r, g, b) with ``channel_order="rgb"``.  ``order=None`` takes
    ``paint_order`` of the first frame's areas (one host read) and uses it for every frame; masks an ``order`` does not name are never
    painted.  ``palette`` is uint8 [60, 3] of (r, g, b), ``conditions.palette60()`` by default."""
    masks, single = _check_masks(masks)
    n = masks.shape[1]
    ids = _check_label_ids(label_ids, n)
    pal = _check_palette(palette, channel_order)
    if order is None:
        order = paint_order(ops.lm_mask_stats(masks[:1], threshold)[0][0]) if n else np.zeros(0, np.int64)
    else:
        order = _check_order(order, n)
    index, color = ops.lm_compose(masks, order.tolist(), ids.tolist(), pal.tolist(), threshold)
    return (index[0], color[0], order) if single else (index, color, order)


def _frame_masks(masks, device):
    if isinstance(masks, np.ndarray):
        if masks.dtype not in (np.bool_, np.uint8, np.float32):
            masks = masks.astype(np.bool_)                            # the reference's own cast (:1396)
        masks = torch.from_numpy(np.ascontiguousarray(masks))
    if isinstance(masks, torch.Tensor) and not masks.is_cuda:
        masks = masks.to(device)
    return masks


@torch.no_grad()
def postprocess_labels(frames, order=None, device="cuda"):
    """The frame loop of ``_postprocess_labels``: ``frames`` = a list of dicts with ``masks`` [n,H,W] and ``label_ids`` [n] (numpy, as the
    per-frame ``.npz`` holds them, or device tensors) -> the same list, every dict given ``annotated_frame_index`` uint8 [H,W] and
    ``annotated_frame_color`` uint8 [H,W,3] as numpy.  A frame that already has both keys is skipped before the order is taken
    (``:1399-1404``), so on a resumed trajectory the order comes from the first frame that is not annotated yet: a defect of the reference
    that ``order=`` avoids by pinning the order.  A frame with fewer masks than the order names raises ``ValueError``; one with more leaves
    the extra masks unpainted."""
    if order is not None:
        order = _host_ints(order, "order")
        if len(order) and order.min() < 0:
            _refuse(f"`order` holds a negative mask number ({order.min()})")
        if len(np.unique(order)) != len(order):
            _refuse("`order` names a mask twice")
    for t, frame in enumerate(frames):
        if "annotated_frame_color" in frame and "annotated_frame_index" in frame:
            continue
        n = len(frame["masks"])
        if order is not None and len(order) and int(order.max()) >= n:
            raise ValueError(f"orv_amd.labelmap: frame {t} holds {n} masks but the paint order names mask {int(order.max())} (the reference "
                             "fails there with an IndexError inside its pool)")
        index, color, used = compose(_frame_masks(frame["masks"], device), frame["label_ids"], order=order)
        if order is None:
            order = used
        frame["annotated_frame_index"], frame["annotated_frame_color"] = index.cpu().numpy(), color.cpu().numpy()
    return frames
