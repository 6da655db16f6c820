"""Video metrics: per-frame PSNR and SSIM of decoded frames against their ground truth on the GPU, and the closed-form tail of FID /
FVD (the Frechet distance between two feature sets) on the host.

Mirrors (behaviour, not code) the last stage of the reference's workflow, ``orv/pipeline/compute_metrics.py``:
* ``_compute_psnr_ssim`` (``:38-80``): per frame ``cv2.resize(..., (320, 256), INTER_LINEAR)`` of both images, then skimage's
  ``peak_signal_noise_ratio`` and ``structural_similarity(channel_axis=-1, data_range=1.)`` on the CPU, over 64 threads.  Here that is
  ``frame_metrics`` / ``psnr_ssim``: two kernel launches per clip (``ops.frame_metrics``, ``csrc/metrics.hip``) that read the frames where
  they are - uint8 or fp32, ``[N, H, W, 3]`` or the pipeline's ``'pt'`` layout ``[N, 3, H, W]``, a width slice of either - and never write
  the resized images to memory.  There is no CPU path: numpy arrays are uploaded, CPU tensors are refused.
* ``_calculate_frechet_distance`` (``:171-204``) and ``_frechet_distance`` (``:278-293``): ``calculate_frechet_distance`` and
  ``frechet_distance``, numpy and ``scipy.linalg.sqrtm`` on the host, the only CPU code in this module.  The feature networks
  (InceptionV3, I3D) stay delegated objects, as do video reading and the CSV writer.

The arithmetic contract is DESIGN.md §16.  Parity statement: ``cv2`` and ``skimage`` could not be run where this was written, so parity
with them is UNPINNED.  The kernel is held bit for bit to the contract and its numpy restatement (``tests/metrics_ref.py``); the
contract's SSIM is tied to ``scipy.ndimage.uniform_filter``, the filter skimage itself calls, in fp64 on the CPU.  Two things are recalled
from memory and not checkable: cv2's coefficient formula, and cv2's switch from ``INTER_LINEAR`` to ``INTER_AREA`` at an exact 2 x 2
downscale (the same average mathematically; its rounding is unverified).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops

SUPPORTED = ("supported: numpy arrays or GPU tensors, torch.uint8 (divided by 255) or torch.float32, N frames x 3 channels as [N, H, W, 3] "
             "(layout='nhwc') or [N, 3, H, W] (layout='nchw'), without grad, the same number of frames on both sides, a resized height and "
             "width of at least 7; SSIM with win_size=7, the uniform window, the sample covariance and an explicit data_range")


@dataclass
class FrameMetrics:
    """Per-frame results on the device: ``mse``, ``psnr``, ``ssim`` fp64 [N]; ``ssim_map`` fp32 [N, h - 6, w - 6, 3] (the SSIM image
    cropped by 3 pixels per border, as skimage crops before it averages) or None."""
    mse: torch.Tensor
    psnr: torch.Tensor
    ssim: torch.Tensor
    ssim_map: Optional[torch.Tensor] = None


def _checked(x, name, layout):
    """Everything that can be said about one side without a device: type, dtype, grad, rank, channels."""
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise RuntimeError(f"orv_amd.metrics: `{name}` must be a numpy array or a GPU tensor (got {type(x).__name__}); {SUPPORTED}")
    if x.dtype not in (np.uint8, np.float32, torch.uint8, torch.float32):
        raise RuntimeError(f"orv_amd.metrics: `{name}` is {x.dtype}; {SUPPORTED}")
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise RuntimeError(f"orv_amd.metrics: `{name}` requires grad; the metrics have no backward; {SUPPORTED}")
    if x.ndim != 4:
        raise ValueError(f"orv_amd.metrics: `{name}` must have 4 dimensions (got {tuple(x.shape)}); {SUPPORTED}")
    channels = x.shape[1] if layout == "nchw" else x.shape[3]
    if channels != 3:
        raise ValueError(f"orv_amd.metrics: `{name}` has {channels} channels in layout {layout!r} (shape {tuple(x.shape)}); {SUPPORTED}")


def _device_view(x, name, layout):
    """-> the [N, H, W, 3] view on the device: a numpy array is uploaded, a tensor is not copied."""
    if isinstance(x, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError(f"orv_amd.metrics: `{name}` is a numpy array and no GPU is available to upload it to; there is no CPU path")
        x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if not x.is_cuda:
        raise RuntimeError(f"orv_amd.metrics: `{name}` is on {x.device}; there is no CPU path; {SUPPORTED}")
    return x.permute(0, 2, 3, 1) if layout == "nchw" else x


def _range(data_range):
    if data_range is None:
        raise ValueError(f"orv_amd.metrics: `data_range` is missing: give the distance between the smallest and largest possible value "
                         f"(1.0 for frames in [0, 1]); {SUPPORTED}")
    data_range = float(data_range)
    if not (0.0 < data_range < float("inf")):
        raise ValueError(f"orv_amd.metrics: data_range = {data_range}; supported: a positive finite range")
    return data_range


def frame_metrics(pred, gt, size: Tuple[int, int] = (256, 320), data_range: float = 1.0, layout: str = "nhwc", full: bool = False) -> FrameMetrics:
    """Per-frame MSE, PSNR and SSIM of ``pred`` against ``gt`` after both are resized to ``size`` = (height, width) by the bilinear rule of
    DESIGN.md §16 (a side already at ``size`` is read exactly).  ``pred`` and ``gt`` may differ
    in their source sizes and dtypes.  ``full=True`` also returns the SSIM map."""
    if layout not in ("nhwc", "nchw"):
        raise ValueError(f"orv_amd.metrics: layout = {layout!r}; supported: 'nhwc' ([N, H, W, 3]) or 'nchw' ([N, 3, H, W])")
    data_range = _range(data_range)
    _checked(pred, "pred", layout), _checked(gt, "gt", layout)
    if pred.shape[0] != gt.shape[0]:
        raise ValueError(f"orv_amd.metrics: `pred` has {pred.shape[0]} frames and `gt` has {gt.shape[0]}; {SUPPORTED}")
    size = tuple(int(s) for s in size)
    if len(size) != 2 or min(size) < 7:
        raise ValueError(f"orv_amd.metrics: size = {size}; supported: (height, width), each at least 7 (one 7 x 7 window); {SUPPORTED}")
    out, ssim_map = ops.frame_metrics(_device_view(pred, "pred", layout), _device_view(gt, "gt", layout), size, data_range, full)
    return FrameMetrics(mse=out[0], psnr=out[1], ssim=out[2], ssim_map=ssim_map)


def _view(frames, view):
    """The reference's ``--view`` slice (``compute_metrics.py:29-32``): one third of the width when the frames are wider than 480."""
    W = frames.shape[2]
    if view >= 0 and W > 480:
        w = W // 3
        return frames[:, :, w * view: w * (view + 1)]
    return frames


def psnr_ssim(pred_video, gt_video, view: int = -1, size: Tuple[int, int] = (256, 320)):
    """The body of ``_compute_psnr_ssim`` after its two reads: videos [N, H, W, 3] (uint8, or fp32 in [0, 1]); the last frame of the
    shorter clip is dropped (``min(len) - 1`` frames are compared, as the reference does), ``view >= 0`` takes that third of a width above
    480 -> ``(n_frames, mean psnr, mean ssim)`` with the means as Python floats (one host read)."""
    for x, name in ((pred_video, "pred_video"), (gt_video, "gt_video")):
        if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim != 4:
            raise ValueError(f"orv_amd.metrics: `{name}` must be [N, H, W, 3]; {SUPPORTED}")
    n = min(pred_video.shape[0], gt_video.shape[0]) - 1
    if n < 1:
        raise ValueError(f"orv_amd.metrics: the clips have {pred_video.shape[0]} and {gt_video.shape[0]} frames; supported: at least 2 each "
                         "(the reference compares min(len) - 1 frames)")
    res = frame_metrics(_view(pred_video, view)[:n], _view(gt_video, view)[:n], size=size, data_range=1.0)
    both = torch.stack([res.psnr, res.ssim]).cpu().numpy()
    return n, float(both[0].mean()), float(both[1].mean())


def _single(a, b, name_a, name_b):
    for x, name in ((a, name_a), (b, name_b)):
        if not isinstance(x, (np.ndarray, torch.Tensor)) or x.ndim != 3:
            raise ValueError(f"orv_amd.metrics: `{name}` must be one image [H, W, 3]; {SUPPORTED}")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"orv_amd.metrics: the images are {tuple(a.shape)} and {tuple(b.shape)}; supported: two images of one shape")
    return a[None], b[None]


def peak_signal_noise_ratio(image_true, image_test, *, data_range=None) -> float:
    """skimage's call shape for one image pair [H, W, 3]; no resize."""
    data_range = _range(data_range)
    a, b = _single(image_true, image_test, "image_true", "image_test")
    return float(frame_metrics(a, b, size=tuple(a.shape[1:3]), data_range=data_range).psnr[0])


def structural_similarity(im1, im2, *, win_size=None, gradient=False, data_range=None, channel_axis=None, gaussian_weights=False, full=False,
                          use_sample_covariance=True):
    """skimage's call shape for one image pair [H, W, 3] with ``channel_axis=-1``; no resize.  ``full=True`` returns ``(mssim, S)`` with S
    fp32 [H - 6, W - 6, 3] on the device: the pixels skimage averages (it returns the uncropped image)."""
    if gaussian_weights or win_size not in (None, 7) or not use_sample_covariance or gradient:
        raise ValueError(f"orv_amd.metrics: gaussian_weights={gaussian_weights}, win_size={win_size}, use_sample_covariance={use_sample_covariance}, "
                         f"gradient={gradient}; supported: gaussian_weights=False, win_size=7 (or None), use_sample_covariance=True, gradient=False")
    if channel_axis not in (-1, 2):
        raise ValueError(f"orv_amd.metrics: channel_axis = {channel_axis}; supported: -1 (images [H, W, 3])")
    data_range = _range(data_range)
    a, b = _single(im1, im2, "im1", "im2")
    res = frame_metrics(a, b, size=tuple(a.shape[1:3]), data_range=data_range, full=full)
    return (float(res.ssim[0]), res.ssim_map[0]) if full else float(res.ssim[0])


# ---- the closed-form tail of FID / FVD: host, numpy + scipy ----
def _sqrtm(m):
    from scipy import linalg
    try:
        res = linalg.sqrtm(m, disp=False)
    except TypeError:                                # a scipy without the `disp` argument
        res = linalg.sqrtm(m)
    return res[0] if isinstance(res, tuple) else res


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """``|mu1 - mu2|^2 + Tr(sigma1) + Tr(sigma2) - 2 Tr(sqrt(sigma1 sigma2))`` (``compute_metrics.py:171-204``): a product whose root is
    not finite is retried with ``eps`` on both diagonals; an imaginary part beyond 1e-3 on the diagonal raises ValueError, a smaller one
    is dropped."""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape:
        raise ValueError(f"orv_amd.metrics: the mean vectors have different lengths ({mu1.shape} and {mu2.shape})")
    if sigma1.shape != sigma2.shape:
        raise ValueError(f"orv_amd.metrics: the covariances have different dimensions ({sigma1.shape} and {sigma2.shape})")
    diff = mu1 - mu2
    covmean = _sqrtm(sigma1.dot(sigma2))
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = _sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def frechet_distance(feats_fake: np.ndarray, feats_real: np.ndarray) -> float:
    """Feature sets [n, d] -> the Frechet distance of their Gaussian fits (``compute_metrics.py:278-293``); a single-row ``feats_fake``
    returns the squared distance of the means, as the reference does."""
    feats_fake, feats_real = np.asarray(feats_fake), np.asarray(feats_real)
    if feats_fake.ndim != 2 or feats_real.ndim != 2 or feats_fake.shape[1] != feats_real.shape[1]:
        raise ValueError(f"orv_amd.metrics: feature sets must be [n, d] with one d (got {feats_fake.shape} and {feats_real.shape})")
    m = np.square(feats_fake.mean(axis=0) - feats_real.mean(axis=0)).sum()
    if feats_fake.shape[0] <= 1:
        return float(np.real(m))
    sigma1, sigma2 = np.atleast_2d(np.cov(feats_fake, rowvar=False)), np.atleast_2d(np.cov(feats_real, rowvar=False))
    s = _sqrtm(np.dot(sigma1, sigma2))
    return float(np.real(m + np.trace(sigma1 + sigma2 - s * 2)))
