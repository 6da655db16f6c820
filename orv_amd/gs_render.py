"""Gaussian rasterizer for ORV's depth / semantic conditioning renders, on the MI355X.

The reference splats the occupied voxels as 3-D Gaussians once per frame and view (``orv/dataset/gs_render.py:97-171``, called from
``orv/dataset/prepare_dataset.py:get_render``) through a CUDA-only extension.  This module is the same Python surface -
``GaussianRasterizationSettings`` / ``GaussianRasterizer`` of ``diff_gaussian_rasterization`` and the helpers of ``gs_render`` - over the
HIP kernels of ``csrc/gs_render.hip``.  Forward only: colours and features are given per Gaussian, covariances come from scale and
rotation.  The arithmetic contract is in DESIGN.md §12.

``install()`` registers the module under the reference's two import names, so ``from diff_gaussian_rasterization import ...`` and
``from gs_render import render, ...`` run unedited.
"""
from __future__ import annotations

import importlib.util
import math
import sys
from typing import NamedTuple

import torch
import torch.nn as nn

from . import ops

MAX_FEATURES = 16
SUPPORTED = ("supported: CUDA float32 tensors without requires_grad; colors_precomp [N,3]; language_feature_precomp [N,F] with F <= "
             f"{MAX_FEATURES}; scales [N,3] + rotations [N,4]; forward only")


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    include_feature: bool


def _refuse(what: str):
    raise NotImplementedError(f"orv_amd.gs_render: {what} ({SUPPORTED})")


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """True for the points in front of the near plane (view-space z > 0.01), the rasterizer's own visibility test."""
        with torch.no_grad():
            v = self.raster_settings.viewmatrix.to(positions.dtype)
            return positions @ v[:3, 2] + v[3, 2] > 0.01

    @torch.no_grad()
    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, language_feature_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None):
        """-> (color [3,H,W], feature [F,H,W], radii [N] int32, depth [1,H,W], alpha [1,H,W]).  ``means2D`` is accepted and ignored
        (it only carries screen-space gradients in the reference, and there is no backward here)."""
        rs = self.raster_settings
        if (shs is None) == (colors_precomp is None):
            raise Exception("Please provide exactly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        if shs is not None:
            _refuse("spherical harmonics (shs) are not implemented, pass colors_precomp")
        if cov3D_precomp is not None:
            _refuse("a precomputed 3-D covariance (cov3D_precomp) is not implemented, pass scales and rotations")
        feats = language_feature_precomp if rs.include_feature else None
        if feats is not None and feats.numel() == 0 and feats.dim() < 2:
            feats = None
        named = [("means3D", means3D), ("opacities", opacities), ("colors_precomp", colors_precomp), ("scales", scales), ("rotations", rotations),
                 ("raster_settings.bg", rs.bg), ("raster_settings.viewmatrix", rs.viewmatrix), ("raster_settings.projmatrix", rs.projmatrix)]
        if feats is not None:
            named.append(("language_feature_precomp", feats))
        for n, t in named:
            if not isinstance(t, torch.Tensor):
                _refuse(f"`{n}` is a {type(t).__name__}, not a tensor")
            if t.dtype != torch.float32:
                _refuse(f"`{n}` is {t.dtype}, not float32")
        if feats is not None and (feats.dim() != 2 or feats.shape[1] > MAX_FEATURES):
            _refuse(f"language_feature_precomp has shape {tuple(feats.shape)}: F > {MAX_FEATURES} feature channels")
        N = means3D.shape[0] if means3D.dim() == 2 else -1
        want = {"means3D": (N, 3), "colors_precomp": (N, 3), "scales": (N, 3), "rotations": (N, 4)}
        if feats is not None:
            want["language_feature_precomp"] = (N, feats.shape[1])
        for n, t in named:
            if (n in want and tuple(t.shape) != want[n]) or (n == "opacities" and t.numel() != N) or N < 0:
                raise ValueError(f"orv_amd.gs_render: `{n}` has shape {tuple(t.shape)}; expected means3D [N,3], opacities [N,1], colors_precomp "
                                 "[N,3], scales [N,3], rotations [N,4], language_feature_precomp [N,F] with one N")
        for n, t in named:
            if t.requires_grad:
                _refuse(f"`{n}` has requires_grad=True and there is no backward pass: detach it")
        for n, t in named:
            if not t.is_cuda:
                _refuse(f"`{n}` is not a CUDA tensor (it is on {t.device}); there is no CPU path")
            if t.device != means3D.device:
                raise RuntimeError(f"orv_amd.gs_render: `{n}` is on {t.device} but means3D is on {means3D.device}; one render uses one device")
        H, W = int(rs.image_height), int(rs.image_width)
        c = lambda t: t.contiguous()
        xy, conic_op, depth, radii, rect, tiles = ops.gs_preprocess(c(means3D), c(scales), c(rotations), c(opacities), c(rs.viewmatrix),
                                                                    c(rs.projmatrix), H, W, rs.tanfovx, rs.tanfovy, rs.scale_modifier)
        offsets = torch.cumsum(tiles, 0, dtype=torch.int64)
        L = int(offsets[-1]) if N else 0                       # the one host sync of a render
        if L >= 2 ** 31:
            raise RuntimeError(f"orv_amd.gs_render: {L} (Gaussian, tile) pairs; the tile lists are indexed with 32 bits, so 2^31 or more "
                               "are refused - render fewer Gaussians or a smaller image")
        keys, idx = ops.gs_tile_keys(rect, depth, offsets, H, W, L)
        keys, order = torch.sort(keys, stable=True)            # (tile, depth) ascending; stability breaks depth ties by Gaussian index
        ranges = ops.gs_tile_ranges(keys, H, W)
        color, feat, dep, alpha = ops.gs_render(ranges, idx[order], xy, conic_op, depth, c(colors_precomp), None if feats is None else c(feats),
                                                c(rs.bg), H, W)
        return color, feat, radii, dep, alpha


def focal2fov(focal, pixels):
    """Full field of view of a pinhole camera whose image is ``pixels`` wide at focal length ``focal`` (in pixels)."""
    return 2.0 * math.atan(0.5 * pixels / focal)


def _frustum_matrix(left, right, bottom, top, near, far):
    # x, y of the frustum to (-1, 1), z to (0, 1) with w = z (no flip of the z axis)
    m = torch.zeros(4, 4, dtype=torch.float32)
    m[0, 0] = 2.0 * near / (right - left)
    m[1, 1] = 2.0 * near / (top - bottom)
    m[0, 2] = (right + left) / (right - left)
    m[1, 2] = (top + bottom) / (top - bottom)
    m[2, 2] = far / (far - near)
    m[2, 3] = -(far * near) / (far - near)
    m[3, 2] = 1.0
    return m


def get_projection_matrix(near, far, fov_x, fov_y):
    """Symmetric perspective projection from the two fields of view."""
    r, t = math.tan(0.5 * fov_x) * near, math.tan(0.5 * fov_y) * near
    return _frustum_matrix(-r, r, -t, t, near, far)


def get_projection_matrix_c(fx, fy, cx, cy, W, H, znear, zfar):
    """Perspective projection of a pinhole camera with an off-centre principal point (cx, cy)."""
    return _frustum_matrix(-(W - cx) * znear / fx, cx * znear / fx, -(H - cy) * znear / fy, cy * znear / fy, znear, zfar)


def create_full_center_coords(range, dim):
    """[X, Y, Z, 3] grid of coordinates: ``range`` = [[lo xyz], [hi xyz]] (numpy), ``dim`` = cell size per axis; axis a has
    (hi - lo) / dim cells and its coordinates run from lo to hi inclusive."""
    shape = [int(v) for v in torch.from_numpy((range[1] - range[0]) / dim).long()]
    axes = [torch.linspace(float(range[0, a]), float(range[1, a]), shape[a]) for a in (0, 1, 2)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)


# the reference's palette for the 12 semantic channels it renders (rows of 0-255 RGB)
_PALETTE = torch.tensor([[255, 120, 50], [255, 192, 203], [255, 255, 0], [0, 150, 245], [0, 255, 255], [255, 127, 0], [255, 0, 0],
                         [255, 240, 150], [135, 60, 0], [160, 32, 240], [255, 0, 255], [139, 137, 137]], dtype=torch.float32)


def apply_semantic_colormap(semantic):
    """(N, H, W) class scores (argmax over N) or (1, H, W) labels -> (3, H, W) colours in [0, 1] on the CPU; labels past 11 stay black."""
    labels = semantic.argmax(dim=0) if semantic.shape[0] != 1 else semantic[0]
    labels = labels.long().cpu()
    known = (labels >= 0) & (labels < _PALETTE.shape[0])
    rgb = _PALETTE[labels.clamp(0, _PALETTE.shape[0] - 1)] * known[..., None]
    return rgb.permute(2, 0, 1) / 255.0


def render(extrinsics, intrinsics, image_shape, pts_xyz, pts_rgb, feat, rotations, scales, opacity, bg_color):
    """Render one view: ``extrinsics`` camera-to-world [4,4], ``intrinsics`` [3,3] in pixels, ``image_shape`` (H, W).
    -> {'render_color', 'radii', 'render_depth', 'render_alpha', 'render_feat'}."""
    height, width = image_shape
    fx, fy, cx, cy = (float(intrinsics[0][0]), float(intrinsics[1][1]), float(intrinsics[0][2]), float(intrinsics[1][2]))
    dev = pts_xyz.device
    view = torch.inverse(extrinsics).transpose(0, 1).to(dev)                       # (world-to-camera)^T
    proj = view.float() @ get_projection_matrix_c(fx, fy, cx, cy, width, height, 0.1, 200.0).transpose(0, 1).to(dev)
    settings = GaussianRasterizationSettings(
        image_height=height, image_width=width, tanfovx=math.tan(0.5 * focal2fov(fx, width)), tanfovy=math.tan(0.5 * focal2fov(fy, height)),
        bg=torch.tensor(bg_color, dtype=torch.float32, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=proj, sh_degree=3,
        campos=view.inverse()[3, :3], prefiltered=False, debug=False, include_feature=True)
    color, feature, radii, depth, alpha = GaussianRasterizer(raster_settings=settings)(
        means3D=pts_xyz, means2D=None, shs=None, colors_precomp=pts_rgb, language_feature_precomp=feat, opacities=opacity, scales=scales,
        rotations=rotations, cov3D_precomp=None)
    return {"render_color": color, "radii": radii, "render_depth": depth, "render_alpha": alpha, "render_feat": feature}


def labels_and_depth(pkg, unique_classes, alpha_min=0.10, none_depth=51.2, depth_clamp=(0.01, 0.4)):
    """The post-processing of ``prepare_dataset.py:2185-2201`` on a ``render`` result: pixels whose alpha is below ``alpha_min`` get the
    "none" one-hot (channel 0) and ``none_depth``; depth is clamped; labels are the feature argmax, clamped into ``unique_classes`` and
    looked up there.  -> (labels [H,W], depth [1,H,W]); ``pkg`` is left unchanged."""
    feat, depth = pkg["render_feat"].clone(), pkg["render_depth"].clone()
    none = pkg["render_alpha"][0] < alpha_min
    none_label = torch.zeros(feat.shape[0], dtype=feat.dtype, device=feat.device)
    none_label[0] = 1
    feat[:, none] = none_label[:, None]
    depth[:, none] = none_depth
    depth = torch.clamp(depth, min=depth_clamp[0], max=depth_clamp[1])
    index = feat.argmax(dim=0) if feat.shape[0] != 1 else feat[0].long()
    index = torch.clamp(index, min=0, max=len(unique_classes) - 1)
    return unique_classes.to(index.device)[index], depth


_ALIASES = ("diff_gaussian_rasterization", "gs_render")
_installed = {}


def _importable(name):
    if name in sys.modules:
        return True
    try:
        return importlib.util.find_spec(name) is not None
    except (ImportError, ValueError):
        return False


def install():
    """Register this module as ``diff_gaussian_rasterization`` (when the CUDA extension is not importable) and as ``gs_render`` (when
    that name is free).  -> the names registered by this call."""
    me = sys.modules[__name__]
    done = []
    for name in _ALIASES:
        if not _importable(name):
            sys.modules[name] = me
            _installed[name] = True
            done.append(name)
    return done


def uninstall():
    """Remove the names ``install()`` registered (and only those, and only while they still point here)."""
    me = sys.modules[__name__]
    for name in list(_installed):
        if sys.modules.get(name) is me:
            del sys.modules[name]
        del _installed[name]
