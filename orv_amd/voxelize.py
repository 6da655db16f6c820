"""Point-cloud voxelization for ORV's occupancy preparation, on the MI355X.

The reference turns every frame's point cloud into occupied, labelled voxels with ``points_to_voxels``
(``orv/dataset/prepare_dataset.py:137-198``, called from ``get_occupancy``, ``:887-1039``) over the CUDA-only extension ``orv/ops/voxelize``
(``voxelization.py:42-122``).  This module is the same Python surface - ``voxelization`` with the call shape of ``_Voxelization.apply`` and
``points_to_voxels`` with the reference's signature - over the HIP kernels of ``csrc/voxelize.hip``.  Outputs are integers and copied
floats, equal bit for bit to the sequential definition of ``voxelization_cpu.cpp:71-102``.  The arithmetic contract is in DESIGN.md §13.

``install()`` registers the module under the two spellings of the reference's import (``ivideogpt.ops.voxelize.voxelization``, the one
``points_to_voxels`` uses, and ``orv.ops.voxelize.voxelization``, where the package lives), so those lines run unedited.
"""
from __future__ import annotations

import importlib.util
import sys
import types

import numpy as np
import torch

from . import ops

MAX_LABEL = 255
SUPPORTED = ("supported: a contiguous CUDA float32 tensor points [N,C] with C >= 3 (x, y, z first) without requires_grad; "
             "deterministic=True; hard (max_points > 0 and max_voxels > 0) or dynamic (either is -1) voxelization; labels that are "
             f"integers in [0, {MAX_LABEL}); forward only")


def _refuse(what: str):
    raise NotImplementedError(f"orv_amd.voxelize: {what} ({SUPPORTED})")


def _floats(values, n, name):
    """A list of python floats, 0-d tensors or an array -> n fp32 values, rounded as ``torch.tensor(values, dtype=torch.float)`` rounds."""
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().tolist()
    out = np.asarray([float(v) for v in values], dtype=np.float64).astype(np.float32)
    if out.shape != (n,):
        raise ValueError(f"orv_amd.voxelize: `{name}` must have {n} values (got {out.size})")
    return out


def _check_points(points, deterministic, flag="deterministic", contiguous=True):
    if not isinstance(points, torch.Tensor):
        _refuse(f"`points` is a {type(points).__name__}, not a tensor")
    if points.dtype != torch.float32:
        _refuse(f"`points` is {points.dtype}, not float32")
    if points.dim() != 2 or points.shape[1] < 3:
        _refuse(f"`points` has shape {tuple(points.shape)}: C < 3 or not [N,C]")
    if points.requires_grad:
        _refuse("`points` has requires_grad=True and there is no backward pass: detach it")
    if contiguous and not points.is_contiguous():
        _refuse("`points` is not contiguous: call .contiguous() on it")
    if not deterministic:
        _refuse(f"{flag}=False asks for the reference's non-deterministic voxel order, which is not reproducible by definition")
    if not points.is_cuda:
        _refuse(f"`points` is not a CUDA tensor (it is on {points.device}); there is no CPU path")


def _numbered(points, vs, rng):
    """The shared front of hard voxelization and the vote -> (point coors, sort order, start, seglen, csum, voxels opened)."""
    pt_coors, keys = ops.voxel_coors(points, vs, rng)
    keys, order = torch.sort(keys, stable=True)            # equal cells stay in point order: a segment's head is the voxel's first point
    start, seglen, first = ops.voxel_segments(keys, order)
    csum = torch.cumsum(first, 0, dtype=torch.int32)       # voxel number + 1 at each voxel's first point: order of first appearance
    opened = int(csum[-1]) if points.shape[0] else 0       # the one host sync of a voxelization
    return pt_coors, order, start, seglen, csum, opened


@torch.no_grad()
def voxelization(points, voxel_size, coors_range, max_points=35, max_voxels=20000, deterministic=True):
    """``points`` [N,C] -> ``coors`` int32 [N,3] in (z, y, x) order with -1 rows for points outside ``coors_range`` when ``max_points`` or
    ``max_voxels`` is -1 (dynamic), else ``(voxels [M, max_points, C], coors [M,3], num_points_per_voxel [M])`` with the voxels in order of
    first appearance and each voxel's points in point order.  ``voxel_size`` [3] and ``coors_range`` [6] (x y z min, then max) may hold
    floats or 0-d tensors."""
    _check_points(points, deterministic)
    max_points, max_voxels = int(max_points), int(max_voxels)
    vs, rng = _floats(voxel_size, 3, "voxel_size"), _floats(coors_range, 6, "coors_range")
    if max_points == -1 or max_voxels == -1:
        return ops.voxel_coors(points, vs, rng, want_keys=False)[0]
    if max_points <= 0 or max_voxels <= 0:
        _refuse(f"max_points = {max_points}, max_voxels = {max_voxels}")
    pt_coors, order, start, seglen, csum, opened = _numbered(points, vs, rng)
    return ops.voxel_scatter(points, pt_coors, order, start, seglen, csum, max_points, min(opened, max_voxels))


def _check_labels(labels):
    bad = (labels != labels) | (labels != torch.floor(labels)) | (labels < 0) | (labels >= MAX_LABEL)
    if bool(bad.any()):
        _refuse(f"`labels` holds values that are not integers in [0, {MAX_LABEL})")


@torch.no_grad()
def points_to_voxels(points, voxel_size=[0.2, 0.2, 0.2], labels=None, max_num_points=-1, point_cloud_range=None,
                     device=torch.device("cuda"), determinstic=True):
    """The reference's ``points_to_voxels``: ``points`` [N, >=3] (numpy or tensor) with one integer label per point -> numpy float64 [M,4] of
    ``x, y, z, label`` per occupied voxel, the label being the most frequent one among the voxel's first 100 points (a tie goes to the
    smallest label).  Like the reference it always voxelizes with ``max_voxels = 1e5`` and 100 points per voxel, whatever ``max_num_points``
    says, drops rows with a NaN coordinate, and takes the range from the data when ``point_cloud_range`` is None."""
    if isinstance(points, np.ndarray):
        points = torch.tensor(points, device=device, dtype=torch.float32)
    _check_points(points, determinstic, "determinstic", contiguous=False)      # the slicing below copies
    if labels is None:
        labels = torch.zeros_like(points[:, 0])
    if isinstance(labels, np.ndarray):
        labels = torch.tensor(labels.astype(np.int32), device=points.device, dtype=torch.float32)
    labels = labels.to(points.device).float()
    if labels.shape != points.shape[:1]:
        raise ValueError(f"orv_amd.voxelize: `labels` has shape {tuple(labels.shape)}; expected one label per point, [{points.shape[0]}]")
    _check_labels(labels)
    points = torch.cat([points[:, :3], labels[..., None] + 1], dim=1)         # x y z and label + 1: zero stays free for padding
    max_voxels, max_num_points = int(1e5), int(1e2)
    points = points[~(torch.isnan(points[:, 0]) | torch.isnan(points[:, 1]) | torch.isnan(points[:, 2]))]
    if point_cloud_range is None:
        if points.shape[0] == 0:
            raise ValueError("orv_amd.voxelize: no point is left to take the range from; pass point_cloud_range")
        point_cloud_range = torch.cat([points[:, :3].min(0).values, points[:, :3].max(0).values])
    vs, rng = _floats(voxel_size, 3, "voxel_size"), _floats(point_cloud_range, 6, "point_cloud_range")
    pt_coors, order, start, seglen, csum, opened = _numbered(points, vs, rng)
    out = ops.voxel_vote(points, pt_coors, order, start, seglen, csum, max_num_points, min(opened, max_voxels))
    return out.cpu().numpy().astype(np.float64)              # the reference concatenates int32 coors with float32 labels: numpy gives float64


_ALIASES = ("ivideogpt.ops.voxelize.voxelization", "orv.ops.voxelize.voxelization")
_installed = {}            # module name -> the module object this module put into sys.modules


def _importable(name):
    if name in sys.modules:
        return True
    try:
        return importlib.util.find_spec(name) is not None
    except (ImportError, ValueError, AttributeError):
        return False


def install():
    """Register this module under the reference's import names for it that are not importable, with empty parent packages where those are
    missing too, so that ``from ivideogpt.ops.voxelize.voxelization import voxelization`` resolves.  -> the aliases registered by this call."""
    me = sys.modules[__name__]
    done = []
    for alias in _ALIASES:
        if _importable(alias):
            continue
        parts = alias.split(".")
        parent = None
        for depth in range(1, len(parts)):
            name = ".".join(parts[:depth])
            if not _importable(name):
                pkg = types.ModuleType(name)
                pkg.__path__ = []                          # a package with nothing on disk
                sys.modules[name] = pkg
                _installed[name] = pkg
                if parent is not None and _installed.get(".".join(parts[:depth - 1])) is parent:
                    setattr(parent, parts[depth - 1], pkg)         # only on a parent this call chain created
            parent = sys.modules.get(name)
        sys.modules[alias] = me
        _installed[alias] = me
        if parent is not None and _installed.get(".".join(parts[:-1])) is parent:
            setattr(parent, parts[-1], me)
        done.append(alias)
    return done


def uninstall():
    """Remove the names ``install()`` registered (and only those, and only while they still point at what it put there)."""
    for name in sorted(_installed, key=len, reverse=True):
        if sys.modules.get(name) is _installed[name]:
            del sys.modules[name]
        del _installed[name]
