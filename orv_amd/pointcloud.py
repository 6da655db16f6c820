"""Point-cloud cleaning and normals in front of ORV's reconstruction stage, on the MI355X.

Stage 2 of the reference's preparation, ``get_dense_points`` (``orv/dataset/prepare_dataset.py:786-875``), runs per frame on one CPU thread
through Open3D's KD-tree: ``_preprocess_points`` (``:806-822``) keeps the points with ``z < 0.6`` and calls
``remove_statistical_outlier(nb_neighbors=30, std_ratio=1.5)``; ``process_nksr._preprocess_point_cloud`` (``:729-741``) calls
``estimate_normals(KDTreeSearchParamKNN(20))`` and ``orient_normals_towards_camera_location()``; only then do the ``[N, 3]`` fp32
``input_xyz`` / ``input_normal`` tensors go to the GPU (``:754-755``).  This module computes all of that on the device over the HIP kernels of
``csrc/pointcloud.hip``: an exact k-nearest-neighbour search on a uniform grid, the outlier statistics and the PCA normals.

PARITY WITH OPEN3D IS UNPINNED.  Open3D is not installed where this was written and has no ROCm path, so its semantics are restated from
memory; the restatement (``tests/pointcloud_ref.py``) is the contract the kernels are held to: fp64 distances on the fp32
values, neighbours ordered by ``(d2, index)``, the centred two-pass covariance.  There is no ``install()`` alias: the reference calls methods
on Open3D objects, which cannot be aliased sensibly; INTEGRATION.md shows the lines these calls replace.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

MAX_K = 64
MAX_CELLS = 1 << 21            # a dense int32 start table of 8 MB at most
SUPPORTED = ("supported: a contiguous CUDA float32 tensor points [N,3] with finite coordinates and without requires_grad; k-nearest-neighbour "
             f"search with 1 <= k <= {MAX_K} (no radius or hybrid search); forward only")


def _refuse(what: str):
    raise NotImplementedError(f"orv_amd.pointcloud: {what} ({SUPPORTED})")


def _check_points(points, name="points"):
    if not isinstance(points, torch.Tensor):
        _refuse(f"`{name}` is a {type(points).__name__}, not a tensor")
    if points.dtype != torch.float32:
        _refuse(f"`{name}` is {points.dtype}, not float32")
    if points.dim() != 2 or points.shape[1] != 3:
        _refuse(f"`{name}` has shape {tuple(points.shape)}, not [N,3]")
    if points.requires_grad:
        _refuse(f"`{name}` has requires_grad=True and there is no backward pass: detach it")
    if not points.is_contiguous():
        _refuse(f"`{name}` is not contiguous: call .contiguous() on it")
    if not points.is_cuda:
        _refuse(f"`{name}` is not a CUDA tensor (it is on {points.device}); there is no CPU path")


def _check_k(k, name="k", radius=None):
    if radius is not None:
        _refuse(f"radius = {radius!r} asks for a radius or hybrid search")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        _refuse(f"{name} = {k!r} is not an integer in [1, {MAX_K}]")
    return int(k)


def _camera(camera_location):
    if isinstance(camera_location, torch.Tensor):
        camera_location = camera_location.detach().cpu().tolist()
    cam = [float(c) for c in camera_location]
    if len(cam) != 3 or not all(math.isfinite(c) for c in cam):
        raise ValueError(f"orv_amd.pointcloud: `camera_location` must be three finite numbers (got {camera_location!r})")
    return cam


_LEVELS = (128, 64, 32, 16, 8)         # cells along the longest axis of the trial grids whose occupancy picks the edge


def _survey(points):
    """One host read: the box of the grid (the data's, cut at three standard deviations around the mean so that a far outlier does not
    stretch it), the number of occupied cells of five trial grids on it, and whether every coordinate is finite."""
    lo_all, hi_all = torch.aminmax(points, dim=0)                            # a NaN anywhere shows here, as an infinity does
    std, mean = torch.std_mean(points, dim=0, unbiased=False)
    lo, hi = torch.maximum(lo_all, mean - 3.0 * std), torch.minimum(hi_all, mean + 3.0 * std)
    m = _LEVELS[0]
    t = ((points - lo) * (m / (hi - lo).max().clamp_min(1e-30))).nan_to_num(0.0).clamp(0, m - 1).long()
    grid = torch.zeros(m ** 3, dtype=torch.uint8, device=points.device)
    grid[(t[:, 2] * m + t[:, 1]) * m + t[:, 0]] = 1                          # every writer of a cell writes the same value
    grid = grid.view(m, m, m)
    occ = []
    for level in _LEVELS:                                                     # each coarser grid is the 2 x 2 x 2 maximum of the finer one
        occ.append(grid.sum(dtype=torch.int64))
        if level > _LEVELS[-1]:
            grid = grid.view(level // 2, 2, level // 2, 2, level // 2, 2).amax(dim=(1, 3, 5))
    finite = torch.isfinite(torch.cat([lo_all, hi_all])).all()
    got = torch.cat([lo.double(), hi.double(), torch.stack(occ).double(), finite.double()[None]]).cpu().numpy()
    return got[0:3], got[3:6], got[6:11], bool(got[11])


def _auto_edge(N, k, length, occ):
    """The edge at which an occupied cell holds about max(2, k / 4) points: the finest trial grid that is at least that full, refined by the
    dimension the occupancy counts show between it and the next finer one (a surface fills cells as edge^-2, a volume as edge^-3)."""
    want = max(2.0, k / 4.0)
    per = [N / max(o, 1.0) for o in occ]                                      # points per occupied cell, finest grid first
    full = [i for i in range(len(_LEVELS)) if per[i] >= want]
    i = full[0] if full else len(_LEVELS) - 1
    j = i - 1 if i > 0 else 1                                                 # the neighbouring level the dimension is taken against
    fine, coarse = min(i, j), max(i, j)
    dim = min(3.0, max(0.5, math.log2(max(occ[fine], 1.0) / max(occ[coarse], 1.0))))
    cells = _LEVELS[i] * (per[i] / want) ** (1.0 / dim)
    if 0 < i and full:
        cells = min(cells, 2.0 * _LEVELS[i])
    return length / max(cells, 1.0)


def _grid(points, k, cell):
    """-> (origin fp32 [3], edge, (gx, gy, gz)) after the one host read of the survey; refuses a NaN or infinite coordinate."""
    lo, hi, occ, finite = _survey(points)
    if not finite:
        _refuse("`points` holds a NaN or infinite coordinate, whose neighbours are undefined")
    ext = hi - lo
    length = float(ext.max())
    if cell is None:
        edge = _auto_edge(points.shape[0], k, length, occ) if length > 0.0 else 1.0
    else:
        edge = float(cell)
        if not (edge > 0.0 and math.isfinite(edge)):
            raise ValueError(f"orv_amd.pointcloud: `cell` must be a positive finite edge (got {cell!r})")
    dims = [max(1, min(int(math.ceil(e / edge)), 1 << 20)) if e > 0.0 else 1 for e in ext]
    while cell is None and dims[0] * dims[1] * dims[2] > MAX_CELLS:          # an automatic edge grows until the table fits
        edge *= 2.0 ** (1.0 / 3.0)
        dims = [max(1, int(math.ceil(e / edge))) for e in ext]
    while dims[0] * dims[1] * dims[2] > MAX_CELLS:                            # a given edge is kept: the grid covers the middle of the box
        a = int(np.argmax(dims))
        dims[a] = (dims[a] + 1) // 2
    origin = np.array([(l + h) / 2.0 - g * edge / 2.0 if g * edge < e else l for l, h, g, e in zip(lo, hi, dims, ext)])
    return origin.astype(np.float32), edge, tuple(dims)


@torch.no_grad()
def knn(points, k, cell=None, return_stats=False, radius=None):
    """The ``k' = min(k, N)`` nearest neighbours of every point, itself included, under the order ``(d2, index)``
    -> ``(idx int32 [N, k'], d2 fp64 [N, k'])``, ascending, and with ``return_stats`` a dict of the grid dimensions ``grid``, its ``origin``,
    the edge ``cell`` and ``brute``, the number of queries the grid walk left to the scan of all points.  ``cell`` overrides the automatic
    edge (tests and tuning): the result does not depend on it.  Two host reads: the extent and the leftover queries."""
    k = _check_k(k, radius=radius)
    _check_points(points)
    N = points.shape[0]
    if N == 0:
        idx, d2 = torch.empty(0, 0, dtype=torch.int32, device=points.device), torch.empty(0, 0, dtype=torch.float64, device=points.device)
        return (idx, d2, {"grid": (0, 0, 0), "origin": (0.0, 0.0, 0.0), "cell": 0.0, "brute": 0}) if return_stats else (idx, d2)
    origin, edge, dims = _grid(points, k, cell)
    keys = ops.pc_cells(points, origin, edge, dims)
    keys, order = torch.sort(keys, stable=True)                # equal cells stay in point order
    start, spts = ops.pc_cell_table(keys, order, points, dims[0] * dims[1] * dims[2])
    idx, d2, pending = ops.pc_knn(spts, order, start, k, origin, edge, dims)
    left = torch.nonzero(pending).flatten()                    # the second host read
    if left.numel():
        ops.pc_knn_brute(points, k, left, out=(idx, d2))
    if return_stats:
        return idx, d2, {"grid": dims, "origin": tuple(float(o) for o in origin), "cell": edge, "brute": int(left.numel())}
    return idx, d2


@torch.no_grad()
def remove_statistical_outlier(points, nb_neighbors=30, std_ratio=1.5, return_stats=False):
    """Open3D's ``remove_statistical_outlier`` -> ``(points[ind], ind)`` with ``ind`` int64 ascending: the points whose mean distance to their
    ``nb_neighbors`` nearest neighbours (themselves included) is positive and below ``mean + std_ratio * std`` of those mean distances.  With
    ``return_stats`` a dict of ``avg`` fp64 [N] and the 0-d fp64 tensors ``mean``, ``std``, ``thr``, ``valid`` follows.  A cloud with one valid
    point has ``std`` = NaN and keeps nothing, as does one with none.  A third host read sizes the output."""
    k = _check_k(nb_neighbors, "nb_neighbors")
    _check_points(points)
    std_ratio = float(std_ratio)
    if not math.isfinite(std_ratio):
        raise ValueError(f"orv_amd.pointcloud: `std_ratio` must be finite (got {std_ratio!r})")
    _, d2 = knn(points, k)
    avg, stats, keep = ops.pc_outlier(d2, k, std_ratio)
    ind = torch.nonzero(keep).flatten()
    out = points[ind]
    if return_stats:
        return out, ind, {"avg": avg, "mean": stats[0], "std": stats[1], "thr": stats[2], "valid": stats[3]}
    return out, ind


@torch.no_grad()
def estimate_normals(points, max_nn=20, camera_location=(0.0, 0.0, 0.0), radius=None):
    """Open3D's ``estimate_normals(KDTreeSearchParamKNN(max_nn))`` followed by ``orient_normals_towards_camera_location(camera_location)``
    -> normals fp32 [N,3]: the unit eigenvector of the smallest eigenvalue of the covariance of every point's ``max_nn`` nearest neighbours,
    turned towards the camera; ``(0, 0, 1)`` before the turn with fewer than three neighbours or identical ones."""
    k = _check_k(max_nn, "max_nn", radius=radius)
    _check_points(points)
    cam = _camera(camera_location)
    if points.shape[0] == 0:
        return torch.empty(0, 3, dtype=torch.float32, device=points.device)
    idx, _ = knn(points, k)
    return ops.pc_normals(points, idx, k, cam)


@torch.no_grad()
def orient_normals_towards_camera_location(points, normals, camera_location=(0.0, 0.0, 0.0)):
    """Open3D's method of that name on given normals -> normals fp32 [N,3]: negated where they point away from the camera; a zero normal
    becomes the unit vector towards the camera, or ``(0, 0, 1)`` at the camera itself."""
    _check_points(normals, "normals")
    _check_points(points)
    if normals.shape != points.shape:
        raise ValueError(f"orv_amd.pointcloud: `normals` has shape {tuple(normals.shape)}; expected one per point, {tuple(points.shape)}")
    return ops.pc_orient(points, normals, _camera(camera_location))


def _take(attrs, ind, n):
    if isinstance(attrs, (tuple, list)):
        return type(attrs)(_take(a, ind, n) for a in attrs)
    if not isinstance(attrs, torch.Tensor) or attrs.dim() < 1 or attrs.shape[0] != n:
        raise ValueError(f"orv_amd.pointcloud: `attrs` must be tensors with one row per point ({n})")
    return attrs[ind.to(attrs.device)]


@torch.no_grad()
def preprocess_points(points, z_max=0.6, nb_neighbors=30, std_ratio=1.5, attrs=None):
    """``_preprocess_points`` of ``prepare_dataset.py:806-822``: the points with ``z < z_max``, then ``remove_statistical_outlier`` -> the kept
    points, or ``(points, attrs)`` when per-point ``attrs`` (a tensor [N, ...] such as the colours, or a tuple of them) are given: they follow
    both masks.  (The reference assigns the points as the colours at ``:817``; that defect is not reproduced.)"""
    _check_k(nb_neighbors, "nb_neighbors")
    _check_points(points)
    first = torch.nonzero(points[:, 2] < float(z_max)).flatten()
    low = points[first]
    out, ind = remove_statistical_outlier(low, nb_neighbors, std_ratio)
    if attrs is None:
        return out
    return out, _take(attrs, first[ind], points.shape[0])


@torch.no_grad()
def nksr_inputs(points, max_nn=20):
    """The two tensors ``process_nksr`` hands to the reconstructor (``:754-755``): ``(input_xyz, input_normal)``, fp32 [N,3] on the device,
    the normals from ``max_nn`` neighbours turned towards the origin."""
    return points, estimate_normals(points, max_nn)
