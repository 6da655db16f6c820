"""Occupancy labelling and sparse Gaussian scene preparation for ORV's conditioning chain, on the MI355X.

Two steps of the reference's dataset preparation sit between the point-cloud voxelization (``orv_amd.voxelize``) and the Gaussian
rasterizer (``orv_amd.gs_render``), and this module is both, over the HIP kernels of ``csrc/occupancy.hip``:

* ``project_labels`` - ``project_3d_to_2d`` (``orv/dataset/prepare_dataset.py:878-884``) and the labelling block of ``get_occupancy``
  (``:999-1008``): every surface point is projected into the 2-D label image and takes the label under it.  One kernel, no temporaries.
  ``occupancy_from_points`` chains it with ``voxelize.points_to_voxels`` to the float64 ``[M, 4]`` array ``get_occupancy`` saves.
* ``OccupancyScene`` - the front of ``get_render`` (``:2069-2086`` and ``:2148-2164``): a frame's occupancy rows become the Gaussians the
  rasterizer splats.  The reference fills a 64 M-cell grid, runs ``torch.unique`` over it, builds a ``[64 M, 12]`` one-hot and gathers six
  dense tensors by a mask; here the work is O(M log M) in the number of rows and no buffer has the size of the grid.  ``scene.render`` and
  ``scene.render_trajectory`` add the existing rasterizer and post-processing, up to the fields of the ``.npz`` the dataset reads.

Every output is equal bit for bit to what the reference's statements produce; the arithmetic contract is in DESIGN.md §14.  Forward only.
"""
from __future__ import annotations

import numpy as np
import torch

from . import gs_render, ops, voxelize

NUM_COLORS = 60            # len(colors60) of the reference: labels live in [0, 59], and 255 in a label image means 59
MAX_CHANNELS = 64
SUPPORTED = ("supported: a CUDA float32 tensor points [N,C] with C >= 3 (x, y, z first) without requires_grad; labels2d [H,W] of uint8 or "
             "an integer type (numpy or tensor); extrin [4,4] camera-to-world and intrin [3,3] or [4,4]; occupancy rows [M,4] = x y z label "
             f"of any real dtype; num_channels in [1, {MAX_CHANNELS}]; forward only")


def _refuse(what: str):
    raise NotImplementedError(f"orv_amd.occupancy: {what} ({SUPPORTED})")


def _check_points(points):
    if not isinstance(points, torch.Tensor):
        _refuse(f"`points` is a {type(points).__name__}, not a tensor")
    if points.dtype != torch.float32:
        _refuse(f"`points` is {points.dtype}, not float32")
    if points.dim() != 2 or points.shape[1] < 3:
        _refuse(f"`points` has shape {tuple(points.shape)}: C < 3 or not [N,C]")
    if points.requires_grad:
        _refuse("`points` has requires_grad=True and there is no backward pass: detach it")
    if not points.is_cuda:
        _refuse(f"`points` is not a CUDA tensor (it is on {points.device}); there is no CPU path")


def _matrix(m, shapes, name, device):
    m = torch.as_tensor(m)
    if m.is_complex() or m.dtype == torch.bool:
        _refuse(f"`{name}` is {m.dtype}, not a real matrix")
    if tuple(m.shape) not in shapes:
        raise ValueError(f"orv_amd.occupancy: `{name}` has shape {tuple(m.shape)}; expected " + " or ".join(str(list(s)) for s in shapes))
    return m.to(device=device, dtype=torch.float32)


def scaled_intrinsics(intrin3, src_w=512, tgt_w=640):
    """``prepare_dataset.py:975-986``: the [3,3] pinhole matrix of the ``src_w``-wide point maps -> the fp32 [4,4] matrix of the
    ``tgt_w``-wide label image: an identity with ``intrin3`` in its corner and the first two rows multiplied by ``tgt_w / src_w`` in fp32."""
    intrin3 = torch.as_tensor(intrin3)
    if tuple(intrin3.shape) != (3, 3):
        raise ValueError(f"orv_amd.occupancy: `intrin3` has shape {tuple(intrin3.shape)}; expected [3, 3]")
    intrin = torch.eye(4, dtype=torch.float32, device=intrin3.device)
    intrin[:3, :3] = intrin3.float()
    intrin[:2, :3] = intrin[:2, :3] * (tgt_w / src_w)
    return intrin


@torch.no_grad()
def projection_matrix(extrin, intrin, device):
    """``intrin4 @ torch.linalg.inv(extrin)`` in fp32 on ``device``, the reference's own expression (``:880``); a [3,3] ``intrin`` sits in
    the corner of an identity."""
    extrin = _matrix(extrin, ((4, 4),), "extrin", device)
    intrin = _matrix(intrin, ((3, 3), (4, 4)), "intrin", device)
    if intrin.shape[0] == 3:
        intrin4 = torch.eye(4, dtype=torch.float32, device=device)
        intrin4[:3, :3] = intrin
        intrin = intrin4
    return (intrin @ torch.linalg.inv(extrin)).contiguous()


def _label_image(labels2d, device):
    if isinstance(labels2d, np.ndarray):
        if labels2d.dtype.kind not in "iu":
            _refuse(f"`labels2d` is {labels2d.dtype}, not uint8 or an integer type")
        if labels2d.dtype != np.uint8:                                   # narrowed on the host: 4 bytes per pixel cross the bus, not 8
            if labels2d.size and (int(labels2d.min()) < -2 ** 31 or int(labels2d.max()) >= 2 ** 31):
                _refuse("`labels2d` holds values outside the int32 range")
            labels2d = labels2d.astype(np.int32)
        labels2d = torch.from_numpy(np.ascontiguousarray(labels2d))
    if not isinstance(labels2d, torch.Tensor):
        _refuse(f"`labels2d` is a {type(labels2d).__name__}, not an array or a tensor")
    if labels2d.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        _refuse(f"`labels2d` is {labels2d.dtype}, not uint8 or an integer type")
    if labels2d.dim() != 2 or labels2d.numel() == 0:
        raise ValueError(f"orv_amd.occupancy: `labels2d` has shape {tuple(labels2d.shape)}; expected [H, W] with H, W >= 1")
    if labels2d.dtype == torch.int64:                                    # the only tensor type that does not fit: checked where it lives
        if bool((labels2d < -2 ** 31).any() | (labels2d >= 2 ** 31).any()):
            _refuse("`labels2d` holds values outside the int32 range")
        labels2d = labels2d.to(torch.int32)
    elif labels2d.dtype != torch.uint8:
        labels2d = labels2d.to(torch.int32)
    return labels2d.to(device).contiguous()


@torch.no_grad()
def project_labels(points, labels2d, extrin, intrin):
    """``points`` [N, >=3] on the device, ``labels2d`` [H,W], ``extrin`` camera-to-world [4,4], ``intrin`` [3,3] or [4,4] -> int64 [N]:
    the label under each point's pixel with 255 -> 59, and 0 for a point that falls outside the image."""
    _check_points(points)
    P = projection_matrix(extrin, intrin, points.device)
    return ops.occ_project_labels(points.contiguous(), P, _label_image(labels2d, points.device))


@torch.no_grad()
def occupancy_from_points(points, labels2d, extrin, intrin, voxel_size=[0.001] * 3, point_cloud_range=[-0.2, -0.2, 0, 0.2, 0.2, 0.4]):
    """One frame of ``get_occupancy`` (``:999-1019``): label the points, then voxelize them with the vote -> numpy float64 [M,4] of
    ``x, y, z, label`` per occupied voxel."""
    labels3d = project_labels(points, labels2d, extrin, intrin)
    return voxelize.points_to_voxels(points, voxel_size=voxel_size, labels=labels3d, point_cloud_range=point_cloud_range, device=points.device)


class OccupancyScene:
    """The Gaussians of an occupancy grid, made from the occupied cells alone.  The constructor keeps four 1-D tables: the coordinate axes
    exactly as ``gs_render.create_full_center_coords`` makes them, and the per-z scale, ``base_scale`` times a ramp from 1 to 2 over the z bins raised to
    ``exp_scale``, that torch computes on the device (``:2074-2076``).  A grid needs at least two cells along z."""

    def __init__(self, point_cloud_range=[-0.2, -0.2, 0, 0.2, 0.2, 0.4], voxel_size=[0.001] * 3, base_scale=0.00023, exp_scale=3.7,
                 num_channels=12, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            _refuse(f"device {self.device} is not a CUDA device; there is no CPU path")
        rng, vs = [float(v) for v in point_cloud_range], [float(v) for v in voxel_size]
        if len(rng) != 6 or len(vs) != 3:
            raise ValueError(f"orv_amd.occupancy: point_cloud_range needs 6 values and voxel_size 3 (got {len(rng)} and {len(vs)})")
        self.num_channels = int(num_channels)
        if not 1 <= self.num_channels <= MAX_CHANNELS:
            _refuse(f"num_channels = {num_channels}")
        occ_range, occ_dim = np.array([rng[0:3], rng[3:6]]), np.array(vs)
        with np.errstate(all="ignore"):
            cells = (occ_range[1] - occ_range[0]) / occ_dim
        if not (np.isfinite(cells).all() and (cells >= 1).all() and (cells < 65536).all()):
            raise ValueError(f"orv_amd.occupancy: the grid (hi - lo) / voxel_size = {cells.tolist()} needs 1 to 65535 cells on every axis")
        self.grid = tuple(int(v) for v in cells.astype(np.uint16))                    # the reference's truncation
        if self.grid[2] < 2:
            raise ValueError("orv_amd.occupancy: the grid needs at least 2 cells along z: the scale table's ramp divides by Z - 1 (the "
                             "reference gets NaN scales there)")
        lin = [int(v) for v in torch.from_numpy(cells).long()]                        # create_full_center_coords' own count
        self.axes = tuple(torch.linspace(float(occ_range[0, a]), float(occ_range[1, a]), lin[a]).float().to(self.device) for a in (0, 1, 2))
        # bin numbers 1 .. Z as int64, a ramp from 1 at the first bin to 2 at the last by a tensor / tensor division on the device (not a
        # multiplication by a host reciprocal), then the power and the product: the operators of :2074-2076, so the bits are torch's
        bins = torch.arange(1, self.grid[2] + 1, device=self.device)
        ramp = (bins - bins[0]) / (bins[-1] - bins[0]) + 1
        self.zscale = (base_scale * ramp ** exp_scale).float().contiguous()
        self.cells = self.grid[0] * self.grid[1] * self.grid[2]

    def _rows(self, occ):
        if isinstance(occ, torch.Tensor):
            if occ.is_complex() or occ.dtype == torch.bool:
                _refuse(f"`occ` is {occ.dtype}, not a real dtype")
            rows = occ.detach().to(device=self.device, dtype=torch.int32)
        else:
            occ = np.asarray(occ)
            if occ.dtype.kind not in "iuf":
                _refuse(f"`occ` is {occ.dtype}, not a real dtype")
            rows = torch.tensor(occ, dtype=torch.int32, device=self.device)            # the reference's cast: toward zero
        if rows.dim() != 2 or rows.shape[1] != 4:
            raise ValueError(f"orv_amd.occupancy: `occ` has shape {tuple(rows.shape)}; expected [M, 4] = x y z label")
        return rows.contiguous()

    @torch.no_grad()
    def gaussians(self, occ):
        """``occ`` [M,4] of ``x y z label`` -> ``(xyz [n,3], rgb [n,3], feat [n,num_channels], rot [n,4], scale [n,3], opacity [n,1],
        unique_classes int64 [k], is_labeled)``: one Gaussian per distinct cell in ascending order of ``(x Y + y) Z + z``, a cell given more
        than once keeping its last row's label, labels clamped to [0, 59].  One host read."""
        rows = self._rows(occ)
        M, dev = rows.shape[0], self.device
        if M == 0:
            count, classes = 0, 1
            keys = order = torch.empty(0, dtype=torch.int64, device=dev)
            last = csum = torch.empty(0, dtype=torch.int32, device=dev)
        else:
            state = torch.zeros(3, dtype=torch.int64, device=dev)                      # class bitmap, out-of-grid flag, cell count
            keys = ops.occ_cell_keys(rows, self.grid, state)
            keys, order = torch.sort(keys, stable=True)                                # equal cells stay in row order: a segment ends on the last row
            last = ops.occ_mark_cells(keys, order, rows, state)
            csum = torch.cumsum(last, 0, dtype=torch.int32)
            state[2] = csum[-1]
            classes, flag, count = state.tolist()                                      # the one host read of a scene preparation
            if flag:
                raise ValueError(f"orv_amd.occupancy: `occ` holds a cell outside the {self.grid[0]} x {self.grid[1]} x {self.grid[2]} grid "
                                 "(the reference would wrap a negative index or fault)")
            if count < self.cells:
                classes |= 1                                                           # the zero-filled grid still shows an empty cell: class 0
        present = [c for c in range(NUM_COLORS) if classes >> c & 1]
        if len(present) > self.num_channels:
            raise ValueError(f"orv_amd.occupancy: {len(present)} classes are present {present} but the one-hot has num_channels = "
                             f"{self.num_channels} (torch.nn.functional.one_hot fails the same way in the reference)")
        out = ops.occ_write_gaussians(order, rows, last, csum, count, self.grid, self.axes, self.zscale, classes, self.num_channels)
        return (*out, torch.tensor(present, dtype=torch.int64, device=dev), len(present) > 1)

    @torch.no_grad()
    def render(self, occ, extrins, intrin, image_shape=None):
        """The view loop of ``get_render`` (``:2166-2204``) for one frame: ``extrins`` [n_view,4,4] camera-to-world, ``intrin`` [3,3] in
        pixels -> ``(semantics uint8 [n_view,H,W], depths float32 [n_view,H,W], is_labeled)`` on the device, with ``H, W = int(2 cy),
        int(2 cx)`` (``:2138-2139``) unless ``image_shape`` gives them."""
        intrin = torch.as_tensor(intrin).float()
        if tuple(intrin.shape) != (3, 3):
            raise ValueError(f"orv_amd.occupancy: `intrin` has shape {tuple(intrin.shape)}; expected [3, 3]")
        extrins = torch.as_tensor(extrins)
        if extrins.dim() != 3 or tuple(extrins.shape[1:]) != (4, 4):
            raise ValueError(f"orv_amd.occupancy: `extrins` has shape {tuple(extrins.shape)}; expected [n_view, 4, 4]")
        if image_shape is None:
            image_shape = [int(intrin[1, -1] * 2), int(intrin[0, -1] * 2)]
        H, W = int(image_shape[0]), int(image_shape[1])
        xyz, rgb, feat, rot, scale, opacity, unique_classes, is_labeled = self.gaussians(occ)
        semantics = torch.empty(len(extrins), H, W, dtype=torch.uint8, device=self.device)
        depths = torch.empty(len(extrins), H, W, dtype=torch.float32, device=self.device)
        for i, extrin in enumerate(extrins):
            pkg = gs_render.render(extrin.float().to(self.device), intrin, [H, W], xyz, rgb, feat, rot, scale, opacity, bg_color=[0, 0, 0])
            labels, depth = gs_render.labels_and_depth(pkg, unique_classes)
            semantics[i], depths[i] = labels.to(torch.uint8), depth[0]
        return semantics, depths, is_labeled

    @torch.no_grad()
    def render_trajectory(self, frames, extrins, intrin):
        """One trajectory of ``get_render``: ``frames`` = the occupancy arrays of its frames -> the three fields it saves (``:2222-2235``)
        as numpy: ``semantics`` uint8 [n_frame, n_view, H, W] (stacked), ``depths`` float32 [n_frame * n_view, H, W] (concatenated:
        ``dataset.py:862-864`` undoes this), and ``is_labeled``, false as soon as one frame holds a single class."""
        semantics, depths, is_labeled = [], [], True
        for occ in frames:
            s, d, labeled = self.render(occ, extrins, intrin)
            semantics.append(s.cpu().numpy()), depths.append(d.cpu().numpy())
            is_labeled = is_labeled and labeled
        if not semantics:
            raise ValueError("orv_amd.occupancy: `frames` is empty (np.stack of no frame fails in the reference too)")
        return {"semantics": np.stack(semantics).astype(np.uint8), "depths": np.concatenate(depths).astype(np.float32), "is_labeled": is_labeled}
