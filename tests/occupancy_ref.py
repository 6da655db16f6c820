"""CPU restatement of the occupancy contract, written from the contract and not from the kernels.

``project_labels`` is numpy float32 with every product, sum and divide rounded on its own.  ``sparse_gaussians`` walks the occupancy rows
into a dict from cell to label and works at any grid size.  ``dense_gaussians`` is the reference's dense formulation
(``orv/dataset/prepare_dataset.py:2069-2086`` and ``:2148-2164``) with the same torch operators on the CPU, for small grids; it makes a fresh zero grid per
call (on the CPU the reference's ``semantics_zero.to(device)`` would alias and carry labels from frame to frame, which is neither what
happens on a GPU nor the contract) and writes the grid on one thread, so that of two rows of one cell the last one stays.  The per-z
scale table is ``torch`` arithmetic, whose ``pow`` is not correctly rounded and may differ by an ulp between backends: the contract takes
it from torch on the device, so both restatements accept the device to compute it on.
"""
import contextlib

import numpy as np
import torch

NUM_COLORS = 60
REAL_RANGE = [-0.2, -0.2, 0, 0.2, 0.2, 0.4]
REAL_VOXEL = [0.001] * 3


def f32(x):
    return np.asarray(x, dtype=np.float32)


# ---- labelling ----
def pixels(points, P):
    """points [N, >=3] fp32, P [4,4] fp32 -> (u, v) fp32 [N]: h_j = ((x P[j][0] + y P[j][1]) + z P[j][2]) + P[j][3], u = h_0 / h_2,
    v = h_1 / h_2, each operation one fp32 numpy ufunc (rounded on its own)."""
    pts, P = f32(points), f32(P)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        h = [np.add(np.add(np.add(np.multiply(x, P[j, 0]), np.multiply(y, P[j, 1])), np.multiply(z, P[j, 2])), P[j, 3]) for j in range(3)]
        assert all(a.dtype == np.float32 for a in h)
        return np.divide(h[0], h[2]), np.divide(h[1], h[2])


def pixel_index(u, v, H, W):
    """-> (inside [N] bool, iu, iv int64 [N], zero where outside): truncation toward zero, a non-finite u or v is outside."""
    finite = np.isfinite(u) & np.isfinite(v)
    tu, tv = np.trunc(np.where(finite, u, -1.0)), np.trunc(np.where(finite, v, -1.0))
    inside = finite & (tu >= 0) & (tu < W) & (tv >= 0) & (tv < H)
    iu, iv = np.where(inside, tu, 0).astype(np.int64), np.where(inside, tv, 0).astype(np.int64)
    return inside, iu, iv


def project_labels(points, labels2d, P):
    """-> int64 [N]: labels2d[v, u] with 255 (and -1) -> 59 for a point inside the image, 0 outside."""
    labels2d = np.asarray(labels2d)
    H, W = labels2d.shape
    u, v = pixels(points, P)
    inside, iu, iv = pixel_index(u, v, H, W)
    lab = labels2d.astype(np.int64)[iv, iu]
    lab[(lab == 255) | (lab == -1)] = NUM_COLORS - 1
    return np.where(inside, lab, 0).astype(np.int64)


def scaled_intrinsics(intrin3, src_w=512, tgt_w=640):
    out = np.eye(4, dtype=np.float32)
    out[:3, :3] = f32(intrin3)
    out[:2, :3] = out[:2, :3] * np.float32(tgt_w / src_w)
    return out


# ---- the scene ----
def grid_shape(point_cloud_range, voxel_size):
    occ_range = np.array([point_cloud_range[0:3], point_cloud_range[3:6]], dtype=np.float64)
    return tuple(int(v) for v in ((occ_range[1] - occ_range[0]) / np.array(voxel_size, dtype=np.float64)).astype(np.uint16))


def axis_tables(point_cloud_range, voxel_size):
    """The three coordinate axes as create_full_center_coords makes them: torch.linspace on the CPU."""
    lo, hi = point_cloud_range[0:3], point_cloud_range[3:6]
    return [torch.linspace(float(lo[a]), float(hi[a]), n).float().numpy() for a, n in enumerate(grid_shape(point_cloud_range, voxel_size))]


def scale_table(nz, base_scale=0.00023, exp_scale=3.7, device="cpu"):
    """prepare_dataset.py:2074-2076 for one z column, computed by torch on ``device`` -> fp32 numpy [nz]."""
    number = torch.arange(1, nz + 1, device=device)                                 # int64 bin numbers 1 .. nz
    first, last = number.min(), number.max()                                        # 0-d tensors on the device: the division stays a tensor op
    ramp = (number - first) / (last - first) + 1                                    # 1 at the first bin .. 2 at the last
    return (base_scale * torch.pow(ramp, exp_scale)).float().cpu().numpy()


def int_rows(occ):
    """[M,4] of any real dtype -> int32 numpy, cast as torch.tensor(occ, dtype=torch.int32) casts (toward zero)."""
    if isinstance(occ, torch.Tensor):
        return occ.detach().cpu().to(torch.int32).numpy().reshape(-1, 4)
    return torch.tensor(np.asarray(occ), dtype=torch.int32).numpy().reshape(-1, 4)


def sparse_gaussians(occ, point_cloud_range, voxel_size, base_scale=0.00023, exp_scale=3.7, num_channels=12, scale_device="cpu"):
    """-> dict of numpy arrays xyz, rgb, feat, rot, scale, opacity, unique_classes and the bool is_labeled."""
    X, Y, Z = grid_shape(point_cloud_range, voxel_size)
    ax, ay, az = axis_tables(point_cloud_range, voxel_size)
    zs = scale_table(Z, base_scale, exp_scale, scale_device)
    cells = {}
    for x, y, z, label in int_rows(occ).tolist():
        if not (0 <= x < X and 0 <= y < Y and 0 <= z < Z):
            raise ValueError(f"cell ({x}, {y}, {z}) is outside the {X} x {Y} x {Z} grid")
        cells[(x * Y + y) * Z + z] = min(max(label, 0), NUM_COLORS - 1)              # a later row replaces an earlier one
    classes = set(cells.values())
    if len(cells) < X * Y * Z:
        classes.add(0)                                                              # the zero-filled grid shows through an empty cell
    classes = sorted(classes)
    if len(classes) > num_channels:
        raise ValueError(f"{len(classes)} classes do not fit a one-hot of {num_channels} channels")
    keys = sorted(cells)
    n = len(keys)
    out = {"xyz": np.zeros((n, 3), np.float32), "rgb": np.zeros((n, 3), np.float32), "feat": np.zeros((n, num_channels), np.float32),
           "rot": np.zeros((n, 4), np.float32), "scale": np.zeros((n, 3), np.float32), "opacity": np.ones((n, 1), np.float32)}
    out["rot"][:, 0] = 1
    for g, k in enumerate(keys):
        x, y, z = k // (Y * Z), (k // Z) % Y, k % Z
        out["xyz"][g] = (ax[x], ay[y], az[z])
        out["scale"][g] = zs[z]
        out["feat"][g, classes.index(cells[k])] = 1
    out["unique_classes"] = np.asarray(classes, dtype=np.int64)
    out["is_labeled"] = len(classes) > 1
    return out


@contextlib.contextmanager
def serial():
    """On the CPU torch writes an indexed assignment in parallel chunks, so which of two rows of one cell is kept depends on the thread
    count; on one thread the rows are written in order and the last one stays, which is what the contract states."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def dense_gaussians(occ, point_cloud_range, voxel_size, base_scale=0.00023, exp_scale=3.7, num_channels=12, scale_device="cpu"):
    """The dense formulation the reference uses (prepare_dataset.py:2069-2086 and :2148-2164), in torch on the CPU, for small grids: one
    entry per cell of the grid for every attribute, a label grid filled by indexed assignment, torch.unique over the whole grid, a one-hot
    of its inverse, and a boolean mask that picks the occupied cells.  The grid is flat here, cell (x, y, z) at (x Y + y) Z + z, which is the
    order the reference's reshape gives.  More classes than channels fails inside one_hot, as in the reference."""
    X, Y, Z = grid_shape(point_cloud_range, voxel_size)
    cells = X * Y * Z
    centres = torch.cartesian_prod(*[torch.from_numpy(t) for t in axis_tables(point_cloud_range, voxel_size)])      # [cells, 3], z fastest
    per_cell_scale = torch.from_numpy(scale_table(Z, base_scale, exp_scale, scale_device)).repeat(X * Y)
    attrs = {"xyz": centres, "rgb": torch.zeros(cells, 3), "rot": torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(cells, 1),
             "scale": torch.ones(cells, 3) * per_cell_scale[:, None], "opacity": torch.ones(cells, 1)}
    rows = torch.from_numpy(int_rows(occ)).long()
    assert bool(((rows[:, :3] >= 0) & (rows[:, :3] < torch.tensor([X, Y, Z]))).all()), "a cell outside the grid"
    flat = (rows[:, 0] * Y + rows[:, 1]) * Z + rows[:, 2]
    labels = torch.zeros(cells, dtype=torch.int64)                                 # a fresh grid per call
    with serial():
        labels[flat] = rows[:, 3]
    labels.clamp_(0, NUM_COLORS - 1)
    classes, rank = torch.unique(labels, sorted=True, return_inverse=True)
    attrs["feat"] = torch.nn.functional.one_hot(rank, num_classes=num_channels).float()
    occupied = torch.zeros(cells, dtype=torch.bool)
    occupied[flat] = True
    out = {k: v[occupied].numpy() for k, v in attrs.items()}
    out.update(unique_classes=classes.numpy(), is_labeled=len(classes) > 1)
    return out


FIELDS = ("xyz", "rgb", "feat", "rot", "scale", "opacity", "unique_classes")


def same_gaussians(a, b, skip=()):
    """Bitwise equality of two results (dicts of numpy arrays, or the module's tuple of tensors)."""
    a, b = as_dict(a), as_dict(b)
    for k in FIELDS:
        if k in skip:
            continue
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (k, a[k].shape, b[k].shape, a[k].dtype, b[k].dtype)
        assert a[k].tobytes() == b[k].tobytes(), k
    assert bool(a["is_labeled"]) == bool(b["is_labeled"])


def as_dict(res):
    if isinstance(res, dict):
        return res
    out = {k: v.cpu().numpy() for k, v in zip(FIELDS, res[:7])}
    out["is_labeled"] = res[7]
    return out
