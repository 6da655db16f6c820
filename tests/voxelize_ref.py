"""CPU restatement (numpy) of the voxelization contract of DESIGN.md §13: dynamic and hard voxelization as the sequential walk of the
reference's CPU kernel (``orv/ops/voxelize/voxelization_cpu.cpp:7-102``) and the semantic vote of ``points_to_voxels``
(``orv/dataset/prepare_dataset.py:179-196``).  The walk keeps a dict from cell to voxel number, so there is no dense grid and any grid size
works.  Everything the GPU path returns is compared with this for exact equality."""
import math

import numpy as np

MAX_LABEL = 255


def f32(values):
    """python floats / numpy values -> fp32, rounded to nearest as ``torch.tensor(values, dtype=torch.float)`` rounds."""
    return np.asarray(values, dtype=np.float64).astype(np.float32)


def grid_size(voxel_size, coors_range):
    """Cells per axis (x, y, z): round((hi - lo) / vs) with the subtraction and the division in fp32 and C's round (halves away from zero)."""
    vs, rng = f32(voxel_size), f32(coors_range)
    out = []
    for a in range(3):
        q = float(np.float32(np.float32(rng[3 + a] - rng[a]) / vs[a]))
        out.append(int(math.copysign(math.floor(abs(q) + 0.5), q)))
    return tuple(out)


def dynamic(points, voxel_size, coors_range):
    """-> coors int32 [N,3] in (z, y, x) order; (-1, -1, -1) for a point outside the grid or with a NaN / infinite coordinate."""
    pts = np.asarray(points, dtype=np.float32)
    vs, rng, grid = f32(voxel_size), f32(coors_range), grid_size(voxel_size, coors_range)
    N = pts.shape[0]
    coors = np.full((N, 3), -1, dtype=np.int32)
    ok = np.ones(N, dtype=bool)
    cells = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            f = np.floor((pts[:, a] - rng[a]) / vs[a])                     # fp32 - fp32, then a correctly rounded fp32 divide
            assert f.dtype == np.float32
            good = np.isfinite(f) & (f >= 0) & (f < 2147483648.0)
            c = np.where(good, f, -1).astype(np.int64)
            ok &= good & (c < grid[a])
            cells.append(c)
    for a in range(3):
        coors[ok, 2 - a] = cells[a][ok]
    return coors


def hard(points, voxel_size, coors_range, max_points, max_voxels):
    """-> (voxels [M, max_points, C] zero-padded, coors int32 [M,3] (z, y, x), num_points_per_voxel int32 [M]): points walked in index order,
    voxels numbered by first appearance, a voxel met once ``max_voxels`` are open is dropped with all its later points, slots in point order."""
    pts = np.asarray(points, dtype=np.float32)
    pc = dynamic(pts, voxel_size, coors_range)
    number, members = {}, []
    for i in range(pts.shape[0]):
        if pc[i, 0] < 0:
            continue
        cell = (int(pc[i, 0]), int(pc[i, 1]), int(pc[i, 2]))
        v = number.get(cell)
        if v is None:
            if len(members) >= max_voxels:
                continue
            v = number[cell] = len(members)
            members.append([])
        if len(members[v]) < max_points:
            members[v].append(i)
    M = len(members)
    voxels = np.zeros((M, max_points, pts.shape[1]), dtype=np.float32)
    coors, num = np.zeros((M, 3), dtype=np.int32), np.zeros(M, dtype=np.int32)
    for v, idx in enumerate(members):
        voxels[v, :len(idx)] = pts[idx]
        coors[v] = pc[idx[0]]
        num[v] = len(idx)
    return voxels, coors, num


def label_counts(voxels):
    """-> int64 [M, 256]: how often each stored label (the last feature, label + 1; 0 = padding) occurs in each voxel."""
    stored = voxels[..., -1].astype(np.int64)
    counts = np.zeros((voxels.shape[0], MAX_LABEL + 1), dtype=np.int64)
    for v in range(voxels.shape[0]):
        counts[v] = np.bincount(stored[v], minlength=MAX_LABEL + 1)
    return counts


def vote(voxels):
    """-> int64 [M]: the most frequent non-zero stored label of each voxel, minus one; a tie goes to the smallest label."""
    counts = label_counts(voxels)[:, 1:]
    return counts.argmax(axis=1).astype(np.int64)            # argmax returns the first (smallest) label among equal counts; stored - 1 = index


def points_to_voxels(points, voxel_size=(0.2, 0.2, 0.2), labels=None, point_cloud_range=None, max_points=100, max_voxels=100000):
    """The whole of the reference's ``points_to_voxels`` -> float64 [M,4] of x, y, z, label."""
    pts = np.asarray(points, dtype=np.float32)
    lab = np.zeros(pts.shape[0], dtype=np.float32) if labels is None else np.asarray(labels).astype(np.int32).astype(np.float32)
    pts = np.concatenate([pts[:, :3], lab[:, None] + 1], axis=1)
    pts = pts[~np.isnan(pts[:, :3]).any(axis=1)]
    if point_cloud_range is None:
        point_cloud_range = np.concatenate([pts[:, :3].min(0), pts[:, :3].max(0)])
    voxels, coors, _ = hard(pts, voxel_size, point_cloud_range, max_points, max_voxels)
    return np.concatenate([coors[:, ::-1].astype(np.float64), vote(voxels)[:, None].astype(np.float64)], axis=1)
