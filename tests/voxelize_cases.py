"""The voxelization fixtures of tests/golden/voxelize/ (written by tools/gen_voxelize_golden.py from the reference's own CPU kernels) and the
seeded point clouds that are too large to store, shared by the host and the GPU tests."""
import functools
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxelize")
HARD = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if not os.path.basename(p).startswith("vote_"))
VOTE = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "vote_*.npz")))
REAL_RANGE, REAL_VOXEL = [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4], [0.001, 0.001, 0.001]       # the reference's 400^3 occupancy grid


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def tie_voxels(fx):
    """True where a vote fixture's voxel has more than one non-zero stored label with the largest count."""
    counts = fx["label_counts"].astype(np.int64)[:, 1:]
    return (counts == counts.max(axis=1, keepdims=True)).sum(axis=1) > 1


def vote_range(fx):
    return None if fx["coors_range"].size == 0 else [float(v) for v in fx["coors_range"]]


def surface_points(seed, n, lo, hi, thickness, C=4):
    """n points about a curved surface inside [lo, hi] (some fall outside), many per voxel near it; features past z are random."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    xy = rng.uniform(lo[:2], hi[:2], size=(n, 2))
    u = (xy - lo[:2]) / (hi[:2] - lo[:2])
    z = lo[2] + (hi[2] - lo[2]) * (0.5 + 0.3 * np.sin(3.0 * u[:, 0]) * np.cos(2.0 * u[:, 1])) + rng.normal(0.0, thickness, n)
    return np.concatenate([xy, z[:, None], rng.uniform(size=(n, C - 3))], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cloud(name):
    """-> (points, voxel_size, coors_range, max_points, max_voxels) of a seeded case."""
    if name == "n70001_grid40":                        # crosses wave, workgroup and multi-block boundaries; both caps bite
        pts = np.random.default_rng(70001).uniform(-0.02, 0.42, size=(70001, 4)).astype(np.float32)
        return pts, [0.01] * 3, [0.0, 0.0, 0.0, 0.4, 0.4, 0.4], 3, 20000
    if name == "real_geometry":                        # 400^3 cells, 50 000 points clustered on a surface (x, y in a patch: several per voxel)
        pts = surface_points(50000, 50000, [-0.05, -0.05, 0.0], [0.05, 0.05, 0.4], 0.0004)
        return pts, REAL_VOXEL, REAL_RANGE, 100, 100000
    if name == "huge_grid":                            # 2000^3 = 8e9 cells: keys past 2^31 (and past 2^32)
        rng = np.random.default_rng(2000)
        base = rng.uniform(0.0, 2.0, size=(600, 3))
        pts = np.repeat(base, 5, axis=0) + rng.uniform(0.0, 0.0004, size=(3000, 3))
        pts = np.concatenate([pts, rng.uniform(size=(3000, 1))], 1).astype(np.float32)[rng.permutation(3000)]
        return pts, [0.001] * 3, [0.0, 0.0, 0.0, 2.0, 2.0, 2.0], 4, 500
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cloud_ref(name):
    import voxelize_ref as ref
    pts, vs, rng, max_points, max_voxels = cloud(name)
    return ref.hard(pts, vs, rng, max_points, max_voxels) + (ref.dynamic(pts, vs, rng),)
