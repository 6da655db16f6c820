"""Seeded point clouds for the point-cloud tests, and the restatement's results on them, computed once and shared (read-only) by the tests."""
import functools

import numpy as np

import pointcloud_ref as ref

FAR = ((3.0, 3.0, 5.0), (-4.0, 2.0, 0.55))


def surface(n=3000, n_out=40, seed=1, far=True):
    """A wavy sheet z = 0.2 + 0.05 sin(12 x) cos(9 y) + N(0, 0.0008) over +-0.2 x +-0.2, ``n_out`` stray points above it in z [0.3, 0.58]
    and the two far points: what the statistical removal is for.  The far points also force the clamped border cells and the brute path."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n)
    z = 0.2 + 0.05 * np.sin(12 * x) * np.cos(9 * y) + rng.normal(0.0, 0.0008, n)
    out = np.stack([rng.uniform(-0.2, 0.2, n_out), rng.uniform(-0.2, 0.2, n_out), rng.uniform(0.3, 0.58, n_out)], axis=1)
    parts = [np.stack([x, y, z], axis=1), out] + ([np.array(FAR)] if far else [])
    return np.concatenate(parts).astype(np.float32)


def lattice(repeat=1):
    """The 9 x 9 x 9 integer lattice scaled by 1/64 (exact in fp32: every distance is tied many times over), each point ``repeat`` times."""
    g = np.arange(9, dtype=np.float32) / 64
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.repeat(p, repeat, axis=0).astype(np.float32)


def copies(n=100):
    return np.tile(np.array([[0.25, -0.5, 0.125]], np.float32), (n, 1))


def collinear(n=200):
    """Exactly collinear in fp32: (0.125, -0.25, 0.5) + i (1, 2, -1) / 64."""
    i = np.arange(n, dtype=np.float32)[:, None]
    return (np.array([[0.125, -0.25, 0.5]], np.float32) + i * np.array([[1.0, 2.0, -1.0]], np.float32) / 64).astype(np.float32)


def cloud(n, seed=7):
    return np.random.default_rng(seed + n).normal(0.0, 0.3, (n, 3)).astype(np.float32)


KS = (1, 20, 30, 64)


def sizes(k):
    return sorted({0, 1, 2, 3, k - 1, k, k + 1, 63, 64, 65, 1025})


NAMED = {"surface1": lambda: surface(seed=1), "surface2": lambda: surface(seed=2), "lattice": lattice, "lattice3": lambda: lattice(3),
         "copies": copies, "collinear": collinear}


@functools.lru_cache(maxsize=None)
def points(name):
    p = NAMED[name]()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def knn(name, k):
    idx, d2 = ref.knn(points(name), k)
    idx.setflags(write=False), d2.setflags(write=False)
    return idx, d2


@functools.lru_cache(maxsize=None)
def removal(name, k=30, std_ratio=1.5):
    """-> (keep, avg, mean, std, thr, V) of the restatement."""
    return ref.outlier(knn(name, k)[1], std_ratio)


@functools.lru_cache(maxsize=None)
def cleaned(name):
    """The surface case after the restatement's removal at (30, 1.5): what the normals are estimated on."""
    p = points(name)[removal(name)[0]].copy()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def cleaned_normals(name, k=20):
    p = cleaned(name)
    idx, _ = ref.knn(p, k)
    return (idx,) + ref.normals(p, idx)
