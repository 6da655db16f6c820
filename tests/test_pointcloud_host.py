"""Point-cloud cleaning and normals, host side (no GPU): the numpy restatement of the contract (tests/pointcloud_ref.py) against
``scipy.spatial.cKDTree`` and hand-computed cases, the conditions the seeded cases must meet for the GPU tests to mean something, the Python
surface of ``orv_amd.pointcloud`` (refusals) and the C ABI of the ``orv_pc_*`` entry points (argument validation happens before any launch)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import pointcloud_cases as cases
import pointcloud_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACES = ("surface1", "surface2")


# ---- the restatement ----
@pytest.mark.parametrize("name", SURFACES)
def test_ref_neighbour_sets_equal_ckdtree_on_every_point(name):
    p = cases.points(name)
    idx, d2 = cases.knn(name, 30)
    assert len(p) == 3042 and idx.shape == (3042, 30) and idx.dtype == np.int32 and d2.dtype == np.float64
    dist, tree_idx = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=30)
    assert np.array_equal(np.sort(idx, axis=1), np.sort(tree_idx, axis=1))
    assert np.allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0) and (np.diff(d2, axis=1) >= 0).all() and (idx[:, 0] == np.arange(3042)).all()


@pytest.mark.parametrize("name,k", [("lattice", 20), ("lattice3", 30)])
def test_ref_takes_the_smallest_indices_among_ckdtrees_equidistant_candidates(name, k):
    p = cases.points(name).astype(np.float64)
    idx, d2 = cases.knn(name, k)
    tree = cKDTree(p)
    ties = 0
    for i in range(0, len(p), 7):
        last = d2[i, -1]
        cand = np.array(sorted(tree.query_ball_point(p[i], np.sqrt(last) * (1 + 1e-9))))
        dc = ((p[cand] - p[i]) ** 2).sum(axis=1)                       # exact: lattice coordinates are multiples of 1/64
        assert (dc <= last).all() and len(cand) >= k
        inside, edge = cand[dc < last], cand[dc == last]
        ties += len(inside) + len(edge) > k
        want = np.concatenate([inside, edge[:k - len(inside)]])        # every closer point, then the smallest indices at the last distance
        assert set(idx[i].tolist()) == set(want.tolist()), i
        order = np.lexsort((idx[i], d2[i]))
        assert np.array_equal(order, np.arange(k)), i                   # ascending in (d2, index)
    assert ties > 50


def test_ref_handles_duplicates_and_short_clouds():
    idx, d2 = ref.knn(cases.copies(), 30)
    assert np.array_equal(idx, np.tile(np.arange(30, dtype=np.int32), (100, 1))) and (d2 == 0).all()      # a point need not be in its own list
    idx, d2 = ref.knn(cases.cloud(3), 20)
    assert idx.shape == (3, 3) and (idx[:, 0] == np.arange(3)).all()
    idx, d2 = ref.knn(np.zeros((0, 3), np.float32), 5)
    assert idx.shape == (0, 0) and d2.shape == (0, 0)


def test_removal_formula_by_hand():
    # five points one apart and a sixth 16 away, two neighbours (self and the nearest): avg = 0.5 x 5 and 8
    p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [20, 0, 0]], np.float32)
    _, d2 = ref.knn(p, 2)
    keep, avg, mean, std, thr, V = ref.outlier(d2, 1.5)
    assert avg.tolist() == [0.5, 0.5, 0.5, 0.5, 0.5, 8.0] and V == 6 and mean == 1.75
    assert std == np.sqrt(46.875 / 5) and thr == 1.75 + 1.5 * np.sqrt(9.375)       # 6.34...: the far point goes
    assert keep.tolist() == [True] * 5 + [False]
    assert ref.outlier(d2, 2.5)[0].all()                                            # thr = 9.40...: everything stays
    # V == 0: six copies, every avg is zero, nothing is kept
    keep, avg, mean, std, thr, V = ref.outlier(ref.knn(np.ones((6, 3), np.float32), 2)[1], 1.5)
    assert V == 0 and not keep.any() and (avg == 0).all() and np.isnan(mean)
    # V == 1: five copies and one other point; only that one has a positive avg, std is 0 / 0 and nothing is kept
    p = np.concatenate([np.ones((5, 3), np.float32), np.array([[1, 1, 3]], np.float32)])
    keep, avg, mean, std, thr, V = ref.outlier(ref.knn(p, 2)[1], 1.5)
    assert V == 1 and avg.tolist() == [0, 0, 0, 0, 0, 1.0] and mean == 1.0 and np.isnan(std) and np.isnan(thr) and not keep.any()


@pytest.mark.parametrize("name", SURFACES)
def test_seeded_surfaces_meet_the_conditions_the_gpu_tests_rely_on(name):
    keep, avg, mean, std, thr, V = cases.removal(name)
    gap = np.abs(avg - thr) / thr
    print(f"{name}: {(~keep).sum()} points removed, nearest avg to thr at relative distance {gap.min():.2e}")
    assert V == 3042 and gap.min() >= 1e-6                  # no point sits on the threshold: the kept set is stable under rounding
    assert not keep[-2:].any() and 2 <= (~keep).sum() <= 60 and keep[:3000].mean() > 0.99                   # the far points go, the sheet stays
    idx, n, C, w, cos = cases.cleaned_normals(name)
    share = (ref.eigen_gap(w) >= ref.GAP_MIN).mean()
    print(f"{name}: eigen-gap >= {ref.GAP_MIN} on {share:.4%} of the points, min |cos(n, camera - p)| = {cos.min():.2e}")
    assert share >= 0.99 and cos.min() >= 1e-3


@pytest.mark.parametrize("name", ["lattice3", "collinear"])
def test_tied_cases_keep_their_averages_off_the_threshold_too(name):
    keep, avg, mean, std, thr, V = cases.removal(name)
    assert V == len(avg) and (np.abs(avg - thr) / thr).min() >= 1e-6 and 0 < keep.sum()


def test_ref_normals_on_a_plane_and_the_orientation_rule():
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.uniform(-1, 1, (50, 2)), np.full((50, 1), 2.0)], axis=1).astype(np.float32)
    idx, _ = ref.knn(p, 10)
    n, C, w, cos = ref.normals(p, idx)
    assert np.allclose(n, (0, 0, -1), atol=1e-12)            # towards the origin, below the plane
    n = ref.normals(p, idx, camera=(0, 0, 5))[0]
    assert np.allclose(n, (0, 0, 1), atol=1e-12)
    assert (ref.normals(p, idx[:, :2])[0] == (0, 0, -1)).all()                                   # fewer than three neighbours: (0, 0, 1), then turned
    pts = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0], [1, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    assert ref.orient(pts, nrm).tolist() == [[0, 0, -1], [0, 0, -1], [0, 0, 1], [-1, 0, 0]]       # flipped; zero -> towards the camera; at it -> (0, 0, 1)


# ---- Python surface ----
SUPPORTED = "supported: a contiguous CUDA float32 tensor points [N,3] with finite coordinates"


def test_refusals_name_the_supported_set():
    from orv_amd import pointcloud as pc
    assert SUPPORTED in pc.SUPPORTED and "1 <= k <= 64" in pc.SUPPORTED and "no radius or hybrid search" in pc.SUPPORTED
    pts = torch.zeros(8, 3)
    calls = (lambda p: pc.knn(p, 5), lambda p: pc.remove_statistical_outlier(p), lambda p: pc.estimate_normals(p),
             lambda p: pc.orient_normals_towards_camera_location(p, p), lambda p: pc.preprocess_points(p), lambda p: pc.nksr_inputs(p))
    for call in calls:
        with pytest.raises(NotImplementedError, match="not a CUDA tensor") as e:
            call(pts)
        assert SUPPORTED in str(e.value) and "there is no CPU path" in str(e.value)
        with pytest.raises(NotImplementedError, match="torch.float64, not float32") as e:
            call(pts.double())
        assert SUPPORTED in str(e.value)
        for bad in (torch.zeros(8, 4), torch.zeros(8), torch.zeros(2, 4, 3)):
            with pytest.raises(NotImplementedError, match=r"not \[N,3\]") as e:
                call(bad)
            assert SUPPORTED in str(e.value)
        with pytest.raises(NotImplementedError, match="no backward") as e:
            call(torch.zeros(8, 3, requires_grad=True))
        assert SUPPORTED in str(e.value)
        with pytest.raises(NotImplementedError, match="not contiguous") as e:
            call(torch.zeros(3, 8).t())
        assert SUPPORTED in str(e.value)
        with pytest.raises(NotImplementedError, match="is a ndarray, not a tensor"):
            call(np.zeros((8, 3), np.float32))
    with pytest.raises(NotImplementedError, match="`normals` is torch.float64"):
        pc.orient_normals_towards_camera_location(pts, pts.double())
    # the neighbour count is checked ahead of the device: 1..64, integers
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(NotImplementedError, match=r"not an integer in \[1, 64\]") as e:
            pc.knn(pts, bad)
        assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match=r"nb_neighbors = 65"):
        pc.remove_statistical_outlier(pts, nb_neighbors=65)
    with pytest.raises(NotImplementedError, match=r"nb_neighbors = 0"):
        pc.preprocess_points(pts, nb_neighbors=0)
    with pytest.raises(NotImplementedError, match=r"max_nn = 100"):
        pc.estimate_normals(pts, max_nn=100)
    with pytest.raises(NotImplementedError, match="radius or hybrid search") as e:
        pc.estimate_normals(pts, max_nn=20, radius=0.1)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="radius or hybrid search"):
        pc.knn(pts, 5, radius=0.05)
    assert not hasattr(pc, "install")


def test_signatures():
    from orv_amd import pointcloud as pc
    d = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items()}
    assert list(d(pc.knn))[:4] == ["points", "k", "cell", "return_stats"] and d(pc.knn)["cell"] is None and d(pc.knn)["return_stats"] is False
    s = d(pc.remove_statistical_outlier)
    assert list(s) == ["points", "nb_neighbors", "std_ratio", "return_stats"] and (s["nb_neighbors"], s["std_ratio"]) == (30, 1.5)
    s = d(pc.estimate_normals)
    assert list(s)[:3] == ["points", "max_nn", "camera_location"] and s["max_nn"] == 20 and tuple(s["camera_location"]) == (0.0, 0.0, 0.0)
    s = d(pc.orient_normals_towards_camera_location)
    assert list(s) == ["points", "normals", "camera_location"] and tuple(s["camera_location"]) == (0.0, 0.0, 0.0)
    s = d(pc.preprocess_points)
    assert list(s) == ["points", "z_max", "nb_neighbors", "std_ratio", "attrs"] and (s["z_max"], s["nb_neighbors"], s["std_ratio"], s["attrs"]) == (0.6, 30, 1.5, None)
    assert list(d(pc.nksr_inputs)) == ["points", "max_nn"] and d(pc.nksr_inputs)["max_nn"] == 20
    import orv_amd
    assert orv_amd.preprocess_points is pc.preprocess_points and orv_amd.nksr_inputs is pc.nksr_inputs
    for text in (pc.__doc__, open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read(), open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()):
        assert re.search(r"parity\s+with\s+open3d\s+is\s+unpinned", text, re.I)


def test_the_automatic_edge_follows_the_occupancy():
    from orv_amd import pointcloud as pc
    # a sheet: occupancy grows fourfold per level; 1e6 points at 7.5 per cell want ~365 cells along the axis
    occ = [m * m for m in pc._LEVELS]
    edge = pc._auto_edge(1_000_000, 30, 1.0, occ)
    assert 1 / 420 < edge < 1 / 320
    # 3000 points on the same sheet: level 16 holds 11.7 per cell, level 32 2.9 -> between them
    edge = pc._auto_edge(3000, 30, 0.4, occ)
    assert 0.4 / 32 < edge < 0.4 / 16
    # fewer points than cells anywhere: coarser than the coarsest trial grid, and never below one cell
    assert pc._auto_edge(5, 30, 2.0, [5, 5, 5, 5, 5]) == 2.0


# ---- C ABI ----
NAMES = ("orv_pc_cells", "orv_pc_cell_table", "orv_pc_knn", "orv_pc_knn_brute", "orv_pc_outlier", "orv_pc_normals", "orv_pc_orient")


def test_pc_symbols_are_declared_exported_and_bound():
    from orv_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(_lib.lib(), name) is not None
        doc = hdr[hdr.index("Point-cloud cleaning and normals"):hdr.index("int " + name + "(")]
        assert "prepare_dataset.py:786-875" in doc and ":806-822" in doc and ":729-741" in doc and "PARITY UNPINNED" in doc
        assert callable(getattr(ops, name[4:]))
        end = hdr.index("int " + name + "(")
        assert re.search(r":\d{3}", hdr[hdr.rindex("/*", 0, end):end]), name        # each cites the reference lines it replaces
    assert "orv_pc_outlier_workspace" in _lib.SIGNATURES and _lib.lib().orv_pc_outlier_workspace(1025) == 2 * 2 * 8
    with open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile"), "r", encoding="utf-8") as f:
        assert "pointcloud.hip" in f.read()


def test_pc_entry_points_validate_before_any_launch():
    """Null pointers, N < 0, k outside 1..64, a non-positive cell edge or grid: nonzero with the reason in orv_last_error(), prefixed by the
    entry point's name, without a GPU (no pointer is followed)."""
    from orv_amd._lib import lib
    h = lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lambda: h.orv_last_error().decode()

    def cells(points=p, N=4, o=(0.0, 0.0, 0.0), cell=0.1, g=(4, 4, 4), keys=p):
        return h.orv_pc_cells(points, N, *o, cell, *g, keys, None)

    def table(keys=p, order=p, points=p, N=4, n_cells=64, start=p, spts=p):
        return h.orv_pc_cell_table(keys, order, points, N, n_cells, start, spts, None)

    def knn(spts=p, order=p, start=p, N=4, k=3, o=(0.0, 0.0, 0.0), cell=0.1, g=(4, 4, 4), idx=p, d2=p, pending=p):
        return h.orv_pc_knn(spts, order, start, N, k, *o, cell, *g, idx, d2, pending, None)

    def brute(points=p, N=4, k=3, queries=p, Q=2, idx=p, d2=p):
        return h.orv_pc_knn_brute(points, N, k, queries, Q, idx, d2, None)

    def outl(d2=p, N=4, k=3, ratio=1.5, avg=p, stats=p, keep=p, ws=p, nbytes=64):
        return h.orv_pc_outlier(d2, N, k, ratio, avg, stats, keep, ws, nbytes, None)

    def nrm(points=p, idx=p, N=4, k=3, cam=(0.0, 0.0, 0.0), out=p):
        return h.orv_pc_normals(points, idx, N, k, *cam, out, None)

    def ori(points=p, normals=p, N=4, cam=(0.0, 0.0, 0.0), out=p):
        return h.orv_pc_orient(points, normals, N, *cam, out, None)

    every = dict(zip(NAMES, (cells, table, knn, brute, outl, nrm, ori)))
    for name, call in every.items():
        assert call(N=-1) != 0 and "N must not be negative" in err() and err().startswith(name + ":"), name
    for name in ("orv_pc_knn", "orv_pc_knn_brute", "orv_pc_outlier", "orv_pc_normals"):
        for bad in (0, 65, -3):
            assert every[name](k=bad) != 0 and f"k = {bad} neighbours" in err() and "1 to 64" in err() and err().startswith(name + ":"), (name, bad)
    for name in ("orv_pc_cells", "orv_pc_knn"):
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            assert every[name](cell=bad) != 0 and "cell edge must be positive" in err() and err().startswith(name + ":"), (name, bad)
        for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (4096, 4096, 4096)):
            assert every[name](g=bad) != 0 and "cells" in err() and "at least 1 per axis" in err() and err().startswith(name + ":"), (name, bad)
        assert every[name](o=(0.0, float("nan"), 0.0)) != 0 and "origin must be finite" in err()
    assert table(n_cells=0) != 0 and "n_cells = 0" in err()
    assert brute(Q=-1) != 0 and "Q = -1" in err() and brute(Q=5) != 0 and "Q = 5" in err()
    assert outl(ratio=float("nan")) != 0 and "std_ratio must be finite" in err()
    assert outl(nbytes=8) != 0 and "orv_pc_outlier_workspace(4) = 16" in err()
    assert nrm(cam=(0.0, float("inf"), 0.0)) != 0 and "camera location must be finite" in err()
    assert ori(cam=(float("nan"), 0.0, 0.0)) != 0 and "camera location must be finite" in err()
    nulls = {"orv_pc_cells": ("points", "keys"), "orv_pc_cell_table": ("keys", "order", "points", "start", "spts"),
             "orv_pc_knn": ("spts", "order", "start", "idx", "d2", "pending"), "orv_pc_knn_brute": ("points", "queries", "idx", "d2"),
             "orv_pc_outlier": ("d2", "avg", "stats", "keep", "ws"), "orv_pc_normals": ("points", "idx", "out"),
             "orv_pc_orient": ("points", "normals", "out")}
    for name, args in nulls.items():
        for a in args:
            assert every[name](**{a: None}) != 0 and "null pointer" in err() and err().startswith(name + ":"), (name, a)
    assert cells(keys=p + 4) != 0 and "aligned" in err()
    # nothing to do is not an error, and launches nothing
    assert cells(N=0, points=None, keys=None) == 0 and table(N=0, keys=None, start=None) == 0 and knn(N=0, spts=None, idx=None) == 0
    assert brute(N=0, Q=0, points=None) == 0 and brute(Q=0, queries=None) == 0 and outl(N=0, d2=None, avg=None, ws=None, nbytes=0) == 0
    assert nrm(N=0, points=None, out=None) == 0 and ori(N=0, points=None, out=None) == 0
    assert h.orv_pc_outlier_workspace(0) == 0 and h.orv_pc_outlier_workspace(-5) == 0 and h.orv_pc_outlier_workspace(1024) == 16
