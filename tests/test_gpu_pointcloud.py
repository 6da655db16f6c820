"""Point-cloud cleaning and normals on the MI355X: ``orv_amd.pointcloud`` against the numpy restatement of DESIGN.md §17
(tests/pointcloud_ref.py).  The neighbour search is exact - idx and d2 equal the restatement bit for bit on every case and for every cell
edge; the removal keeps exactly the restatement's points; the normals meet the eigenvector residual and the recorded angle."""
import numpy as np
import pytest
import torch

import pointcloud_cases as cases
import pointcloud_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP32 = float(np.finfo(np.float32).eps)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # a copy: the shared cases are read-only


def host(t):
    return t.cpu().numpy()


def assert_knn(got, want, what):
    (idx, d2), (ridx, rd2) = got, want
    assert idx.dtype == torch.int32 and d2.dtype == torch.float64 and tuple(idx.shape) == ridx.shape and tuple(d2.shape) == rd2.shape, what
    assert np.array_equal(host(idx), ridx), what
    assert host(d2).tobytes() == rd2.tobytes(), what


# ---- the search ----
@pytest.mark.parametrize("name,k", [("surface1", 30), ("surface2", 20), ("lattice", 20), ("lattice3", 30), ("copies", 30), ("collinear", 20),
                                    ("lattice", 64), ("surface1", 1)])
def test_knn_equals_the_restatement_exactly(name, k):
    from orv_amd import pointcloud as pc
    p = dev(cases.points(name))
    before = p.clone()
    idx, d2, stats = pc.knn(p, k, return_stats=True)
    print(f"{name} k={k}: grid {stats['grid']}, cell {stats['cell']:.4g}, {stats['brute']} of {len(p)} queries to the brute kernel")
    assert_knn((idx, d2), cases.knn(name, k), name)
    assert torch.equal(p, before)                                            # the input is left unchanged
    again = pc.knn(p, k)
    assert torch.equal(again[0], idx) and torch.equal(again[1], d2)          # two runs are bit-identical
    if name.startswith("surface") and k >= 20:
        assert stats["brute"] >= 2                                           # the far points reach no full list within the walk


@pytest.mark.parametrize("name,k", [("surface1", 30), ("lattice3", 20), ("collinear", 20)])
def test_knn_does_not_depend_on_the_cell_edge(name, k):
    from orv_amd import pointcloud as pc
    p = dev(cases.points(name))
    want = cases.knn(name, k)
    _, _, auto = pc.knn(p, k, return_stats=True)
    same = pc.knn(p, k, cell=auto["cell"], return_stats=True)
    assert same[2]["grid"] == auto["grid"] and same[2]["cell"] == auto["cell"]
    assert_knn(same[:2], want, "the automatic edge, given")
    small = pc.knn(p, k, cell=0.004, return_stats=True)                       # every distinct point has a cell of its own
    assert small[2]["brute"] > 0
    assert_knn(small[:2], want, "a small edge")
    tiny = pc.knn(p, k, cell=1e-5, return_stats=True)                         # the capped grid covers the middle only: all else is clamped
    assert tiny[2]["grid"][0] * tiny[2]["grid"][1] * tiny[2]["grid"][2] <= pc.MAX_CELLS
    assert_knn(tiny[:2], want, "a tiny edge")
    one = pc.knn(p, k, cell=100.0, return_stats=True)                         # larger than the extent: one cell
    assert one[2]["grid"] == (1, 1, 1) and one[2]["brute"] == 0
    assert_knn(one[:2], want, "one cell")
    mid = pc.knn(p, k, cell=auto["cell"] * 0.37)
    assert_knn(mid, want, "an edge off the automatic one")


@pytest.mark.parametrize("name,k", [("surface2", 30), ("lattice3", 64), ("copies", 20)])
def test_the_brute_kernel_on_every_query_equals_the_grid_kernel(name, k):
    from orv_amd import ops, pointcloud as pc
    p = dev(cases.points(name))
    grid = pc.knn(p, k)
    every = torch.arange(len(p), device=DEV, dtype=torch.int64)
    idx, d2 = ops.pc_knn_brute(p, k, every)
    assert torch.equal(idx, grid[0]) and torch.equal(d2, grid[1])
    assert_knn((idx, d2), cases.knn(name, k), name)


@pytest.mark.parametrize("k", cases.KS)
def test_knn_at_every_small_size(k):
    from orv_amd import pointcloud as pc
    for n in cases.sizes(k):
        p = cases.cloud(n)
        idx, d2, stats = pc.knn(dev(p), k, return_stats=True)
        assert tuple(idx.shape) == (n, min(k, n)), n
        assert_knn((idx, d2), ref.knn(p, k), f"N = {n}, k = {k}")
        if n:
            forced = pc.knn(dev(p), k, cell=0.02)
            assert_knn(forced, ref.knn(p, k), f"N = {n}, k = {k}, small cells")


def test_knn_at_200k_points_against_ckdtree():
    from scipy.spatial import cKDTree
    from orv_amd import pointcloud as pc
    p = cases.surface(n=200_000 - 42, n_out=40, seed=3)
    assert len(p) == 200_000
    idx, d2, stats = pc.knn(dev(p), 30, return_stats=True)
    p64 = p.astype(np.float64)
    dist, tidx = cKDTree(p64).query(p64, k=31, workers=-1)
    clear = dist[:, 29] != dist[:, 30]                                        # the 30th and 31st are apart: the set is unique
    print(f"200k: grid {stats['grid']}, cell {stats['cell']:.4g}, brute {stats['brute']}, unique sets on {clear.mean():.5f} of the points")
    assert clear.mean() >= 0.999
    got = np.sort(host(idx), axis=1)
    assert np.array_equal(got[clear], np.sort(tidx[:, :30], axis=1)[clear])
    assert np.allclose(np.sqrt(host(d2)), dist[:, :30], rtol=1e-12, atol=0)


def test_points_with_nan_or_inf_are_refused():
    from orv_amd import pointcloud as pc
    for bad in (float("nan"), float("inf"), -float("inf")):
        p = dev(cases.cloud(65))
        p[17, 1] = bad
        for call in (lambda: pc.knn(p, 5), lambda: pc.remove_statistical_outlier(p), lambda: pc.estimate_normals(p)):
            with pytest.raises(NotImplementedError, match="NaN or infinite coordinate") as e:
                call()
            assert pc.SUPPORTED in str(e.value)


# ---- the removal ----
@pytest.mark.parametrize("name", ["surface1", "surface2", "lattice3", "collinear"])
def test_removal_equals_the_restatement(name):
    from orv_amd import pointcloud as pc
    p = dev(cases.points(name))
    before = p.clone()
    keep, avg, mean, std, thr, V = cases.removal(name)
    out, ind, st = pc.remove_statistical_outlier(p, 30, 1.5, return_stats=True)
    got_avg, got = host(st["avg"]), [float(st[q]) for q in ("mean", "std", "thr", "valid")]
    rel = np.abs(got_avg - avg) / np.maximum(avg, 1e-300)
    print(f"{name}: {len(p) - len(ind)} removed; avg rel err {rel.max():.2e}; mean {got[0]!r} vs {mean!r}; std {got[1]!r} vs {std!r}; thr {got[2]!r} vs {thr!r}")
    assert np.allclose(got_avg, avg, rtol=1e-13, atol=0)
    assert got[3] == V and np.isclose(got[0], mean, rtol=1e-10, atol=0) and np.isclose(got[1], std, rtol=1e-10, atol=0)
    assert np.isclose(got[2], thr, rtol=1e-10, atol=0)
    assert ind.dtype == torch.int64 and np.array_equal(host(ind), np.flatnonzero(keep))
    assert torch.equal(out, p[ind]) and torch.equal(p, before)
    again = pc.remove_statistical_outlier(p, 30, 1.5, return_stats=True)
    assert torch.equal(again[1], ind) and torch.equal(again[2]["avg"], st["avg"])
    assert all(torch.equal(again[2][q], st[q]) for q in ("mean", "std", "thr"))                  # two runs are bit-identical


def test_removal_with_no_or_one_valid_point_keeps_nothing():
    from orv_amd import pointcloud as pc
    out, ind, st = pc.remove_statistical_outlier(dev(cases.copies()), 30, 1.5, return_stats=True)
    assert len(ind) == 0 and out.shape == (0, 3) and float(st["valid"]) == 0 and bool((st["avg"] == 0).all()) and np.isnan(float(st["mean"]))
    p = np.concatenate([np.ones((5, 3), np.float32), np.array([[1, 1, 3]], np.float32)])
    out, ind, st = pc.remove_statistical_outlier(dev(p), 2, 1.5, return_stats=True)
    assert host(st["avg"]).tolist() == [0, 0, 0, 0, 0, 1.0] and float(st["valid"]) == 1 and float(st["mean"]) == 1.0
    assert np.isnan(float(st["std"])) and np.isnan(float(st["thr"])) and len(ind) == 0
    p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [20, 0, 0]], np.float32)          # the hand-computed case
    out, ind, st = pc.remove_statistical_outlier(dev(p), 2, 1.5, return_stats=True)
    assert host(ind).tolist() == [0, 1, 2, 3, 4] and float(st["mean"]) == 1.75 and float(st["std"]) == np.sqrt(9.375)
    assert len(pc.remove_statistical_outlier(dev(p), 2, 2.5)[1]) == 6
    out, ind = pc.remove_statistical_outlier(torch.zeros(0, 3, device=DEV))
    assert out.shape == (0, 3) and ind.shape == (0,) and ind.dtype == torch.int64


# ---- the normals ----
def check_normals(p, got, k, camera, what):
    """Unit length, the eigenvector residual on every point, the angle on the points with a clear smallest eigenvalue -> the worst angle."""
    idx, _ = ref.knn(p, k)
    n, C, w, cos = ref.normals(p, idx, camera)
    g = got.astype(np.float64)
    assert got.dtype == np.float32 and np.abs(np.linalg.norm(g, axis=1) - 1.0).max() <= 2 * ULP32, what
    res = np.linalg.norm(np.einsum("nij,nj->ni", C, g) - w[:, :1] * g, axis=1)
    frob = np.linalg.norm(C.reshape(len(C), 9), axis=1)
    assert (res <= 1e-6 * frob).all(), (what, float((res / np.maximum(frob, 1e-300)).max()))
    sure = (ref.eigen_gap(w) >= ref.GAP_MIN) & (cos >= 1e-3)
    worst = float(ref.angle(g[sure], n[sure]).max()) if sure.any() else 0.0
    print(f"{what}: residual / |C|_F <= {float((res / np.maximum(frob, 1e-300)).max()):.2e}; worst angle {worst:.3e} rad over {sure.sum()} of {len(p)} points")
    return worst


def test_normals_meet_the_residual_and_the_recorded_angle():
    from orv_amd import pointcloud as pc
    assert 10 * ref.MEASURED_ANGLE <= 1e-5
    worst = 0.0
    for name in ("surface1", "surface2"):
        p = cases.cleaned(name)
        t = dev(p)
        before = t.clone()
        got = pc.estimate_normals(t, 20)
        assert torch.equal(t, before) and torch.equal(pc.estimate_normals(t, 20), got)
        worst = max(worst, check_normals(p, host(got), 20, (0.0, 0.0, 0.0), name))
        away = pc.estimate_normals(t, 20, camera_location=(0.3, -0.1, 1.5))          # a camera above the sheet
        worst = max(worst, check_normals(p, host(away), 20, (0.3, -0.1, 1.5), name + ", camera above"))
        flipped = (host(away) * host(got)).sum(axis=1) < 0
        assert flipped.mean() > 0.9                                                  # the origin is below the sheet
    p = cases.cloud(1025)
    worst = max(worst, check_normals(p, host(pc.estimate_normals(dev(p), 64)), 64, (0.0, 0.0, 0.0), "cloud 1025, k = 64"))
    print(f"worst angle {worst:.3e} rad; recorded {ref.MEASURED_ANGLE:.3e}")
    assert worst <= 10 * ref.MEASURED_ANGLE


def test_normals_of_degenerate_neighbourhoods():
    from orv_amd import pointcloud as pc
    # fewer than three neighbours, and identical neighbours: (0, 0, 1), then the turn towards the camera
    two = dev(np.array([[0, 0, 1], [1, 0, -1]], np.float32))
    assert host(pc.estimate_normals(two, 20)).tolist() == [[0, 0, -1], [0, 0, 1]]
    assert host(pc.estimate_normals(two[:1], 20)).tolist() == [[0, 0, -1]]
    assert host(pc.estimate_normals(dev(cases.cloud(65)), 2, camera_location=(0, 0, 9))).tolist() == [[0, 0, 1]] * 65
    c = dev(cases.copies())                                                           # at (0.25, -0.5, 0.125): the origin is below
    assert host(pc.estimate_normals(c, 20)).tolist() == [[0, 0, -1]] * 100
    assert host(pc.estimate_normals(c, 20, camera_location=(0.0, 0.0, 1.0))).tolist() == [[0, 0, 1]] * 100
    assert pc.estimate_normals(torch.zeros(0, 3, device=DEV)).shape == (0, 3)
    # collinear neighbours: any unit vector across the line conforms; the kernel gives e x u for the axis e of the smallest |u| component
    p = cases.collinear()
    got = host(pc.estimate_normals(dev(p), 20)).astype(np.float64)
    u = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 2 * ULP32 and np.abs(got @ u).max() <= 1e-6
    want = np.cross([1.0, 0.0, 0.0], u)                                               # |u.x| = |u.z| is the smallest: the first such axis
    want = want / np.linalg.norm(want)
    sign = np.where((got @ want) < 0, -1.0, 1.0)
    assert np.abs(got - sign[:, None] * want[None, :]).max() <= 1e-6
    check_normals(p, got.astype(np.float32), 20, (0.0, 0.0, 0.0), "collinear")
    # an exact plane: the normal is the axis, exactly
    rng = np.random.default_rng(0)
    plane = np.concatenate([rng.integers(-64, 64, (300, 2)) / 64.0, np.full((300, 1), 2.0)], axis=1).astype(np.float32)
    assert host(pc.estimate_normals(dev(plane), 10)).tolist() == [[0, 0, -1]] * 300
    assert host(pc.estimate_normals(dev(plane), 10, camera_location=(0, 0, 5))).tolist() == [[0, 0, 1]] * 300


def test_orientation_alone():
    from orv_amd import pointcloud as pc
    pts = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0], [1, 0, 0], [0.5, 0.25, -2]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    got = host(pc.orient_normals_towards_camera_location(dev(pts), dev(nrm)))
    assert got[:4].tolist() == [[0, 0, -1], [0, 0, -1], [0, 0, 1], [-1, 0, 0]] and np.array_equal(got, ref.orient(pts, nrm))
    rng = np.random.default_rng(5)
    p, n = rng.normal(0, 1, (1025, 3)).astype(np.float32), rng.normal(0, 1, (1025, 3)).astype(np.float32)
    n[::7] = 0
    for cam in ((0.0, 0.0, 0.0), (0.5, -2.0, 3.0)):
        tp, tn = dev(p), dev(n)
        got = pc.orient_normals_towards_camera_location(tp, tn, cam)
        assert np.array_equal(host(got), ref.orient(p, n, cam)) and torch.equal(tn, dev(n)) and torch.equal(tp, dev(p))
    p[3] = (0.5, -2.0, 3.0)                                                            # a zero normal at the camera itself
    n[3] = 0
    assert host(pc.orient_normals_towards_camera_location(dev(p), dev(n), (0.5, -2.0, 3.0)))[3].tolist() == [0, 0, 1]


# ---- the composed calls ----
def test_preprocess_points_and_nksr_inputs_are_the_composition_of_the_parts():
    from orv_amd import pointcloud as pc
    p = cases.points("surface1").copy()
    p[::11, 2] += 0.5                                                                  # some points above z_max
    t = dev(p)
    colours = torch.arange(len(p) * 3, device=DEV, dtype=torch.float32).reshape(-1, 3)
    labels = torch.arange(len(p), device=DEV)
    before = t.clone()
    low = torch.nonzero(t[:, 2] < 0.6).flatten()
    assert 0 < len(low) < len(p)
    want, ind = pc.remove_statistical_outlier(t[low], 30, 1.5)
    got = pc.preprocess_points(t)
    assert torch.equal(got, want) and 0 < len(got) < len(low)
    got, (c, l) = pc.preprocess_points(t, attrs=(colours, labels))
    assert torch.equal(got, want) and torch.equal(c, colours[low[ind]]) and torch.equal(l, labels[low[ind]])
    assert torch.equal(t[l], got)                                                      # the attributes followed both masks
    got2, c2 = pc.preprocess_points(t, z_max=0.4, nb_neighbors=20, std_ratio=2.0, attrs=colours)
    low2 = torch.nonzero(t[:, 2] < 0.4).flatten()
    want2, ind2 = pc.remove_statistical_outlier(t[low2], 20, 2.0)
    assert torch.equal(got2, want2) and torch.equal(c2, colours[low2[ind2]])
    xyz, normal = pc.nksr_inputs(got)
    assert xyz.dtype == torch.float32 and normal.dtype == torch.float32 and xyz.is_cuda and normal.is_cuda and xyz.shape == normal.shape
    assert torch.equal(xyz, got) and torch.equal(normal, pc.estimate_normals(got, 20))
    assert torch.equal(pc.nksr_inputs(got, max_nn=10)[1], pc.estimate_normals(got, 10))
    assert torch.equal(t, before)
