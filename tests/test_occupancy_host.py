"""Occupancy labelling and scene preparation, host side (no GPU): the CPU restatement of the contract (tests/occupancy_ref.py) against every
fixture the reference's own statements produced (tests/golden/occupancy/), the sparse restatement against the dense one on small grids, the
Python surface of ``orv_amd.occupancy`` (refusals) and the C ABI of the ``orv_occ_*`` entry points (validation before any launch)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import occupancy_ref as ref
from orv_amd import occupancy as oc          # every test here is about this module: none passes without it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "occupancy")
SCENES = ("scene_small", "scene_duplicates", "scene_full", "scene_single_class", "scene_grid40")
SMALL = ([0.0, 0.0, 0.0, 1.0, 0.75, 0.625], [0.125] * 3)          # 8 x 6 x 5 cells: unequal axes, so an axis mix-up shows


def fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def ulps(a, b):
    """Distance in units of the last place between two positive fp32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- the restatement equals the reference ----
def test_there_are_fixtures():
    have = {f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")}
    assert have == {"project_exact", "project_real", *SCENES}


def test_projection_restatement_equals_the_reference_where_the_arithmetic_is_exact():
    fx = fixture("project_exact")
    assert fx["labels2d"].shape == (12, 16) and fx["labels2d"].dtype == np.uint8 and (fx["labels2d"] == 255).any()
    got = ref.project_labels(fx["points"], fx["labels2d"], fx["P"])
    assert got.dtype == np.int64 and np.array_equal(got, fx["labels3d"])
    u, v = ref.pixels(fx["points"], fx["P"])
    inside, _, _ = ref.pixel_index(u, v, 12, 16)
    assert (~np.isfinite(u)).any() and inside.any() and (~inside).any() and (got == 59).any()      # h_2 = 0, both outcomes, 255 -> 59
    assert (inside & (fx["points"][:, 2] < -0.125)).any()                                          # behind the camera and counted
    # the matrix the reference formed is the exact one, so any backend's inverse gives these bits
    P = torch.from_numpy(fx["intrin"]) @ torch.linalg.inv(torch.from_numpy(fx["extrin"]))
    assert np.array_equal(P.numpy(), fx["P"])


def test_projection_restatement_against_the_reference_at_the_real_geometry():
    """The reference multiplies [N,4] by P^T as one fp32 matrix product, whose summation order is the BLAS's; the contract fixes the order.
    Condition (not a measurement): at most 0.1 % of the labels differ, and a differing point's pixel differs by one step in one coordinate."""
    fx = fixture("project_real")
    assert fx["labels2d"].shape == (480, 640) and len(fx["points"]) == 20000
    got = ref.project_labels(fx["points"], fx["labels2d"], fx["P"])
    diff = np.flatnonzero(got != fx["labels3d"])
    print(f"project_real: {len(diff)} of 20000 labels differ")
    assert len(diff) <= 20
    u, v = ref.pixels(fx["points"], fx["P"])
    mine = np.stack([np.trunc(u), np.trunc(v)], 1).astype(np.int64)
    step = np.abs(mine - fx["ref_pixels"])
    moved = np.flatnonzero(step.any(1))
    print(f"project_real: {len(moved)} of 20000 pixels differ")
    assert len(moved) <= 20 and set(diff) <= set(moved) and (step[moved].sum(1) == 1).all()
    assert (got != 0).sum() > 15000 and (got == 59).sum() > 500


def test_scaled_intrinsics_is_the_references_fp32_scaling():
    k = np.array([[487.3, 0.0, 255.9], [0.0, 488.1, 191.7], [0.0, 0.0, 1.0]])
    got = oc.scaled_intrinsics(torch.from_numpy(k))
    want = torch.eye(4)
    want[:3, :3] = torch.from_numpy(k).float()
    want[:2, :3] = want[:2, :3] * (640 / 512)
    assert got.dtype == torch.float32 and torch.equal(got, want) and np.array_equal(got.numpy(), ref.scaled_intrinsics(k))
    assert torch.equal(oc.scaled_intrinsics(k, 512, 320)[:2, :3], torch.from_numpy(k).float()[:2] * 0.625)
    with pytest.raises(ValueError, match=r"expected \[3, 3\]"):
        oc.scaled_intrinsics(np.eye(4))


@pytest.mark.parametrize("name", SCENES)
def test_scene_restatements_equal_the_reference(name):
    """Both restatements against the reference's dense statements, bit for bit.  ``scale`` goes through torch's fp32 pow, which is not
    correctly rounded and may differ by an ulp from one CPU build to another: it is held to 2 ulps here and pinned exactly against torch on the
    same device in the GPU tests."""
    fx = fixture(name)
    args = (fx["occ"], fx["point_cloud_range"].tolist(), fx["voxel_size"].tolist(), float(fx["base_scale"]), float(fx["exp_scale"]), int(fx["num_channels"]))
    want = {k: fx[k] for k in ref.FIELDS}
    assert want["feat"].ndim == 3 and want["feat"].shape[1] == 1                   # the reference carries a singleton axis
    want["feat"] = want["feat"].reshape(-1, int(fx["num_channels"]))
    want["is_labeled"] = bool(fx["is_labeled"])
    for fn in (ref.sparse_gaussians, ref.dense_gaussians):
        got = fn(*args)
        ref.same_gaussians(got, want, skip=("scale",))
        assert got["scale"].shape == want["scale"].shape and ulps(got["scale"], want["scale"]).max(initial=0) <= 2
        assert (got["scale"][:, 0] == got["scale"][:, 1]).all() and (got["scale"][:, 0] == got["scale"][:, 2]).all()


def test_fixtures_cover_what_they_claim():
    full, dup, one = fixture("scene_full"), fixture("scene_duplicates"), fixture("scene_single_class")
    assert len(full["xyz"]) == 8 * 6 * 5 and full["unique_classes"].tolist() == [1, 2, 3, 4] and full["feat"][:, 0, :4].sum() == 240
    assert len(dup["occ"]) == 65 and len(dup["xyz"]) == 40 and dup["occ"][:, 3].min() == -1 and dup["occ"][:, 3].max() == 200
    assert dup["unique_classes"].max() <= 59
    assert one["unique_classes"].tolist() == [0] and not bool(one["is_labeled"])
    assert fixture("scene_small")["occ"].dtype == np.float64
    g40 = fixture("scene_grid40")
    assert len(g40["unique_classes"]) == 12 and len(g40["xyz"]) < len(g40["occ"])


def _random_occ(seed, shape, m, labels, dtype=np.int64):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, s, (m, 1)) for s in shape] + [rng.integers(labels[0], labels[1], (m, 1))], 1).astype(dtype)


def test_sparse_restatement_equals_the_dense_one_on_small_grids():
    shape = ref.grid_shape(*SMALL)
    assert shape == (8, 6, 5)
    for seed, m, labels in ((1, 1, (3, 4)), (2, 50, (0, 11)), (3, 400, (-3, 9)), (4, 30, (55, 70))):
        occ = _random_occ(seed, shape, m, labels)
        ref.same_gaussians(ref.sparse_gaussians(occ, *SMALL), ref.dense_gaussians(occ, *SMALL))
    frac = _random_occ(5, shape, 60, (0, 5)).astype(np.float64) + 0.75          # fractional parts are cut toward zero
    frac[:, 3] -= 1.5                                                           # labels -0.75 .. 3.25: -0.75 becomes 0
    ref.same_gaussians(ref.sparse_gaussians(frac, *SMALL), ref.dense_gaussians(frac, *SMALL))
    ref.same_gaussians(ref.sparse_gaussians(frac, *SMALL), ref.sparse_gaussians(np.trunc(frac), *SMALL))
    empty = np.zeros((0, 4))
    got = ref.sparse_gaussians(empty, *SMALL)
    ref.same_gaussians(got, ref.dense_gaussians(empty, *SMALL))
    assert got["unique_classes"].tolist() == [0] and not got["is_labeled"] and got["xyz"].shape == (0, 3)
    occ = _random_occ(6, ref.grid_shape(ref.REAL_RANGE, [0.01] * 3), 5000, (0, 12))
    ref.same_gaussians(ref.sparse_gaussians(occ, ref.REAL_RANGE, [0.01] * 3), ref.dense_gaussians(occ, ref.REAL_RANGE, [0.01] * 3))


def test_restatements_refuse_what_the_contract_refuses():
    occ = np.array([[0, 0, 0, c] for c in range(1, 13)] + [[1, 1, 1, 13]])     # 13 labels + the empty cells' 0
    occ[:, 2] = np.arange(13) % 5
    occ[:, 1] = np.arange(13) // 5
    with pytest.raises(ValueError, match="classes do not fit"):
        ref.sparse_gaussians(occ, *SMALL)
    with pytest.raises(RuntimeError):                                         # one_hot, as in the reference
        ref.dense_gaussians(occ, *SMALL)
    for bad in ([8, 0, 0, 1], [0, 6, 0, 1], [0, 0, 5, 1], [-1, 0, 0, 1]):
        with pytest.raises(ValueError, match="outside the 8 x 6 x 5 grid"):
            ref.sparse_gaussians(np.array([bad]), *SMALL)


# ---- Python surface ----
SUPPORTED = "supported: a CUDA float32 tensor points [N,C] with C >= 3"


def test_refusals_name_the_supported_set():
    img, eye, k = np.zeros((12, 16), np.uint8), np.eye(4), np.eye(3)
    with pytest.raises(NotImplementedError, match="not a CUDA tensor") as e:
        oc.project_labels(torch.zeros(4, 3), img, eye, k)
    assert SUPPORTED in str(e.value) and "there is no CPU path" in str(e.value)
    with pytest.raises(NotImplementedError, match="torch.float64, not float32") as e:
        oc.project_labels(torch.zeros(4, 3, dtype=torch.float64), img, eye, k)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="C < 3"):
        oc.project_labels(torch.zeros(4, 2), img, eye, k)
    with pytest.raises(NotImplementedError, match="no backward"):
        oc.project_labels(torch.zeros(4, 3, requires_grad=True), img, eye, k)
    with pytest.raises(NotImplementedError, match="is a list, not a tensor"):
        oc.project_labels([[0.0, 0.0, 0.0]], img, eye, k)
    with pytest.raises(NotImplementedError, match="not a CUDA tensor"):
        oc.occupancy_from_points(torch.zeros(4, 3), img, eye, k)
    with pytest.raises(NotImplementedError, match="float32, not uint8 or an integer type") as e:
        oc._label_image(np.zeros((12, 16), np.float32), "cpu")
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="torch.float16, not uint8 or an integer type"):
        oc._label_image(torch.zeros(12, 16, dtype=torch.float16), "cpu")
    with pytest.raises(ValueError, match=r"expected \[H, W\]"):
        oc._label_image(np.zeros((3, 12, 16), np.uint8), "cpu")
    assert oc._label_image(img, "cpu").dtype == torch.uint8 and oc._label_image(img.astype(np.int64), "cpu").dtype == torch.int32
    with pytest.raises(ValueError, match=r"`extrin` has shape \(3, 3\)"):
        oc.projection_matrix(k, k, "cpu")
    with pytest.raises(ValueError, match=r"`intrin` has shape \(2, 2\)"):
        oc.projection_matrix(eye, np.eye(2), "cpu")
    P = oc.projection_matrix(eye, k, "cpu")
    assert P.dtype == torch.float32 and torch.equal(P, torch.eye(4))
    with pytest.raises(NotImplementedError, match="not a CUDA device") as e:
        oc.OccupancyScene(device="cpu")
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="num_channels = 0"):
        oc.OccupancyScene(num_channels=0)
    with pytest.raises(NotImplementedError, match="num_channels = 65"):
        oc.OccupancyScene(num_channels=65)
    with pytest.raises(ValueError, match="needs 6 values"):
        oc.OccupancyScene(point_cloud_range=[0, 0, 0, 1, 1])
    with pytest.raises(ValueError, match="1 to 65535 cells on every axis"):
        oc.OccupancyScene(point_cloud_range=[0, 0, 0, 1, 1, 0])
    with pytest.raises(ValueError, match="1 to 65535 cells on every axis"):
        oc.OccupancyScene(point_cloud_range=[0, 0, 0, 100, 1, 1])
    with pytest.raises(ValueError, match="at least 2 cells along z"):
        oc.OccupancyScene(point_cloud_range=[0, 0, 0, 1, 1, 0.1], voxel_size=[0.1, 0.1, 0.1])
    wide = np.zeros((12, 16), np.uint32)
    assert oc._label_image(wide, "cpu").dtype == torch.int32 and oc._label_image(wide.astype(np.uint16), "cpu").dtype == torch.int32
    wide[3, 4] = 2 ** 31
    for bad in (wide, wide.astype(np.int64), torch.from_numpy(wide.astype(np.int64)), -wide.astype(np.int64) - 1):
        with pytest.raises(NotImplementedError, match="outside the int32 range"):
            oc._label_image(bad, "cpu")


def test_signatures_and_defaults():
    import orv_amd
    d = {k: p.default for k, p in inspect.signature(oc.occupancy_from_points).parameters.items()}
    assert list(d) == ["points", "labels2d", "extrin", "intrin", "voxel_size", "point_cloud_range"]
    assert d["voxel_size"] == [0.001] * 3 and d["point_cloud_range"] == [-0.2, -0.2, 0, 0.2, 0.2, 0.4]
    d = {k: p.default for k, p in inspect.signature(oc.OccupancyScene.__init__).parameters.items()}
    assert (d["base_scale"], d["exp_scale"], d["num_channels"]) == (0.00023, 3.7, 12)
    assert list(inspect.signature(oc.project_labels).parameters) == ["points", "labels2d", "extrin", "intrin"]
    assert list(inspect.signature(oc.scaled_intrinsics).parameters) == ["intrin3", "src_w", "tgt_w"]
    assert list(inspect.signature(oc.OccupancyScene.render).parameters) == ["self", "occ", "extrins", "intrin", "image_shape"]
    assert list(inspect.signature(oc.OccupancyScene.render_trajectory).parameters) == ["self", "frames", "extrins", "intrin"]
    assert "occupancy" not in inspect.getsource(orv_amd.install)                   # the package-level install() is unchanged


# ---- C ABI ----
NAMES = ("orv_occ_project_labels", "orv_occ_cell_keys", "orv_occ_mark_cells", "orv_occ_write_gaussians")


def test_occ_symbols_are_declared_exported_bound_and_cited():
    from orv_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(_lib.lib(), name) is not None
        assert callable(getattr(ops, name[4:]))
    for name, cites in (("orv_occ_project_labels", ("prepare_dataset.py:878-884", ":999-1008")), ("orv_occ_cell_keys", ("prepare_dataset.py:2153-2154",)),
                        ("orv_occ_mark_cells", ("prepare_dataset.py:2155-2157",)), ("orv_occ_write_gaussians", ("prepare_dataset.py:2158", ":2077-2086"))):
        end = hdr.index("int " + name + "(")
        doc = hdr[hdr.rindex("/*", 0, end):end]
        assert all(c in doc for c in cites), name                                # each cites the reference lines it replaces
    assert "section 14" in hdr[hdr.index("Occupancy labelling"):hdr.index("int orv_occ_project_labels(")]
    with open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile"), "r", encoding="utf-8") as f:
        assert "occupancy.hip" in f.read()


def test_occ_entry_points_validate_before_any_launch():
    """Null pointers, negative sizes, C < 3, a bad label width, grid or class bitmap: nonzero with the reason in orv_last_error(), prefixed by
    the entry point's name, without a GPU (no pointer is followed)."""
    from orv_amd._lib import lib
    h = lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lambda: h.orv_last_error().decode()

    def proj(points=p, N=4, C=3, P=p, img=p, nbytes=1, H=12, W=16, out=p):
        return h.orv_occ_project_labels(points, N, C, P, img, nbytes, H, W, out, None)

    def keys(occ=p, M=4, grid=(8, 6, 5), out=p, state=p):
        return h.orv_occ_cell_keys(occ, M, *grid, out, state, None)

    def mark(k=p, order=p, occ=p, M=4, last=p, state=p):
        return h.orv_occ_mark_cells(k, order, occ, M, last, state, None)

    def write(order=p, occ=p, last=p, csum=p, M=4, n=2, grid=(8, 6, 5), ax=p, zs=p, classes=3, F=12, xyz=p, rot=p, opacity=p):
        return h.orv_occ_write_gaussians(order, occ, last, csum, M, n, *grid, ax, p, p, zs, classes, F, xyz, p, p, rot, p, opacity, None)

    assert proj(N=-1) != 0 and "N must not be negative" in err() and err().startswith(NAMES[0] + ":")
    for call, name in ((keys, NAMES[1]), (mark, NAMES[2]), (write, NAMES[3])):
        assert call(M=-1) != 0 and "M must not be negative" in err() and err().startswith(name + ":"), name
    assert proj(C=2) != 0 and "C = 2" in err() and "C >= 3" in err()
    assert proj(nbytes=2) != 0 and "label_bytes = 2" in err() and "1 (uint8) or 4 (int32)" in err()
    for bad in (dict(H=0), dict(W=0), dict(H=65536, W=65536)):
        assert proj(**bad) != 0 and "label image" in err() and err().startswith(NAMES[0] + ":"), bad
    for bad in (dict(points=None), dict(P=None), dict(img=None), dict(out=None)):
        assert proj(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[0] + ":"), bad
    assert proj(img=p + 2, nbytes=4) != 0 and "aligned" in err()
    for call, name in ((keys, NAMES[1]), (write, NAMES[3])):
        for bad in ((0, 6, 5), (8, -1, 5), (8, 6, 65536)):
            assert call(grid=bad) != 0 and "1 to 65535 cells on every axis" in err() and err().startswith(name + ":"), (name, bad)
    for bad in (dict(occ=None), dict(out=None), dict(state=None)):
        assert keys(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[1] + ":"), bad
    assert keys(occ=p + 4) != 0 and "16-byte" in err()
    for bad in (dict(k=None), dict(order=None), dict(occ=None), dict(last=None), dict(state=None)):
        assert mark(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[2] + ":"), bad
    for bad in (dict(order=None), dict(occ=None), dict(last=None), dict(csum=None), dict(ax=None), dict(zs=None), dict(xyz=None),
                dict(rot=None), dict(opacity=None)):
        assert write(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[3] + ":"), bad
    assert write(n=-1) != 0 and "n = -1" in err()
    assert write(n=5) != 0 and "n = 5" in err()
    assert write(F=0) != 0 and "F = 0" in err()
    assert write(F=65) != 0 and "F = 65" in err()
    assert write(classes=(1 << 13) - 1) != 0 and "holds 13 classes" in err() and "F = 12" in err()
    assert write(classes=1 << 60) != 0 and "labels 0 to 59 only" in err()
    # nothing to do is not an error, and launches nothing
    assert proj(N=0, points=None, P=None, img=None, out=None) == 0
    assert keys(M=0, occ=None, out=None, state=None) == 0 and mark(M=0, k=None) == 0
    assert write(M=0, n=0, order=None, xyz=None) == 0 and write(n=0, xyz=None) == 0
