"""Gaussian rasterizer, host side (no GPU): hand-derived known answers through the CPU oracle (tests/gs_render_ref.py), the cap on the share of
fragile pixels in every scene the GPU tests use, the Python surface of ``orv_amd.gs_render`` (refusals, the two import aliases, the helpers)
and the C ABI of the four ``orv_gs_*`` entry points (argument validation happens before any launch)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import gs_render_ref as ref
import gs_render_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(means, opac, scales, colors=None, feats=None, W=48, H=32, f=40.0, dtype=np.float32, bg=(0.0, 0.0, 0.0)):
    """Isotropic, unrotated Gaussians seen by an identity camera with the principal point on pixel ((W-1)/2 + 0.5, (H-1)/2 + 0.5)."""
    means = np.asarray(means, np.float64).reshape(-1, 3)
    N = means.shape[0]
    tfx, tfy, view, proj = scenes.camera(W, H, f, f, W / 2, H / 2)
    rots = np.zeros((N, 4))
    rots[:, 0] = 1
    colors = np.zeros((N, 3)) if colors is None else colors
    return ref.rasterize(means, np.asarray(opac, np.float64), np.repeat(np.asarray(scales, np.float64).reshape(-1, 1), 3, 1), rots, colors, feats,
                         H, W, tfx, tfy, bg, 1.0, view, proj, dtype=dtype)


# ---- known answers ----
@pytest.mark.parametrize("dtype,tol", [(np.float32, 2e-5), (np.float64, 1e-9)])
def test_one_isotropic_gaussian_on_the_axis_has_the_closed_form(dtype, tol):
    """alpha(x, y) = min(.99, o exp(-d^2 / (2 (sigma^2 + 0.3)))) with sigma = f s / z where that is >= 1/255, depth = z alpha; the centre of
    a point on the optical axis is pixel (W/2 - 0.5, H/2 - 0.5)."""
    W, H, f, s, z, o = 48, 32, 40.0, 0.1, 1.6, 0.7
    out = _one([[0, 0, z]], [o], [s], colors=np.array([[0.2, 0.5, 0.9]]), W=W, H=H, f=f, dtype=dtype, bg=(0.3, 0.1, 0.0))
    sigma = f * s / z
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    d2 = (x - (W / 2 - 0.5)) ** 2 + (y - (H / 2 - 0.5)) ** 2
    a = np.minimum(0.99, o * np.exp(-0.5 * d2 / (sigma ** 2 + 0.3)))
    radius = math.ceil(3 * math.sqrt(sigma ** 2 + 0.3 + math.sqrt(0.1)))            # mid = a = c, det = mid^2: lambda = mid + sqrt(0.1)
    assert out["radii"].tolist() == [radius]
    a = np.where(a >= 1 / 255, a, 0.0)                                              # the whole image is inside the one tile rectangle here
    assert np.abs(out["alpha"][0] - a).max() <= tol
    assert np.abs(out["depth"][0] - z * a).max() <= tol * z
    for c, (col, b) in enumerate(zip((0.2, 0.5, 0.9), (0.3, 0.1, 0.0))):
        assert np.abs(out["color"][c] - (col * a + (1 - a) * b)).max() <= tol
    assert out["count"].max() == 1 and out["count"][H // 2, W // 2] == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_gaussians_blend_front_to_back_in_either_input_order(dtype):
    mean = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0]])             # both on the axis: the projected covariance is sigma^2 I exactly
    op, sc, col = np.array([0.8, 0.6]), np.array([0.2, 0.5]), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    feats = np.array([[1.0, 0.0], [0.0, 1.0]])
    a = _one(mean, op, sc, col, feats, dtype=dtype)
    b = _one(mean[::-1], op[::-1], sc[::-1], col[::-1], feats[::-1], dtype=dtype)
    for k in ("color", "feat", "depth", "alpha"):
        assert np.array_equal(a[k], b[k]), k
    # by hand at one pixel: near first, the far one seen through 1 - alpha_near
    x, y, f = 20, 14, 40.0
    al = []
    for (mx, my, mz), o, s in zip(mean, op, sc):
        cx, cy = f * mx / mz + 24 - 0.5, f * my / mz + 16 - 0.5
        al.append(min(0.99, o * math.exp(-0.5 * ((cx - x) ** 2 + (cy - y) ** 2) / ((f * s / mz) ** 2 + 0.3))))
    tol = 2e-5 if dtype == np.float32 else 1e-9
    assert abs(a["alpha"][0, y, x] - (1 - (1 - al[0]) * (1 - al[1]))) <= tol
    assert abs(a["color"][0, y, x] - al[0]) <= tol and abs(a["color"][1, y, x] - (1 - al[0]) * al[1]) <= tol
    assert abs(a["feat"][1, y, x] - (1 - al[0]) * al[1]) <= tol
    assert abs(a["depth"][0, y, x] - (al[0] * 1.0 + (1 - al[0]) * al[1] * 2.0)) <= 2 * tol


def test_three_opaque_coincident_gaussians_pin_the_fp32_stop():
    """At a pixel on the common centre each alpha is capped at 0.99.  In fp32 (1 - 0.99f)^2 < 1e-4, so the SECOND Gaussian already stops the
    pixel and is not added: alpha = 0.99f exactly, one contributor.  In fp64 0.01^2 rounds above 1e-4: the second is added, the third stops.
    The kernel therefore has to form T (1 - alpha) in fp32."""
    assert np.float32(1) - np.float32(0.99) < np.float32(0.01) and (np.float32(1) - np.float32(0.99)) ** 2 < np.float32(1e-4)
    assert (1.0 - 0.99) * (1.0 - 0.99) > 1e-4
    W, H = 33, 17                                                       # odd: pixel (16, 8) is the centre of a point on the axis
    mean = np.array([[0, 0, 1.0]] * 3)
    o32 = _one(mean, [1, 1, 1], [0.3] * 3, W=W, H=H, dtype=np.float32)
    o64 = _one(mean, [1, 1, 1], [0.3] * 3, W=W, H=H, dtype=np.float64)
    assert o32["count"][8, 16] == 1 and o32["alpha"][0, 8, 16] == np.float32(1) - (np.float32(1) - np.float32(0.99))
    assert o32["depth"][0, 8, 16] == np.float32(0.99)
    assert o64["count"][8, 16] == 2 and abs(o64["alpha"][0, 8, 16] - (1 - 0.01 ** 2)) < 1e-12
    assert o32["fragile"][8, 16] and o64["fragile"][8, 16]            # and the oracle knows this pixel sits on the threshold


def test_depth_ties_go_by_index_and_are_not_fragile():
    mean = np.array([[0.0, 0, 1.0], [0.01, 0, 1.0]])
    col = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    out = _one(mean, [0.5, 0.5], [0.2, 0.2], col)
    y, x = 16, 24
    assert out["color"][0, y, x] > out["color"][1, y, x] > 0           # index 0 is blended first
    assert not out["fragile_by"]["near_tie"].any()
    near = _one(np.array([[0.0, 0, 1.0], [0.01, 0, 1.0 + 2e-7]]), [0.5, 0.5], [0.2, 0.2], col, dtype=np.float64)
    assert near["fragile_by"]["near_tie"].any()


def test_projection_helpers_against_hand_computed_matrices():
    from orv_amd import gs_render as g
    assert g.focal2fov(50.0, 100) == pytest.approx(math.pi / 2) and g.focal2fov(1.0, 2 * math.sqrt(3)) == pytest.approx(2 * math.pi / 3)
    P = g.get_projection_matrix(0.1, 200.0, math.pi / 2, 2 * math.atan(0.5))
    want = torch.zeros(4, 4)
    want[0, 0], want[1, 1], want[2, 2], want[2, 3], want[3, 2] = 1.0, 2.0, 200.0 / 199.9, -20.0 / 199.9, 1.0
    assert P.dtype == torch.float32 and torch.allclose(P, want, rtol=1e-6, atol=1e-7)
    # fx = 100, cx = 30 of W = 80: right = 30 n / fx, left = -50 n / fx -> P00 = 2 fx / W, P02 = (30 - 50) / 80
    Pc = g.get_projection_matrix_c(100.0, 50.0, 30.0, 10.0, 80, 40, 0.5, 10.0)
    want = torch.zeros(4, 4)
    want[0, 0], want[1, 1], want[0, 2], want[1, 2] = 2.5, 2.5, -0.25, -0.5
    want[2, 2], want[2, 3], want[3, 2] = 10.0 / 9.5, -5.0 / 9.5, 1.0
    assert torch.allclose(Pc, want, rtol=1e-6, atol=1e-7)
    # centred principal point: the two constructions agree
    assert torch.allclose(g.get_projection_matrix_c(60.0, 40.0, 32.0, 24.0, 64, 48, 0.1, 200.0),
                          g.get_projection_matrix(0.1, 200.0, g.focal2fov(60.0, 64), g.focal2fov(40.0, 48)), rtol=1e-6, atol=1e-7)
    grid = g.create_full_center_coords(range=np.array([[0.0, -1.0, 2.0], [1.0, 1.0, 2.5]]), dim=np.array([0.5, 0.5, 0.25]))
    assert grid.shape == (2, 4, 2, 3)
    assert grid[1, 0, 0].tolist() == [1.0, -1.0, 2.0] and grid[0, 3, 1].tolist() == [0.0, 1.0, 2.5]
    assert torch.allclose(grid[0, 1, 0], torch.tensor([0.0, -1.0 / 3.0, 2.0]))
    # the scene helper of the tests builds the same camera
    tfx, tfy, view, proj = scenes.camera(64, 48, 60.0, 40.0, 32.0, 24.0)
    assert tfx == pytest.approx(math.tan(0.5 * g.focal2fov(60.0, 64))) and np.array_equal(view, np.eye(4, dtype=np.float32))
    assert np.allclose(proj, g.get_projection_matrix_c(60.0, 40.0, 32.0, 24.0, 64, 48, 0.1, 200.0).T.numpy(), rtol=1e-6, atol=1e-7)


def test_semantic_colormap_and_labels_and_depth():
    from orv_amd import gs_render as g
    sem = torch.zeros(12, 2, 3)
    sem[3, 0, 0], sem[11, 1, 2] = 1.0, 2.0
    rgb = g.apply_semantic_colormap(sem)
    assert rgb.shape == (3, 2, 3) and torch.allclose(rgb[:, 0, 0], torch.tensor([0.0, 150.0, 245.0]) / 255)
    assert torch.allclose(rgb[:, 1, 2], torch.tensor([139.0, 137.0, 137.0]) / 255) and torch.allclose(rgb[:, 0, 1], torch.tensor([255.0, 120.0, 50.0]) / 255)
    assert torch.equal(g.apply_semantic_colormap(torch.tensor([[[3, 15]]])), torch.stack([rgb[:, 0, 0], torch.zeros(3)], 1)[:, None])
    feat = torch.zeros(12, 1, 4)
    feat[2, 0, 0], feat[11, 0, 1], feat[5, 0, 2], feat[1, 0, 3] = 0.9, 0.8, 0.05, 0.6
    pkg = {"render_feat": feat, "render_depth": torch.tensor([[[0.2, 0.7, 0.3, 0.001]]]), "render_alpha": torch.tensor([[[0.9, 0.8, 0.05, 0.6]]])}
    classes = torch.tensor([0, 4, 9])                                   # three classes present: argmax 11 clamps to the last
    labels, depth = g.labels_and_depth(pkg, classes)
    assert labels.tolist() == [[9, 9, 0, 4]]
    assert torch.allclose(depth, torch.tensor([[[0.2, 0.4, 0.4, 0.01]]])) and pkg["render_depth"][0, 0, 2] == 0.3


# ---- the fragile-share cap ----
@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_fragile_share_of_every_gpu_scene_is_capped(name):
    frag = scenes.fragile(name)
    o32, o64 = scenes.oracle(name, 32), scenes.oracle(name, 64)
    by = {k: round(float((o32["fragile_by"][k] | o64["fragile_by"][k]).mean()), 4) for k in o32["fragile_by"]}
    print(f"{name}: fragile share {frag.mean():.4f} {by}")
    assert frag.mean() <= 0.05
    ok = ~frag
    assert np.array_equal(o32["count"][ok], o64["count"][ok])          # off the fragile pixels both precisions take the same decisions
    for plane in ("color", "feat", "depth", "alpha"):
        top = np.abs(o64[plane]).max(initial=0.0)
        if top:
            e = np.abs(o32[plane] - o64[plane])[:, ok].max() / top
            print(f"  {plane}: E_ref {e:.2e}")
            assert e <= 2e-5


def test_scene_recipes_hold():
    s = scenes.scene("e_faint_ladder")
    z = np.sort(s["means"][:, 2].astype(np.float64))
    assert (np.diff(z) / z[1:]).min() > 1e-4
    for name in ("e_faint_stop", "e_faint_ladder"):
        o, n = scenes.oracle(name, 32), scenes.scene(name)["means"].shape[0]
        assert (o["pre"]["rect"] == [0, 0, 3, 2]).all()                # every Gaussian is in every tile's list
    c = scenes.oracle("e_faint_stop", 32)["count"]
    assert c.min() > 256 and c.max() < 330                             # two staged batches, the stop in the second
    assert scenes.oracle("e_faint_ladder", 32)["count"].min() == 700   # three batches, no stop
    f = scenes.scene("f_occupancy")
    assert len(np.unique(f["means"][:, 2])) == 6 and (f["opacities"] == 1).all() and not f["colors"].any()
    a = scenes.scene("a_generic_400")
    assert (a["opacities"][::7] == 1).all() and 0 < (~scenes.oracle("a_generic_400", 32)["pre"]["front"]).mean() < 0.12
    assert scenes.oracle("d_70_tiles", 32)["alpha"].shape == (1, 112, 160)


# ---- Python surface ----
def _cpu_call(**over):
    from orv_amd.gs_render import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3), False, False, True)
    kw = dict(means3D=torch.zeros(2, 3), means2D=None, opacities=torch.ones(2, 1), colors_precomp=torch.zeros(2, 3),
              language_feature_precomp=torch.zeros(2, 12), scales=torch.ones(2, 3), rotations=torch.ones(2, 4))
    kw.update(over)
    return GaussianRasterizer(s)(**kw)


def test_settings_have_the_reference_fields():
    from orv_amd.gs_render import GaussianRasterizationSettings
    assert GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                                                     "projmatrix", "sh_degree", "campos", "prefiltered", "debug", "include_feature")


def test_exactly_one_of_checks():
    with pytest.raises(Exception, match="exactly one of either SHs or precomputed colors"):
        _cpu_call(colors_precomp=None)
    with pytest.raises(Exception, match="exactly one of either SHs or precomputed colors"):
        _cpu_call(shs=torch.zeros(2, 16, 3))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        _cpu_call(scales=None)
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        _cpu_call(cov3D_precomp=torch.zeros(2, 6))


def test_refusals_name_the_supported_set():
    supported = "supported: CUDA float32 tensors"
    with pytest.raises(NotImplementedError, match="spherical harmonics") as e:
        _cpu_call(shs=torch.zeros(2, 16, 3), colors_precomp=None)
    assert supported in str(e.value)
    with pytest.raises(NotImplementedError, match="cov3D_precomp") as e:
        _cpu_call(cov3D_precomp=torch.zeros(2, 6), scales=None, rotations=None)
    assert supported in str(e.value)
    with pytest.raises(NotImplementedError, match="not a CUDA tensor") as e:
        _cpu_call()
    assert supported in str(e.value) and "means3D" in str(e.value)
    from orv_amd import gs_render as g
    with pytest.raises(NotImplementedError, match="float32") as e:
        _cpu_call(scales=torch.ones(2, 3, dtype=torch.float16))
    assert supported in str(e.value) and "scales" in str(e.value)
    with pytest.raises(NotImplementedError, match="F > 16") as e:
        _cpu_call(language_feature_precomp=torch.zeros(2, 17))
    assert supported in str(e.value)
    with pytest.raises(NotImplementedError, match="no backward") as e:
        _cpu_call(opacities=torch.ones(2, 1, requires_grad=True))
    assert supported in str(e.value) and "opacities" in str(e.value)
    assert g.MAX_FEATURES == 16


def test_shapes_are_checked_before_anything_is_launched():
    for bad in (dict(means3D=torch.zeros(2, 2)), dict(means3D=torch.zeros(6)), dict(colors_precomp=torch.zeros(3, 3)), dict(scales=torch.ones(2, 2)),
                dict(rotations=torch.ones(2, 3)), dict(opacities=torch.ones(3, 1)), dict(language_feature_precomp=torch.zeros(1, 12))):
        with pytest.raises(ValueError, match=r"means3D \[N,3\]"):
            _cpu_call(**bad)


def test_mark_visible_is_the_near_plane_test():
    from orv_amd.gs_render import GaussianRasterizationSettings, GaussianRasterizer
    view = torch.eye(4)
    view[3, 2] = 0.5                                                    # camera 0.5 behind the origin along z
    s = GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, view, view, 3, torch.zeros(3), False, False, True)
    pts = torch.tensor([[0, 0, 1.0], [0, 0, -0.49], [0, 0, -0.4899], [0, 0, -2.0], [5, 5, 0.0]])
    assert GaussianRasterizer(s).markVisible(pts).tolist() == [True, False, True, False, True]


def test_install_makes_the_reference_import_lines_work_and_uninstall_restores():
    from orv_amd import gs_render as g
    before = dict(sys.modules)
    assert "gs_render" not in sys.modules and "diff_gaussian_rasterization" not in sys.modules
    names = g.install()
    try:
        assert set(names) == {"diff_gaussian_rasterization", "gs_render"}
        from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer  # noqa: F401
        from gs_render import render, focal2fov, get_projection_matrix_c, create_full_center_coords, apply_semantic_colormap  # noqa: F401
        assert GaussianRasterizer is g.GaussianRasterizer and render is g.render
        assert g.install() == []                                        # the names are taken now: nothing more to register
    finally:
        g.uninstall()
    assert "gs_render" not in sys.modules and "diff_gaussian_rasterization" not in sys.modules
    assert {k for k in sys.modules if k not in before} <= {"orv_amd.gs_render", "orv_amd.ops"} | {k for k in sys.modules if k.startswith("orv_amd")}
    taken = type(sys)("gs_render")
    sys.modules["gs_render"] = taken                                    # a name that is not free is left alone
    try:
        assert g.install() == ["diff_gaussian_rasterization"] and sys.modules["gs_render"] is taken
    finally:
        g.uninstall()
        del sys.modules["gs_render"]
    assert "diff_gaussian_rasterization" not in sys.modules
    import orv_amd
    import inspect
    assert "gs_render" not in inspect.getsource(orv_amd.install)       # the package-level install() is unchanged


# ---- C ABI ----
NAMES = ("orv_gs_preprocess", "orv_gs_tile_keys", "orv_gs_tile_ranges", "orv_gs_render")


def test_gs_symbols_are_declared_exported_and_bound():
    from orv_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(_lib.lib(), name) is not None
        doc = hdr[hdr.index("Gaussian rasterizer"):hdr.index("int " + name + "(")]
        assert "gs_render.py:" in doc and "diff-gaussian-rasterization" in doc
        assert callable(getattr(ops, name[4:]))
    with open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile"), "r", encoding="utf-8") as f:
        assert "gs_render.hip" in f.read()


def test_gs_entry_points_validate_before_any_launch():
    """Null pointers, H or W <= 0, N < 0, F > 16: nonzero with the reason in orv_last_error(), without a GPU (no pointer is followed)."""
    from orv_amd._lib import lib
    h = lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lambda: h.orv_last_error().decode()

    def pre(means=p, view=p, out=p, N=4, H=32, W=32):
        return h.orv_gs_preprocess(means, p, p, p, view, p, N, H, W, 0.5, 0.5, 1.0, out, p, p, p, p, p, None)

    def keys(rect=p, keys_=p, N=4, H=32, W=32, L=8):
        return h.orv_gs_tile_keys(rect, p, p, N, H, W, L, keys_, p, None)

    def rng(k=p, L=8, H=32, W=32, out=p):
        return h.orv_gs_tile_ranges(k, L, H, W, out, None)

    def ren(ranges=p, lst=p, L=8, xy=p, feats=p, N=4, F=12, bg=p, H=32, W=32, out=p, out_f=p):
        return h.orv_gs_render(ranges, lst, L, xy, p, p, p, feats, N, F, bg, H, W, out, out_f, p, p, None)

    for call, name in ((pre, NAMES[0]), (keys, NAMES[1]), (rng, NAMES[2]), (ren, NAMES[3])):
        for bad in (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
            assert call(**bad) != 0 and "height and width must be positive" in err() and err().startswith(name), (name, bad)
    for call, name in ((pre, NAMES[0]), (keys, NAMES[1]), (ren, NAMES[3])):
        assert call(N=-1) != 0 and "N must not be negative" in err() and err().startswith(name)
    assert pre(means=None) != 0 and "null pointer" in err()
    assert pre(view=None) != 0 and "null pointer" in err()
    assert pre(out=None) != 0 and "null pointer" in err()
    assert keys(rect=None) != 0 and "null pointer" in err()
    assert keys(keys_=None) != 0 and "null pointer" in err()
    assert rng(k=None) != 0 and "null pointer" in err()
    assert rng(out=None) != 0 and "null pointer" in err()
    for bad in (dict(ranges=None), dict(lst=None), dict(xy=None), dict(feats=None), dict(bg=None), dict(out=None), dict(out_f=None)):
        assert ren(**bad) != 0 and "null pointer" in err(), bad
    assert ren(F=17) != 0 and "F = 17" in err() and "0 to 16" in err()
    assert ren(F=-1) != 0 and "0 to 16" in err()
    for call in (keys, rng, ren):
        assert call(L=2 ** 31) != 0 and "2^31" in err()
        assert call(L=-1) != 0 and "2^31" in err()
    # nothing to do is not an error, and launches nothing
    assert pre(N=0, means=None, out=None) == 0 and keys(N=0, rect=None) == 0 and keys(L=0, keys_=None) == 0 and rng(L=0, k=None) == 0
