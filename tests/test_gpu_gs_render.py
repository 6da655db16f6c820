"""GPU: the Gaussian rasterizer (``orv_amd.gs_render`` over csrc/gs_render.hip) against the CPU oracle of tests/gs_render_ref.py.

The kernel is held to the fp64 oracle on every pixel that is not fragile, per plane, within 8 x E_ref x max|plane|, where E_ref is the fp32
oracle's own error against the fp64 oracle on that scene and plane: the kernel's fp32 arithmetic may round like the fp32 restatement does
(another exponential, fused multiply-adds in the sums, up to 700 accumulated terms), and no worse than a small multiple of it.  Fragile pixels
(a decision of a live entry within 1e-4 of its threshold) only have to be finite with alpha in [0, 1].

Kernel / E_ref ratios measured on an MI355X are recorded in DESIGN.md §12.
"""
import functools

import numpy as np
import pytest
import torch

import gs_render_ref as ref
import gs_render_scenes as scenes

pytestmark = pytest.mark.gpu
PLANES = ("color", "feat", "depth", "alpha")


def _settings(s, dev):
    from orv_amd.gs_render import GaussianRasterizationSettings
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    view = t(s["view"])
    return GaussianRasterizationSettings(image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
                                         scale_modifier=1.0, viewmatrix=view, projmatrix=t(s["proj"]), sh_degree=3, campos=view.inverse()[3, :3],
                                         prefiltered=False, debug=False, include_feature=s["include_feature"])


def _rasterize(name):
    from orv_amd.gs_render import GaussianRasterizer
    s, dev = scenes.scene(name), torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = GaussianRasterizer(_settings(s, dev))(means3D=t(s["means"]), means2D=None, opacities=t(s["opacities"]), colors_precomp=t(s["colors"]),
                                                language_feature_precomp=t(s["feats"]), scales=t(s["scales"]), rotations=t(s["rots"]))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _kernel(name):
    color, feat, radii, depth, alpha = _rasterize(name)
    return dict(color=color.cpu().numpy(), feat=feat.cpu().numpy(), radii=radii.cpu().numpy(), depth=depth.cpu().numpy(), alpha=alpha.cpu().numpy())


def _bound(name, plane):
    """8 x E_ref x max|oracle64 plane| = 8 x the fp32 oracle's largest error on the non-fragile pixels."""
    o32, o64, ok = scenes.oracle(name, 32)[plane], scenes.oracle(name, 64)[plane], ~scenes.fragile(name)
    return 8.0 * float(np.abs(o32.astype(np.float64) - o64)[:, ok].max(initial=0.0))


@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_planes_match_the_fp64_oracle_off_the_fragile_pixels(name):
    s, got, o64 = scenes.scene(name), _kernel(name), scenes.oracle(name, 64)
    H, W = s["H"], s["W"]
    F = s["feats"].shape[1] if s["include_feature"] else 0
    assert got["color"].shape == (3, H, W) and got["feat"].shape == (F, H, W) and got["depth"].shape == (1, H, W) and got["alpha"].shape == (1, H, W)
    frag = scenes.fragile(name)
    ok = ~frag
    for plane in PLANES:
        k = got[plane]
        assert np.isfinite(k).all(), plane
        if k.size == 0:
            continue
        bound = _bound(name, plane)
        err = float(np.abs(k.astype(np.float64) - o64[plane])[:, ok].max(initial=0.0))
        print(f"{name} {plane}: kernel err {err:.3e}, E_ref x max {bound / 8:.3e}, ratio {err / (bound / 8) if bound else 0.0:.2f}, fragile {frag.mean():.4f}")
        assert err <= bound, (name, plane, err, bound)
    assert (got["alpha"] >= 0).all() and (got["alpha"] <= 1).all()


@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_radii_and_visible_set_equal_the_oracle(name):
    got, pre = _kernel(name)["radii"], scenes.oracle(name, 32)["pre"]
    want = scenes.oracle(name, 32)["radii"]
    assert got.dtype == np.int32 and got.shape == want.shape
    lam3, z = pre["lam3"].astype(np.float64), pre["z"].astype(np.float64)
    z_ok = np.abs(z - ref.NEAR) > 1e-6 * ref.NEAR
    r_ok = np.abs(lam3 - np.round(lam3)) > ref.DELTA
    assert np.array_equal((got > 0)[z_ok & r_ok], (want > 0)[z_ok & r_ok])
    assert np.array_equal(got[z_ok & r_ok], want[z_ok & r_ok])


def test_nothing_visible_gives_background_zeros_and_alpha_zero():
    for name in ("g_behind", "g_empty"):
        s, got = scenes.scene(name), _kernel(name)
        assert np.array_equal(got["color"], np.broadcast_to(s["bg"][:, None, None], got["color"].shape))
        assert not got["feat"].any() and not got["depth"].any() and not got["alpha"].any() and not got["radii"].any()
        assert got["radii"].shape == (s["means"].shape[0],)


def test_occupancy_labels_and_depth_match_the_oracle():
    from orv_amd.gs_render import labels_and_depth
    name = "f_occupancy"
    _, classes = scenes.occupancy(17)
    color, feat, radii, depth, alpha = _rasterize(name)
    pkg = {"render_color": color, "radii": radii, "render_depth": depth, "render_alpha": alpha, "render_feat": feat}
    keep = {k: v.clone() for k, v in pkg.items()}
    labels, dep = labels_and_depth(pkg, torch.from_numpy(classes).to(color.device))
    assert all(torch.equal(pkg[k], keep[k]) for k in pkg)                       # the render result is left unchanged
    o = scenes.oracle(name, 64)
    none = o["alpha"][0] < 0.10
    f = o["feat"].copy()
    f[:, none] = np.eye(12)[0][:, None]
    want = classes[np.clip(f.argmax(0), 0, len(classes) - 1)]
    top = np.sort(f, axis=0)
    clear = (top[-1] - top[-2] > _bound(name, "feat")) & (np.abs(o["alpha"][0] - 0.10) > _bound(name, "alpha")) & ~scenes.fragile(name)
    assert clear.mean() > 0.8 and len(np.unique(want[clear])) > 3
    assert labels.shape == (48, 64) and np.array_equal(labels.cpu().numpy()[clear], want[clear])
    d = np.clip(np.where(none, 51.2, o["depth"][0]), 0.01, 0.4)
    assert dep.shape == (1, 48, 64) and np.abs(dep[0].cpu().numpy() - d)[clear].max() <= _bound(name, "depth") + 1e-7


def test_two_calls_are_bit_identical():
    a, b = _rasterize("b_generic_1500"), _rasterize("b_generic_1500")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, b = _rasterize("e_faint_stop"), _rasterize("e_faint_stop")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_render_returns_the_reference_dict():
    from orv_amd.gs_render import render
    s, dev = scenes.scene("f_occupancy"), torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    intr = torch.tensor([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1]], device=dev)
    pkg = render(torch.eye(4, device=dev), intr, [48, 64], t(s["means"]), t(s["colors"]), t(s["feats"]), t(s["rots"]), t(s["scales"]),
                 t(s["opacities"]), bg_color=[0, 0, 0])
    assert set(pkg) == {"render_color", "radii", "render_depth", "render_alpha", "render_feat"}
    N = s["means"].shape[0]
    assert pkg["render_color"].shape == (3, 48, 64) and pkg["render_feat"].shape == (12, 48, 64) and pkg["radii"].shape == (N,)
    assert pkg["render_depth"].shape == (1, 48, 64) and pkg["render_alpha"].shape == (1, 48, 64) and pkg["radii"].dtype == torch.int32
    # the same camera as the scene's.  `render` derives tanfov through atan / tan, which may land one fp32 ulp (6e-8 relative) from the scene's
    # W / (2 fx): the conic moves by 1.2e-7 relative, |power| <= ln(255) = 5.5 on a contributor, so each alpha by 7e-7 relative, and a pixel
    # has at most 38 contributors here: 3e-5 of slack on top of the plane's bound
    o = scenes.oracle("f_occupancy", 64)
    ok = ~scenes.fragile("f_occupancy")
    assert scenes.oracle("f_occupancy", 32)["count"].max() <= 38
    assert np.abs(pkg["render_alpha"].cpu().numpy() - o["alpha"])[:, ok].max() <= _bound("f_occupancy", "alpha") + 3e-5


def test_gpu_refusals_need_no_launch():
    from orv_amd.gs_render import GaussianRasterizer
    s, dev = scenes.scene("a_generic_400"), torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    r = GaussianRasterizer(_settings(s, dev))
    kw = dict(means3D=t(s["means"]), means2D=None, opacities=t(s["opacities"]), colors_precomp=t(s["colors"]), language_feature_precomp=t(s["feats"]),
              scales=t(s["scales"]), rotations=t(s["rots"]))
    with pytest.raises(NotImplementedError, match="F > 16"):
        r(**{**kw, "language_feature_precomp": torch.zeros(400, 17, device=dev)})
    with pytest.raises(NotImplementedError, match="no backward"):
        r(**{**kw, "means3D": t(s["means"]).requires_grad_()})
    with pytest.raises(NotImplementedError, match="float32"):
        r(**{**kw, "scales": t(s["scales"]).half()})
    vis = r.markVisible(t(s["means"]))
    assert np.array_equal(vis.cpu().numpy(), scenes.oracle("a_generic_400", 32)["pre"]["front"])
