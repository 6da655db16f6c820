"""The scenes of the Gaussian-rasterizer tests (host and GPU share them) and their CPU oracle results, computed once per process.

A scene is a dict of numpy fp32 arrays (means, opacities, scales, rots, colors, feats or None) plus the camera (H, W, tanfovx, tanfovy, bg,
view, proj in the row-vector convention: view = (world-to-camera)^T, proj = view @ P^T)."""
from __future__ import annotations

import functools
import math

import numpy as np

import gs_render_ref as ref

F32 = np.float32


def camera(W, H, fx, fy, cx, cy, c2w=None, znear=0.1, zfar=200.0):
    """Pinhole camera -> (tanfovx, tanfovy, view, proj) as the reference's ``render`` derives them (float64 inside, fp32 out)."""
    c2w = np.eye(4) if c2w is None else c2w
    view = np.linalg.inv(c2w).T
    left, right = -(W - cx) * znear / fx, cx * znear / fx
    bottom, top = -(H - cy) * znear / fy, cy * znear / fy
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 2 * znear / (right - left), 2 * znear / (top - bottom)
    P[0, 2], P[1, 2] = (right + left) / (right - left), (top + bottom) / (top - bottom)
    P[2, 2], P[2, 3], P[3, 2] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear), 1.0
    view32 = view.astype(F32)
    proj32 = (view32 @ P.T.astype(F32)).astype(F32)
    return W / (2.0 * fx), H / (2.0 * fy), view32, proj32


def tilted_pose():
    """A camera-to-world pose with a small rotation about a skew axis and a small offset."""
    ax = np.array([0.3, -0.5, 0.2])
    ax /= np.linalg.norm(ax)
    ang = 0.06
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    c2w = np.eye(4)
    c2w[:3, :3] = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
    c2w[:3, 3] = [0.02, -0.015, 0.01]
    return c2w


def _pack(means, opac, scales, rots, colors, feats, H, W, cam, bg=(0.1, 0.2, 0.3), include_feature=True):
    tfx, tfy, view, proj = cam
    return dict(means=means.astype(F32), opacities=opac.astype(F32).reshape(-1, 1), scales=scales.astype(F32), rots=rots.astype(F32),
                colors=colors.astype(F32), feats=None if feats is None else feats.astype(F32), H=H, W=W, tanfovx=tfx, tanfovy=tfy,
                bg=np.asarray(bg, F32), view=view, proj=proj, include_feature=include_feature)


def generic(W, H, N, seed, F=12, include_feature=True):
    """Random anisotropic Gaussians seen by the tilted camera: scales 0.004-0.12 at depths 0.3-2, random quaternions, opacities 0.05-1 with
    every seventh exactly 1, 5 % of the Gaussians behind the near plane."""
    rng = np.random.RandomState(seed)
    fx, fy = 0.9 * W, 1.1 * H
    c2w = tilted_pose()
    cam = camera(W, H, fx, fy, W / 2 + 0.3, H / 2 - 0.4, c2w)
    z = rng.uniform(0.3, 2.0, N)
    behind = rng.rand(N) < 0.05
    z[behind] = -rng.uniform(0.05, 1.0, behind.sum())
    pc = np.stack([rng.uniform(-1.1, 1.1, N) * np.abs(z) * W / (2 * fx), rng.uniform(-1.1, 1.1, N) * np.abs(z) * H / (2 * fy), z], 1)
    means = pc @ c2w[:3, :3].T + c2w[:3, 3]
    scales = np.exp(rng.uniform(math.log(0.004), math.log(0.12), (N, 3)))
    rots = rng.randn(N, 4)
    opac = rng.uniform(0.05, 1.0, N)
    opac[::7] = 1.0
    return _pack(means, opac, scales, rots, rng.rand(N, 3), rng.rand(N, F) if F else None, H, W, cam, include_feature=include_feature)


def faint(N, seed, ladder):
    """Faint wide Gaussians at 40x24 with an identity camera: scales 2-4 at depths 1-2 keep exp(power) >= 0.5 over the whole image, so every
    Gaussian is in every tile's list and no alpha nears 1/255.  ``ladder``: opacities around 0.01 on a jittered depth ladder (no two depths
    closer than 1e-4 relative, no stop); otherwise opacities 0.02-0.04 at random depths (the stop fires in the second batch)."""
    rng = np.random.RandomState(seed)
    W, H, f = 40, 24, 42.0
    cam = camera(W, H, f, f, W / 2, H / 2)
    if ladder:
        z = 1.0 + (rng.permutation(N) + rng.uniform(-0.3, 0.3, N)) / N
        opac = rng.uniform(0.009, 0.011, N)
    else:
        z = rng.uniform(1.0, 2.0, N)
        opac = rng.uniform(0.02, 0.04, N)
    means = np.stack([rng.uniform(-0.45, 0.45, N) * z * W / (2 * f), rng.uniform(-0.45, 0.45, N) * z * H / (2 * f), z], 1)
    return _pack(means, opac, rng.uniform(2.0, 4.0, (N, 3)), rng.randn(N, 4), rng.rand(N, 3), rng.rand(N, 12), H, W, cam)


def occupancy(seed):
    """ORV-style occupancy grid at 64x48: 14x10x6 cell centres, 30 % occupied, identity rotation, opacity 1, isotropic scale 0.02, one-hot
    12-class features, zero colour, identity camera: full of exact depth ties.  -> (scene, unique_classes)."""
    rng = np.random.RandomState(seed)
    W, H, f = 64, 48, 60.0
    cam = camera(W, H, f, f, W / 2, H / 2)
    gx, gy, gz = np.meshgrid(np.linspace(-0.187, 0.193, 14), np.linspace(-0.131, 0.137, 10), np.linspace(0.152, 0.401, 6), indexing="ij")
    means = np.stack([gx, gy, gz], -1).reshape(-1, 3)
    occ = rng.rand(means.shape[0]) < 0.30
    means = means[occ]
    N = means.shape[0]
    cls = rng.randint(0, 12, N)
    rots = np.zeros((N, 4))
    rots[:, 0] = 1
    scene = _pack(means, np.ones(N), np.full((N, 3), 0.02), rots, np.zeros((N, 3)), np.eye(12)[cls], H, W, cam, bg=(0, 0, 0))
    return scene, np.array([0, 2, 3, 5, 7, 8, 11, 13, 17, 19, 23, 29], dtype=np.int64)


def behind_camera(N=64, seed=5):
    s = generic(48, 32, N, seed)
    pc = np.random.RandomState(seed).uniform(-1, 1, (N, 3))
    pc[:, 2] = -np.abs(pc[:, 2]) - 0.05
    c2w = tilted_pose()
    s["means"] = (pc @ c2w[:3, :3].T + c2w[:3, 3]).astype(F32)
    return s


def empty():
    s = generic(48, 32, 4, 6)
    for k in ("means", "opacities", "scales", "rots", "colors", "feats"):
        s[k] = s[k][:0]
    return s


SCENES = {
    "a_generic_400": lambda: generic(80, 56, 400, 11),
    "b_generic_1500": lambda: generic(80, 56, 1500, 12),
    "c_partial_tiles": lambda: generic(37, 21, 300, 13),
    "d_70_tiles": lambda: generic(160, 112, 5000, 14),
    "e_faint_stop": lambda: faint(330, 15, ladder=False),
    "e_faint_ladder": lambda: faint(700, 16, ladder=True),
    "f_occupancy": lambda: occupancy(17)[0],
    "g_behind": behind_camera,
    "g_empty": empty,
    "h_no_feature": lambda: generic(80, 56, 400, 19, include_feature=False),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name, bits):
    """The oracle's result on a scene at fp32 (bits = 32) or fp64 (bits = 64); shared by every test of the process, never modified."""
    s = scene(name)
    feats = s["feats"] if s["include_feature"] else None
    return ref.rasterize(s["means"], s["opacities"], s["scales"], s["rots"], s["colors"], feats, s["H"], s["W"], s["tanfovx"], s["tanfovy"],
                         s["bg"], 1.0, s["view"], s["proj"], dtype=np.float32 if bits == 32 else np.float64)


def fragile(name):
    """Fragile pixels of a scene: flagged by either precision's run."""
    return oracle(name, 32)["fragile"] | oracle(name, 64)["fragile"]
