#!/usr/bin/env python
"""Writes the reference-generated voxelization fixtures of tests/golden/voxelize/ (inputs and outputs only, one small .npz per case).

    python tools/gen_voxelize_golden.py --reference /path/to/ORV [--out tests/golden/voxelize]

The outputs come from the reference's own code, run on the CPU:
  * its CPU kernels (orv/ops/voxelize/voxelization_cpu.cpp), built with torch.utils.cpp_extension.load in a temporary directory outside the
    tree.  That file declares hard_voxelize_forward_impl / dynamic_voxelize_forward_impl without defining them, so it is linked with the
    small translation unit below, which defines both as device dispatches;
  * its Python wrapper (orv/ops/voxelize/voxelization.py), imported with the extension loader pointed at that build;
  * its points_to_voxels (orv/dataset/prepare_dataset.py), compiled from the function's own source and run with device="cpu" - the rest of
    that module needs packages that have nothing to do with voxelization.
No test runs this tool; tests/test_voxelize_host.py checks the CPU restatement (tests/voxelize_ref.py) against what it wrote.
"""
import argparse
import ast
import importlib.util
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include <torch/extension.h>
#include "pytorch_cpp_helper.hpp"
#include "pytorch_device_registry.hpp"

int hard_voxelize_forward_impl(const at::Tensor& points, at::Tensor& voxels, at::Tensor& coors, at::Tensor& num_points_per_voxel,
                               const std::vector<float> voxel_size, const std::vector<float> coors_range, const int max_points,
                               const int max_voxels, const int NDim) {
    return DISPATCH_DEVICE_IMPL(hard_voxelize_forward_impl, points, voxels, coors, num_points_per_voxel, voxel_size, coors_range, max_points,
                                max_voxels, NDim);
}

void dynamic_voxelize_forward_impl(const at::Tensor& points, at::Tensor& coors, const std::vector<float> voxel_size,
                                   const std::vector<float> coors_range, const int NDim) {
    DISPATCH_DEVICE_IMPL(dynamic_voxelize_forward_impl, points, coors, voxel_size, coors_range, NDim);
}
"""

MAX_TIE_SHARE = 0.20


def load_reference(ref_root):
    """-> (voxelization, points_to_voxels) of the reference, running on the CPU."""
    from torch.utils import cpp_extension
    ops_dir = os.path.join(ref_root, "orv", "ops")
    build = tempfile.mkdtemp(prefix="voxelize_golden_")
    shim = os.path.join(build, "voxelize_impl_shim.cpp")
    with open(shim, "w", encoding="utf-8") as f:
        f.write(SHIM)
    op = cpp_extension.load("voxelization_cpu_golden", sources=[os.path.join(ops_dir, "voxelize", "voxelization_cpu.cpp"), shim],
                            extra_include_paths=[os.path.join(ops_dir, "include")], build_directory=build, verbose=False)
    name = "ivideogpt.ops.voxelize.voxelization"                      # the spelling points_to_voxels imports
    parts = name.split(".")
    for depth in range(1, len(parts)):
        pkg = types.ModuleType(".".join(parts[:depth]))
        pkg.__path__ = []
        sys.modules[pkg.__name__] = pkg
    spec = importlib.util.spec_from_file_location(name, os.path.join(ops_dir, "voxelize", "voxelization.py"))
    mod = importlib.util.module_from_spec(spec)
    real_load, real_avail = cpp_extension.load, torch.cuda.is_available
    cpp_extension.load, torch.cuda.is_available = (lambda *a, **k: op), (lambda: False)      # its CPU branch, with the build from above
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec.loader.exec_module(mod)
    finally:
        cpp_extension.load, torch.cuda.is_available = real_load, real_avail
    assert mod.voxelization_op is op
    sys.modules[name] = mod
    path = os.path.join(ref_root, "orv", "dataset", "prepare_dataset.py")
    with open(path, "r", encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "points_to_voxels")
    import numpy.typing as npt
    from typing import List
    ns = {"np": np, "npt": npt, "torch": torch, "Tensor": torch.Tensor, "List": List}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return mod.voxelization, ns["points_to_voxels"]


def save(out_dir, name, **arrays):
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 512 * 1024, (name, size)
    print(f"{name}: {size} bytes")


def hard_case(voxelization, out_dir, name, points, voxel_size, coors_range, max_points, max_voxels, seed, note):
    pts = torch.from_numpy(points)
    voxels, coors, num = voxelization(pts.clone(), voxel_size, coors_range, max_points, max_voxels, True)
    dyn = voxelization(pts.clone(), voxel_size, coors_range, -1, -1, True)
    save(out_dir, name, points=points, voxel_size=np.asarray(voxel_size, np.float64), coors_range=np.asarray(coors_range, np.float64),
         max_points=np.int64(max_points), max_voxels=np.int64(max_voxels), seed=np.int64(seed), note=np.str_(note),
         voxels=voxels.numpy(), coors=coors.numpy(), num_points_per_voxel=num.numpy(), dynamic_coors=dyn.numpy())
    return voxels.numpy(), coors.numpy(), num.numpy(), dyn.numpy()


def vote_case(voxelization, points_to_voxels, out_dir, name, xyz, labels, voxel_size, coors_range, seed, note):
    """points_to_voxels of the reference, plus the per-voxel counts of the stored labels in the reference's voxels (which voxels are ties)."""
    rng_arg = None if coors_range is None else list(coors_range)
    out = points_to_voxels(xyz.copy(), list(voxel_size), labels.copy(), point_cloud_range=rng_arg, device=torch.device("cpu"))
    pts = torch.cat([torch.from_numpy(xyz)[:, :3], torch.from_numpy(labels.astype(np.int32)).float()[:, None] + 1], 1)
    pts = pts[~torch.isnan(pts[:, :3]).any(1)]
    rng_used = rng_arg if rng_arg is not None else [pts[:, 0].min(), pts[:, 1].min(), pts[:, 2].min(), pts[:, 0].max(), pts[:, 1].max(), pts[:, 2].max()]
    voxels, coors, num = voxelization(pts, list(voxel_size), rng_used, 100, 100000, True)
    stored = voxels[..., -1].numpy().astype(np.int64)
    counts = np.stack([np.bincount(row, minlength=256) for row in stored]) if len(stored) else np.zeros((0, 256), np.int64)
    assert counts.max(initial=0) < 65536 and np.array_equal(coors.numpy()[:, ::-1], out[:, :3])
    top = counts[:, 1:].max(axis=1)
    ties = (counts[:, 1:] == top[:, None]).sum(axis=1) > 1
    assert ties.mean() <= MAX_TIE_SHARE, (name, ties.mean())
    print(f"  {name}: M = {len(out)}, dtype {out.dtype}, tie share {ties.mean():.3f}, fullest voxel {int(num.max())}")
    save(out_dir, name, points=xyz, labels=labels, voxel_size=np.asarray(voxel_size, np.float64),
         coors_range=np.zeros(0) if coors_range is None else np.asarray(coors_range, np.float64), seed=np.int64(seed), note=np.str_(note),
         out=out, out_dtype=np.str_(str(out.dtype)), label_counts=counts.astype(np.uint16), num_points_per_voxel=num.numpy())


def surface_points(rng, n, lo, hi, thickness):
    """n points scattered about the surface z = f(x, y) inside [lo, hi]: many points per voxel near it, like a reconstructed scene."""
    xy = rng.uniform(lo[:2], hi[:2], size=(n, 2))
    u = (xy - lo[:2]) / (hi[:2] - lo[:2])
    z = lo[2] + (hi[2] - lo[2]) * (0.5 + 0.3 * np.sin(3.0 * u[:, 0]) * np.cos(2.0 * u[:, 1])) + rng.normal(0.0, thickness, n)
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


def boundary_points():
    """Every edge the cell rule has, on the 8-cell axes of range [-0.2, -0.2, 0, 0.2, 0.2, 0.4], voxel 0.05."""
    vs = np.float32(0.05)
    lo, hi = np.array([-0.2, -0.2, 0.0], np.float32), np.array([0.2, 0.2, 0.4], np.float32)
    mid = (lo + np.float32(3.5) * vs).astype(np.float32)
    rows = [lo.copy(), hi.copy(), np.nextafter(hi, np.float32(-np.inf)), np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))]
    for a in range(3):
        for k in range(9):                                             # lo + k vs in fp32; k = 8 is the upper face (outside)
            for step in (0, -1, 1):
                p = mid.copy()
                p[a] = np.float32(lo[a] + np.float32(k) * vs)
                if step:
                    p[a] = np.nextafter(p[a], np.float32(step * np.inf))
                rows.append(p)
        for bad in (np.nan, np.inf, -np.inf):
            p = mid.copy()
            p[a] = bad
            rows.append(p)
        p = hi.copy()                                                   # at the upper face on one axis only
        p[(a + 1) % 3], p[(a + 2) % 3] = mid[(a + 1) % 3], mid[(a + 2) % 3]
        rows.append(p)
    rows.append(np.full(3, np.nan, np.float32))
    pts = np.stack(rows).astype(np.float32)
    feat = np.arange(len(pts), dtype=np.float32)[:, None] + 1             # a fourth feature that tells the rows apart
    return np.concatenate([pts, feat], 1), [0.05] * 3, [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds orv/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "voxelize"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    voxelization, points_to_voxels = load_reference(args.reference)

    # both caps biting at once, and the voxel cap lifted
    seed = 11
    pts = np.random.default_rng(seed).uniform(0.0, 0.05, size=(2000, 4)).astype(np.float32)
    v, c, n, d = hard_case(voxelization, args.out, "caps_both", pts, [0.005] * 3, [0, 0, 0, 0.04, 0.04, 0.04], 5, 300, seed,
                           "uniform [0, 0.05)^3 (fourth feature too), 8^3 grid; max_points 5 and max_voxels 300 both bite")
    print(f"  caps_both: M = {len(c)}, voxels with 5 points {(n == 5).sum()}, points out of range {(d[:, 0] < 0).sum()}")
    assert len(c) == 300 and (n == 5).any() and 900 < (d[:, 0] < 0).sum() < 1020
    v, c, n, d = hard_case(voxelization, args.out, "caps_points_only", pts, [0.005] * 3, [0, 0, 0, 0.04, 0.04, 0.04], 5, 20000, seed,
                           "the points of caps_both with max_voxels large")
    assert 300 < len(c) <= 512

    bp, bvs, brange = boundary_points()
    v, c, n, d = hard_case(voxelization, args.out, "boundaries", bp, bvs, brange, 35, 20000, 0,
                           "points at lo, at hi, one ulp inside and outside, lo + k vs in fp32 (and its neighbours) for k = 0..8 per axis, NaN and +-inf rows")
    print(f"  boundaries: N = {len(bp)}, M = {len(c)}, invalid {(d[:, 0] < 0).sum()}")
    assert (d[0] == 0).all() and (d[1] == -1).all() and (d[2] == 7).all()

    seed = 12
    far = np.random.default_rng(seed).uniform(1.0, 2.0, size=(300, 4)).astype(np.float32)
    far[::7, 0] = -far[::7, 0]
    v, c, n, d = hard_case(voxelization, args.out, "all_invalid", far, [0.05] * 3, [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4], 35, 20000, seed,
                           "every point outside the range: M = 0")
    assert len(c) == 0 and (d == -1).all()
    seed = 13
    one = np.random.default_rng(seed).uniform(0.1001, 0.1499, size=(150, 5)).astype(np.float32)
    v, c, n, d = hard_case(voxelization, args.out, "one_voxel", one, [0.05] * 3, [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4], 35, 20000, seed,
                           "every point in one voxel: 150 points, 35 kept")
    assert len(c) == 1 and n[0] == 35

    # small N across the feature widths: sizes around one wave (64) and one workgroup (256), 12^3 grid with some points outside
    for N, C in ((1, 3), (63, 4), (64, 7), (65, 3), (257, 4), (1025, 7)):
        seed = 100 + N
        p = np.random.default_rng(seed).uniform(-0.05, 0.65, size=(N, C)).astype(np.float32)
        hard_case(voxelization, args.out, f"small_n{N}_c{C}", p, [0.05, 0.05, 0.05], [0.0, 0.0, 0.0, 0.6, 0.6, 0.6], 3, 500, seed,
                  "uniform [-0.05, 0.65)^C on a 12^3 grid of [0, 0.6]^3; max_points 3, max_voxels 500")

    # the vote: a dominant class per voxel, so that ties stay below MAX_TIE_SHARE
    for name, n_pts, given_range, vsz, seed in (("vote_given_range", 4000, [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4], 0.02, 21),
                                                ("vote_data_range", 3000, None, 0.04, 22)):
        rng = np.random.default_rng(seed)
        lo, hi = np.array([-0.2, -0.2, 0.0]), np.array([0.2, 0.2, 0.4])
        xyz = surface_points(rng, n_pts, lo - 0.02, hi + 0.02, 0.01)
        xyz[::97, rng.integers(0, 3)] = np.nan                           # rows the reference strips
        cell = np.floor((np.nan_to_num(xyz) - lo) / 0.1).astype(np.int64)
        dominant = (cell[:, 0] * 7 + cell[:, 1] * 3 + cell[:, 2]) % 12
        labels = np.where(rng.uniform(size=n_pts) < 0.85, dominant, rng.integers(0, 12, n_pts)).astype(np.int64)
        labels[rng.integers(0, n_pts, 40)] = 254                         # the largest label the contract allows
        vote_case(voxelization, points_to_voxels, args.out, name, xyz, labels, [vsz] * 3, given_range, seed,
                  f"surface points about [-0.2, 0.2]^2 x [0, 0.4] with NaN rows, voxel {vsz}, labels: the dominant class of the point's 0.1 cell with p = 0.85")
    rng = np.random.default_rng(23)
    xyz = surface_points(rng, 4000, np.array([-0.2, -0.2, 0.0]), np.array([0.2, 0.2, 0.4]), 0.01)
    vote_case(voxelization, points_to_voxels, args.out, "vote_crowded", xyz, (rng.uniform(size=4000) < 0.8).astype(np.int64) * 3, [0.1] * 3,
              [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4], 23, "4^3 coarse voxels: most hold more than 100 points, so the vote sees the first 100 only")


if __name__ == "__main__":
    main()
