#!/usr/bin/env python
"""Writes the reference-generated occupancy fixtures of tests/golden/occupancy/ (inputs and outputs only, one small .npz per case).

    python tools/gen_occupancy_golden.py --reference /path/to/ORV [--out tests/golden/occupancy]

The outputs come from the reference's own code, run on the CPU.  orv/dataset/prepare_dataset.py cannot be imported (it needs packages that
have nothing to do with these lines), so its syntax tree is cut instead, at run time:
  * project_3d_to_2d and generate_colors are compiled from their own source;
  * the labelling statements of get_occupancy (the body of the try block that assigns labels2d, without its first statement, which reads a
    file) are executed with points, labels2d, extrin and intrin in their namespace;
  * the scene statements of get_render are executed in two runs: from the assignment of occ_range to that of opacity (the dense attribute
    tensors), and, inside the frame loop, from the torch.tensor(...) of occ_data to the reshape of occ_mask, with a fresh namespace per case
    (on the CPU semantics_zero.to(device) aliases the zero grid, which a second frame would inherit);
  * create_full_center_coords is compiled from orv/dataset/gs_render.py.
No reference text is in this tool or in the fixtures.  No test runs this tool; tests/test_occupancy_host.py checks the CPU restatement
(tests/occupancy_ref.py) against what it wrote.
"""
import argparse
import ast
import colorsys
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import occupancy_ref as ref  # noqa: E402

MAX_DIFF_SHARE = 0.001            # the real-geometry projection fixture: reference and contract may disagree on at most 0.1 % of the points


def _parse(path):
    with open(path, "r", encoding="utf-8") as f:
        return ast.parse(f.read(), filename=path)


def _function(tree, name):
    return next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)


def _targets(stmt):
    return [t.id for t in stmt.targets if isinstance(t, ast.Name)] if isinstance(stmt, ast.Assign) else []


def _run(stmts, path, ns):
    exec(compile(ast.Module(body=list(stmts), type_ignores=[]), path, "exec"), ns)
    return ns


def _span(body, first, last, nth_last=-1):
    """The consecutive statements of ``body`` from the first assignment to ``first`` to the last (or nth) assignment to ``last``."""
    i0 = next(i for i, s in enumerate(body) if first in _targets(s))
    hits = [i for i, s in enumerate(body) if last in _targets(s) and i >= i0]
    return body[i0:hits[nth_last] + 1]


class Reference:
    def __init__(self, root):
        self.path = os.path.join(root, "orv", "dataset", "prepare_dataset.py")
        tree = _parse(self.path)
        gs_path = os.path.join(root, "orv", "dataset", "gs_render.py")
        base = {"np": np, "torch": torch, "colorsys": colorsys}
        self.ns = _run([_function(tree, "project_3d_to_2d"), _function(tree, "generate_colors")], self.path, dict(base))
        self.ns.update(_run([_function(_parse(gs_path), "create_full_center_coords")], gs_path, dict(base)))
        occupancy = _function(tree, "get_occupancy")
        tries = [n for n in ast.walk(occupancy) if isinstance(n, ast.Try) and n.body and "labels2d" in _targets(n.body[0])]
        assert len(tries) == 1, "the labelling block of get_occupancy was not found"
        self.labelling = tries[0].body[1:]                              # without the np.load(...) that reads the label file
        assert "labels2d" in _targets(self.labelling[0]) and "labels3d" in ast.unparse(self.labelling[-1])
        render = _function(tree, "get_render")
        self.scene_init = _span(render.body, "occ_range", "opacity", 0)
        loops = [n for n in ast.walk(render) if isinstance(n, ast.For) and any("occ_data" in _targets(s) for s in n.body)]
        assert len(loops) == 1, "the frame loop of get_render was not found"
        frame = _span(loops[0].body, "occ_data", "occ_mask")
        assert "np.load" in ast.unparse(frame[0]) and "torch.tensor" in ast.unparse(frame[1])
        self.scene_frame = frame[1:]                                    # without the np.load(...) that reads the occupancy file

    def labels(self, points, labels2d, extrin, intrin):
        """-> (labels3d, the reference's P, its truncated pixels of every point)."""
        h, w = labels2d.shape
        ns = dict(self.ns, points=torch.from_numpy(points), labels2d=labels2d.copy(), extrin=torch.from_numpy(extrin),
                  intrin=torch.from_numpy(intrin), labels2d_size=(h, w), colors60=self.ns["generate_colors"](), device=torch.device("cpu"))
        _run(self.labelling, self.path, ns)
        P = ns["intrin"] @ torch.linalg.inv(ns["extrin"])
        with np.errstate(all="ignore"):
            uv = self.ns["project_3d_to_2d"](ns["points"], extrin=ns["extrin"], intrin=ns["intrin"])[:, :2].numpy()
        return ns["labels3d"].numpy(), P.numpy(), uv

    def gaussians(self, occ, point_cloud_range, voxel_size, base_scale, exp_scale, num_channels):
        ns = dict(self.ns, point_cloud_range=list(point_cloud_range), voxel_size=list(voxel_size), base_scale=base_scale, exp_scale=exp_scale,
                  device=torch.device("cpu"), num_channels_language_feature=num_channels, colors60=torch.zeros(60, 3), is_labeled=True)
        _run(self.scene_init, self.path, ns)
        ns["occ_data"] = occ
        with ref.serial():                                              # rows of one cell are written in order: the last one stays
            _run(self.scene_frame, self.path, ns)
        m = ns["occ_mask"]
        return {"xyz": ns["xyz"][m].numpy(), "rgb": ns["rgb"][m].numpy(), "feat": ns["feat"][m].numpy(), "rot": ns["rot"][m].numpy(),
                "scale": ns["scale"][m].numpy(), "opacity": ns["opacity"][m].numpy(), "unique_classes": ns["unique_classes"].numpy(),
                "is_labeled": np.bool_(ns["is_labeled"])}


def save(out_dir, name, **arrays):
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 512 * 1024, (name, size)
    print(f"{name}: {size} bytes")


def camera(angle, back):
    """Camera-to-world: a rotation about y by ``angle`` rad, the camera set ``back`` behind the scene's centre along its own axis."""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    m = np.eye(4)
    m[:3, :3] = rot
    m[:3, 3] = np.array([0.0, 0.0, 0.2]) - rot @ np.array([0.0, 0.0, back])
    return m.astype(np.float32)


def surface_points(rng, n, lo, hi, thickness):
    """n points scattered about the surface z = f(x, y) inside [lo, hi], like a reconstructed scene (as tools/gen_voxelize_golden.py)."""
    xy = rng.uniform(lo[:2], hi[:2], size=(n, 2))
    u = (xy - lo[:2]) / (hi[:2] - lo[:2])
    z = lo[2] + (hi[2] - lo[2]) * (0.5 + 0.3 * np.sin(3.0 * u[:, 0]) * np.cos(2.0 * u[:, 1])) + rng.normal(0.0, thickness, n)
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


def label_image(rng, h, w):
    """Blocks of labels 0..11 with some 255 (unlabelled) pixels, uint8 like the files the reference reads."""
    img = ((np.arange(h)[:, None] // max(h // 6, 1)) * 5 + np.arange(w)[None, :] // max(w // 8, 1)) % 12
    img = img.astype(np.uint8)
    img[rng.uniform(size=(h, w)) < 0.05] = 255
    return img


def projection_cases(reference, out_dir):
    # every product and sum exact: coordinates on a 1/64 lattice, a quarter turn, translations and intrinsics with few mantissa bits
    seed = 31
    rng = np.random.default_rng(seed)
    pts = (rng.integers(-96, 97, size=(3000, 3)) / 64.0).astype(np.float32)
    pts[:, 2] = (rng.integers(-16, 160, size=3000) / 64.0).astype(np.float32)          # some behind the camera, some at h_2 = 0
    extrin = np.array([[0, -1, 0, 0.25], [1, 0, 0, -0.5], [0, 0, 1, -0.125], [0, 0, 0, 1]], dtype=np.float32)
    intrin = np.array([[8, 0, 8], [0, 8, 6], [0, 0, 1]], dtype=np.float32)
    intrin4 = np.eye(4, dtype=np.float32)
    intrin4[:3, :3] = intrin
    img = label_image(rng, 12, 16)
    lab, P, uv = reference.labels(pts, img, extrin, intrin4)
    assert np.array_equal(P, intrin4 @ np.linalg.inv(extrin.astype(np.float64)).astype(np.float32))
    mine = ref.project_labels(pts, img, P)
    assert np.array_equal(mine, lab), "the exact fixture must agree on every point"
    print(f"  project_exact: {np.isfinite(uv).all(1).sum()} finite, inside {(lab != 0).sum()} labelled, label 59: {(lab == 59).sum()}")
    save(out_dir, "project_exact", points=pts, labels2d=img, extrin=extrin, intrin=intrin4, P=P, labels3d=lab, seed=np.int64(seed),
         note=np.str_("lattice points, quarter-turn camera, 12 x 16 label image: every product and sum of the projection is exact in fp32"))

    # the real geometry: range +-0.2 x +-0.2 x 0.4, focal length 650 px, 640 x 480, camera rotated 0.3 rad and set back 0.45
    seed = 32
    rng = np.random.default_rng(seed)
    pts = surface_points(rng, 20000, np.array([-0.2, -0.2, 0.0]), np.array([0.2, 0.2, 0.4]), 0.01)
    extrin = camera(0.3, 0.45)
    intrin4 = np.eye(4, dtype=np.float32)
    intrin4[:3, :3] = np.array([[650, 0, 320], [0, 650, 240], [0, 0, 1]], dtype=np.float32)
    img = label_image(rng, 480, 640)
    lab, P, uv = reference.labels(pts, img, extrin, intrin4)
    mine = ref.project_labels(pts, img, P)
    diff = np.flatnonzero(mine != lab)
    print(f"  project_real: {len(diff)} of {len(pts)} labels differ from the reference's, {(lab != 0).sum()} labelled, label 59: {(lab == 59).sum()}")
    assert len(diff) <= MAX_DIFF_SHARE * len(pts), "over the cap: no fixture is written"
    save(out_dir, "project_real", points=pts, labels2d=img, extrin=extrin, intrin=intrin4, P=P, labels3d=lab,
         ref_pixels=np.trunc(uv).astype(np.int64), seed=np.int64(seed),
         note=np.str_("surface points in +-0.2 x +-0.2 x [0, 0.4], f = 650 px, 640 x 480, camera rotated 0.3 rad and set back 0.45"))


def scene_cases(reference, out_dir):
    def case(name, occ, rng6, vs, note, base_scale=0.00023, exp_scale=3.7, num_channels=12):
        got = reference.gaussians(occ, rng6, vs, base_scale, exp_scale, num_channels)
        print(f"  {name}: M = {len(occ)}, n = {len(got['xyz'])}, classes {got['unique_classes'].tolist()}, feat {got['feat'].shape}")
        save(out_dir, name, occ=occ, point_cloud_range=np.asarray(rng6, np.float64), voxel_size=np.asarray(vs, np.float64),
             base_scale=np.float64(base_scale), exp_scale=np.float64(exp_scale), num_channels=np.int64(num_channels), note=np.str_(note), **got)

    rng = np.random.default_rng(41)
    small = ([0.0, 0.0, 0.0, 1.0, 0.75, 0.625], [0.125] * 3)
    shape = ref.grid_shape(*small)
    print(f"  small grid {shape}")
    cells = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    pick = cells[rng.permutation(len(cells))[:90]]
    occ = np.concatenate([pick, rng.integers(0, 7, (90, 1))], 1).astype(np.float64)
    case("scene_small", occ, *small, "90 distinct cells of an unequal-axis grid, labels 0..6, float64 rows as get_occupancy saves them")
    dup = np.concatenate([occ[:40], occ[:25]], 0)
    dup[40:, 3] = (dup[40:, 3] + 3) % 9
    dup[5, 3], dup[6, 3] = -1, 200
    case("scene_duplicates", dup, *small, "25 cells given twice with another label (the last row wins), labels -1 and 200 (clamped)")
    full = np.concatenate([cells, rng.integers(1, 5, (len(cells), 1))], 1).astype(np.int64)
    case("scene_full", full[rng.permutation(len(full))], *small, "every cell occupied with labels 1..4: no extra class 0")
    one = np.array([[3, 2, 1, 0]], dtype=np.int32)
    case("scene_single_class", one, *small, "one cell of label 0: a single class, is_labeled false")
    real = ([-0.2, -0.2, 0, 0.2, 0.2, 0.4], [0.01] * 3)
    pts = surface_points(rng, 3000, np.array([-0.2, -0.2, 0.0]), np.array([0.2, 0.2, 0.4]), 0.01)
    cell = np.clip(np.floor((pts - np.array([-0.2, -0.2, 0.0])) / 0.01), 0, np.array(ref.grid_shape(*real)) - 1)
    occ = np.concatenate([cell, rng.integers(0, 12, (len(cell), 1))], 1).astype(np.float64)
    case("scene_grid40", occ, *real, "3000 surface rows on the reference's range cut into 0.01 cells, 12 classes, many duplicates")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds orv/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "occupancy"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    reference = Reference(args.reference)
    projection_cases(reference, args.out)
    scene_cases(reference, args.out)


if __name__ == "__main__":
    main()
