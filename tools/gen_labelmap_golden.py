#!/usr/bin/env python
"""Writes the reference-generated label-map fixtures of tests/golden/labelmap/ (inputs and outputs only, one small .npz per case).

    python tools/gen_labelmap_golden.py --reference /path/to/ORV [--out tests/golden/labelmap]

The outputs come from the reference's own statements, run on the CPU.  orv/dataset/prepare_dataset.py cannot be imported (it needs packages
that have nothing to do with these lines), so its syntax tree is cut instead, at run time: the body of the frame loop of
_postprocess_labels, from the assignment of ``masks`` to the last assignment of ``indices_2d``, without the ``if ... continue`` that tests
for the two annotation keys (a ``continue`` does not compile outside its loop; the fixtures hold no annotated frame).  The cut is executed
once per frame with ``labels``, ``mask_annotator`` and ``mask_indices_sequence`` in its namespace, and ``mask_indices_sequence`` is carried
from frame to frame as the loop does.

supervision and cv2 are not installed where this was written, so the cut runs against this tool's own stand-ins, and what they define is
NOT pinned by the fixtures:
  * sv.Detections(...).area is the count of set pixels of each mask, and sv.mask_to_xyxy the inclusive bounding box (unused by the cut's
    outputs);
  * resolve_color looks the colour up by class id modulo the palette's length, the class id being the label id (ColorLookup.CLASS);
  * Color.as_bgr() is the triple reversed;
  * cv2.addWeighted rounds and saturates src1 * alpha + src2 * beta + gamma into dst: the identity at opacity 1.
What the fixtures do pin is everything the reference's statements do with those: the paint order and its freezing from the first frame, the
two paint loops, the int32 -1 background and its cast to uint8.

The reference's order is np.flip(np.argsort(area)) with numpy's default sort, which is not stable: the order among equal areas is
unspecified, so the tool asserts that the order-setting frame of every fixture has pairwise distinct areas.  No reference text is in this
tool or in the fixtures.  No test runs this tool; tests/test_labelmap_host.py checks the CPU restatement (tests/labelmap_ref.py) against
what it wrote, and tests/test_gpu_labelmap.py the kernels.
"""
import argparse
import ast
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import labelmap_ref as ref  # noqa: E402


# ---- stand-ins (this tool's own; see the docstring for what they leave unpinned) ----
class Color:
    def __init__(self, r, g, b):
        self.r, self.g, self.b = int(r), int(g), int(b)

    def as_bgr(self):
        return (self.b, self.g, self.r)


class ColorPalette:
    def __init__(self, colors):
        self.colors = list(colors)

    def by_idx(self, idx):
        return self.colors[int(idx) % len(self.colors)]


def mask_to_xyxy(masks):
    out = np.zeros((len(masks), 4), dtype=int)
    for i, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        if len(ys):
            out[i] = xs.min(), ys.min(), xs.max(), ys.max()
    return out


class Detections:
    def __init__(self, xyxy, mask=None, class_id=None):
        self.xyxy, self.mask, self.class_id = xyxy, mask, class_id

    @property
    def area(self):
        return np.array([np.count_nonzero(m) for m in self.mask])


def resolve_color(color, detections, detection_idx, color_lookup=None):
    return color.by_idx(detections.class_id[detection_idx])


def add_weighted(src1, alpha, src2, beta, gamma, dst=None):
    out = np.clip(np.rint(src1.astype(np.float64) * alpha + src2.astype(np.float64) * beta + gamma), 0, 255).astype(np.uint8)
    if dst is not None:
        dst[...] = out
        return dst
    return out


# ---- the cut ----
def _targets(stmt):
    return [t.id for t in stmt.targets if isinstance(t, ast.Name)] if isinstance(stmt, ast.Assign) else []


class Reference:
    def __init__(self, root):
        self.path = os.path.join(root, "orv", "dataset", "prepare_dataset.py")
        with open(self.path, "r", encoding="utf-8") as f:
            tree = ast.parse(f.read(), filename=self.path)
        fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_postprocess_labels")
        loops = [n for n in ast.walk(fn) if isinstance(n, ast.For) and any("masks" in _targets(s) for s in n.body)]
        assert len(loops) == 1, "the frame loop of _postprocess_labels was not found"
        body = loops[0].body
        i0 = next(i for i, s in enumerate(body) if "masks" in _targets(s))
        i1 = [i for i, s in enumerate(body) if "indices_2d" in _targets(s)][-1]
        cut = body[i0:i1 + 1]
        skips = [s for s in cut if isinstance(s, ast.If) and any(isinstance(c, ast.Continue) for c in ast.walk(s))]
        assert len(skips) == 1 and "annotated_frame_index" in ast.unparse(skips[0].test), "the test for annotated frames was not found"
        self.cut = [s for s in cut if s is not skips[0]]
        assert not any(isinstance(c, (ast.Continue, ast.Break, ast.Return)) for s in self.cut for c in ast.walk(s))
        self.code = compile(ast.Module(body=self.cut, type_ignores=[]), self.path, "exec")
        palette = ColorPalette([Color(*c) for c in ref.palette60().tolist()])
        self.annotator = types.SimpleNamespace(color=palette, opacity=1.0, color_lookup="class")
        self.base = {"np": np, "sv": types.SimpleNamespace(Detections=Detections, mask_to_xyxy=mask_to_xyxy), "resolve_color": resolve_color,
                     "cv2": types.SimpleNamespace(addWeighted=add_weighted)}

    def trajectory(self, masks, label_ids):
        """masks bool [F,n,H,W], label_ids uint8 [n] -> (index [F,H,W], color [F,H,W,3], the frozen order)."""
        sequence, index, color = None, [], []
        for frame in masks:
            ns = dict(self.base, labels={"masks": frame.copy(), "label_ids": label_ids.copy()}, mask_annotator=self.annotator,
                      mask_indices_sequence=sequence)
            exec(self.code, ns)
            sequence = ns["mask_indices_sequence"]
            index.append(ns["indices_2d"]), color.append(ns["annotated_frame"])
        return np.stack(index), np.stack(color), np.asarray(sequence).astype(np.int64)


# ---- cases ----
def blobs(rng, F, n, H, W, drift=1):
    """n random ellipses per frame that drift a little from frame to frame and overlap freely."""
    cy, cx = rng.uniform(0, H, n), rng.uniform(0, W, n)
    ry, rx = rng.uniform(1.0, H / 2, n), rng.uniform(1.0, W / 2, n)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((F, n, H, W), dtype=np.bool_)
    for f in range(F):
        for j in range(n):
            out[f, j] = ((yy - cy[j]) / ry[j]) ** 2 + ((xx - cx[j]) / rx[j]) ** 2 <= 1.0
        cy, cx = cy + rng.uniform(-drift, drift, n), cx + rng.uniform(-drift, drift, n)
    return out


def save(reference, out_dir, name, masks, label_ids, note):
    label_ids = np.asarray(label_ids, dtype=np.uint8)
    area0 = masks[0].reshape(masks.shape[1], -1).sum(1)
    assert len(set(area0.tolist())) == len(area0), f"{name}: the order-setting frame has equal areas {area0.tolist()}; the reference's order is unspecified"
    index, color, order = reference.trajectory(masks, label_ids)
    assert index.dtype == np.uint8 and color.dtype == np.uint8
    mine = ref.compose(masks, label_ids)
    assert all(np.array_equal(a, b) for a, b in zip(mine, (index, color, order))), f"{name}: the restatement differs from the reference"
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, masks_packed=np.packbits(masks), shape=np.array(masks.shape, np.int64), label_ids=label_ids, order=order,
                        index=index, color=color, note=np.str_(note))
    size = os.path.getsize(path)
    assert size < 64 * 1024, (name, size)
    print(f"{name}: masks {masks.shape}, areas of frame 0 {area0.tolist()}, order {order.tolist()}, painted {(index != 255).mean():.2f}, {size} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds orv/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "labelmap"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    reference = Reference(args.reference)

    rng = np.random.default_rng(181)
    save(reference, args.out, "blobs_3x7x13x21", blobs(rng, 3, 7, 13, 21), [3, 0, 59, 61, 12, 200, 7],
         "3 frames of 7 drifting ellipses at 13 x 21; label ids beyond the palette (61, 200) and the black entry 59")

    m = blobs(rng, 2, 5, 12, 18)
    m[:, 2] = False
    save(reference, args.out, "empty_mask", m, [1, 2, 3, 4, 5], "mask 2 is empty in both frames: area 0, painted last, paints nothing")

    m = np.zeros((2, 5, 16, 20), dtype=np.bool_)
    for j in range(5):                                                 # stored largest first
        k = 5 - j
        m[0, j, 8 - k:8 + k, 10 - k - 1:10 + k + 1] = True
        m[1, j, 8 - k:8 + k, 10 - k:10 + k + 2] = True
    save(reference, args.out, "nested", m, [10, 255, 30, 40, 50],
         "five fully nested rectangles: each smaller one stays visible inside the larger; id 255 is painted and keeps palette[255 % 60]")

    m = np.zeros((3, 3, 10, 24), dtype=np.bool_)                       # frame 0: areas 80 > 48 > 24; later frames: mask 2 outgrows mask 0
    m[0, 0, 1:9, 2:12], m[0, 1, 2:8, 8:16], m[0, 2, 3:7, 10:16] = True, True, True
    m[1, 0, 1:9, 2:12], m[1, 1, 2:8, 8:16], m[1, 2, 0:10, 6:22] = True, True, True
    m[2, 0, 4:6, 2:6], m[2, 1, 2:8, 8:16], m[2, 2, 0:10, 0:24] = True, True, True
    save(reference, args.out, "frozen_order", m, [5, 6, 7],
         "mask 2 is the smallest in frame 0 and the largest afterwards: the order frozen from frame 0 lets it cover the others in frames 1 and 2")
    fx = ref.load_fixture(os.path.join(args.out, "frozen_order.npz"))
    per_frame = ref.compose(fx["masks"][1:2], fx["label_ids"])
    assert not np.array_equal(per_frame[0][0], fx["index"][1]), "frozen_order: a per-frame order gives the same image; the case shows nothing"


if __name__ == "__main__":
    main()
