"""Label-map compositing on the GPU: ``orv_amd.labelmap`` over csrc/labelmap.hip against the CPU restatement of the contract
(tests/labelmap_ref.py), against the fixtures the reference's own statements produced (tests/golden/labelmap/), and into
``occupancy.project_labels``.  Every comparison is exact equality of integers."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import labelmap_ref as ref
from orv_amd import labelmap as lm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("blobs_3x7x13x21", "empty_mask", "nested", "frozen_order")
DEV = "cuda:0"
# (F, n, H, W): one pixel; 63 pixels, fewer than four groups, with a tail; whole groups only; every row misaligned; the reference's check
# shape; no mask at all; more masks than lanes in a wave and than palette entries; many workgroups
SHAPES = ((1, 1, 1, 1), (2, 3, 7, 9), (1, 4, 16, 16), (2, 5, 5, 17), (3, 7, 13, 21), (1, 0, 6, 10), (1, 70, 9, 11), (2, 59, 120, 160))
KINDS = ("bool", "uint8", "logits")
TINY = np.float32(1e-45)                             # the smallest positive denormal
SET_VALUES = np.array([np.inf, TINY, 1e-30, 0.25, 3.0], dtype=np.float32)
UNSET_VALUES = np.array([0.0, -0.0, np.nan, -np.inf, -TINY, -1e-30, -0.25, -3.0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """-> (masks as numpy in the dtype of ``kind``, label ids, which pixels are set): per mask a random rectangle with holes plus scattered pixels."""
    F, n, H, W = shape
    rng = np.random.default_rng(zlib.crc32(repr((shape, kind)).encode()))
    on = np.zeros(shape, dtype=np.bool_)
    for f in range(F):
        for j in range(n):
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            y1, x1 = rng.integers(y0, H) + 1, rng.integers(x0, W) + 1
            on[f, j, y0:y1, x0:x1] = rng.uniform(size=(y1 - y0, x1 - x0)) < 0.8
            on[f, j] |= rng.uniform(size=(H, W)) < 0.03
    ids = rng.integers(0, 255, n)
    if n >= 70:
        ids[:3], ids[n // 2] = (254, 60, 59), 255                     # past the palette, its black entry, and the id that equals the background
        on[:, :, 0, :] = False                                        # so many masks cover everything: keep a row of background
        on[:, :, H - 1, W - 1] = False                                # and the last pixel for the mask of id 255 alone
        on[:, n // 2, H - 1, W - 1] = True
    if kind == "bool":
        masks = on
    elif kind == "uint8":
        masks = np.where(on, rng.choice(np.array([1, 2, 255], np.uint8), size=shape), np.uint8(0)).astype(np.uint8)
    else:
        masks = np.where(on, rng.choice(SET_VALUES, size=shape), rng.choice(UNSET_VALUES, size=shape)).astype(np.float32)
        assert np.array_equal(ref.is_set(masks), on)                  # the restatement's threshold rule against the construction
    masks.setflags(write=False), ids.setflags(write=False)
    return masks, ids, on


@functools.lru_cache(maxsize=None)
def expected(shape, kind):
    masks, ids, _ = case(shape, kind)
    return ref.stats(masks), ref.compose(masks, ids)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(DEV)                     # a copy: the cached cases are read-only


def same(got, want):
    """Exact equality of a device result and a numpy array, dtype and shape included."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


# ---- compose and mask_stats against the restatement ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compose_and_stats_equal_the_restatement(shape, kind):
    masks, ids, _ = case(shape, kind)
    (area, xyxy), (index, color, order) = expected(shape, kind)
    t = on_device(masks)
    got_area, got_xyxy = lm.mask_stats(t)
    assert same(got_area, area) and same(got_xyxy, xyxy)
    got_index, got_color, got_order = lm.compose(t, ids)
    assert same(got_order, order) and same(got_index, index) and same(got_color, color)
    assert got_index.is_cuda and got_color.is_cuda
    if shape[1] == 0:
        assert (index == 255).all() and (color == 0).all()
    if shape[1] >= 70:                                                # id 255 is painted: it has the colour of palette[255 % 60], not black
        assert ((index == 255) & (color.sum(-1) > 0)).any() and ((index == 255) & (color.sum(-1) == 0)).any()
    rgb = lm.compose(t, ids, channel_order="rgb")[1]
    assert same(rgb, np.ascontiguousarray(color[..., ::-1]))
    if shape[0] == 1:                                                 # one frame without the frame axis
        one = lm.compose(t[0], ids)
        assert same(one[0], index[0]) and same(one[1], color[0]) and same(lm.mask_stats(t[0])[0], area[0]) and same(lm.mask_stats(t[0])[1], xyxy[0])


def test_threshold_other_than_zero_and_nan():
    rng = np.random.default_rng(5)
    x = rng.normal(0.4, 1.0, size=(2, 5, 9, 23)).astype(np.float32)
    x[0, 0, 0, :6] = [0.5, np.nan, np.inf, 0.50000006, -np.inf, 0.49999997]
    ids = np.arange(5)
    t = on_device(x)
    for thr in (0.5, -0.0, -1e-30, float(TINY), float("nan"), float("inf")):
        assert same(lm.mask_stats(t, threshold=thr)[0], ref.stats(x, thr)[0]), thr
        got, want = lm.compose(t, ids, threshold=thr), ref.compose(x, ids, threshold=thr)
        assert all(same(g, w) for g, w in zip(got, want)), thr
    assert ref.stats(x, 0.5)[0].sum() not in (0, ref.stats(x, 0.0)[0].sum())
    palette = np.random.default_rng(6).integers(0, 256, (60, 3)).astype(np.uint8)
    got, want = lm.compose(t, ids, palette=palette), ref.compose(x, ids, palette=palette)
    assert same(got[1], want[1]) and not same(got[1], ref.compose(x, ids)[1])


# ---- addressing ----
@pytest.mark.parametrize("shape", ((2, 3, 8, 20), (1, 2, 5, 17)), ids=("whole_groups", "odd_plane"))
def test_every_plane_base_residue_gives_the_same_result(shape):
    """The masks start at every byte residue mod 16 (every multiple of 4 for fp32): a slice of a padded byte buffer viewed as the tensor."""
    for kind in KINDS:
        masks, ids, _ = case(shape, kind)
        (area, xyxy), (index, color, order) = expected(shape, kind)
        raw = np.array(masks).view(np.uint8).reshape(-1)              # a copy: the cached cases are read-only
        buf = torch.zeros(len(raw) + 64, dtype=torch.uint8, device=DEV)
        base = (-buf.data_ptr()) % 16                                 # buf[base] sits on a 16-byte boundary
        for off in range(0, 16, 4 if kind == "logits" else 1):
            buf.fill_(0xA5)
            view = buf[base + off:base + off + len(raw)]
            view.copy_(torch.from_numpy(raw))
            t = view.view({"bool": torch.bool, "uint8": torch.uint8, "logits": torch.float32}[kind]).view(shape)
            assert t.data_ptr() % 16 == off
            got = lm.mask_stats(t)
            assert same(got[0], area) and same(got[1], xyxy), (kind, off)
            got = lm.compose(t, ids)
            assert same(got[0], index) and same(got[1], color) and same(got[2], order), (kind, off)


@pytest.mark.parametrize("kind", KINDS)
def test_strided_views_equal_their_contiguous_copies(kind):
    shape = (3, 7, 13, 21)
    masks, ids, _ = case(shape, kind)
    (area, xyxy), (index, color, order) = expected(shape, kind)
    F, n, H, W = shape
    t = on_device(masks)
    views = {"[F,n,1,H,W][:, :, 0]": t.reshape(F, n, 1, H, W).clone()[:, :, 0],
             "[n,F,H,W] permuted": t.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3),
             "every other mask of [F,2n,H,W]": torch.stack([t, t.flip(1)], 2).reshape(F, 2 * n, H, W)[:, ::2]}
    assert not views["[n,F,H,W] permuted"].is_contiguous() and not views["every other mask of [F,2n,H,W]"].is_contiguous()
    for name, v in views.items():
        got = lm.mask_stats(v)
        assert same(got[0], area) and same(got[1], xyxy), name
        got = lm.compose(v, ids)
        assert same(got[0], index) and same(got[1], color), name
    # the [n,1,H,W] logits of one frame, as the segmenter returns them: permuted to [1,n,H,W] without a copy
    per_frame = t[0].reshape(n, 1, H, W).permute(1, 0, 2, 3)
    got = lm.compose(per_frame, ids)
    assert same(got[0], index[:1]) and same(got[1], color[:1])
    # one frame broadcast over three: stride 0
    got = lm.compose(t[:1].expand(3, n, H, W), ids)
    assert all(same(got[0][f], index[0]) for f in range(3)) and same(lm.mask_stats(t[:1].expand(3, n, H, W))[0], np.repeat(area[:1], 3, 0))


def test_plane_offsets_beyond_31_bits():
    """Two planes 2^31 + 37 bytes apart in one buffer: the plane offset is 64-bit arithmetic."""
    H, W, gap = 6, 40, (1 << 31) + 37
    buf = torch.zeros(gap + H * W, dtype=torch.uint8, device=DEV)
    on = np.zeros((1, 2, H, W), np.bool_)
    on[0, 0, 1:5, 3:30], on[0, 1, 2:4, 20:39] = True, True
    buf[:H * W] = on_device(on[0, 0].reshape(-1).astype(np.uint8))
    buf[gap:] = on_device(on[0, 1].reshape(-1).astype(np.uint8) * 200)
    t = torch.as_strided(buf, (1, 2, H, W), (0, gap, W, 1))
    got = lm.mask_stats(t)
    area, xyxy = ref.stats(on)
    assert same(got[0], area) and same(got[1], xyxy) and area.tolist() == [[108, 38]]
    got, want = lm.compose(t, [4, 9]), ref.compose(on, [4, 9])
    assert all(same(g, w) for g, w in zip(got, want))


# ---- ordering ----
def test_given_orders_shorter_permuted_and_tied():
    shape = (3, 7, 13, 21)
    masks, ids, _ = case(shape, "uint8")
    t = on_device(masks)
    rng = np.random.default_rng(11)
    for order in ([4, 1], [6], [], rng.permutation(7).tolist(), rng.permutation(7)[:5], torch.tensor([0, 1, 2, 3, 4, 5, 6]), np.arange(6, -1, -1)):
        got, want = lm.compose(t, ids, order=order), ref.compose(masks, ids, order=np.asarray(order, dtype=np.int64))
        assert all(same(g, w) for g, w in zip(got, want)), order
    assert not same(lm.compose(t, ids, order=[4, 1])[0], expected(shape, "uint8")[1][0])
    # equal areas: the larger mask number is painted first, the smaller one wins the shared pixels
    on = np.zeros((1, 4, 6, 12), np.bool_)
    for j in range(4):
        on[0, j, 1:5, 2 * j:2 * j + 5] = True                          # four 4 x 5 rectangles, each overlapping the next
    tied_ids = [10, 20, 30, 40]
    index, color, order = lm.compose(on_device(on), tied_ids)
    assert order.tolist() == [3, 2, 1, 0] and lm.mask_stats(on_device(on))[0].tolist() == [[20] * 4]
    want = ref.compose(on, tied_ids)
    assert same(index, want[0]) and same(color, want[1]) and same(order, want[2])
    assert index[0, 2, 2].item() == 10 and index[0, 2, 4].item() == 10 and index[0, 2, 5].item() == 20 and index[0, 2, 10].item() == 40


def test_two_runs_are_identical():
    shape = (2, 59, 120, 160)
    for kind in ("bool", "logits"):
        masks, ids, _ = case(shape, kind)
        t = on_device(masks)
        a, b = lm.compose(t, ids), lm.compose(t, ids)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        s, u = lm.mask_stats(t), lm.mask_stats(t)
        assert torch.equal(s[0], u[0]) and torch.equal(s[1], u[1])


# ---- against the reference and downstream ----
@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_equals_the_reference_fixture(name):
    fx = ref.load_fixture(os.path.join(GOLDEN, "labelmap", name + ".npz"))
    for masks in (fx["masks"], fx["masks"].astype(np.uint8) * 255, np.where(fx["masks"], 2.5, -2.5).astype(np.float32)):
        index, color, order = lm.compose(on_device(masks), fx["label_ids"])
        assert same(order, fx["order"]) and same(index, fx["index"]) and same(color, fx["color"])


def test_index_image_feeds_project_labels():
    from orv_amd import occupancy
    fx = ref.load_fixture(os.path.join(GOLDEN, "labelmap", "blobs_3x7x13x21.npz"))
    with np.load(os.path.join(GOLDEN, "occupancy", "project_exact.npz")) as z:
        points, extrin, intrin = on_device(z["points"]), z["extrin"], z["intrin"]
    index = lm.compose(on_device(fx["masks"]), fx["label_ids"])[0]
    for f in range(3):
        got = occupancy.project_labels(points, index[f], extrin, intrin)
        want = occupancy.project_labels(points, fx["index"][f], extrin, intrin)
        assert torch.equal(got, want) and (got == 59).any() and len(torch.unique(got)) > 3


def test_postprocess_labels_skips_annotated_frames():
    fx = ref.load_fixture(os.path.join(GOLDEN, "labelmap", "frozen_order.npz"))
    ids = fx["label_ids"]
    mark_i, mark_c = np.full((10, 24), 9, np.uint8), np.full((10, 24, 3), 8, np.uint8)
    frames = [{"masks": fx["masks"][0], "label_ids": ids},
              {"masks": fx["masks"][1], "label_ids": ids, "annotated_frame_index": mark_i, "annotated_frame_color": mark_c},
              {"masks": on_device(fx["masks"][2]), "label_ids": torch.from_numpy(ids)}]
    out = lm.postprocess_labels(frames)
    assert out is frames and frames[1]["annotated_frame_index"] is mark_i and frames[1]["annotated_frame_color"] is mark_c
    for f in (0, 2):                                                  # the order of frame 0 holds for frame 2
        assert same(frames[f]["annotated_frame_index"], fx["index"][f]) and same(frames[f]["annotated_frame_color"], fx["color"][f])
    # a resumed trajectory: frame 0 is annotated, so the order comes from frame 1 (the reference's defect) unless order= pins it
    resumed = [dict(frames[0]), {"masks": fx["masks"][1], "label_ids": ids}, {"masks": fx["masks"][2], "label_ids": ids}]
    lm.postprocess_labels(resumed)
    drift = ref.compose(fx["masks"][1:], ids)
    assert drift[2].tolist() != fx["order"].tolist()
    assert same(resumed[1]["annotated_frame_index"], drift[0][0]) and same(resumed[2]["annotated_frame_index"], drift[0][1])
    pinned = [dict(frames[0]), {"masks": fx["masks"][1], "label_ids": ids}, {"masks": fx["masks"][2], "label_ids": ids}]
    lm.postprocess_labels(pinned, order=fx["order"])
    assert same(pinned[1]["annotated_frame_index"], fx["index"][1]) and same(pinned[2]["annotated_frame_color"], fx["color"][2])
    # more masks than the order names: the extra ones stay unpainted; fewer: ValueError
    extra = [{"masks": fx["masks"][0], "label_ids": ids}]
    lm.postprocess_labels(extra, order=[0, 1])
    assert same(extra[0]["annotated_frame_index"], ref.compose(fx["masks"][:1], ids, order=[0, 1])[0][0]) and (extra[0]["annotated_frame_index"] != 7).all()
    with pytest.raises(ValueError, match="holds 2 masks but the paint order names mask 2"):
        lm.postprocess_labels([{"masks": fx["masks"][0, :2], "label_ids": ids[:2]}], order=[0, 1, 2])
