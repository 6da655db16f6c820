"""Label-map compositing, host side (no GPU): the CPU restatement of the contract (tests/labelmap_ref.py) against every fixture the
reference's own statements produced (tests/golden/labelmap/), the tie rule of the paint order, the Python surface of ``orv_amd.labelmap``
(refusals, the skip and ValueError rules of ``postprocess_labels``) and the C ABI of the ``orv_lm_*`` entry points (validation before any
launch).  Every comparison is exact equality of integers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import labelmap_ref as ref
from orv_amd import labelmap as lm          # every test here is about this module: none passes without it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "labelmap")
FIXTURES = ("blobs_3x7x13x21", "empty_mask", "nested", "frozen_order")


def fixture(name):
    return ref.load_fixture(os.path.join(GOLDEN, name + ".npz"))


# ---- the restatement equals the reference ----
def test_there_are_fixtures():
    assert {f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")} == set(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference(name):
    fx = fixture(name)
    index, color, order = ref.compose(fx["masks"], fx["label_ids"])
    assert index.dtype == np.uint8 and color.dtype == np.uint8 and order.dtype == np.int64
    assert np.array_equal(order, fx["order"]) and np.array_equal(index, fx["index"]) and np.array_equal(color, fx["color"])
    area0 = ref.stats(fx["masks"])[0][0]
    assert len(set(area0.tolist())) == len(area0)                      # the order-setting frame has no tie: the reference's order is defined
    assert np.array_equal(order, np.flip(np.argsort(area0)))


def test_fixtures_cover_what_they_claim():
    blobs, empty, nested, frozen = (fixture(n) for n in FIXTURES)
    assert blobs["masks"].shape == (3, 7, 13, 21) and blobs["label_ids"].max() > 59 and (blobs["index"] == 255).any()
    area, xyxy = ref.stats(empty["masks"])
    assert (area[:, 2] == 0).all() and (xyxy[:, 2] == 0).all() and empty["order"][-1] == 2 and (area[:, [0, 1, 3, 4]] > 0).all()
    m = nested["masks"]
    assert all((m[f, j + 1] & ~m[f, j]).sum() == 0 and m[f, j + 1].sum() < m[f, j].sum() for f in range(2) for j in range(4))
    assert sorted(np.unique(nested["index"]).tolist()) == [10, 30, 40, 50, 255]          # every nested mask stays visible
    inner = nested["masks"][0, 1] & ~nested["masks"][0, 2]                                # the ring of id 255: painted, so coloured
    assert (nested["index"][0][inner] == 255).all() and (nested["color"][0][inner] == ref.palette60()[255 % 60][::-1]).all()
    assert (nested["color"][0][~nested["masks"][0, 0]] == 0).all()
    a = ref.stats(frozen["masks"])[0]
    assert a[0].tolist() == [80, 48, 24] and a[1, 2] > a[1, 0] and a[2, 2] > a[2, 0]
    assert (frozen["index"][2] == 7).all()                                               # mask 2 is still painted last and covers the frame
    later = ref.compose(frozen["masks"][2:], frozen["label_ids"])
    assert later[2].tolist() == [2, 1, 0] and not np.array_equal(later[0][0], frozen["index"][2])


def test_palette_is_the_package_palette():
    from orv_amd import conditions
    assert np.array_equal(ref.palette60().astype(np.float32), conditions.palette60())
    assert (ref.palette60()[59] == 0).all()


def test_paint_order_tie_rule_and_distinct_areas():
    tied = np.array([5, 9, 5, 9, 1, 5])
    want = [3, 1, 5, 2, 0, 4]                                          # ascending stable [4, 0, 2, 5, 1, 3], flipped
    assert lm.paint_order(tied).tolist() == want and ref.paint_order(tied).tolist() == want
    assert lm.paint_order(torch.from_numpy(tied)).tolist() == want
    assert lm.paint_order(tied).dtype == np.int64
    assert lm.paint_order(np.zeros(4, np.int64)).tolist() == [3, 2, 1, 0]               # all equal: the smaller number is painted last and wins
    rng = np.random.default_rng(3)
    for n in (1, 2, 17, 70):
        a = rng.permutation(4000)[:n]
        assert np.array_equal(lm.paint_order(a), np.flip(np.argsort(a))) and np.array_equal(ref.paint_order(a), np.flip(np.argsort(a)))
    assert lm.paint_order(np.zeros(0, np.int64)).shape == (0,)
    with pytest.raises(ValueError, match=r"expected the \[n\] areas of one frame"):
        lm.paint_order(np.zeros((2, 3)))


def test_threshold_rule_of_the_restatement():
    tiny = np.float32(1e-45)                                           # the smallest positive denormal
    x = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, tiny, -tiny, 1e-30, -1e-30, 0.5, 0.75, -2.0], dtype=np.float32)
    assert ref.is_set(x).tolist() == [False, False, False, False, True, False, True, False, True, False, True, True, False]
    bits = x.view(np.int32)
    assert np.array_equal(ref.is_set(x), (bits >= 1) & (bits <= 0x7F800000))             # the contract's statement for threshold 0
    assert ref.is_set(x, 0.5).tolist() == [False] * 4 + [True] + [False] * 6 + [True, False]
    assert ref.is_set(x, -1e-30).tolist() == [True, True, False, False, True, False, True, True, True, False, True, True, False]
    assert not ref.is_set(x, np.nan).any()
    assert ref.is_set(np.array([0, 1, 2, 255], np.uint8)).tolist() == [False, True, True, True]


# ---- Python surface ----
SUPPORTED = "supported: a CUDA tensor masks [F,n,H,W] or [n,H,W] of torch.bool, torch.uint8"


def test_refusals_name_the_supported_set():
    ids = [1, 2]
    with pytest.raises(NotImplementedError, match="not a CUDA tensor") as e:
        lm.compose(torch.zeros(2, 4, 5, dtype=torch.bool), ids)
    assert SUPPORTED in str(e.value) and "there is no CPU path" in str(e.value)
    with pytest.raises(NotImplementedError, match="not a CUDA tensor"):
        lm.mask_stats(torch.zeros(1, 2, 4, 5, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="torch.float16, not bool, uint8 or float32") as e:
        lm.compose(torch.zeros(2, 4, 5, dtype=torch.float16), ids)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="torch.int64, not bool, uint8 or float32"):
        lm.mask_stats(torch.zeros(2, 4, 5, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="is a ndarray, not a tensor"):
        lm.compose(np.zeros((2, 4, 5), np.bool_), ids)
    with pytest.raises(NotImplementedError, match="no backward") as e:
        lm.compose(torch.zeros(2, 4, 5, requires_grad=True), ids)
    assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match=r"not \[F,n,H,W\] or \[n,H,W\]"):
        lm.mask_stats(torch.zeros(4, 5, dtype=torch.bool))
    meta = lambda *shape, **kw: torch.empty(*shape, device="meta", **kw)      # a shape only: no 4 GB of host memory
    for bad, why in ((torch.zeros(2, 5, 4, dtype=torch.bool).transpose(1, 2), "is not contiguous"),
                     (torch.zeros(2, 4, 10, dtype=torch.uint8)[:, :, ::2], "is not contiguous"),
                     (torch.zeros(2, 8, 5)[:, ::2], "is not contiguous"), (torch.zeros(2, 0, 5), "H \\* W == 0"),
                     (torch.zeros(2, 4, 0, dtype=torch.bool), "H \\* W == 0"), (meta(1, 65536, 1, dtype=torch.bool), "H or W >= 65536"),
                     (meta(1, 1, 65536, dtype=torch.uint8), "H or W >= 65536")):
        with pytest.raises(NotImplementedError, match=why) as e:
            lm.mask_stats(bad)
        assert SUPPORTED in str(e.value)
        with pytest.raises(NotImplementedError, match=why):
            lm.compose(bad, ids)
    for bad, why in (([1], "holds 1 values for n = 2"), ([1, 256], "outside \\[0, 255\\]"), ([-1, 3], "outside \\[0, 255\\]"),
                     (np.array([1.0, 2.0]), "float64, not an integer type"), (torch.tensor([True, False]), "torch.bool, not an integer type"),
                     (np.zeros((2, 1), np.int64), "not one dimension")):
        with pytest.raises(NotImplementedError, match=why) as e:
            lm._check_label_ids(bad, 2)
        assert SUPPORTED in str(e.value)
    assert lm._check_label_ids(np.array([0, 255], np.uint8), 2).tolist() == [0, 255] and lm._check_label_ids([], 0).shape == (0,)
    for bad, why in (([0, 1, 2, 3], "more than n = 3"), ([0, 3], "outside \\[0, n = 3\\)"), ([-1], "outside \\[0, n = 3\\)"), ([1, 1], "names a mask twice"),
                     ([0.5], "not an integer type")):
        with pytest.raises(NotImplementedError, match=why) as e:
            lm._check_order(bad, 3)
        assert SUPPORTED in str(e.value)
    assert lm._check_order([2, 0], 3).tolist() == [2, 0] and lm._check_order((), 3).shape == (0,)
    for bad, why in ((np.zeros((59, 3), np.uint8), "not uint8 \\[60, 3\\]"), (np.zeros((60, 3), np.float32), "float32 \\[60, 3\\], not uint8"),
                     (torch.zeros(60, 4, dtype=torch.uint8), "not uint8 \\[60, 3\\]")):
        with pytest.raises(NotImplementedError, match=why) as e:
            lm._check_palette(bad, "bgr")
        assert SUPPORTED in str(e.value)
    with pytest.raises(NotImplementedError, match="channel_order = 'gbr'"):
        lm._check_palette(None, "gbr")
    pal = ref.palette60()
    assert np.array_equal(lm._check_palette(None, "rgb"), pal) and np.array_equal(lm._check_palette(None, "bgr"), pal[:, ::-1])
    assert np.array_equal(lm._check_palette(pal[::-1].copy(), "bgr"), pal[::-1, ::-1])


def test_postprocess_labels_skip_and_value_error_rules_on_the_host():
    masks, ids = np.zeros((3, 4, 5), np.bool_), np.array([1, 2, 3], np.uint8)
    done = {"masks": masks, "label_ids": ids, "annotated_frame_index": np.full((4, 5), 7, np.uint8), "annotated_frame_color": np.zeros((4, 5, 3), np.uint8)}
    frames = [dict(done), dict(done)]
    assert lm.postprocess_labels(frames) is frames and (frames[0]["annotated_frame_index"] == 7).all()     # all annotated: nothing to do, no device
    short = {"masks": masks[:2], "label_ids": ids[:2]}
    with pytest.raises(ValueError, match="frame 1 holds 2 masks but the paint order names mask 2"):
        lm.postprocess_labels([dict(done), short], order=[2, 0, 1])
    assert "annotated_frame_index" not in short
    with pytest.raises(NotImplementedError, match="names a mask twice"):
        lm.postprocess_labels([short], order=[1, 1])
    with pytest.raises(NotImplementedError, match="negative mask number"):
        lm.postprocess_labels([short], order=[-1])
    half = {"masks": masks, "label_ids": ids, "annotated_frame_index": np.zeros((4, 5), np.uint8)}       # one key only: not skipped
    with pytest.raises(ValueError, match="frame 0 holds 3 masks"):
        lm.postprocess_labels([half], order=[3])


def test_signatures_and_defaults():
    import orv_amd
    d = {k: p.default for k, p in inspect.signature(lm.compose).parameters.items()}
    assert list(d) == ["masks", "label_ids", "order", "threshold", "channel_order", "palette"]
    assert (d["order"], d["threshold"], d["channel_order"], d["palette"]) == (None, 0.0, "bgr", None)
    assert list(inspect.signature(lm.mask_stats).parameters) == ["masks", "threshold"] and list(inspect.signature(lm.paint_order).parameters) == ["area0"]
    assert list(inspect.signature(lm.postprocess_labels).parameters)[:2] == ["frames", "order"]
    assert "labelmap" not in inspect.getsource(orv_amd.install)                    # the package-level install() is unchanged


# ---- C ABI ----
NAMES = ("orv_lm_mask_stats", "orv_lm_compose")


def test_lm_symbols_are_declared_exported_bound_and_cited():
    from orv_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(_lib.lib(), name) is not None
        assert callable(getattr(ops, name[4:]))
    for name, cites in (("orv_lm_mask_stats", ("prepare_dataset.py:1406-1420", ":1275-1279")), ("orv_lm_compose", ("prepare_dataset.py:1412-1444",))):
        end = hdr.index("int " + name + "(")
        doc = hdr[hdr.rindex("/*", 0, end):end]
        assert all(c in doc for c in cites), name                                # each cites the reference lines it replaces
    assert "section 18" in hdr[hdr.index("Label-map compositing"):hdr.index("int orv_lm_mask_stats(")]
    with open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile"), "r", encoding="utf-8") as f:
        assert "labelmap.hip" in f.read()


def test_lm_entry_points_validate_before_any_launch():
    """Null pointers, negative counts, plane sizes, the mask width, strides, bands and order entries: nonzero with the reason in
    orv_last_error(), prefixed by the entry point's name, without a GPU (no device pointer is followed; ``order`` is a host array)."""
    from orv_amd._lib import lib
    h = lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lambda: h.orv_last_error().decode()
    ids, pal = (ctypes.c_ubyte * 4)(1, 2, 3, 4), (ctypes.c_ubyte * 180)()

    def stats(masks=p, mb=1, F=2, n=4, H=6, W=10, sf=240, sn=60, bands=2, ws=p, area=p, xyxy=p):
        return h.orv_lm_mask_stats(masks, mb, F, n, H, W, sf, sn, 0.0, bands, ws, area, xyxy, None)

    def compose(masks=p, mb=1, F=2, n=4, H=6, W=10, sf=240, sn=60, order=(3, 1, 0), m=None, label_ids=ids, palette=pal, steps=p, index=p, color=p):
        arr = None if order is None else (ctypes.c_int * max(len(order), 1))(*order)
        return h.orv_lm_compose(masks, mb, F, n, H, W, sf, sn, 0.0, arr, len(order or ()) if m is None else m, label_ids, palette, steps, index, color, None)

    for call, name in ((stats, NAMES[0]), (compose, NAMES[1])):
        assert call(F=-1) != 0 and "F must not be negative" in err() and err().startswith(name + ":"), name
        assert call(n=-1) != 0 and "n must not be negative" in err() and err().startswith(name + ":"), name
        for bad in (dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(H=-3)):
            assert call(**bad) != 0 and "1 <= H, W < 65536" in err() and err().startswith(name + ":"), (name, bad)
        for mb in (0, 2, 3, 8):
            assert call(mb=mb) != 0 and f"mask_bytes = {mb}" in err() and "1 (bool or uint8, set where nonzero) or 4 (fp32 logits)" in err(), (name, mb)
            assert err().startswith(name + ":")
        for bad in (dict(sf=-1), dict(sn=-60), dict(sn=1 << 40)):
            assert call(**bad) != 0 and "element strides" in err() and err().startswith(name + ":"), (name, bad)
        assert call(masks=p + 2, mb=4) != 0 and "4-byte" in err() and err().startswith(name + ":")
    for bad in (dict(masks=None), dict(ws=None), dict(area=None), dict(xyxy=None)):
        assert stats(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[0] + ":"), bad
    for bands in (0, -1, 7):
        assert stats(bands=bands) != 0 and f"bands = {bands}" in err() and "1 to H = 6" in err()
    assert stats(F=40000, n=40000, bands=6) != 0 and "below 2^31" in err()
    for bad in (dict(masks=None), dict(steps=None), dict(index=None), dict(color=None), dict(palette=None), dict(label_ids=None), dict(order=None, m=2)):
        assert compose(**bad) != 0 and "null pointer" in err() and err().startswith(NAMES[1] + ":"), bad
    assert compose(m=-1) != 0 and "m = -1" in err() and err().startswith(NAMES[1] + ":")
    assert compose(order=(0, 1, 2, 3, 0)) != 0 and "m = 5" in err() and "0 to n = 4" in err()
    for order, k in (((3, 4, 0), 1), ((0, 1, 70), 2), ((-1,), 0)):
        assert compose(order=order) != 0 and f"order[{k}] = {order[k]}" in err() and "[0, n = 4)" in err() and err().startswith(NAMES[1] + ":"), order
    assert compose(index=p + 8) != 0 and "16-byte aligned" in err()
    # nothing to do is not an error, and launches nothing
    assert stats(F=0, masks=None, ws=None, area=None, xyxy=None) == 0 and stats(n=0, masks=None, ws=None, area=None, xyxy=None) == 0
    assert compose(F=0, order=(), masks=None, steps=None, index=None, color=None) == 0
