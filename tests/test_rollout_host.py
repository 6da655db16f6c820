"""Cascaded rollouts, host side (no GPU): the slice planner and the stitch rule against every case the reference's own loops produced
(tests/golden/rollout_plan.json, written by tools/gen_rollout_golden.py), the refusals, the numpy restatement of the two value contracts
(tests/rollout_ref.py) against ``VideoProcessor.postprocess_video`` / ``preprocess``, and the C ABI of the ``orv_frames_*`` entry points
(declared, exported, bound, validation before any launch)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import rollout_ref as ref
from orv_amd import rollout as ro           # every test here is about this module: none passes without it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "rollout_plan.json"), "r", encoding="utf-8") as _f:
    CASES = json.load(_f)["cases"]
KEYS = ("frame_ids", "start_frame_idx", "next_start_frame_idx", "is_last", "sample_index")


def _id(case):
    i = case["inputs"]
    return f"n{i['n_frames']}-L{i['sequence_length']}-i{i['sequence_interval']}-s{i['start_frame_interval']}-f{int(i['vae_has_first_single_frame'])}"


def test_the_fixture_covers_the_cases():
    have = {(c["inputs"]["n_frames"], c["inputs"]["sequence_length"], c["inputs"]["sequence_interval"], c["inputs"]["start_frame_interval"],
             c["inputs"]["vae_has_first_single_frame"]) for c in CASES}
    assert {(n, 16, 1, 16, True) for n in (17, 18, 20, 31, 32, 33, 34, 40, 47, 48, 49, 50)} <= have
    assert {(n, 8, 1, 8, True) for n in (12, 17, 19, 20, 25)} <= have
    assert len({c for c in have if c[1:] == (8, 1, 4, True)}) >= 5                # 17 and 25 are refused by the reference itself: 16 and 24
    assert any(not c[4] for c in have) and sum(c[2] == 2 for c in have) == 2
    assert all((c["stitched"] is None) == (c["inputs"]["sequence_interval"] != 1) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_planner_and_stitch_equal_the_reference(case):
    plan = ro.plan_slices(**case["inputs"])
    assert [{k: (list(getattr(s, k)) if k == "frame_ids" else getattr(s, k)) for k in KEYS} for s in plan] == case["slices"]
    ranges = ro.stitch_ranges(plan)
    assert [k for k, _, _ in ranges] == list(range(len(plan))) and all(b == 0 for _, b, _ in ranges)
    if case["stitched"] is not None:
        assert ro.stitched_frame_ids(plan) == case["stitched"]
        starts = [0] + [s.next_start_frame_idx for s in plan[:-1]]               # the reference's own arithmetic at interval 1
        assert [e for _, _, e in ranges] == [starts[k + 1] - starts[k] for k in range(len(plan) - 1)] + [len(plan[-1].frame_ids) - 1]
    kept = ro.stitch_ranges(plan, keep_last_frame=True)
    assert kept[:-1] == ranges[:-1] and kept[-1] == (len(plan) - 1, 0, len(plan[-1].frame_ids))
    assert ro.stitched_frame_ids(plan, keep_last_frame=True) == ro.stitched_frame_ids(plan) + [plan[-1].frame_ids[-1]]


def test_quirks_are_kept():
    plan = ro.plan_slices(20, 8, 1, 8)                                           # the regenerated last slice: a hand-off in mid-slice
    assert [s.start_frame_idx for s in plan] == [0, 8, 11] and [e for _, _, e in ro.stitch_ranges(plan)] == [8, 3, 8]
    assert plan[-1].is_last and plan[-1].frame_ids == tuple(range(11, 20))
    assert not any(s.is_last for s in ro.plan_slices(31)) and len(ro.plan_slices(31)) == 1       # short by 2: dropped, nobody is last
    assert ro.plan_slices(17)[0].frame_ids[0] == 0 and ro.plan_slices(17, vae_has_first_single_frame=False)[0].frame_ids == tuple(range(16))


def test_interval_two_does_not_repeat_the_handoff_frame():
    plan = ro.plan_slices(70, 16, 2, 16)
    ids = ro.stitched_frame_ids(plan)
    assert plan[0].next_start_frame_idx == 32 and ids.count(32) == 1 and ids == sorted(set(ids))
    assert ro.stitch_ranges(plan)[0] == (0, 0, 16)                                # the position of frame 32, not 32 - 0
    assert "deviation" in ro.stitch_ranges.__doc__.lower()


def test_refusals():
    with pytest.raises(ValueError, match="too short for one slice"):
        ro.plan_slices(16)
    with pytest.raises(ValueError, match="too short for one slice"):
        ro.plan_slices(8, 8, 1, 8)
    with pytest.raises(ValueError, match="hand-off frame inside the current slice"):
        ro.plan_slices(60, 8, 1, 12)                                             # a stride larger than the slice
    with pytest.raises(ValueError, match="equal to it without the first single frame.*hand-off frame inside the current slice"):
        ro.plan_slices(40, 16, 1, 16, vae_has_first_single_frame=False)
    good = ro.plan_slices(33)
    bad = [ro.Slice(good[0].frame_ids, 0, 40, False, 0), good[1]]
    with pytest.raises(ValueError, match="not among its frame_ids"):
        ro.stitch_ranges(bad)
    with pytest.raises(ValueError, match="positive integers"):
        ro.plan_slices(33, 16, 0, 16)
    with pytest.raises(ValueError, match="plan is empty"):
        ro.stitch_ranges([])


class _CpuPipe:
    _execution_device = torch.device("cpu")
    vae = None


def test_rollout_refuses_before_it_runs():
    plan = ro.plan_slices(20, 8, 1, 8)
    kw = dict(height=64, width=96)
    with pytest.raises(ValueError, match="num_views = 2"):
        ro.rollout(_CpuPipe(), None, plan, lambda s: {}, num_views=2, **kw)
    with pytest.raises(ValueError, match="output_type = 'pt'"):
        ro.rollout(_CpuPipe(), None, plan, lambda s: {}, output_type="pt", **kw)
    with pytest.raises(ValueError, match="gave 2 entries"):
        ro.rollout(_CpuPipe(), None, plan, [{}, {}], **kw)
    with pytest.raises(ValueError, match="no resize between chunks"):
        ro.rollout(_CpuPipe(), None, plan, lambda s: {})
    with pytest.raises(RuntimeError, match="no CPU path"):
        ro.rollout(_CpuPipe(), None, plan, lambda s: {}, **kw)


class _WrongSizePipe:
    """Everything ``rollout`` touches in front of its first kernel launch, with a decoder that returns another frame size."""
    _execution_device = torch.device("cuda:0")

    class vae:
        encode_channels_last = staticmethod(lambda h, dtype=None: None)

    class video_processor:
        class _Image:
            def to(self, **kw):
                return self
        preprocess = staticmethod(lambda image, height=None, width=None: _WrongSizePipe.video_processor._Image())

    def __init__(self, shape):
        self.shape, self.calls = shape, 0

    def _prepare_call(self, image, **kw):
        from types import SimpleNamespace
        return SimpleNamespace(batch_size=1, dtype=torch.bfloat16, generator=kw["generator"])

    def _generate(self, image, call):
        self.calls += 1
        return torch.zeros(self.shape)

    def maybe_free_model_hooks(self):
        pass


def test_rollout_refuses_a_decoded_size_that_is_not_the_calls():
    plan = ro.plan_slices(20, 8, 1, 8)
    pipe = _WrongSizePipe((1, 3, 9, 32, 48))
    with pytest.raises(RuntimeError, match=r"chunk 0 generated 32 x 48 frames.*\(64, 96\).*no resize between chunks"):
        ro.rollout(pipe, None, plan, lambda s: {}, height=64, width=96)
    assert pipe.calls == 1                                                        # refused at the first chunk, before any launch
    with pytest.raises(RuntimeError, match="chunk 0 decoded .* for a slice of 9 RGB frames"):
        ro.rollout(_WrongSizePipe((1, 3, 5, 64, 96)), None, plan, lambda s: {}, height=64, width=96)


def test_exports():
    import orv_amd
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj as Pipe
    assert orv_amd.plan_slices is ro.plan_slices and orv_amd.stitch_ranges is ro.stitch_ranges
    assert callable(orv_amd.rollout) and callable(Pipe.rollout) and callable(Pipe._generate) and callable(Pipe._prepare_call)
    from orv_amd import rollout
    assert rollout is ro and orv_amd.rollout is ro and orv_amd.rollout is ro      # one object under that name, before and after the import
    assert ro.rollout is not ro and callable(ro.rollout)                          # the callable module; the function is its attribute
    with pytest.raises(ValueError, match="num_views = 3"):
        rollout(_CpuPipe(), None, ro.plan_slices(17), lambda s: {}, num_views=3, height=8, width=8)


# ---- the value contracts ----
def _processor():
    from orv_amd.components import VideoProcessor
    return VideoProcessor(vae_latent_channels=16, vae_scale_factor=8)


def test_quantize_ref_equals_postprocess_video():
    video = ref.sweep_video(nan=False)                                            # numpy's cast of a NaN is platform-defined: left out here
    x, k = ref.halfway_inputs()
    assert len(set(k.tolist())) >= 150 and any(v % 2 for v in k) and any(v % 2 == 0 for v in k)
    y = (x / np.float32(2) + np.float32(0.5)) * np.float32(255)
    assert np.array_equal(y, k + 0.5) and np.array_equal(ref.quantize_ref(x), k + (k % 2))       # half to even: k even stays, k odd goes up
    pil = _processor().postprocess_video(torch.from_numpy(video), "pil")
    got = np.stack([np.array(f) for f in pil[0]])[None]
    want = ref.quantize_frames_ref(video)
    assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)
    assert set(np.unique(want).tolist()) == set(range(256))                      # the sweep reaches every level
    assert ref.quantize_ref(np.array([np.inf, -np.inf, np.nan, 1.5, -1.5, 0.0], dtype=np.float32)).tolist() == [255, 0, 0, 255, 0, 128]


def test_handoff_table_equals_preprocess_of_all_grey_levels():
    import PIL.Image
    levels = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = PIL.Image.fromarray(np.stack([levels] * 3, axis=-1))
    pre = _processor().preprocess([img], height=16, width=16)
    assert tuple(pre.shape) == (1, 3, 16, 16) and pre.dtype == torch.float32 and float(pre.min()) == -1.0
    want = pre.to(torch.bfloat16)[0, 0].reshape(256)
    table = ro.handoff_table()
    assert table.dtype == torch.bfloat16 and torch.equal(table, want) and torch.equal(table, pre.to(torch.bfloat16)[0, 2].reshape(256))
    assert np.array_equal(table.view(torch.int16).numpy().view(np.uint16), ref.handoff_table_ref())
    bright = PIL.Image.fromarray(np.full((8, 8, 3), 200, dtype=np.uint8))       # no dark pixel: still normalised exactly once
    assert torch.equal(_processor().preprocess([bright], height=8, width=8).to(torch.bfloat16)[0, 0, 0, 0], table[200])


# ---- C ABI ----
NAMES = ("orv_frames_quantize", "orv_frames_handoff")


def test_frames_symbols_are_declared_exported_bound_and_cited():
    from orv_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(_lib.lib(), name) is not None
        assert callable(getattr(ops, name[4:]))
        end = hdr.index("int " + name + "(")
        assert "evaluation_control_to_video.py:" in hdr[hdr.rindex("/*", 0, end):end], name       # cites the reference lines it replaces
    assert "section 19" in hdr[hdr.index("Cascaded rollouts"):hdr.index("int orv_frames_quantize(")]
    with open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile"), "r", encoding="utf-8") as f:
        assert "frames.hip" in f.read()


def test_frames_entry_points_validate_before_any_launch():
    """Null pointers, sizes, frame ranges, strides and extents: nonzero with the reason in orv_last_error(), prefixed by the entry point's
    name, without a GPU (no device pointer is followed)."""
    from orv_amd._lib import lib
    h = lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lambda: h.orv_last_error().decode()

    def quant(src=p, sb=2, extent=2 * 3 * 4 * 8 * 16, strides=(1536, 512, 128, 16, 1), B=2, H=8, W=16, f0=0, f1=4, dst=p, dext=2 * 4 * 384, dsb=4 * 384,
              dsf=384, d0=0):
        return h.orv_frames_quantize(src, sb, extent, None if strides is None else (ctypes.c_long * 5)(*strides), B, H, W, f0, f1, dst, dext, dsb, dsf, d0, None)

    def hand(src=p, extent=2 * 4 * 384, strides=(4 * 384, 384, 48, 3, 1), B=2, F=4, H=8, W=16, frame=1, table=p, out=p):
        return h.orv_frames_handoff(src, extent, None if strides is None else (ctypes.c_long * 5)(*strides), B, F, H, W, frame, table, out, None)

    q, n = NAMES
    for sb in (0, 1, 3, 8):
        assert quant(sb=sb) != 0 and f"src_bytes = {sb}" in err() and err().startswith(q + ":")
    for bad in (dict(src=None), dict(dst=None), dict(strides=None)):
        assert quant(**bad) != 0 and "null pointer" in err() and err().startswith(q + ":"), bad
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(W=(1 << 20) + 1)):
        assert quant(**bad) != 0 and "supported: 1 to" in err() and err().startswith(q + ":"), bad
    for bad in (dict(f0=-1), dict(f0=3, f1=2), dict(d0=-1)):
        assert quant(**bad) != 0 and "0 <= f0 <= f1" in err(), bad
    for bad in (dict(strides=(1536, 512, 128, 16, -1)), dict(strides=(1 << 40, 512, 128, 16, 1))):
        assert quant(**bad) != 0 and "[0, 2^40) elements" in err(), bad
    assert quant(src=p + 1) != 0 and "aligned to its element size" in err()
    for bad in (dict(dsf=383), dict(dsb=3 * 384), dict(dsb=-1)):
        assert quant(**bad) != 0 and "destination strides" in err() and "do not overlap" in err(), bad
    assert quant(f1=5) != 0 and "last source element read" in err()              # one frame beyond the source
    assert quant(extent=2 * 3 * 4 * 8 * 16 - 1) != 0 and "last source element read is 3071 and the buffer holds 3071" in err()
    assert quant(d0=1) != 0 and "last byte written" in err()                     # one frame beyond the destination
    assert quant(dext=2 * 4 * 384 - 1) != 0 and "last byte written is 3071 and the destination holds 3071" in err()
    assert quant(f0=2, f1=2, d0=1 << 19) == 0                                    # an empty range launches nothing

    for bad in (dict(src=None), dict(table=None), dict(out=None), dict(strides=None)):
        assert hand(**bad) != 0 and "null pointer" in err() and err().startswith(n + ":"), bad
    for bad in (dict(B=0), dict(F=0), dict(H=-2), dict(W=0)):
        assert hand(**bad) != 0 and "supported: 1 to" in err() and err().startswith(n + ":"), bad
    for frame in (-1, 4):
        assert hand(frame=frame) != 0 and f"frame = {frame}" in err() and "0 to F - 1 = 3" in err()
    assert hand(strides=(4 * 384, 384, 48, -3, 1)) != 0 and "[0, 2^40) bytes" in err()
    assert hand(out=p + 8) != 0 and "16-byte aligned" in err()
    assert hand(extent=2 * 4 * 384 - 1, frame=3) != 0 and "last source byte read is 3071 and the buffer holds 3071" in err()
