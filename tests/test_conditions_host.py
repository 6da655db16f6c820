"""Host: control encoding (orv_amd.conditions) without a GPU - the plan arithmetic, the palette, every refusal, and the
numpy restatement (tests/conditions_ref.py) against the torch CPU operator chain the reference's torchvision transforms come down to:
two ``F.interpolate(..., antialias=True)`` calls and two crops, clamp and scale (``mode="nearest"`` for labels).  The fp64 run of that
chain is the oracle; its fp32 run is the yardstick: the restatement may miss the oracle by at most twice what the yardstick misses it
by, plus 2^-22 (both are fp32 evaluations of one formula whose error is dominated by the fp32 sample coordinate and grows with the
image, so a fixed absolute bound would be wrong; the floor covers shapes where both errors are about one ulp)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conditions_ref as ref
from orv_amd import conditions as cond
from orv_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = dict(ori_size=(256, 320), video_size=(320, 480), source_size=(320, 480), render_size=(480, 640))
SMALL = dict(ori_size=(26, 32), video_size=(32, 48), source_size=(32, 48), render_size=(48, 64))


def stage_ints(plan):
    return [s.ints() for s in plan.stages]


def torch_chain(x, stages, mode):
    """x [N, C, h, w] -> the reference's transform chain on torch CPU operators, in x's dtype."""
    for rh, rw, top, left, ch, cw in stages:
        kw = dict(mode="bilinear", align_corners=False, antialias=True) if mode == "bilinear" else dict(mode="nearest")
        x = F.interpolate(x, size=(rh, rw), **kw)[..., top:top + ch, left:left + cw]
    return x


def torch_depth(x, stages):
    return torch.clamp(torch_chain(x, stages, "bilinear"), min=0.01, max=0.4) * 2.5


# ---- plan arithmetic ----
def test_plan_of_the_real_geometry():
    assert cond.ResizePlan.new_size((256, 320), (320, 480)) == (384, 480)
    plan = cond.ResizePlan.for_controls(**REAL)
    s1, s2 = plan.stages
    assert (s1.in_size, s1.resize, s1.crop, s1.top, s1.left) == ((320, 480), (480, 720), (480, 640), 0, 40)
    assert (s2.in_size, s2.resize, s2.crop, s2.top, s2.left) == ((480, 640), (384, 480), (320, 480), 32, 0)
    assert plan.out_size == (320, 480)
    assert stage_ints(plan) == [(480, 720, 0, 40, 480, 640), (384, 480, 32, 0, 320, 480)]


def test_plan_of_the_small_geometry_rounds_half_to_even():
    assert cond.ResizePlan.new_size((26, 32), (32, 48)) == (39, 48)
    plan = cond.ResizePlan.for_controls(**SMALL)
    s1, s2 = plan.stages
    assert (s1.resize, s1.crop, s1.top, s1.left) == ((48, 72), (48, 64), 0, 4)
    assert (s2.resize, s2.crop, s2.top, s2.left) == ((39, 48), (32, 48), 4, 0)          # (39 - 32) / 2 = 3.5 -> 4


def test_a_crop_difference_of_five_gives_offset_two():
    plan = cond.ResizePlan((20, 30), [((21, 29), (16, 24))])
    assert (plan.stages[0].top, plan.stages[0].left) == (2, 2)                            # 2.5 -> 2


def test_render_size_defaults_to_ori_size_and_frames_use_stage_two_alone():
    plan = cond.ResizePlan.for_controls((256, 320), (320, 480), (320, 480))
    assert plan.stages[0].resize == (256, 384) and plan.stages[0].crop == (256, 320) and plan.stages[0].left == 32
    frames = cond.ResizePlan.for_frames((256, 320), (320, 480))
    assert len(frames.stages) == 1 and stage_ints(frames) == [(384, 480, 32, 0, 320, 480)]
    tall = cond.ResizePlan.for_controls((320, 256), (480, 320), (480, 320))             # portrait source: the shorter edge is the width
    assert tall.stages[0].resize == (int(320 * 480 / 320), 320)


def test_new_size_takes_the_other_branch_for_a_narrow_target():
    assert cond.ResizePlan.new_size((256, 320), (256, 256)) == (256, int(320 * (256 / 256)))


# ---- palette ----
def test_palette_entries():
    colors = cond.generate_colors(60)
    assert len(colors) == 60 and colors[0] == (242, 60, 60) and colors[1] == (242, 78, 60) and colors[59] == (242, 60, 78)
    pal = cond.palette60()
    assert pal.shape == (60, 3) and pal.dtype == np.float32
    assert tuple(pal[0]) == (242, 60, 60) and tuple(pal[58]) == colors[58] and tuple(pal[59]) == (0, 0, 0)
    assert np.array_equal(pal, ref.palette60())


# ---- refusals ----
def test_plan_refusals():
    with pytest.raises(ValueError, match="multiples of 8"):
        cond.ResizePlan.for_controls((256, 320), (320, 481), (320, 480))
    with pytest.raises(ValueError, match="multiples of 8"):
        cond.ResizePlan.for_frames((256, 320), (324, 480))
    with pytest.raises(ValueError, match="no larger than its input"):
        cond.ResizePlan((32, 48), [((32, 48), (33, 48))])
    with pytest.raises(ValueError, match="no larger than its input"):                     # stage 1 of a plan whose render_size is too wide
        cond.ResizePlan.for_controls((26, 32), (32, 48), (32, 40), render_size=(48, 64))
    with pytest.raises(ValueError, match="at most 4x"):
        cond.ResizePlan((41, 48), [((10, 48), (10, 48))])
    cond.ResizePlan((40, 48), [((10, 12), (10, 12))])                                     # exactly 4x is supported
    with pytest.raises(ValueError, match="1 or 2 stages"):
        cond.ResizePlan((8, 8), [])


def test_tensor_refusals_name_the_supported_set():
    plan = cond.ResizePlan.for_controls(**SMALL)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        cond.prepare_depths(torch.zeros(2, 32, 48), plan)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.cond_prepare(torch.zeros(2, 32, 48), stage_ints(plan), "bilinear", "depth")
    with pytest.raises(RuntimeError, match=r"torch.float32 \[N,h,w\], torch.uint8"):
        cond.prepare_depths(torch.zeros(2, 32, 48, dtype=torch.float64), plan)
    with pytest.raises(RuntimeError, match=r"torch.float32 \[N,h,w\], torch.uint8"):
        ops.cond_prepare(torch.zeros(2, 32, 48, dtype=torch.int64), stage_ints(plan), "nearest")
    with pytest.raises(RuntimeError, match="requires grad"):
        cond.prepare_depths(torch.zeros(2, 32, 48, requires_grad=True), plan)
    with pytest.raises(ValueError, match="must be contiguous"):
        cond.prepare_depths(torch.zeros(2, 48, 32).transpose(1, 2), plan)
    with pytest.raises(ValueError, match="the plan starts from"):
        cond.prepare_depths(torch.zeros(2, 30, 48), plan)
    with pytest.raises(ValueError, match="'nchw'"):
        cond.prepare_depths(torch.zeros(2, 32, 48), plan, out="nhwc")
    with pytest.raises(ValueError, match="`palette` goes with uint8 label ids"):
        ops.cond_prepare(torch.zeros(2, 32, 48, dtype=torch.uint8), stage_ints(plan), "nearest")
    with pytest.raises(IndexError, match="label id 60 is outside the palette; supported: ids 0 to 59"):
        cond.prepare_labels(np.full((1, 32, 48), 60, dtype=np.uint8), plan)


def test_encode_controls_refuses_bad_ids_and_sizes_before_touching_the_device():
    render = {"semantics": np.zeros((3, 2, 32, 48), np.uint8), "depths": np.zeros((6, 32, 48), np.float32), "is_labeled": True}
    kw = dict(ori_size=(26, 32), video_size=(32, 48), render_size=(48, 64))
    with pytest.raises(IndexError, match="frame_ids.*0 to 2"):
        cond.encode_controls(None, render, [0, 3], **kw)
    with pytest.raises(IndexError, match="frame_ids.*0 to 2"):
        cond.encode_controls(None, render, [-1], **kw)
    with pytest.raises(IndexError, match="view_ids.*0 to 1"):
        cond.encode_controls(None, render, [0, 1], view_ids=(0, 2), **kw)
    with pytest.raises(ValueError, match="multiples of 8"):
        cond.encode_controls(None, render, [0, 1], ori_size=(26, 32), video_size=(30, 48))
    with pytest.raises(ValueError, match="supported: 'depth', 'label'"):
        cond.encode_controls(None, render, [0, 1], control_keys=("depth", "normal"), **kw)


def test_header_and_binding_declare_the_entry_point():
    from orv_amd import _lib
    header = open(os.path.join(ROOT, "include", "orv_mi355.h")).read()
    assert "int orv_cond_prepare(" in header and "ORV_COND_OUT_VAE" in header
    assert "orv_cond_prepare" in _lib.SIGNATURES and len(_lib.SIGNATURES["orv_cond_prepare"][1]) == 16
    assert "conditions.hip" in open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile")).read()


# ---- the restatement against torch on the CPU ----
def _depth_input(shape, seed):
    g = np.random.default_rng(seed)
    x = g.uniform(0.0, 0.5, size=shape).astype(np.float32)                                # below 0.01 and above 0.4 both occur
    x[..., ::7, ::5] = 0.001
    return x


GEOMETRIES = {
    "real": (cond.ResizePlan.for_controls(**REAL), 1),
    "small": (cond.ResizePlan.for_controls(**SMALL), 3),
    "identity": (cond.ResizePlan((10, 15), [((10, 15), (10, 15))]), 3),
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_restatement_meets_the_fp64_chain(name):
    plan, n = GEOMETRIES[name]
    stages = stage_ints(plan)
    x = _depth_input((n,) + plan.source_size, seed=len(name))
    oracle = torch_depth(torch.from_numpy(x).double()[:, None], stages).numpy()
    yard = torch_depth(torch.from_numpy(x)[:, None], stages).numpy()
    got64 = ref.depths(x, stages, dt=np.float64)
    got32 = ref.depths(x, stages)
    assert got32.dtype == np.float32 and got32.shape == oracle.shape == (n, 1) + plan.out_size
    e64 = np.abs(got64 - oracle).max()
    e32 = np.abs(got32.astype(np.float64) - oracle).max()
    ey = np.abs(yard.astype(np.float64) - oracle).max()
    print(f"{name}: fp64 restatement {e64:.3e}, fp32 restatement {e32:.3e}, fp32 torch chain {ey:.3e}")
    assert e64 <= 1e-12
    assert e32 <= 2 * ey + 2.0 ** -22


@pytest.mark.parametrize("n,o", [(10, 16), (16, 10), (39, 10), (15, 15), (48, 72)])
def test_unscaled_resize_restatement_in_fp64(n, o):
    """the resize alone (no clamp), upscaling, downscaling, 3.9x and the identity: fp64 restatement == fp64 F.interpolate to 1e-12"""
    x = np.random.default_rng(n * 100 + o).standard_normal((2, n + 1, n)).astype(np.float32)
    want = F.interpolate(torch.from_numpy(x).double()[:, None], size=(o + 2, o), mode="bilinear", align_corners=False, antialias=True)[:, 0]
    got = ref.resize_bilinear(x, o + 2, o, dt=np.float64)
    assert np.abs(got - want.numpy()).max() <= 1e-12


def test_nearest_resize_and_palette_are_bit_equal_to_torch():
    for n in range(1, 70, 3):
        for o in range(1, 70):
            want = F.interpolate(torch.arange(n, dtype=torch.float32).view(1, 1, 1, n), size=(1, o), mode="nearest").view(-1).long().numpy()
            assert np.array_equal(ref.nearest_index(n, o), want), (n, o)
    plan = cond.ResizePlan.for_controls(**SMALL)
    stages = stage_ints(plan)
    ids = np.random.default_rng(3).integers(0, 60, size=(3, 32, 48)).astype(np.uint8)
    ids[0, 0, :3] = (0, 58, 59)
    # the reference paints first and resizes the colours, nearest, then the encoder side divides nothing: labels are palette / 255
    painted = torch.from_numpy(ref.palette60())[torch.from_numpy(ids).long()].permute(0, 3, 1, 2) / 255.0
    want = torch_chain(painted, stages, "nearest").numpy()
    assert np.array_equal(ref.labels(ids, stages), want)


def test_frames_restatement_meets_the_fp64_chain():
    plan = cond.ResizePlan.for_frames((26, 32), (32, 48))
    stages = stage_ints(plan)
    x = np.random.default_rng(9).integers(0, 256, size=(2, 26, 32, 3)).astype(np.uint8)

    def chain(t):
        return (torch_chain(t.permute(0, 3, 1, 2) / 255.0, stages, "bilinear") - 0.5) / 0.5

    oracle, yard = chain(torch.from_numpy(x).double()).numpy(), chain(torch.from_numpy(x).float()).numpy()
    e64 = np.abs(ref.frames(x, stages, dt=np.float64) - oracle).max()
    e32 = np.abs(ref.frames(x, stages).astype(np.float64) - oracle).max()
    ey = np.abs(yard.astype(np.float64) - oracle).max()
    assert e64 <= 1e-12
    assert e32 <= 2 * ey + 2.0 ** -21                                                     # the floor doubled by the (x - 0.5) / 0.5 post-scale
