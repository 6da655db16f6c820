"""GPU: control encoding (orv_amd.conditions, csrc/conditions.hip).
* the kernel against the numpy restatement (tests/conditions_ref.py), bit for bit: the contract fixes every rounding, so nothing but
  equality is accepted, and two runs of a case must agree;
* the bf16 channels-last form against ``AutoencoderKLCogVideoX._channels_last`` of the fp32 form, bit for bit;
* ``encode_controls`` end to end on the tiny random-weight VAE of tests/test_gpu_vae.py, and through the pipeline;
* the kernel against the fp64 torch chain with the bound of tests/test_conditions_host.py (PARITY UNPINNED beyond that chain: torchvision
  is absent, so that its ``Resize`` adds nothing to ``F.interpolate(antialias=True)`` is not checked here)."""
import numpy as np
import pytest
import torch

import conditions_ref as ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
SMALL = dict(ori_size=(26, 32), video_size=(32, 48), source_size=(32, 48), render_size=(48, 64))
TINY = dict(ori_size=(8, 10), video_size=(16, 24), source_size=(10, 15), render_size=(16, 20))
INDEX = [2, 0, 2, 1]                                      # permuted, frame 2 twice


def cond():
    from orv_amd import conditions
    return conditions


def plans():
    c = cond()
    return {
        "small": c.ResizePlan.for_controls(**SMALL),
        "tiny": c.ResizePlan.for_controls(**TINY),
        "identity": c.ResizePlan((10, 15), [((10, 15), (10, 15))]),
        "down3.9": c.ResizePlan((39, 78), [((10, 20), (10, 20))]),
        # 3.9x down in the SECOND stage over 3 x 3 tiles: the largest LDS block a tile may need (68 of 72 per axis)
        "up_then_down3.9": c.ResizePlan((40, 48), [((156, 187), (156, 184)), ((40, 48), (40, 48))]),
        "frames_small": c.ResizePlan.for_frames((26, 32), (32, 48)),
        "frames_tiny": c.ResizePlan.for_frames((8, 10), (16, 24)),
    }


def ints(plan):
    return [s.ints() for s in plan.stages]


def depth_input(plan, n=3, seed=0):
    x = np.random.default_rng(seed).uniform(-0.05, 0.5, size=(n,) + plan.source_size).astype(np.float32)
    x[:, ::3, ::4] = 0.001                               # below 0.01; the draw also goes above 0.4
    x[:, 1::5, 1::3] = 0.7
    return x


def label_input(plan, n=3, seed=1):
    ids = np.random.default_rng(seed).integers(0, 60, size=(n,) + plan.source_size).astype(np.uint8)
    ids[:, 0, :3] = (0, 58, 59)
    ids[:, -1, -3:] = (59, 0, 58)
    return ids


def frame_input(plan, n=3, seed=2):
    return np.random.default_rng(seed).integers(0, 256, size=(n,) + plan.source_size + (3,)).astype(np.uint8)


def twice(fn):
    a, b = fn(), fn()
    assert torch.equal(a, b), "two runs of the same case differ"
    return a


@pytest.mark.parametrize("name", ["small", "tiny", "identity", "down3.9", "up_then_down3.9"])
def test_depth_equals_the_restatement_bit_for_bit(name):
    c, plan = cond(), plans()[name]
    x = depth_input(plan)
    assert (x < 0.01).any() and (x > 0.4).any()
    got = twice(lambda: c.prepare_depths(x, plan, INDEX))
    want = ref.depths(x, ints(plan), INDEX)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (4, 1) + plan.out_size
    assert np.array_equal(got.cpu().numpy(), want)
    # a device tensor and no index: all frames in order
    assert np.array_equal(c.prepare_depths(torch.from_numpy(x).to(DEV), plan).cpu().numpy(), ref.depths(x, ints(plan)))


@pytest.mark.parametrize("name", ["small", "tiny", "identity", "down3.9"])
def test_labels_equal_the_restatement_bit_for_bit(name):
    c, plan = cond(), plans()[name]
    ids = label_input(plan)
    got = twice(lambda: c.prepare_labels(ids, plan, INDEX))
    want = ref.labels(ids, ints(plan), INDEX)
    assert tuple(got.shape) == want.shape == (4, 3) + plan.out_size
    assert np.array_equal(got.cpu().numpy(), want)
    black = (want == 0).all(axis=1)
    assert black.any() and not black.all()               # id 59 is painted black, and not everything is


@pytest.mark.parametrize("name,normalize", [("frames_small", True), ("frames_tiny", True), ("frames_tiny", False), ("small", True),
                                            ("identity", True), ("down3.9", False), ("up_then_down3.9", True)])
def test_frames_equal_the_restatement_bit_for_bit(name, normalize):
    c, plan = cond(), plans()[name]
    x = frame_input(plan)
    got = twice(lambda: c.prepare_frames(x, plan, INDEX, normalize=normalize))
    want = ref.frames(x, ints(plan), INDEX, normalize=normalize)
    assert tuple(got.shape) == want.shape == (4, 3) + plan.out_size
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", ["small", "tiny"])
def test_vae_form_is_channels_last_of_the_nchw_form(name):
    from orv_amd.vae import AutoencoderKLCogVideoX
    c, plan = cond(), plans()[name]
    index = [[2, 0, 1], [1, 2, 2]]                       # V = 2, F = 3
    H, W = plan.out_size
    for fn, x, rep in ((c.prepare_depths, depth_input(plan), 3), (c.prepare_labels, label_input(plan), 1),
                       (c.prepare_frames, frame_input(plan), 1)):
        got = twice(lambda: fn(x, plan, index, out="vae"))
        nchw = fn(x, plan, index)                                                       # [V * F, C, H, W], (v f) order
        assert got.dtype == BF and tuple(got.shape) == (2, 3, H, W, 8)
        x5 = nchw.view(2, 3, -1, H, W).repeat(1, 1, rep, 1, 1).permute(0, 2, 1, 3, 4)   # [V, 3, F, H, W]
        assert torch.equal(got, AutoencoderKLCogVideoX._channels_last(x5, cpad=5))
        assert not got[..., 3:].any() and got[..., :3].any()
    one = c.prepare_depths(depth_input(plan), plan, [1, 0], out="vae")                  # a flat index is one view
    assert tuple(one.shape) == (1, 2, H, W, 8)


def test_device_side_refusals():
    c, plan = cond(), plans()["small"]
    with pytest.raises(IndexError, match="label id 60 is outside the palette; supported: ids 0 to 59"):
        c.prepare_labels(torch.full((1, 32, 48), 60, dtype=torch.uint8, device=DEV), plan)
    with pytest.raises(IndexError, match="supported: 0 to 2"):
        c.prepare_depths(torch.zeros(3, 32, 48, device=DEV), plan, [0, 3])
    with pytest.raises(IndexError, match="supported: 0 to 2"):
        c.prepare_depths(torch.zeros(3, 32, 48, device=DEV), plan, torch.tensor([-1, 0], device=DEV))
    with pytest.raises(RuntimeError, match="torch.uint8"):
        c.prepare_labels(torch.zeros(1, 32, 48, dtype=torch.int64, device=DEV), plan)
    with pytest.raises(RuntimeError, match=r"torch.uint8 \[N, h, w, 3\]"):
        c.prepare_frames(torch.zeros(1, 32, 48, 3, device=DEV), plan)
    with pytest.raises(ValueError, match="must be contiguous"):
        c.prepare_depths(torch.zeros(3, 48, 32, device=DEV).transpose(1, 2), plan)


def test_depth_meets_the_fp64_chain_like_the_restatement_does():
    import torch.nn.functional as F
    c, plan = cond(), plans()["small"]
    x = depth_input(plan)

    def chain(t):
        for rh, rw, top, left, ch, cw in ints(plan):
            t = F.interpolate(t, size=(rh, rw), mode="bilinear", align_corners=False, antialias=True)[..., top:top + ch, left:left + cw]
        return torch.clamp(t, min=0.01, max=0.4) * 2.5

    oracle = chain(torch.from_numpy(x).double()[:, None])
    yard = chain(torch.from_numpy(x)[:, None])
    got = c.prepare_depths(x, plan).cpu()
    e, ey = (got.double() - oracle).abs().max().item(), (yard.double() - oracle).abs().max().item()
    print(f"kernel vs fp64 chain {e:.3e}, fp32 torch chain vs fp64 chain {ey:.3e}")
    assert e <= 2 * ey + 2.5 * 2.0 ** -22


# ---- end to end on the tiny random-weight VAE ----
@pytest.fixture(scope="module")
def tiny_vae():
    import test_gpu_vae as tv
    return tv.make(tv.TINY, seed=5)[1]


def synthetic_render(n_frame=5, n_view=2, size=(32, 48), labeled=True, seed=4):
    g = np.random.default_rng(seed)
    depths = g.uniform(0.0, 0.5, size=(n_frame, n_view) + size).astype(np.float32)
    depths[:, 1:] *= 0.5                                 # the views differ
    sem = g.integers(0, 60, size=(n_frame, n_view) + size).astype(np.uint8)
    return {"semantics": sem, "depths": depths.reshape(n_frame * n_view, *size), "is_labeled": labeled}


def test_encode_refactor_keeps_encode(tiny_vae):
    x = (torch.rand(2, 3, 5, 32, 48, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV, BF)
    want = tiny_vae.encode(x).latent_dist.parameters
    got = tiny_vae.encode_channels_last(tiny_vae._channels_last(x, 5))
    assert got.dtype == BF and tuple(got.shape) == (2, 32, 2, 4, 6) and torch.equal(got, want)
    x32 = x.float()
    assert torch.equal(tiny_vae.encode(x32).latent_dist.parameters, tiny_vae.encode_channels_last(tiny_vae._channels_last(x32, 5), dtype=torch.float32))
    with pytest.raises(RuntimeError, match=r"bf16 \[B, F, H, W, 8\]"):
        tiny_vae.encode_channels_last(x)


def test_encode_controls_equals_encode_of_the_assembled_tensor(tiny_vae):
    c = cond()
    render = synthetic_render()
    kw = dict(ori_size=SMALL["ori_size"], video_size=SMALL["video_size"], render_size=SMALL["render_size"])
    frame_ids, view_ids = [0, 1, 2, 3, 4], (0, 1)
    got = c.encode_controls(tiny_vae, render, frame_ids, view_ids, **kw)
    assert sorted(got) == ["depths", "labels"]
    plan = c.ResizePlan.for_controls(source_size=(32, 48), **kw)
    index = [[f * 2 + v for f in frame_ids] for v in view_ids]
    d = c.prepare_depths(render["depths"], plan, index).view(2, 5, 1, 32, 48).repeat(1, 1, 3, 1, 1).permute(0, 2, 1, 3, 4)
    l = c.prepare_labels(render["semantics"].reshape(10, 32, 48), plan, index).view(2, 5, 3, 32, 48).permute(0, 2, 1, 3, 4)
    for key, x in (("depths", d), ("labels", l)):
        m = tiny_vae.encode(x).latent_dist.parameters                                   # [V, 32, F', 4, 6], fp32 like x
        want = torch.cat([m[v] for v in range(2)], dim=1)[None]                         # views joined along frames, view 0 first
        assert got[key].dtype == BF and tuple(got[key].shape) == (1, 32, 2 * 2, 4, 6)
        assert torch.equal(got[key].float(), want)
    assert not torch.equal(got["depths"][:, :, :2], got["depths"][:, :, 2:])            # the two views differ, and view 0 comes first:
    first = c.encode_controls(tiny_vae, render, frame_ids, (0,), control_keys=("depth",), **kw)
    second = c.encode_controls(tiny_vae, render, frame_ids, (1,), control_keys=("depth",), **kw)
    assert sorted(first) == ["depths"] and tuple(first["depths"].shape) == (1, 32, 2, 4, 6)
    d0 = (got["depths"][:, :, :2].float() - first["depths"].float()).norm()
    d1 = (got["depths"][:, :, :2].float() - second["depths"].float()).norm()
    assert d0 < 0.1 * d1
    # is_labeled false: no labels, as in the reference
    unlabeled = c.encode_controls(tiny_vae, synthetic_render(labeled=np.bool_(False)), frame_ids, view_ids, **kw)
    assert sorted(unlabeled) == ["depths"] and torch.equal(unlabeled["depths"], got["depths"])
    # fp32 on request
    assert c.encode_controls(tiny_vae, render, [0], (1,), dtype=torch.float32, **kw)["labels"].dtype == torch.float32


def test_encode_frames_on_the_tiny_vae(tiny_vae):
    c = cond()
    x = np.random.default_rng(6).integers(0, 256, size=(2 * 5, 26, 32, 3)).astype(np.uint8)          # 2 views of 5 frames
    got = c.encode_frames(tiny_vae, x, video_size=(32, 48), n_view=2)
    plan = c.ResizePlan.for_frames((26, 32), (32, 48))
    f = c.prepare_frames(x, plan).view(2, 5, 3, 32, 48).permute(0, 2, 1, 3, 4)
    m = tiny_vae.encode(f).latent_dist.parameters
    assert tuple(got.shape) == (1, 32, 4, 4, 6) and torch.equal(got.float(), torch.cat([m[0], m[1]], dim=1)[None])


def test_pipeline_takes_encode_controls_like_loaded_moments(tiny_vae, tmp_path):
    from conftest import load_golden
    from orv_amd import schedulers
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj, CogVideoXTransformer3DModelTraj
    from orv_amd.data import load_latent_controls
    c = cond()
    cfg, _, ins, _, _ = load_golden("pipe_ddim")
    torch.manual_seed(21)
    m = CogVideoXTransformer3DModelTraj(**{**cfg, "visual_guidance": True, "num_control_keys": 2})
    for p in m.parameters():
        if p.ndim >= 2:
            p.data.normal_(0, 0.02)                      # the reference zero-initialises the guidance fuse: given weights so it counts
    m = m.to(DEV, BF).eval()
    m.action_embed.forced_mask = torch.zeros(1, dtype=torch.bool)
    render = synthetic_render(n_frame=9, n_view=1, size=(40, 60), seed=8)
    controls = c.encode_controls(tiny_vae, render, list(range(9)), ori_size=(48, 64), video_size=(64, 96))
    assert tuple(controls["depths"].shape) == tuple(controls["labels"].shape) == (1, 32, 3, 8, 12)
    # the load_latent_controls way: one [2C, F', h, w] file per key and view, read back and batched as the collate function does
    for key in ("depths", "labels"):
        torch.save(controls[key][0].cpu(), str(tmp_path / f"{key}.pt"))
    loaded = load_latent_controls(str(tmp_path), ("depth", "label"), ["depths.pt"], ["labels.pt"])
    assert torch.equal(loaded["latents_depth"], controls["depths"][0].permute(1, 0, 2, 3).cpu())
    loaded = {"depths": loaded["latents_depth"][None].permute(0, 2, 1, 3, 4).to(DEV), "labels": loaded["latents_label"][None].permute(0, 2, 1, 3, 4).to(DEV)}
    g = torch.Generator().manual_seed(11)
    image_lat = torch.randn(1, 16, 1, 8, 12, generator=g).to(DEV, BF)
    lat0 = torch.randn(1, 3, 16, 8, 12, generator=g).to(DEV, BF)
    res = []
    for ctrl in (controls, loaded, {"depths": loaded["depths"], "labels": -loaded["labels"]}):
        torch.manual_seed(1234)                          # the pipeline samples the control latents from the global generator
        sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                                  prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=3.0,
                                                  timestep_spacing="trailing")
        pipe = CogVideoXImageToVideoPipelineTraj(transformer=m, scheduler=sched)
        out = pipe(image=image_lat, height=64, width=96, num_frames=9, num_inference_steps=2, guidance_scale=1.0, latents=lat0.clone(),
                   prompt_embeds=ins["prompt_embeds"][:1].to(DEV, BF), output_type="latent",
                   controls_or_guidances={"actions": ins["actions"][:1].to(DEV), **ctrl})
        res.append(out.frames.clone())
    assert torch.isfinite(res[0].float()).all() and torch.equal(res[0], res[1])
    assert not torch.equal(res[0], res[2])               # the controls reach the latents
