"""Cascaded rollouts on the MI355X: the two chunk-boundary kernels bit for bit against their numpy restatement (tests/rollout_ref.py) and
against ``VideoProcessor.preprocess``, and ``pipe.rollout`` bit for bit in uint8 against the loop written by hand from the public pieces
(``pipe(..., output_type='pil')``, ``videos[0][index]`` as the next ``image=[...]``, the reference's stitch).

Reproducibility of the by-hand loop itself at this shape, measured here before anything is held to it: two runs gave 0 differing bytes."""
import numpy as np
import pytest
import torch

import rollout_ref as ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
SIZES = ((8, 16), (5, 13), (16, 24))          # all vector groups; rows off 16-byte boundaries and a W % 8 tail; W * 3 not a multiple of 16


def ops():
    from orv_amd import ops
    return ops


def _video(B, F, H, W, dtype, seed):
    x = torch.randn(B, 3, F, H, W, generator=torch.Generator().manual_seed(seed)) * 0.9        # a good part beyond [-1, 1]
    return x.to(dtype).to(DEV)


def _want(video):
    return ref.quantize_frames_ref(video.float().cpu().numpy())


# ---- quantize ----
@pytest.mark.parametrize("dtype", (BF, torch.float32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantize_equals_the_restatement(dtype, size):
    video = _video(2, 3, *size, dtype, 3)
    out = ops().frames_quantize(video)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 3, *size, 3) and out.is_contiguous()
    assert np.array_equal(out.cpu().numpy(), _want(video))
    part = ops().frames_quantize(video, 1, 2)
    assert np.array_equal(part.cpu().numpy(), _want(video)[:, 1:2])


@pytest.mark.parametrize("dtype", (BF, torch.float32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantize_reads_strided_sources(dtype, size):
    base = _video(3, 4, *size, dtype, 4)
    view = base[::2][:, :, 1:]                                                   # a non-contiguous batch and a frame slice
    assert not view.is_contiguous() and tuple(view.shape) == (2, 3, 3, *size)
    assert np.array_equal(ops().frames_quantize(view).cpu().numpy(), _want(view))
    wide = _video(2, 3, size[0], size[1] + 3, dtype, 5)[..., 3:]                 # a width slice: rows that start off their alignment
    assert np.array_equal(ops().frames_quantize(wide).cpu().numpy(), _want(wide))
    flipped = _video(2, 3, size[1], size[0], dtype, 6).transpose(3, 4)           # x is not the unit stride: every pixel on the scalar path
    assert np.array_equal(ops().frames_quantize(flipped).cpu().numpy(), _want(flipped))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantize_writes_its_range_and_nothing_else(size):
    video = _video(2, 3, *size, BF, 7)
    want = _want(video)
    out = torch.full((2, 7, *size, 3), 0xA5, dtype=torch.uint8, device=DEV)
    assert ops().frames_quantize(video, 1, 3, out=out, dst_f0=2) is out
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 2:4], want[:, 1:3])
    assert (got[:, :2] == 0xA5).all() and (got[:, 4:] == 0xA5).all()
    big = torch.full((5, 9, *size, 3), 0x5A, dtype=torch.uint8, device=DEV)      # a destination with strides of its own
    ops().frames_quantize(video, 0, 3, out=big[1:4:2, 2:8], dst_f0=3)
    got = big.cpu().numpy()
    assert np.array_equal(got[1:4:2, 5:8], want)
    got[1:4:2, 5:8] = 0x5A
    assert (got == 0x5A).all()
    with pytest.raises(ValueError, match="frame offset"):
        ops().frames_quantize(video, 0, 3, out=out, dst_f0=5)


def test_quantize_value_sweep():
    video = ref.sweep_video()                                                    # every bf16 value in [-1.5, 1.5], the half-way cases, +-inf, a NaN
    want = ref.quantize_frames_ref(video)
    assert np.array_equal(ops().frames_quantize(torch.from_numpy(video).to(DEV)).cpu().numpy(), want)
    as_bf = torch.from_numpy(video).to(BF)
    assert np.array_equal(ops().frames_quantize(as_bf.to(DEV)).cpu().numpy(), ref.quantize_frames_ref(as_bf.float().numpy()))
    x, k = ref.halfway_inputs()
    lone = torch.zeros(1, 3, 1, 1, x.size)
    lone[0, 1, 0, 0] = torch.from_numpy(x)
    assert np.array_equal(ops().frames_quantize(lone.to(DEV)).cpu().numpy()[0, 0, 0, :, 1], k + (k % 2))     # half to even


# ---- hand-off ----
def _processor():
    from orv_amd.components import VideoProcessor
    return VideoProcessor(vae_latent_channels=16, vae_scale_factor=8)


def _table():
    from orv_amd import rollout
    return rollout.handoff_table().to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_handoff_equals_the_restatement_at_any_index_and_strides(size):
    g = torch.Generator().manual_seed(8)
    frames = torch.randint(0, 256, (3, 5, size[0], size[1] + 2, 3), dtype=torch.uint8, generator=g)
    view = frames[::2, :, :, 1:-1]                                               # a non-contiguous batch and a width slice
    for index in (0, 3, 4):
        out = ops().frames_handoff(view.to(DEV)[:], index, _table())
        assert out.dtype == BF and tuple(out.shape) == (2, 1, *size, 8) and out.is_contiguous()
        assert np.array_equal(_bits(out), ref.handoff_ref(view.numpy(), index))
        strided = frames.to(DEV)[::2, :, :, 1:-1]
        assert not strided.is_contiguous() and np.array_equal(_bits(ops().frames_handoff(strided, index, _table())), ref.handoff_ref(view.numpy(), index))
    channels_first = frames.to(DEV).permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)   # the channel stride is not 1
    assert np.array_equal(_bits(ops().frames_handoff(channels_first, 2, _table())), ref.handoff_ref(frames.numpy(), 2))
    with pytest.raises(ValueError, match="frame 5 of clips of 5"):
        ops().frames_handoff(frames.to(DEV), 5, _table())


@pytest.mark.parametrize("size", ((8, 16), (16, 24)), ids=lambda s: f"{s[0]}x{s[1]}")      # preprocess rounds a size down to a multiple of 8
def test_handoff_equals_preprocess_of_the_pil_frame(size):
    import PIL.Image
    from orv_amd.vae import AutoencoderKLCogVideoX
    g = torch.Generator().manual_seed(9)
    frames = torch.randint(128, 256, (2, 4, *size, 3), dtype=torch.uint8, generator=g)         # no value below 128: the double-normalise trap
    out = ops().frames_handoff(frames.to(DEV), 2, _table())
    for b in range(2):
        pre = _processor().preprocess([PIL.Image.fromarray(frames[b, 2].numpy())], height=size[0], width=size[1])
        assert tuple(pre.shape) == (1, 3, *size) and float(pre.min()) >= 0.0     # already "non-negative": a second preprocess would rescale it
        laid_out = AutoencoderKLCogVideoX._channels_last(pre.to(BF).unsqueeze(2), cpad=5)      # as vae.encode lays its input out
        assert np.array_equal(_bits(out[b:b + 1]), _bits(laid_out))


# ---- the rollout ----
def tiny_vae(seed):
    from oracle import vae as ovae  # checker only: the source of the state dict's names and shapes
    from orv_amd.vae import AutoencoderKLCogVideoX
    cfg = dict(block_out_channels=(32, 64, 64, 128), layers_per_block=1)
    torch.manual_seed(seed)
    src = ovae.AutoencoderKLCogVideoX(**cfg)
    g = torch.Generator().manual_seed(seed + 1)
    for n, p in src.named_parameters():
        if p.ndim > 1:
            p.data.copy_(torch.randn(p.shape, generator=g) * (1.5 / (p[0].numel() ** 0.5)))
        elif "norm" in n and n.endswith("weight"):
            p.data.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
        else:
            p.data.copy_(0.1 * torch.randn(p.shape, generator=g))
        p.data.copy_(p.data.to(BF).float())
    m = AutoencoderKLCogVideoX(**cfg)
    m.load_state_dict(src.state_dict(), strict=True)
    return m.to(DEV, BF).eval()


H, W, FRAMES, STEPS, SEED = 64, 96, 9, 2, 5


class World:
    """The tiny pipeline of tests/test_gpu_metrics.py, the plan, per-slice controls and every run the tests below share (each made once)."""

    def __init__(self):
        import PIL.Image
        from conftest import load_golden
        from orv_amd import rollout, schedulers
        from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj, CogVideoXTransformer3DModelTraj
        cfg, _, ins, w, _ = load_golden("pipe_ddim")
        tr = CogVideoXTransformer3DModelTraj(**cfg)
        tr.load_state_dict(w)
        self.tr = tr.to(DEV, BF).eval()
        sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                                  prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=3.0,
                                                  timestep_spacing="trailing")
        self.pipe = CogVideoXImageToVideoPipelineTraj(transformer=self.tr, scheduler=sched, vae=tiny_vae(seed=5))
        self.plan = rollout.plan_slices(20, 8, 1, 8)
        assert [s.start_frame_idx for s in self.plan] == [0, 8, 11]              # hand-offs at the end of a slice and at position 3
        self.embeds = ins["prompt_embeds"][:1].to(DEV, BF)
        base = ins["actions"][:1]
        g = torch.Generator().manual_seed(21)
        self.actions = [(base + 0.1 * torch.randn(base.shape, generator=g)).to(DEV) for _ in self.plan]       # every slice its own controls
        rgb = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=g).numpy()
        self.images = [PIL.Image.fromarray(a) for a in rgb]
        self.cache = {}

    def _batch(self, B):
        self.tr.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
        return dict(height=H, width=W, num_inference_steps=STEPS, guidance_scale=1.0, prompt_embeds=self.embeds.expand(B, -1, -1).contiguous())

    def by_hand(self, which, run=0):
        """The loop written by hand from the public pieces, B = 1 as the reference runs it -> (episode uint8 [N, H, W, 3], last slice)."""
        key = ("hand", which, run)
        if key not in self.cache:
            kw = self._batch(1)
            image, slices = [self.images[which]], []
            for k, s in enumerate(self.plan):
                videos = self.pipe(image=image, num_frames=FRAMES, generator=torch.Generator().manual_seed(SEED), output_type="pil",
                                   controls_or_guidances={"actions": self.actions[k]}, **kw).frames
                slices.append(videos[0])
                if s.next_start_frame_idx != -1:
                    image = [videos[0][s.frame_ids.index(s.next_start_frame_idx)]]
            starts = [0] + [s.next_start_frame_idx for s in self.plan[:-1]]
            episode = []
            for k in range(len(slices)):                                         # evaluation_control_to_video.py:366-375
                end = starts[k + 1] - starts[k] if k < len(slices) - 1 else -1
                episode.extend(slices[k][0:end])
            self.cache[key] = (np.stack([np.array(f) for f in episode]), np.stack([np.array(f) for f in slices[-1]]))
        return self.cache[key]

    def rolled(self, which, **extra):
        key = ("roll", tuple(which), tuple(sorted(extra.items())))
        if key not in self.cache:
            kw = self._batch(len(which))
            images = [self.images[i] for i in which]
            self.cache[key] = self.pipe.rollout(images, self.plan, lambda s: {"actions": self.actions[s.sample_index].expand(len(which), -1, -1).contiguous()},
                                                seed=SEED, **kw, **extra)
        return self.cache[key]


@pytest.fixture(scope="module")
def world():
    return World()


def _spread(world):
    """The by-hand loop run twice: the largest difference of a byte between the two runs (0 when the pipeline is bit-reproducible)."""
    a, b = world.by_hand(0, 0)[0], world.by_hand(0, 1)[0]
    spread = int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())
    print(f"by-hand loop, two runs: {int((a != b).sum())} of {a.size} bytes differ, largest difference {spread}")
    return spread


def test_encode_channels_last_equals_encode(world):
    """What lets the hand-off write the channels-last layout: both entry points give the same moments on the same pixels."""
    vae = world.pipe.vae
    x = (torch.rand(1, 3, 1, H, W, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV, BF)
    a = vae.encode(x).latent_dist.parameters
    b = vae.encode_channels_last(vae._channels_last(x, cpad=5), dtype=BF)
    assert a.dtype == b.dtype and torch.equal(a, b)


def test_rollout_equals_the_loop_written_by_hand(world):
    spread = _spread(world)
    want, _ = world.by_hand(0)
    graphed = world.pipe._graphed
    assert graphed is not None                                                   # the by-hand calls replayed their steps from a HIP graph
    captured = {k: st["graph"] for k, st in graphed._state.items() if "graph" in st}
    assert captured
    out = world.rolled([0])
    assert out.frames.dtype == torch.uint8 and out.frames.is_cuda and tuple(out.frames.shape) == (1, 19, H, W, 3) == (1, *want.shape)
    assert out.ranges == [(0, 0, 8), (1, 0, 3), (2, 0, 8)] and out.slices == world.plan
    got = out.frames[0].cpu().numpy()
    diff = int(np.abs(got.astype(np.int16) - want.astype(np.int16)).max())
    print(f"rollout against the by-hand loop: {int((got != want).sum())} of {got.size} bytes differ, largest difference {diff}")
    assert diff <= spread                                                        # spread == 0: bit for bit
    assert len(np.unique(got)) > 32                                              # a picture, not a saturated plane
    now = world.pipe._graphed._state                                             # every chunk replayed that graph: no new key, no new capture
    assert world.pipe._graphed is graphed and set(now) == set(captured) and all(now[k]["graph"] is g for k, g in captured.items())


def test_rollout_batch_equals_its_episodes(world):
    spread = _spread(world)
    singles = [world.rolled([i]).frames[0].cpu().numpy() for i in (0, 1)]
    assert not np.array_equal(singles[0], singles[1])
    both = world.rolled([0, 1]).frames
    assert tuple(both.shape) == (2, 19, H, W, 3) and both.is_contiguous()
    for i in (0, 1):
        diff = int(np.abs(both[i].cpu().numpy().astype(np.int16) - singles[i].astype(np.int16)).max())
        print(f"episode {i} of the batch against its own rollout: largest difference {diff}")
        assert diff <= spread
    second = world.by_hand(1)[0]
    assert int(np.abs(singles[1].astype(np.int16) - second.astype(np.int16)).max()) <= spread


def test_keep_last_frame_adds_the_last_slices_final_frame(world):
    spread = _spread(world)
    base = world.rolled([0]).frames[0].cpu().numpy()
    kept = world.rolled([0], keep_last_frame=True)
    assert kept.ranges[-1] == (2, 0, 9) and tuple(kept.frames.shape) == (1, 20, H, W, 3)
    got = kept.frames[0].cpu().numpy()
    last = world.by_hand(0)[1][-1]
    assert int(np.abs(got[:-1].astype(np.int16) - base.astype(np.int16)).max()) <= spread
    assert int(np.abs(got[-1].astype(np.int16) - last.astype(np.int16)).max()) <= spread


def test_rollout_output_types_and_refusals(world):
    u8 = world.rolled([0]).frames
    as_np = world.rolled([0], output_type="np").frames
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.uint8 and np.array_equal(as_np, u8.cpu().numpy())
    import PIL.Image
    as_pil = world.rolled([0], output_type="pil").frames
    assert len(as_pil) == 1 and len(as_pil[0]) == 19 and all(isinstance(f, PIL.Image.Image) and f.size == (W, H) and f.mode == "RGB" for f in as_pil[0])
    assert np.array_equal(np.stack([np.array(f) for f in as_pil[0]]), as_np[0])
    by_hand = world.by_hand(0)[0]                                                # the PIL frames the loop written by hand stitches
    assert int(np.abs(as_np[0].astype(np.int16) - by_hand.astype(np.int16)).max()) <= _spread(world)
    with pytest.raises(ValueError, match="gave 1 entries"):
        world.pipe.rollout([world.images[0]], world.plan, [{}], seed=SEED, **world._batch(1))


def test_rollout_frames_are_scored_where_they_are(world):
    from orv_amd import metrics
    frames = world.rolled([0]).frames[0]                                         # uint8 [N, H, W, 3] on the device
    gt = torch.randint(0, 256, tuple(frames.shape), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    res = metrics.frame_metrics(frames, gt.to(DEV), size=(40, 52))
    again = metrics.frame_metrics(frames.cpu().numpy(), gt.numpy(), size=(40, 52))
    assert tuple(res.psnr.shape) == (19,) and bool(torch.isfinite(res.psnr).all()) and bool(torch.isfinite(res.ssim).all())
    assert torch.equal(res.psnr, again.psnr) and torch.equal(res.ssim, again.ssim) and torch.equal(res.mse, again.mse)
