"""GPU: video metrics (orv_amd.metrics, csrc/metrics.hip).
* the kernel against the numpy restatement (tests/metrics_ref.py): ``ssim_map`` bit for bit - the contract fixes every rounding - and
  ``mse`` / ``ssim`` / ``psnr`` to relative 1e-10: they differ from the restatement only in the order of at most 8e4 fp64 additions (and
  one fp64 log10), which bounds the error near n * 2^-53 = 1e-11;
* shapes where the kernel can go wrong: one window, ragged tiles in both axes, one row and column past a tile, up- and downscale, the
  identity, two source sizes, one and five frames; every input form (uint8 / fp32 NHWC, fp32 NCHW, a width slice, numpy);
* the real geometry once, also against the fp64 restatement within the gap tests/test_metrics_host.py measures;
* reproducibility, exact values, ``psnr_ssim``, the single-image wrappers, the pipeline's ``'pt'`` output, device-side refusals.
PARITY UNPINNED: cv2 and skimage are absent; see tests/test_metrics_host.py for what ties the contract to scipy's filter."""
import ctypes
import math

import numpy as np
import pytest
import torch

import metrics_ref as ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
REL = 1e-10


def mt():
    from orv_amd import metrics
    return metrics


def frames_u8(n, shape, seed):
    """uint8 [n, h, w, 3] prediction and ground truth of one shape; even frames are noise against a slightly disturbed copy (near-equal
    and equal pixels occur), odd frames a constant +-1."""
    g = np.random.default_rng(seed)
    h, w = shape
    pred = g.integers(0, 256, (n, h, w, 3))
    gt = np.clip(pred + g.integers(-2, 3, (n, h, w, 3)) * (g.uniform(size=(n, h, w, 1)) < 0.5), 0, 255)
    pred[1::2] = 128 + g.integers(-1, 2, pred[1::2].shape)
    gt[1::2] = 128 + g.integers(-1, 2, gt[1::2].shape)
    return pred.astype(np.uint8), gt.astype(np.uint8)


def f32(u8):
    return u8.astype(np.float32) / np.float32(255)


def check(res, want, n):
    got_map = res.ssim_map.cpu().numpy()
    assert got_map.dtype == np.float32 and got_map.shape == want["ssim_map"].shape
    assert np.array_equal(got_map.view(np.int32), want["ssim_map"].view(np.int32)), np.abs(got_map - want["ssim_map"]).max()
    for key in ("mse", "ssim", "psnr"):
        got = getattr(res, key)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n,) and got.is_cuda
        got, w = got.cpu().numpy(), want[key]
        finite = np.isfinite(w)
        assert np.array_equal(np.isfinite(got), finite) and np.array_equal(got[~finite], w[~finite])
        err = np.abs(got[finite] - w[finite]) / np.maximum(np.abs(w[finite]), 1e-300)
        print(f"{key}: largest relative difference {err.max() if err.size else 0.0:.3e}")
        assert np.all(err <= REL), (key, got, w)


# (frames, prediction source, ground-truth source, resized)
SHAPES = {
    "one_window": (1, (11, 13), (11, 13), (7, 7)),
    "8x9_up": (5, (5, 6), (5, 6), (8, 9)),
    "ragged_up": (5, (37, 53), (37, 53), (45, 70)),
    "down": (1, (96, 144), (96, 144), (40, 52)),
    "identity_aligned": (5, (64, 64), (64, 64), (64, 64)),
    "one_past_a_tile": (1, (41, 90), (41, 90), (33, 65)),
    "two_sources": (5, (48, 72), (32, 40), (32, 40)),
}


def case_inputs(name):
    n, ps, gs, size = SHAPES[name]
    seed = sorted(SHAPES).index(name)
    pred = frames_u8(n, ps, seed)[0]
    gt = frames_u8(n, gs, seed)[1] if gs == ps else frames_u8(n, gs, seed + 50)[1]
    return n, size, pred, gt


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fp32_frames_equal_the_restatement(name):
    n, size, pred, gt = case_inputs(name)
    want = ref.frame_metrics_ref(f32(pred), f32(gt), size)
    res = mt().frame_metrics(torch.from_numpy(f32(pred)).to(DEV), torch.from_numpy(f32(gt)).to(DEV), size=size, full=True)
    check(res, want, n)
    plain = mt().frame_metrics(torch.from_numpy(f32(pred)).to(DEV), torch.from_numpy(f32(gt)).to(DEV), size=size)
    assert plain.ssim_map is None and torch.equal(plain.ssim, res.ssim) and torch.equal(plain.mse, res.mse)       # storing S changes nothing


@pytest.mark.parametrize("form", ["uint8_nhwc", "fp32_nchw", "width_slice", "numpy", "mixed"])
@pytest.mark.parametrize("name", ["ragged_up", "two_sources"])
def test_every_input_form_equals_the_restatement(name, form):
    m = mt()
    n, size, pred, gt = case_inputs(name)
    if form == "uint8_nhwc":
        want = ref.frame_metrics_ref(pred, gt, size)
        res = m.frame_metrics(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), size=size, full=True)
    elif form == "fp32_nchw":
        want = ref.frame_metrics_ref(f32(pred), f32(gt), size)
        nchw = lambda x: torch.from_numpy(f32(x)).to(DEV).permute(0, 3, 1, 2).contiguous()
        res = m.frame_metrics(nchw(pred), nchw(gt), size=size, layout="nchw", full=True)
    elif form == "width_slice":                  # the middle third of three views side by side, uint8 and fp32: views, not copies
        wide = lambda x, fill: np.concatenate([np.full_like(x, fill), x, np.full_like(x, 255 - fill)], axis=2)
        wp, wg = torch.from_numpy(wide(pred, 9)).to(DEV), torch.from_numpy(f32(wide(gt, 200))).to(DEV)
        sp, sg = wp[:, :, pred.shape[2]:2 * pred.shape[2]], wg[:, :, gt.shape[2]:2 * gt.shape[2]]
        assert not sp.is_contiguous() and not sg.is_contiguous()
        want = ref.frame_metrics_ref(pred, f32(gt), size)
        res = m.frame_metrics(sp, sg, size=size, full=True)
    elif form == "numpy":
        want = ref.frame_metrics_ref(pred, f32(gt), size)
        res = m.frame_metrics(pred, f32(gt), size=size, full=True)
    else:                                        # fp32 NCHW slice of a larger batch against uint8: a storage offset and two dtypes
        want = ref.frame_metrics_ref(f32(pred), gt, size)
        big = torch.zeros(n + 2, 3, *pred.shape[1:3], device=DEV)
        big[1:n + 1] = torch.from_numpy(f32(pred)).to(DEV).permute(0, 3, 1, 2)
        res = m.frame_metrics(big[1:n + 1], torch.from_numpy(gt).to(DEV).permute(0, 3, 1, 2), size=size, layout="nchw", full=True)
    check(res, want, n)


def test_real_geometry_and_the_fp64_formula():
    """17 frames 320 x 480 against 256 x 320 at 256 x 320 (8 x 10 tiles per frame): the restatement, and the fp64 formula within twice the
    gap the host test measures for each frame's kind (a property of the fp32 formula, see tests/test_metrics_host.py)."""
    pred, gt = ref.real_clip()
    want = ref.frame_metrics_ref(pred, gt, (256, 320))
    w64 = ref.frame_metrics_ref(pred, gt, (256, 320), dtype=np.float64)
    res = mt().frame_metrics(pred, gt, full=True)                  # the default size
    check(res, want, 17)
    ssim, psnr = res.ssim.cpu().numpy(), res.psnr.cpu().numpy()
    for i in range(17):
        bound = ref.MEASURED_GAP[ref.KINDS[i % 3]]
        gs, gp = abs(ssim[i] - w64["ssim"][i]), abs(psnr[i] - w64["psnr"][i])
        print(f"frame {i} ({ref.KINDS[i % 3]}): ssim gap {gs:.3e}, psnr gap {gp:.3e} dB")
        assert gs <= 2 * bound["ssim"] and gp <= 2 * bound["psnr"]


def test_two_calls_are_bit_identical():
    n, size, pred, gt = case_inputs("ragged_up")
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    a, b = (mt().frame_metrics(p, g, size=size, full=True) for _ in range(2))
    for key in ("mse", "psnr", "ssim", "ssim_map"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key


def test_exact_values():
    m = mt()
    x = torch.from_numpy(frames_u8(3, (40, 50), 9)[0]).to(DEV)
    for size in ((40, 50), (33, 47)):
        same = m.frame_metrics(x, x.clone(), size=size, full=True)
        assert torch.all(same.ssim == 1.0) and torch.all(same.ssim_map == 1.0) and torch.all(same.mse == 0.0) and torch.all(torch.isinf(same.psnr))
    # constant images 0.5 and 0.25: S = (0.25 + C1) / (0.3125 + C1) up to the rounding of two fp32 products and one division (1.5 ulp)
    a, b = torch.full((2, 35, 40, 3), 0.5, device=DEV), torch.full((2, 35, 40, 3), 0.25, device=DEV)
    c1 = float(np.float32(0.01 * 0.01))
    closed = (0.25 + c1) / (0.3125 + c1)
    r = m.frame_metrics(a, b, size=(35, 40), full=True)
    assert float((r.ssim_map.double() - closed).abs().max()) <= 2.0 ** -23 and float((r.ssim - closed).abs().max()) <= 2.0 ** -23
    assert torch.all(r.mse == 0.0625) and float((r.psnr - 10 * math.log10(16)).abs().max()) <= 1e-12
    # data_range scales C1, C2 and the PSNR peak
    r255 = m.frame_metrics(a * 255, b * 255, size=(35, 40), data_range=255.0)
    assert float((r255.psnr - r.psnr).abs().max()) <= 1e-9 and float((r255.ssim - r.ssim).abs().max()) <= 1e-6


def test_psnr_ssim_is_the_mean_over_the_compared_frames_and_view_takes_its_third():
    m = mt()
    g = np.random.default_rng(12)
    pred = g.integers(0, 256, (6, 20, 3 * 164, 3)).astype(np.uint8)          # three views of 164 columns: wider than 480
    gt = g.integers(0, 256, (4, 24, 3 * 170, 3)).astype(np.uint8)
    n, psnr, ssim = m.psnr_ssim(pred, gt, view=1, size=(16, 24))
    assert n == 3                                                            # min(6, 4) - 1, as the reference compares
    want = m.frame_metrics(np.ascontiguousarray(pred[:3, :, 164:328]), np.ascontiguousarray(gt[:3, :, 170:340]), size=(16, 24))
    assert psnr == float(want.psnr.cpu().numpy().mean()) and ssim == float(want.ssim.cpu().numpy().mean())
    r = ref.frame_metrics_ref(pred[:3, :, 164:328], gt[:3, :, 170:340], (16, 24))
    assert abs(psnr - r["psnr"].mean()) <= REL * psnr and abs(ssim - r["ssim"].mean()) <= REL * abs(ssim)
    n0, p0, s0 = m.psnr_ssim(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), view=-1, size=(16, 24))      # no view: the whole width
    whole = m.frame_metrics(pred[:3], gt[:3], size=(16, 24))
    assert n0 == 3 and p0 == float(whole.psnr.cpu().numpy().mean()) and p0 != psnr
    narrow = g.integers(0, 256, (3, 20, 480, 3)).astype(np.uint8)            # not wider than 480: the view is ignored, as in the reference
    assert m.psnr_ssim(narrow, narrow[:, :, ::-1].copy(), view=2, size=(16, 24)) == m.psnr_ssim(narrow, narrow[:, :, ::-1].copy(), view=-1, size=(16, 24))


def test_single_image_wrappers_equal_frame_metrics_at_the_images_own_size():
    m = mt()
    pred, gt = frames_u8(1, (23, 37), 14)
    a, b = f32(pred[0]), f32(gt[0])
    want = m.frame_metrics(a[None], b[None], size=(23, 37), full=True)
    assert m.peak_signal_noise_ratio(a, b, data_range=1.0) == float(want.psnr[0])
    assert m.structural_similarity(a, b, channel_axis=-1, data_range=1.0) == float(want.ssim[0])
    s, smap = m.structural_similarity(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), channel_axis=-1, data_range=1.0, full=True)
    assert s == float(want.ssim[0]) and torch.equal(smap, want.ssim_map[0])
    with pytest.raises(ValueError, match="two images of one shape"):
        m.structural_similarity(a, b[:-1], channel_axis=-1, data_range=1.0)


# ---- the pipeline's 'pt' output on the tiny random-weight VAE (the construction of tests/test_gpu_vae.py, restated) ----
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


def test_pipeline_pt_frames_are_scored_where_they_are():
    from conftest import load_golden
    from orv_amd import schedulers
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj, CogVideoXTransformer3DModelTraj
    cfg, _, ins, w, _ = load_golden("pipe_ddim")
    tr = CogVideoXTransformer3DModelTraj(**cfg)
    tr.load_state_dict(w)
    tr = tr.to(DEV, BF).eval()
    tr.action_embed.forced_mask = torch.zeros(1, dtype=torch.bool)
    sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                              prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=3.0,
                                              timestep_spacing="trailing")
    pipe = CogVideoXImageToVideoPipelineTraj(transformer=tr, scheduler=sched, vae=tiny_vae(seed=5))
    g = torch.Generator().manual_seed(11)
    image_lat = torch.randn(1, 16, 1, 8, 12, generator=g).to(DEV, BF)
    lat0 = torch.randn(1, 3, 16, 8, 12, generator=g).to(DEV, BF)
    video = pipe(image=image_lat, height=64, width=96, num_frames=9, num_inference_steps=2, guidance_scale=1.0, latents=lat0,
                 prompt_embeds=ins["prompt_embeds"][:1].to(DEV, BF), output_type="pt",
                 controls_or_guidances={"actions": ins["actions"][:1].to(DEV)}).frames[0]
    assert tuple(video.shape) == (9, 3, 64, 96) and video.dtype == torch.float32 and video.is_cuda
    gt = torch.rand(9, 3, 64, 96, generator=torch.Generator().manual_seed(2)).to(DEV)
    res = mt().frame_metrics(video, gt, size=(40, 52), layout="nchw", full=True)
    nhwc = lambda t: np.ascontiguousarray(t.cpu().permute(0, 2, 3, 1).numpy())
    check(res, ref.frame_metrics_ref(nhwc(video), nhwc(gt), (40, 52)), 9)


def test_device_side_refusals_launch_nothing():
    from orv_amd import _lib
    h = _lib.lib()
    err = lambda: h.orv_last_error().decode()
    src = torch.rand(2, 8, 8, 3, device=DEV)
    out = torch.full((3, 2), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)

    def frames(**kw):
        f = _lib.Frames()
        f.data, f.kind, f.h, f.w, f.extent, f.offset = src.data_ptr(), 0, 8, 8, src.numel(), 0
        for k, v in enumerate(kw.pop("stride", (192, 24, 3, 1))):
            f.stride[k] = v
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def call(p, g, hh=8, ww=8, o=out.data_ptr(), w=ws.data_ptr()):
        return h.orv_frame_metrics(ctypes.byref(p) if p is not None else None, ctypes.byref(g), 2, hh, ww, 1.0, o, None, w, 64, None)

    ok = frames()
    assert call(None, ok) != 0 and "null pointer" in err()
    assert call(frames(data=None), ok) != 0 and "null pointer" in err()
    assert call(ok, ok, o=None) != 0 and "null pointer" in err()
    assert call(ok, ok, hh=6) != 0 and "supported: 7 to 32768" in err()
    assert call(ok, ok, ww=6) != 0 and "supported: 7 to 32768" in err()
    assert call(ok, frames(stride=(192, 24, 3, -1))) != 0 and "bad strides: gt" in err()
    assert call(frames(stride=(193, 24, 3, 1)), ok) != 0 and "bad strides: pred" in err()
    assert call(frames(offset=1), ok) != 0 and "bad strides: pred" in err()
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(ws == -7.0)                  # nothing ran
    assert call(ok, ok) == 0                                                 # and the same arguments, valid, do
    torch.cuda.synchronize()
    assert torch.all(out[2] == 1.0) and torch.all(out[0] == 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mt().frame_metrics(src.cpu(), src, size=(8, 8))
