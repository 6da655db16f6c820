#!/usr/bin/env python3
"""Time the per-frame PSNR / SSIM at the reference's geometry: a 17-frame prediction of 320 x 480 against a 256 x 320 ground truth, both
compared at 256 x 320 (orv/pipeline/compute_metrics.py:38-80).

    python tools/metrics_bench.py [--out profiles/metrics.txt] [--iters 30]

Compared:
  * `orv_amd.metrics.frame_metrics` (two launches) from uint8 [N, H, W, 3] frames and from the pipeline's 'pt' output, fp32 [N, 3, H, W];
  * the same result out of torch operators on the same GPU: F.interpolate(mode="bilinear", align_corners=False), five
    avg_pool2d(7, stride=1), the SSIM expression and two reductions, from the same resident tensors (the largest differences of the
    per-frame PSNR and SSIM are printed);
  * the fp32 numpy restatement (tests/metrics_ref.py) on the host cores, standing in for the reference's CPU path, whose libraries (cv2,
    skimage) are not installed here: one process, numpy's own threading, not the reference's 64 threads.

It is a tool, not a test: there is no pass / fail bar.  The parent process never touches the GPU; every GPU step is a child process under
its own time limit, and the first failing step ends the run.  GPU times are medians of --iters runs after a warm-up, HIP events around
the calls; the host time is the median of three runs of a wall clock.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAME, PRED, GT, SIZE = 17, (320, 480), (256, 320), (256, 320)
STEPS = (("gpu", 300), ("host", 300))             # (child step, its time limit in seconds)


def _event_ms(fn, iters, warm=3):
    import torch
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(ms_median=t[len(t) // 2], ms_min=t[0], ms_max=t[-1])


def clip():
    """uint8 [17, 320, 480, 3] and [17, 256, 320, 3]: a smooth pattern plus noise, so that the SSIM is neither 0 nor 1."""
    import numpy as np
    g = np.random.default_rng(0)
    out = []
    for h, w in (PRED, GT):
        y, x = np.mgrid[0:h, 0:w]
        base = 0.5 + 0.4 * np.sin(6.0 * y / h)[..., None] * np.cos(9.0 * x[..., None] / w + np.arange(3))
        out.append(np.round(np.clip(base[None] + g.normal(0, 0.05, (N_FRAME, h, w, 3)), 0, 1) * 255).astype(np.uint8))
    return out


def torch_ops(pred, gt, data_range=1.0):
    """pred, gt fp32 [N, 3, H, W] in [0, 1] -> (psnr [N], ssim [N]) out of stock torch operators: the yardstick."""
    import torch
    import torch.nn.functional as F
    a = F.interpolate(pred, size=SIZE, mode="bilinear", align_corners=False)
    b = F.interpolate(gt, size=SIZE, mode="bilinear", align_corners=False)
    mse = ((a - b) ** 2).double().mean(dim=(1, 2, 3))
    psnr = 10.0 * torch.log10(data_range ** 2 / mse)
    box = lambda t: F.avg_pool2d(t, 7, stride=1)
    ux, uy, uxx, uyy, uxy = box(a), box(b), box(a * a), box(b * b), box(a * b)
    cn, c1, c2 = 49.0 / 48.0, (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return psnr, S.double().mean(dim=(1, 2, 3))


def child(step, iters):
    import numpy as np
    pred8, gt8 = clip()
    out = {"step": step}
    if step == "host":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import metrics_ref as ref
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = ref.frame_metrics_ref(pred8, gt8, SIZE)
            times.append((time.perf_counter() - t0) * 1e3)
        out["numpy"] = dict(ms_median=sorted(times)[1], ms_min=min(times), ms_max=max(times))
        out["psnr"], out["ssim"] = float(r["psnr"].mean()), float(r["ssim"].mean())
    else:
        import torch
        sys.path.insert(0, ROOT)
        from orv_amd import metrics
        dev = torch.device("cuda:0")
        p8, g8 = torch.from_numpy(pred8).to(dev), torch.from_numpy(gt8).to(dev)
        ppt, gpt = ((t.float() / 255).permute(0, 3, 1, 2).contiguous() for t in (p8, g8))          # the 'pt' form
        fused8 = lambda: metrics.frame_metrics(p8, g8, size=SIZE)
        fusedpt = lambda: metrics.frame_metrics(ppt, gpt, size=SIZE, layout="nchw")
        yard = lambda: torch_ops(ppt, gpt)
        a, b, (yp, ys) = fused8(), fusedpt(), yard()
        out["psnr"], out["ssim"] = float(a.psnr.mean()), float(a.ssim.mean())
        out["u8_vs_pt"] = dict(psnr=float((a.psnr - b.psnr).abs().max()), ssim=float((a.ssim - b.ssim).abs().max()))
        out["fused_vs_torch"] = dict(psnr=float((b.psnr - yp).abs().max()), ssim=float((b.ssim - ys).abs().max()))
        out["fused_u8"], out["fused_pt"], out["torch_ops"] = _event_ms(fused8, iters), _event_ms(fusedpt, iters), _event_ms(yard, iters)
        out["fused_pt_full"] = _event_ms(lambda: metrics.frame_metrics(ppt, gpt, size=SIZE, layout="nchw", full=True), iters)
        out["bytes_u8"], out["bytes_pt"] = int(p8.numel() + g8.numel()), int(4 * (ppt.numel() + gpt.numel()))
    print("METRICS_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return child(a.step, a.iters)
    f = lambda k: f"{k['ms_median']:.3f} ms ({k['ms_min']:.3f} .. {k['ms_max']:.3f})"
    lines = [f"metrics_bench: {N_FRAME} frames, prediction {PRED[0]} x {PRED[1]}, ground truth {GT[0]} x {GT[1]}, compared at {SIZE[0]} x {SIZE[1]}; "
             f"synthetic frames; GPU: HIP events, median of {a.iters} (min .. max); host: wall clock, median of 3"]
    failed = False
    for step, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters)],
                           capture_output=True, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("METRICS_BENCH ")]
        if r.returncode != 0 or not got:
            lines.append(f"step {step}: FAILED (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            failed = True                                        # nothing more is started after a failing step
            break
        d = json.loads(got[-1][len("METRICS_BENCH "):])
        if step == "gpu":
            lines.append(f"  mean psnr {d['psnr']:.4f} dB, mean ssim {d['ssim']:.6f}")
            lines.append(f"  fused frame_metrics, uint8 [N,H,W,3]    {f(d['fused_u8'])}   {d['bytes_u8'] / 1e6:.1f} MB read")
            lines.append(f"  fused frame_metrics, 'pt' fp32 [N,3,H,W] {f(d['fused_pt'])}   {d['bytes_pt'] / 1e6:.1f} MB read")
            lines.append(f"  the same with full=True (SSIM map stored) {f(d['fused_pt_full'])}")
            lines.append(f"  torch-ops yardstick, 'pt' fp32            {f(d['torch_ops'])}   ratio {d['torch_ops']['ms_median'] / d['fused_pt']['ms_median']:.2f}x")
            lines.append(f"  largest per-frame difference fused vs torch ops: psnr {d['fused_vs_torch']['psnr']:.3e} dB, ssim {d['fused_vs_torch']['ssim']:.3e}; "
                         f"uint8 vs 'pt' input: psnr {d['u8_vs_pt']['psnr']:.3e} dB, ssim {d['u8_vs_pt']['ssim']:.3e}")
        else:
            lines.append(f"  fp32 numpy restatement on the host (one process)   {f(d['numpy'])}; mean psnr {d['psnr']:.4f} dB, mean ssim {d['ssim']:.6f}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(report + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
