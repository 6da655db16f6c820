#!/usr/bin/env python3
"""Time control preparation at the reference's geometry: 17 frames x 1 and 3 views of 320 x 480 renders, the bridge plan
ori_size (256, 320) / render_size (480, 640) -> video_size (320, 480), and the VAE encode it feeds.

    python tools/conditions_bench.py [--out profiles/conditions.txt] [--iters 30]

Compared per view count, depth and labels each:
  * the fused preparation (`orv_amd.conditions.prepare_*`, one launch writing the bf16 [V, F, H, W, 8] tensor) against the same tensor
    built from torch operators on the same GPU: F.interpolate (antialiased bilinear / nearest) twice with the two crops, clamp and scale
    or the palette lookup, repeat, permute, pad to 8 channels, cast.  The yardstick starts from the render arrays already on the device
    and gathered in (v f) order by one index_select, as the fused call does; it must give the same tensor up to the bf16 rounding of
    fp32 results that differ in their last bits (the largest difference is printed, in bf16 ulps at 1.0 = 2^-8);
  * `vae.encode_channels_last` of that tensor on a random-weight VAE of the real widths, for scale.
The reference prepares on the CPU through torchvision, which is not installed here: there is no timing of that path.

It is a tool, not a test: there is no pass / fail bar.  The parent process never touches the GPU; every GPU step is a child process under
its own time limit, and the first failing step ends the run.  Times are medians of --iters runs after a warm-up, HIP events around the
calls (the label check's one host read is inside the fused label time).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAME, SOURCE = 17, (320, 480)
GEOMETRY = dict(ori_size=(256, 320), video_size=(320, 480), render_size=(480, 640))
STEPS = (("prepare", 300), ("encode", 420))       # (child step, its time limit in seconds)


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


def render(n_view, dev):
    import numpy as np
    import torch
    g = np.random.default_rng(n_view)
    depths = g.uniform(0.0, 0.5, size=(N_FRAME * n_view,) + SOURCE).astype(np.float32)
    ids = g.integers(0, 60, size=(N_FRAME * n_view,) + SOURCE).astype(np.uint8)
    index = torch.tensor([[f * n_view + v for f in range(N_FRAME)] for v in range(n_view)], dtype=torch.int32)
    return torch.from_numpy(depths).to(dev), torch.from_numpy(ids).to(dev), index.to(dev)


def torch_ops(x, index, stages, kind, palette):
    """The [V, F, H, W, 8] bf16 tensor out of stock torch operators: the yardstick."""
    import torch
    import torch.nn.functional as F
    V, Fr = index.shape
    x = x.index_select(0, index.reshape(-1).long())
    if kind == "depth":
        x = x[:, None]
    else:
        x = (palette[x.long()] / 255.0).permute(0, 3, 1, 2)          # painted first, as the reference does
    for rh, rw, top, left, ch, cw in stages:
        kw = dict(mode="bilinear", align_corners=False, antialias=True) if kind == "depth" else dict(mode="nearest")
        x = F.interpolate(x, size=(rh, rw), **kw)[..., top:top + ch, left:left + cw]
    if kind == "depth":
        x = (torch.clamp(x, min=0.01, max=0.4) * 2.5).repeat(1, 3, 1, 1)
    x = x.view(V, Fr, 3, *x.shape[-2:]).permute(0, 1, 3, 4, 2)
    return F.pad(x, (0, 5)).to(torch.bfloat16).contiguous()


def child(step, n_view, iters):
    import torch
    sys.path.insert(0, ROOT)
    from orv_amd import conditions as cond
    dev = torch.device("cuda:0")
    depths, ids, index = render(n_view, dev)
    plan = cond.ResizePlan.for_controls(source_size=SOURCE, **GEOMETRY)
    stages = [s.ints() for s in plan.stages]
    out = {"step": step, "n_view": n_view}
    fused = {"depth": lambda: cond.prepare_depths(depths, plan, index, out="vae"), "label": lambda: cond.prepare_labels(ids, plan, index, out="vae")}
    if step == "prepare":
        palette = torch.from_numpy(cond.palette60()).to(dev)
        yard = {"depth": lambda: torch_ops(depths, index, stages, "depth", None), "label": lambda: torch_ops(ids, index, stages, "label", palette)}
        for kind in ("depth", "label"):
            a, b = fused[kind](), yard[kind]()
            out[kind] = dict(shape=list(a.shape), max_diff=float((a.float() - b.float()).abs().max()), share_equal=float((a == b).float().mean()),
                             fused=_event_ms(fused[kind], iters), torch_ops=_event_ms(yard[kind], iters),
                             bytes_in=int((depths if kind == "depth" else ids).numel() * (4 if kind == "depth" else 1)), bytes_out=int(a.numel() * 2))
    else:
        from orv_amd.vae import AutoencoderKLCogVideoX
        torch.manual_seed(0)
        vae = AutoencoderKLCogVideoX().to(dev, torch.bfloat16).eval()
        h = fused["depth"]()
        out["moments"] = list(vae.encode_channels_last(h).shape)
        out["encode"] = _event_ms(lambda: vae.encode_channels_last(h), max(3, iters // 6), warm=1)
    print("COND_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help=argparse.SUPPRESS)
    ap.add_argument("--views", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return child(a.step, a.views, a.iters)
    f = lambda k: f"{k['ms_median']:.3f} ms ({k['ms_min']:.3f} .. {k['ms_max']:.3f})"
    lines = [f"conditions_bench: {N_FRAME} frames of {SOURCE[0]} x {SOURCE[1]} renders, ori_size {GEOMETRY['ori_size']}, render_size "
             f"{GEOMETRY['render_size']} -> video_size {GEOMETRY['video_size']}; synthetic renders; HIP events, median of {a.iters} (min .. max)"]
    failed = False
    for n_view in (1, 3):
        if failed:
            break
        lines.append(f"views = {n_view}")
        for step, limit in STEPS:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--views", str(n_view),
                                "--iters", str(a.iters)], capture_output=True, text=True)
            got = [l for l in r.stdout.splitlines() if l.startswith("COND_BENCH ")]
            if r.returncode != 0 or not got:
                lines.append(f"step {step}: FAILED (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                failed = True                                    # nothing more is started on the GPU after a failing step
                break
            d = json.loads(got[-1][11:])
            if step == "prepare":
                for kind in ("depth", "label"):
                    k = d[kind]
                    mb = (k["bytes_in"] + k["bytes_out"]) / 1e6
                    lines.append(f"  {kind}: -> bf16 {k['shape']}, {mb:.1f} MB read + written by the fused call")
                    lines.append(f"    fused prepare_{kind}s          {f(k['fused'])}   {mb / k['fused']['ms_median']:.0f} GB/s")
                    lines.append(f"    torch-ops yardstick           {f(k['torch_ops'])}   ratio {k['torch_ops']['ms_median'] / k['fused']['ms_median']:.2f}x; "
                                 f"largest difference {k['max_diff']:.3e}, {100 * k['share_equal']:.3f} % of the values equal")
            else:
                lines.append(f"  vae.encode_channels_last of the depth tensor (random weights, real widths) -> {d['moments']}: {f(d['encode'])}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(report + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
