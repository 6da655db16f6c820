#!/usr/bin/env python
"""Wall time of one chunk boundary of a cascaded rollout, from the decoded clip on the device to the encoder's input on the device (ending in
a synchronise): the host path of the loop written by hand (``postprocess_video('pil')``, the frame pick, ``preprocess``, the copy to
the device in bf16) against the two launches of ``orv_amd.rollout`` (``frames_quantize`` of the whole clip, ``frames_handoff``).

    python tools/rollout_time.py [--repeats 20] [--out profiles/rollout.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/rollout_time.py --kernels-only      (the two kernels' own durations)

320 x 480 x 17 frames at B = 1 and B = 4, warm-up first, the two paths alternated in one process, median and spread over the repeats.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from orv_amd import ops, rollout  # noqa: E402
from orv_amd.components import VideoProcessor  # noqa: E402

DEV, BF = "cuda:0", torch.bfloat16
F, H, W, INDEX = 17, 320, 480, 16


def host_path(vp, video):
    clips = vp.postprocess_video(video, "pil")
    image = [clip[INDEX] for clip in clips]
    out = vp.preprocess(image, height=H, width=W).to(device=DEV, dtype=BF)
    torch.cuda.synchronize()
    return out


def device_path(table, video):
    u8 = ops.frames_quantize(video)
    out = ops.frames_handoff(u8, INDEX, table)
    torch.cuda.synchronize()
    return u8, out


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="a few launches of the two kernels and nothing else (for a kernel trace)")
    args = ap.parse_args()
    vp = VideoProcessor(vae_latent_channels=16, vae_scale_factor=8)
    table = rollout.handoff_table().to(DEV)
    lines = [f"chunk boundary, decoded clip on the device -> encoder input on the device, {H} x {W} x {F} frames, bf16 clip, wall ms incl. synchronise",
             f"{args.repeats} repeats after 3 warm-up rounds, the two paths alternated in one process; median [min .. max]"]
    for B in (1, 4):
        video = (torch.rand(B, 3, F, H, W, generator=torch.Generator().manual_seed(B)) * 2.2 - 1.1).to(DEV, BF)
        if args.kernels_only:
            for _ in range(5):
                device_path(table, video)
            continue
        u8, handed = device_path(table, video)
        want = host_path(vp, video)                                              # the two paths give the same tensor
        assert torch.equal(handed[:, 0, :, :, :3].permute(0, 3, 1, 2), want) and not bool(handed[..., 3:].any())
        for _ in range(3):
            host_path(vp, video), device_path(table, video)
        host, dev = [], []
        for _ in range(args.repeats):
            host.append(timed(host_path, vp, video))
            dev.append(timed(device_path, table, video))
        fmt = lambda v: f"{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"
        lines.append(f"B = {B}: host path {fmt(host)}   device path {fmt(dev)}   ratio of medians {statistics.median(host) / statistics.median(dev):.0f}x")
    text = "\n".join(lines)
    print(text)
    if args.out and not args.kernels_only:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
