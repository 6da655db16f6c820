#!/usr/bin/env python3
"""Time label-map compositing at the reference's geometry: 480 x 640 frames, 17 and 30 frames per trajectory, 8 and 59 masks per frame
(59 = every palette entry but the black one), as bool masks and as fp32 logits.

    python tools/labelmap_bench.py [--out profiles/labelmap.txt] [--iters 20]

The masks are synthetic: per (frame, mask) a random ellipse, built on the device; logits are +-2 plus noise around them.  Per size:
  * `ops.lm_compose` with a given order and `ops.lm_mask_stats`, by HIP events, with the bytes each must move (compose: F m H W bytes per
    mask pixel read + 4 F H W written, the traffic floor; stats: F n H W bytes per mask pixel read) and the rate that gives;
  * `labelmap.compose` with `order=None` (statistics of the first frame, one host read, then the kernel), wall clock;
  * the same images out of stock torch operators on the same GPU, written here: 2 m `torch.where` passes over [F, H, W] (and a threshold
    pass for logits), native and yardstick interleaved run by run, and checked to give the same images;
  * the numpy restatement (tests/labelmap_ref.py) on the host, once: the 2 m boolean-index stores per frame of the reference, without its
    disk round trip and its process pool.
The kernel walks the paint order forwards; the backward walk with an early exit was not built, so there is one form to time.
It is a tool, not a test: there is no pass / fail bar.  The parent process never touches the GPU; every GPU step is a child process under its
own time limit, and the first failing step ends the run.  Times are medians of --iters runs after a warm-up.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 480, 640
SIZES = ((17, 8), (17, 59), (30, 8), (30, 59))
KINDS = (("bool", 360), ("logits", 360))             # (child step, its time limit in seconds)


def ellipses(F, n, dev, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda lo, hi: (torch.rand(F, n, 1, 1, generator=g) * (hi - lo) + lo).to(dev)
    cy, cx, ry, rx = r(0, H), r(0, W), r(10, H / 3), r(10, W / 3)
    yy, xx = torch.arange(H, device=dev).view(1, 1, H, 1), torch.arange(W, device=dev).view(1, 1, 1, W)
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def torch_compose(on, ids, cols, order):
    """The yardstick: the reference's two paint loops out of stock torch operators, all frames at once; ``ids`` uint8 [n] and ``cols`` uint8
    [n, 3] (each mask's triple) on the device."""
    import torch
    F = on.shape[0]
    index = torch.full((F, H, W), 255, dtype=torch.uint8, device=on.device)
    color = torch.zeros(F, H, W, 3, dtype=torch.uint8, device=on.device)
    for j in order:
        m = on[:, j]
        index = torch.where(m, ids[j], index)
        color = torch.where(m[..., None], cols[j], color)
    return index, color


def _summary(t):
    t = sorted(t)
    return dict(ms_median=t[len(t) // 2], ms_min=t[0], ms_max=t[-1])


def _wall_pair(fa, fb, iters, warm=2):
    import torch
    ta, tb = [], []
    for i in range(warm + iters):
        for fn, t in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                t.append((time.perf_counter() - t0) * 1e3)
    return _summary(ta), _summary(tb)


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
    return _summary([a.elapsed_time(b) for a, b in ev])


def child(kind, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import labelmap_ref as ref
    from orv_amd import labelmap as lm, ops
    dev = torch.device("cuda:0")
    mb = 1 if kind == "bool" else 4
    pal = lm._check_palette(None, "bgr")
    for F, n in SIZES:
        on = ellipses(F, n, dev, 1000 * F + n)
        masks = on if kind == "bool" else torch.where(on, 2.0, -2.0) + torch.randn(F, n, H, W, device=dev) * 0.5
        ids = np.arange(1, n + 1, dtype=np.int64)
        ids_dev = torch.from_numpy(ids).to(dev).to(torch.uint8)
        cols = torch.from_numpy(np.ascontiguousarray(pal[ids % 60])).to(dev)
        order = lm.paint_order(ops.lm_mask_stats(masks[:1])[0][0])
        thresholded = (lambda: masks > 0.0) if kind == "logits" else (lambda: masks)
        native, yard = (lambda: lm.compose(masks, ids)), (lambda: torch_compose(thresholded(), ids_dev, cols, order.tolist()))
        a, b = native(), yard()
        out = {"kind": kind, "F": F, "n": n, "same": bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])),
               "painted": float((a[0] != 255).float().mean())}
        del a, b
        out["native"], out["yard"] = _wall_pair(native, yard, iters)
        out["compose"] = dict(_event_ms(lambda: ops.lm_compose(masks, order.tolist(), ids.tolist(), pal.tolist()), iters),
                              bytes=F * n * H * W * mb + 4 * F * H * W)
        out["stats"] = dict(_event_ms(lambda: ops.lm_mask_stats(masks), iters), bytes=F * n * H * W * mb)
        out["stats0"] = dict(_event_ms(lambda: ops.lm_mask_stats(masks[:1]), iters), bytes=n * H * W * mb)
        host = thresholded().cpu().numpy()                            # the paint loops alone: the masks already thresholded
        t0 = time.perf_counter()
        want = ref.compose(host, ids, order=order)
        out["numpy_ms"] = (time.perf_counter() - t0) * 1e3
        got = lm.compose(masks, ids, order=order)
        out["same_numpy"] = bool(np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]))
        del host, want, got, on, masks
        print("LM_BENCH " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kind", choices=[k for k, _ in KINDS], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kind:
        return child(a.kind, a.iters)
    f = lambda k: f"{k['ms_median']:.3f} ms ({k['ms_min']:.3f} .. {k['ms_max']:.3f})"
    rate = lambda k: f"{k['bytes'] / 1e6:.1f} MB -> {k['bytes'] / k['ms_median'] / 1e6:.0f} GB/s"
    lines = [f"labelmap_bench: synthetic ellipses, {H} x {W} frames, median of {a.iters} (min .. max), native and yardstick interleaved; "
             "the kernel walks the paint order forwards (the backward walk was not built)"]
    print(lines[0], flush=True)
    failed = False
    for kind, limit in KINDS:
        shown = len(lines)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--kind", kind, "--iters", str(a.iters)],
                           capture_output=True, text=True)
        got = [json.loads(l[9:]) for l in r.stdout.splitlines() if l.startswith("LM_BENCH ")]
        for d in got:
            lines.append(f"{d['kind']}, F = {d['F']} frames x n = {d['n']} masks ({d['painted']:.2f} of the pixels painted); same images as the torch "
                         f"operators: {d['same']}, as the numpy restatement: {d['same_numpy']}")
            lines.append(f"    orv_lm_compose, HIP events          {f(d['compose'])}   {rate(d['compose'])} of the traffic floor")
            lines.append(f"    orv_lm_mask_stats, all frames       {f(d['stats'])}   {rate(d['stats'])}")
            lines.append(f"    orv_lm_mask_stats, first frame      {f(d['stats0'])}   {rate(d['stats0'])}")
            lines.append(f"    labelmap.compose(order=None), wall  {f(d['native'])}")
            lines.append(f"    torch-ops yardstick, GPU, wall      {f(d['yard'])}")
            lines.append(f"    numpy restatement, host, one run    {d['numpy_ms']:.0f} ms")
        if r.returncode != 0 or len(got) != len(SIZES):
            lines.append(f"step {kind}: FAILED (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            failed = True                                    # nothing more is started on the GPU after a failing step
        print("\n".join(lines[shown:]), flush=True)
        if failed:
            break
    report = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(report + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
