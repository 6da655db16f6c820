#!/usr/bin/env python3
"""Time the Gaussian rasterizer on the scene `get_render` builds (prepare_dataset.py:2060-2086) at 320x480.

    python tools/gs_render_bench.py [--out profiles/gs_render.txt] [--iters 30]

The reference renders the occupied cells of a 400^3 grid over [-0.2, 0.2] x [-0.2, 0.2] x [0, 0.4] (cell 0.001): identity rotation, opacity 1,
zero colour, one-hot 12-class features and an isotropic scale that grows with the depth bin, base 0.00023 x (1 + k / 399)^3.7.  The occupancy
itself comes from a dataset that is not here, so this tool fills the grid with a synthetic scene of the same kind: a tilted table surface three
cells thick and a few boxes standing on it.  The camera is the first view's (identity pose), focal length 400 px, principal point at the centre.

It is a tool, not a test: there is no pass / fail bar.  The parent process never touches the GPU; every GPU step is a child process under its
own time limit, and the first failing step ends the run.  Reported per step: milliseconds (median of --iters after warm-up), and for the
kernels the bytes and FLOPs their launch implies.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FOCAL, F = 320, 480, 400.0, 12
STEPS = (("render", 240), ("kernels", 240))       # (child step, its time limit in seconds)


def scene(dev):
    """-> the arguments of `render` for the synthetic occupancy (torch tensors on `dev`)."""
    import numpy as np
    import torch
    n = 400
    ax = [torch.linspace(-0.2, 0.2, n), torch.linspace(-0.2, 0.2, n), torch.linspace(0.0, 0.4, n)]   # create_full_center_coords' axes
    i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    table = (0.55 * n + 0.25 * (j - n // 2)).long().clamp(0, n - 4)                                   # depth index of the surface, tilted in y
    cells = [torch.stack([i, j, table + t], -1).reshape(-1, 3) for t in range(3)]
    labels = [torch.full((n * n,), 1 + t % 2) for t in range(3)]
    rng = np.random.RandomState(0)
    for b in range(6):                                                                                # boxes in front of the table
        x0, y0, sx, sy, sz = rng.randint(60, 280), rng.randint(120, 300), rng.randint(30, 70), rng.randint(30, 70), rng.randint(20, 60)
        bi, bj, bk = torch.meshgrid(torch.arange(x0, x0 + sx), torch.arange(y0, y0 + sy), torch.arange(sz), indexing="ij")
        front = table[bi, bj] - 1 - bk
        shell = (bk == sz - 1) | (bi == x0) | (bi == x0 + sx - 1) | (bj == y0) | (bj == y0 + sy - 1)
        keep = shell & (front > 40)
        cells.append(torch.stack([bi[keep], bj[keep], front[keep]], -1))
        labels.append(torch.full((int(keep.sum()),), 3 + b))
    ijk, lab = torch.cat(cells), torch.cat(labels)
    xyz = torch.stack([ax[0][ijk[:, 0]], ax[1][ijk[:, 1]], ax[2][ijk[:, 2]]], -1)
    bins = 1.0 + torch.arange(n, dtype=torch.float32) / (n - 1)
    scale = (0.00023 * bins ** 3.7)[ijk[:, 2]][:, None].expand(-1, 3).contiguous()
    N = xyz.shape[0]
    rot = torch.zeros(N, 4)
    rot[:, 0] = 1
    feat = torch.nn.functional.one_hot(lab, F).float()
    intr = torch.tensor([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]])
    d = lambda t: t.to(dev)
    return dict(extrinsics=torch.eye(4, device=dev), intrinsics=d(intr), image_shape=[H, W], pts_xyz=d(xyz), pts_rgb=torch.zeros(N, 3, device=dev),
                feat=d(feat), rotations=d(rot), scales=d(scale), opacity=torch.ones(N, 1, device=dev), bg_color=[0, 0, 0])


def _median_ms(fn, iters, warm=5):
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
    return t[len(t) // 2], t[0], t[-1]


def child(step, iters):
    import math
    import time
    import torch
    sys.path.insert(0, ROOT)
    from orv_amd import gs_render as g, ops
    dev = torch.device("cuda:0")
    s = scene(dev)
    N = s["pts_xyz"].shape[0]
    out = {"step": step, "N": N, "H": H, "W": W, "F": F}
    if step == "render":
        pkg = g.render(**s)
        torch.cuda.synchronize()
        wall = []
        for _ in range(iters):                                  # wall clock: the call has one host sync inside (the pair count)
            t0 = time.perf_counter()
            pkg = g.render(**s)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        wall.sort()
        out.update(render_ms_median=wall[len(wall) // 2], render_ms_min=wall[0], render_ms_max=wall[-1],
                   visible=int((pkg["radii"] > 0).sum()), covered=float((pkg["render_alpha"] > 0.1).float().mean()),
                   alpha_max=float(pkg["render_alpha"].max()), depth_max=float(pkg["render_depth"].max()))
    else:
        view = torch.eye(4, device=dev)
        proj = view @ g.get_projection_matrix_c(FOCAL, FOCAL, W / 2, H / 2, W, H, 0.1, 200.0).t().to(dev)
        tf = (math.tan(0.5 * g.focal2fov(FOCAL, W)), math.tan(0.5 * g.focal2fov(FOCAL, H)))
        pre = lambda: ops.gs_preprocess(s["pts_xyz"], s["scales"], s["rotations"], s["opacity"], view, proj, H, W, tf[0], tf[1], 1.0)
        xy, conic_op, depth, radii, rect, tiles = pre()
        offsets = torch.cumsum(tiles, 0, dtype=torch.int64)
        L = int(offsets[-1])
        keys, idx = ops.gs_tile_keys(rect, depth, offsets, H, W, L)
        skeys, order = torch.sort(keys, stable=True)
        plist = idx[order]
        ranges = ops.gs_tile_ranges(skeys, H, W)
        bg = torch.zeros(3, device=dev)
        ntiles = ranges.shape[0]
        lens = (ranges[:, 1] - ranges[:, 0]).long()
        out.update(L=L, tiles=ntiles, list_mean=float(lens.float().mean()), list_max=int(lens.max()))
        steps = {
            "preprocess": (pre, N * (3 + 3 + 4 + 1 + 2 + 4 + 1 + 1 + 4 + 1) * 4, N * 150),
            "cumsum": (lambda: torch.cumsum(tiles, 0, dtype=torch.int64), N * 12, 0),
            "tile_keys": (lambda: ops.gs_tile_keys(rect, depth, offsets, H, W, L), N * 28 + L * 12, 0),
            "sort": (lambda: torch.sort(keys, stable=True), 0, 0),
            "gather": (lambda: idx[order], L * 16, 0),
            "tile_ranges": (lambda: ops.gs_tile_ranges(skeys, H, W), L * 8 + ntiles * 8, 0),
            # staged once per tile entry: 10 + F floats and the index; planes written once.  FLOPs: an upper bound, every pixel of a tile
            # evaluating every entry of its list (11 for the power, ~8 for the exponential, 4 for the tests, 2 (4 + F) for the sums)
            "render": (lambda: ops.gs_render(ranges, plist, xy, conic_op, depth, s["pts_rgb"], s["feat"], bg, H, W),
                       L * (10 + F + 1) * 4 + (3 + F + 2) * H * W * 4, L * 256 * (23 + 2 * (4 + F))),
        }
        for name, (fn, nbytes, flops) in steps.items():
            med, lo, hi = _median_ms(fn, iters)
            out[name] = dict(ms_median=med, ms_min=lo, ms_max=hi, bytes=nbytes, flops=flops, gb_per_s=nbytes / med / 1e6 if nbytes else None,
                             gflop_per_s=flops / med / 1e6 if flops else None)
    print("GS_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return child(a.step, a.iters)
    lines = [f"gs_render_bench: synthetic occupancy on the 400^3 get_render grid, {H}x{W}, F = {F}, median of {a.iters} (min .. max)"]
    for step, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters)],
                           capture_output=True, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("GS_BENCH ")]
        if r.returncode != 0 or not got:
            lines.append(f"step {step}: FAILED (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            break                                                # nothing more is started on the GPU after a failing step
        d = json.loads(got[-1][9:])
        if step == "render":
            lines.append(f"N = {d['N']} Gaussians, {d['visible']} visible, {d['covered'] * 100:.1f} % of pixels with alpha > 0.1")
            lines.append(f"render(): {d['render_ms_median']:.3f} ms wall ({d['render_ms_min']:.3f} .. {d['render_ms_max']:.3f}), one host sync inside")
        else:
            lines.append(f"L = {d['L']} (Gaussian, tile) pairs over {d['tiles']} tiles: mean list {d['list_mean']:.0f}, longest {d['list_max']}")
            for name in ("preprocess", "cumsum", "tile_keys", "sort", "gather", "tile_ranges", "render"):
                k = d[name]
                rate = (f", {k['bytes'] / 1e6:.2f} MB -> {k['gb_per_s']:.0f} GB/s" if k["bytes"] else "") + \
                       (f", at most {k['flops'] / 1e9:.2f} GFLOP (every pixel evaluating its tile's whole list; early stops do less)"
                        if name == "render" else f", {k['flops'] / 1e9:.3f} GFLOP -> {k['gflop_per_s']:.0f} GFLOP/s" if k["flops"] else "")
                lines.append(f"  {name:<12} {k['ms_median']:.4f} ms ({k['ms_min']:.4f} .. {k['ms_max']:.4f}){rate}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(report + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
