#!/usr/bin/env python3
"""Time point-cloud voxelization at the reference's occupancy geometry: 400^3 cells over [-0.2, 0.2] x [-0.2, 0.2] x [0, 0.4] (cell 0.001),
max_points 100, max_voxels 1e5, the values points_to_voxels fixes (prepare_dataset.py:162-163).

    python tools/voxelize_bench.py [--out profiles/voxelize.txt] [--iters 20]

The size of a real reconstructed point cloud is not in the reference tree, so N = 100 k and 1 M are assumptions; the points are synthetic, a
curved surface over the whole x, y range with a little noise in z, [N, 4] with an integer class in the fourth feature.  Compared per size:
  * `voxelization` (hard) against a plain torch-ops formulation written here (coordinates by tensor arithmetic, torch.unique with
    return_inverse, a stable sort, scatter), which must return the same three tensors;
  * the fused `points_to_voxels` against native hard voxelization followed by the reference's torch post-processing (prepare_dataset.py:
    179-196) of the [M, 100, 4] buffer, kept on the GPU here (the reference copies the buffer to the host first, which costs more);
  * the split of one voxelization into its kernels and torch steps.
The reference's own CUDA kernels do not run on this hardware, so there is no timing of them.

It is a tool, not a test: there is no pass / fail bar.  The parent process never touches the GPU; every GPU step is a child process under its
own time limit, and the first failing step ends the run.  Times are medians of --iters runs after a warm-up: wall clock for the whole calls
(each has one host sync inside), HIP events for the kernels.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS, RANGE, MAX_POINTS, MAX_VOXELS = [0.001] * 3, [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4], 100, 100000
SIZES = (100_000, 1_000_000)
STEPS = (("hard", 300), ("fused", 300), ("kernels", 300))     # (child step, its time limit in seconds)


def cloud(n, dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(n)
    xy = rng.uniform(-0.21, 0.21, size=(n, 2))                  # a rim of points falls outside the range
    z = 0.2 + 0.1 * np.sin(12.0 * xy[:, 0]) * np.cos(9.0 * xy[:, 1]) + rng.normal(0.0, 0.0005, n)
    lab = rng.integers(0, 12, n)
    return torch.from_numpy(np.concatenate([xy, z[:, None], lab[:, None]], 1).astype(np.float32)).to(dev)


def torch_ops_hard(pts, vs, rng, grid, max_points, max_voxels):
    """Hard voxelization out of stock torch operators: the yardstick."""
    import torch
    N, dev = pts.shape[0], pts.device
    c = torch.floor((pts[:, :3] - rng[:3]) / vs)
    valid = ((c >= 0) & (c < grid)).all(1)
    ci = c.long()
    key = torch.where(valid, (ci[:, 2] * grid[1].long() + ci[:, 1]) * grid[0].long() + ci[:, 0], torch.full_like(ci[:, 0], 2 ** 62))
    _, inv = torch.unique(key, return_inverse=True)
    sinv, order = torch.sort(inv, stable=True)
    head = torch.ones(N, dtype=torch.bool, device=dev)
    head[1:] = sinv[1:] != sinv[:-1]
    head_pos = torch.nonzero(head)[:, 0]
    first_pt = order[head_pos]
    first_pt = torch.where(valid[first_pt], first_pt, torch.full_like(first_pt, N))      # the group of invalid points is numbered last
    vnum = torch.empty_like(first_pt)
    vnum[torch.argsort(first_pt)] = torch.arange(len(first_pt), device=dev)
    seglen = torch.diff(head_pos, append=torch.tensor([N], device=dev))
    rank = torch.arange(N, device=dev) - head_pos[sinv]
    v = vnum[sinv]
    M = min(int(valid[order[head_pos]].sum()), max_voxels)
    keep = valid[order] & (v < M) & (rank < max_points)
    voxels = torch.zeros(M, max_points, pts.shape[1], device=dev)
    voxels[v[keep], rank[keep]] = pts[order[keep]]
    hk = keep & (rank == 0)
    coors = torch.zeros(M, 3, dtype=torch.int32, device=dev)
    coors[v[hk]] = ci[order[hk]][:, [2, 1, 0]].int()
    num = torch.zeros(M, dtype=torch.int32, device=dev)
    num[v[hk]] = seglen[sinv[hk]].clamp(max=max_points).int()
    return voxels, coors, num


def torch_vote(voxels, coors):
    """The torch post-processing points_to_voxels applies to the hard voxels (prepare_dataset.py:179-196), on the device the buffer is on."""
    import torch
    stored = voxels[..., -1]
    uniq, mapped = torch.unique(stored, sorted=True, return_inverse=True)
    counts = torch.zeros(len(voxels), len(uniq), dtype=torch.long, device=voxels.device)
    counts.scatter_add_(1, mapped, torch.ones_like(mapped))
    idx = torch.argsort(counts, dim=-1, descending=True)
    top = uniq[idx[:, 0]]
    if idx.shape[-1] > 1:
        top = torch.where(top == 0, uniq[idx[:, 1]], top)
    return torch.cat([coors[:, [2, 1, 0]].double(), (top - 1).double()[:, None]], 1)


def _wall_ms(fn, iters, warm=3):
    import time
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return dict(ms_median=t[len(t) // 2], ms_min=t[0], ms_max=t[-1])


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


def child(step, n, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from orv_amd import ops, voxelize as vz
    dev = torch.device("cuda:0")
    pts = cloud(n, dev)
    vs, rng = vz._floats(VS, 3, "voxel_size"), vz._floats(RANGE, 6, "coors_range")
    out = {"step": step, "N": n}
    native = lambda: vz.voxelization(pts, VS, RANGE, MAX_POINTS, MAX_VOXELS)
    if step == "hard":
        tvs, trng = torch.from_numpy(vs).to(dev), torch.from_numpy(rng).to(dev)
        grid = torch.tensor(ops.voxel_grid_size(vs, rng), device=dev)
        yard = lambda: torch_ops_hard(pts, tvs, trng, grid, MAX_POINTS, MAX_VOXELS)
        a, b = native(), yard()
        out["same"] = all(torch.equal(x, y) for x, y in zip(a, b))
        out.update(M=int(a[1].shape[0]), fullest=int(a[2].max()), native=_wall_ms(native, iters), torch_ops=_wall_ms(yard, iters))
    elif step == "fused":
        xyz, lab = pts[:, :3].contiguous(), pts[:, 3].contiguous()
        fused = lambda: vz.points_to_voxels(xyz, VS, lab, point_cloud_range=RANGE)
        four = torch.cat([xyz, lab[:, None] + 1], 1)

        def unfused():
            voxels, coors, _ = vz.voxelization(four, VS, RANGE, MAX_POINTS, MAX_VOXELS)
            return torch_vote(voxels, coors).cpu().numpy()
        a, b = fused(), unfused()
        stored = vz.voxelization(four, VS, RANGE, MAX_POINTS, MAX_VOXELS)[0][..., -1]
        counts = torch.stack([(stored == k + 1).sum(1) for k in range(12)], 1)
        ties = ((counts == counts.max(1, keepdim=True).values).sum(1) > 1).cpu().numpy()
        out["same_off_ties"] = bool(np.array_equal(a[~ties], b[~ties]) and np.array_equal(a[:, :3], b[:, :3]))
        out.update(M=int(a.shape[0]), tie_share=float(ties.mean()), buffer_mb=a.shape[0] * MAX_POINTS * 4 * 4 / 1e6,
                   fused=_wall_ms(fused, iters), unfused=_wall_ms(unfused, iters))
    else:
        four = torch.cat([pts[:, :3], pts[:, 3:] + 1], 1)                  # the stored label is label + 1
        pt_coors, keys = ops.voxel_coors(four, vs, rng)
        skeys, order = torch.sort(keys, stable=True)
        start, seglen, first = ops.voxel_segments(skeys, order)
        csum = torch.cumsum(first, 0, dtype=torch.int32)
        M = min(int(csum[-1]), MAX_VOXELS)
        out["M"] = M
        steps = {
            "coors": (lambda: ops.voxel_coors(four, vs, rng), n * (16 + 12 + 8)),
            "sort": (lambda: torch.sort(keys, stable=True), 0),
            "segments": (lambda: ops.voxel_segments(skeys, order), n * (8 + 8 + 4 + 4 + 4)),
            "cumsum": (lambda: torch.cumsum(first, 0, dtype=torch.int32), n * 8),
            "scatter": (lambda: ops.voxel_scatter(four, pt_coors, order, start, seglen, csum, MAX_POINTS, M), 0),
            "vote": (lambda: ops.voxel_vote(four, pt_coors, order, start, seglen, csum, MAX_POINTS, M), 0),
        }
        for name, (fn, nbytes) in steps.items():
            out[name] = dict(_event_ms(fn, iters), bytes=nbytes)
    print("VOXEL_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return child(a.step, a.n, a.iters)
    f = lambda k: f"{k['ms_median']:.3f} ms ({k['ms_min']:.3f} .. {k['ms_max']:.3f})"
    lines = [f"voxelize_bench: synthetic surface points on the 400^3 occupancy grid, max_points {MAX_POINTS}, max_voxels {MAX_VOXELS}, "
             f"median of {a.iters} (min .. max); N is an assumption, the reference tree holds no real point cloud"]
    failed = False
    for n in SIZES:
        if failed:
            break
        lines.append(f"N = {n}")
        for step, limit in STEPS:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(n),
                                "--iters", str(a.iters)], capture_output=True, text=True)
            got = [l for l in r.stdout.splitlines() if l.startswith("VOXEL_BENCH ")]
            if r.returncode != 0 or not got:
                lines.append(f"step {step}: FAILED (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                failed = True                                    # nothing more is started on the GPU after a failing step
                break
            d = json.loads(got[-1][12:])
            if step == "hard":
                lines.append(f"  hard voxelization, wall, one host sync inside: M = {d['M']} voxels, fullest {d['fullest']} points")
                lines.append(f"    orv_amd.voxelize.voxelization   {f(d['native'])}")
                lines.append(f"    torch-ops yardstick             {f(d['torch_ops'])}   same result: {d['same']}")
            elif step == "fused":
                lines.append(f"  points_to_voxels, wall: M = {d['M']}, the unfused buffer is {d['buffer_mb']:.1f} MB, tie share {d['tie_share']:.3f}")
                lines.append(f"    fused vote                      {f(d['fused'])}")
                lines.append(f"    native hard + torch vote on GPU {f(d['unfused'])}   same off the ties: {d['same_off_ties']}")
            else:
                lines.append(f"  kernels and torch steps, HIP events (M = {d['M']}):")
                for name in ("coors", "sort", "segments", "cumsum", "scatter", "vote"):
                    k = d[name]
                    rate = f", {k['bytes'] / 1e6:.1f} MB -> {k['bytes'] / k['ms_median'] / 1e6:.0f} GB/s" if k["bytes"] else ""
                    note = " (with the zero fill of the [M, 100, 4] buffer)" if name == "scatter" else ""
                    lines.append(f"    {name:<9} {k['ms_median']:.4f} ms ({k['ms_min']:.4f} .. {k['ms_max']:.4f}){rate}{note}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(report + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
