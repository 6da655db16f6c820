#!/usr/bin/env python3
"""Time the point-cloud front of the reconstruction stage (orv_amd.pointcloud): k-nearest neighbours, statistical outlier removal, normals.

    python tools/pointcloud_bench.py [--out profiles/pointcloud.txt] [--iters 20]

The size of a real reconstructed point cloud is not in the reference tree, so N = 100 k and 1 M are assumptions; the points are the bench
surface of tools/voxelize_bench.py (a curved sheet over the whole x, y range with a little noise in z), xyz only.  Per size:
  * wall times of knn(k = 30), remove_statistical_outlier(30, 1.5), estimate_normals(20) and preprocess_points + nksr_inputs, and the share
    of queries the grid walk leaves to the brute kernel;
  * the split of the calls into their kernels and torch steps (HIP events);
  * yardstick 1, on the same GPU and the same points: a torch-ops formulation, a chunked fp64 distance matrix + topk, then the removal and
    the normals by tensor arithmetic (torch.linalg.eigh).  It scans all pairs, so above --yard-full points only --yard-queries queries are
    timed and the time is scaled to N: the report says which;
  * yardstick 2, on the host: scipy.spatial.cKDTree build + query(k = 30, workers = 16), the stand-in for the Open3D KD-tree the reference
    runs single-threaded (Open3D itself is not installed here).

It is a tool, not a test: there is no pass / fail bar.  The parent process never touches the GPU; every step is a child process under its
own time limit, and the first failing step ends the run.  Times are medians of --iters runs after a warm-up (fewer for the yardsticks, as
the report says): wall clock around a device synchronise for whole calls, HIP events for the kernels.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (100_000, 1_000_000)
STEPS = (("native", 300), ("kernels", 300), ("torch", 420), ("ckdtree", 300))     # (child step, its time limit in seconds)
K, K_NORMALS, CHUNK = 30, 20, 1024


def cloud(n):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    rng = np.random.default_rng(n)                              # the surface of voxelize_bench.cloud, xyz only
    xy = rng.uniform(-0.21, 0.21, size=(n, 2))
    z = 0.2 + 0.1 * np.sin(12.0 * xy[:, 0]) * np.cos(9.0 * xy[:, 1]) + rng.normal(0.0, 0.0005, n)
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


def _wall_ms(fn, iters, warm=2):
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
    return dict(ms_median=t[len(t) // 2], ms_min=t[0], ms_max=t[-1], iters=iters)


def _event_ms(fn, iters, warm=2):
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
    return dict(ms_median=t[len(t) // 2], ms_min=t[0], ms_max=t[-1], iters=iters)


def torch_knn(pts64, queries, k):
    """k smallest distances of every query row by stock torch operators: the fp64 distance matrix of a chunk of queries by tensor arithmetic,
    then topk.  (torch.cdist(compute_mode="donot_use_mm_for_euclid_dist") was the first choice; at [1024, 100 000] x 3 in fp64 it returned
    wrong distances on all but the first rows with the torch build this was measured on, so the three differences are written out.)"""
    import torch
    idx, dist = [], []
    x, y, z = pts64[:, 0][None, :], pts64[:, 1][None, :], pts64[:, 2][None, :]
    for a in range(0, len(queries), CHUNK):
        q = pts64[queries[a:a + CHUNK]]
        dx, dy, dz = x - q[:, 0:1], y - q[:, 1:2], z - q[:, 2:3]
        d = (dx * dx + dy * dy + dz * dz).sqrt_()
        v, i = torch.topk(d, k, dim=1, largest=False, sorted=True)
        idx.append(i), dist.append(v)
    return torch.cat(idx), torch.cat(dist)


def torch_removal(dist, std_ratio):
    avg = dist.mean(1)
    ok = avg > 0
    thr = avg[ok].mean() + std_ratio * avg[ok].std()
    return (ok & (avg < thr)).nonzero().flatten()


def torch_normals(pts64, idx):
    import torch
    nb = pts64[idx]
    d = nb - nb.mean(1, keepdim=True)
    C = d.transpose(1, 2) @ d / idx.shape[1]
    n = torch.linalg.eigh(C)[1][:, :, 0]
    flip = (n * -pts64[:len(idx)]).sum(1) < 0
    return torch.where(flip[:, None], -n, n).float()


def child(step, n, iters, yard_full, yard_queries):
    import numpy as np
    out = {"step": step, "N": n}
    p = cloud(n)
    if step == "ckdtree":
        import time
        from scipy.spatial import cKDTree
        p64 = p.astype(np.float64)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            tree = cKDTree(p64)
            t1 = time.perf_counter()
            tree.query(p64, k=K, workers=16)
            t.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        t.sort()
        out.update(ms_median=t[1][0], ms_min=t[0][0], ms_max=t[2][0], build_ms=t[1][1], iters=3)
        print("PC_BENCH " + json.dumps(out))
        return
    import torch
    sys.path.insert(0, ROOT)
    from orv_amd import ops, pointcloud as pc
    pts = torch.from_numpy(p).to("cuda:0")
    if step == "native":
        idx, d2, stats = pc.knn(pts, K, return_stats=True)
        out.update(grid=stats["grid"], cell=stats["cell"], brute=stats["brute"])
        out["knn"] = _wall_ms(lambda: pc.knn(pts, K), iters)
        out["removal"] = _wall_ms(lambda: pc.remove_statistical_outlier(pts, K, 1.5), iters)
        out["normals"] = _wall_ms(lambda: pc.estimate_normals(pts, K_NORMALS), iters)
        out["chain"] = _wall_ms(lambda: pc.nksr_inputs(pc.preprocess_points(pts)), iters)
        out["kept"] = int(pc.preprocess_points(pts).shape[0])
    elif step == "kernels":
        origin, edge, dims = pc._grid(pts, K, None)
        keys = ops.pc_cells(pts, origin, edge, dims)
        skeys, order = torch.sort(keys, stable=True)
        n_cells = dims[0] * dims[1] * dims[2]
        start, spts = ops.pc_cell_table(skeys, order, pts, n_cells)
        idx, d2, pending = ops.pc_knn(spts, order, start, K, origin, edge, dims)
        left = torch.nonzero(pending).flatten()
        if left.numel():
            ops.pc_knn_brute(pts, K, left, out=(idx, d2))
        some = torch.arange(0, n, max(1, n // 256), device=pts.device)[:256].contiguous()
        idx20 = idx[:, :K_NORMALS].contiguous()
        out.update(n_cells=n_cells, brute=int(left.numel()), brute_timed=int(some.numel()))
        steps = {
            "survey (torch, one host read)": lambda: pc._survey(pts),
            "orv_pc_cells": lambda: ops.pc_cells(pts, origin, edge, dims),
            "sort (torch)": lambda: torch.sort(keys, stable=True),
            "orv_pc_cell_table": lambda: ops.pc_cell_table(skeys, order, pts, n_cells),
            "orv_pc_knn": lambda: ops.pc_knn(spts, order, start, K, origin, edge, dims, out=(idx, d2)),
            "orv_pc_knn_brute": lambda: ops.pc_knn_brute(pts, K, some),
            "orv_pc_outlier": lambda: ops.pc_outlier(d2, K, 1.5),
            "orv_pc_normals": lambda: ops.pc_normals(pts, idx20, K_NORMALS, (0.0, 0.0, 0.0)),
        }
        out["steps"] = {name: _event_ms(fn, iters) for name, fn in steps.items()}
    else:
        pts64 = pts.double()
        full = n <= yard_full
        queries = torch.arange(n, device=pts.device) if full else torch.arange(0, n, n // yard_queries, device=pts.device)[:yard_queries]
        scale = n / len(queries)
        reps = 5 if full else 3
        out.update(full=full, queries=int(len(queries)), scale=scale)
        out["knn"] = _wall_ms(lambda: torch_knn(pts64, queries, K), reps, warm=1)
        ti, td = torch_knn(pts64, queries, K)
        ni, nd2 = pc.knn(pts, K)
        out["same_sets"] = float((torch.sort(ti, 1)[0] == torch.sort(ni[queries].long(), 1)[0]).all(1).float().mean())
        out["max_rel_dist"] = float(((td - nd2[queries].sqrt()).abs() / nd2[queries].sqrt().clamp_min(1e-30))[:, 1:].max())
        out["removal_after_knn"] = _wall_ms(lambda: torch_removal(td, 1.5), reps, warm=1)
        out["normals_after_knn"] = _wall_ms(lambda: torch_normals(pts64, ti[:, :K_NORMALS]), reps, warm=1)
    print("PC_BENCH " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES), help="comma-separated point counts")
    ap.add_argument("--yard-full", type=int, default=100_000, help="largest N at which the torch-ops yardstick runs every query")
    ap.add_argument("--yard-queries", type=int, default=16384, help="queries the torch-ops yardstick times above that")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return child(a.step, a.n, a.iters, a.yard_full, a.yard_queries)
    f = lambda k: f"{k['ms_median']:.3f} ms ({k['ms_min']:.3f} .. {k['ms_max']:.3f}; {k['iters']} runs)"
    lines = [f"pointcloud_bench: the bench surface of voxelize_bench, xyz, k = {K} (normals {K_NORMALS}); median (min .. max; runs); N is an "
             "assumption, the reference tree holds no real point cloud; the LDS-shared candidate blocks of the issue were not built"]
    failed = False
    for n in [int(s) for s in a.sizes.split(",")]:
        if failed:
            break
        lines.append(f"N = {n}")
        native = None
        for step, limit in STEPS:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(n),
                                "--iters", str(a.iters), "--yard-full", str(a.yard_full), "--yard-queries", str(a.yard_queries)],
                               capture_output=True, text=True)
            got = [l for l in r.stdout.splitlines() if l.startswith("PC_BENCH ")]
            if r.returncode != 0 or not got:
                lines.append(f"step {step}: FAILED (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                failed = True                                    # nothing more is started on the GPU after a failing step
                break
            d = json.loads(got[-1][9:])
            if step == "native":
                native = d
                lines.append(f"  orv_amd.pointcloud, wall: grid {tuple(d['grid'])}, cell {d['cell']:.5g}, {d['brute']} of {n} queries "
                             f"({d['brute'] / n:.4%}) to the brute kernel")
                lines.append(f"    knn(k = {K})                               {f(d['knn'])}")
                lines.append(f"    remove_statistical_outlier({K}, 1.5)       {f(d['removal'])}")
                lines.append(f"    estimate_normals({K_NORMALS})                       {f(d['normals'])}")
                lines.append(f"    preprocess_points + nksr_inputs           {f(d['chain'])}   ({d['kept']} points kept)")
            elif step == "kernels":
                lines.append(f"  kernels and torch steps, HIP events ({d['n_cells']} cells; the brute kernel on {d['brute_timed']} queries):")
                for name, k in d["steps"].items():
                    lines.append(f"    {name:<30} {k['ms_median']:.4f} ms ({k['ms_min']:.4f} .. {k['ms_max']:.4f})")
            elif step == "torch":
                how = "every query" if d["full"] else f"{d['queries']} queries timed, scaled by {d['scale']:.1f} to N"
                k = d["knn"]
                lines.append(f"  torch-ops yardstick on the same GPU (chunked fp64 distance matrix + topk, {how}):")
                lines.append(f"    knn(k = {K})                               {k['ms_median'] * d['scale']:.1f} ms ({k['iters']} runs)   "
                             f"native is {k['ms_median'] * d['scale'] / native['knn']['ms_median']:.1f}x faster; same neighbour sets on "
                             f"{d['same_sets']:.5f} of the queries, distances within {d['max_rel_dist']:.1e}")
                lines.append(f"    removal after it                          {f(d['removal_after_knn'])}")
                lines.append(f"    normals after it (eigh, {d['queries']} points)    {f(d['normals_after_knn'])}")
            else:
                lines.append(f"  scipy cKDTree on the host, build + query(k = {K}, workers = 16):")
                lines.append(f"    knn(k = {K})                               {f(d)}, of which build {d['build_ms']:.1f} ms   native is "
                             f"{d['ms_median'] / native['knn']['ms_median']:.1f}x faster")
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(report + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
