#!/usr/bin/env python3
"""Time occupancy labelling and the sparse scene preparation at the reference's geometry: a 480 x 640 label image, 400^3 cells over
[-0.2, 0.2] x [-0.2, 0.2] x [0, 0.4] (cell 0.001), at most 1e5 occupied voxels per frame (points_to_voxels' max_voxels).

    python tools/occupancy_bench.py [--out profiles/occupancy.txt] [--iters 20]

The size of a real reconstructed point cloud is not in the reference tree, so N = 100 k and 1 M points are assumptions (the sizes of
profiles/voxelize.txt); the points are synthetic, a curved surface over the x, y range with a little noise in z.  Compared per size, native
and yardstick interleaved run by run on the same device:
  * `project_labels` against the formulation of the reference (project_3d_to_2d and the labelling block, prepare_dataset.py:878-884 and
    :999-1008) out of stock torch operators on the GPU, written here; both get the label image in the same form, once as the uint8 numpy
    array of the label file and once resident on the device;
  * `OccupancyScene.gaussians` on the frame's occupancy rows (what points_to_voxels returns for the cloud) against the dense formulation
    of the reference (:2148-2164 over the resident tensors of :2069-2086) out of stock torch operators on the GPU, written here, with the
    peak device memory of both;
  * the split of one scene preparation into its kernels and torch steps.
It is a tool, not a test: there is no pass / fail bar.  The parent process never touches the GPU; every GPU step is a child process under its
own time limit, and the first failing step ends the run.  Times are medians of --iters runs after a warm-up: wall clock for whole calls,
HIP events for the kernels.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS, RANGE = [0.001] * 3, [-0.2, -0.2, 0.0, 0.2, 0.2, 0.4]
SIZES = (100_000, 1_000_000)
STEPS = (("label", 300), ("scene", 420), ("kernels", 300))     # (child step, its time limit in seconds)


def cloud(n, dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(n)
    xy = rng.uniform(-0.21, 0.21, size=(n, 2))                  # a rim of points falls outside the range
    z = 0.2 + 0.1 * np.sin(12.0 * xy[:, 0]) * np.cos(9.0 * xy[:, 1]) + rng.normal(0.0, 0.0005, n)
    return torch.from_numpy(np.concatenate([xy, z[:, None]], 1).astype(np.float32)).to(dev)


def camera_and_labels(dev):
    """A camera rotated 0.3 rad and set back 0.45 from the scene's centre, f = 650 px, and a 480 x 640 uint8 label image with 255s."""
    import numpy as np
    import torch
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    extrin = np.eye(4)
    extrin[:3, :3], extrin[:3, 3] = rot, np.array([0.0, 0.0, 0.2]) - rot @ np.array([0.0, 0.0, 0.45])
    intrin = np.eye(4)
    intrin[:3, :3] = [[650, 0, 320], [0, 650, 240], [0, 0, 1]]
    rng = np.random.default_rng(0)
    img = ((np.arange(480)[:, None] // 80) * 5 + np.arange(640)[None, :] // 80) % 11     # with 59 for the 255s: twelve classes
    img = img.astype(np.uint8)
    img[rng.uniform(size=img.shape) < 0.05] = 255
    return torch.from_numpy(extrin).float().to(dev), torch.from_numpy(intrin).float().to(dev), img


def torch_labels(points, image, extrin, intrin):
    """The yardstick for labelling: the formulation the reference uses (a homogeneous [N,4] matrix product, whole-tensor divides, masks and
    indexed gathers) out of stock torch operators on the device the points are on.  ``image`` is the uint8 numpy label image or, already
    converted, an int64 tensor on the device."""
    import torch
    if not isinstance(image, torch.Tensor):
        image = torch.from_numpy(image).to(torch.int64).to(points.device)        # as the reference: widened on the host, then moved
    H, W = image.shape
    P = intrin @ torch.linalg.inv(extrin)
    h = torch.cat([points, torch.ones_like(points[:, :1])], dim=1) @ P.T
    col, row = (h[:, 0] / h[:, 2]).long(), (h[:, 1] / h[:, 2]).long()
    inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    out = torch.zeros(points.shape[0], dtype=torch.int64, device=points.device)
    out[inside] = image[row[inside], col[inside]]
    out[out == 255] = 59
    return out


class DenseScene:
    """The yardstick for the scene front: the dense formulation the reference uses, out of stock torch operators on the GPU.  Resident, built
    once: one entry per cell of the grid for every attribute.  Per frame: a label grid filled by indexed assignment, torch.unique over the
    whole grid with its inverse, a one-hot of the inverse, a boolean occupancy grid, six boolean gathers.  The grids are flat, cell (x, y, z)
    at (x Y + y) Z + z."""

    def __init__(self, scene, base_scale=0.00023, exp_scale=3.7):
        import torch
        self.dev, self.grid, self.num_channels = scene.device, scene.grid, scene.num_channels
        X, Y, Z = self.grid
        self.cells = X * Y * Z
        self.xyz = torch.cartesian_prod(*scene.axes).contiguous()                  # [cells, 3], z fastest
        self.rgb = torch.zeros(self.cells, 3, device=self.dev)
        self.rot = torch.tensor([1.0, 0.0, 0.0, 0.0], device=self.dev).repeat(self.cells, 1)
        self.scale = torch.ones(self.cells, 3, device=self.dev) * scene.zscale.repeat(X * Y)[:, None]
        self.opacity = torch.ones(self.cells, 1, device=self.dev)

    def gaussians(self, occ_np):
        import torch
        X, Y, Z = self.grid
        rows = torch.tensor(occ_np, dtype=torch.int32, device=self.dev).long()
        flat = (rows[:, 0] * Y + rows[:, 1]) * Z + rows[:, 2]
        labels = torch.zeros(self.cells, dtype=torch.int64, device=self.dev)
        labels[flat] = rows[:, 3]
        labels.clamp_(0, 59)
        classes, rank = torch.unique(labels, sorted=True, return_inverse=True)
        feat = torch.nn.functional.one_hot(rank, num_classes=self.num_channels).float()
        occupied = torch.zeros(self.cells, dtype=torch.bool, device=self.dev)       # on the device (the reference builds it on the host)
        occupied[flat] = True
        return (self.xyz[occupied], self.rgb[occupied], feat[occupied], self.rot[occupied], self.scale[occupied], self.opacity[occupied],
                classes, len(classes) > 1)


def _summary(t):
    t = sorted(t)
    return dict(ms_median=t[len(t) // 2], ms_min=t[0], ms_max=t[-1])


def _wall_pair(fa, fb, iters, warm=2):
    """Wall-clock times of two callables, alternating run by run."""
    import time
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


def _peak(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def child(step, n, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from orv_amd import occupancy as oc, ops
    dev = torch.device("cuda:0")
    pts = cloud(n, dev)
    extrin, intrin, img = camera_and_labels(dev)
    out = {"step": step, "N": n}
    if step == "label":
        # both sides get the image in the same form: the uint8 numpy array a caller loads from the label file (each converts and uploads it
        # on every call), and then resident on the device, each in the type it consumes (uint8 here, int64 for the torch statements)
        img_u8, img_i64 = torch.from_numpy(img).to(dev), torch.from_numpy(img).to(torch.int64).to(dev)
        native, yard = (lambda: oc.project_labels(pts, img, extrin, intrin)), (lambda: torch_labels(pts, img, extrin, intrin))
        native_r, yard_r = (lambda: oc.project_labels(pts, img_u8, extrin, intrin)), (lambda: torch_labels(pts, img_i64, extrin, intrin))
        a, b = native(), yard()
        out.update(differ=int((a != b).sum()), labelled=int((a != 0).sum()), same_resident=bool(torch.equal(a, native_r()) and torch.equal(b, yard_r())))
        out.update(peak_native=_peak(native), peak_yard=_peak(yard), peak_native_r=_peak(native_r), peak_yard_r=_peak(yard_r))
        out["native"], out["yard"] = _wall_pair(native, yard, iters)
        out["native_r"], out["yard_r"] = _wall_pair(native_r, yard_r, iters)
        P = oc.projection_matrix(extrin, intrin, dev)
        out["kernel"] = _event_ms(lambda: ops.occ_project_labels(pts, P, img_u8), iters)
        out["matrix"] = _event_ms(lambda: oc.projection_matrix(extrin, intrin, dev), iters)
    else:
        occ = oc.occupancy_from_points(pts, img, extrin, intrin, VS, RANGE)
        out["M"] = len(occ)
        scene = oc.OccupancyScene(RANGE, VS, device=dev)
        if step == "scene":
            dense = DenseScene(scene)
            native, yard = (lambda: scene.gaussians(occ)), (lambda: dense.gaussians(occ))
            a, b = native(), yard()
            out["same"] = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                              for x, y in zip(a[:7], b[:7])) and a[7] == b[7]
            out.update(n=int(a[0].shape[0]), classes=a[6].tolist(), resident_yard=torch.cuda.memory_allocated())
            del a, b
            out.update(peak_native=_peak(native), peak_yard=_peak(yard))
            out["native"], out["yard"] = _wall_pair(native, yard, iters)
        else:
            rows = scene._rows(occ)
            state = torch.zeros(3, dtype=torch.int64, device=dev)
            keys = ops.occ_cell_keys(rows, scene.grid, state)
            skeys, order = torch.sort(keys, stable=True)
            last = ops.occ_mark_cells(skeys, order, rows, state)
            csum = torch.cumsum(last, 0, dtype=torch.int32)
            classes, _, _ = state.tolist()
            count = int(csum[-1])
            M = len(occ)
            steps = {
                "upload": (lambda: scene._rows(occ), M * 16),
                "keys": (lambda: ops.occ_cell_keys(rows, scene.grid, state), M * (16 + 8)),
                "sort": (lambda: torch.sort(keys, stable=True), 0),
                "mark": (lambda: ops.occ_mark_cells(skeys, order, rows, state), M * (8 + 8 + 4 + 4)),
                "cumsum": (lambda: torch.cumsum(last, 0, dtype=torch.int32), M * 8),
                "write": (lambda: ops.occ_write_gaussians(order, rows, last, csum, count, scene.grid, scene.axes, scene.zscale, classes | 1, 12),
                          M * (8 + 4 + 4) + count * (16 + 26 * 4)),
            }
            for name, (fn, nbytes) in steps.items():
                out[name] = dict(_event_ms(fn, iters), bytes=nbytes)
            out["n"] = count
    print("OCC_BENCH " + json.dumps(out))


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
    mb = lambda b: f"{b / 1e6:.1f} MB"
    lines = [f"occupancy_bench: synthetic surface points, 480 x 640 label image, 400^3 occupancy grid, median of {a.iters} (min .. max), native and "
             "yardstick interleaved; N is an assumption, the reference tree holds no real point cloud"]
    failed = False
    for n in SIZES:
        if failed:
            break
        lines.append(f"N = {n}")
        for step, limit in STEPS:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(n),
                                "--iters", str(a.iters)], capture_output=True, text=True)
            got = [l for l in r.stdout.splitlines() if l.startswith("OCC_BENCH ")]
            if r.returncode != 0 or not got:
                lines.append(f"step {step}: FAILED (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                failed = True                                    # nothing more is started on the GPU after a failing step
                break
            d = json.loads(got[-1][10:])
            if step == "label":
                lines.append(f"  labelling, wall: {d['labelled']} points labelled, {d['differ']} labels differ between the two, "
                             f"resident image gives the same: {d['same_resident']}")
                lines.append("   from the uint8 numpy image (converted and uploaded inside every call, on both sides)")
                lines.append(f"    orv_amd.occupancy.project_labels  {f(d['native'])}   peak {mb(d['peak_native'])}")
                lines.append(f"    torch-ops yardstick, GPU          {f(d['yard'])}   peak {mb(d['peak_yard'])}")
                lines.append("   image resident on the device (uint8 for the kernel, int64 for the torch statements)")
                lines.append(f"    orv_amd.occupancy.project_labels  {f(d['native_r'])}   peak {mb(d['peak_native_r'])}")
                lines.append(f"    torch-ops yardstick, GPU          {f(d['yard_r'])}   peak {mb(d['peak_yard_r'])}")
                lines.append(f"   of the native call, HIP events: kernel {f(d['kernel'])}, torch inverse and product {f(d['matrix'])}")
            elif step == "scene":
                lines.append(f"  scene front, wall, from the numpy rows: M = {d['M']} rows -> n = {d['n']} Gaussians, classes {d['classes']}, same result: {d['same']}")
                lines.append(f"    OccupancyScene.gaussians          {f(d['native'])}   peak {mb(d['peak_native'])}")
                lines.append(f"    dense torch-ops yardstick, GPU    {f(d['yard'])}   peak {mb(d['peak_yard'])} on top of {mb(d['resident_yard'])} resident")
            else:
                lines.append(f"  kernels and torch steps of the scene front, HIP events (M = {d['M']}, n = {d['n']}):")
                for name in ("upload", "keys", "sort", "mark", "cumsum", "write"):
                    k = d[name]
                    rate = f", {k['bytes'] / 1e6:.1f} MB -> {k['bytes'] / k['ms_median'] / 1e6:.0f} GB/s" if k["bytes"] and name != "upload" else ""
                    note = " (numpy float64 rows -> int32 on the device)" if name == "upload" else ""
                    lines.append(f"    {name:<7} {k['ms_median']:.4f} ms ({k['ms_min']:.4f} .. {k['ms_max']:.4f}){rate}{note}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(report + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
