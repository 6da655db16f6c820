"""Developer measurement (not part of any test) of the fused CAME optimizer on one MI355X, one process, interleaved repetitions, medians
(results in profiles/came.txt):

  (a) the seven launches of a step (``orv_came_launch`` which = 0 .. 6) and ``orv_adamw_flat`` (mode 0, the plain bf16 AdamW kernel) on the
      same flat buffers, at the real parameter shapes of the 2B model (all parameters, 1.69 B elements) and at those of its r = 64 adapter,
      device events around every launch, with the achieved bytes per second on the compulsory bytes of the four sweeps:
      q sums g 2; u u sums g 2; m and s sums g 2 + m (4 + 4) = 10; weights m 4 + p (2 + 2) = 8 (mode 0); the AdamW kernel
      g 2 + p (2 + 2) + (m, v) 2 x (4 + 4) = 22.  The three finishing launches move the partial sums only; their bytes are printed.
  (b) the resident optimizer bytes of both (AdamW: m + v; CAME: m + statistics, and its scratch);
  (c) the 2B B = 4 SFT step (``sft.sft_step``, the shape of ``bench.py --mode train``, all parameters trainable) under ``FusedAdamW`` and
      under ``FusedCAME``: two models in the one process, steps alternating.

Usage: python tools/came_time.py [--rounds 15] [--train-rounds 5] [--skip-train] [--skip-full] [--out profiles/came.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16
SWEEP_BYTES = {"q_sums": 2, "usq_sums": 2, "m_and_s_sums": 10, "weights": 8, "adamw": 22}


def model_shapes(r=64):
    """-> (shapes of every parameter of the 2B model, shapes of its r = 64 adapter's parameters)."""
    import bench
    dev = torch.device("cuda:0")
    model = bench.build_model(dict(bench.CFG_2B), dev)
    full = [tuple(p.shape) for p in model.parameters()]
    model.add_adapter(r=r, lora_alpha=r)
    adapter = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    torch.cuda.empty_cache()
    return full, adapter


def time_kernels(what, shapes, rounds, warmup, iters):
    from orv_amd import ops
    dev = torch.device("cuda:0")
    numels = [int(torch.Size(s).numel()) for s in shapes]
    starts, o = [], 0
    for k in numels:
        starts.append(o)
        o += (k + 2047) // 2048 * 2048
    n, nseg = o, len(shapes)
    geo = ops.came_geometry(shapes)
    g = torch.Generator(device=dev).manual_seed(0)
    p = (torch.randn(n, device=dev, generator=g) * 0.02).to(BF)
    grad = (torch.randn(n, device=dev, generator=g) * 1e-3).to(BF)
    m, m2, v2 = (torch.zeros(n, device=dev) for _ in range(3))
    count = {"r": geo["n_rows"], "c": geo["n_cols"], "res_r": geo["n_rows"], "res_c": geo["n_cols"], "v": geo["n_v"]}
    stats = {k: (torch.zeros(c, device=dev) if c else None) for k, c in count.items()}
    scratch = torch.zeros(geo["n_scratch"], device=dev)
    geom = torch.tensor(geo["table"], dtype=torch.int64, device=dev)
    seg_start = torch.tensor(starts + [n], dtype=torch.int64, device=dev)
    active = torch.ones(nseg, dtype=torch.uint8, device=dev)
    seg_step = torch.full((nseg,), 2, dtype=torch.int32, device=dev)
    clip = torch.ones(1, device=dev)
    step = [1]
    came = lambda which: ops.came_step(p, grad, m, stats, seg_start, active, geom, geo, scratch, 1e-5, (0.9, 0.95, 0.98), (1e-30, 1e-16), 1.0,
                                       1e-3, clip, mode=0, which=which)
    legs = {name: (lambda w=i: came(w)) for i, name in enumerate(ops.CAME_LAUNCHES)}
    legs["adamw"] = lambda: ops.adamw_flat(p, grad, m2, v2, seg_start, active, 1e-5, 0.9, 0.95, 1e-8, 1e-3, step[0], clip, seg_step=seg_step)
    for i in range(7):                       # one whole step first: every launch then finds what the launches before it wrote
        came(i)
    times = {k: [] for k in legs}
    for r in range(warmup + rounds):
        for name, fn in legs.items():
            step[0] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1) / iters)
    med = {k: statistics.median(t) for k, t in times.items()}
    finish_bytes = {"statistics": 4 * (geo["n_rowp"] + geo["n_colp"]) + 12 * (geo["n_rows"] + geo["n_cols"]), "k": 4 * geo["n_tiles"],
                    "confidence": 4 * (geo["n_rowp"] + geo["n_colp"]) + 12 * (geo["n_rows"] + geo["n_cols"])}
    lines = [f"{what}: {n} flat elements ({sum(numels)} real) in {nseg} segments, {geo['n_tiles']} tiles, {geo['n_mats']} matrices, {rounds} interleaved "
             f"rounds of {iters} launch(es) after {warmup} warm-up"]
    for k in legs:
        if k in SWEEP_BYTES:
            rate = f"  {SWEEP_BYTES[k]:2d} B/element  {SWEEP_BYTES[k] * n / med[k] / 1e9:.2f} TB/s"
        else:
            rate = f"  {finish_bytes[k] / 1e6:.2f} MB of partial sums and vectors"
        lines.append(f"  {k:13s} median {med[k]:8.4f} ms  (min {min(times[k]):.4f}, max {max(times[k]):.4f}){rate}")
    tot = sum(med[k] for k in ops.CAME_LAUNCHES)
    rate = {k: SWEEP_BYTES[k] * n / med[k] for k in SWEEP_BYTES}
    lines.append(f"  came step (seven launches) {tot:.4f} ms = x{tot / med['adamw']:.3f} of the bf16 AdamW kernel (22 / 22 = 1.000 from the sweeps' traffic "
                 "alone); bytes per second against that kernel: " + ", ".join(f"{k} x{rate[k] / rate['adamw']:.3f}" for k in SWEEP_BYTES if k != "adamw"))
    state = 4 * n + 4 * sum(count.values())
    lines.append(f"  resident optimizer bytes: AdamW m + v {8 * n} ({8 * n / sum(numels):.4f} B / real element); CAME m + statistics {state} "
                 f"({state / sum(numels):.4f}), scratch {4 * geo['n_scratch']} ({4 * geo['n_scratch'] / sum(numels):.4f})")
    del p, grad, m, m2, v2, stats, scratch
    torch.cuda.empty_cache()
    return lines


def time_train(rounds, warm=2, B=4):
    import bench
    from orv_amd import schedulers, sft
    from orv_amd.optim import FusedAdamW, FusedCAME
    dev = torch.device("cuda:0")
    lat, img, prompt, actions = bench.synthetic_inputs(B, dev, BF)
    sched = schedulers.CogVideoXDDIMScheduler(**bench.SCHED)
    batch = sft.Batch(lat, img, prompt, actions, None, None, torch.ones(lat.shape[1], dtype=torch.bool, device=dev), 1)
    legs = {}
    for name in ("adamw", "came"):
        model = bench.build_model(dict(bench.CFG_2B), dev).train()
        model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
        if name == "came":
            opt = FusedCAME(model.parameters(), lr=1e-5, betas=(0.9, 0.95, 0.98), weight_decay=1e-3, max_grad_norm=1.0)
        else:
            opt = FusedAdamW(model.parameters(), lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0)
        legs[name] = (model, opt, torch.Generator(device=dev).manual_seed(42))
    times = {k: [] for k in legs}
    for rnd in range(warm + rounds):
        for name, (model, opt, gen) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = sft.sft_step(model, sched, opt, batch, generator=gen)[0]
            b.record()
            b.synchronize()
            if rnd >= warm:
                times[name].append(a.elapsed_time(b))
    lines = [f"2B B={B} SFT step (sft.sft_step), all {sum(p.numel() for p in legs['came'][1].params)} elements trainable, {rounds} alternating steps "
             f"after {warm} warm-up"]
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in times.items():
        lines.append(f"  {k:6s} median {med[k]:9.2f} ms per step  (min {min(t):.2f}, max {max(t):.2f})")
    state, scratch = legs["came"][1].state_bytes()
    fa = legs["adamw"][1]._flat
    lines.append(f"  came / adamw: x{med['came'] / med['adamw']:.4f};  optimizer state {state / 2**30:.2f} GiB + scratch {scratch / 2**30:.3f} GiB against "
                 f"{(fa['m'].numel() + fa['v'].numel()) * 4 / 2**30:.2f} GiB;  loss {float(loss):.4f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-rounds", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-full", action="store_true", help="time the adapter shapes only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("came_time.py measures on the MI355X only")
    lines = [f"# tools/came_time.py on {torch.cuda.get_device_name(0)}"]
    full, adapter = model_shapes()
    for what, shapes, iters in (("2B model, every parameter", full, 1), ("r = 64 adapter", adapter, 10)):
        if a.skip_full and shapes is full:
            continue
        new = time_kernels(what, shapes, a.rounds, a.warmup, iters)
        lines += new
        print("\n".join(new), flush=True)
    if not a.skip_train:
        new = time_train(a.train_rounds)
        lines += new
        print("\n".join(new), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
