"""Developer measurement (not part of any test) of the fused Prodigy optimizer on one MI355X, one process, interleaved repetitions, medians
(results in profiles/prodigy.txt):

  (a) the three launches of a step (``orv_prodigy_moments`` / ``_recurrence`` / ``_update``) and ``orv_adamw_flat_ex`` mode 1 (the split-fp32
      AdamW kernel) at the flat size of the 2B model and at that of an r = 64 adapter, device events around every launch, with the achieved
      bytes per second on the compulsory bytes: launch 1 g 2 + p 2 + lo 2 + p0 2 + (m, v, s) 3 x (4 + 4) = 32 B per element, launch 3
      p (2 + 2) + lo (2 + 2) + m 4 + v 4 = 16, the AdamW kernel 26;
  (b) the 2B B = 4 SFT step (``sft.sft_step``, the shape of ``bench.py --mode train``) with an r = 64 adapter under
      ``FusedAdamW(param_precision="split_fp32")`` and under ``FusedProdigy``: two models in the one process, steps alternating.

Usage: python tools/prodigy_time.py [--elements 1690000000 29500000] [--rounds 15] [--train-rounds 5] [--skip-train] [--out profiles/prodigy.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16
BYTES = {"moments": 32, "update": 16, "adamw_ex1": 26}


def time_kernels(n, segments, rounds, warmup, iters):
    from orv_amd import ops
    dev = torch.device("cuda:0")
    n = n // 2048 * 2048
    per = max(1, n // 2048 // segments) * 2048
    starts = list(range(0, n, per))[:segments]
    nseg = len(starts)
    starts.append(n)
    g = torch.Generator(device=dev).manual_seed(0)
    p = (torch.randn(n, device=dev, generator=g) * 0.02).to(BF)
    grad = (torch.randn(n, device=dev, generator=g) * 1e-3).to(BF)
    lo, p0 = torch.zeros(n, dtype=torch.int16, device=dev), p.clone()
    m, v, s, m2, v2 = (torch.zeros(n, device=dev) for _ in range(5))
    seg_start = torch.tensor(starts, dtype=torch.int64, device=dev)
    active = torch.ones(nseg, dtype=torch.uint8, device=dev)
    seg_step = torch.full((nseg,), 2, dtype=torch.int32, device=dev)
    state = torch.tensor([1e-6, 1e-6, 0, 0, 0, 1, 0, 0], dtype=torch.float64, device=dev)
    partials = torch.zeros(2 * (n // 2048), dtype=torch.float64, device=dev)
    clip = torch.ones(1, device=dev)
    step = [1]
    legs = {
        "moments": lambda: ops.prodigy_moments(p, lo, grad, p0, m, v, s, seg_start, active, seg_step, state, partials, 1.0, 0.9, 0.95, 0.98,
                                               0.0, True, False, False, 1e-6, clip),
        "recurrence": lambda: ops.prodigy_recurrence(state, partials, 1.0, 0.9, 0.95, 0.98, False, 1e-6, 1.0, float("inf")),
        "update": lambda: ops.prodigy_update(p, lo, m, v, seg_start, active, state, 1e-8, 0.0, True),
        "adamw_ex1": lambda: ops.adamw_flat_ex(p, grad, m2, v2, seg_start, active, 1e-5, 0.9, 0.95, 1e-8, 1e-3, step[0], clip,
                                               seg_step=seg_step, lo=lo, mode=1),
    }
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
    lines = [f"{n} elements in {nseg} segments ({n // 2048} chunks), {rounds} interleaved rounds of {iters} launch(es) after {warmup} warm-up"]
    for k in legs:
        rate = f"  {BYTES[k]} B/element  {BYTES[k] * n / med[k] / 1e9:.2f} TB/s" if k in BYTES else f"  {16 * (n // 2048) / 1e6:.2f} MB of partials"
        lines.append(f"  {k:11s} median {med[k]:8.4f} ms  (min {min(times[k]):.4f}, max {max(times[k]):.4f}){rate}")
    tot = med["moments"] + med["recurrence"] + med["update"]
    rate = {k: BYTES[k] * n / med[k] for k in BYTES}
    lines.append(f"  prodigy step (three launches) {tot:.4f} ms = x{tot / med['adamw_ex1']:.3f} of the split-fp32 AdamW kernel (48 / 26 = 1.846 from "
                 f"traffic alone); bytes per second against that kernel: moments x{rate['moments'] / rate['adamw_ex1']:.3f}, "
                 f"update x{rate['update'] / rate['adamw_ex1']:.3f}")
    del p, grad, lo, p0, m, v, s, m2, v2, partials
    torch.cuda.empty_cache()
    return lines


def time_train(rounds, warm=2, B=4, r=64):
    import bench
    from orv_amd import schedulers, sft
    from orv_amd.optim import FusedAdamW, FusedProdigy
    dev = torch.device("cuda:0")
    lat, img, prompt, actions = bench.synthetic_inputs(B, dev, BF)
    sched = schedulers.CogVideoXDDIMScheduler(**bench.SCHED)
    batch = sft.Batch(lat, img, prompt, actions, None, None, torch.ones(lat.shape[1], dtype=torch.bool, device=dev), 1)
    legs = {}
    for name in ("adamw_split_fp32", "prodigy"):
        model = bench.build_model(dict(bench.CFG_2B), dev).train()
        model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
        model.add_adapter(r=r, lora_alpha=r)
        params = [p for p in model.parameters() if p.requires_grad]
        if name == "prodigy":
            opt = FusedProdigy(params, lr=1.0, betas=(0.9, 0.95), beta3=0.98, weight_decay=1e-3, max_grad_norm=1.0)
        else:
            opt = FusedAdamW(params, lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0, param_precision="split_fp32")
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
    lines = [f"2B B={B} SFT step (sft.sft_step), r={r} adapter, {sum(p.numel() for p in legs['prodigy'][1].params)} trainable elements, "
             f"{rounds} alternating steps after {warm} warm-up"]
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in times.items():
        lines.append(f"  {k:17s} median {med[k]:9.2f} ms per step  (min {min(t):.2f}, max {max(t):.2f})")
    opt = legs["prodigy"][1]
    lines.append(f"  prodigy / adamw: x{med['prodigy'] / med['adamw_split_fp32']:.4f};  after {warm + rounds} steps d = {opt.d:.3e}, k = {opt.k}, "
                 f"loss {float(loss):.4f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, nargs="+", default=[1_690_000_000, 29_500_000])
    ap.add_argument("--segments", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-rounds", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prodigy_time.py measures on the MI355X only")
    lines = [f"# tools/prodigy_time.py on {torch.cuda.get_device_name(0)}"]
    for n in a.elements:
        new = time_kernels(n, a.segments, a.rounds, a.warmup, iters=1 if n > 200_000_000 else 10)
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
