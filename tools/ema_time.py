"""Developer measurement (not part of any test) of ``orv_amd.FusedEMA`` on one MI355X, one process, interleaved repetitions, medians
(results in profiles/ema.txt):

  (a) ``orv_ema_update`` and ``orv_ema_swap_in`` (store-and-write form), each without and with low halves, and ``orv_adamw_flat`` (the plain
      bf16 AdamW kernel) on the same flat buffers at the size of the 2B model with every parameter trainable, device events around every
      launch, with the achieved bytes per second on the compulsory bytes: update s (4 + 4) + p 2 = 10, + lo 2 = 12; swap-in s 4 + p (2 + 2) +
      stash 2 = 10, + lo 2 + stash 2 = 14; AdamW g 2 + p (2 + 2) + (m, v) 2 x (4 + 4) = 22;
  (b) the 2B B = 4 SFT step (``sft.sft_step``, the shape of ``bench.py --mode train``, all parameters trainable) without and with ``ema=``:
      one model and optimizer, steps alternating;
  (c) peak device memory of that step before a ``FusedEMA`` exists, with one, and inside ``average_parameters()``.

Usage: python tools/ema_time.py [--rounds 15] [--train-rounds 5] [--skip-train] [--elements N] [--out profiles/ema.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16
BYTES = {"ema_update": 10, "ema_update_lo": 12, "ema_swap_in": 10, "ema_swap_in_lo": 14, "adamw": 22}
N_2B = 1695358976          # flat elements of the 2B model with every parameter trainable (741 segments padded to 2048; profiles/came.txt)


def time_kernels(n, rounds, warmup):
    from orv_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    p = (torch.randn(n, device=dev, generator=g) * 0.02).to(BF)
    grad = (torch.randn(n, device=dev, generator=g) * 1e-3).to(BF)
    lo = torch.randint(-32768, 32768, (n,), device=dev, generator=g, dtype=torch.int32).to(torch.int16)
    shadow = p.float()
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    stash_p, stash_lo = torch.empty_like(p), torch.empty_like(lo)
    seg_start = torch.tensor([0, n], dtype=torch.int64, device=dev)
    active = torch.ones(1, dtype=torch.uint8, device=dev)
    clip = torch.ones(1, device=dev)
    step = [1]
    legs = {
        "ema_update": lambda: ops.ema_update(shadow, p, None, 1e-4),
        "ema_update_lo": lambda: ops.ema_update(shadow, p, lo, 1e-4),
        "ema_swap_in": lambda: ops.ema_swap_in(p, shadow, None, stash_p=stash_p),
        "ema_swap_in_lo": lambda: ops.ema_swap_in(p, shadow, lo, stash_p=stash_p, stash_lo=stash_lo),
        "adamw": lambda: ops.adamw_flat(p, grad, m, v, seg_start, active, 1e-5, 0.9, 0.95, 1e-8, 1e-3, step[0], clip),
    }
    times = {k: [] for k in legs}
    for r in range(warmup + rounds):
        for name, fn in legs.items():
            step[0] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(t) for k, t in times.items()}
    rate = {k: BYTES[k] * n / med[k] / 1e9 for k in legs}
    lines = [f"[kernels] {n} flat elements, {rounds} interleaved rounds of 1 launch after {warmup} warm-up"]
    for k in legs:
        lines.append(f"  {k:15s} median {med[k]:8.4f} ms  (min {min(times[k]):.4f}, max {max(times[k]):.4f})  {BYTES[k]:2d} B/element  "
                     f"{rate[k]:.2f} TB/s  x{rate[k] / rate['adamw']:.3f} of the AdamW kernel's bytes per second")
    del p, grad, lo, shadow, m, v, stash_p, stash_lo
    torch.cuda.empty_cache()
    return lines


def time_train(rounds, warm=2, B=4):
    import bench
    from orv_amd import FusedEMA, schedulers, sft
    from orv_amd.optim import FusedAdamW
    dev = torch.device("cuda:0")
    lat, img, prompt, actions = bench.synthetic_inputs(B, dev, BF)
    sched = schedulers.CogVideoXDDIMScheduler(**bench.SCHED)
    batch = sft.Batch(lat, img, prompt, actions, None, None, torch.ones(lat.shape[1], dtype=torch.bool, device=dev), 1)
    model = bench.build_model(dict(bench.CFG_2B), dev).train()
    model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
    opt = FusedAdamW(model.parameters(), lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0)
    gen = torch.Generator(device=dev).manual_seed(42)
    gib = lambda b: b / 2 ** 30

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()

    for _ in range(warm):
        sft.sft_step(model, sched, opt, batch, generator=gen)
    peak_plain = peak_of(lambda: sft.sft_step(model, sched, opt, batch, generator=gen))
    resident = torch.cuda.memory_allocated()
    ema = FusedEMA(opt)
    torch.cuda.synchronize()
    shadow_bytes = torch.cuda.memory_allocated() - resident
    peak_ema = peak_of(lambda: sft.sft_step(model, sched, opt, batch, generator=gen, ema=ema))

    def swapped():
        with ema.average_parameters():
            pass
    peak_swap = peak_of(swapped) - torch.cuda.memory_allocated()
    times = {"plain": [], "ema": []}
    for rnd in range(warm + rounds):
        for name in times:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = sft.sft_step(model, sched, opt, batch, generator=gen, ema=ema if name == "ema" else None)[0]
            b.record()
            b.synchronize()
            if rnd >= warm:
                times[name].append(a.elapsed_time(b))
    med = {k: statistics.median(t) for k, t in times.items()}
    n_real = sum(p.numel() for p in opt.params)
    lines = [f"[sft step] 2B B={B} (sft.sft_step), all {n_real} elements trainable, {rounds} alternating steps after {warm} warm-up"]
    for k, t in times.items():
        lines.append(f"  {k:6s} median {med[k]:9.2f} ms per step  (min {min(t):.2f}, max {max(t):.2f})")
    lines.append(f"  ema / plain: x{med['ema'] / med['plain']:.4f} (+{med['ema'] - med['plain']:.2f} ms);  loss {float(loss):.4f}")
    lines.append("[memory] torch.cuda.max_memory_allocated of one step")
    lines.append(f"  before a FusedEMA exists {gib(peak_plain):8.2f} GiB;  with one {gib(peak_ema):8.2f} GiB  (+{gib(peak_ema - peak_plain):.2f} GiB)")
    lines.append(f"  the shadow {gib(shadow_bytes):.2f} GiB = {shadow_bytes / n_real:.4f} B / real element;  stash inside average_parameters() "
                 f"+{gib(peak_swap):.2f} GiB")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-rounds", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--elements", type=int, default=N_2B, help="flat elements of the kernel section (a multiple of 2048)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_time.py measures on the MI355X only")
    lines = [f"# tools/ema_time.py on {torch.cuda.get_device_name(0)}"]
    new = time_kernels(a.elements, a.rounds, a.warmup)
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
