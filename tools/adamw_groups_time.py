"""Developer measurement (not part of any test) of FusedAdamW's parameter groups and step guard on one MI355X, one process, interleaved
repetitions, medians (results in profiles/adamw_groups.txt).  Everything runs on the REAL flat buffers of the 2B model
with every parameter trainable (``FusedAdamW`` over ``bench.build_model``: 741 segments padded to 2048):

  (a) ``orv_adamw_flat_groups`` at one and at three groups (segment i in group i % 3) against ``orv_adamw_flat_ex``, the parent, which is
      timed TWICE in the same rotation so that its own run-to-run spread is on the page; the same for the fp8-moment pair
      (``orv_adamw_flat_s8_groups`` / ``orv_adamw_flat_s8``), which is also timed with the per-segment step counts behind the host's
      count, as they are after a skipped step.  Device events around every launch;
  (b) ``orv_segment_sumsq`` + ``orv_step_guard`` against what they replace: a zeroed scalar, ``orv_sumsq`` and the torch clip arithmetic;
  (c) the 2B B = 4 SFT step (``sft.sft_step``, the shape of ``bench.py --mode train``) with one group and with ``named_groups``.

Usage: python tools/adamw_groups_time.py [--rounds 20] [--train-rounds 5] [--skip-train] [--out profiles/adamw_groups.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16
HYPER = (0.9, 0.95, 1e-8)


def _rotate(legs, rounds, warmup):
    times = {k: [] for k in legs}
    for r in range(warmup + rounds):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return times


def _report(title, times, base):
    med = {k: statistics.median(t) for k, t in times.items()}
    lines = [title]
    for k, t in times.items():
        lines.append(f"  {k:24s} median {med[k]:8.4f} ms  (min {min(t):.4f}, max {max(t):.4f})  x{med[k] / med[base]:.4f} of {base}")
    return lines


def time_kernels(opt, rounds, warmup):
    from orv_amd import ops
    f = opt._flat
    dev, n, nseg = f["p"].device, f["p"].numel(), f["active"].numel()
    gen = torch.Generator(device=dev).manual_seed(0)
    f["g"][:n].copy_((torch.randn(n, device=dev, generator=gen) * 1e-3).to(BF))
    active = torch.ones(nseg, dtype=torch.uint8, device=dev)
    seg_step = torch.ones(nseg, dtype=torch.int32, device=dev)
    clip = torch.ones(1, device=dev)
    one = torch.zeros(nseg, dtype=torch.uint8, device=dev)
    three = (torch.arange(nseg, device=dev) % 3).to(torch.uint8)
    lr, wd = 1e-5, 1e-3
    lines = [f"[layout] {n} flat elements in {nseg} segments (the 2B model, every parameter trainable)"]
    for mode in ("bf16", "stochastic"):
        a = (f["p"], f["g"], f["m"], f["v"], f["seg_start"], active)
        kw = dict(seg_step=seg_step, mode=mode, seed=1)
        legs = {
            "parent": lambda: ops.adamw_flat_ex(*a, lr, *HYPER[:2], HYPER[2], wd, 1, clip, **kw),
            "groups, 1 group": lambda: ops.adamw_flat_groups(*a, one, [lr], [wd], *HYPER, 1, clip, max_group=0, **kw),
            "groups, 3 groups": lambda: ops.adamw_flat_groups(*a, three, [lr, 2 * lr, 3 * lr], [wd, 0.0, wd], *HYPER, 1, clip, max_group=2, **kw),
            "parent again": lambda: ops.adamw_flat_ex(*a, lr, *HYPER[:2], HYPER[2], wd, 1, clip, **kw),
        }
        lines += _report(f"[update, fp32 moments, mode {mode}] {rounds} interleaved rounds of 1 launch after {warmup} warm-up",
                         _rotate(legs, rounds, warmup), "parent")
    z8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)
    s8 = (z8(n), z8(n), z8(n // 256), z8(n // 256))
    a = (f["p"], f["g"], *s8, f["seg_start"], active)
    kw = dict(seg_step=seg_step, mode="bf16", seed=1)
    legs = {
        "parent": lambda: ops.adamw_flat_s8(*a, lr, *HYPER[:2], HYPER[2], wd, 1, clip, **kw),
        "groups, 1 group": lambda: ops.adamw_flat_s8_groups(*a, one, [lr], [wd], *HYPER, 1, clip, max_group=0, **kw),
        "groups, 3 groups": lambda: ops.adamw_flat_s8_groups(*a, three, [lr, 2 * lr, 3 * lr], [wd, 0.0, wd], *HYPER, 1, clip, max_group=2, **kw),
        "parent again": lambda: ops.adamw_flat_s8(*a, lr, *HYPER[:2], HYPER[2], wd, 1, clip, **kw),
        # per-segment counts behind the entry's `step`, as after a skipped step: the kernel takes its own bias corrections (two powf per
        # lane) instead of the host's - parent and group kernel alike
        "parent, counts behind": lambda: ops.adamw_flat_s8(*a, lr, *HYPER[:2], HYPER[2], wd, 2, clip, **kw),
        "groups, counts behind": lambda: ops.adamw_flat_s8_groups(*a, three, [lr, 2 * lr, 3 * lr], [wd, 0.0, wd], *HYPER, 2, clip, max_group=2, **kw),
        # ... which the group entry's common_count argument gives back (FusedAdamW passes step_count - skipped_steps)
        "groups, common_count": lambda: ops.adamw_flat_s8_groups(*a, three, [lr, 2 * lr, 3 * lr], [wd, 0.0, wd], *HYPER, 2, clip, max_group=2,
                                                                 common_count=1, **kw),
    }
    lines += _report(f"[update, fp8 moments, mode bf16] {rounds} interleaved rounds of 1 launch after {warmup} warm-up",
                     _rotate(legs, rounds, warmup), "parent")
    del s8, a, legs
    seg_ss = torch.zeros(nseg, dtype=torch.float64, device=dev)
    report = torch.zeros(len(ops.GUARD_REPORT), dtype=torch.float64, device=dev)
    coef = torch.zeros(1, device=dev)

    def scalar_path():
        ss = torch.zeros(1, dtype=torch.float32, device=dev)
        ops.sumsq(f["g_params"], ss)
        norm = ss.sqrt() / 1
        return torch.clamp(1.0 / (norm + 1e-6), max=1.0)

    def guarded_path():
        ops.segment_sumsq(f["g"], f["seg_start"], seg_ss)
        ops.step_guard(seg_ss, three, active, coef, report, 1.0, 1.0, True)

    legs = {"sumsq + torch clip": scalar_path, "segment_sumsq + guard": guarded_path,
            "segment_sumsq alone": lambda: ops.segment_sumsq(f["g"], f["seg_start"], seg_ss),
            "guard alone": lambda: ops.step_guard(seg_ss, three, active, coef, report, 1.0, 1.0, True)}
    lines += _report(f"[norm and clip coefficient] {rounds} interleaved rounds after {warmup} warm-up", _rotate(legs, rounds, warmup),
                     "sumsq + torch clip")
    largest = int((f["seg_start"][1:] - f["seg_start"][:-1]).max())
    lines.append(f"  (one workgroup per segment; the largest segment holds {largest} elements = {2 * largest / 2 ** 20:.1f} MiB)")
    return lines


def time_train(model, make_opt, rounds, warm=2, B=4):
    import bench
    from orv_amd import schedulers, sft
    dev = torch.device("cuda:0")
    lat, img, prompt, actions = bench.synthetic_inputs(B, dev, BF)
    sched = schedulers.CogVideoXDDIMScheduler(**bench.SCHED)
    batch = sft.Batch(lat, img, prompt, actions, None, None, torch.ones(lat.shape[1], dtype=torch.bool, device=dev), 1)
    gen = torch.Generator(device=dev).manual_seed(42)
    times, info = {}, {}
    for name in ("one group", "named_groups", "one group again"):
        opt = make_opt(name)
        times[name] = []
        for rnd in range(warm + rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = sft.sft_step(model, sched, opt, batch, generator=gen)[0]
            b.record()
            b.synchronize()
            if rnd >= warm:
                times[name].append(a.elapsed_time(b))
        info[name] = f"{len(opt.param_groups)} group(s) {[g['name'] for g in opt.param_groups]}, loss {float(loss):.4f}"
        del opt
        torch.cuda.empty_cache()
    lines = _report(f"[sft step] 2B B={B} (sft.sft_step), {rounds} steps after {warm} warm-up per optimizer, built one after the other",
                    times, "one group")
    return lines + [f"  {k}: {v}" for k, v in info.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-rounds", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_groups_time.py measures on the MI355X only")
    import bench
    from orv_amd.optim import FusedAdamW, named_groups
    dev = torch.device("cuda:0")
    model = bench.build_model(dict(bench.CFG_2B), dev).train()
    model.action_embed.forced_mask = torch.zeros(4, dtype=torch.bool)
    common = dict(lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0)
    lines = [f"# tools/adamw_groups_time.py on {torch.cuda.get_device_name(0)}"]
    opt = FusedAdamW(model.parameters(), **common)
    opt._build()
    new = time_kernels(opt, a.rounds, a.warmup)
    del opt
    torch.cuda.empty_cache()
    lines += new
    print("\n".join(new), flush=True)
    if not a.skip_train:
        def make_opt(name):
            if name == "named_groups":
                groups = named_groups(model, weight_decay=1e-3, lr_overrides={"action_embed": 5e-5, "action_recon": 5e-5})
                return FusedAdamW(groups, **common)
            return FusedAdamW(model.parameters(), **common)
        new = time_train(model, make_opt, a.train_rounds)
        lines += new
        print("\n".join(new), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
