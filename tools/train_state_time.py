"""Developer measurement (not part of any test) of ``orv_amd.train_state`` on one MI355X at the 2B training shape with FusedAdamW and a
FusedEMA, one process, interleaved repetitions, medians (results in profiles/train_state.txt):

  (a) how long ``save_state(blocking=False)`` holds the training stream (device events around the call, and the host time of the call),
      against what a user can do without it, written with torch calls only: ``model.save_pretrained`` plus ``.cpu()`` of every tensor of
      the optimizer's and the EMA's ``state_dict()``;
  (b) the snapshot kernel's bytes per second (2 x bytes: read + write) over the tensors of that state, against ``Tensor.copy_`` device to
      device over the same buffers (2 x bytes), against ``copy_`` plus a separate ``ops.checksum`` pass (3 x bytes moved for the same
      result), and against ``orv_adamw_flat`` on the optimizer's flat buffers (22 bytes per element);
  (c) three consecutive ``sft_step`` calls without and with a write in flight;
  (d) the wall time from the call to the rename.

Usage: python tools/train_state_time.py [--rounds 7] [--saves 3] [--out profiles/train_state.txt] [--dir /tmp/orv_train_state]"""
import argparse
import os
import shutil
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--saves", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/orv_train_state")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_state_time.py measures on the MI355X only")
    import bench
    from orv_amd import FusedEMA, ops, schedulers, sft, train_state
    from orv_amd.optim import FusedAdamW
    dev, B = torch.device("cuda:0"), 4
    lat, img, prompt, actions = bench.synthetic_inputs(B, dev, BF)
    sched = schedulers.CogVideoXDDIMScheduler(**bench.SCHED)
    batch = sft.Batch(lat, img, prompt, actions, None, None, torch.ones(lat.shape[1], dtype=torch.bool, device=dev), 1)
    model = bench.build_model(dict(bench.CFG_2B), dev).train()
    model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
    opt = FusedAdamW(model.parameters(), lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0)
    ema = FusedEMA(opt)
    gen = torch.Generator(device=dev).manual_seed(42)
    step = lambda: sft.sft_step(model, sched, opt, batch, generator=gen, ema=ema)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    lines = [f"# tools/train_state_time.py on {torch.cuda.get_device_name(0)}: 2B, B = {B}, FusedAdamW (bf16, fp32 moments) + FusedEMA"]

    # (b) the kernels, on the tensors save_state walks
    groups, _ = train_state._walk(model, opt, ema)
    tensors = [t for named in groups.values() for t, copy in named.values() if copy]
    nbytes = sum(t.numel() * t.element_size() for t in tensors)
    copies = [torch.empty_like(t) for t in tensors]
    f = opt._flat
    clip = torch.ones(1, device=dev)
    legs = {
        "snapshot (copy + sums)": (2 * nbytes, lambda: ops.snapshot_into(tensors, copies)),
        "Tensor.copy_ per tensor": (2 * nbytes, lambda: [c.copy_(t) for c, t in zip(copies, tensors)]),
        "torch._foreach_copy_": (2 * nbytes, lambda: torch._foreach_copy_(copies, tensors)),
        "copy_ + ops.checksum": (3 * nbytes, lambda: ([c.copy_(t) for c, t in zip(copies, tensors)], ops.checksum(tensors))),
        "ops.checksum alone": (nbytes, lambda: ops.checksum(tensors)),
        "orv_adamw_flat": (22 * f["p"].numel(), lambda: ops.adamw_flat(f["p"], f["g"], f["m"], f["v"], f["seg_start"], f["active"], 0.0, 0.9, 0.95,
                                                                        1e-8, 0.0, 3, clip, seg_step=f["seg_step"])),
    }
    f["g"].zero_()                                    # lr 0, no decay, zero gradient: the AdamW leg leaves the weights alone
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.rounds):
        for name, (_, fn) in legs.items():
            ms, _ = _event_ms(fn)
            if r >= a.warmup:
                times[name].append(ms)
    lines.append(f"[kernels] {len(tensors)} tensors, {nbytes / 2 ** 30:.2f} GiB of state; {a.rounds} interleaved rounds after {a.warmup} warm-up, device events")
    for name, (moved, _) in legs.items():
        med = statistics.median(times[name])
        lines.append(f"  {name:26s} median {med:9.3f} ms  (min {min(times[name]):.3f}, max {max(times[name]):.3f})  {moved / med / 1e9:6.2f} TB/s "
                     f"on {moved / 2 ** 30:.1f} GiB moved")
    del copies
    torch.cuda.empty_cache()
    print("\n".join(lines), flush=True)

    # (a), (d): the save, against the torch-only way
    shutil.rmtree(a.dir, ignore_errors=True)
    hold, host, whole = [], [], []
    for i in range(a.saves):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms, handle = _event_ms(lambda: train_state.save_state(a.dir, i, model=model, optimizer=opt, ema=ema, generator=gen, total_limit=1))
        host.append((time.perf_counter() - t0) * 1e3)
        hold.append(ms)
        handle.wait()
        whole.append((time.perf_counter() - t0) * 1e3)
    naive = []
    for i in range(max(1, a.saves - 1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.save_pretrained(os.path.join(a.dir, "naive", "transformer"))
        kept = [t.cpu() for t in train_state.split_state(opt.state_dict())[0].values()]
        kept += [t.cpu() for t in train_state.split_state(ema.state_dict())[0].values()]
        torch.cuda.synchronize()
        naive.append((time.perf_counter() - t0) * 1e3)
        del kept
    size = sum(os.path.getsize(os.path.join(b, n)) for b, _, names in os.walk(train_state.latest_checkpoint(a.dir)) for n in names)
    new = [f"[save] {a.saves} saves of {size / 2 ** 30:.2f} GiB to {a.dir}",
           f"  save_state(blocking=False) holds the training stream  median {statistics.median(hold):9.2f} ms  (all: {', '.join(f'{x:.2f}' for x in hold)})",
           f"  host time of the call                                 median {statistics.median(host):9.2f} ms",
           f"  wall time from the call to the rename                 median {statistics.median(whole) / 1e3:9.2f} s",
           f"  torch only: save_pretrained + .cpu() of every state tensor, the loop waits  median {statistics.median(naive) / 1e3:9.2f} s "
           f"(all: {', '.join(f'{x / 1e3:.2f}' for x in naive)})"]
    lines += new
    print("\n".join(new), flush=True)

    # (c) three steps without and with a write in flight
    def three():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    quiet, busy = [], []
    for i in range(a.saves):
        quiet.append(three())
        handle = train_state.save_state(a.dir, 100 + i, model=model, optimizer=opt, ema=ema, generator=gen, total_limit=1)
        busy.append(three())
        in_flight = not handle.done
        handle.wait()
    new = [f"[steps] three consecutive sft_step calls, {a.saves} alternating rounds",
           f"  no write in flight   median {statistics.median(quiet):9.2f} ms  (all: {', '.join(f'{x:.1f}' for x in quiet)})",
           f"  a write in flight    median {statistics.median(busy):9.2f} ms  (all: {', '.join(f'{x:.1f}' for x in busy)}); includes the snapshot; "
           f"the writer was {'still' if in_flight else 'NOT'} writing when the last three ended"]
    lines += new
    print("\n".join(new), flush=True)
    shutil.rmtree(a.dir, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
