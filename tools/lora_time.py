"""LoRA timings on one MI355X, one process, interleaved repetitions (results in profiles/lora.txt):

  (a) ``orv_gemm_tn_skinny_bf16`` at M = 12904 on (P, Q) = (64, 1920), (1920, 64), (128, 1920), (1920, 128) against ``training._wgrad`` on the
      same operands (two transposes + NT GEMM), with the achieved bytes/s of the compulsory traffic (U + V read once, C written);
  (b) the 2B B = 4 inference forward (bench weights / inputs, eager launches): default, r = 64 adapter unmerged, r = 64 adapter fused;
  (c) the 2B B = 4 SFT step (``sft.sft_step``, the shape of ``bench.py --mode train``) full-parameter against an r = 64 adapter, with peak
      memory, each in a fresh child process (``--leg train-full`` / ``--leg train-lora``) so that the peaks do not mix;
  (d) the adapter gradient-error distribution against oracle autograd: the ``[lora-grad-err]`` lines of tests/test_gpu_lora.py, run as a child.

Usage: python tools/lora_time.py [--reps 7] [--iters 20] [--out profiles/lora.txt] [--skip-train] [--skip-forward] [--skip-grad-err]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def time_kernel(reps, iters, M=12904):
    from orv_amd import ops, training
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for P, Q in ((64, 1920), (1920, 64), (128, 1920), (1920, 128)):
        U = torch.randn(M, P, device=dev, generator=g).to(BF)
        V = torch.randn(M, Q, device=dev, generator=g).to(BF)
        C1, C2 = torch.empty(P, Q, dtype=BF, device=dev), torch.empty(P, Q, dtype=BF, device=dev)
        scratch = torch.empty(ops.gemm_tn_skinny_scratch(M, P, Q), dtype=torch.uint8, device=dev)
        f_new = lambda: ops.gemm_tn_skinny(U, V, C1, M, P, Q, scratch=scratch)
        f_old = lambda: training._wgrad(U, V, C2, M, P, Q, accumulate=False)
        for f in (f_new, f_old):
            _time(f, 3)
        t = {"skinny": [], "wgrad": []}
        for _ in range(reps):
            t["skinny"].append(_time(f_new, iters))
            t["wgrad"].append(_time(f_old, iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        nbytes = 2.0 * (M * P + M * Q + P * Q)
        ref = U.double().T @ V.double()
        rows.append(dict(M=M, P=P, Q=Q, skinny_ms=round(med["skinny"], 4), wgrad_ms=round(med["wgrad"], 4),
                         speedup=round(med["wgrad"] / med["skinny"], 2), skinny_tb_per_s=round(nbytes / med["skinny"] / 1e9, 2),
                         ln_mod_rows_tb_per_s=4.9, scratch_mb=round(scratch.numel() / 2 ** 20, 1),
                         spread_skinny=[round(min(t["skinny"]), 4), round(max(t["skinny"]), 4)],
                         spread_wgrad=[round(min(t["wgrad"]), 4), round(max(t["wgrad"]), 4)],
                         max_abs_diff_vs_fp64=[round(float((C1.double() - ref).abs().max()), 3), round(float((C2.double() - ref).abs().max()), 3)]))
        print(json.dumps(rows[-1]), flush=True)
        del U, V, C1, C2, scratch, ref
        torch.cuda.empty_cache()
    return rows


def _adapter(model, r=64, seed=0):
    model.add_adapter(r=r, lora_alpha=r)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for A, B in model._lora_adapters["default"].params.values():
            B.copy_((0.01 * torch.randn(B.shape, generator=g)).to(B.device, BF))


def time_forward(reps, iters, B=4):
    import bench
    dev = torch.device("cuda:0")
    model = bench.build_model(dict(bench.CFG_2B), dev)
    lat, img, prompt, actions = bench.synthetic_inputs(B, dev, BF)
    x = torch.cat([lat, img], dim=2)
    ts = torch.full((B,), 500, device=dev)
    model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
    run = lambda: model(x, prompt, {"actions": actions}, ts, return_dict=False)
    _adapter(model)
    modes = ("default", "unmerged", "fused")

    def switch(mode):
        model.unfuse_lora()
        if mode == "default":
            model.disable_adapters()
        else:
            model.enable_adapters()
            if mode == "fused":
                model.fuse_lora()
    res = {m: [] for m in modes}
    with torch.no_grad():
        for mode in modes:
            switch(mode)
            _time(run, 2)
        for _ in range(reps):
            for mode in modes:
                switch(mode)
                _time(run, 1)
                res[mode].append(_time(run, iters))
    med = {k: statistics.median(v) for k, v in res.items()}
    row = dict(config=f"2B B={B} forward (eager), r=64 adapter on to_q/to_k/to_v/to_out.0", **{f"{k}_ms": round(v, 2) for k, v in med.items()},
               unmerged_over_default=round(med["unmerged"] / med["default"], 3), fused_over_default=round(med["fused"] / med["default"], 4),
               **{f"all_{k}": [round(v, 2) for v in res[k]] for k in modes})
    print(json.dumps(row), flush=True)
    return row


def train_leg(lora, steps=4, warm=2, B=4):
    import bench
    from orv_amd import schedulers, sft
    from orv_amd.optim import FusedAdamW
    dev = torch.device("cuda:0")
    model = bench.build_model(dict(bench.CFG_2B), dev).train()
    model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
    if lora:
        _adapter(model, lora)
    lat, img, prompt, actions = bench.synthetic_inputs(B, dev, BF)
    sched = schedulers.CogVideoXDDIMScheduler(**bench.SCHED)
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0,
                     param_precision="split_fp32" if lora else "bf16")
    batch = sft.Batch(lat, img, prompt, actions, None, None, torch.ones(lat.shape[1], dtype=torch.bool, device=dev), 1)
    g = torch.Generator(device=dev).manual_seed(42)
    torch.cuda.reset_peak_memory_stats()
    for _ in range(warm):
        sft.sft_step(model, sched, opt, batch, generator=g)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        loss = sft.sft_step(model, sched, opt, batch, generator=g)[0]
    b.record()
    b.synchronize()
    row = dict(leg="train-lora" if lora else "train-full", rank=lora, batch=B, ms_per_step=round(a.elapsed_time(b) / steps, 2),
               peak_allocated_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), trainable_params=sum(p.numel() for p in opt.params),
               optimizer_param_precision=opt.param_precision, final_loss=round(float(loss), 5))
    print("LEG " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fwd-reps", type=int, default=5)
    ap.add_argument("--fwd-iters", type=int, default=3)
    ap.add_argument("--train-rounds", type=int, default=2)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--skip-grad-err", action="store_true")
    ap.add_argument("--leg", default=None, choices=["train-full", "train-lora"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_time.py needs the MI355X")
    if a.leg:
        train_leg(64 if a.leg == "train-lora" else 0)
        return
    res = {"device": torch.cuda.get_device_name(0), "kernel": time_kernel(a.reps, a.iters)}
    if not a.skip_forward:
        res["forward"] = time_forward(a.fwd_reps, a.fwd_iters)
    if not a.skip_train:
        # fresh child processes (peak memory per leg), alternating full / adapter
        legs = []
        for _ in range(a.train_rounds):
            for leg in ("train-full", "train-lora"):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], check=True, capture_output=True, text=True,
                                     timeout=600).stdout
                legs += [json.loads(l[4:]) for l in out.splitlines() if l.startswith("LEG ")]
                print(json.dumps(legs[-1]), flush=True)
        res["train"] = legs
    if not a.skip_grad_err:
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lora.py"), "-k", "adapter_gradients", "-s", "-q",
                              "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=600, cwd=ROOT).stdout
        res["grad_err"] = [l[l.index("[lora-grad-err]"):] for l in out.splitlines() if "[lora-grad-err]" in l] + \
                          [l for l in out.splitlines()[-1:] if "passed" in l or "failed" in l]
        print("\n".join(res["grad_err"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/lora_time.py on " + res["device"] + "\n")
            for sec in ("kernel", "forward", "train"):
                if sec in res:
                    f.write(f"## {sec}\n")
                    for row in (res[sec] if isinstance(res[sec], list) else [res[sec]]):
                        f.write(json.dumps(row) + "\n")
            if "grad_err" in res:
                f.write("## gradient error (rel-L2 of every adapter tensor's gradient against fp32 oracle autograd, bound 3e-2)\n")
                f.write("\n".join(res["grad_err"]) + "\n")


if __name__ == "__main__":
    main()
