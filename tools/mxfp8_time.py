"""MXFP8 mode timings, one process, interleaved repetitions (results in profiles/mxfp8_timing.txt):

  1. the four block GEMMs (QKV, out-projection, FFN1, FFN2) at 2B B = 1, 2B B = 4 and 5B B = 1: the shipped bf16 GEMM (``orv_gemm_bf16``,
     row-major operands, the library's tile choice) against ``orv_gemm_mxfp8`` on operands quantised beforehand, and the standalone
     ``orv_mxfp8_quantize`` pass of the GEMMs whose A operand is not written by the LayerNorm (out-projection, FFN2);
  2. the 2B B = 4 transformer forward (bench weights / inputs, eager launches) with the MXFP8 mode off and on.

Usage: python tools/mxfp8_time.py [--reps 7] [--iters 20] [--fwd-reps 5] [--out FILE]
       python tools/mxfp8_time.py --profile-forward 3     (only: 3 MXFP8 forwards, for a separate rocprofv3 --kernel-trace --stats run)"""
import argparse
import json
import os
import statistics
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


def gemm_cases():
    # (config, M, D, FF): 2B S = 3226 tokens per clip (the bench clip), 5B S = 1762 (a 256 x 384 DROID clip)
    out = []
    for name, M, D, FF in (("2B B=1", 3226, 1920, 7680), ("2B B=4", 4 * 3226, 1920, 7680), ("5B B=1", 1762, 3072, 12288)):
        for gname, N, K, epi in (("QKV", 3 * D, D, 0), ("out", D, D, 2), ("FFN1", FF, D, 1), ("FFN2", D, FF, 2)):
            out.append((name, gname, M, N, K, epi))
    return out


def time_gemms(reps, iters):
    from orv_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for cfg, gname, M, N, K, epi in gemm_cases():
        A = torch.randn(M, K, device=dev, generator=g).to(BF)
        W = (0.02 * torch.randn(N, K, device=dev, generator=g)).to(BF)
        bias = (0.1 * torch.randn(N, device=dev, generator=g)).to(BF)
        C = torch.empty(M, N, dtype=BF, device=dev)
        R = torch.randn(M, N, device=dev, generator=g).to(BF) if epi == 2 else None
        qa, sa = ops.mxfp8_quantize(A)
        qw, sw = ops.mxfp8_quantize(W)
        kw = dict(R=R, ldr=N) if epi == 2 else {}
        f_bf = lambda: ops.gemm(A, W, bias, C, M, N, K, epilogue=epi, **kw)
        f_mx = lambda: ops.gemm_mxfp8(qa, sa, qw, sw, bias, C, M, N, K, epilogue=epi, **kw)
        f_q = lambda: ops.mxfp8_quantize(A, q=qa, s=sa)
        for f in (f_bf, f_mx, f_q):            # warm-up: code objects, first-touch
            _time(f, 3)
        t = {"bf16": [], "mxfp8": [], "quant": []}
        for _ in range(reps):                  # interleaved: bf16, MXFP8, quantise, bf16, ...
            t["bf16"].append(_time(f_bf, iters))
            t["mxfp8"].append(_time(f_mx, iters))
            t["quant"].append(_time(f_q, iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        flop = 2.0 * M * N * K
        rows.append(dict(config=cfg, gemm=gname, M=M, N=N, K=K, epilogue=epi, bf16_kernel=ops.gemm_kernel_name(M, N, K, epi),
                         bf16_ms=round(med["bf16"], 4), mxfp8_ms=round(med["mxfp8"], 4), quant_ms=round(med["quant"], 4),
                         ratio=round(med["mxfp8"] / med["bf16"], 3), bf16_tflops=round(flop / med["bf16"] / 1e9, 1),
                         mxfp8_tflops=round(flop / med["mxfp8"] / 1e9, 1),
                         spread_bf16=[round(min(t["bf16"]), 4), round(max(t["bf16"]), 4)],
                         spread_mxfp8=[round(min(t["mxfp8"]), 4), round(max(t["mxfp8"]), 4)]))
        print(json.dumps(rows[-1]), flush=True)
        del A, W, C, R, qa, sa, qw, sw
        torch.cuda.empty_cache()
    return rows


def time_forward(reps, iters, B=4):
    import bench
    dev = torch.device("cuda:0")
    model = bench.build_model(dict(bench.CFG_2B), dev)
    lat, img, prompt, actions = bench.synthetic_inputs(B, dev, BF)
    x = torch.cat([lat, img], dim=2)
    ts = torch.full((B,), 500, device=dev)
    model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
    run = lambda: model(x, prompt, {"actions": actions}, ts, return_dict=False)
    res = {"bf16": [], "mxfp8": []}
    with torch.no_grad():
        for mode in ("bf16", "mxfp8"):         # warm-up of both modes (weights quantised once on enable)
            model.enable_mxfp8(mode == "mxfp8")
            _time(run, 2)
        model.enable_mxfp8(True)               # keep the quantised weights: toggle the flag alone from here on
        for _ in range(reps):
            for mode in ("bf16", "mxfp8"):
                model._mxfp8 = mode == "mxfp8"
                res[mode].append(_time(run, iters))
    med = {k: statistics.median(v) for k, v in res.items()}
    row = dict(config=f"2B B={B} forward (eager)", bf16_ms=round(med["bf16"], 2), mxfp8_ms=round(med["mxfp8"], 2),
               ratio=round(med["mxfp8"] / med["bf16"], 3), all_bf16=[round(v, 2) for v in res["bf16"]],
               all_mxfp8=[round(v, 2) for v in res["mxfp8"]])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fwd-reps", type=int, default=5)
    ap.add_argument("--fwd-iters", type=int, default=3)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--profile-forward", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp8_time.py needs the MI355X")
    if a.profile_forward:
        import bench
        dev = torch.device("cuda:0")
        model = bench.build_model(dict(bench.CFG_2B), dev).enable_mxfp8()
        lat, img, prompt, actions = bench.synthetic_inputs(4, dev, BF)
        x = torch.cat([lat, img], dim=2)
        model.action_embed.forced_mask = torch.zeros(4, dtype=torch.bool)
        with torch.no_grad():
            for _ in range(a.profile_forward):
                model(x, prompt, {"actions": actions}, torch.full((4,), 500, device=dev), return_dict=False)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "gemms": time_gemms(a.reps, a.iters)}
    if not a.skip_forward:
        res["forward"] = time_forward(a.fwd_reps, a.fwd_iters)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
