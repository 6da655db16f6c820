"""T5 text-encoder measurements on one MI355X, one process, interleaved repetitions (results in profiles/t5.txt):

  (a) ``orv_t5_attention_fwd`` at (B, S, H) = (2, 226, 64) against ``F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=1.0)``
      on the same operands (the [H, S, S] bias tensor torch needs is built outside the timed window);
  (b) ``orv_amd.t5.T5EncoderModel.forward`` at the CogVideoX shape (d_model 4096, 64 heads, d_ff 10240, 24 layers, random weights, B = 2,
      S = 226) against the plain-torch restatement (tests/t5_ref.py) run with torch's own bf16 ops on the same device and the same weights:
      what attaching a PyTorch T5 gives;
  (c) the whole-encoder accuracies of the GPU tests next to their yardsticks (the restatement in bf16 on the CPU against its fp32 run);
  (d) whether B = 2 equals two B = 1 encodes bit for bit (through the GEMM tile planner; reported, not asserted).

Usage: python tools/t5_time.py [--reps 7] [--iters 20] [--layers 24] [--out profiles/t5.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BF = torch.bfloat16


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _ab(fns, reps, iters):
    """{name: fn} -> {name: (median, min, max) ms}; the candidates alternate inside every repetition."""
    for f in fns.values():
        _time(f, 3)
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(_time(f, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def time_attention(reps, iters, B=2, S=226, H=64):
    from orv_amd import ops
    from orv_amd.t5 import build_bias_rel
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B, S, 3, H, 64, device=dev, generator=g)
    qkv[:, :, 0] *= 0.25
    qkv = qkv.to(BF)
    bias_rel = build_bias_rel(torch.randn(32, H, device=dev, generator=g), S)
    i, j = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    bias = bias_rel[:, j - i + S - 1].to(BF)[None].contiguous()                        # [1, H, S, S]
    q, k, v = (qkv[:, :, n].permute(0, 2, 1, 3).contiguous() for n in range(3))         # [B, H, S, 64], contiguous: torch's best case
    flat, out = qkv.view(B * S, 3 * H * 64), torch.empty(B * S, H * 64, dtype=BF, device=dev)
    res = _ab({"native": lambda: ops.t5_attention_fwd(flat, bias_rel, out, B, S, H),
               "sdpa": lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=1.0)}, reps, iters)
    ref = F.scaled_dot_product_attention(q.float(), k.float(), v.float(), attn_mask=bias.float(), scale=1.0).permute(0, 2, 1, 3).reshape(B * S, -1)
    flops = 4.0 * B * H * S * S * 64
    return dict(B=B, S=S, H=H, native_ms=[round(x, 4) for x in res["native"]], sdpa_ms=[round(x, 4) for x in res["sdpa"]],
                speedup=round(res["sdpa"][0] / res["native"][0], 2), native_tflops=round(flops / res["native"][0] / 1e9, 1),
                max_abs_diff_vs_fp32_sdpa=float((out.float() - ref).abs().max()))


def time_encoder(reps, iters, layers, B=2, S=226):
    import t5_ref
    from orv_amd.t5 import T5EncoderModel
    dev = torch.device("cuda:0")
    cfg = t5_ref.tiny_config(d_model=4096, num_heads=64, d_ff=10240, num_layers=layers, vocab_size=32128)
    with torch.device(dev):
        enc = T5EncoderModel(cfg)
    enc = enc.to(BF)
    g = torch.Generator(device=dev).manual_seed(0)
    D, dk, dff = cfg["d_model"], cfg["d_kv"], cfg["d_ff"]
    for name, p in enc.named_parameters():
        leaf = name.split(".")[-2]
        std = {"q": 2.0 * (D * dk) ** -0.5, "k": D ** -0.5, "v": D ** -0.5, "o": D ** -0.5, "wi_0": D ** -0.5, "wi_1": D ** -0.5,
               "wo": dff ** -0.5}.get(leaf, 1.0)
        t = torch.randn(p.shape, device=dev, generator=g) * std
        p.data.copy_(1.0 + 0.1 * t if "layer_norm" in leaf else t)
    ids = torch.randint(0, cfg["vocab_size"], (B, S), device=dev, generator=g)
    enc(ids)                                                   # stacks q | k | v and wi_0 | wi_1; the parameters now view the stacks
    state = dict(enc.state_dict())                             # the same tensors: both sides read one copy of the weights
    with torch.no_grad():
        res = _ab({"native": lambda: enc(ids), "torch_bf16": lambda: t5_ref.encode(state, cfg, ids, dtype=BF)}, reps, iters)
        a, b = enc(ids)[0].float(), t5_ref.encode(state, cfg, ids, dtype=BF).float()
        singles = torch.cat([enc(ids[n:n + 1])[0] for n in range(B)])
        both = enc(ids)[0]
    nbytes = sum(p.numel() for n, p in enc.named_parameters() if "shared" not in n and "embed" not in n) * 2.0
    gemm_flops = 2.0 * B * S * layers * (4 * D * D + 3 * D * dff)
    return dict(B=B, S=S, layers=layers, native_ms=[round(x, 3) for x in res["native"]], torch_bf16_ms=[round(x, 3) for x in res["torch_bf16"]],
                speedup=round(res["torch_bf16"][0] / res["native"][0], 2), weight_gb=round(nbytes / 1e9, 2),
                native_weight_tb_per_s=round(nbytes / res["native"][0] / 1e9, 2), native_gemm_tflops=round(gemm_flops / res["native"][0] / 1e9, 1),
                rel_l2_native_vs_torch_bf16=float((a - b).norm() / b.norm()),
                b2_equals_two_b1=bool(torch.equal(both, singles)), b2_vs_b1_max_abs_diff=float((both.float() - singles.float()).abs().max()))


def accuracy():
    import t5_ref
    from orv_amd.t5 import T5EncoderModel
    dev = torch.device("cuda:0")
    cases = {"small": (128, 2, 256, 2, 226, 2, 64), "inner_ne_d": (128, 3, 320, 4, 300, 1, 64), "deep": (256, 4, 640, 6, 226, 2, 64),
             "full_width": (4096, 64, 10240, 1, 226, 2, 512)}
    rows = []
    for name, (D, H, Fd, L, S, B, V) in cases.items():
        cfg = t5_ref.tiny_config(d_model=D, num_heads=H, d_ff=Fd, num_layers=L, vocab_size=V)
        state, ids = t5_ref.make_state(cfg, seed=3), t5_ref.make_ids(cfg, B, S, seed=4)
        with torch.no_grad():
            ref = t5_ref.encode(state, cfg, ids)
            yard = t5_ref.rel_l2(t5_ref.encode(state, cfg, ids, dtype=BF).float(), ref)
        enc = T5EncoderModel(cfg)
        enc.load_state_dict(state)
        err = t5_ref.rel_l2(enc.to(dev, BF)(ids.to(dev))[0].float().cpu(), ref)
        rows.append(dict(case=name, shape=[D, H, Fd, L, S, B], rel_l2_native=round(err, 6), rel_l2_bf16_restatement=round(yard, 6),
                         ratio=round(err / yard, 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/t5_time.py measures on the MI355X; there is no CPU path"
    lines = [f"# tools/t5_time.py --reps {a.reps} --iters {a.iters} --layers {a.layers}: one process, candidates alternate inside every repetition;",
             "# times are [median, min, max] ms over the repetitions, each repetition the mean of `iters` back-to-back calls (device events)",
             f"# device: {torch.cuda.get_device_name(0)}", "", "## (a) attention kernel vs F.scaled_dot_product_attention(attn_mask=bias, scale=1.0)"]
    lines.append(json.dumps(time_attention(a.reps, a.iters * 10)))
    lines += ["", "## (b) whole encoder vs the plain-torch restatement in bf16 on the same device (same weights)"]
    lines.append(json.dumps(time_encoder(a.reps, a.iters, a.layers)))
    lines += ["", "## (c) whole-encoder accuracy vs the fp32 restatement, next to the bf16 restatement's own (tests/test_gpu_t5.py bar: ratio <= 1.25)"]
    lines += [json.dumps(r) for r in accuracy()]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
