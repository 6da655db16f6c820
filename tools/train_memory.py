"""Peak device memory of two training steps of the 2B model:  python tools/train_memory.py [BATCH] [--param-precision bf16|split_fp32|stochastic] [--state-precision fp32|fp8] [--lora-rank R]
(--lora-rank R: a rank-R LoRA adapter on the attention projections is the only trainable state, orv_amd/lora.py; "split_fp32" keeps 2 more bytes per parameter: the int16 low halves of the fp32 masters, 3.4 GB at 1.69 B parameters; "fp8" keeps the two
moments in 2 + 2/256 instead of 8 bytes per parameter)."""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from orv_amd import sft, schedulers
from orv_amd.optim import FusedAdamW
ap = argparse.ArgumentParser()
ap.add_argument("batch", nargs="?", type=int, default=4)
ap.add_argument("--param-precision", default="bf16", choices=["bf16", "split_fp32", "stochastic"])
ap.add_argument("--state-precision", default="fp32", choices=["fp32", "fp8"])
ap.add_argument("--lora-rank", type=int, default=0)
args = ap.parse_args()
B = args.batch
dev = torch.device("cuda:0")
model = bench.build_model(bench.CFG_2B, dev).train()
model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
if args.lora_rank:
    model.add_adapter(r=args.lora_rank, lora_alpha=args.lora_rank)
lat, img, prompt, actions = bench.synthetic_inputs(B, dev, torch.bfloat16)
sched = schedulers.CogVideoXDDIMScheduler(**bench.SCHED)
params = [p for p in model.parameters() if p.requires_grad] if args.lora_rank else model.parameters()
opt = FusedAdamW(params, lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0,
                 param_precision=args.param_precision, state_precision=args.state_precision)
b = sft.Batch(lat, img, prompt, actions, None, None, torch.ones(lat.shape[1], dtype=torch.bool, device=dev), 1)
for _ in range(2):
    sft.sft_step(model, sched, opt, b)
torch.cuda.synchronize()
lo = opt._flat.get("lo")
moments = sum(opt._flat[k].numel() * opt._flat[k].element_size() for k in ("m", "v", "m8", "v8", "m_exp", "v_exp") if k in opt._flat)
if args.lora_rank:
    print("lora_rank=%d trainable parameters %d" % (args.lora_rank, sum(p.numel() for p in opt.params)))
print("B=%d param_precision=%s state_precision=%s peak allocated %.1f GB, reserved %.1f GB, optimizer low halves %.2f GB, moments %.2f GB" % (
      B, args.param_precision, args.state_precision, torch.cuda.max_memory_allocated() / 2**30, torch.cuda.max_memory_reserved() / 2**30,
      0.0 if lo is None else lo.numel() * 2 / 2**30, moments / 2**30))
