"""Where does the MXFP8 path's distance from the emulated-MXFP8 oracle come from? (profiles/mxfp8_accuracy.txt)

Per depth L (CogVideoX-2B widths, bench weights / inputs, one clip, t = 500), rel-L2 between:
  mx~emu    the HIP MXFP8 path and the oracle with the six block linears on MXFP8 (tests/test_gpu_mxfp8.py's emulation)
  emu~emu'  that emulated oracle and the SAME emulated oracle fed latents perturbed by one bf16 rounding step (x (1 + 2^-9 n), n ~ N(0, 1),
            rounded to bf16): how far two MXFP8 computations land apart when their inputs differ at bf16 resolution only - quantisation-
            boundary flips (an e4m3 step is 1/8 of the value, a bf16 one 1/256) amplified through the blocks
  fp~fp'    the same perturbation through the fp32 oracle (no quantisation): the model's own sensitivity
  bf~fp     the shipped bf16 HIP path and the fp32 oracle
  mx~fp, emu~fp
Usage: python tools/mxfp8_drift.py [--depths 1,6,30]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BF = torch.bfloat16


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="1,6,30")
    a = ap.parse_args()
    import bench
    from oracle import dit
    from test_gpu_mxfp8 import _emulated_lin
    dev = torch.device("cuda:0")
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 2) // 2)))
    lat, img, prompt, actions = bench.synthetic_inputs(1, dev, BF)
    x = torch.cat([lat, img], dim=2)
    ts = torch.tensor([500], device=dev)
    g = torch.Generator().manual_seed(1)
    xp = (x.float().cpu() * (1 + 2.0 ** -9 * torch.randn(x.shape, generator=g))).to(BF).float()
    plain_lin = dit._lin
    print("depth  mx~emu     emu~emu'   fp~fp'     bf~fp      mx~fp      emu~fp", flush=True)
    for L in [int(v) for v in a.depths.split(",")]:
        m = bench.build_model(dict(bench.CFG_2B, num_layers=L), dev)
        m.action_embed.forced_mask = torch.zeros(1, dtype=torch.bool)
        with torch.no_grad():
            bf = m(x, prompt, {"actions": actions}, ts, return_dict=False)[0].cpu()
            mx = m.enable_mxfp8()(x, prompt, {"actions": actions}, ts, return_dict=False)[0].cpu()
        sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
        del m
        torch.cuda.empty_cache()
        kw = dict(actions=actions.float().cpu(), is_mask=torch.zeros(1, dtype=torch.bool))
        args = lambda xx: (sd, dict(bench.CFG_2B, num_layers=L), xx, prompt.float().cpu(), ts.cpu())
        with torch.no_grad():
            dit._lin = plain_lin
            fp, fpp = dit.dit_forward(*args(x.float().cpu()), **kw)[0], dit.dit_forward(*args(xp), **kw)[0]
            dit._lin = _emulated_lin(plain_lin)
            emu, emup = dit.dit_forward(*args(x.float().cpu()), **kw)[0], dit.dit_forward(*args(xp), **kw)[0]
            dit._lin = plain_lin
        print(f"{L:5d}  {rel(mx, emu):.3e}  {rel(emu, emup):.3e}  {rel(fp, fpp):.3e}  {rel(bf, fp):.3e}  {rel(mx, fp):.3e}  {rel(emu, fp):.3e}",
              flush=True)


if __name__ == "__main__":
    main()
