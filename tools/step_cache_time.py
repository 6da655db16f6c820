"""Developer measurement (not part of any test) of the first-block step cache on one MI355X, one process, candidates interleaved, medians
with spread (results in profiles/step_cache.txt).  Shape: the bench shape, 2B, 320 x 480 x 17 frames, B = 4 and B = 1.

  (a) the three kernels (probe with its finishing launch, store, apply) standalone, device events around every launch, on buffer sets
      rotated so that the footprint exceeds the 256 MiB last-level cache; bytes per second on their compulsory traffic (probe 5, store 5,
      apply 3 times B Nv D 2 bytes; the snapshot of E, a strided copy, is timed beside them: 2 times);
      and the step: uncached, cached and computed (``force_compute`` ahead of every call), cached and skipped (threshold inf), all three
      replayed from HIP graphs, one host synchronisation around every step for all three alike;
  (b) is the skipped step of (a);
  (c) 50-step DDIM and DPM loops (``pipe(...)``, guidance 1, output_type latent) at a few thresholds on the random-init weights of
      ``bench.build_model`` and on the same weights with trained-LIKE qk-LayerNorm gains (the recipe of bench.py's ``attn_mixed`` leg): skipped
      steps, loop time against the uncached loop, rel-L2 of the final latents against the uncached run.  These are deviations on UNTRAINED
      weights; they say nothing about a trained ORV checkpoint.

Usage: python tools/step_cache_time.py [--batches 4,1] [--rounds 7] [--thresholds 0.1,0.15,0.2,0.3] [--skip-loops] [--out profiles/step_cache.txt]"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16
DEV = torch.device("cuda:0")
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def stats(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, max(0, int(round(f * (len(v) - 1)))))]
    return f"median {statistics.median(v):8.4f} ms  (p10 {q(0.1):.4f}, p90 {q(0.9):.4f}, n = {len(v)})"


def time_kernels(B, Nt, Nv, D, rounds):
    from orv_amd import ops
    elems = B * Nv * D
    nsets = max(2, math.ceil(600e6 / (5 * elems * 2)))
    sets = []
    for k in range(nsets):
        g = torch.Generator(device=DEV).manual_seed(k)
        r = lambda *s: torch.randn(*s, generator=g, device=DEV).to(BF)
        sets.append(dict(x=r(B, Nt + Nv, D), e=r(B, Nv, D), p=r(B, Nv, D), f=r(B, Nv, D), c=r(B, Nv, D), t=r(B, Nv, D),
                         sums=torch.zeros(B, 2, dtype=torch.float64, device=DEV),
                         scratch=torch.zeros(ops.step_cache_scratch(B, Nv, D), dtype=torch.float64, device=DEV)))
    cands = {
        "probe (+ finish)": (5, lambda s: ops.step_cache_probe(s["x"], s["e"], s["p"], s["f"], s["c"], s["sums"], B, Nt, Nv, D, scratch=s["scratch"])),
        "store": (5, lambda s: ops.step_cache_store(s["x"], s["f"], s["c"], s["t"], s["p"], B, Nt, Nv, D)),
        "apply": (3, lambda s: ops.step_cache_apply(s["x"], s["t"], B, Nt, Nv, D)),
        "snapshot of E (copy_)": (2, lambda s: s["e"].copy_(s["x"].view(B, Nt + Nv, D)[:, Nt:])),
    }
    times = {k: [] for k in cands}
    for rd in range(rounds + 2):
        for name, (_, fn) in cands.items():
            s = sets[rd % nsets]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(s)
            b.record()
            torch.cuda.synchronize()
            if rd >= 2:
                times[name].append(a.elapsed_time(b))
    say(f"  kernels standalone, B = {B}, Nt = {Nt}, Nv = {Nv}, D = {D} ({nsets} rotating buffer sets, {5 * elems * 2 * nsets / 2 ** 20:.0f} MiB)")
    total = 0.0
    for name, (mult, _) in cands.items():
        med = statistics.median(times[name])
        total += med
        say(f"    {name:24s} {stats(times[name])}  {mult} x B Nv D 2 = {mult * elems * 2 / 1e6:7.1f} MB  -> {mult * elems * 2 / med / 1e9:6.2f} TB/s")
    floor_bytes = 12 * elems * 2
    say(f"    sum of medians (probe + store + snapshot: what a computed step adds) "
        f"{statistics.median(times['probe (+ finish)']) + statistics.median(times['store']) + statistics.median(times['snapshot of E (copy_)']):.4f} ms; "
        f"derived floor 12 B Nv D 2 = {floor_bytes / 1e9:.3f} GB = {floor_bytes / 4.9e12 * 1e3:.4f} ms at 4.9 TB/s")


def build(B):
    import bench
    from orv_amd import schedulers
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj
    model = bench.build_model(dict(bench.CFG_2B), DEV)
    model.action_embed.forced_mask = torch.zeros(B, dtype=torch.bool)
    lat, img, prompt, actions = bench.synthetic_inputs(B, DEV, BF)
    mk = lambda cls: CogVideoXImageToVideoPipelineTraj(transformer=model, scheduler=getattr(schedulers, cls)(**bench.SCHED))
    return model, lat, img, prompt, actions, mk


def time_steps(B, rounds):
    """(a) / (b): one transformer forward of the loop, three candidates, interleaved."""
    import bench
    model, lat, img, prompt, actions, mk = build(B)
    pipe = mk("CogVideoXDDIMScheduler")
    model_in = torch.cat([lat, img], dim=2)
    kw = dict(hidden_states=model_in, encoder_hidden_states=prompt, controls_or_guidances={"actions": actions}, return_dict=False)
    tv = lambda t: torch.full((B,), t, device=DEV, dtype=torch.int64)

    @torch.no_grad()
    def fwd(t):
        return pipe.transformer_forward(timestep=tv(t), **kw)[0]

    def timed(t):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fwd(t)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    res = {"uncached": [], "cached, computed": [], "cached, skipped": []}
    # warm every graph first: uncached (3 calls), then the cache's front / tail / skip entries (3 calls each)
    for i in range(3):
        fwd(900 - i)
    cache = model.enable_step_cache(float("inf"))
    for i in range(4):
        cache.force_compute()
        fwd(900 - i)
    for i in range(4):
        fwd(900 - i)
    assert [h.skipped for h in cache.history[-4:]] == [True] * 4
    model.disable_step_cache()
    for rd in range(rounds):
        t = 800 - 10 * rd
        model._step_cache = None
        res["uncached"].append(timed(t))
        model._step_cache = cache
        cache.force_compute()
        res["cached, computed"].append(timed(t))
        res["cached, skipped"].append(timed(t - 5))
        assert cache.history[-1].skipped and not cache.history[-2].skipped
    model._step_cache = None
    say(f"  one transformer forward of the loop, B = {B}, HIP-graph replay, host synchronisation around every forward")
    for k, v in res.items():
        say(f"    {k:18s} {stats(v)}")
    mu, mc, ms = (statistics.median(res[k]) for k in res)
    say(f"    computed - uncached = {mc - mu:+.4f} ms ({100 * (mc - mu) / mu:+.2f} %); skipped / uncached = {ms / mu:.4f} (1 / {mu / ms:.1f})")
    del pipe, model
    torch.cuda.empty_cache()


def trained_like(model):
    """bench.py's ``attn_mixed`` recipe: per layer max|gamma_q gamma_k| log-uniform in [1, 16]."""
    g = torch.Generator().manual_seed(46)
    with torch.no_grad():
        for blk in model.transformer_blocks:
            at = blk.attn1
            tgt = float(torch.exp(torch.rand(1, generator=g) * math.log(16.0)))
            pert = 1.0 + 0.15 * torch.randn(2, 64, generator=g)
            at.norm_q.weight.copy_((pert[0].abs() * math.sqrt(tgt)).to(DEV, BF))
            at.norm_k.weight.copy_((pert[1].abs() * math.sqrt(tgt)).to(DEV, BF))


def time_loops(B, thresholds, steps=50):
    model, lat, img, prompt, actions, mk = build(B)
    image = (img[:, :1] / 1.15258426).permute(0, 2, 1, 3, 4).contiguous()             # [B, 16, 1, h, w] latents of the reference frame
    for weights in ("random-init", "trained-like qk-LayerNorm gains"):
        if weights != "random-init":
            trained_like(model)
        for cls in ("CogVideoXDDIMScheduler", "CogVideoXDPMScheduler"):
            pipe = mk(cls)

            def loop():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(image=image, height=320, width=480, num_frames=17, num_inference_steps=steps, guidance_scale=1.0,
                           generator=torch.Generator(device=DEV).manual_seed(3), latents=lat.clone(), prompt_embeds=prompt, output_type="latent",
                           controls_or_guidances={"actions": actions}).frames
                torch.cuda.synchronize()
                return out.float(), time.perf_counter() - t0
            pipe.disable_step_cache()
            loop()                                                                     # warm-up: graphs, tables
            base, t_base = loop()
            say(f"  {steps}-step {cls[9:-9]} loop, B = {B}, {weights}: uncached {t_base:.3f} s")
            for th in thresholds:
                pipe.enable_step_cache(th)
                loop()                                                                 # warm-up of the three segments' graphs
                out, t_c = loop()
                rep = pipe.step_cache_report
                skipped = sum(1 for r in rep if r[2])
                ds = [r[1] for r in rep if r[1] is not None]
                rel = ((out - base).norm() / base.norm()).item()
                say(f"    threshold {th:<6g} skipped {skipped:2d} / {steps}  loop {t_c:.3f} s = {t_c / t_base:.3f} x uncached  rel-L2 of the final latents "
                    f"{rel:.3e}  distances min {min(ds):.3e} median {statistics.median(ds):.3e} max {max(ds):.3e}")
            pipe.disable_step_cache()
    del model
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,1")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--thresholds", default="0.1,0.15,0.2,0.3")
    ap.add_argument("--skip-loops", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_cache.txt"))
    args = ap.parse_args()
    from orv_amd._lib import check, lib
    check(lib().orv_device_check(0), "orv_device_check")
    say("First-block step cache: tools/step_cache_time.py on one MI355X, one process, candidates interleaved.")
    say("Untrained weights throughout: the deviations below say nothing about a trained ORV checkpoint, and no threshold is recommended from them.")
    for B in [int(b) for b in args.batches.split(",")]:
        say()
        say(f"== B = {B} ==")
        say("(a) overhead of a computed step, (b) cost of a skipped step")
        time_kernels(B, 226, 3000, 1920, max(args.rounds, 15))
        time_steps(B, args.rounds)
        if not args.skip_loops:
            say("(c) 50-step loops")
            time_loops(B, [float(t) for t in args.thresholds.split(",")])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
