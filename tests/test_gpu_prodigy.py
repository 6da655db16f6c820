"""GPU: the fused Prodigy optimizer (``orv_prodigy_moments`` / ``orv_prodigy_recurrence`` / ``orv_prodigy_update``, ``FusedProdigy``,
``get_optimizer``) against its CPU restatement (tests/prodigy_ref.py).  The storage of the master (split / rebuild) is held bit for bit; the
fp32 arithmetic is held to a float64 evaluation of the rule with the error of a CPU fp32 evaluation as the yardstick - the convention of
test_gpu_adamw_precision.py, for the same reasons (FMA contraction and a one-step difference of a library function between the two
machines are allowed, so bit-equality of the arithmetic is not demanded).  Measured figures are printed before they are asserted.

Layout of the kernel tests: segments of 4101 elements (three chunks, the last mostly padding), 1 element, 4096 elements and one INACTIVE
segment of 2048 - seven chunks of 2048."""
import itertools

import pytest
import torch

import adamw_ref
import prodigy_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEG = 2048
SIZES = [4101, 1, 4096, 2048]
STARTS = [0, 6144, 8192, 12288, 14336]
N = STARTS[-1]
HYPER = dict(lr=1.0, betas=(0.9, 0.95), beta3=None, eps=1e-8, d0=1e-6, d_coef=1.0, growth_rate=float("inf"))
SCALARS = dict(d=3e-4, d_max=5e-4, d_numerator=2e-3, d_denom=0.0, d_hat=0.0, k=7, dlr=0.0, skip=0)
CLIP = 0.37


def _dev():
    return torch.device("cuda:0")


def _real_mask():
    real = torch.zeros(N, dtype=torch.bool)
    for a, n in zip(STARTS, SIZES):
        real[a:a + n] = True
    return real


def _inputs(seed=0):
    """A non-trivial state: random m, v >= 0, s, p0 != w, random low halves; padding all zero; the inactive segment as random as the rest."""
    g = torch.Generator().manual_seed(seed)
    real = _real_mask()
    z = lambda x: torch.where(real, x, torch.zeros_like(x))
    d = SCALARS["d"]
    p = z((torch.randn(N, generator=g) * 0.02).to(BF))
    lo = z(torch.randint(-32768, 32768, (N,), generator=g, dtype=torch.int64).to(torch.int16))
    grad = z((torch.randn(N, generator=g) * 0.05).to(BF))
    m = z(torch.randn(N, generator=g) * 0.03 * d)
    v = z((torch.randn(N, generator=g) * 0.05 * d) ** 2)
    s = z(torch.randn(N, generator=g) * 1e-3)
    p0 = z((p.float() + torch.randn(N, generator=g) * 0.01).to(BF))
    return dict(p=p, lo=lo, g=grad, m=m, v=v, s=s, p0=p0, seg_start=torch.tensor(STARTS, dtype=torch.int64),
                active=torch.tensor([1, 1, 1, 0], dtype=torch.uint8), seg_step=torch.tensor([5, 3, 9, 2], dtype=torch.int32))


def _active_mask(inp):
    act = torch.zeros(N, dtype=torch.bool)
    for i, a in enumerate(inp["active"].tolist()):
        act[STARTS[i]:STARTS[i + 1]] = bool(a)
    return act


def _launch(inp, sc, clip=CLIP, **flags):
    """The three launches on the GPU -> CPU copies of every buffer, the partials and the state."""
    from orv_amd import ops
    dev = _dev()
    h = dict(R.DEFAULTS, **HYPER, **flags)
    b3 = h["betas"][1] ** 0.5 if h["beta3"] is None else h["beta3"]
    t = {k: inp[k].to(dev).clone() for k in ("p", "lo", "g", "p0", "m", "v", "s", "seg_start", "active", "seg_step")}
    state = R.state_tensor(sc).to(dev)
    partials = torch.full((2 * (N // SEG),), 7.0, dtype=torch.float64, device=dev)        # every pair must be written, zeros included
    cl = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=dev)
    ops.prodigy_moments(t["p"], t["lo"], t["g"], t["p0"], t["m"], t["v"], t["s"], t["seg_start"], t["active"], t["seg_step"], state, partials,
                        h["lr"], h["betas"][0], h["betas"][1], b3, h["weight_decay"], h["decouple"], h["safeguard_warmup"],
                        h["use_bias_correction"], h["d0"], cl)
    ops.prodigy_recurrence(state, partials, h["lr"], h["betas"][0], h["betas"][1], b3, h["use_bias_correction"], h["d0"], h["d_coef"],
                           h["growth_rate"])
    ops.prodigy_update(t["p"], t["lo"], t["m"], t["v"], t["seg_start"], t["active"], state, h["eps"], h["weight_decay"], h["decouple"])
    torch.cuda.synchronize()
    out = {k: x.cpu() for k, x in t.items()}
    out.update(partials=partials.cpu(), state=state.cpu())
    return out


def _reference(inp, sc, dtype, clip=CLIP, **flags):
    sc = dict(sc)
    w_old = adamw_ref.rebuild(inp["p"], inp["lo"])
    w, p0, m, v, s, num, den = R.flat_step(w_old, inp["g"], inp["p0"], inp["m"], inp["v"], inp["s"], inp["seg_start"], inp["active"],
                                           inp["seg_step"], sc, dtype, clip=clip, **dict(HYPER, **flags))
    return dict(w=w, p0=p0, m=m, v=v, s=s, num=num, den=den, sc=sc)


_ref_cache = {}


def _references(key, inp, sc, **flags):
    if key not in _ref_cache:
        _ref_cache[key] = (_reference(inp, sc, torch.float64, **flags), _reference(inp, sc, torch.float32, **flags))
    return _ref_cache[key]


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("decouple,safeguard,bias", list(itertools.product([True, False], repeat=3)))
def test_one_step_from_a_non_trivial_state_against_float64(decouple, safeguard, bias, wd):
    """d = 3e-4, d_max = 5e-4, d_numerator = 2e-3, k = 7, clip coefficient 0.37.  Weights: error against float64 in units of the fp32 step
    of max(|w_old|, |w_new|, |w_new - w_old|), at most twice the worst error of the CPU fp32 evaluation.  m, v, s: 1e-6 of the scale of
    their two terms.  The two sums: 1e-6 of sum |c g (p0 - w)| and of sum |s|.  d, d_max, d_numerator, k follow from the GPU's own sums by
    the recurrence, in fp64."""
    flags = dict(decouple=decouple, safeguard_warmup=safeguard, use_bias_correction=bias, weight_decay=wd)
    inp = _inputs()
    got = _launch(inp, SCALARS, **flags)
    r64, r32 = _references((decouple, safeguard, bias, wd), inp, SCALARS, **flags)
    act = _active_mask(inp)
    w_old = adamw_ref.rebuild(inp["p"], inp["lo"]).double()
    w_gpu = adamw_ref.rebuild(got["p"], got["lo"]).double()
    unit = adamw_ref.fp32_ulp(torch.maximum(torch.maximum(w_old.abs(), r64["w"].abs()), (r64["w"] - w_old).abs()))
    yard = float(((r32["w"].double() - r64["w"]).abs() / unit)[act].max())
    err = float(((w_gpu - r64["w"]).abs() / unit)[act].max())
    print(f"\nprodigy one step {flags}: weights vs float64 in fp32 steps - CPU fp32 (yardstick) {yard:.3f}, GPU {err:.3f} (bound {2 * yard:.3f})")
    # the scales of the moments' two terms, from the rule
    b1, b2 = R.f32(0.9), R.f32(0.95)
    b3 = R.f32(0.95 ** 0.5)
    d = SCALARS["d"]
    dlr = R.step_dlr(SCALARS, 1.0, b1, b2, bias)
    gr = inp["g"].double() * R.f32(CLIP)
    if wd and not decouple:
        gr = gr + R.f32(wd) * w_old
    ratio = d / HYPER["d0"]
    scales = dict(m=(b1 * inp["m"].double()).abs() + (d * (1 - b1) * gr).abs(), v=b2 * inp["v"].double() + d * d * (1 - b2) * gr * gr,
                  s=(b3 * inp["s"].double()).abs() + (ratio * (d if safeguard else dlr) * gr).abs())
    real = act & _real_mask()
    errs = {k: float(((got[k].double() - r64[k]).abs() / scales[k])[real].max()) for k in "mvs"}
    num_gpu, den_gpu = float(got["partials"][0::2].sum()), float(got["partials"][1::2].sum())
    num_scale = float((ratio * dlr * gr * (inp["p0"].double() - w_old)).abs()[act].sum())
    num_err, den_err = abs(num_gpu - r64["num"]) / num_scale, abs(den_gpu - r64["den"]) / r64["den"]
    print(f"prodigy one step: m {errs['m']:.3e}, v {errs['v']:.3e}, s {errs['s']:.3e}, num {num_err:.3e}, den {den_err:.3e} (bound 1e-6 each); "
          f"CPU fp32: num {abs(r32['num'] - r64['num']) / num_scale:.3e}, den {abs(r32['den'] - r64['den']) / r64['den']:.3e}")
    assert err <= 2 * yard, (err, yard)
    assert all(e <= 1e-6 for e in errs.values()), errs
    assert num_err <= 1e-6 and den_err <= 1e-6, (num_err, den_err)
    # the recurrence, from the GPU's own sums
    sc = dict(SCALARS)
    R.recurrence_(sc, num_gpu, den_gpu, dlr, b3, HYPER["d0"], HYPER["d_coef"], HYPER["growth_rate"])
    st = R.scalars_of(got["state"])
    assert st["k"] == 8 == sc["k"] and st["skip"] == 0
    for key in ("d", "d_max", "d_numerator", "d_denom", "d_hat", "dlr"):
        assert abs(st[key] - sc[key]) <= 1e-13 * abs(sc[key]), (key, st[key], sc[key])
    assert st["d"] == min(st["d_max"], st["d"]) and st["d_max"] >= SCALARS["d_max"]
    # the pairs of the inactive segment's chunk are zeros, p0 is not rewritten (no segment is at its first update)
    assert got["partials"][12:].tolist() == [0.0, 0.0] and torch.equal(got["p0"].view(torch.int16), inp["p0"].view(torch.int16))


@pytest.mark.parametrize("nchunks", [1, 511, 513, 4095, 4096, 4097, 3 * 4096 + 512 + 3])
def test_recurrence_alone_at_chunk_counts_that_reach_every_loop(nchunks):
    """orv_prodigy_recurrence on random fp64 pairs.  Its 512 lanes take eight pairs per lane and trip while at least 4096 chunks remain,
    then one pair per lane, so 513 reaches the strided tail, 4095 / 4096 / 4097 sit around the first unrolled trip and 12803 = 3 x 4096 + 512 + 3
    takes three trips, a full tail round and a partial one (an r = 64 adapter has 14404 chunks, the 2B model 825195).  A dropped or doubled
    chunk would move both sums by about 1 / nchunks; they are held to 1e-13 of an fp64 torch sum, and d, d_max, d_numerator, d_hat, k to
    the recurrence on those sums."""
    from orv_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(nchunks)
    partials = torch.empty(2 * nchunks, dtype=torch.float64)
    partials[0::2] = (torch.randn(nchunks, generator=g, dtype=torch.float64) * 0.1 + 1.0) * 3e-9      # numerator terms, mostly one sign
    partials[1::2] = torch.rand(nchunks, generator=g, dtype=torch.float64) * 2e-6 + 1e-8             # sums of |s|
    sc = dict(SCALARS)
    state = R.state_tensor(sc).to(dev)
    b1, b2, b3 = R.f32(0.9), R.f32(0.95), R.f32(0.98)
    ops.prodigy_recurrence(state, partials.to(dev), 0.5, 0.9, 0.95, 0.98, True, 1e-6, 2.0, float("inf"))
    torch.cuda.synchronize()
    got = R.scalars_of(state.cpu())
    num_sum, den = float(partials[0::2].sum()), float(partials[1::2].sum())
    R.recurrence_(sc, num_sum, den, R.step_dlr(SCALARS, 0.5, b1, b2, True), b3, 1e-6, 2.0, float("inf"))
    print(f"\nprodigy recurrence, {nchunks} chunks: d_denom {got['d_denom']:.15e} (torch {den:.15e}), d_numerator {got['d_numerator']:.15e} "
          f"(torch {sc['d_numerator']:.15e}), d {got['d']:.6e}")
    assert got["k"] == 8 == sc["k"] and got["skip"] == 0
    for key in ("d_denom", "d_numerator", "d_hat", "d", "d_max", "dlr"):
        assert abs(got[key] - sc[key]) <= 1e-13 * abs(sc[key]), (key, got[key], sc[key])
    assert got["d"] == got["d_max"] == got["d_hat"] > SCALARS["d_max"]             # d itself depends on both sums here


def test_inactive_segment_and_padding_keep_every_byte():
    inp = _inputs(1)
    inp["seg_step"] = torch.tensor([1, 1, 4, 1], dtype=torch.int32)        # first update of two active segments; the inactive one is NOT captured
    got = _launch(inp, SCALARS, weight_decay=1e-2, decouple=False)
    a, b = STARTS[3], STARTS[4]
    for k in ("p", "lo", "p0"):
        assert torch.equal(got[k][a:b].view(torch.int16), inp[k][a:b].view(torch.int16)), k
    for k in ("m", "v", "s"):
        assert torch.equal(got[k][a:b].view(torch.int32), inp[k][a:b].view(torch.int32)), k
    pad = ~_real_mask()
    for k in ("p", "lo", "m", "v", "s", "p0"):
        assert not bool(got[k][pad].view(torch.int16 if got[k].element_size() == 2 else torch.int32).any()), k
    # captured where seg_step == 1: the bf16 part of the master (the low halves here are random, so p0 != master), else kept
    assert torch.equal(got["p0"][:STARTS[2]].view(torch.int16), inp["p"][:STARTS[2]].view(torch.int16))
    assert torch.equal(got["p0"][STARTS[2]:].view(torch.int16), inp["p0"][STARTS[2]:].view(torch.int16))
    act = _active_mask(inp) & _real_mask()
    assert float((adamw_ref.rebuild(got["p"], got["lo"]) != adamw_ref.rebuild(inp["p"], inp["lo"]))[act].float().mean()) > 0.99


def _sizes_params(dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=g) * 0.02).to(BF).to(dev)) for n in SIZES]


def _feed(params, t, dev, scale=0.05):
    for i, p in enumerate(params):
        g = torch.Generator().manual_seed(1000 * t + i)
        p.grad = None if i == 3 else (torch.randn(p.shape, generator=g) * scale).to(BF).to(dev)


_FLAT = ("p", "lo", "m", "v", "s", "p0", "pstate", "seg_step", "partials")


def _snapshot(opt):
    torch.cuda.synchronize()
    return {k: opt._flat[k].cpu().clone() for k in _FLAT}


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int16) if a[k].dtype == BF else a[k], b[k].view(torch.int16) if b[k].dtype == BF else b[k]) for k in _FLAT)


def _run(steps, dev, save_at=None, **kw):
    from orv_amd.optim import FusedProdigy
    kw = dict(dict(lr=1.0, betas=(0.9, 0.95), weight_decay=1e-2, max_grad_norm=0.0, use_bias_correction=True), **kw)
    params = _sizes_params(dev)
    opt = FusedProdigy(params, **kw)
    for t in range(steps):
        if t == save_at:
            sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
            weights = [p.detach().clone() for p in params]
            params = _sizes_params(dev, seed=6)
            with torch.no_grad():
                for p, w in zip(params, weights):
                    p.copy_(w)
            opt = FusedProdigy(params, **kw)
            opt.load_state_dict(sd)
        _feed(params, t, dev)
        opt.step()
        opt.zero_grad()
    return opt


def test_two_runs_give_identical_bytes():
    """max_grad_norm = 0: the clip coefficient does not come from orv_sumsq's atomics, and nothing else depends on arrival order."""
    dev = _dev()
    a, b = _snapshot(_run(4, dev)), _snapshot(_run(4, dev))
    assert _same(a, b)
    assert float(a["pstate"][5]) == 4 and bool(a["lo"].any())


def test_state_dict_resume_is_bit_identical():
    dev = _dev()
    a, b = _snapshot(_run(15, dev)), _snapshot(_run(15, dev, save_at=10))
    assert _same(a, b)
    assert float(a["pstate"][5]) == 15


def test_first_step_captures_p0_and_moves_the_weights_at_d0():
    from orv_amd.optim import FusedProdigy
    dev = _dev()
    params = _sizes_params(dev)
    init = [p.detach().cpu().clone() for p in params]
    opt = FusedProdigy(params, lr=1.0, betas=(0.9, 0.95), max_grad_norm=1.0)
    _feed(params, 0, dev)
    assert opt.step() > 0
    s, p0 = opt.prodigy_state()
    masters = [x.cpu() for x in opt.master_params()]
    for i in range(3):
        assert torch.equal(p0[i].cpu().view(torch.int16), init[i].view(torch.int16))
        assert bool((masters[i] != init[i].float()).float().mean() > 0.99) and bool(s[i].any())
        assert float((masters[i] - init[i].float()).abs().max()) <= 1.001e-6           # |dlr m / (sqrt(v) + d eps)| <= d0 at the first step
    assert torch.equal(masters[3], init[3].float()) and not bool(p0[3].any()) and not bool(s[3].any())
    assert opt._scalar("d_numerator") == 0.0 and opt.d == 1e-6 and opt.d_max == 1e-6 and opt.k == 1 and opt.dlr == 1e-6
    assert opt._scalar("d_denom") > 0


def test_all_zero_gradients_on_a_fresh_optimizer_change_nothing():
    from orv_amd.optim import FusedProdigy
    dev = _dev()
    params = _sizes_params(dev)
    init = [p.detach().cpu().clone() for p in params]
    opt = FusedProdigy(params, lr=1.0, weight_decay=1e-2, max_grad_norm=1.0)
    for p in params:
        p.grad = torch.zeros_like(p)
    assert opt.step() == 0.0
    torch.cuda.synchronize()
    for p, x in zip(params, init):
        assert torch.equal(p.detach().cpu().view(torch.int16), x.view(torch.int16))
    assert not bool(opt._flat["lo"].any()) and opt.k == 0 and opt.d == 1e-6 and opt._scalar("skip") == 1.0


def test_sixty_steps_on_the_quadratic_follow_the_float64_reference():
    """The run of DESIGN.md 4.3.3 (n = 4096, bf16 start, gradient w - target rounded to bf16, lr 1, betas 0.9 / 0.95) on the GPU: d after
    every step against the float64 reference.  Allowed relative error: four times the worst relative error of the CPU fp32 restatement over
    the run (fp32 in-chunk sums in another association, FMA contraction), floor 1e-6.  The mean squared distance ends below 1e-5."""
    from orv_amd.optim import FusedProdigy
    dev = _dev()
    h64, _ = R.quadratic_run(torch.float64)
    h32, _ = R.quadratic_run(torch.float32)
    yard = max(abs(a - b) / b for a, b in zip(h32, h64))
    p0, target = R.quadratic_problem()
    p = torch.nn.Parameter(p0.to(dev))
    tgt = target.to(dev)
    opt = FusedProdigy([p], lr=1.0, betas=(0.9, 0.95), weight_decay=0.0, max_grad_norm=0.0)
    hist = []
    for _ in range(60):
        p.grad = (opt.master_params()[0] - tgt).to(BF)
        opt.step()
        hist.append(opt.d)
    loss = float(((opt.master_params()[0].double() - tgt.double()) ** 2).mean())
    worst = max(abs(a - b) / b for a, b in zip(hist, h64))
    bound = max(4 * yard, 1e-6)
    print(f"\nprodigy 60 steps: worst relative error of d vs float64 - CPU fp32 (yardstick) {yard:.3e}, GPU {worst:.3e} (bound {bound:.3e}); "
          f"d at 60 = {hist[-1]:.6e} (float64 {h64[-1]:.6e}), loss {loss:.3e}")
    assert worst <= bound, (worst, bound)
    assert loss < 1e-5 and hist[0] == 1e-6 and hist[-1] > 1e-2


def test_in_the_model_three_sft_steps_on_a_fresh_adapter():
    """The tiny fwd_actions configuration with add_adapter(r=16), get_optimizer(..., "prodigy", learning_rate=1.0), three sft_steps.  After
    each step every adapter master is compared with the reference fed the state the step started from and the gradients the GPU produced
    (yardstick bound of the one-step test); base weights never move."""
    from conftest import load_golden
    from orv_amd import get_optimizer, schedulers, sft
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    dev = _dev()
    cfg, extra, ins, w, outs = load_golden("fwd_actions")
    sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                              beta_schedule="scaled_linear", prediction_type="v_prediction",
                                              rescale_betas_zero_snr=True, snr_shift_scale=3.0, timestep_spacing="trailing")
    g0 = torch.Generator().manual_seed(9)
    x0 = torch.randn(2, 3, 16, 8, 12, generator=g0).to(dev, BF)
    batch = sft.Batch(x0, torch.zeros_like(x0), ins["encoder_hidden_states"].to(dev, BF), ins["actions"].to(dev), None, None,
                      torch.ones(3, dtype=torch.bool, device=dev), 1)
    m = CogVideoXTransformer3DModelTraj(**cfg)
    m.load_state_dict(w)
    m = m.to(dev, BF).train()
    m.action_embed.forced_mask = torch.zeros(2, dtype=torch.bool)
    m.add_adapter(r=16, lora_alpha=32)
    base0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == 2 * 4 * cfg["num_layers"]
    hyper = dict(lr=1.0, betas=(0.9, 0.95), beta3=0.98, eps=1e-8, weight_decay=1e-2, decouple=True, use_bias_correction=True, safeguard_warmup=True)
    opt = get_optimizer(params, "prodigy", learning_rate=1.0, weight_decay=1e-2, prodigy_decouple=True, prodigy_use_bias_correction=True,
                        prodigy_safeguard_warmup=True, max_grad_norm=1.0)
    assert type(opt).__name__ == "FusedProdigy"
    opt._build()
    f = opt._flat
    n = f["p"].numel()
    for step in range(3):
        torch.cuda.synchronize()
        before = {k: f[k].cpu().clone() for k in ("p", "lo", "m", "v", "s", "p0")}
        sc = R.scalars_of(f["pstate"].cpu())
        loss, parts = sft.sft_step(m, sched, opt, batch, generator=torch.Generator(device=dev).manual_seed(100 + step))
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and parts["grad_norm"] > 0
        clip = float(torch.clamp(1.0 / (torch.tensor(parts["grad_norm"], dtype=torch.float32) + 1e-6), max=1.0))
        inp = dict(before, g=f["g"][:n].cpu(), seg_start=f["seg_start"].cpu(), active=f["active"].cpu(), seg_step=f["seg_step"].cpu())
        w_old = adamw_ref.rebuild(inp["p"], inp["lo"])
        ref = {}
        for dtype in (torch.float64, torch.float32):
            ref[dtype] = R.flat_step(w_old, inp["g"], inp["p0"], inp["m"], inp["v"], inp["s"], inp["seg_start"], inp["active"], inp["seg_step"],
                                     dict(sc), dtype, clip=clip, **hyper)[0]
        w_gpu = adamw_ref.rebuild(f["p"].cpu(), f["lo"].cpu()).double()
        w64 = ref[torch.float64]
        unit = adamw_ref.fp32_ulp(torch.maximum(torch.maximum(w_old.double().abs(), w64.abs()), (w64 - w_old.double()).abs()))
        yard = float(((ref[torch.float32].double() - w64).abs() / unit).max())
        err = float(((w_gpu - w64).abs() / unit).max())
        print(f"\nprodigy in the model, step {step + 1}: loss {float(loss):.4f}, d {opt.d:.3e}, masters vs float64 in fp32 steps - CPU fp32 "
              f"{yard:.3f}, GPU {err:.3f} (bound {2 * yard:.3f})")
        assert err <= 2 * yard, (step, err, yard)
        if step == 0:
            assert torch.equal(f["p0"].cpu().view(torch.int16), before["p"].view(torch.int16))      # captured before anything moved
    assert opt.k == 3 and opt.d >= 1e-6
    now = m.state_dict()
    assert all(torch.equal(now[k], base0[k]) for k in base0), "a base weight moved"
    assert any(bool((a != b).any()) for a, b in zip(opt.master_params(), [p.detach().float() for p in params])) or bool(f["lo"].any())


def test_argument_validation_returns_a_status_and_a_message_without_a_launch():
    from orv_amd import _lib
    h = _lib.lib()
    dev = _dev()
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    p = buf.data_ptr()
    msg = lambda: h.orv_last_error().decode()
    moments = lambda n=2048, bufs=None, st=p: h.orv_prodigy_moments(*(bufs or [p] * 7), n, p, p, p, 1, st, p, 1.0, 0.9, 0.95, 0.97, 0.0, 1, 0, 0, 1e-6,
                                                                    None, None)
    update = lambda n=2048, eps=1e-8, pp=p: h.orv_prodigy_update(pp, p, p, p, n, p, p, 1, p, eps, 0.0, 1, None)
    assert moments(n=2047) != 0 and "multiple of 2048" in msg()
    assert moments(n=0) != 0 and "multiple of 2048" in msg()
    for i in range(7):
        assert moments(bufs=[None if j == i else p for j in range(7)]) != 0 and "null buffer" in msg()
    assert moments(st=None) != 0 and "null buffer" in msg()
    assert update(n=4097) != 0 and "multiple of 2048" in msg()
    assert update(eps=0.0) != 0 and "eps=0" in msg() and "greater than 0" in msg()
    assert update(pp=None) != 0 and "null buffer" in msg()
    assert h.orv_prodigy_recurrence(None, p, 1, 1.0, 0.9, 0.95, 0.97, 0, 1e-6, 1.0, float("inf"), None) != 0 and "null buffer" in msg()
    assert h.orv_prodigy_recurrence(p, p, 0, 1.0, 0.9, 0.95, 0.97, 0, 1e-6, 1.0, float("inf"), None) != 0 and "nchunks=0" in msg()
    torch.cuda.synchronize()
    assert not bool(buf.any())                                 # nothing was launched: the buffer every pointer named is untouched
