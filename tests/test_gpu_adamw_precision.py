"""GPU: the opt-in parameter-precision modes of the flat fused AdamW (``orv_adamw_flat_ex``, ``FusedAdamW(param_precision=...)``) against
their CPU restatement (tests/adamw_ref.py).  The FORMAT (split / rebuild, stochastic offsets and carry) is held bit for bit; the fp32
ARITHMETIC is held to a float64 evaluation of the same formula, with the error of a CPU fp32 evaluation of it as the yardstick (hipcc's
``powf`` may differ from the CPU's by a step, so bit-equality of the arithmetic between the two machines is not demanded).  The measured
figures are printed; profiles/adamw_precision.txt keeps those of the run the pull request was made with."""
import numpy as np
import pytest
import torch

import adamw_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=1e-3)          # the reference's recipe (base_train.yaml:143-166)
SEG = 2048


def _dev():
    return torch.device("cuda:0")


def _inputs(seed=0):
    """>= 2^20 elements in 4 segments (the third inactive), differing step counts, a clip scalar, weights N(0, 0.02), random low halves;
    forced ties (lo -32768 / 32767), +-0 and the largest finite weight in front."""
    g = torch.Generator().manual_seed(seed)
    sizes = [300 * SEG, 150 * SEG, 40 * SEG, 60 * SEG]
    n = sum(sizes)
    assert n >= 2 ** 20
    p = (torch.randn(n, generator=g) * 0.02).to(BF)
    lo = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int64).to(torch.int16)
    special_p = adamw_ref.bits_bf16(torch.tensor([0x0000, 0x8000, 0x7F7F, 0xFF7F, 0x3C00, 0x3C01, 0xBC00, 0xBC01, 0x0001, 0x8001, 0x0000, 0x8000]))      # (-0 with a negative lo would be a NaN pattern)
    special_lo = torch.tensor([0, 0, -32768, 32767, -32768, -32768, 32767, 32767, -1, 1, 32767, 32767], dtype=torch.int16)
    p[:12], lo[:12] = special_p, special_lo
    p[n - 12:], lo[n - 12:] = special_p, special_lo                                   # ... and in the last (active) segment
    grad = (torch.randn(n, generator=g) * 0.05).to(BF)
    m = torch.randn(n, generator=g) * 0.01
    v = (torch.randn(n, generator=g) * 0.01) ** 2
    for i in (1, n - 11):            # the two -0 weights: in IEEE arithmetic -0 - (-0) is +0, so a zero-sized update keeps -0 only if it is +0
        grad[i], m[i] = grad[i].abs(), m[i].abs()
    starts = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64)
    active = torch.tensor([1, 1, 0, 1], dtype=torch.uint8)
    seg_step = torch.tensor([1, 7, 50, 300], dtype=torch.int32)
    return dict(p=p, lo=lo, g=grad, m=m, v=v, seg_start=starts, active=active, seg_step=seg_step, clip=0.37, step=300, n=n)


def _launch(inp, mode, seed=0, lo=None, **over):
    """-> (p, lo, m, v) on the CPU after one ops.adamw_flat_ex launch on the GPU."""
    from orv_amd import ops
    dev = _dev()
    h = dict(HYPER, **over)
    p, g, m, v = (inp[k].to(dev).clone() for k in "pgmv")
    lo_d = None if lo is None else lo.to(dev).clone()
    clip = torch.tensor([inp["clip"]], dtype=torch.float32, device=dev)
    ops.adamw_flat_ex(p, g, m, v, inp["seg_start"].to(dev), inp["active"].to(dev), h["lr"], h["beta1"], h["beta2"], h["eps"],
                      h["weight_decay"], inp["step"], clip, seg_step=inp["seg_step"].to(dev), lo=lo_d, mode=mode, seed=seed)
    torch.cuda.synchronize()
    return p.cpu(), (None if lo_d is None else lo_d.cpu()), m.cpu(), v.cpu()


def _active_mask(inp):
    act = torch.zeros(inp["n"], dtype=torch.bool)
    s = inp["seg_start"].tolist()
    for i, a in enumerate(inp["active"].tolist()):
        act[s[i]:s[i + 1]] = bool(a)
    return act


def _reference(inp, w, dtype, **over):
    h = dict(HYPER, **over)
    return adamw_ref.flat_update(w, inp["g"].float(), inp["m"], inp["v"], inp["seg_start"], inp["active"], inp["seg_step"], inp["clip"],
                                 h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], inp["step"], dtype)


def test_split_format_is_exact_when_the_master_does_not_move():
    """lr = 0 and wd = 0: the new master is the old one, so p and lo must come back bit for bit (forced ties, +-0, the largest finite weight
    and denormal masters included) while m and v moved; the inactive segment is untouched, lo and moments included."""
    inp = _inputs()
    p, lo, m, v = _launch(inp, 1, lo=inp["lo"], lr=0.0, weight_decay=0.0)
    assert torch.equal(adamw_ref.bf16_bits(p), adamw_ref.bf16_bits(inp["p"]))
    assert torch.equal(lo, inp["lo"])
    act = _active_mask(inp)
    assert bool((m[act] != inp["m"][act]).float().mean() > 0.99) and bool((v[act] != inp["v"][act]).float().mean() > 0.99)
    assert torch.equal(m[~act], inp["m"][~act]) and torch.equal(v[~act], inp["v"][~act])


def test_split_arithmetic_against_float64_with_the_cpu_fp32_error_as_yardstick():
    """Mode 1: the master rebuilt from the GPU's p and lo against a float64 evaluation of the formula.  Unit: the fp32 step of
    max(|w_old|, |w_new|, |w_new - w_old|).  Yardstick: the worst error, in that unit, of the same formula evaluated in fp32 on the CPU.
    The GPU may show at most twice that (FMA contraction, a one-step powf difference in the bias corrections), on every element.
    m and v: relative 1e-6 of the float64 value; for m, whose two terms may cancel, relative to |b1 m_old| + |(1 - b1) g| (the scale its
    fp32 rounding errors live on - v has two non-negative terms, where this is the plain relative error).  Relative to |m| itself no fp32
    evaluation can hold 1e-6 on these inputs: the CPU fp32 evaluation misses it on 5225 of the 1,044,480 active elements, worst 2.7e-3,
    all where b1 m_old and (1 - b1) g cancel."""
    inp = _inputs()
    w_old = adamw_ref.rebuild(inp["p"], inp["lo"])
    p, lo, m, v = _launch(inp, 1, lo=inp["lo"])
    w_gpu = adamw_ref.rebuild(p, lo)
    w64, m64, v64 = _reference(inp, w_old, torch.float64)
    w32, _, _ = _reference(inp, w_old, torch.float32)
    act = _active_mask(inp) & torch.isfinite(w64)
    unit = adamw_ref.fp32_ulp(torch.maximum(torch.maximum(w_old.double().abs(), w64.abs()), (w64 - w_old.double()).abs()))
    yard = float(((w32.double() - w64).abs() / unit)[act].max())
    got = float(((w_gpu.double() - w64).abs() / unit)[act].max())
    print(f"\nadamw split_fp32 arithmetic: worst error vs float64 in fp32 steps - CPU fp32 (yardstick) {yard:.3f}, GPU {got:.3f} "
          f"(bound {2 * yard:.3f}); bit-equal to the CPU fp32 evaluation on {float((adamw_ref.f32_bits(w_gpu) == adamw_ref.f32_bits(w32))[act].double().mean()):.6f} of the elements")
    assert got <= 2 * yard, (got, yard)
    inact = ~_active_mask(inp)
    assert torch.equal(adamw_ref.bf16_bits(p)[inact], adamw_ref.bf16_bits(inp["p"])[inact]) and torch.equal(lo[inact], inp["lo"][inact])
    assert torch.equal(m[inact], inp["m"][inact]) and torch.equal(v[inact], inp["v"][inact])
    act = _active_mask(inp)
    b1 = float(torch.tensor(HYPER["beta1"], dtype=torch.float32))
    m_scale = (b1 * inp["m"].double()).abs() + ((1 - b1) * inp["g"].double() * float(torch.tensor(inp["clip"], dtype=torch.float32))).abs()
    m_err = float(((m.double() - m64).abs() / m_scale)[act].max())
    v_err = float(((v.double() - v64).abs() / v64.abs())[act].max())
    print(f"adamw split_fp32 moments vs float64: m {m_err:.3e}, v {v_err:.3e} (bound 1e-6)")
    assert m_err <= 1e-6 and v_err <= 1e-6


def test_stochastic_rounding_is_the_integer_definition_bit_for_bit():
    """Mode 2 shares the fp32 arithmetic with mode 1, so its fp32 result is the mode-1 master of the same inputs with incoming lo = 0;
    then p == (master_bits + r) >> 16 for every element, r from the Python restatement of the hash for that seed, step and flat index."""
    inp = _inputs(1)
    zero = torch.zeros_like(inp["lo"])
    act = _active_mask(inp)
    carried = 0
    # second pass: a negative decay of 1e-3 at lr 1 lifts the largest finite weights above the largest finite bf16, where r may carry the
    # value into infinity: those must come out as the largest finite bf16
    for over in ({}, dict(lr=1.0, weight_decay=-1e-3)):
        p1, lo1, m1, v1 = _launch(inp, 1, lo=zero, **over)
        master = adamw_ref.rebuild(p1, lo1)
        for seed in (0, 0xDEADBEEF):
            p2, _, m2, v2 = _launch(inp, 2, seed=seed, **over)
            r = adamw_ref.sr_offsets(seed, inp["step"], np.arange(inp["n"]))
            want = adamw_ref.stochastic_round(master, r)
            assert torch.equal(adamw_ref.bf16_bits(p2)[act], adamw_ref.bf16_bits(want)[act]), seed
            assert torch.equal(adamw_ref.bf16_bits(p2)[~act], adamw_ref.bf16_bits(inp["p"])[~act])
            assert torch.equal(m2, m1) and torch.equal(v2, v1)
            plain = ((adamw_ref.f32_bits(master) + r) & 0xFFFFFFFF) >> 16
            ok = act & torch.isfinite(master) & ((plain & 0x7FFF) < 0x7F80)
            assert torch.equal(adamw_ref.bf16_bits(p2)[ok], plain[ok])
            over_top = act & torch.isfinite(master) & ((plain & 0x7FFF) >= 0x7F80)
            carried += int(over_top.sum())
            assert bool((adamw_ref.bf16_bits(p2)[over_top] & 0x7FFF == 0x7F7F).all())
    assert carried > 0


def test_mode_0_through_the_new_entry_point_gives_the_bytes_of_adamw_flat():
    from orv_amd import ops
    dev = _dev()
    inp = _inputs(2)
    outs = []
    for use_ex in (False, True):
        p, g, m, v = (inp[k].to(dev).clone() for k in "pgmv")
        clip = torch.tensor([inp["clip"]], dtype=torch.float32, device=dev)
        args = (p, g, m, v, inp["seg_start"].to(dev), inp["active"].to(dev), HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"],
                HYPER["weight_decay"], inp["step"], clip)
        if use_ex:
            ops.adamw_flat_ex(*args, seg_step=inp["seg_step"].to(dev), lo=None, mode="bf16", seed=9)
        else:
            ops.adamw_flat(*args, seg_step=inp["seg_step"].to(dev))
        torch.cuda.synchronize()
        outs.append((p.cpu(), m.cpu(), v.cpu()))
    (pa, ma, va), (pb, mb, vb) = outs
    assert torch.equal(adamw_ref.bf16_bits(pa), adamw_ref.bf16_bits(pb)) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(adamw_ref.bf16_bits(pa), adamw_ref.bf16_bits(inp["p"]))
    with pytest.raises(RuntimeError, match="lo"):
        ops.adamw_flat_ex(*args, lo=None, mode="split_fp32")
    with pytest.raises(RuntimeError, match="int16"):
        ops.adamw_flat_ex(*args, lo=torch.zeros(inp["n"], dtype=torch.int32, device=dev), mode=1)


def _hundred_steps(mode, seed=0):
    from orv_amd.optim import FusedAdamW
    dev = _dev()
    p = torch.nn.Parameter(torch.ones(2 ** 20, device=dev, dtype=BF))
    opt = FusedAdamW([p], lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, param_precision=mode, seed=seed)
    g = torch.ones(2 ** 20, device=dev, dtype=BF)
    for _ in range(100):
        p.grad = g
        opt.step()
    torch.cuda.synchronize()
    return p.detach().cpu(), opt.master_params()[0].cpu()


def test_updates_below_half_a_bf16_step_are_lost_by_default_and_kept_by_the_new_modes():
    """One parameter of 2^20 ones, gradient all ones, lr 1e-3, no decay, no clipping, 100 steps: every step moves the weight by lr, which is
    below half a bf16 step under 1.0 (1.95e-3).  The default leaves every element at exactly 1.0; the split master arrives at 0.9 and the
    bf16 weight is its tie-away rounding; the stochastic mode arrives at 0.9 in the mean (6 standard errors of the sample's own spread),
    the same bits for the same seed and others for another."""
    p, _ = _hundred_steps("bf16")
    assert bool((p.float() == 1.0).all())
    p, master = _hundred_steps("split_fp32")
    rel = float(((master.double() - 0.9).abs() / 0.9).max())
    print(f"\nadamw 100 steps of 1e-3 from 1.0: split_fp32 master worst relative distance from 0.9 = {rel:.3e} (bound 1e-5)")
    assert rel <= 1e-5
    assert torch.equal(adamw_ref.bf16_bits(p), adamw_ref.bf16_bits(adamw_ref.split(master)[0]))
    p, _ = _hundred_steps("stochastic", seed=0)
    x = p.double()
    se = float(x.std()) / x.numel() ** 0.5
    z = (float(x.mean()) - 0.9) / se
    print(f"adamw 100 steps of 1e-3 from 1.0: stochastic mean {float(x.mean()):.6f}, per-element std {float(x.std()):.3e}, standard error {se:.3e}, z = {z:.2f}")
    assert se > 0 and abs(z) <= 6
    again, _ = _hundred_steps("stochastic", seed=0)
    assert torch.equal(adamw_ref.bf16_bits(p), adamw_ref.bf16_bits(again))
    other, _ = _hundred_steps("stochastic", seed=1)
    assert not torch.equal(adamw_ref.bf16_bits(p), adamw_ref.bf16_bits(other))


def _distance(a, b, init):
    """mean |a - b| over all elements of all parameters, in units of the mean parameter movement |b - init|."""
    num = sum(float((x.double() - y.double()).abs().sum()) for x, y in zip(a, b))
    den = sum(float((y.double() - z.double()).abs().sum()) for y, z in zip(b, init))
    return num / den


def test_split_fp32_follows_torch_adamw_in_fp32_and_the_default_does_not():
    """The layout of test_gpu_backward.py::test_fused_adamw_flat_matches_torch_adamw (an Attention module's parameters, an odd-sized one,
    one that never has a gradient, one without a gradient on some steps; clipping on), 20 steps with the reference's hyper-parameters.
    The torch side holds fp32 parameters and gets the same bf16 gradients upcast.  Yardstick: the distance of torch's own fp32 AdamW from
    torch's float64 AdamW on these inputs (CPU); the split masters may be 8 x that from the fp32 torch parameters (operation order and
    powf differ), and the default mode must be at least 100 x further away than the split mode."""
    from orv_amd.cogvideox_control import Attention
    from orv_amd.optim import FusedAdamW
    dev = _dev()
    torch.manual_seed(0)
    at = Attention(128, 2, 64, bias=True, out_bias=True)
    shapes = [tuple(p.shape) for p in at.parameters()] + [(777,), (33,), (5000,)]
    gen = torch.Generator().manual_seed(3)
    init = [p.detach().to(BF) for p in at.parameters()] + [torch.randn(s, generator=gen).mul_(0.02).to(BF) for s in shapes[-3:]]
    i_unused, i_sometimes = len(shapes) - 2, len(shapes) - 1
    steps = 20
    grads = [[None if i == i_unused or (i == i_sometimes and it % 3 == 1)
              else (torch.randn(s, generator=gen) * (3.0 if it == 0 else 0.05)).to(BF) for i, s in enumerate(shapes)] for it in range(steps)]
    kw = dict(lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], weight_decay=HYPER["weight_decay"])

    def torch_run(dtype):
        ref = [x.to(dtype).clone().requires_grad_(True) for x in init]
        topt = torch.optim.AdamW(ref, **kw)
        for it in range(steps):
            for r, g in zip(ref, grads[it]):
                r.grad = None if g is None else g.to(dtype)
            torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], 1.0)
            topt.step()
        return [r.detach() for r in ref]

    t32, t64 = torch_run(torch.float32), torch_run(torch.float64)
    yard = _distance(t32, t64, init)

    def fused_run(mode):
        params = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
        opt = FusedAdamW(params, max_grad_norm=1.0, param_precision=mode, **kw)
        for it in range(steps):
            for p, g in zip(params, grads[it]):
                p.grad = None if g is None else g.to(dev)
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        by_param = {id(p): mp_.cpu() for p, mp_ in zip(opt.params, opt.master_params())}
        assert opt._flat["seg_step"].tolist() == [0 if p is params[i_unused] else (13 if p is params[i_sometimes] else 20) for p in opt.params]
        return [by_param[id(p)] for p in params], [p.detach().cpu() for p in params]

    split_m, split_p = fused_run("split_fp32")
    plain_m, plain_p = fused_run("bf16")
    d_split, d_plain = _distance(split_m, t32, init), _distance(plain_m, t32, init)
    print(f"\nadamw 20 steps vs torch.optim.AdamW fp32, in units of the mean parameter movement: torch fp32 vs torch float64 (yardstick) {yard:.3e}, "
          f"split_fp32 masters vs torch fp32 {d_split:.3e} (bound {8 * yard:.3e}), default bf16 vs torch fp32 {d_plain:.3e} "
          f"(ratio {d_plain / d_split:.0f}, at least 100)")
    assert d_split <= 8 * yard, (d_split, yard)
    assert d_plain >= 100 * d_split, (d_plain, d_split)
    assert torch.equal(split_m[i_unused], init[i_unused].float()) and torch.equal(plain_p[i_unused], init[i_unused])
    for mst, p in zip(split_m, split_p):
        assert torch.equal(adamw_ref.bf16_bits(p), adamw_ref.bf16_bits(adamw_ref.split(mst)[0]))


def test_split_fp32_in_the_model_three_sft_steps():
    """Three sft_step calls on the small golden-config model with param_precision="split_fp32": after each, every parameter is the tie-away
    rounding of its master, the weights epoch moved (derived-weight caches and captured graphs are dropped as in the default) and a forward
    reads the new weights."""
    from conftest import load_golden
    from orv_amd import _state, schedulers, sft
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    from orv_amd.optim import FusedAdamW
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
    opt = FusedAdamW(m.parameters(), lr=2e-4, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0, param_precision="split_fp32")
    attn = m.transformer_blocks[0].attn1
    prev_masters = None
    for step in range(3):
        epoch = _state.weights_epoch[0]
        loss, parts = sft.sft_step(m, sched, opt, batch, generator=torch.Generator(device=dev).manual_seed(100 + step))
        assert torch.isfinite(loss) and parts["grad_norm"] > 0
        assert _state.weights_epoch[0] > epoch
        masters = opt.master_params()
        for p, mst in zip(opt.params, masters):
            assert torch.equal(adamw_ref.bf16_bits(p.detach()), adamw_ref.bf16_bits(adamw_ref.split(mst.cpu())[0]))
        if prev_masters is not None:
            moved = sum(int((a != b).sum()) for a, b in zip(masters, prev_masters)) / sum(a.numel() for a in masters)
            assert moved > 0.5, moved                                      # at lr 2e-4 most bf16 weights stand still; the masters do not
        prev_masters = masters
        wq, _ = attn.packed_qkv()
        assert torch.equal(wq, torch.cat([attn.to_q.weight, attn.to_k.weight, attn.to_v.weight]).detach())
    assert int(opt._flat["lo"].abs().max()) > 0
