"""CPU: the fused Prodigy optimizer's rule (tests/prodigy_ref.py), the host logic of ``FusedProdigy`` over CPU stand-ins of its three kernels
(test infrastructure, never shipped: flat storage, p0 capture, skip rules, checkpointing and the data-parallel bookkeeping are the product
code), and the ``get_optimizer`` surface of the reference."""
import ast
import inspect
import math
import os
import socket
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import adamw_ref
import prodigy_ref as R

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule ----
def test_reference_reproduces_the_master_run_and_the_bf16_stall():
    """n = 4096, weights N(0, 0.02^2) in bf16, loss 1/2 |w - target|^2, bf16 gradients, lr 1, betas 0.9 / 0.95, 60 steps.  With the fp32
    master d leaves d0 (1.73e-6 at step 6, 6.8e-4 at step 21), reaches 1.23e-2 at step 41 and stays; the mean squared distance ends below
    1e-5.  With bf16 weights every update vanishes, p0 - w stays 0 and d is d0 at all 60 steps."""
    hist, loss = R.quadratic_run(torch.float64)
    print(f"\nprodigy fp32 master: d {hist[0]:.3e} -> {hist[5]:.3e} (6) -> {hist[20]:.3e} (21) -> {hist[40]:.3e} (41) -> {hist[59]:.3e} (60), loss {loss:.3e}")
    assert hist[0] == 1e-6 and abs(hist[5] - 1.73e-6) <= 1e-8 and abs(hist[20] - 6.8e-4) <= 1e-5
    assert abs(hist[40] - 1.23e-2) <= 1e-3 and hist[59] == hist[40]
    assert loss < 1e-5
    stalled, loss_bf16 = R.quadratic_run(torch.float64, weights_mode="bf16")
    print(f"prodigy bf16 weights: d in {set(stalled)}, loss {loss_bf16:.3e}")
    assert len(stalled) == 60 and all(d == 1e-6 for d in stalled)
    assert loss_bf16 > 50 * loss
    h32, loss32 = R.quadratic_run(torch.float32)
    rel = max(abs(a - b) / b for a, b in zip(h32, hist))
    print(f"prodigy fp32 restatement vs float64: worst relative error of d over the run {rel:.3e}, at step 60 {abs(h32[-1] - hist[-1]) / hist[-1]:.3e}")
    assert rel < 1e-2 and loss32 < 1e-5


def _hand_step(w, g, st, sc, lr, b1, b2, b3, eps, wd, decouple, bias, safeguard, d0, d_coef, growth):
    """The rule on Python floats, one element at a time (independent of the tensor code)."""
    d, k = sc["d"], sc["k"]
    bc = math.sqrt(1 - b2 ** (k + 1)) / (1 - b1 ** (k + 1)) if bias else 1.0
    dlr = d * lr * bc
    num, den = b3 * sc["num"], 0.0
    for i in range(len(w)):
        if st["p0"][i] is None:
            st["p0"][i] = w[i]
        gi = g[i] + (wd * w[i] if wd and not decouple else 0.0)
        g[i] = gi
        num += (d / d0) * dlr * gi * (st["p0"][i] - w[i])
        st["m"][i] = b1 * st["m"][i] + d * (1 - b1) * gi
        st["v"][i] = b2 * st["v"][i] + d * d * (1 - b2) * gi * gi
        st["s"][i] = b3 * st["s"][i] + (d / d0) * (d if safeguard else dlr) * gi
        den += abs(st["s"][i])
    if den == 0:
        return
    d_hat = d_coef * num / den
    if d == d0:
        d = max(d, d_hat)
    sc["d_max"] = max(sc["d_max"], d_hat)
    sc["d"] = min(sc["d_max"], d * growth)
    sc["num"] = num
    for i in range(len(w)):
        if wd and decouple:
            w[i] = w[i] - wd * dlr * w[i]
        w[i] = w[i] - dlr * st["m"][i] / (math.sqrt(st["v"][i]) + sc["d"] * eps)
    sc["k"] = k + 1


def test_one_step_computed_by_hand_on_four_elements():
    """w = (1, -2, 1/2, 1/4), g = w - (3, 1, -2, 2) = (-2, -3, 5/2, -7/4), fresh state, d0 = 2^-10, lr 1/2, betas 1/2 and 3/4, beta3 7/8,
    eps 2^-20, no decay.  By hand: dlr = 2^-11; p0 = w, so the numerator is 0, d_hat = 0 and d stays d0; m = d (1 - b1) g = 2^-11 g;
    v = d^2 (1 - b2) g^2 = 2^-22 g^2; s = (d / d0) dlr g = 2^-11 g; den = 2^-11 (2 + 3 + 5/2 + 7/4) = 37 / 8192;
    w - dlr m / (sqrt(v) + d eps) = w - 2^-11 g / (|g| + 2^-19).  The literals are those fractions evaluated exactly and rounded to double."""
    w0, g = [1.0, -2.0, 0.5, 0.25], [-2.0, -3.0, 2.5, -1.75]
    hyper = dict(lr=0.5, betas=(0.5, 0.75), beta3=0.875, eps=2.0 ** -20, d0=2.0 ** -10)
    want = dict(m=[-0.0009765625, -0.00146484375, 0.001220703125, -0.0008544921875],
                v=[9.5367431640625e-07, 2.1457672119140625e-06, 1.4901161193847656e-06, 7.301568984985352e-07],
                s=[-0.0009765625, -0.00146484375, 0.001220703125, -0.0008544921875],
                w=[1.0004882807843392, -1.9995117190604406, 0.49951171912252873, 0.25048828071781626])
    for dtype, tol in ((torch.float64, 1e-15), (torch.float32, 2e-7)):
        weights, states, sc = [torch.tensor(w0, dtype=dtype)], [R.new_param_state(torch.tensor(w0, dtype=dtype))], R.new_scalars(2.0 ** -10)
        num, den = R.step(weights, [torch.tensor(g, dtype=BF)], states, sc, dtype, **hyper)
        assert num == 0.0 and den == 0.0045166015625                      # 37 / 8192: every term and the sum are exact in fp32
        assert (sc["d"], sc["d_max"], sc["d_numerator"], sc["d_hat"], sc["k"], sc["dlr"], sc["skip"]) == (2.0 ** -10, 2.0 ** -10, 0.0, 0.0, 1, 2.0 ** -11, 0)
        for name in "mvs":
            assert states[0][name].tolist() == want[name], (dtype, name)         # powers of two times small integers: exact in both dtypes
        assert torch.equal(states[0]["p0"], torch.tensor(w0, dtype=dtype))
        assert max(abs(a - b) / abs(b) for a, b in zip(weights[0].tolist(), want["w"])) <= tol, (dtype, weights[0].tolist())
    # the stand-ins of the three kernels (what FusedProdigy runs on the CPU) give the same step on a one-chunk flat buffer
    pad = lambda x, dt: torch.cat([torch.tensor(x, dtype=dt), torch.zeros(2044, dtype=dt)])
    p, lo, gg, p0 = pad(w0, BF), pad([0] * 4, torch.int16), pad(g, BF), pad([0.0] * 4, BF)
    m, v, s_ = (pad([0.0] * 4, torch.float32) for _ in range(3))
    state, partials = R.state_tensor(R.new_scalars(2.0 ** -10)), torch.zeros(2, dtype=torch.float64)
    seg = (torch.tensor([0, 2048]), torch.tensor([1], dtype=torch.uint8))
    R.prodigy_moments(p, lo, gg, p0, m, v, s_, *seg, torch.tensor([1], dtype=torch.int32), state, partials, 0.5, 0.5, 0.75, 0.875, d0=2.0 ** -10)
    R.prodigy_recurrence(state, partials, 0.5, 0.5, 0.75, 0.875, d0=2.0 ** -10)
    R.prodigy_update(p, lo, m, v, *seg, state, 2.0 ** -20)
    assert partials.tolist() == [0.0, 0.0045166015625] and state.tolist() == [2.0 ** -10, 2.0 ** -10, 0.0, 0.0045166015625, 0.0, 1.0, 2.0 ** -11, 0.0]
    assert m[:4].tolist() == want["m"] and v[:4].tolist() == want["v"] and s_[:4].tolist() == want["s"] and p0[:4].tolist() == w0
    got = adamw_ref.rebuild(p, lo)[:4].tolist()
    assert max(abs(a - b) / abs(b) for a, b in zip(got, want["w"])) <= 2e-7, got
    assert not bool(p[4:].float().any()) and not bool(lo[4:].any())


@pytest.mark.parametrize("decouple,bias,safeguard,wd", [(True, False, False, 0.0), (False, True, True, 0.25), (True, True, False, 0.25)])
def test_steps_by_hand_on_four_elements(decouple, bias, safeguard, wd):
    """Eight steps on four elements towards a target (gradient w - target, rounded to bf16) against the rule written out on Python floats;
    from the second step on the numerator is non-zero, and d0 = 2^-10 is large enough that d moves within the eight."""
    w0 = [1.0, -2.0, 0.5, 0.25]
    target, d0 = torch.tensor([3.0, 1.0, -2.0, 2.0], dtype=torch.float64), 2.0 ** -10
    hyper = dict(lr=0.5, betas=(0.5, 0.75), beta3=0.875, eps=2.0 ** -20, weight_decay=wd, decouple=decouple, use_bias_correction=bias,
                 safeguard_warmup=safeguard, d0=d0, d_coef=2.0, growth_rate=4.0)
    weights, states, sc = [torch.tensor(w0, dtype=torch.float64)], [R.new_param_state(torch.tensor(w0, dtype=torch.float64))], R.new_scalars(d0)
    hw, hst = list(w0), dict(m=[0.0] * 4, v=[0.0] * 4, s=[0.0] * 4, p0=[None] * 4)
    hsc = dict(d=d0, d_max=d0, num=0.0, k=0)
    moved = False
    for _ in range(8):
        g = (weights[0] - target).to(BF)
        R.step(weights, [g], states, sc, torch.float64, **hyper)
        _hand_step(hw, g.double().tolist(), hst, hsc, 0.5, 0.5, 0.75, 0.875, 2.0 ** -20, wd, decouple, bias, safeguard, d0, 2.0, 4.0)
        assert sc["k"] == hsc["k"]
        for got, want in ((sc["d"], hsc["d"]), (sc["d_max"], hsc["d_max"]), (sc["d_numerator"], hsc["num"])):
            assert abs(got - want) <= 1e-13 * max(abs(want), 1e-30), (got, want)
        for name, got in (("m", states[0]["m"]), ("v", states[0]["v"]), ("s", states[0]["s"]), ("w", weights[0])):
            want = torch.tensor(hw if name == "w" else hst[name], dtype=torch.float64)
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-300), name
        moved |= sc["d"] != d0
    assert moved and sc["k"] == 8
    assert torch.equal(states[0]["p0"], torch.tensor(w0, dtype=torch.float64))


def test_growth_rate_caps_d_and_a_zero_gradient_step_is_skipped():
    w = [torch.tensor([1.0, -1.0], dtype=torch.float64)]
    st, sc = [R.new_param_state(w[0])], R.new_scalars()
    R.step(w, [torch.zeros(2, dtype=BF)], st, sc, torch.float64)
    assert sc["k"] == 0 and sc["skip"] == 1 and sc["d"] == 1e-6 and torch.equal(w[0], torch.tensor([1.0, -1.0], dtype=torch.float64))
    for _ in range(12):
        before = sc["d"]
        R.step(w, [(w[0] - 3.0).to(BF)], st, sc, torch.float64, growth_rate=1.5)
        assert before == 1e-6 or sc["d"] <= before * 1.5 * (1 + 1e-15)       # the jump away from d0 itself is not capped (d = max(d, d_hat) first)
    assert sc["d"] > 1e-6 and sc["k"] == 12


# ---- FusedProdigy over the stand-ins ----
def _install_standins(calls=None):
    from orv_amd import ops

    def sumsq(g, out):
        out.add_(g.float().pow(2).sum())

    def spy(name, fn):
        def f(*a, **k):
            if calls is not None:
                calls.append((name, a, k))
            return fn(*a, **k)
        return f

    ops.sumsq = sumsq
    ops.prodigy_moments = spy("prodigy_moments", R.prodigy_moments)
    ops.prodigy_recurrence = spy("prodigy_recurrence", R.prodigy_recurrence)
    ops.prodigy_update = spy("prodigy_update", R.prodigy_update)


_NAMES = ("sumsq", "prodigy_moments", "prodigy_recurrence", "prodigy_update", "adamw_flat", "adamw_flat_ex", "adamw_flat_s8")


@pytest.fixture
def standins():
    from orv_amd import ops
    saved = {n: getattr(ops, n) for n in _NAMES}
    calls = []
    _install_standins(calls)
    yield calls
    for n, fn in saved.items():
        setattr(ops, n, fn)


_SHAPES = {"A": (64, 40), "B": (3000,), "C": (17, 9), "D": (5,)}
_KW = dict(lr=1.0, betas=(0.9, 0.95), weight_decay=0.0, max_grad_norm=0.0)


def _params(seed=7):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(BF)) for n, s in _SHAPES.items()}


def _grad(name, step, scale=0.05):
    g = torch.Generator().manual_seed(100 * step + sum(map(ord, name)))
    return (torch.randn(_SHAPES[name], generator=g) * scale).to(BF)


# A every step, B every step but the second, C first used at step 3 (index 2), D never
_USED = {"A": lambda t: True, "B": lambda t: t != 1, "C": lambda t: t >= 2, "D": lambda t: False}


def _feed(params, t):
    for n, p in params.items():
        p.grad = _grad(n, t) if _USED[n](t) else None


def _reference_run(steps, **hyper):
    """The list-of-parameters reference (fp32 evaluation) on the same gradients."""
    init = _params()
    names = list(_SHAPES)
    weights = [init[n].detach().float() for n in names]
    states, sc = [R.new_param_state(w) for w in weights], R.new_scalars()
    for t in range(steps):
        R.step(weights, [_grad(n, t) if _USED[n](t) else None for n in names], states, sc, torch.float32, **hyper)
    return dict(zip(names, weights)), dict(zip(names, states)), sc


def test_fused_prodigy_follows_the_reference_and_captures_p0_at_each_first_use(standins):
    from orv_amd.optim import FusedProdigy
    params = _params()
    init = {n: p.detach().clone() for n, p in params.items()}
    opt = FusedProdigy(params.values(), **_KW)
    assert (opt.d, opt.d_max, opt.k) == (1e-6, 1e-6, 0)
    for t in range(5):
        _feed(params, t)
        if t == 2:
            c_before = opt.master_params()[2].clone()
        norm = opt.step()
        opt.zero_grad()
        assert norm > 0
    ref_w, ref_st, sc = _reference_run(5, lr=1.0, betas=(0.9, 0.95), weight_decay=0.0)
    assert opt.k == 5 == sc["k"] and opt.d == sc["d"] and opt.d_max == sc["d_max"] and opt.dlr == sc["dlr"] and opt.d_hat == sc["d_hat"]
    masters = dict(zip(_SHAPES, opt.master_params()))
    s, p0 = (dict(zip(_SHAPES, x)) for x in opt.prodigy_state())
    m, v = (dict(zip(_SHAPES, x)) for x in opt.moments())
    for n in "ABC":
        assert torch.equal(masters[n], ref_w[n]), n
        assert torch.equal(s[n], ref_st[n]["s"]) and torch.equal(m[n], ref_st[n]["m"]) and torch.equal(v[n], ref_st[n]["v"]), n
        assert torch.equal(params[n].detach(), adamw_ref.split(masters[n])[0])       # the model reads the rounding of the master
    assert torch.equal(p0["A"], init["A"]) and torch.equal(p0["B"], init["B"])       # captured at the first step, before anything moved
    assert torch.equal(p0["C"].float(), adamw_ref.split(c_before)[0].float()) and torch.equal(p0["C"], init["C"])     # ... at step 3
    assert not torch.equal(masters["A"], init["A"].float())
    # D never had a gradient: every buffer of its segment is untouched
    assert torch.equal(params["D"].detach(), init["D"]) and torch.equal(masters["D"], init["D"].float())
    for x in (s["D"], m["D"], v["D"], p0["D"].float()):
        assert not bool(x.any())
    assert opt._flat["seg_step"].tolist() == [5, 4, 3, 0]
    # three launches per step, in order, lr and clip handed to the first
    assert [c[0] for c in standins] == ["prodigy_moments", "prodigy_recurrence", "prodigy_update"] * 5


def test_inactive_parameter_keeps_every_byte_in_a_step_it_sits_out(standins):
    from orv_amd.optim import FusedProdigy
    params = _params()
    opt = FusedProdigy(params.values(), **_KW)
    _feed(params, 0); opt.step(); opt.zero_grad()
    f = opt._flat
    a, b = f["offs"][1], f["offs"][2]
    before = {k: f[k][a:b].clone() for k in ("p", "lo", "m", "v", "s", "p0")}
    assert bool(before["m"].any()) and bool(before["s"].any())
    _feed(params, 1); opt.step(); opt.zero_grad()          # B sits out step index 1
    for k, x in before.items():
        assert torch.equal(f[k][a:b], x), k
    assert opt.k == 2


def test_zero_gradient_step_leaves_the_weights_and_k_alone(standins):
    from orv_amd.optim import FusedProdigy
    params = _params()
    init = {n: p.detach().clone() for n, p in params.items()}
    opt = FusedProdigy(params.values(), **_KW)
    for p in params.values():
        p.grad = torch.zeros_like(p)
    assert opt.step() == 0.0
    assert opt.k == 0 and opt.d == 1e-6 and opt._scalar("skip") == 1.0
    assert all(torch.equal(params[n].detach(), init[n]) for n in _SHAPES) and not bool(opt._flat["lo"].any())
    assert all(torch.equal(x, init[n]) for n, x in zip(_SHAPES, opt.prodigy_state()[1]))       # p0 was captured and is still the weight
    opt.zero_grad()
    _feed(params, 0); opt.step()
    assert opt.k == 1 and opt._scalar("skip") == 0.0 and not torch.equal(opt.master_params()[0], init["A"].float())
    # p0 of a parameter whose first (skipped) step moved nothing is still the starting weight
    assert torch.equal(opt.prodigy_state()[1][0], init["A"])


def test_state_dict_round_trip_continues_bit_for_bit(standins):
    from orv_amd.optim import FusedProdigy
    kw = dict(_KW, weight_decay=1e-2, use_bias_correction=True, max_grad_norm=1.0)

    def run(split_at):
        params = _params()
        opt = FusedProdigy(params.values(), **kw)
        for t in range(6):
            if t == split_at:
                sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
                weights = {n: p.detach().clone() for n, p in params.items()}
                params = _params(seed=99)
                with torch.no_grad():
                    for n, p in params.items():
                        p.copy_(weights[n])
                opt = FusedProdigy(params.values(), **kw)
                opt.load_state_dict(sd)
                assert opt.k == t
            _feed(params, t); opt.step(); opt.zero_grad()
        return opt

    a, b = run(None), run(3)
    for key in ("p", "lo", "m", "v", "s", "p0", "pstate", "seg_step"):
        assert torch.equal(a._flat[key], b._flat[key]), key
    sd = a.state_dict()
    assert sd["optimizer"] == "prodigy" and sd["prodigy_state"].dtype == torch.float64 and sd["prodigy_state"].numel() == 8
    assert set(("exp_avg", "exp_avg_sq", "prodigy_s", "prodigy_p0", "param_lo", "seg_step")) <= set(sd)
    # an AdamW checkpoint (moments without the Prodigy state) is refused, not misread
    fresh = FusedProdigy(_params().values(), **kw)
    with pytest.raises(ValueError, match="no Prodigy state"):
        fresh.load_state_dict({k: v for k, v in sd.items() if not k.startswith("prodigy_")})
    # ... and FusedAdamW does not take Prodigy's d-scaled moments for its own
    from orv_amd.optim import FusedAdamW
    adam = FusedAdamW(_params().values(), param_precision="split_fp32")
    with pytest.raises(ValueError, match=r"FusedAdamW.load_state_dict: the checkpoint was written by the 'prodigy' optimizer"):
        adam.load_state_dict(sd)
    assert adam._flat is None and adam.step_count == 0


def test_refusals_name_the_reason_and_the_supported_set():
    from orv_amd.optim import FusedProdigy
    ps = list(_params().values())
    for mode in ("bf16", "stochastic"):
        with pytest.raises(ValueError, match=r"vanish in bf16.*d never grows.*split_fp32"):
            FusedProdigy(ps, param_precision=mode)
    with pytest.raises(ValueError, match=r"state_precision='fp8'.*supported: 'fp32'"):
        FusedProdigy(ps, state_precision="fp8")
    with pytest.raises(ValueError, match="unknown param_precision"):
        FusedProdigy(ps, param_precision="fp64")
    with pytest.raises(ValueError, match="eps=0"):
        FusedProdigy(ps, eps=0)
    opt = FusedProdigy(ps)
    assert opt.param_precision == "split_fp32" and opt.state_precision == "fp32" and opt.betas == (0.9, 0.999)
    assert opt.beta3 == math.sqrt(0.999) and opt.decouple and not opt.use_bias_correction and not opt.safeguard_warmup
    assert (opt.param_groups[0]["lr"], opt.eps, opt.weight_decay, opt.d0, opt.d_coef, opt.growth_rate) == (1.0, 1e-8, 0.0, 1e-6, 1.0, float("inf"))
    for name in ("d", "d_max", "d_hat", "k", "dlr"):
        with pytest.raises(AttributeError):
            setattr(opt, name, 1.0)


def test_lr_schedule_is_read_at_every_step(standins):
    from orv_amd.optim import FusedProdigy, get_scheduler
    params = _params()
    opt = FusedProdigy(params.values(), **_KW)
    sched = get_scheduler("linear", opt, num_warmup_steps=2, num_training_steps=6)
    want = []
    for t in range(4):
        want.append(opt.param_groups[0]["lr"])
        _feed(params, t); opt.step(); opt.zero_grad(); sched.step()
    assert want == [0.0, 0.5, 1.0, 0.75]
    lrs = [c[1][12] for c in standins if c[0] == "prodigy_moments"]
    lrs2 = [c[1][2] for c in standins if c[0] == "prodigy_recurrence"]
    assert lrs == want and lrs2 == want


# ---- get_optimizer ----
_REFERENCE_SIGNATURE = [          # orv/utils.py:16-34 of the reference: names, order, defaults
    ("params_to_optimize", inspect.Parameter.empty), ("optimizer_name", "adam"), ("learning_rate", 1e-3), ("beta1", 0.9), ("beta2", 0.95),
    ("beta3", 0.98), ("epsilon", 1e-8), ("weight_decay", 1e-4), ("prodigy_decouple", False), ("prodigy_use_bias_correction", False),
    ("prodigy_safeguard_warmup", False), ("use_8bit", False), ("use_4bit", False), ("use_torchao", False), ("use_deepspeed", False),
    ("use_cpu_offload_optimizer", False), ("offload_gradients", False)]


def test_get_optimizer_signature_is_the_reference_s_plus_two_of_our_own():
    tree = ast.parse(open(os.path.join(ROOT, "orv_amd", "optim.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_optimizer")
    names = [a.arg for a in fn.args.args]
    defaults = [inspect.Parameter.empty] * (len(names) - len(fn.args.defaults)) + [ast.literal_eval(d) for d in fn.args.defaults]
    got = list(zip(names, defaults))
    assert got[:len(_REFERENCE_SIGNATURE)] == _REFERENCE_SIGNATURE
    assert got[len(_REFERENCE_SIGNATURE):] == [("max_grad_norm", 1.0)] and fn.args.kwarg.arg == "fused_kwargs"
    assert not fn.args.kwonlyargs and fn.args.vararg is None
    import orv_amd
    from orv_amd import optim
    assert orv_amd.get_optimizer is optim.get_optimizer and orv_amd.FusedProdigy is optim.FusedProdigy
    assert [p for p in inspect.signature(optim.get_optimizer).parameters][:17] == [n for n, _ in _REFERENCE_SIGNATURE]


def test_get_optimizer_mapping():
    from orv_amd.optim import FusedAdamW, FusedProdigy, get_optimizer
    ps = list(_params().values())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        o = get_optimizer(ps, "adamw", learning_rate=2e-4, weight_decay=1e-3)
        assert type(o) is FusedAdamW and (o.param_groups[0]["lr"], o.betas, o.eps, o.weight_decay, o.max_grad_norm) == (2e-4, (0.9, 0.95), 1e-8, 1e-3, 1.0)
        assert o.state_precision == "fp32" and o.param_precision == "bf16"
        o = get_optimizer(ps, "AdamW", use_8bit=True, param_precision="split_fp32", max_grad_norm=0.5)
        assert type(o) is FusedAdamW and o.state_precision == "fp8" and o.param_precision == "split_fp32" and o.max_grad_norm == 0.5
        o = get_optimizer(ps, "adam", weight_decay=0.0)
        assert type(o) is FusedAdamW and o.weight_decay == 0.0
        o = get_optimizer(ps, "prodigy", learning_rate=1.0, beta3=0.98, weight_decay=1e-2, prodigy_decouple=True,
                          prodigy_use_bias_correction=True, prodigy_safeguard_warmup=True, d0=1e-5)
        assert type(o) is FusedProdigy and (o.param_groups[0]["lr"], o.betas, o.beta3, o.weight_decay) == (1.0, (0.9, 0.95), 0.98, 1e-2)
        assert o.decouple and o.use_bias_correction and o.safeguard_warmup and o.d0 == 1e-5 and o.max_grad_norm == 1.0
        o = get_optimizer(ps, "prodigy", learning_rate=1.0)
        assert not o.decouple and not o.use_bias_correction and not o.safeguard_warmup and o.weight_decay == 1e-4      # the reference's defaults
        # the reference's list of one {"params", "lr"} dict
        o = get_optimizer([{"params": ps, "lr": 3e-4}], "adamw", learning_rate=1.0)
        assert type(o) is FusedAdamW and o.param_groups[0]["lr"] == 3e-4 and len(o.params) == len(ps)
        o = get_optimizer(iter(ps), "adamw")
        assert len(o.params) == len(ps)
    with pytest.warns(UserWarning, match=r"learning_rate=0.1 is small for prodigy.*near 1.0"):
        assert type(get_optimizer(ps, "prodigy", learning_rate=0.1)) is FusedProdigy
    with pytest.warns(UserWarning, match=r"optimizer_name='lion' is not known.*supported: .*adamw, prodigy.*falling back to 'adamw'"):
        assert type(get_optimizer(ps, "Lion")) is FusedAdamW
    with pytest.raises(ValueError, match=r"coupled weight decay.*adamw.*supported"):
        get_optimizer(ps)                                      # the defaults: adam with weight_decay 1e-4
    with pytest.raises(ValueError, match=r"CAME is not built.*supported: .*adamw, prodigy"):
        get_optimizer(ps, "came")
    with pytest.raises(ValueError, match=r"use_8bit=True goes with adam / adamw only, not with 'prodigy'.*supported"):
        get_optimizer(ps, "prodigy", learning_rate=1.0, use_8bit=True)
    for flag in ("use_4bit", "use_torchao", "use_deepspeed", "use_cpu_offload_optimizer"):
        with pytest.raises(ValueError, match=flag + r"=True is not built.*supported: .*adamw, prodigy"):
            get_optimizer(ps, "adamw", **{flag: True})
    with pytest.raises(ValueError, match="vanish in bf16"):
        get_optimizer(ps, "prodigy", learning_rate=1.0, param_precision="bf16")
    # keyword arguments the chosen class does not take are refused with the accepted set, not passed on into a TypeError
    with pytest.raises(ValueError, match=r"FusedProdigy takes no seed \(accepted.*d0, d_coef, growth_rate"):
        get_optimizer(ps, "prodigy", learning_rate=1.0, seed=1)
    with pytest.raises(ValueError, match=r"FusedAdamW takes no d0 \(accepted.*param_precision, state_precision, seed"):
        get_optimizer(ps, "adamw", d0=1e-5)
    assert get_optimizer(ps, "adamw", seed=5, param_precision="stochastic").seed == 5
    with pytest.raises(ValueError, match="one group"):
        get_optimizer([{"params": ps[:1]}, {"params": ps[1:]}], "adamw")


# ---- data parallel: two gloo ranks against one rank on the summed batch ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_DP_STEPS = 6
_DP_USED = {"A": [(1, 1)] * 6, "B": [(1, 0), (0, 0), (1, 0), (0, 1), (1, 1), (1, 0)], "C": [(0, 0), (0, 0), (0, 1), (1, 1), (1, 0), (1, 1)],
            "D": [(0, 0)] * 6}
_DP_KW = dict(lr=1.0, betas=(0.9, 0.95), weight_decay=1e-2, max_grad_norm=0.5, d0=1e-4)


def _dp_grad(name, rank, p):
    """Each rank pulls towards a target of its own (the gradient of 1/2 |w - target_rank|^2), so that the estimate has something to find."""
    g = torch.Generator().manual_seed(10 * rank + sum(map(ord, name)))
    return (p.detach().float() - torch.randn(_SHAPES[name], generator=g) * 0.3).to(BF)


def _dp_result(opt, norms):
    f = opt._flat
    return dict(d=opt.d, d_max=opt.d_max, k=opt.k, norms=norms, **{k: f[k].clone().view(torch.int16 if f[k].dtype == BF else f[k].dtype).numpy()
                                                                  for k in ("p", "lo", "s", "p0")})


def _dp_worker(rank, world, port, max_grad_norm, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_standins()
    from orv_amd.optim import FusedProdigy
    params = _params()
    opt = FusedProdigy(params.values(), **dict(_DP_KW, max_grad_norm=max_grad_norm))
    norms = []
    for t in range(_DP_STEPS):
        for n, p in params.items():
            p.grad = _dp_grad(n, rank, p) if _DP_USED[n][t][rank] else None
        norms.append(opt.step(average_over=world))
        opt.zero_grad()
    out.put((rank, _dp_result(opt, norms)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("max_grad_norm", [0.0, 0.5])
def test_two_ranks_agree_on_d_and_weights_and_match_one_rank_on_the_summed_batch(standins, max_grad_norm):
    """Both ranks end with identical bytes.  Against ONE rank fed the bf16 SUM of the two ranks' gradients with the coefficient halved (what
    the exchange and the 1 / world fold leave the kernels with): without clipping the coefficient is exactly 1 / 2 on both sides and the
    runs are equal bit for bit.  With clipping the two sides form the coefficient differently - max / (norm / 2 + 1e-6) / 2 on two ranks,
    2 max / (norm + 1e-6) / 2 on one, which differ by 1e-6 / norm relative - so that case is held to 1e-5 of d and 1e-4 of the largest weight
    movement; the bound is this test's own set-up, not the optimizer's."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, max_grad_norm, q)) for r in range(2)]
    [p.start() for p in procs]
    got = dict(q.get(timeout=180) for _ in range(2))
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    # one rank, fed what the exchange leaves in the flat buffer: the bf16 SUM of the two ranks' gradients; the mean's 1 / 2 is folded
    # into the clip coefficient there, so here the gradient is the sum and the coefficient is halved the same way
    from orv_amd import ops
    from orv_amd.optim import FusedProdigy
    params = _params()
    opt = FusedProdigy(params.values(), **dict(_DP_KW, max_grad_norm=max_grad_norm * 2))     # clips against the norm of the SUM
    real_moments, norms = ops.prodigy_moments, []
    ops.prodigy_moments = lambda *a, **k: real_moments(*a[:-1], a[-1] / 2, **k)
    for t in range(_DP_STEPS):
        for n, p in params.items():
            u = _DP_USED[n][t]
            p.grad = (sum((_dp_grad(n, r, p).float() if u[r] else torch.zeros(_SHAPES[n])) for r in range(2)).to(BF) if any(u) else None)
        norms.append(opt.step() / 2)
        opt.zero_grad()
    one = _dp_result(opt, norms)
    a, b = got[0], got[1]
    assert a["k"] == b["k"] == one["k"] == _DP_STEPS and a["d"] == b["d"] and a["d_max"] == b["d_max"] and a["d"] > _DP_KW["d0"]
    for key in ("p", "lo", "s", "p0"):
        assert (a[key] == b[key]).all(), f"ranks diverged on {key}"
    assert a["norms"] == b["norms"] and all(abs(x - y) <= 1e-6 * y for x, y in zip(a["norms"], one["norms"]))
    if not max_grad_norm:
        assert a["d"] == one["d"] and a["d_max"] == one["d_max"] and a["norms"] == one["norms"]
        for key in ("p", "lo", "s", "p0"):
            assert (a[key] == one[key]).all(), f"two ranks and one rank on the summed batch differ on {key}"
        return
    assert abs(a["d"] - one["d"]) <= 1e-5 * one["d"], (a["d"], one["d"])
    wa = adamw_ref.rebuild(torch.from_numpy(a["p"]).view(BF), torch.from_numpy(a["lo"]))
    w1 = adamw_ref.rebuild(torch.from_numpy(one["p"]).view(BF), torch.from_numpy(one["lo"]))
    moved = (w1 - torch.cat([torch.nn.functional.pad(p.detach().float().view(-1), (0, (-p.numel()) % 2048)) for p in _params().values()])).abs()
    assert float((wa - w1).abs().max()) <= 1e-4 * float(moved.max()), (float((wa - w1).abs().max()), float(moved.max()))
    assert (a["p0"] == one["p0"]).all()
