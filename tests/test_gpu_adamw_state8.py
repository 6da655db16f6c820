"""GPU: the opt-in block-scaled fp8 optimizer moments of the flat fused AdamW (``orv_adamw_flat_s8``, ``orv_state8_quantize``,
``orv_state8_dequantize``, ``FusedAdamW(state_precision="fp8")``) against their CPU restatement (tests/adamw_state8_ref.py).  The FORMAT
(block exponent, stochastic rounding, hash offsets, dequantisation) is held bit for bit wherever the fp32 values that enter it are known
exactly; with general hyper-parameters the fp32 ARITHMETIC of the two machines may differ by a step, so there the bytes are held on every
element whose code a float64 evaluation decides, and to the two grid neighbours on the rest.  The measured figures are printed;
profiles/adamw_state8.txt keeps those of the run the pull request was made with."""
import numpy as np
import pytest
import torch

import adamw_ref
import adamw_state8_ref as s8

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=1e-3)          # the reference's recipe (base_train.yaml:143-166)
SEG = 2048


def _dev():
    return torch.device("cuda:0")


def _specials():
    """fp32 values that exercise the format's edges: +-0, amax at 1.75 2^k and one step above, the carry out of the subnormal range,
    subnormal fp32, NaN and infinities."""
    nxt = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    return torch.tensor([0.0, -0.0, 1.0, 0.3, -0.3, 7.5 * 2.0 ** -17, 15.5 / 256, 1.75, nxt(1.75), -1.75 * 2.0 ** -20, 2.0 ** -130, -2.0 ** -140,
                         float("nan"), float("inf"), float("-inf"), 448.0, 57344.0, 3.0e38], dtype=torch.float32)


def _format_input(seed):
    """2^20 fp32 values over ~40 binades, the specials in front (one per block, so that each meets its own block exponent too) and in the
    last block, an all-zero block and a block without a finite element."""
    g = torch.Generator().manual_seed(seed)
    n = 1 << 20
    x = (torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 3.0)).float()
    sp = _specials()
    x[:len(sp)] = sp
    for j, val in enumerate(sp):
        x[(j + 1) * 256:(j + 2) * 256] *= 2.0 ** -12
        x[(j + 1) * 256 + 7] = val
    x[30 * 256:31 * 256] = 0.0
    x[31 * 256:32 * 256] = float("nan")
    x[32 * 256:33 * 256] *= 1e-42                                                     # a block of subnormals
    x[n - len(sp):] = sp
    return x


def _gpu_quantize(x, fmt, seed, step):
    from orv_amd import ops
    dev = _dev()
    q = torch.full((x.numel(),), 0xAA, dtype=torch.uint8, device=dev)
    ex = torch.full((x.numel() // 256,), 0xAA, dtype=torch.uint8, device=dev)
    ops.state8_quantize(x.to(dev), q, ex, fmt, seed=seed, step=step)
    torch.cuda.synchronize()
    return q.cpu(), ex.cpu()


def _gpu_dequantize(q, ex, fmt):
    from orv_amd import ops
    dev = _dev()
    x = torch.full((q.numel(),), 7.0, dtype=torch.float32, device=dev)
    ops.state8_dequantize(q.to(dev), ex.to(dev), x, fmt)
    torch.cuda.synchronize()
    return x.cpu()


def _same_f32(a, b):
    """bit for bit, any NaN equal to any NaN"""
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(((adamw_ref.f32_bits(a) == adamw_ref.f32_bits(b)) | nan).all())


# ---- 5. the format, bit for bit ----
@pytest.mark.parametrize("fmt", [0, 1])
def test_quantize_matches_the_restatement_bit_for_bit(fmt):
    for seed, step, data in ((0, 1, 0), (0xDEADBEEF, 300, 1), (7, 2 ** 31 - 1, 0)):
        x = _format_input(data)
        q, ex = _gpu_quantize(x, fmt, seed, step)
        wq, we = s8.quantize(x, fmt, seed=seed, step=step)
        assert torch.equal(ex, we), (seed, step, int((ex != we).sum()))
        assert torch.equal(q, wq), (seed, step, int((q != wq).sum()))
    other, _ = _gpu_quantize(x, fmt, 8, step)
    assert not torch.equal(other, q)


@pytest.mark.parametrize("fmt", [0, 1])
def test_dequantize_is_exact_and_requantising_returns_the_values(fmt):
    # every code in every position of a lane's 8 bytes, under scale bytes from 0 (subnormal results) to the largest the format writes
    codes = torch.arange(256, dtype=torch.uint8).repeat(8 + 247)[:256 * 255].contiguous()
    codes = torch.cat([codes, codes.flip(0)])
    if fmt == 1:
        codes = torch.where((codes & 0x7F >= 0x7C) & (codes & 0x7F <= 0x7E), torch.tensor(0x7F, dtype=torch.uint8), codes)     # never written
    top = 246 if fmt == 0 else 239                                                    # F 2^(top - 127) = 1.75 2^127: still finite
    ex = torch.cat([torch.arange(0, 255, dtype=torch.int64).clamp(max=top), torch.arange(0, 255, dtype=torch.int64).clamp(max=top)]).to(torch.uint8)
    got = _gpu_dequantize(codes, ex, fmt)
    assert _same_f32(got, s8.dequantize(codes, ex, fmt))
    # a quantised random buffer: dequantise on the GPU, quantise that again (other offsets), dequantise: the same values
    x = _format_input(2)
    q, e1 = _gpu_quantize(x, fmt, 3, 5)
    d = _gpu_dequantize(q, e1, fmt)
    assert _same_f32(d, s8.dequantize(q, e1, fmt))
    d0 = torch.where(torch.isnan(d), torch.zeros_like(d), d)
    for seed, step in ((3, 5), (11, 6)):
        q2, e2 = _gpu_quantize(d0, fmt, seed, step)
        assert _same_f32(_gpu_dequantize(q2, e2, fmt), d0)


# ---- the fused kernel ----
def _inputs(seed=0):
    """>= 2^20 elements in 4 segments (the third inactive), differing step counts, a clip scalar, weights N(0, 0.02), random low halves (the
    layout of tests/test_gpu_adamw_precision.py); the incoming moments are fp32 values spread over many binades, quantised by the
    restatement as an earlier step would have left them."""
    g = torch.Generator().manual_seed(seed)
    sizes = [300 * SEG, 150 * SEG, 40 * SEG, 60 * SEG]
    n = sum(sizes)
    assert n >= 2 ** 20
    p = (torch.randn(n, generator=g) * 0.02).to(BF)
    lo = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int64).to(torch.int16)
    grad = (torch.randn(n, generator=g) * 0.05).to(BF)
    m = torch.randn(n, generator=g) * 0.01 * torch.exp(torch.randn(n, generator=g))
    v = (torch.randn(n, generator=g) * 0.01 * torch.exp(torch.randn(n, generator=g))) ** 2
    m[5 * 256:6 * 256] = 0.0                                                          # a never-written block (scale byte 0) ...
    v[5 * 256:6 * 256] = 0.0
    m8, m_exp = s8.quantize(m, 0, seed=seed, step=299)
    v8, v_exp = s8.quantize(v, 1, seed=seed, step=299)
    starts = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64)
    active = torch.tensor([1, 1, 0, 1], dtype=torch.uint8)
    seg_step = torch.tensor([1, 7, 50, 300], dtype=torch.int32)
    return dict(p=p, lo=lo, g=grad, m8=m8, v8=v8, m_exp=m_exp, v_exp=v_exp, seg_start=starts, active=active, seg_step=seg_step, clip=0.37,
                step=300, n=n)


def _launch(inp, mode, seed=0, lo=None, clip=True, **over):
    """-> dict of the six buffers on the CPU after one ops.adamw_flat_s8 launch on the GPU."""
    from orv_amd import ops
    dev = _dev()
    h = dict(HYPER, **over)
    t = {k: inp[k].to(dev).clone() for k in ("p", "g", "m8", "v8", "m_exp", "v_exp")}
    lo_d = None if lo is None else lo.to(dev).clone()
    clip_d = torch.tensor([inp["clip"]], dtype=torch.float32, device=dev) if clip else None
    seg_step = None if inp["seg_step"] is None else inp["seg_step"].to(dev)
    ops.adamw_flat_s8(t["p"], t["g"], t["m8"], t["v8"], t["m_exp"], t["v_exp"], inp["seg_start"].to(dev), inp["active"].to(dev), h["lr"],
                      h["beta1"], h["beta2"], h["eps"], h["weight_decay"], inp["step"], clip_d, seg_step=seg_step, lo=lo_d, mode=mode, seed=seed)
    torch.cuda.synchronize()
    out = {k: t[k].cpu() for k in ("p", "m8", "v8", "m_exp", "v_exp")}
    out["lo"] = None if lo_d is None else lo_d.cpu()
    return out


def _active_mask(inp):
    return s8.active_mask(inp["n"], inp["seg_start"], inp["active"])


def _assert_inactive_untouched(inp, out, lo_in):
    act = _active_mask(inp)
    inact, inact_b = ~act, ~act[::256]
    assert int(inact.sum()) > 0
    assert torch.equal(adamw_ref.bf16_bits(out["p"])[inact], adamw_ref.bf16_bits(inp["p"])[inact])
    if lo_in is not None:
        assert torch.equal(out["lo"][inact], lo_in[inact])
    for k in ("m8", "v8"):
        assert torch.equal(out[k][inact], inp[k][inact]), k
    for k in ("m_exp", "v_exp"):
        assert torch.equal(out[k][inact_b], inp[k][inact_b]), k


def test_fused_kernel_stores_the_restatements_bytes_where_the_arithmetic_is_exact():
    """beta1 = beta2 = 0 and no clip: m = g and v = g^2 exactly (the operands are bf16), so the stored element and scale bytes must be the
    restatement's for (g, g^2) at (seed, step, flat index) on every active element, in every weight mode."""
    inp = _inputs()
    act = _active_mask(inp)
    # non-finite gradients make non-finite moments: stored as 0x7F, left out of their block's maximum (first and last segment)
    for at in (3, 4 * 256 + 9, inp["n"] - 700):
        inp["g"][at:at + 3] = torch.tensor([float("inf"), float("-inf"), float("nan")]).to(BF)
    g32 = inp["g"].float()
    for mode, seed in ((1, 0), (2, 0xC0FFEE), (0, 5)):
        lo_in = inp["lo"] if mode == 1 else None
        out = _launch(inp, mode, seed=seed, lo=lo_in, clip=False, beta1=0.0, beta2=0.0)
        for x, q, e, fmt in ((g32, "m8", "m_exp", 0), (g32 * g32, "v8", "v_exp", 1)):
            wq, we = s8.quantize(x, fmt, seed=seed, step=inp["step"])
            assert torch.equal(out[e][act[::256]], we[act[::256]]), (mode, e)
            assert torch.equal(out[q][act], wq[act]), (mode, q, int((out[q][act] != wq[act]).sum()))
            assert out[q][3:6].tolist() == [0x7F] * 3 and int(out[e][0]) > 0
        _assert_inactive_untouched(inp, out, lo_in)
        assert not torch.equal(adamw_ref.bf16_bits(out["p"])[act], adamw_ref.bf16_bits(inp["p"])[act])


def _grid_floor_ceil(z, fmt):
    """Signed floor and ceiling of the float64 values z on the element grid of ``fmt`` (unit scale)."""
    f = s8.FORMATS[fmt]
    a = np.abs(z)
    _, ae = np.frexp(a)
    E = np.maximum(np.where(a > 0, ae - 1, f["Emin"]), f["Emin"])
    s = np.ldexp(1.0, E - f["M"])
    dn, up = np.floor(a / s) * s, np.ceil(a / s) * s
    return np.where(z >= 0, dn, -up), np.where(z >= 0, up, -dn)


def test_fused_kernel_with_the_references_recipe():
    """General hyper-parameters.  The moments are evaluated in float64 from the dequantised old state.  An element is DECIDABLE when moving
    the float64 value by +-1e-6 of its error scale (|b1 m_old| + |(1 - b1) g clip| for m, v itself for v - the scales of
    tests/test_gpu_adamw_precision.py) changes neither its code nor its block's exponent: there the GPU's bytes must be the restatement's.
    At most 1e-3 of the active elements per moment may be left out (the restatement alone leaves out 7.4e-5 / 1.1e-5 on inputs of this kind).
    Every element, decidable or not, must dequantise to a value between the grid neighbours of the float64 value widened by that allowance,
    under a block exponent one of the perturbed evaluations gives.  Weights (mode 1): against a float64 evaluation of the formula with the
    floor, unit and yardstick of test_split_arithmetic_against_float64_with_the_cpu_fp32_error_as_yardstick, bound 2 x the CPU fp32 error.
    Mode 2: bit for bit the stochastic rounding of mode 1's master with lo = 0; mode 0: its nearest-even bf16."""
    inp = _inputs(1)
    seed, step, n = 21, inp["step"], inp["n"]
    act = _active_mask(inp)
    actn, actb = act.numpy(), act[::256].numpy()
    m_old, v_old = s8.dequantize(inp["m8"], inp["m_exp"], 0), s8.dequantize(inp["v8"], inp["v_exp"], 1)
    vfloor = s8.v_floor(inp["v_exp"])
    w_old = adamw_ref.rebuild(inp["p"], inp["lo"])
    args = (inp["seg_start"], inp["active"], inp["seg_step"], inp["clip"], HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"],
            HYPER["weight_decay"], step)
    w64, m64, v64 = s8.flat_update(w_old, inp["g"].float(), m_old, v_old, vfloor, *args, torch.float64)
    w32, m32, v32 = s8.flat_update(w_old, inp["g"].float(), m_old, v_old, vfloor.float(), *args, torch.float32)
    out = _launch(inp, 1, seed=seed, lo=inp["lo"])
    _assert_inactive_untouched(inp, out, inp["lo"])
    b1 = float(torch.tensor(HYPER["beta1"], dtype=torch.float32))
    clip = float(torch.tensor(inp["clip"], dtype=torch.float32))
    m_scale = (b1 * m_old.double()).abs() + ((1 - b1) * inp["g"].double() * clip).abs()
    lines = []
    for name, fmt, x64, x32, scale, q, e in (("m", 0, m64, m32, m_scale, "m8", "m_exp"), ("v", 1, v64, v32, v64.abs(), "v8", "v_exp")):
        d = 1e-6 * scale
        trio = [s8.quantize(z, fmt, seed=seed, step=step, dtype=np.float64) for z in (x64 - d, x64, x64 + d)]
        codes = [t[0].numpy() for t in trio]
        exps = [t[1].numpy().astype(np.int64) for t in trio]
        exp_ok = (exps[0] == exps[1]) & (exps[2] == exps[1])
        decidable = (codes[0] == codes[1]) & (codes[2] == codes[1]) & np.repeat(exp_ok, 256) & actn
        left_out = 1 - decidable.sum() / actn.sum()
        cpu_q, _ = s8.quantize(x32, fmt, seed=seed, step=step)
        cpu_agrees = bool((cpu_q.numpy() == codes[1])[decidable].all())
        gq, ge = out[q].numpy(), out[e].numpy().astype(np.int64)
        bad = int((gq != codes[1])[decidable].sum())
        lines.append(f"{name}: left out {left_out:.2e} of the active elements (bound 1e-3), undecidable block exponents "
                     f"{int((~exp_ok & actb).sum())}, GPU bytes differing on decidable elements {bad}, CPU fp32 agrees on all decidable: {cpu_agrees}")
        print("\nadamw fp8 state, " + lines[-1])
        assert left_out <= 1e-3
        assert bad == 0
        assert bool(((ge == exps[1]) | ~exp_ok)[actb].all())
        assert bool(((ge >= np.minimum(exps[0], exps[2])) & (ge <= np.maximum(exps[0], exps[2])))[actb].all())
        # every element: between the grid neighbours of the float64 value, widened, on the GPU's own block grid
        ee = np.repeat(ge - 127, 256)
        val = s8.code_values(gq, fmt)
        lo_b, _ = _grid_floor_ceil(np.ldexp((x64 - d).numpy(), -ee), fmt)
        _, hi_b = _grid_floor_ceil(np.ldexp((x64 + d).numpy(), -ee), fmt)
        inside = (val >= lo_b) & (val <= hi_b)
        assert bool(inside[actn].all()), (name, int((~inside & actn).sum()))
    # weights
    w_gpu = adamw_ref.rebuild(out["p"], out["lo"])
    ok = act & torch.isfinite(w64)
    unit = adamw_ref.fp32_ulp(torch.maximum(torch.maximum(w_old.double().abs(), w64.abs()), (w64 - w_old.double()).abs()))
    yard = float(((w32.double() - w64).abs() / unit)[ok].max())
    got = float(((w_gpu.double() - w64).abs() / unit)[ok].max())
    print(f"adamw fp8 state, split_fp32 weights: worst error vs float64 in fp32 steps - CPU fp32 (yardstick) {yard:.3f}, GPU {got:.3f} (bound {2 * yard:.3f})")
    assert got <= 2 * yard, (got, yard)
    # modes 2 and 0 from mode 1's master with lo = 0
    zero = torch.zeros_like(inp["lo"])
    o1 = _launch(inp, 1, seed=seed, lo=zero)
    master = adamw_ref.rebuild(o1["p"], o1["lo"])
    o2 = _launch(inp, 2, seed=seed)
    want2 = adamw_ref.stochastic_round(master, adamw_ref.sr_offsets(seed, step, np.arange(n)))
    assert torch.equal(adamw_ref.bf16_bits(o2["p"])[act], adamw_ref.bf16_bits(want2)[act])
    o0 = _launch(inp, 0, seed=seed)
    assert torch.equal(adamw_ref.bf16_bits(o0["p"])[act], adamw_ref.bf16_bits(master.to(BF))[act])
    for o in (o1, o2, o0):                                                            # the state does not depend on the weight mode
        assert all(torch.equal(o[k], out[k]) for k in ("m8", "v8", "m_exp", "v_exp"))
        _assert_inactive_untouched(inp, o, zero if o is o1 else None)


# ---- 8. the floor ----
def test_second_moment_floor_bounds_the_step_where_v_flushed_to_zero():
    """A block whose incoming v code is 0 for all but one element, with non-zero m, zero gradient, no decay, weight 0: v stays 0 and
    m = b1 m_old, so the master moves by exactly lr |b1 m_old ibc1| / (sqrt(vfloor ibc2) + eps), vfloor = 2^(e_v_old - 16).  With the scale
    byte forced to 0 (vfloor = 2^-143) the same elements show the unfloored step: the test can see the floor."""
    n, step = SEG, 10
    g = torch.Generator().manual_seed(4)
    m8, m_exp = s8.quantize(torch.randn(n, generator=g) * 0.01, 0, seed=1, step=step - 1)
    v = torch.zeros(n)
    v[::256] = 1.0
    v8, v_exp = s8.quantize(v, 1, seed=1, step=step - 1)
    assert set(v_exp.tolist()) == {112} and int((v8 == 0).sum()) == n - n // 256
    m_old = s8.dequantize(m8, m_exp, 0).double()
    sel = (v8 == 0) & (m_old != 0)
    assert int(sel.sum()) > n // 2
    inp = dict(p=torch.zeros(n, dtype=BF), g=torch.zeros(n, dtype=BF), m8=m8, v8=v8, m_exp=m_exp, v_exp=v_exp,
               seg_start=torch.tensor([0, n], dtype=torch.int64), active=torch.ones(1, dtype=torch.uint8), seg_step=None, clip=1.0, step=step, n=n)
    f = lambda x: torch.tensor(float(x), dtype=torch.float32).double()
    lr, b1, b2, eps = f(HYPER["lr"]), f(HYPER["beta1"]), f(HYPER["beta2"]), f(HYPER["eps"])
    ibc1, ibc2 = 1 / (1 - b1 ** step), 1 / (1 - b2 ** step)
    steps = {}
    for name, exps, vfloor in (("floored", v_exp, 2.0 ** (112 - 127 - 16)), ("unfloored", torch.zeros_like(v_exp), 2.0 ** -143)):
        out = _launch(dict(inp, v_exp=exps), 1, lo=torch.zeros(n, dtype=torch.int16), clip=False, weight_decay=0.0)
        moved = adamw_ref.rebuild(out["p"], out["lo"]).double()
        want = -(lr * (b1 * m_old * ibc1)) / (torch.sqrt(torch.tensor(vfloor, dtype=torch.float64) * ibc2) + eps)
        rel = float(((moved - want).abs() / want.abs())[sel].max())
        steps[name] = float(moved.abs()[sel].max() / lr)
        print(f"\nadamw fp8 state, {name} step: worst relative error {rel:.3e} (bound 1e-5), largest step {steps[name]:.4g} lr")
        assert rel <= 1e-5
    assert steps["unfloored"] > 1e3 * steps["floored"]


# ---- 9. optimizer level ----
class _Standins:
    """The restatement in place of orv_amd.ops for a CPU run of FusedAdamW (context manager)."""
    NAMES = ("sumsq", "adamw_flat_s8", "state8_quantize", "state8_dequantize")

    def __enter__(self):
        from orv_amd import ops
        self.saved = {k: getattr(ops, k) for k in self.NAMES}
        ops.sumsq = lambda g, out: out.add_(g.float().pow(2).sum())
        ops.adamw_flat_s8, ops.state8_quantize, ops.state8_dequantize = s8.adamw_flat_s8, s8.state8_quantize, s8.state8_dequantize

    def __exit__(self, *a):
        from orv_amd import ops
        for k, fn in self.saved.items():
            setattr(ops, k, fn)


def test_hundred_steps_land_where_the_restatement_lands():
    """One parameter at 1.0, constant unit gradient, lr 1e-3, no decay, no clipping, 100 steps with fp8 moments under split_fp32: the
    master must land where the restatement's CPU run of the same optimizer lands, to 1e-6 relative."""
    from orv_amd.optim import FusedAdamW

    def run(dev):
        p = torch.nn.Parameter(torch.ones(2 ** 16, device=dev, dtype=BF))
        opt = FusedAdamW([p], lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, param_precision="split_fp32",
                         state_precision="fp8", seed=6)
        g = torch.ones(2 ** 16, device=dev, dtype=BF)
        for _ in range(100):
            p.grad = g
            opt.step()
        return opt.master_params()[0].cpu().double(), [x[0].cpu() for x in opt.moments()]

    gpu, gm = run(_dev())
    torch.cuda.synchronize()
    with _Standins():
        cpu, cm = run(torch.device("cpu"))
    rel = float(((gpu - cpu).abs() / cpu.abs()).max())
    same = [float((a == b).double().mean()) for a, b in zip(gm, cm)]
    print(f"\nadamw fp8 state, 100 steps of 1e-3 from 1.0: master mean {float(gpu.mean()):.6f} (fp32 moments: 0.9), worst relative distance from the "
          f"restatement's run {rel:.3e} (bound 1e-6); moments equal on {same[0]:.6f} / {same[1]:.6f} of the elements")
    assert rel <= 1e-6


def _distance(a, b, init):
    """mean |a - b| over all elements of all parameters, in units of the mean parameter movement |b - init|."""
    num = sum(float((x.double() - y.double()).abs().sum()) for x, y in zip(a, b))
    den = sum(float((y.double() - z.double()).abs().sum()) for y, z in zip(b, init))
    return num / den


def test_twenty_steps_against_torch_adamw_stay_as_close_as_the_restatement():
    """The parameter set of test_split_fp32_follows_torch_adamw_in_fp32_and_the_default_does_not, 20 steps.  The distance of the fp8-state
    split masters from torch.optim.AdamW in fp32 (units of the mean parameter movement) is measured against the same figure of the CPU
    restatement run with the same seed: the trajectories differ only where fp32 rounding flips a code, so the GPU may show 1.25 x it."""
    from orv_amd.cogvideox_control import Attention
    from orv_amd.optim import FusedAdamW
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
    ref = [x.float().clone().requires_grad_(True) for x in init]
    topt = torch.optim.AdamW(ref, **kw)
    for it in range(steps):
        for r, g in zip(ref, grads[it]):
            r.grad = None if g is None else g.float()
        torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], 1.0)
        topt.step()
    t32 = [r.detach() for r in ref]

    def fused_run(dev, state):
        params = [torch.nn.Parameter(x.to(dev).clone()) for x in init]
        opt = FusedAdamW(params, max_grad_norm=1.0, param_precision="split_fp32", state_precision=state, seed=13, **kw)
        for it in range(steps):
            for p, g in zip(params, grads[it]):
                p.grad = None if g is None else g.to(dev)
            opt.step()
            opt.zero_grad()
        by_param = {id(p): mp_.cpu() for p, mp_ in zip(opt.params, opt.master_params())}
        return [by_param[id(p)] for p in params]

    d_gpu = _distance(fused_run(_dev(), "fp8"), t32, init)
    d_fp32 = _distance(fused_run(_dev(), "fp32"), t32, init)
    torch.cuda.synchronize()
    with _Standins():
        d_cpu = _distance(fused_run(torch.device("cpu"), "fp8"), t32, init)
    print(f"\nadamw fp8 state, 20 steps vs torch.optim.AdamW fp32, in units of the mean parameter movement: GPU {d_gpu:.4e}, CPU restatement "
          f"{d_cpu:.4e} (bound {1.25 * d_cpu:.4e}), fp32 state on the GPU {d_fp32:.3e}")
    assert d_gpu <= 1.25 * d_cpu, (d_gpu, d_cpu)


# ---- 10. model level ----
def test_fp8_state_in_the_model_three_sft_steps():
    """Three sft_step calls on the small golden-config model with state_precision="fp8": finite losses; after each step the stored
    moments are a fixed point of dequantise -> quantise; moments() finite; the state_dict saved after step 2, loaded into a fresh
    optimizer over copies of the step-2 weights and fed the gradients of step 3, reproduces step 3's weights bit for bit.
    (A block whose largest element was rounded down to exactly F 2^(e-1) requantises under e - 1 to other bytes with the same values;
    such blocks are held on their values, every other block on its bytes.)"""
    from conftest import load_golden
    from orv_amd import ops, schedulers, sft
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
    # no clipping: the clip coefficient comes from a sum of squares whose cross-workgroup order is not fixed, and the resume check below
    # is bit for bit
    kw = dict(lr=2e-4, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=0.0, state_precision="fp8")
    opt = FusedAdamW(m.parameters(), seed=17, **kw)
    saved = None
    for step in range(3):
        if step == 2:
            saved = ({k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}, [p.detach().clone() for p in opt.params])
        loss, parts = sft.sft_step(m, sched, opt, batch, generator=torch.Generator(device=dev).manual_seed(100 + step))
        assert torch.isfinite(loss) and parts["grad_norm"] > 0
        f = opt._flat
        for q, e, fmt in ((f["m8"], f["m_exp"], "m"), (f["v8"], f["v_exp"], "v")):
            d = torch.empty(q.numel(), dtype=torch.float32, device=dev)
            ops.state8_dequantize(q, e, d, fmt)
            assert bool(torch.isfinite(d).all()) and float(d.abs().max()) > 0
            q2, e2, d2 = torch.empty_like(q), torch.empty_like(e), torch.empty_like(d)
            ops.state8_quantize(d, q2, e2, fmt, seed=opt.seed + 1, step=step + 5)
            ops.state8_dequantize(q2, e2, d2, fmt)
            assert torch.equal(d2, d)
            same_exp = e2 == e
            assert bool(((e2.int() == e.int() - 1) | same_exp).all())
            assert torch.equal(q2.view(-1, 256)[same_exp], q.view(-1, 256)[same_exp])
            assert float(same_exp.float().mean()) > 0.5
        mom = opt.moments()
        assert all(bool(torch.isfinite(t).all()) for t in mom[0] + mom[1]) and all(t.shape == p.shape for t, p in zip(mom[0], opt.params))
    torch.cuda.synchronize()
    sd, weights2 = saved
    assert sd["state_precision"] == "fp8" and sd["step"] == 2
    has_grad = [bool(a) for a in opt._flat["active"].tolist()]
    grads3 = [v.clone() for v in opt._flat["views_g"]]                               # the flat buffer still holds step 3's gradients
    params2 = [torch.nn.Parameter(x.clone()) for x in weights2]
    opt2 = FusedAdamW(params2, **kw)
    opt2.load_state_dict(sd)
    assert opt2.seed == 17 and opt2.step_count == 2
    for p, g, h in zip(params2, grads3, has_grad):
        p.grad = g if h else None
    opt2.step()
    torch.cuda.synchronize()
    for a, b in zip(opt.params, params2):
        assert torch.equal(adamw_ref.bf16_bits(a.detach()), adamw_ref.bf16_bits(b.detach()))
    assert all(torch.equal(opt._flat[k], opt2._flat[k]) for k in ("m8", "v8", "m_exp", "v_exp"))
    assert sum(int((a.detach() != b).sum()) for a, b in zip(opt.params, weights2)) > 0
