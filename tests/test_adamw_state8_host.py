"""CPU: the opt-in block-scaled fp8 optimizer moments of FusedAdamW (``state_precision="fp8"``).

The format is checked on its Python restatement (tests/adamw_state8_ref.py) against answers derived by hand from the rule, its statistics
on the same restatement, the C ABI symbols on the built library, and the optimizer's host logic (argument, buffers, dispatch, checkpoints
across precisions) with the kernels replaced by the restatement - test infrastructure in the style of tests/test_adamw_precision_host.py."""
import os
import re

import numpy as np
import pytest
import torch

import adamw_ref
import adamw_state8_ref as s8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
F32 = np.float32


def _block(values, fill=0.0):
    x = np.full(256, fill, dtype=F32)
    x[:len(values)] = np.asarray(values, dtype=F32)
    return x


# ---- 1. known answers ----
def test_e4m3_block_with_amax_one():
    """amax = 1: 448 2^-8 = 1.75 >= 1 > 448 2^-9, so e = -8 and y = 256 x.  1.0 -> y = 2^8: E = 8, s = 32, w = 8 * 65536, n = 8 for every r,
    magnitude 256.  fp32(0.3) -> y = 76.8: E = 6, s = 8, a / s = 9.6, w = 629145 = 9 * 65536 + 39321, so n = 10 (80, value 0.3125) iff
    r >= 65536 - 39321 = 26215, else n = 9 (72, value 0.28125)."""
    x = _block([1.0, 0.3, -0.3])
    for r in (0, 26214, 26215, 65535):
        q, ex = s8.quantize(x, 0, r=r)
        assert ex.tolist() == [119]                                              # e + 127 = -8 + 127
        vals = s8.code_values(q, 0)
        assert vals[0] == 256.0 and int(q[0]) == 0x78                            # exponent field 8 + 7, mantissa 0
        assert vals[1] == (80.0 if r >= 26215 else 72.0) and vals[2] == -vals[1]
        d = s8.dequantize(q, ex, 0)
        assert float(d[0]) == 1.0 and float(d[1]) == (0.3125 if r >= 26215 else 0.28125)
        assert int(q[3]) == 0                                                    # a = 0: code 0


def test_carries_are_the_next_code():
    """In the amax = 1 e4m3 block (y = 256 x): y = 7.5 2^-9 lies between the largest subnormal 7 2^-9 (code 7) and the smallest normal
    2^-6 (code 8): w = 7.5 * 65536, n = 8 iff r >= 32768.  y = 15.5 (E = 3, s = 1) goes to 15 (code 0x57) or, carried into the next
    binade, 16 (code 0x58) iff r >= 32768."""
    x = _block([1.0, 7.5 * 2.0 ** -9 / 256, 15.5 / 256])
    lo, _ = s8.quantize(x, 0, r=32767)
    hi, ex = s8.quantize(x, 0, r=32768)
    assert lo[1:3].tolist() == [7, 0x57] and hi[1:3].tolist() == [8, 0x58]
    assert s8.dequantize(hi, ex, 0)[1:3].tolist() == [2.0 ** -14, 16.0 / 256]
    # e5m2, amax = 1 -> e = -15 (57344 2^-15 = 1.75), y = 32768 x: 3.5 2^-16 between codes 3 (largest subnormal) and 4 (2^-14)
    x = _block([1.0, 3.5 * 2.0 ** -16 / 32768])
    lo, ex = s8.quantize(x, 1, r=32767)
    hi, _ = s8.quantize(x, 1, r=32768)
    assert ex.tolist() == [112] and int(lo[1]) == 3 and int(hi[1]) == 4 and int(lo[0]) == 0x78      # 2^15: field 15 + 15 = 30, 30 << 2


def test_block_exponent_edges():
    nxt = lambda v: np.nextafter(F32(v), F32(np.inf))
    # amax exactly 1.75 2^k fills the block range; one fp32 step above needs the next exponent
    for k in (-20, 0, 9):
        a = F32(1.75 * 2.0 ** k)
        assert s8.block_exponents(_block([a]), 0).tolist() == [k - 8] and s8.block_exponents(_block([nxt(a)]), 0).tolist() == [k - 7]
        assert s8.block_exponents(_block([a]), 1).tolist() == [k - 15] and s8.block_exponents(_block([nxt(a)]), 1).tolist() == [k - 14]
    # the largest finite fp32 bounds e: 120 for e4m3, 113 for e5m2
    big = np.finfo(F32).max
    assert s8.block_exponents(_block([big]), 0).tolist() == [120] and s8.block_exponents(_block([big]), 1).tolist() == [113]
    # the bit formula of the format on random magnitudes: e = ef - 135 (142) + (mant > 0x600000), clamped at -127
    g = torch.Generator().manual_seed(1)
    amax = (torch.randn(4096, generator=g).abs() * torch.exp(torch.randn(4096, generator=g) * 30)).clamp(1e-44, 3e38)
    x = np.zeros((4096, 256), dtype=F32)
    x[:, 5] = amax.numpy()
    u = adamw_ref.f32_bits(torch.from_numpy(x[:, 5].copy()))
    ef, mant = (u >> 23).numpy(), (u & 0x7FFFFF).numpy()
    for fmt, adj in ((0, 135), (1, 142)):
        want = np.where(ef == 0, -127, np.maximum(ef - adj + (mant > 0x600000), -127))
        assert np.array_equal(s8.block_exponents(x, fmt), want)


def test_zero_subnormal_and_nonfinite_blocks():
    for fmt in (0, 1):
        q, ex = s8.quantize(_block([0.0, -0.0]), fmt, r=65535)
        assert ex.tolist() == [0] and q[:3].tolist() == [0, 0x80, 0]                               # the sign is kept
        # a subnormal amax clamps to e = -127: y = x 2^127
        tiny = F32(2.0 ** -130)
        q, ex = s8.quantize(_block([tiny, -tiny]), fmt, r=0)
        assert ex.tolist() == [0]
        assert s8.code_values(q, fmt)[:2].tolist() == [0.125, -0.125] and s8.dequantize(q, ex, fmt)[:2].tolist() == [float(tiny), -float(tiny)]
        # non-finite elements store 0x7F (no sign) and do not enter amax
        q, ex = s8.quantize(_block([np.nan, np.inf, -np.inf, 1.0, -np.nan]), fmt, r=123)
        assert q[:5].tolist() == [0x7F, 0x7F, 0x7F, 0x78, 0x7F] and ex.tolist() == [119 if fmt == 0 else 112]
        d = s8.dequantize(q, ex, fmt)
        assert bool(torch.isnan(d[:3]).all()) and float(d[3]) == 1.0
        q, ex = s8.quantize(_block([np.nan], fill=np.inf), fmt, r=0)                              # nothing finite: byte 0
        assert ex.tolist() == [0] and set(q.tolist()) == {0x7F}


def _spread(n, seed, sigma=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * sigma)).float()


@pytest.mark.parametrize("fmt", [0, 1])
def test_stored_values_stay_within_range_and_on_the_torch_float8_grid(fmt):
    f = s8.FORMATS[fmt]
    x = _spread(1 << 20, 3)
    dt = torch.float8_e4m3fn if fmt == 0 else torch.float8_e5m2
    for r in (0, 65535, None):
        q, ex = s8.quantize(x, fmt, seed=5, step=2, r=r)
        vals = s8.code_values(q, fmt)
        assert float(np.abs(vals).max()) <= f["F"]                                                 # n s <= F, also with the largest offset
        if fmt == 1:
            assert int((q & 0x7F).max()) <= 0x7B                                                   # 0x7C..0x7E never written
        t = torch.from_numpy(vals).float()
        assert torch.equal(t.to(dt).float(), t)                                                    # every stored value is on torch's grid
        assert torch.equal(q.view(dt).float(), t)                                                  # ... and the bytes are torch's encoding
        # the stored value is one of the two grid neighbours of y
        e = np.repeat(ex.numpy().astype(np.int64) - 127, 256)
        y = np.ldexp(x.numpy().astype(np.float64), -e)
        fl, _ = s8.quantize(x, fmt, r=0)
        lo = np.abs(s8.code_values(fl, fmt))
        step = s8.grid_step(fl, torch.full_like(ex, 127), fmt)
        assert bool(((lo <= np.abs(y)) & (np.abs(y) < lo + step)).all())
        assert bool(((np.abs(vals) == lo) | (np.abs(vals) == lo + step)).all())


def test_hash_stream_known_answers():
    """The two offset streams, hand-run with Python integers from the definition."""
    def mix(x):
        x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF; x ^= x >> 16
        return x
    for seed, step, i in [(0, 1, 0), (7, 3, 12345), (0xFFFFFFFF, 100, 2 ** 32 + 5), (11, 2, 3 * 2 ** 32 + 2 ** 31 + 77)]:
        key2 = mix(((i >> 32) + mix((step + mix(seed ^ 0x9E3779B9)) & 0xFFFFFFFF)) & 0xFFFFFFFF)
        h = mix((i & 0xFFFFFFFF) ^ key2)
        rm, rv = s8.state_offsets(seed, step, [i])
        assert (int(rm[0]), int(rv[0])) == (h >> 16, h & 0xFFFF)
    # fully worked: seed 0x9E3779B9 makes the innermost argument 0, and mix(0) = 0
    assert mix(0) == 0
    key2 = mix(mix(1))
    rm, rv = s8.state_offsets(0x9E3779B9, 1, [0])
    assert (int(rm[0]) << 16) | int(rv[0]) == mix(key2)
    # independent of the weight mode's stream, uniform
    idx = np.arange(1 << 20)
    rm, rv = s8.state_offsets(3, 9, idx)
    rw = adamw_ref.sr_offsets(3, 9, idx).numpy()
    for a in (rm, rv):
        assert abs(float(a.mean()) - 32767.5) < 6 * 18918 / 1024
    for a, b in ((rm, rv), (rm, rw), (rv, rw)):
        assert abs(float(np.corrcoef(a, b)[0, 1])) < 5 / 1024                                       # 5 standard deviations of 2^-10


# ---- 2. statistics ----
@pytest.mark.parametrize("fmt", [0, 1])
def test_rounding_is_unbiased(fmt):
    """mean((dq - x) / s) over N = 2^20: each term is a centred Bernoulli (variance <= 1/4), so 2.5 / sqrt(N) is five standard deviations."""
    n = 1 << 20
    x = _spread(n, 11 + fmt, sigma=1.0)
    q, ex = s8.quantize(x, fmt, seed=17, step=4)
    fl, _ = s8.quantize(x, fmt, r=0)
    step = s8.grid_step(fl, ex, fmt)                                                               # the step of the cell x lies in
    err = (s8.dequantize(q, ex, fmt).numpy().astype(np.float64) - x.numpy().astype(np.float64)) / step
    assert float(np.abs(err).max()) < 1.0
    print(f"fmt {fmt}: mean error {err.mean():+.3e} grid steps, bound {2.5 / np.sqrt(n):.3e}")
    assert abs(float(err.mean())) <= 2.5 / np.sqrt(n)


@pytest.mark.parametrize("fmt", [0, 1])
def test_quantising_dequantised_values_returns_them(fmt):
    x = torch.cat([_spread(1 << 16, 21), torch.zeros(256), _spread(256, 22) * 1e-42])
    q, ex = s8.quantize(x, fmt, seed=1, step=1)
    d = s8.dequantize(q, ex, fmt)
    for kw in (dict(r=0), dict(r=65535), dict(seed=2, step=9)):
        q2, ex2 = s8.quantize(d, fmt, **kw)
        assert torch.equal(s8.dequantize(q2, ex2, fmt), d)


def test_zero_gradient_decay_needs_the_stochastic_rule():
    """v <- 0.95 v for 200 steps in e5m2.  A 5 % decay is below half a grid step (12.5 ... 25 % of the value), so rounding to nearest
    (r = 32768) returns the old code every time; the stochastic rule follows 0.95^200 = 3.5e-5 in the mean."""
    g = torch.Generator().manual_seed(5)
    v0 = (1e-3 * (1 + torch.rand(1 << 16, generator=g))).float()
    v0[::256] = 1.0                                                                                 # the element that sets each block's scale
    small = torch.ones(1 << 16, dtype=torch.bool)
    small[::256] = False
    want = 0.95 ** 200
    out = {}
    for name in ("stochastic", "nearest"):
        q, ex = s8.quantize(v0, 1, seed=3, step=0, r=None if name == "stochastic" else 32768)
        start = s8.dequantize(q, ex, 1).double()[small].mean()
        for step in range(1, 201):
            v = s8.dequantize(q, ex, 1) * torch.tensor(0.95, dtype=torch.float32)
            q, ex = s8.quantize(v, 1, seed=3, step=step, r=None if name == "stochastic" else 32768)
        out[name] = float(s8.dequantize(q, ex, 1).double()[small].mean() / start)
    print(f"after 200 steps: stochastic {out['stochastic']:.3e}, nearest {out['nearest']:.3e}, exact {want:.3e}")
    assert want / 2 <= out["stochastic"] <= want * 2
    assert out["nearest"] > 0.5


# ---- 3. host behaviour of FusedAdamW on stand-in kernels ----
@pytest.fixture
def standins():
    from orv_amd import ops
    names = ("sumsq", "adamw_flat", "adamw_flat_ex", "adamw_flat_s8", "state8_quantize", "state8_dequantize")
    saved = {n: getattr(ops, n, None) for n in names}
    calls = []

    def sumsq(g, out):
        out.add_(g.float().pow(2).sum())

    def adamw_flat(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None, seg_step=None):
        calls.append("adamw_flat")
        adamw_ref.adamw_flat_ex(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef, seg_step)

    def wrap(name, fn):
        def f(*a, **k):
            calls.append(name)
            fn(*a, **k)
        return f

    ops.sumsq, ops.adamw_flat = sumsq, adamw_flat
    ops.adamw_flat_ex = wrap("adamw_flat_ex", adamw_ref.adamw_flat_ex)
    ops.adamw_flat_s8 = wrap("adamw_flat_s8", s8.adamw_flat_s8)
    ops.state8_quantize = wrap("state8_quantize", s8.state8_quantize)
    ops.state8_dequantize = wrap("state8_dequantize", s8.state8_dequantize)
    yield calls
    for n, f in saved.items():
        if f is None:
            delattr(ops, n)
        else:
            setattr(ops, n, f)


_SHAPES = {"A": (64, 40), "B": (3000,), "C": (17, 9)}
_TOTAL = 4096 + 4096 + 2048


def _params(seed=7):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(BF)) for n, s in _SHAPES.items()}


def _feed(params, step, skip=()):
    for n, p in params.items():
        g = torch.Generator().manual_seed(100 * step + sum(map(ord, n)))
        p.grad = None if n in skip else (torch.randn(p.shape, generator=g) * 0.1).to(BF)


def _opt(params, **kw):
    from orv_amd.optim import FusedAdamW
    return FusedAdamW(params.values(), lr=2e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-3, max_grad_norm=1.0, **kw)


def _run(opt, params, steps, skip_at=None):
    for step in steps:
        _feed(params, step, skip=("B",) if step == skip_at else ())
        opt.step()
        opt.zero_grad()


def test_unknown_state_precision_raises():
    from orv_amd.optim import FusedAdamW
    with pytest.raises(ValueError, match="state_precision"):
        FusedAdamW(_params().values(), state_precision="fp16")
    with pytest.raises(ValueError, match="state_precision"):
        FusedAdamW(_params().values(), state_precision="bf16", param_precision="stochastic")


def test_default_constructor_is_unchanged(standins):
    params = _params()
    opt = _opt(params)
    assert opt.state_precision == "fp32" and opt.param_precision == "bf16"
    assert set(opt.state_dict()) == {"step", "exp_avg", "exp_avg_sq", "numels", "param_precision", "seed", "state_precision"}
    _run(opt, params, range(2))
    assert standins == ["adamw_flat"] * 2
    f = opt._flat
    assert f["m"].dtype == torch.float32 and f["v"].dtype == torch.float32 and not {"m8", "v8", "m_exp", "v_exp"} & set(f)
    sd = opt.state_dict()
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "numels", "seg_start", "seg_step", "param_precision", "seed", "state_precision"}
    assert sd["state_precision"] == "fp32" and sd["exp_avg"] is f["m"]
    m, v = opt.moments()
    assert all(torch.equal(a, f["m"][o:o + p.numel()].view(p.shape)) for a, p, o in zip(m, opt.params, f["seg_start"].tolist()))
    assert all(a.shape == p.shape and a.dtype == torch.float32 for a, p in zip(v, opt.params))


@pytest.mark.parametrize("mode", ["bf16", "split_fp32", "stochastic"])
def test_fp8_buffers_dispatch_and_every_param_precision(standins, mode):
    params = _params()
    opt = _opt(params, state_precision="fp8", param_precision=mode, seed=9)
    start = {n: p.detach().clone() for n, p in params.items()}
    _run(opt, params, range(3))
    assert standins == ["adamw_flat_s8"] * 3
    f = opt._flat
    assert f["p"].numel() == _TOTAL
    assert [(f[k].dtype, f[k].numel()) for k in ("m8", "v8", "m_exp", "v_exp")] == [(torch.uint8, _TOTAL), (torch.uint8, _TOTAL),
                                                                                    (torch.uint8, _TOTAL // 256), (torch.uint8, _TOTAL // 256)]
    assert "m" not in f and "v" not in f
    assert not any(torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() >= _TOTAL for t in f.values())     # no fp32 moment buffer
    # the moment buffers shrink by 8 total - (2 + 2/256) total bytes exactly
    fp8_bytes = sum(f[k].numel() * f[k].element_size() for k in ("m8", "v8", "m_exp", "v_exp"))
    assert 8 * _TOTAL - fp8_bytes == 8 * _TOTAL - (2 * _TOTAL + 2 * _TOTAL // 256)
    assert ("lo" in f) == (mode == "split_fp32")
    assert all(not torch.equal(params[n], start[n]) for n in params)
    m, v = opt.moments()
    assert all(bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 for a in m + v) and all(bool((a >= 0).all()) for a in v)
    # After the FIRST step (from zero state the fp32 moments are the same in both runs) every stored moment is a grid neighbour of the fp32
    # one: an element above 2^-5 of the largest lies in the normal range of its block (|y| > 224 * 2^-5), where a step is at most 2^-M of
    # the value.
    params1, params2 = _params(), _params()
    one, ref = _opt(params1, state_precision="fp8", param_precision=mode, seed=9), _opt(params2, param_precision=mode, seed=9)
    _run(one, params1, range(1)), _run(ref, params2, range(1))
    (m, v), (rm, rv) = one.moments(), ref.moments()
    for a, b, tol in [(x, y, 2.0 ** -3) for x, y in zip(m, rm)] + [(x, y, 2.0 ** -2) for x, y in zip(v, rv)]:
        big = b.abs() > b.abs().max() * 2.0 ** -5
        assert float(((a - b).abs() / b.abs())[big].max()) < tol


def test_fp8_state_dict_round_trip_and_resume(standins):
    params = _params()
    opt = _opt(params, state_precision="fp8", param_precision="split_fp32", seed=11)
    _run(opt, params, range(3), skip_at=1)
    sd = opt.state_dict()
    assert sd["state_precision"] == "fp8" and "exp_avg" not in sd and "exp_avg_sq" not in sd
    assert [sd[k].dtype for k in ("exp_avg8", "exp_avg_sq8", "exp_avg_exp", "exp_avg_sq_exp")] == [torch.uint8] * 4
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    params2 = {n: torch.nn.Parameter(p.detach().clone()) for n, p in params.items()}
    opt2 = _opt(params2, state_precision="fp8", param_precision="split_fp32")
    opt2.load_state_dict(sd)
    assert opt2.seed == 11 and opt2.step_count == 3 and opt2._flat["seg_step"].tolist() == [3, 2, 3]
    for k in ("m8", "v8", "m_exp", "v_exp", "lo"):
        assert torch.equal(opt2._flat[k], opt._flat[k])
    for o, ps in ((opt, params), (opt2, params2)):
        _feed(ps, 3)
        o.step()
    assert all(torch.equal(params[n], params2[n]) for n in params)
    assert all(torch.equal(opt._flat[k], opt2._flat[k]) for k in ("m8", "v8", "m_exp", "v_exp", "lo"))
    assert "state8_quantize" not in standins and "state8_dequantize" not in standins                # same precision: bytes are copied
    # a state dict taken before the first step
    empty = _opt(_params(), state_precision="fp8").state_dict()
    assert empty["exp_avg8"] is None and empty["exp_avg_exp"] is None and "exp_avg" not in empty
    # layout mismatches keep raising
    bad = dict(sd, exp_avg_exp=sd["exp_avg_exp"][:-1])
    with pytest.raises(ValueError, match="flat layout"):
        _opt(_params(), state_precision="fp8").load_state_dict(bad)
    with pytest.raises(ValueError, match="different set"):
        _opt(_params(), state_precision="fp8").load_state_dict(dict(sd, numels=[1, 2]))


def test_loads_across_state_precisions(standins):
    params = _params()
    src32 = _opt(params, seed=4)
    _run(src32, params, range(3), skip_at=2)
    sd32 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in src32.state_dict().items()}
    # fp32 -> fp8: quantised with the checkpoint's seed and step
    dst8 = _opt(_params(), state_precision="fp8", seed=99)
    dst8.load_state_dict(sd32)
    assert dst8.seed == 4 and dst8.step_count == 3 and dst8._flat["seg_step"].tolist() == [3, 2, 3]
    for key, q, e, fmt in (("exp_avg", "m8", "m_exp", 0), ("exp_avg_sq", "v8", "v_exp", 1)):
        wq, we = s8.quantize(sd32[key], fmt, seed=4, step=3)
        assert torch.equal(dst8._flat[q], wq) and torch.equal(dst8._flat[e], we)
    old = {k: v for k, v in sd32.items() if k not in ("param_precision", "seed", "state_precision")}        # written before the arguments existed
    dst8b = _opt(_params(), state_precision="fp8", seed=4)
    dst8b.load_state_dict(old)
    assert torch.equal(dst8b._flat["m8"], dst8._flat["m8"]) and torch.equal(dst8b._flat["v_exp"], dst8._flat["v_exp"])
    # fp8 -> fp32: exact, equal to moments()
    m8, v8 = dst8.moments()
    sd8 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in dst8.state_dict().items()}
    dst32 = _opt(_params())
    dst32.load_state_dict(sd8)
    assert dst32.state_precision == "fp32" and dst32._flat["m"].dtype == torch.float32
    m32, v32 = dst32.moments()
    assert all(torch.equal(a, b) for a, b in zip(m8 + v8, m32 + v32))
    # ... and back again without a change of value (the rule is idempotent on values)
    again = _opt(_params(), state_precision="fp8")
    again.load_state_dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in dst32.state_dict().items()})
    ma, va = again.moments()
    assert all(torch.equal(a, b) for a, b in zip(ma + va, m8 + v8))
    with pytest.raises(ValueError, match="flat layout"):
        _opt(_params(), state_precision="fp8").load_state_dict(dict(sd32, exp_avg=sd32["exp_avg"][:2048]))
    with pytest.raises(ValueError, match="flat layout"):
        _opt(_params()).load_state_dict(dict(sd8, exp_avg_sq8=sd8["exp_avg_sq8"][:2048]))


def test_inactive_parameters_keep_every_byte(standins):
    params = _params()
    opt = _opt(params, state_precision="fp8", param_precision="split_fp32")
    _run(opt, params, range(2))
    f = opt._flat
    a, b = f["seg_start"].tolist()[1:3]                                                            # segment of "B"
    keep = {k: f[k][a // d:b // d].clone() for k, d in (("p", 1), ("lo", 1), ("m8", 1), ("v8", 1), ("m_exp", 256), ("v_exp", 256))}
    rest = {k: f[k].clone() for k in ("m8", "v8", "m_exp")}
    _run(opt, params, [2], skip_at=2)
    for k, d in (("p", 1), ("lo", 1), ("m8", 1), ("v8", 1), ("m_exp", 256), ("v_exp", 256)):
        assert torch.equal(f[k][a // d:b // d], keep[k]), k
    assert all(not torch.equal(f[k], rest[k]) for k in rest)                                       # the others moved
    assert f["seg_step"].tolist() == [3, 2, 3]


# ---- 4. exports ----
def test_state8_entry_points_are_declared_exported_and_in_signatures():
    from orv_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "orv_mi355.h")).read()
    h = _lib.lib()
    for name in ("orv_adamw_flat_s8", "orv_state8_quantize", "orv_state8_dequantize"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and getattr(h, name) is not None
    assert len(_lib.SIGNATURES["orv_adamw_flat_s8"][1]) == len(_lib.SIGNATURES["orv_adamw_flat_ex"][1]) + 2      # m, v -> m8, v8, m_exp, v_exp
    assert all(callable(getattr(ops, n)) for n in ("adamw_flat_s8", "state8_quantize", "state8_dequantize"))
    p = 1 << 20                                                                                    # never dereferenced: validation fails first
    call = lambda n, lo, mode: h.orv_adamw_flat_s8(p, p, p, p, p, p, n, p, p, None, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, None, lo, mode, 0, None)
    assert call(2048, None, 3) != 0 and b"mode" in h.orv_last_error()
    assert call(2048, None, 1) != 0 and b"lo" in h.orv_last_error()
    assert call(1000, None, 0) != 0 and b"2048" in h.orv_last_error()
    assert h.orv_state8_quantize(p, p, p, 256, 2, 0, 1, None) != 0 and b"format" in h.orv_last_error()
    assert h.orv_state8_quantize(p, p, p, 100, 0, 0, 1, None) != 0 and b"256" in h.orv_last_error()
    assert h.orv_state8_dequantize(p, p, p, 256, -1, None) != 0 and b"format" in h.orv_last_error()
    assert h.orv_state8_dequantize(p, p, p, 0, 1, None) != 0 and b"256" in h.orv_last_error()
