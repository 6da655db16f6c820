"""CPU: the opt-in parameter-precision modes of FusedAdamW (``param_precision="split_fp32"`` / ``"stochastic"``).

The split format and the stochastic hash are checked on their Python restatement (tests/adamw_ref.py), the C ABI symbol on the built
library, and the optimizer's host logic (argument, dispatch, checkpoint, stale low halves, data parallel) with the kernels replaced by
that restatement - test infrastructure in the style of tests/test_dp_optimizer.py, never shipped."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import adamw_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


# ---- 1. split / rebuild ----
def _specials():
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,
            0x3F800000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x00008000, 0x80018000]
    return adamw_ref.bits_f32(torch.tensor(bits, dtype=torch.int64))


def test_split_rebuild_is_exact_and_lo_fits_int16():
    g = torch.Generator().manual_seed(0)
    parts = [torch.randn(220_000, generator=g) * s for s in (1e-30, 1e-3, 0.02, 1.0, 1e20)]
    # forced exact ties: low half exactly 0x8000, on even and odd upper halves, both signs
    u = adamw_ref.f32_bits(torch.randn(100_000, generator=g) * 0.02)
    ties = adamw_ref.bits_f32((u & 0xFFFF0000) | 0x8000)
    denorm = adamw_ref.bits_f32(torch.randint(1, 0x00800000, (50_000,), generator=g, dtype=torch.int64))
    x = torch.cat(parts + [ties, denorm, -denorm, _specials()])
    assert x.numel() >= 10 ** 6 and bool(torch.isfinite(x).all())
    p, lo = adamw_ref.split(x)
    assert p.dtype == BF and lo.dtype == torch.int16
    back = adamw_ref.rebuild(p, lo)
    assert torch.equal(adamw_ref.f32_bits(back), adamw_ref.f32_bits(x))          # bit for bit, -0 and denormals included
    # p is the nearest-even bf16 everywhere except on exact ties, where it is the one away from zero
    tie = (adamw_ref.f32_bits(x) & 0xFFFF) == 0x8000
    rne = x.to(BF)
    assert torch.equal(adamw_ref.bf16_bits(p)[~tie], adamw_ref.bf16_bits(rne)[~tie])
    assert int(tie.sum()) >= 100_000
    assert bool((p[tie].float().abs() > x[tie].abs()).all())
    assert bool(((p[tie].float() - x[tie]).abs() == (rne[tie].float() - x[tie]).abs()).all())      # still a nearest value
    odd = tie & ((adamw_ref.f32_bits(x) >> 16) & 1 == 1)
    assert int(odd.sum()) > 0 and torch.equal(adamw_ref.bf16_bits(p)[odd], adamw_ref.bf16_bits(rne)[odd])   # odd upper half: RNE goes away too
    assert int(lo.min()) == -32768 and int(lo.max()) == 32767


def test_split_nonfinite_writes_matching_bf16_and_zero_lo():
    x = adamw_ref.bits_f32(torch.tensor([0x7F800000, 0xFF800000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF], dtype=torch.int64))
    p, lo = adamw_ref.split(x)
    assert adamw_ref.bf16_bits(p).tolist() == [0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7FFF] and lo.tolist() == [0] * 5


def test_stochastic_round_restatement():
    """Known answers of the hash (computed by hand-running the definition with Python integers) and the rounding rules."""
    def mix(x):
        x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF; x ^= x >> 16
        return x
    for seed, step, i in [(0, 1, 0), (7, 3, 12345), (0xFFFFFFFF, 100, 2 ** 32 + 5), (1, 1, 1_690_000_000)]:
        key = mix(((i >> 32) + mix((step + mix(seed)) & 0xFFFFFFFF)) & 0xFFFFFFFF)
        assert int(adamw_ref.sr_offsets(seed, step, [i])[0]) == mix((i & 0xFFFFFFFF) ^ key) >> 16
    r = adamw_ref.sr_offsets(3, 9, np.arange(1 << 20))
    assert int(r.min()) >= 0 and int(r.max()) <= 65535 and abs(float(r.double().mean()) - 32767.5) < 6 * 18918 / 1024     # uniform: std 65536 / sqrt(12)
    assert not torch.equal(r, adamw_ref.sr_offsets(4, 9, np.arange(1 << 20))) and not torch.equal(r, adamw_ref.sr_offsets(3, 10, np.arange(1 << 20)))
    x = adamw_ref.bits_f32(torch.tensor([0x3F800000, 0x3F80FFFF, 0x3F800001, 0x7F7FFFFF, 0xFF7F0001, 0x7F800000, 0x7FA00000], dtype=torch.int64))
    rr = torch.tensor([0xFFFF, 1, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF])
    assert adamw_ref.bf16_bits(adamw_ref.stochastic_round(x, rr)).tolist() == [0x3F80, 0x3F81, 0x3F81, 0x7F7F, 0xFF7F, 0x7F80, 0x7FE0]
    # unbiased: the mean of the rounded values of one number over all 65536 offsets is the number
    one = torch.full((65536,), 0.999, dtype=torch.float32)
    mean = adamw_ref.stochastic_round(one, torch.arange(65536)).double().mean()
    assert abs(float(mean) - float(one[0].double())) < 1e-9


# ---- 2. symbol ----
def test_adamw_flat_ex_is_declared_exported_and_in_signatures():
    from orv_amd import _lib
    header = open(os.path.join(ROOT, "include", "orv_mi355.h")).read()
    assert re.search(r"\bint\s+orv_adamw_flat_ex\s*\(", header)
    assert "orv_adamw_flat_ex" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["orv_adamw_flat_ex"]
    assert len(args) == len(_lib.SIGNATURES["orv_adamw_flat_steps"][1]) + 3          # + lo, mode, seed
    h = _lib.lib()
    assert h.orv_adamw_flat_ex is not None
    p = 1 << 20                                                                        # never dereferenced: validation fails first
    call = lambda n, lo, mode: h.orv_adamw_flat_ex(p, p, p, p, n, p, p, None, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, None, lo, mode, 0, None)
    assert call(2048, None, 3) != 0 and b"mode" in h.orv_last_error()
    assert call(2048, None, 1) != 0 and b"lo" in h.orv_last_error()                    # split_fp32 needs the low halves
    assert call(1000, p, 1) != 0 and b"2048" in h.orv_last_error()
    assert call(1000, None, 2) != 0 and call(1000, None, 0) != 0


# ---- 3. host behaviour of FusedAdamW on stand-in kernels ----
def _install_standins(calls=None):
    from orv_amd import ops

    def sumsq(g, out):
        out.add_(g.float().pow(2).sum())

    def adamw_flat(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None, seg_step=None):
        if calls is not None:
            calls.append("adamw_flat")
        adamw_ref.adamw_flat_ex(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef, seg_step)

    def adamw_flat_ex(*a, **k):
        if calls is not None:
            calls.append("adamw_flat_ex")
        adamw_ref.adamw_flat_ex(*a, **k)

    ops.sumsq, ops.adamw_flat, ops.adamw_flat_ex = sumsq, adamw_flat, adamw_flat_ex


@pytest.fixture
def standins():
    from orv_amd import ops
    saved = ops.sumsq, ops.adamw_flat, ops.adamw_flat_ex
    calls = []
    _install_standins(calls)
    yield calls
    ops.sumsq, ops.adamw_flat, ops.adamw_flat_ex = saved


_SHAPES = {"A": (64, 40), "B": (3000,), "C": (17, 9)}


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


def test_unknown_param_precision_raises():
    from orv_amd.optim import FusedAdamW
    with pytest.raises(ValueError, match="param_precision"):
        FusedAdamW(_params().values(), param_precision="fp32")
    with pytest.raises(ValueError, match="seed"):
        FusedAdamW(_params().values(), param_precision="stochastic", seed=-1)


def test_default_mode_calls_adamw_flat_and_new_modes_the_new_op(standins):
    for mode, want in (("bf16", "adamw_flat"), ("split_fp32", "adamw_flat_ex"), ("stochastic", "adamw_flat_ex")):
        del standins[:]
        params = _params()
        opt = _opt(params, param_precision=mode)
        for step in range(2):
            _feed(params, step)
            opt.step()
            opt.zero_grad()
        assert standins == [want] * 2, (mode, standins)
        assert ("lo" in opt._flat) == (mode == "split_fp32")
    from orv_amd.optim import FusedAdamW
    assert FusedAdamW(_params().values()).param_precision == "bf16"


def test_split_mode_tracks_an_fp32_adamw_and_keeps_p_equal_to_the_rounded_master(standins):
    params = _params()
    ref = {n: p.detach().double().clone() for n, p in params.items()}
    opt = _opt(params, param_precision="split_fp32")
    rm = {n: torch.zeros(s, dtype=torch.float64) for n, s in _SHAPES.items()}
    rv = {n: torch.zeros(s, dtype=torch.float64) for n, s in _SHAPES.items()}
    for step in range(1, 6):
        _feed(params, step)
        grads = {n: p.grad.double() for n, p in params.items()}
        norm = torch.sqrt(sum((g ** 2).sum() for g in grads.values()))
        clip = min(1.0, 1.0 / (float(norm) + 1e-6))
        for n in ref:
            ref[n], rm[n], rv[n] = adamw_ref.formula(ref[n], grads[n], rm[n], rv[n], clip, 2e-4, 0.9, 0.95, 1e-8, 1e-3, step, torch.float64)
        opt.step()
        opt.zero_grad()
    for (n, p), master in zip(params.items(), opt.master_params()):
        assert master.dtype == torch.float32 and master.shape == p.shape
        assert torch.equal(adamw_ref.bf16_bits(p), adamw_ref.bf16_bits(adamw_ref.split(master)[0]))
        moved = (ref[n] - _params()[n].detach().double()).abs().mean()
        assert (master.double() - ref[n]).abs().mean() <= 1e-4 * moved          # fp32 accumulation, far below a bf16 step


def test_state_dict_round_trip_keeps_param_lo_seed_and_step_counts(standins):
    params = _params()
    opt = _opt(params, param_precision="split_fp32", seed=11)
    for step in range(3):
        _feed(params, step, skip=("B",) if step == 1 else ())
        opt.step()
        opt.zero_grad()
    sd = opt.state_dict()
    assert sd["param_precision"] == "split_fp32" and sd["seed"] == 11 and sd["param_lo"].dtype == torch.int16
    assert int(sd["param_lo"].abs().max()) > 0
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    params2 = {n: torch.nn.Parameter(p.detach().clone()) for n, p in params.items()}
    opt2 = _opt(params2, param_precision="split_fp32")
    opt2.load_state_dict(sd)
    assert opt2.seed == 11 and opt2.step_count == 3 and opt2._flat["seg_step"].tolist() == [3, 2, 3]
    assert torch.equal(opt2._flat["lo"], opt._flat["lo"]) and torch.equal(opt2._flat["m"], opt._flat["m"])
    for a, b in zip(opt.master_params(), opt2.master_params()):
        assert torch.equal(a, b)
    # ... and the resumed run continues bit for bit
    for o, ps in ((opt, params), (opt2, params2)):
        _feed(ps, 3)
        o.step()
    assert all(torch.equal(a, b) for a, b in zip(opt.master_params(), opt2.master_params()))
    assert all(torch.equal(params[n], params2[n]) for n in params)


def test_default_checkpoint_loads_into_split_mode_with_zero_lo_and_wrong_length_raises(standins):
    params = _params()
    opt = _opt(params)
    for step in range(2):
        _feed(params, step)
        opt.step()
        opt.zero_grad()
    sd = opt.state_dict()
    assert sd["param_precision"] == "bf16" and "param_lo" not in sd
    old = {k: v for k, v in sd.items() if k not in ("param_precision", "seed")}          # a checkpoint from before the argument existed
    for ckpt in (sd, old):
        params2 = {n: torch.nn.Parameter(p.detach().clone()) for n, p in params.items()}
        opt2 = _opt(params2, param_precision="split_fp32", seed=5)
        opt2._build()
        opt2._flat["lo"].fill_(123)                                                       # must not survive the load
        opt2.load_state_dict(ckpt)
        assert opt2.param_precision == "split_fp32" and int(opt2._flat["lo"].abs().max()) == 0
        assert opt2.seed == (0 if ckpt is sd else 5)
        assert all(torch.equal(mp_, p.detach().float()) for mp_, p in zip(opt2.master_params(), params2.values()))
    bad = dict(sd, param_lo=torch.zeros(2048, dtype=torch.int16))
    with pytest.raises(ValueError, match="param_lo"):
        _opt(_params(), param_precision="split_fp32").load_state_dict(bad)
    # a split checkpoint loads into the default mode, which keeps no low halves
    opt3 = _opt(_params())
    opt3.load_state_dict(dict(sd, param_lo=torch.zeros(opt._flat["p"].numel(), dtype=torch.int16), param_precision="split_fp32"))
    assert "lo" not in opt3._flat


def test_external_write_zeroes_that_parameters_lo_only(standins):
    params = _params()
    opt = _opt(params, param_precision="split_fp32")
    for step in range(2):
        _feed(params, step)
        opt.step()
        opt.zero_grad()
    names = list(params)
    views = dict(zip(names, opt._flat["views_lo"]))
    assert all(int(views[n].abs().max()) > 0 for n in names)
    before = {n: views[n].clone() for n in names}
    with torch.no_grad():
        params["B"].copy_(torch.full(_SHAPES["B"], 0.5, dtype=BF))
    seen = []
    real = adamw_ref.adamw_flat_ex

    def spy(p, g, m, v, *a, **k):
        seen.append(k["lo"].clone())
        real(p, g, m, v, *a, **k)

    from orv_amd import ops
    ops.adamw_flat_ex = spy
    _feed(params, 2)
    opt.step()
    lo_in = seen[0]
    off = dict(zip(names, opt._flat["seg_start"].tolist()))
    for n in names:
        got = lo_in[off[n]:off[n] + before[n].numel()]
        if n == "B":
            assert int(got.abs().max()) == 0
        else:
            assert torch.equal(got, before[n])
    # the optimizer's own writes never trigger it: the next step sees the low halves the last one left
    after = opt._flat["lo"].clone()
    _feed(params, 3)
    opt.step()
    assert torch.equal(seen[1], after)
    # writes through .data cannot be seen: reset_param_lo is for those
    params["A"].data.copy_(torch.full(_SHAPES["A"], 0.25, dtype=BF))
    opt.reset_param_lo([params["A"]])
    assert int(views["A"].abs().max()) == 0 and int(views["C"].abs().max()) > 0
    assert torch.equal(opt.master_params()[0], params["A"].detach().float())
    opt.reset_param_lo()
    assert int(opt._flat["lo"].abs().max()) == 0


# ---- 4. two ranks over gloo ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_USAGE = {"A": [(1, 1)] * 4, "B": [(1, 0), (0, 0), (1, 0), (0, 1)], "C": [(1, 0)] * 4}


def _rank_grad(name, step, rank):
    g = torch.Generator().manual_seed(1000 * step + 10 * rank + sum(map(ord, name)))
    return (torch.randn(_SHAPES[name], generator=g) * 0.3).to(BF)


def _dp_worker(rank, world, port, mode, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_standins()
    params = _params()
    opt = _opt(params, param_precision=mode, seed=3)
    for step in range(4):
        for n, p in params.items():
            p.grad = _rank_grad(n, step, rank) if _USAGE[n][step][rank] else None
        opt.step(average_over=world)
        opt.zero_grad()
    out.put((rank, {n: p.detach().float().numpy().copy() for n, p in params.items()},
             [mp_.numpy().copy() for mp_ in opt.master_params()]))
    dist.barrier()
    dist.destroy_process_group()


def _single_process(mode, monkeypatch):
    """One process on the rank-averaged gradient: p.grad is the SUM over ranks as the bf16 exchange leaves it (zeros for a rank without a
    gradient), the exchange itself is replaced by the identity and the world size reads 2, so the 1 / world rides in the clip coefficient
    exactly as in the two-rank run; a parameter nobody used has no gradient and is skipped."""
    from orv_amd import ops, sharding
    for name in ("sumsq", "adamw_flat", "adamw_flat_ex"):
        monkeypatch.setattr(ops, name, getattr(ops, name))          # restored after the test
    _install_standins()
    monkeypatch.setattr(sharding, "allreduce_flat_", lambda *a, **k: None)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    params = _params()
    opt = _opt(params, param_precision=mode, seed=3)
    for step in range(4):
        for n, p in params.items():
            u = _USAGE[n][step]
            p.grad = None
            if any(u):
                p.grad = sum((_rank_grad(n, step, r).float() if u[r] else torch.zeros(_SHAPES[n])) for r in range(2)).to(BF)
        opt.step(average_over=2)
        opt.zero_grad()
    return {n: p.detach().float().clone() for n, p in params.items()}, opt.master_params()


@pytest.mark.parametrize("mode", ["split_fp32", "stochastic"])
def test_two_ranks_stay_bit_identical_and_on_the_single_process_trajectory(mode, monkeypatch):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, mode, q)) for r in range(2)]
    [p.start() for p in procs]
    got = sorted([q.get(timeout=180) for _ in range(2)], key=lambda t: t[0])
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    (_, p0, m0), (_, p1, m1) = got
    ref_p, ref_m = _single_process(mode, monkeypatch)
    for i, n in enumerate(_SHAPES):
        assert np.array_equal(p0[n], p1[n]) and np.array_equal(m0[i], m1[i]), f"ranks diverged on {n}"
        assert torch.equal(torch.from_numpy(p0[n]), ref_p[n]), f"{n} left the single-process trajectory"
        assert torch.equal(torch.from_numpy(m0[i]), ref_m[i])
