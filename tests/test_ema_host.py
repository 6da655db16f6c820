"""CPU: the decay schedule of ``orv_amd.FusedEMA`` against hand-derived values, the bf16 stall that makes an fp32 shadow necessary, the fp32
recurrence of tests/ema_ref.py against float64, the C ABI surface and its validation, and the host logic of ``FusedEMA`` (shadow layout,
stash refusals, checkpoints) over a CPU stand-in for the two kernel entry points."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
SHAPES = [(1,), (2047,), (2049,), (3, 5)]
# 4 x the largest relative error test_fp32_recurrence_against_float64 prints (1.077e-6).  A property of the rule.
RECURRENCE_BOUND = 4.31e-6


# ---- the schedule ----
def _ema(params=None, precision="bf16", **kw):
    from orv_amd import FusedEMA
    from orv_amd.optim import FusedAdamW
    params = _params() if params is None else params
    return FusedEMA(FusedAdamW(params, param_precision=precision), **kw), params


def _params(seed=7, shapes=SHAPES):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.02).to(BF)) for s in shapes]


@pytest.mark.parametrize("after", [0, 5])
def test_get_decay_hand_derived_values(after):
    plain, _ = _ema(update_after_step=after)
    warm, _ = _ema(update_after_step=after, use_ema_warmup=True)
    for e in (plain, warm):
        assert all(e.get_decay(k) == 0.0 for k in range(0, after + 2))                # 0 up to update_after_step + 1
    assert plain.get_decay(after + 2) == 2 / 11                                       # step 1: (1 + 1) / (10 + 1)
    assert plain.get_decay(after + 3) == 3 / 12
    assert warm.get_decay(after + 2) == 1 - 2 ** (-2 / 3)                             # step 1: 1 - (1 + 1 / 1)^(-2/3)
    assert abs(warm.get_decay(after + 2) - 0.37003947505256) < 1e-13
    slow, _ = _ema(update_after_step=after, use_ema_warmup=True, inv_gamma=4.0, power=1.0)
    assert slow.get_decay(after + 5) == 1 - 1 / (1 + 4 / 4.0)                         # step 4: 1 - (1 + 4/4)^-1 = 0.5
    # the cap and the floor
    assert plain.get_decay(after + 10 ** 7) == 0.9999 and warm.get_decay(after + 10 ** 9) == 0.9999
    capped, _ = _ema(decay=0.5, update_after_step=after)
    assert capped.get_decay(after + 2) == 2 / 11 and capped.get_decay(after + 10) == 0.5 and capped.get_decay(after + 1000) == 0.5
    floored, _ = _ema(decay=0.9, min_decay=0.3, update_after_step=after)
    assert floored.get_decay(after + 2) == 0.3 and floored.get_decay(after + 3) == 0.3 and floored.get_decay(after + 5) == 5 / 14
    assert floored.get_decay(after + 1) == 0.0                                        # before the first counted step the floor does not apply
    for k in (0, 1, 2, 3, 17, 5000):
        kw = dict(decay=0.999, min_decay=0.1, update_after_step=after, use_ema_warmup=bool(k & 1), inv_gamma=2.0, power=0.75)
        assert _ema(**kw)[0].get_decay(k) == R.get_decay(k, **kw)
    with pytest.raises(ValueError, match=r"must lie in \[0, 1\]"):
        _ema(decay=1.5)
    with pytest.raises(TypeError, match="FusedAdamW / FusedProdigy / FusedCAME"):
        from orv_amd import FusedEMA
        FusedEMA(torch.optim.SGD(_params(), lr=0.1))


# ---- why the shadow is fp32 ----
def test_bf16_shadow_stalls_and_fp32_shadow_moves():
    """1000 steps at decay 0.9999 towards weights 25 % away: ``EMAModel``'s expression ``s.sub_(omd * (s - p))`` on a bf16 shadow changes
    no element (omd |s - p| = 2.5e-5 |s| is below half a bf16 step, 2^-9 |s| at least); the fp32 rule follows the closed form."""
    gen = torch.Generator().manual_seed(0)
    s0 = (torch.randn(4096, generator=gen) * 0.02).to(BF)
    s0 = torch.where(s0 == 0, torch.full_like(s0, 0.02), s0)
    p = (s0.float() * 1.25).to(BF)                                # exact in bf16 up to one rounding; fixed target
    omd = 1.0 - 0.9999
    s16 = s0.clone()
    p_bits = R.bits_of_bf16(p)
    s32 = s0.float().numpy().copy()
    for _ in range(1000):
        s16.sub_(omd * (s16 - p))
        s32 = R.update(s32, p_bits, None, R.omd_of(0.9999))
    assert torch.equal(s16, s0), "the bf16 shadow moved"
    want = p.double().numpy() + (s0.double().numpy() - p.double().numpy()) * (1.0 - float(R.omd_of(0.9999))) ** 1000
    assert np.all(s32 != s0.float().numpy())
    progress = (s32.astype(np.float64) - s0.double().numpy()) / (p.double().numpy() - s0.double().numpy())
    assert abs(progress.mean() - (1 - 0.9999 ** 1000)) < 1e-4 and 0.09 < progress.min() <= progress.max() < 0.1       # 0.0952
    assert np.max(np.abs(s32 - want) / np.abs(want)) < 1e-4            # at most 1000 roundings of 2^-24 each, 6e-5


def test_fp32_recurrence_against_float64():
    """2000 steps of the rule in fp32 (ema_ref.update) and in float64 on the same data: fp32 masters doing a random walk (relative step
    1e-3) from N(0, 0.02), the default schedule (decay (1 + k) / (10 + k) capped at 0.9999), the same fp32-rounded ``omd``.  The error of an
    element is taken relative to the largest magnitude its inputs took (the scale fp32 rounding works at)."""
    rng = np.random.default_rng(0)
    n = 4096
    w = (rng.standard_normal(n) * 0.02).astype(np.float32)
    s32, s64 = w.copy(), w.astype(np.float64)
    scale = np.abs(w).astype(np.float64)
    for k in range(1, 2001):
        w = (w * (1 + 1e-3 * rng.standard_normal(n))).astype(np.float32)
        omd = R.omd_of(R.get_decay(k))
        u = w.view(np.uint32)
        p_bits = ((u + np.uint32(0x8000)) >> np.uint32(16)).astype(np.uint16)
        lo = (u - (p_bits.astype(np.uint32) << np.uint32(16))).astype(np.int32).astype(np.int16)     # tie-away split: theta == w
        assert np.array_equal(R.theta(p_bits, lo).view(np.uint32), u)
        s32 = R.update(s32, p_bits, lo, omd)
        s64 = s64 - float(omd) * (s64 - w.astype(np.float64))
        scale = np.maximum(scale, np.abs(w))
    err = float(np.max(np.abs(s32.astype(np.float64) - s64) / scale))
    print(f"\nema fp32 recurrence vs float64, 2000 steps: largest relative error {err:.3e} (bound {RECURRENCE_BOUND:.1e})")
    assert err <= RECURRENCE_BOUND


# ---- C ABI ----
NAMES = ("orv_ema_update", "orv_ema_swap_in")


def test_symbols_are_declared_exported_and_bound():
    import orv_amd
    from orv_amd import _lib, ema, ops, sft
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(_lib.lib(), name) is not None
        params = re.search(r"^int " + name + r"\(([^)]*)\)", hdr, re.M).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert callable(ops.ema_update) and callable(ops.ema_swap_in)
    assert orv_amd.FusedEMA is ema.FusedEMA
    assert "optim_ema.hip" in open(os.path.join(ROOT, "orv_amd", "csrc", "Makefile")).read()
    assert inspect.signature(sft.sft_step).parameters["ema"].default is None
    assert list(inspect.signature(ema.FusedEMA.__init__).parameters)[1:] == ["optimizer", "decay", "min_decay", "update_after_step",
                                                                           "use_ema_warmup", "inv_gamma", "power"]


def test_entry_points_validate_before_any_launch():
    """The C entry points return before any HIP call on a bad argument (addresses are never dereferenced on the host), so this runs without
    a GPU; the Python wrappers refuse CPU tensors before they reach the library."""
    from orv_amd import _lib, ops
    h = _lib.lib()
    A, B, C, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    err = lambda: h.orv_last_error().decode()
    assert h.orv_ema_update(A, B, None, 2049, 0.5, None) != 0 and "multiple of 2048" in err()
    assert h.orv_ema_update(A, B, None, 0, 0.5, None) != 0 and "multiple of 2048" in err()
    for args in ((A + 4, B, None), (A, B + 2, None), (A, B, C + 8)):
        assert h.orv_ema_update(*args, 4096, 0.5, None) != 0 and "16-byte aligned" in err()
    assert h.orv_ema_update(None, B, None, 2048, 0.5, None) != 0 and "null buffer" in err()
    assert h.orv_ema_update(A, None, None, 2048, 0.5, None) != 0 and "null buffer" in err()
    for omd in (-0.1, 1.5, float("nan")):
        assert h.orv_ema_update(A, B, None, 2048, omd, None) != 0 and "[0, 1]" in err()
    assert h.orv_ema_swap_in(A, None, C, None, None, 2047, 0, None) != 0 and "multiple of 2048" in err()
    for args in ((A + 2, B, C, D, E), (A, B + 2, C, D, E), (A, B, C + 4, D, E), (A, B, C, D + 8, E), (A, B, C, D, E + 2)):
        assert h.orv_ema_swap_in(*args, 2048, 0, None) != 0 and "16-byte aligned" in err()
    assert h.orv_ema_swap_in(None, B, C, None, None, 2048, 0, None) != 0 and "null buffer" in err()
    assert h.orv_ema_swap_in(A, None, C, None, None, 2048, 1, None) != 0 and "without the low-half buffer" in err()
    assert h.orv_ema_swap_in(A, None, C, D, E, 2048, 0, None) != 0 and "without the low-half buffer" in err()
    assert h.orv_ema_swap_in(A, B, C, None, E, 2048, 0, None) != 0 and "without stash_p" in err()
    assert h.orv_ema_swap_in(A, B, C, A, E, 2048, 0, None) != 0 and "aliases" in err()
    s, p, lo = torch.zeros(2048), torch.zeros(2048, dtype=BF), torch.zeros(2048, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.ema_update(s, p, lo, 0.5)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.ema_swap_in(p, s, lo)


# ---- FusedEMA over the stand-in ----
@pytest.fixture
def standin():
    """``ops.ema_update`` / ``ops.ema_swap_in`` on CPU tensors through tests/ema_ref.py, in place; records (name, omd) per call."""
    from orv_amd import ops
    saved = ops.ema_update, ops.ema_swap_in
    calls = []

    def ema_update(shadow, p, lo=None, one_minus_decay=0.0):
        calls.append(("update", one_minus_decay))
        new = R.update(shadow.numpy(), R.bits_of_bf16(p), None if lo is None else lo.numpy(), one_minus_decay)
        shadow.copy_(torch.from_numpy(new))

    def ema_swap_in(p, shadow, lo=None, stash_p=None, stash_lo=None, zero_lo=False):
        calls.append(("swap_in", bool(zero_lo)))
        if stash_p is not None:
            stash_p.copy_(p)
        if stash_lo is not None:
            stash_lo.copy_(lo)
        p.copy_(R.bf16_of_bits(R.bf16_rne(shadow.numpy())))
        if zero_lo:
            lo.zero_()

    ops.ema_update, ops.ema_swap_in = ema_update, ema_swap_in
    yield calls
    ops.ema_update, ops.ema_swap_in = saved


def _fill_lo(opt, seed=3):
    gen = torch.Generator().manual_seed(seed)
    for v in opt._flat["views_lo"]:                      # parameters only: the padding keeps lo = 0
        v.copy_(torch.randint(-32768, 32768, v.shape, generator=gen, dtype=torch.int64).to(torch.int16))


@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_shadow_layout_initialisation_and_state_dict_keys(precision):
    from orv_amd import FusedEMA
    from orv_amd.optim import FusedAdamW
    params = _params()
    opt = FusedAdamW(params, param_precision=precision)
    if precision == "split_fp32":
        opt._build()
        _fill_lo(opt)
    ema = FusedEMA(opt, decay=0.99, update_after_step=2)
    f = opt._flat
    assert ema.shadow.dtype == torch.float32 and ema.shadow.numel() == f["p"].numel() == sum(-(-p.numel() // 2048) * 2048 for p in params)
    views = ema.shadow_tensors()
    assert list(views) == opt.params
    inside = torch.zeros(ema.shadow.numel(), dtype=torch.bool)
    for (p, v), m, o in zip(views.items(), opt.master_params(), f["offs"]):
        assert v.shape == p.shape and v.data_ptr() == ema.shadow.data_ptr() + 4 * o
        assert torch.equal(v.view(torch.int32), m.view(torch.int32))           # the master, bit for bit
        inside[o:o + p.numel()] = True
    assert not bool(ema.shadow[~inside].view(torch.int32).any()), "padding of the shadow is not zero"
    if precision == "split_fp32":
        assert any(not torch.equal(v, p.detach().float()) for p, v in views.items())
    sd = ema.state_dict()
    assert set(sd) == {"decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power",
                       "shadow_params", "shapes"}
    assert (sd["decay"], sd["min_decay"], sd["optimization_step"], sd["update_after_step"], sd["use_ema_warmup"], sd["inv_gamma"],
            sd["power"]) == (0.99, 0.0, 0, 2, False, 1.0, 2 / 3)
    assert sd["shapes"] == [list(p.shape) for p in opt.params]
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(sd["shadow_params"], views.values()))


def _feed(params, t):
    for i, p in enumerate(params):
        gen = torch.Generator().manual_seed(1000 * t + i)
        p.grad = (torch.randn(p.shape, generator=gen) * 0.05).to(BF)


@pytest.fixture
def adamw_standin():
    import adamw_ref
    from orv_amd import ops
    saved = ops.sumsq, ops.adamw_flat, ops.adamw_flat_ex

    def sumsq(g, out):
        out.add_(g.float().pow(2).sum())

    def adamw_flat(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None, seg_step=None):
        adamw_ref.adamw_flat_ex(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef, seg_step=seg_step)

    ops.sumsq, ops.adamw_flat, ops.adamw_flat_ex = sumsq, adamw_flat, adamw_ref.adamw_flat_ex
    yield
    ops.sumsq, ops.adamw_flat, ops.adamw_flat_ex = saved


@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_step_swap_restore_and_refusals(standin, adamw_standin, precision):
    from orv_amd import FusedEMA, _state
    from orv_amd.optim import FusedAdamW
    params = _params()
    opt = FusedAdamW(params, lr=1e-2, param_precision=precision)
    ema = FusedEMA(opt, decay=0.3)
    want = ema.shadow.numpy().copy()
    for t in range(1, 5):
        _feed(params, t)
        opt.step()
        opt.zero_grad()
        ema.step()
        want = R.update(want, R.bits_of_bf16(opt._flat["p"]), opt._flat["lo"].numpy() if precision == "split_fp32" else None,
                        R.omd_of(R.get_decay(t, decay=0.3)))
    assert ema.optimization_step == 4 and ema.cur_decay_value == 0.3
    assert [c for c in standin] == [("update", 1.0), ("update", float(np.float32(1 - 2 / 11))), ("update", 0.75), ("update", float(np.float32(1 - 0.3)))]
    assert np.array_equal(ema.shadow.numpy().view(np.uint32), want.view(np.uint32))
    f = opt._flat
    p0, lo0 = f["p"].clone(), f["lo"].clone() if "lo" in f else None
    versions = [p._version for p in params]
    epoch = _state.weights_epoch[0]
    with ema.average_parameters() as inner:
        assert inner is ema and _state.weights_epoch[0] > epoch
        assert np.array_equal(R.bits_of_bf16(f["p"]), R.bf16_rne(want))
        assert all(torch.equal(p.detach(), v.to(BF)) for p, v in ema.shadow_tensors().items())
        assert lo0 is None or torch.equal(f["lo"], lo0)
        with pytest.raises(RuntimeError, match=r"FusedEMA.step: the averaged weights are swapped in.*restore\(\)"):
            ema.step()
        with pytest.raises(RuntimeError, match=r"FusedEMA.store: a stash is already held.*restore\(\)"):
            ema.store()
        with pytest.raises(RuntimeError, match="a stash is already held"):
            with ema.average_parameters():
                pass
        epoch = _state.weights_epoch[0]
    assert _state.weights_epoch[0] > epoch and ema._stash is None
    assert torch.equal(f["p"].view(torch.int16), p0.view(torch.int16)) and (lo0 is None or torch.equal(f["lo"], lo0))
    assert [p._version for p in params] == versions           # a moved version would make the optimizer drop the low halves
    assert standin[-1] == ("swap_in", False) and ema.optimization_step == 4
    with pytest.raises(RuntimeError, match="nothing is stashed"):
        ema.restore()
    # store / copy_to / restore by hand: the same
    ema.store()
    ema.copy_to()
    assert standin[-1] == ("swap_in", False) and np.array_equal(R.bits_of_bf16(f["p"]), R.bf16_rne(want))
    ema.restore()
    assert torch.equal(f["p"].view(torch.int16), p0.view(torch.int16)) and (lo0 is None or torch.equal(f["lo"], lo0))
    # copy_to outside a pair: the averages become the weights, masters included
    ema.copy_to()
    assert standin[-1] == ("swap_in", precision == "split_fp32")
    for m, v in zip(opt.master_params(), ema.shadow_tensors().values()):
        assert torch.equal(m, v.to(BF).float())


class _Saver:
    def __init__(self, params):
        self.params, self.seen = params, None

    def save_pretrained(self, directory, **kw):
        self.seen = (directory, kw, [p.detach().clone() for p in self.params])


def test_save_pretrained_swaps_and_restores(standin):
    ema, params = _ema(precision="split_fp32")
    with torch.no_grad():
        ema.shadow.mul_(1.5)
    before = [p.detach().clone() for p in params]
    model = _Saver(params)
    ema.save_pretrained(model, "somewhere", max_shard_size="1MB")
    assert model.seen[:2] == ("somewhere", {"max_shard_size": "1MB"})
    assert all(torch.equal(w, v.to(BF)) for w, v in zip(model.seen[2], ema.shadow_tensors().values()))
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before)) and ema._stash is None


def test_state_dict_round_trip_and_refusals(standin, adamw_standin):
    from orv_amd import FusedEMA
    from orv_amd.optim import FusedAdamW

    def run(steps, save_at=None):
        params = _params()
        opt = FusedAdamW(params, lr=1e-2, param_precision="split_fp32")
        ema = FusedEMA(opt, decay=0.9, use_ema_warmup=True)
        for t in range(1, steps + 1):
            if t == save_at:
                sd = {k: ([x.clone() for x in v] if k == "shadow_params" else v) for k, v in ema.state_dict().items()}
                osd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
                weights = [p.detach().clone() for p in params]
                params = _params(seed=8)
                with torch.no_grad():
                    for p, w in zip(params, weights):
                        p.copy_(w)
                opt = FusedAdamW(params, lr=1e-2, param_precision="split_fp32")
                opt.load_state_dict(osd)
                ema = FusedEMA(opt)                      # other hyper-parameters: the checkpoint's win
                ema.load_state_dict(sd)
                assert (ema.decay, ema.use_ema_warmup, ema.optimization_step) == (0.9, True, t - 1)
            _feed(params, t)
            opt.step()
            opt.zero_grad()
            ema.step()
        return ema

    a, b = run(6), run(6, save_at=4)
    assert torch.equal(a.shadow.view(torch.int32), b.shadow.view(torch.int32)) and a.optimization_step == b.optimization_step == 6
    sd = a.state_dict()
    permuted, _ = _ema(params=_params(shapes=SHAPES[::-1]))
    with pytest.raises(ValueError, match="FusedEMA.load_state_dict: same parameters, another flat-buffer ORDER"):
        permuted.load_state_dict(sd)
    other, _ = _ema(params=_params(shapes=SHAPES[:2]))
    with pytest.raises(ValueError, match="different set of trainable parameters"):
        other.load_state_dict(sd)
    legacy = {k: v for k, v in sd.items() if k != "shapes"}            # EMAModel's own keys only: the tensors' shapes are compared
    with pytest.raises(ValueError, match="another flat-buffer ORDER"):
        permuted.load_state_dict(legacy)
