"""GPU: FusedAdamW's parameter groups, per-parameter gradient norms and skip guard.

The per-group update kernels are held to their PARENTS bit for bit - one ``_groups`` launch against one parent launch per group on copies of
the same buffers - so no tolerance is involved; the two reductions are held bit for bit to their numpy restatement
(tests/adamw_groups_ref.py).  Layout of the kernel tests: seven segments of 1, 2047, 2048, 2049, 4096, 5000 and 3 elements, padded to 2048
by the optimizer's rule, three groups alternating so that neighbours differ, one segment inactive, one with its own step count - the
smallest table in which a wrong group lookup, an off-by-one at a segment edge or a workgroup reading its neighbour's group shows up.
A non-finite VALUE planted in a gradient buffer is ordinary data to these kernels; nothing here provokes a device fault."""
import numpy as np
import pytest
import torch

import adamw_groups_ref as R
import lora_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = torch.device("cuda:0")
SEG = 2048
COUNTS = [1, 2047, 2048, 2049, 4096, 5000, 3]
PADDED = [-(-c // SEG) * SEG for c in COUNTS]
STARTS = [0] + list(np.cumsum(PADDED))
N = STARTS[-1]
GROUP = [0, 1, 2, 0, 1, 2, 0]
ACTIVE = [1, 1, 1, 1, 0, 1, 1]
SEG_STEP = [5, 5, 9, 5, 5, 5, 5]
STEP = 5
LRS, WDS = [2e-4, 5e-3, 1e-5], [1e-3, 0.0, 0.3]
BETAS, EPS, CLIP = (0.9, 0.95), 1e-8, 0.37


def _table():
    return dict(seg_start=torch.tensor(STARTS, dtype=torch.int64, device=DEV), active=torch.tensor(ACTIVE, dtype=torch.uint8, device=DEV),
                seg_group=torch.tensor(GROUP, dtype=torch.uint8, device=DEV), seg_step=torch.tensor(SEG_STEP, dtype=torch.int32, device=DEV),
                clip=torch.tensor([CLIP], dtype=torch.float32, device=DEV))


def _unpadded(x):
    """zero the padding, as the optimizer's buffers have it"""
    for a, c, pad in zip(STARTS, COUNTS, PADDED):
        x[a + c:a + pad] = 0
    return x


def _buffers(seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(p=_unpadded((torch.randn(N, generator=g) * 0.02).to(BF)).to(DEV),
                lo=_unpadded(torch.randint(-32768, 32768, (N,), generator=g, dtype=torch.int64).to(torch.int16)).to(DEV),
                g=_unpadded((torch.randn(N, generator=g) * 0.05).to(BF)).to(DEV),
                m=(torch.randn(N, generator=g) * 0.01).to(DEV), v=((torch.randn(N, generator=g) * 0.01) ** 2).to(DEV))


def _same(a, b):
    """equal in every byte (torch.equal would call a NaN unequal to itself)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def _inactive(x):
    a = STARTS[ACTIVE.index(0)]
    return x[a:a + PADDED[ACTIVE.index(0)]]


def _masked(t, j):
    return t["active"] * (t["seg_group"] == j).to(torch.uint8)


@pytest.mark.parametrize("mode", ["bf16", "split_fp32", "stochastic"])
def test_groups_update_equals_one_parent_launch_per_group(mode):
    from orv_amd import ops
    t, b = _table(), _buffers()
    lo = mode == "split_fp32"
    keys = ("p", "m", "v") + (("lo",) if lo else ())
    new, old = {k: b[k].clone() for k in keys}, {k: b[k].clone() for k in keys}
    ops.adamw_flat_groups(new["p"], b["g"], new["m"], new["v"], t["seg_start"], t["active"], t["seg_group"], LRS, WDS, *BETAS, EPS, STEP,
                          t["clip"], seg_step=t["seg_step"], lo=new.get("lo"), mode=mode, seed=11)
    for j in range(3):
        ops.adamw_flat_ex(old["p"], b["g"], old["m"], old["v"], t["seg_start"], _masked(t, j), LRS[j], *BETAS, EPS, WDS[j], STEP, t["clip"],
                          seg_step=t["seg_step"], lo=old.get("lo"), mode=mode, seed=11)
    torch.cuda.synchronize()
    for k in keys:
        assert _same(new[k], old[k]), (mode, k, int((new[k] != old[k]).sum()))
        assert _same(_inactive(new[k]), _inactive(b[k])), (mode, k)                # the inactive segment keeps every byte
    assert not torch.equal(new["p"], b["p"])
    # one group through the new entry: the bytes of the parent entry
    one, par = {k: b[k].clone() for k in keys}, {k: b[k].clone() for k in keys}
    ops.adamw_flat_groups(one["p"], b["g"], one["m"], one["v"], t["seg_start"], t["active"], torch.zeros_like(t["seg_group"]), LRS[:1], WDS[:1],
                          *BETAS, EPS, STEP, t["clip"], seg_step=t["seg_step"], lo=one.get("lo"), mode=mode, seed=11)
    ops.adamw_flat_ex(par["p"], b["g"], par["m"], par["v"], t["seg_start"], t["active"], LRS[0], *BETAS, EPS, WDS[0], STEP, t["clip"],
                      seg_step=t["seg_step"], lo=par.get("lo"), mode=mode, seed=11)
    torch.cuda.synchronize()
    assert all(_same(one[k], par[k]) for k in keys)


@pytest.mark.parametrize("mode", ["bf16", "split_fp32", "stochastic"])
def test_fp8_groups_update_equals_one_parent_launch_per_group(mode):
    from orv_amd import ops
    t, b = _table(), _buffers(1)
    z8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=DEV)
    b.update(m8=z8(N), v8=z8(N), m_exp=z8(N // 256), v_exp=z8(N // 256))
    ops.state8_quantize(b["m"], b["m8"], b["m_exp"], "m", seed=11, step=STEP - 1)
    ops.state8_quantize(b["v"], b["v8"], b["v_exp"], "v", seed=11, step=STEP - 1)
    lo = mode == "split_fp32"
    keys = ("p", "m8", "v8", "m_exp", "v_exp") + (("lo",) if lo else ())
    state = lambda d: (d["m8"], d["v8"], d["m_exp"], d["v_exp"])
    new, old, one, par = ({k: b[k].clone() for k in keys} for _ in range(4))
    ops.adamw_flat_s8_groups(new["p"], b["g"], *state(new), t["seg_start"], t["active"], t["seg_group"], LRS, WDS, *BETAS, EPS, STEP, t["clip"],
                             seg_step=t["seg_step"], lo=new.get("lo"), mode=mode, seed=11)
    for j in range(3):
        ops.adamw_flat_s8(old["p"], b["g"], *state(old), t["seg_start"], _masked(t, j), LRS[j], *BETAS, EPS, WDS[j], STEP, t["clip"],
                          seg_step=t["seg_step"], lo=old.get("lo"), mode=mode, seed=11)
    ops.adamw_flat_s8_groups(one["p"], b["g"], *state(one), t["seg_start"], t["active"], torch.zeros_like(t["seg_group"]), LRS[:1], WDS[:1],
                             *BETAS, EPS, STEP, t["clip"], seg_step=t["seg_step"], lo=one.get("lo"), mode=mode, seed=11)
    ops.adamw_flat_s8(par["p"], b["g"], *state(par), t["seg_start"], t["active"], LRS[0], *BETAS, EPS, WDS[0], STEP, t["clip"],
                      seg_step=t["seg_step"], lo=par.get("lo"), mode=mode, seed=11)
    # common_count only says for which count the host's bias corrections hold (segment 2 is at 9, the rest at 5): it never shows in the bytes
    for count in (9, 3):
        hint = {k: b[k].clone() for k in keys}
        ops.adamw_flat_s8_groups(hint["p"], b["g"], *state(hint), t["seg_start"], t["active"], t["seg_group"], LRS, WDS, *BETAS, EPS, STEP,
                                 t["clip"], seg_step=t["seg_step"], lo=hint.get("lo"), mode=mode, seed=11, common_count=count)
        assert all(_same(hint[k], new[k]) for k in keys), (mode, count)
    torch.cuda.synchronize()
    for k in keys:
        assert _same(new[k], old[k]), (mode, k, int((new[k] != old[k]).sum()))
        if k in ("m_exp", "v_exp"):
            a = STARTS[ACTIVE.index(0)] // 256
            assert torch.equal(new[k][a:a + PADDED[ACTIVE.index(0)] // 256], b[k][a:a + PADDED[ACTIVE.index(0)] // 256])
        else:
            assert _same(_inactive(new[k]), _inactive(b[k])), (mode, k)
        assert _same(one[k], par[k]), (mode, k)
    assert not torch.equal(new["p"], b["p"])


def test_entries_refuse_bad_arguments_before_launching():
    from orv_amd import ops
    t, b = _table(), _buffers()
    args = lambda grp, lrs, wds: (b["p"], b["g"], b["m"], b["v"], t["seg_start"], t["active"], grp, lrs, wds, *BETAS, EPS, STEP, t["clip"])
    with pytest.raises(RuntimeError, match=r"names group 2, the table holds 2"):
        ops.adamw_flat_groups(*args(t["seg_group"], LRS[:2], WDS[:2]))
    with pytest.raises(RuntimeError, match=r"supported: 1\.\.8"):
        ops.adamw_flat_groups(*args(t["seg_group"], [1e-4] * 9, [0.0] * 9))
    with pytest.raises(RuntimeError, match=r"multiple of 2048"):
        ops.adamw_flat_groups(b["p"][:N - 8], b["g"], b["m"][:N - 8], b["v"][:N - 8], t["seg_start"], t["active"], t["seg_group"], LRS, WDS,
                              *BETAS, EPS, STEP, t["clip"])
    from orv_amd._lib import AdamwGroups, lib
    tab = AdamwGroups()
    tab.ngroups = 9
    assert lib().orv_adamw_flat_groups(b["p"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), N, t["seg_start"].data_ptr(),
                                       t["active"].data_ptr(), None, 7, t["seg_group"].data_ptr(), tab, 0.9, 0.95, 1e-8, 1, None, None, 0, 0,
                                       None) != 0
    assert b"ngroups=9" in lib().orv_last_error()
    assert lib().orv_segment_sumsq(None, t["seg_start"].data_ptr(), 7, None, None) != 0 and b"null buffer" in lib().orv_last_error()
    assert lib().orv_step_guard(None, None, 7, 1.0, 1.0, 0, None, None, None, None) != 0 and b"null buffer" in lib().orv_last_error()
    torch.cuda.synchronize()


# ---- the two reductions ----
def _gradient(seed=2):
    """random bf16 data of mixed scale, bf16 denormals, and one segment of zeros"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(N, generator=gen) * torch.tensor([1e-3, 1.0, 30.0])[torch.randint(0, 3, (N,), generator=gen)]
    g = g.to(BF)
    den = torch.randint(1, 0x80, (64,), generator=gen, dtype=torch.int32).to(torch.int16).view(BF)          # subnormal bf16 patterns
    g[torch.randint(0, N, (64,), generator=gen)] = den
    g[STARTS[5] + 4990:STARTS[5] + 5000] = den[:10]                                                          # ... and in a cut-short round
    g = _unpadded(g)
    g[STARTS[2]:STARTS[3]] = 0
    return g


def _sumsq(g):
    from orv_amd import ops
    out = torch.full((7,), -1.0, dtype=torch.float64, device=DEV)
    ops.segment_sumsq(g.to(DEV), torch.tensor(STARTS, dtype=torch.int64, device=DEV), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_segment_sumsq_equals_the_restatement_bit_for_bit():
    g = _gradient()
    want = R.segment_sumsq(g.double().numpy(), STARTS)
    got = _sumsq(g)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    assert got[2] == 0.0 and np.all(got[[0, 1, 3, 4, 5, 6]] > 0)
    assert np.array_equal(_sumsq(g).view(np.uint64), got.view(np.uint64))                  # two runs: identical bits
    for bad in (float("inf"), float("nan")):
        h = g.clone()
        h[STARTS[3] + 2048] = bad                                                         # the one element beyond the first 2048 of segment 3
        out = _sumsq(h)
        assert not np.isfinite(out[3])
        assert np.array_equal(np.delete(out, 3).view(np.uint64), np.delete(got, 3).view(np.uint64))


@pytest.mark.parametrize("case", ["clean", "clean_world4", "unclipped", "no_clipping", "nan_skip", "nan_keep", "inf_skip", "inf_keep"])
def test_step_guard_equals_the_restatement(case):
    from orv_amd import ops
    ss = R.segment_sumsq(_gradient().double().numpy(), STARTS)
    if case == "unclipped":
        ss = ss * 1e-12
    if case.startswith(("nan", "inf")):
        ss[4] = float(case[:3])
    max_norm = 0.0 if case == "no_clipping" else 1.0
    inv_world = 0.25 if case == "clean_world4" else 1.0
    skip = case.endswith("skip")
    active = np.array(ACTIVE, dtype=np.uint8)
    want_clip, want_active, want_rep = R.step_guard(ss, GROUP, active, max_norm, inv_world, skip, skip_count=3.0)
    t = _table()
    clip = torch.full((1,), -7.0, dtype=torch.float32, device=DEV)
    rep = torch.zeros(R.REPORT, dtype=torch.float64, device=DEV)
    rep[9] = 3.0
    ops.step_guard(torch.tensor(ss, device=DEV), t["seg_group"], t["active"], clip, rep, max_norm, inv_world, skip)
    torch.cuda.synchronize()
    got_clip, got_rep = clip.cpu().numpy(), rep.cpu().numpy()
    # NaN carries no agreed payload between the two machines: a NaN must be a NaN, everything else is compared in its bits
    same = lambda a, b, bits: np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(bits), b[~np.isnan(b)].view(bits))
    assert same(got_clip, np.array([want_clip], dtype=np.float32), np.uint32), (got_clip, want_clip)
    assert same(got_rep, want_rep, np.uint64), (got_rep, want_rep)
    assert np.array_equal(t["active"].cpu().numpy(), want_active)
    assert bool(got_rep[10]) == (skip and case[:3] in ("nan", "inf")) and got_rep[9] == 3.0 + got_rep[10]


# ---- FusedAdamW end to end ----
SHAPES = [(7,), (33, 65), (2049,), (5, 1000)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(DEV, BF)) for s in SHAPES]


def _grads(step, scale=0.3):
    g = torch.Generator().manual_seed(1000 + step)
    return [(torch.randn(s, generator=g) * scale).to(DEV, BF) for s in SHAPES]


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g.clone()


TWO = dict(lr=(3e-3, 2e-4), wd=(0.0, 0.1))


def _two_groups(ps, **kw):
    from orv_amd.optim import FusedAdamW
    return FusedAdamW([{"params": ps[:2], "lr": TWO["lr"][0], "weight_decay": TWO["wd"][0], "name": "new"},
                       {"params": ps[2:], "lr": TWO["lr"][1], "weight_decay": TWO["wd"][1], "name": "backbone"}], betas=BETAS, **kw)


def _bytes(opt):
    f = opt._flat
    keys = [k for k in ("p", "lo", "m", "v", "m8", "v8", "m_exp", "v_exp", "seg_step") if k in f]
    return {k: f[k].clone() for k in keys}


@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_two_groups_equal_two_single_group_optimizers_without_clipping(precision):
    from orv_amd.optim import FusedAdamW
    ps, qs = _params(), _params()
    opt = _two_groups(ps, max_grad_norm=0, param_precision=precision)
    halves = [FusedAdamW(qs[:2], lr=TWO["lr"][0], weight_decay=TWO["wd"][0], betas=BETAS, max_grad_norm=0, param_precision=precision),
              FusedAdamW(qs[2:], lr=TWO["lr"][1], weight_decay=TWO["wd"][1], betas=BETAS, max_grad_norm=0, param_precision=precision)]
    for step in range(3):
        grads = _grads(step)
        _set_grads(ps, grads), _set_grads(qs, grads)
        norm = opt.step()
        parts = [h.step() for h in halves]
        assert norm == pytest.approx((parts[0] ** 2 + parts[1] ** 2) ** 0.5, rel=1e-5)
    torch.cuda.synchronize()
    masters = lambda o: o.master_params()
    for i, (p, q) in enumerate(zip(ps, qs)):
        assert torch.equal(p.data, q.data), i
    both = masters(halves[0]) + masters(halves[1])
    assert all(torch.equal(a, b) for a, b in zip(masters(opt), both))
    for which in (0, 1):
        got, want = opt.moments(), [a + b for a, b in zip(halves[0].moments(), halves[1].moments())]
        assert all(torch.equal(a, b) for a, b in zip(got[which], want[which]))


def test_with_clipping_the_step_follows_the_restated_global_norm():
    """One optimizer step with two groups and clipping on = the parent kernel launched per group with the clip coefficient that the
    restatement of the two reductions derives from the same gradients; the returned norm is that restatement's."""
    from orv_amd import ops
    ps = _params()
    opt = _two_groups(ps, max_grad_norm=1.0, track_grad_norms=True)
    for step in range(2):
        _set_grads(ps, _grads(step, scale=0.5))
        if step == 0:
            opt.step()
            continue
        before = _bytes(opt)
        norm = opt.step()
        torch.cuda.synchronize()
        f = opt._flat
        starts = f["seg_start"].tolist()
        ss = R.segment_sumsq(f["g"][:starts[-1]].double().cpu().numpy(), starts)
        clip, _, rep = R.step_guard(ss, [0, 0, 1, 1], [1, 1, 1, 1], 1.0)
        assert clip < 1.0 and norm == float(np.sqrt(rep[0]))
        clip_d = torch.tensor([clip], dtype=torch.float32, device=DEV)
        for j in range(2):
            mask = torch.tensor([1, 1, 0, 0] if j == 0 else [0, 0, 1, 1], dtype=torch.uint8, device=DEV)
            ops.adamw_flat_ex(before["p"], f["g"], before["m"], before["v"], f["seg_start"], mask, TWO["lr"][j], *BETAS, 1e-8, TWO["wd"][j], 2,
                              clip_d, seg_step=f["seg_step"], mode=0)
        torch.cuda.synchronize()
        assert all(_same(before[k], f[k]) for k in ("p", "m", "v"))
        norms = opt.grad_norms()
        assert norms["global"] == norm and set(norms["groups"]) == {"new", "backbone"}
        assert norms["groups"]["new"] == float(np.sqrt(rep[1])) and norms["groups"]["backbone"] == float(np.sqrt(rep[2]))


def test_grad_norms_per_parameter():
    ps = _params()
    opt = _two_groups(ps, max_grad_norm=1.0)
    grads = _grads(5, scale=2.0)
    _set_grads(ps, grads)
    total = opt.step()
    norms = opt.grad_norms()
    want = [float(g.double().norm()) for g in grads]                 # the fp64 norm of the same bf16 values
    got = norms["params"].cpu().tolist()
    assert len(got) == len(ps)
    for a, b in zip(got, want):
        assert abs(a - b) <= 2.0 ** -20 * b, (a, b)
    assert abs(total - sum(w * w for w in want) ** 0.5) <= 2.0 ** -20 * total and norms["global"] == total
    assert abs(norms["groups"]["new"] - (want[0] ** 2 + want[1] ** 2) ** 0.5) <= 2.0 ** -20 * norms["groups"]["new"]


@pytest.mark.parametrize("precision,state", [("split_fp32", "fp32"), ("stochastic", "fp8")])
def test_skip_guard_keeps_every_byte_and_its_absence_poisons_the_weights(precision, state):
    ps, qs = _params(), _params()
    opt = _two_groups(ps, max_grad_norm=1.0, param_precision=precision, state_precision=state, skip_nonfinite=True)
    bare = _two_groups(qs, max_grad_norm=1.0, param_precision=precision, state_precision=state)
    grads = _grads(0)
    _set_grads(ps, grads), _set_grads(qs, grads)
    assert opt.step() == bare.step() and opt.skipped_steps == 0 and not opt.last_step_skipped
    before = _bytes(opt)
    bad = _grads(1)
    bad[2][1234] = float("nan")
    _set_grads(ps, bad), _set_grads(qs, bad)
    norm = opt.step()
    torch.cuda.synchronize()
    assert norm != norm and opt.skipped_steps == 1 and opt.last_step_skipped and opt.step_count == 2
    after = _bytes(opt)
    assert set(after) == set(before) and all(_same(after[k], before[k]) for k in before), [k for k in before if not _same(after[k], before[k])]
    assert all(torch.isfinite(p).all() for p in ps)
    bare.step()                                                      # the same step without the guard: what the guard buys
    torch.cuda.synchronize()
    assert all(torch.isnan(q).all() for q in qs)
    # the next clean step runs, counts for every parameter, and the counter stays
    _set_grads(ps, _grads(2))
    assert opt.step() > 0 and opt.skipped_steps == 1 and not opt.last_step_skipped
    assert opt._flat["seg_step"].tolist() == [2, 2, 2, 2] and not torch.equal(opt._flat["p"], before["p"])
    # an infinite gradient is skipped as well
    bad = _grads(3)
    bad[0][3] = float("inf")
    _set_grads(ps, bad)
    assert opt.step() == float("inf") and opt.skipped_steps == 2 and opt._flat["seg_step"].tolist() == [2, 2, 2, 2]


def test_state_dict_round_trip_with_groups():
    from orv_amd.optim import FusedAdamW
    ps = _params()
    kw = dict(max_grad_norm=1.0, param_precision="split_fp32", skip_nonfinite=True)
    opt = _two_groups(ps, **kw)
    for step in range(2):
        _set_grads(ps, _grads(step))
        opt.step()
    bad = _grads(7)
    bad[1][0, 0] = float("nan")
    _set_grads(ps, bad)
    opt.step()                                                       # one skipped step: the counter travels
    opt.param_groups[1]["lr"] = 1e-4                                 # a schedule has moved a rate
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    assert sd["skipped_steps"] == 1 and [g["params"] for g in sd["groups"]] == [[0, 1], [2, 3]]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    new = _two_groups(qs, **kw)
    new.load_state_dict(sd)
    assert new.skipped_steps == 1 and new.param_groups[1]["lr"] == 1e-4 and new.step_count == 3
    for step in range(2, 4):
        grads = _grads(step)
        _set_grads(ps, grads), _set_grads(qs, grads)
        assert opt.step() == new.step()
    torch.cuda.synchronize()
    a, b = _bytes(opt), _bytes(new)
    assert all(_same(a[k], b[k]) for k in a) and new.skipped_steps == opt.skipped_steps == 1
    # a state dict with the key set of a checkpoint written before groups existed still loads (one group over everything)
    total = opt._flat["p"].numel()
    old = {"step": 4, "exp_avg": torch.full((total,), 0.5, device=DEV), "exp_avg_sq": torch.full((total,), 0.25, device=DEV),
           "numels": [int(p.numel()) for p in ps], "seg_start": opt._flat["seg_start"].tolist(),
           "seg_step": torch.tensor([4, 4, 3, 4], dtype=torch.int32, device=DEV), "param_precision": "bf16", "state_precision": "fp32", "seed": 0}
    for extra in ({}, {"skip_nonfinite": True}):
        rs = _params()
        plain = FusedAdamW(rs, **extra)
        plain.load_state_dict(old)
        assert plain.step_count == 4 and plain.skipped_steps == 0 and plain._flat["seg_step"].tolist() == [4, 4, 3, 4]
        assert float(plain._flat["m"][0]) == 0.5 and float(plain._flat["v"][0]) == 0.25
    with pytest.raises(ValueError, match=r"checkpoint holds 1 parameter group\(s\) of \[4\] parameters, this optimizer 2 of \[2, 2\]"):
        _two_groups(_params()).load_state_dict(old)
    rs = _params()
    with pytest.raises(ValueError, match=r"another partition"):
        FusedAdamW([{"params": rs[:1]}, {"params": rs[1:]}]).load_state_dict(sd)


def test_sft_step_reports_a_skipped_step_and_leaves_ema_and_schedule_alone():
    from conftest import load_golden
    from orv_amd import FusedEMA, schedulers, sft
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    from orv_amd.optim import get_optimizer, get_scheduler, named_groups
    cfg, extra, ins, w, _ = load_golden("fwd_actions")
    sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                              beta_schedule="scaled_linear", prediction_type="v_prediction",
                                              rescale_betas_zero_snr=True, snr_shift_scale=3.0, timestep_spacing="trailing")
    x0 = torch.randn(2, 3, 16, 8, 12, generator=torch.Generator().manual_seed(9)).to(DEV, BF)
    mk = lambda x: sft.Batch(x, torch.zeros_like(x), ins["encoder_hidden_states"].to(DEV, BF), ins["actions"].to(DEV), None, None,
                             torch.ones(3, dtype=torch.bool, device=DEV), 1)
    m = lora_ref.build_model(CogVideoXTransformer3DModelTraj, cfg, extra, ins, w, DEV).train()
    m.action_embed.forced_mask = torch.zeros(2, dtype=torch.bool)
    groups = named_groups(m, weight_decay=1e-3, lr_overrides={"action_embed": 5e-4})
    assert {"decay", "no_decay", "action_embed"} <= {g["name"] for g in groups}
    opt = get_optimizer(groups, "adamw", learning_rate=2e-4, beta2=0.95, weight_decay=1e-3, skip_nonfinite=True)
    ema = FusedEMA(opt)
    lrs = get_scheduler("constant_with_warmup", opt, num_warmup_steps=4)
    gen = lambda s: torch.Generator(device=DEV).manual_seed(100 + s)
    loss, parts = sft.sft_step(m, sched, opt, mk(x0), generator=gen(1), lr_scheduler=lrs, ema=ema)
    torch.cuda.synchronize()
    assert parts["skipped"] is False and parts["grad_norm"] > 0 and ema.optimization_step == 1 and lrs.last_epoch == 1
    assert parts["lr"] == lrs.get_last_lr()[0] and len(lrs.get_last_lr()) == len(groups)
    before, shadow, rates = _bytes(opt), ema.shadow.clone(), lrs.get_last_lr()
    poisoned = x0.clone()
    poisoned[0, 0, 0, 0, 0] = float("nan")
    loss, parts = sft.sft_step(m, sched, opt, mk(poisoned), generator=gen(2), lr_scheduler=lrs, ema=ema)
    torch.cuda.synchronize()
    assert parts["skipped"] is True and parts["grad_norm"] != parts["grad_norm"] and opt.skipped_steps == 1
    after = _bytes(opt)
    assert all(_same(after[k], before[k]) for k in before)
    assert torch.equal(ema.shadow, shadow) and ema.optimization_step == 1 and lrs.last_epoch == 1 and lrs.get_last_lr() == rates
    loss, parts = sft.sft_step(m, sched, opt, mk(x0), generator=gen(3), lr_scheduler=lrs, ema=ema)
    torch.cuda.synchronize()
    assert parts["skipped"] is False and torch.isfinite(loss) and ema.optimization_step == 2 and lrs.last_epoch == 2
    assert not torch.equal(opt._flat["p"], before["p"]) and all(torch.isfinite(p).all() for p in opt.params)
