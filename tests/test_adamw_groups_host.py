"""Host side of FusedAdamW's parameter groups, gradient norms and skip guard: the construction surface, ``named_groups``,
the refusals, the schedule over several groups, and the numpy restatement of the two device reductions (tests/adamw_groups_ref.py) against
exact sums.  No GPU: the optimizers build their flat buffers on first use only."""
import math

import numpy as np
import pytest
import torch

import adamw_groups_ref as R
import orv_amd
from orv_amd.optim import FusedAdamW, FusedCAME, FusedProdigy, LambdaSchedule, get_optimizer, get_scheduler, named_groups


def _params(n=4):
    return [torch.nn.Parameter(torch.zeros(3 + i, 5)) for i in range(n)]


# ---- construction ----
def test_get_optimizer_takes_two_groups_for_adamw():
    ps = _params()
    opt = get_optimizer([{"params": ps[:1], "lr": 5e-4, "weight_decay": 0.0, "name": "new"}, {"params": ps[1:]}], "adamw", learning_rate=2e-4,
                        weight_decay=1e-3)
    assert type(opt) is FusedAdamW and len(opt.param_groups) == 2
    a, b = opt.param_groups
    assert (a["lr"], a["initial_lr"], a["weight_decay"], a["name"], len(a["params"])) == (5e-4, 5e-4, 0.0, "new", 1)
    assert (b["lr"], b["initial_lr"], b["weight_decay"], b["name"], len(b["params"])) == (2e-4, 2e-4, 1e-3, "group1", 3)
    assert opt.lr == 5e-4 and opt.weight_decay == 0.0                # group 0, for existing callers
    assert [id(p) for p in opt.params] == [id(p) for p in ps]       # groups do not reorder storage
    # fp8 moments take groups as well; adam coincides with adamw where nothing is decayed
    assert get_optimizer([{"params": ps[:2], "name": "a"}, {"params": ps[2:]}], "adamw", use_8bit=True).state_precision == "fp8"
    # dicts that carry nothing but params would all run at the same two numbers: the factory says that this is one group
    with pytest.raises(ValueError, match=r"carry nothing but `params` are one group.*own lr / weight_decay / name"):
        get_optimizer([{"params": ps[:2]}, {"params": ps[2:]}], "adamw")
    assert len(get_optimizer([{"params": ps[:2], "weight_decay": 0.0}, {"params": ps[2:], "weight_decay": 0.0}], "adam").param_groups) == 2
    with pytest.raises(ValueError, match=r"coupled weight decay.*adamw"):
        get_optimizer([{"params": ps[:2]}, {"params": ps[2:], "weight_decay": 0.0}], "adam", weight_decay=1e-2)


def test_one_group_without_a_dict_keeps_the_one_scalar_path():
    ps = _params()
    opt = FusedAdamW(ps, lr=3e-4, weight_decay=1e-2)
    assert not opt._guarded and len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert (g["lr"], g["initial_lr"], g["weight_decay"], len(g["params"])) == (3e-4, 3e-4, 1e-2, 4)
    assert FusedAdamW(ps, skip_nonfinite=True)._guarded and FusedAdamW(ps, track_grad_norms=True)._guarded
    assert FusedAdamW([{"params": ps}])._guarded                     # given as a dict: the groups path
    opt.weight_decay = 0.5                                           # optimizer.lr / .weight_decay are group 0
    opt.lr = 0.25
    assert (g["lr"], g["weight_decay"]) == (0.25, 0.5)
    with pytest.raises(RuntimeError, match="track_grad_norms=True"):
        opt.grad_norms()


class _Attn(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.to_q, self.to_out = torch.nn.Linear(d, d), torch.nn.Linear(d, d)
        self.norm_q, self.norm_k = torch.nn.LayerNorm(d // 2), torch.nn.LayerNorm(d // 2)      # qk-norm vectors


class _Block(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.norm1, self.attn1, self.ff = torch.nn.LayerNorm(d), _Attn(d), torch.nn.Linear(d, 2 * d)


class _Toy(torch.nn.Module):
    def __init__(self, d=8):
        super().__init__()
        self.transformer_blocks = torch.nn.ModuleList([_Block(d), _Block(d)])
        self.action_embed = torch.nn.Linear(3, d)
        self.initial_combine_linear = torch.nn.Linear(d, d)
        self.frozen = torch.nn.Linear(d, d).requires_grad_(False)


def test_named_groups_decay_split_overrides_and_coverage():
    model = _Toy()
    named = dict(model.named_parameters())
    groups = named_groups(model, weight_decay=1e-3, lr_overrides={"action_embed": 5e-4, "initial_combine_linear": 7e-4})
    by = {g["name"]: g for g in groups}
    assert list(by) == ["decay", "no_decay", "action_embed", "action_embed.no_decay", "initial_combine_linear", "initial_combine_linear.no_decay"]
    where = {id(p): g["name"] for g in groups for p in g["params"]}
    trainable = {n: p for n, p in named.items() if p.requires_grad}
    assert sum(len(g["params"]) for g in groups) == len(where) == len(trainable)          # each exactly once
    assert set(where) == {id(p) for p in trainable.values()}                               # and nothing frozen
    for n, p in trainable.items():
        plain = "bias" in n or "norm" in n
        assert where[id(p)].endswith("no_decay") == plain, n                               # every bias, LayerNorm and qk-norm vector
        assert where[id(p)].startswith("action_embed") == n.startswith("action_embed"), n
    assert by["decay"]["weight_decay"] == 1e-3 and by["no_decay"]["weight_decay"] == 0.0 and "lr" not in by["decay"]
    assert by["action_embed"]["lr"] == by["action_embed.no_decay"]["lr"] == 5e-4 and by["initial_combine_linear"]["lr"] == 7e-4
    assert by["action_embed"]["weight_decay"] == 1e-3 and by["action_embed.no_decay"]["weight_decay"] == 0.0
    # a name pattern takes a matrix out of the decay as well; lr= sets the rate of everything without an override
    g2 = {g["name"]: g for g in named_groups(model, weight_decay=0.1, no_decay=("bias", "norm", "to_out"), lr=1e-5)}
    assert any(p is model.transformer_blocks[0].attn1.to_out.weight for p in g2["no_decay"]["params"]) and g2["decay"]["lr"] == 1e-5
    opt = get_optimizer(groups, "adamw", learning_rate=2e-4)
    assert [g["lr"] for g in opt.param_groups] == [2e-4, 2e-4, 5e-4, 5e-4, 7e-4, 7e-4]
    assert orv_amd.named_groups is named_groups


def test_refusals_name_the_supported_set():
    ps = _params(10)
    with pytest.raises(ValueError, match=r"9 parameter groups \(supported: 1\.\.8"):
        FusedAdamW([{"params": [p]} for p in ps[:9]])
    with pytest.raises(ValueError, match=r"in two groups.*supported: every parameter in exactly one group"):
        FusedAdamW([{"params": ps[:2]}, {"params": ps[1:3]}])
    with pytest.raises(ValueError, match=r"group 1 \('empty'\) is empty \(supported: at least one trainable parameter"):
        FusedAdamW([{"params": ps[:2]}, {"params": [], "name": "empty"}])
    with pytest.raises(ValueError, match=r"group 0 carries betas; a group may carry params, lr, weight_decay, name.*betas, eps.*are global"):
        FusedAdamW([{"params": ps[:2], "betas": (0.9, 0.99)}, {"params": ps[2:]}])
    two = [{"params": ps[:2]}, {"params": ps[2:]}]
    with pytest.raises(ValueError, match=r"FusedProdigy: 2 parameter groups.*FusedAdamW is the class that has parameter groups.*supported here: one group"):
        FusedProdigy(two)
    with pytest.raises(ValueError, match=r"FusedCAME: 2 parameter groups.*FusedAdamW is the class that has parameter groups.*supported here: one group"):
        FusedCAME(two, lr=1e-4)
    with pytest.raises(ValueError, match=r"2 parameter groups; FusedProdigy keeps one group.*adam / adamw.*supported"):
        get_optimizer(two, "prodigy", learning_rate=1.0)
    assert len(FusedProdigy([{"params": ps}]).params) == 10          # one dict is one group


def test_state_dict_carries_the_groups_and_refuses_another_partition():
    ps = _params()
    mk = lambda cut: FusedAdamW([{"params": ps[:cut], "lr": 1e-3, "name": "a"}, {"params": ps[cut:], "weight_decay": 0.0, "name": "b"}])
    sd = mk(1).state_dict()
    assert [g["params"] for g in sd["groups"]] == [[0], [1, 2, 3]] and sd["skipped_steps"] == 0
    assert [(g["name"], g["lr"], g["weight_decay"]) for g in sd["groups"]] == [("a", 1e-3, 1e-3), ("b", 1e-4, 0.0)]
    sd["groups"][0]["lr"], sd["skipped_steps"] = 0.5, 3
    other = mk(1)
    other.load_state_dict(sd)
    assert other.param_groups[0]["lr"] == 0.5 and other.skipped_steps == 3
    with pytest.raises(ValueError, match=r"checkpoint holds 2 parameter group\(s\) of \[1, 3\] parameters, this optimizer 2 of \[2, 2\]"):
        mk(2).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"checkpoint holds 1 parameter group"):
        mk(1).load_state_dict(FusedAdamW(ps).state_dict())           # a checkpoint without groups is one group over everything
    assert "groups" not in FusedAdamW(ps).state_dict()               # the one-scalar path writes what it always wrote


# ---- schedules ----
def test_lambda_schedule_scales_every_group_from_its_own_initial_lr():
    lam = lambda s: 1.0 / (1 + s)
    opt = FusedAdamW([{"params": _params(2), "lr": 1e-3}, {"params": _params(2), "lr": 4e-5}])
    sched = LambdaSchedule(opt, lam)
    for step in range(5):
        assert sched.get_last_lr() == [1e-3 * lam(step), 4e-5 * lam(step)] == [g["lr"] for g in opt.param_groups]
        assert [g["initial_lr"] for g in opt.param_groups] == [1e-3, 4e-5]
        sched.step()
    # one group: the hand-derived known answers of tests/test_lr_schedule.py (warm-up 4, T = 20, two cycles: ramp 0, 1/4, ..., then
    # 0.5 (1 + cos(pi ((2 prog) mod 1))), prog = (s - 4) / 16), through a FusedAdamW built without groups; a second group follows the same
    # multipliers from its own initial_lr
    one = FusedAdamW(_params(2), lr=2e-4)
    two = FusedAdamW([{"params": _params(2), "lr": 2e-4}, {"params": _params(2), "lr": 1e-5}])
    s1 = get_scheduler("cosine_with_restarts", one, num_warmup_steps=4, num_training_steps=20, num_cycles=2)
    s2 = get_scheduler("cosine_with_restarts", two, num_warmup_steps=4, num_training_steps=20, num_cycles=2)
    lr, lr2 = [], []
    for _ in range(23):
        assert s1.get_last_lr() == [one.param_groups[0]["lr"]] == [one.lr] and s2.get_last_lr() == [g["lr"] for g in two.param_groups]
        lr.append(s1.get_last_lr()[0]), lr2.append(s2.get_last_lr())
        s1.step(), s2.step()
    known = {0: 0.0, 2: 1e-4, 4: 2e-4, 6: 2e-4 * 0.5 * (1 + math.cos(math.pi / 4)), 8: 1e-4, 12: 2e-4, 16: 1e-4, 20: 0.0, 22: 0.0}
    for s, want in known.items():
        assert lr[s] == pytest.approx(want), s
        assert lr2[s][0] == lr[s] and lr2[s][1] == pytest.approx(want / 20), s
    assert lr[0] == 0.0 and lr[20] == 0.0 and lr[22] == 0.0


# ---- the restatement of the two reductions ----
def _bf16_values(rng, n, scale):
    return torch.tensor(rng.standard_normal(n) * scale, dtype=torch.float32).bfloat16().double().numpy()


@pytest.mark.parametrize("n", [1, 3, 2047, 2048, 2049, 4096, 5000, 8192 + 9, 20000])
def test_segment_sum_in_the_stated_order_is_within_one_ulp_of_the_exact_sum(n):
    rng = np.random.default_rng(n)
    for scale in (1e-3, 1.0, 30.0):
        x = _bf16_values(rng, n, scale)
        got, exact = R.segment_sumsq_one(x), math.fsum((x * x).tolist())          # x * x is exact in fp64
        assert abs(got - exact) <= math.ulp(exact), (n, scale, got, exact)
    assert R.segment_sumsq_one(np.zeros(n)) == 0.0


def test_segment_sums_keep_a_nonfinite_value_inside_its_segment():
    rng = np.random.default_rng(7)
    counts = [1, 2047, 2048, 2049, 4096, 5000, 3]
    starts = np.cumsum([0] + [-(-c // 2048) * 2048 for c in counts])
    g = np.zeros(starts[-1])
    for a, c in zip(starts, counts):
        g[a:a + c] = _bf16_values(rng, c, 1.0)
    clean = R.segment_sumsq(g, starts)
    for bad in (np.inf, -np.inf, np.nan):
        h = g.copy()
        h[starts[3] + 77] = bad
        out = R.segment_sumsq(h, starts)
        assert not np.isfinite(out[3]) and np.array_equal(np.delete(out, 3), np.delete(clean, 3))


def test_guard_sums_in_index_order_clips_and_skips():
    rng = np.random.default_rng(3)
    ss = rng.random(7) * 10
    grp = np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.uint8)
    act = np.array([1, 1, 1, 1, 0, 1, 1], dtype=np.uint8)
    clip, active, rep = R.step_guard(ss, grp, act, 1.0, 0.5, True, skip_count=2.0)
    total = math.fsum(ss.tolist())
    assert abs(rep[0] - total) <= math.ulp(total) and rep[9] == 2.0 and rep[10] == 0.0 and np.array_equal(active, act)
    for j in range(3):
        exact = math.fsum(ss[grp == j].tolist())
        assert abs(rep[1 + j] - exact) <= math.ulp(exact), j
    assert np.all(rep[4:9] == 0.0)
    want = min(1.0, 1.0 / (math.sqrt(rep[0]) * 0.5 + 1e-6)) * 0.5
    assert clip.dtype == np.float32 and clip == np.float32(want)
    assert R.step_guard(ss * 1e-6, grp, act, 1.0)[0] == np.float32(1.0)          # below the threshold: no clipping
    assert R.step_guard(ss, grp, act, 0.0, 0.25)[0] == np.float32(0.25)          # max_grad_norm 0: no clipping, 1 / world only
    bad = ss.copy()
    bad[4] = np.nan
    clip, active, rep = R.step_guard(bad, grp, act, 1.0, 1.0, True, skip_count=2.0)
    assert clip == 0.0 and not active.any() and rep[9] == 3.0 and rep[10] == 1.0
    assert np.isnan(rep[0]) and np.isnan(rep[2]) and np.isfinite(rep[1]) and np.isfinite(rep[3])      # group 1 holds it, 0 and 2 do not
    clip, active, rep = R.step_guard(bad, grp, act, 1.0, 1.0, False, skip_count=2.0)
    assert np.isnan(clip) and np.array_equal(active, act) and rep[9] == 2.0 and rep[10] == 0.0         # guard off: the NaN goes through
    bad[4] = np.inf
    assert R.step_guard(bad, grp, act, 1.0, 1.0, False)[0] == 0.0                                     # an infinite norm clips to 0
