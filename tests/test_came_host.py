"""CPU: the CAME rule (tests/came_ref.py) against its two closed forms, the shapes of its state, the all-zero gradient, and the host logic of
``orv_amd.optim.FusedCAME`` (constructor refusals, storage, checkpoints) over a CPU stand-in for the one kernel entry point it calls."""
import math

import pytest
import torch

import came_ref as R

BF = torch.bfloat16
BETAS = [R.DEFAULTS["betas"], R.REFERENCE_BETAS]
SHAPES = [(3, 5), (1, 7), (7, 1), (5, 3, 2, 2), (9,), ()]


# ---- the rule ----
@pytest.mark.parametrize("clip_threshold", [1.0, 0.5])
@pytest.mark.parametrize("betas", BETAS)
def test_rank_one_gradient_moves_every_weight_by_the_closed_form(betas, clip_threshold):
    """g_ij = a_i b_j from zero state: u = sign(g) / sqrt(1-b2), k = 1 / (sqrt(1-b2) clip_threshold), and every weight moves by
    lr (1-b1) / (b1 sqrt(1-b3)), independent of b2 and clip_threshold (0.11111 at the defaults with lr = 1e-2)."""
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(37, generator=gen, dtype=torch.float64).abs() + 0.1
    b = (torch.randn(53, generator=gen, dtype=torch.float64).abs() + 0.1) * torch.where(torch.rand(53, generator=gen) < 0.5, -1.0, 1.0)
    g = a[:, None] * b[None, :] * 1e-2
    w = torch.randn(37, 53, generator=gen, dtype=torch.float64) * 0.02
    st = R.new_state(w.shape)
    w2, k, rms = R.param_step(w, g, st, torch.float64, 1e-2, betas=betas, clip_threshold=clip_threshold)
    b1, b2, b3 = (R.f32(x) for x in betas)
    want = R.rank_one_step(1e-2, betas)
    assert float(((w2 - w) + want * g.sign()).abs().max()) <= 1e-12 * want
    assert abs(float(rms) - 1 / math.sqrt(1 - b2)) <= 1e-12 / math.sqrt(1 - b2)
    assert abs(float(k) - 1 / (math.sqrt(1 - b2) * clip_threshold)) <= 1e-12 * float(k)
    if betas == R.DEFAULTS["betas"]:
        assert abs(want - 0.11111) < 1e-4           # 0.11111 lr / 1e-2; the fp32 rounding of b3 = 0.9999 moves the fifth digit


@pytest.mark.parametrize("clip_threshold", [1.0, 0.5])
@pytest.mark.parametrize("betas", BETAS)
def test_unfactored_parameter_moves_by_the_closed_form(betas, clip_threshold):
    gen = torch.Generator().manual_seed(2)
    g = torch.randn(2049, generator=gen, dtype=torch.float64) * 0.05
    g = torch.where(g.abs() < 1e-4, torch.full_like(g, 1e-3), g)
    w = torch.randn(2049, generator=gen, dtype=torch.float64) * 0.02
    w2, k, _ = R.param_step(w, g, R.new_state(w.shape), torch.float64, 1e-2, betas=betas, clip_threshold=clip_threshold)
    want = R.unfactored_step(1e-2, betas, clip_threshold)
    assert float(((w2 - w) + want * g.sign()).abs().max()) <= 1e-12 * want
    assert float(k) > 1


@pytest.mark.parametrize("shape", SHAPES)
def test_state_shapes(shape):
    st = R.new_state(shape)
    assert st["exp_avg"].shape == torch.Size(shape)
    if len(shape) >= 2:
        assert set(st) == {"exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row", "exp_avg_res_col"}
        assert st["exp_avg_sq_row"].shape == st["exp_avg_res_row"].shape == torch.Size(shape[:-1])
        assert st["exp_avg_sq_col"].shape == st["exp_avg_res_col"].shape == torch.Size(shape[:-2] + shape[-1:])
    else:
        assert set(st) == {"exp_avg", "exp_avg_sq"} and st["exp_avg_sq"].shape == torch.Size(shape)
    # one step keeps them
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(shape, generator=gen, dtype=torch.float64)
    w2, _, _ = R.param_step(w, torch.randn(shape, generator=gen, dtype=torch.float64), st, torch.float64, 1e-3)
    assert w2.shape == w.shape and all(torch.isfinite(x).all() for x in st.values())
    assert R.new_state(shape)["exp_avg"].shape == st["exp_avg"].shape
    for key, x in R.new_state(shape).items():
        assert st[key].shape == x.shape, key


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", [(3, 5), (9,)])
def test_all_zero_gradient_gives_finite_state_and_moves_weights_by_the_decay_only(shape, dtype):
    gen = torch.Generator().manual_seed(4)
    w = (torch.randn(shape, generator=gen) * 0.02).to(dtype)
    st = R.new_state(shape, dtype)
    w2, k, rms = R.param_step(w, torch.zeros(shape), st, dtype, 1e-2, weight_decay=0.1)
    assert all(torch.isfinite(x).all() for x in st.values()) and float(k) == 1.0 and float(rms) == 0.0
    assert not bool(st["exp_avg"].any())
    T = lambda x: torch.tensor(R.f32(x), dtype=dtype)
    assert torch.equal(w2, w - (T(0.1) * T(1e-2)) * w)


# ---- the geometry table of the kernels ----
def test_geometry_table_agrees_with_the_reference_layout():
    from orv_amd import ops
    shapes = SHAPES + [(130, 257), (64, 256), (65, 257), (1920, 32, 2, 2), (2049,)]
    geo = ops.came_geometry(shapes)
    lays, (rows, cols, nv) = R.layout(shapes)
    assert (geo["n_rows"], geo["n_cols"], geo["n_v"]) == (rows, cols, nv)
    tiles = mats = rowp = colp = 0
    for shape, row, lay in zip(shapes, geo["table"], lays):
        B, Rr, C, tile0, mat0, row0, col0, v0, rowp0, colp0, numel, pad = row
        assert (B, Rr, C, row0, col0, v0) == lay and numel == math.prod(shape) and pad == 0
        assert (tile0, mat0, rowp0, colp0) == (tiles, mats, rowp, colp)
        if Rr:
            nrt, nct = -(-Rr // 64), -(-C // 256)
            tiles, mats, rowp, colp = tiles + B * nrt * nct, mats + B, rowp + B * Rr * nct, colp + B * C * nrt
        else:
            tiles += -(-numel // 2048)
    assert (geo["n_tiles"], geo["n_mats"], geo["n_rowp"], geo["n_colp"]) == (tiles, mats, rowp, colp)
    assert geo["n_scratch"] == rowp + colp + tiles + rows + cols + 2 * len(shapes)
    assert ops.came_geometry([(65, 257)])["n_tiles"] == 4 and ops.came_geometry([(64, 256)])["n_tiles"] == 1
    with pytest.raises(ValueError, match="no elements"):
        ops.came_geometry([(3, 0)])


# ---- FusedCAME over the stand-in ----
@pytest.fixture
def standin():
    from orv_amd import ops
    saved = ops.sumsq, ops.came_step
    calls = []

    def sumsq(g, out):
        out.add_(g.float().pow(2).sum())

    def step(*a, **k):
        calls.append((a, k))
        return R.came_step(*a, **k)

    ops.sumsq, ops.came_step = sumsq, step
    yield calls
    ops.sumsq, ops.came_step = saved


def _params(seed=7, shapes=SHAPES):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.02).to(BF)) for s in shapes]


def _feed(params, t, skip=()):
    for i, p in enumerate(params):
        gen = torch.Generator().manual_seed(1000 * t + i)
        p.grad = None if i in skip else (torch.randn(p.shape, generator=gen) * 0.05).to(BF)


def test_lazy_export_and_constructor_refusals():
    import orv_amd
    from orv_amd import optim
    assert orv_amd.FusedCAME is optim.FusedCAME and issubclass(optim.FusedCAME, optim.FusedAdamW)
    ps = _params()
    with pytest.raises(TypeError):
        optim.FusedCAME(ps)                                           # lr is required
    with pytest.raises(ValueError, match=r"param_precision='stochastic'.*supported: 'bf16', 'split_fp32'"):
        optim.FusedCAME(ps, 1e-3, param_precision="stochastic")
    with pytest.raises(ValueError, match=r"state_precision='fp8'.*supported: 'fp32'"):
        optim.FusedCAME(ps, 1e-3, state_precision="fp8")
    for lr in (0.0, -1e-3):
        with pytest.raises(ValueError, match=r"lr=.*supported: lr > 0"):
            optim.FusedCAME(ps, lr)
    for betas in ((0.9, 0.999, 1.5), (-0.1, 0.999, 0.9999), (0.9, 0.999)):
        with pytest.raises(ValueError, match=r"betas=.*supported: three values.*\[0, 1\]"):
            optim.FusedCAME(ps, 1e-3, betas=betas)
    for eps in ((0.0, 1e-16), (-1e-30, 1e-16)):
        with pytest.raises(ValueError, match=r"eps=.*supported: \(eps1, eps2\) with eps1 > 0"):
            optim.FusedCAME(ps, 1e-3, eps=eps)
    opt = optim.FusedCAME(ps, 1e-3)
    assert (opt.eps, opt.clip_threshold, opt.betas, opt.weight_decay, opt.max_grad_norm, opt.param_precision) == \
        ((1e-30, 1e-16), 1.0, (0.9, 0.999, 0.9999), 0.0, 1.0, "bf16")
    assert opt.state_dict()["optimizer"] == "came"
    with pytest.raises(ValueError, match=r"CAME is not built into get_optimizer.*orv_amd.FusedCAME\(params, lr=.*supported: .*adamw, prodigy"):
        optim.get_optimizer(ps, "came")


@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_fused_came_follows_the_reference_keeps_no_v_and_shapes_its_state(standin, precision):
    from orv_amd.optim import FusedCAME
    params = _params()
    init = [p.detach().clone() for p in params]
    kw = dict(betas=R.REFERENCE_BETAS, weight_decay=1e-2)
    opt = FusedCAME(params, 1e-3, max_grad_norm=0.0, param_precision=precision, **kw)
    weights = [p.detach().float() for p in params]
    states = [R.new_state(p.shape, torch.float32) for p in params]
    for t in range(3):
        _feed(params, t, skip=(2,) if t == 1 else ())
        opt.step()
        for i, p in enumerate(params):
            if p.grad is not None:
                weights[i], _, _ = R.param_step(weights[i], p.grad, states[i], torch.float32, 1e-3, **kw)
                if precision == "bf16":
                    weights[i] = weights[i].to(BF).float()
        opt.zero_grad()
    f = opt._flat
    assert "v" not in f and f["m"].numel() == f["p"].numel()
    assert all(t.numel() < f["p"].numel() for t in f["came_stats"].values() if t is not None)
    assert opt.moments()[1] is None
    for i, (p, st, got) in enumerate(zip(params, states, opt.came_state())):
        assert set(got) == set(st), i
        for key in st:
            assert got[key].shape == st[key].shape and torch.equal(got[key], st[key]), (i, key)
        assert torch.equal(opt.master_params()[i], weights[i]), i
        assert not torch.equal(p.detach(), init[i])
    assert len(standin) == 3 and standin[0][1]["mode"] == (1 if precision == "split_fp32" else 0)
    state, scratch = opt.state_bytes()
    assert state == 4 * f["m"].numel() + sum(4 * t.numel() for t in f["came_stats"].values()) and scratch == 4 * f["came_geo"]["n_scratch"]


def test_zero_gradient_and_inactive_parameter(standin):
    from orv_amd.optim import FusedCAME
    params = _params()
    init = [p.detach().clone() for p in params]
    opt = FusedCAME(params, 1e-2, weight_decay=0.1, max_grad_norm=1.0, param_precision="split_fp32")
    for i, p in enumerate(params):
        p.grad = None if i == 1 else torch.zeros_like(p)
    assert opt.step() == 0.0
    st = opt.came_state()
    T = lambda x: torch.tensor(R.f32(x))
    for i, (p, w0) in enumerate(zip(opt.master_params(), init)):
        if i == 1:
            assert torch.equal(p, w0.float()) and all(not bool(x.any()) for x in st[i].values())
        else:
            assert torch.equal(p, w0.float() - (T(0.1) * T(1e-2)) * w0.float())
            assert all(bool(torch.isfinite(x).all()) for x in st[i].values()) and not bool(st[i]["exp_avg"].any())


def _run(steps, save_at=None, precision="split_fp32"):
    from orv_amd.optim import FusedCAME
    kw = dict(betas=R.REFERENCE_BETAS, weight_decay=1e-2, max_grad_norm=0.0, param_precision=precision)
    params = _params()
    opt = FusedCAME(params, 1e-3, **kw)
    for t in range(steps):
        if t == save_at:
            sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
            weights = [p.detach().clone() for p in params]
            params = _params(seed=8)
            with torch.no_grad():
                for p, w in zip(params, weights):
                    p.copy_(w)
            opt = FusedCAME(params, 1e-3, **kw)
            opt.load_state_dict(sd)
        _feed(params, t, skip=(3,) if t % 2 else ())
        opt.step()
        opt.zero_grad()
    return opt


@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_state_dict_round_trip_continues_bit_for_bit(standin, precision):
    a, b = _run(6, precision=precision), _run(6, save_at=3, precision=precision)
    for x, y in zip(a.master_params(), b.master_params()):
        assert torch.equal(x, y)
    for sa, sb in zip(a.came_state(), b.came_state()):
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
    sd = a.state_dict()
    assert sd["optimizer"] == "came" and "exp_avg_sq" not in sd and sd["exp_avg"].numel() == a._flat["p"].numel()


def test_checkpoints_of_the_other_optimizers_are_refused(standin):
    from orv_amd import optim
    came = optim.FusedCAME(_params(), 1e-3)
    adamw_sd = optim.FusedAdamW(_params()).state_dict()
    with pytest.raises(ValueError, match=r"FusedCAME.load_state_dict: the checkpoint was written by the 'adamw' optimizer.*supported: checkpoints of FusedCAME"):
        came.load_state_dict(adamw_sd)
    prodigy_sd = optim.FusedProdigy(_params()).state_dict()
    with pytest.raises(ValueError, match=r"written by the 'prodigy' optimizer"):
        came.load_state_dict(prodigy_sd)
    with pytest.raises(ValueError, match=r"FusedAdamW.load_state_dict: the checkpoint was written by the 'came' optimizer"):
        optim.FusedAdamW(_params()).load_state_dict(came.state_dict())
    with pytest.raises(ValueError, match=r"FusedProdigy.load_state_dict: the checkpoint was written by the 'came' optimizer"):
        optim.FusedProdigy(_params()).load_state_dict(came.state_dict())
    other = optim.FusedCAME(_params(shapes=[s[::-1] for s in SHAPES]), 1e-3)
    with pytest.raises(ValueError, match="other shapes"):
        other.load_state_dict(came.state_dict())


def test_lr_schedule_is_read_at_every_step(standin):
    from orv_amd.optim import FusedCAME
    params = _params()
    opt = FusedCAME(params, 1e-3, max_grad_norm=0.0)
    _feed(params, 0)
    opt.step()
    opt.param_groups[0]["lr"] = 0.0              # a warm-up schedule's first value: allowed after construction
    _feed(params, 1)
    before = [p.detach().clone() for p in params]
    opt.step()
    assert [c[0][9] for c in standin] == [1e-3, 0.0]
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
