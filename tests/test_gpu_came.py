"""GPU: the fused CAME optimizer (``orv_came_step`` / ``orv_came_launch``, ``FusedCAME``) against its CPU restatement (tests/came_ref.py).
The storage of the weights (split / rebuild, nearest-even bf16) is held bit for bit; the fp32 arithmetic is held to a float64 evaluation of
the rule with the error of a CPU fp32 evaluation as the yardstick - the convention of test_gpu_prodigy.py, for the same reasons (FMA
contraction and a one-step difference of a library function are allowed, so bit-equality of the arithmetic is not demanded).  Every quantity
is compared in units of the scale of its terms (EPS = 2^-23, one fp32 epsilon):
    weights   max(|w_old|, |w_new|, |w_new - w_old|)
    m         b1 |m_old| + (1-b1) |u|
    r, c, Rr, Cc, v, k   the new value itself (sums of non-negative terms)
and the bound is twice the worst CPU fp32 error of that quantity, with a floor of 4 EPS: a stored value is a handful of fp32 roundings.
Measured figures are printed before they are asserted.

The kernels cut a factored matrix into tiles of 64 rows x 256 columns, a lane owns 8 consecutive columns, and rows are read with 16-byte
accesses where C % 8 == 0 and element by element otherwise.  The layout of the kernel tests therefore holds, beside the shapes every CAME
test wants ([3,5], [130,257], [1,7], [7,1], [5,3,2,2], [2049], []), the shapes [63,255], [64,256], [65,257] (one below, at and one above both
tile edges; 255 and 257 take the element path, 256 the 16-byte path) and [65,264] (16-byte path with a column tile of one lane), and an
INACTIVE [33,65].  Every scratch value is poisoned with NaN before a step: a value read before it is written would reach the outputs."""
import pytest
import torch

import adamw_ref
import came_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEG = 2048
EPS = 2.0 ** -23
SHAPES = [(3, 5), (130, 257), (1, 7), (7, 1), (5, 3, 2, 2), (2049,), (), (63, 255), (64, 256), (65, 257), (65, 264), (33, 65)]
ACTIVE = [1] * 11 + [0]
# statistics scaled so that u is small (k == 1) for the even parameters and large (k > 1) for the odd ones
STAT_SCALE = [4.0 if i % 2 == 0 else 0.25 for i in range(len(SHAPES))]
LR = 1e-3


def _dev():
    return torch.device("cuda:0")


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def _starts(shapes):
    starts, o = [], 0
    for s in shapes:
        starts.append(o)
        o += (_numel(s) + SEG - 1) // SEG * SEG
    return starts + [o]


def _real_mask(shapes):
    starts = _starts(shapes)
    real = torch.zeros(starts[-1], dtype=torch.bool)
    for a, s in zip(starts, shapes):
        real[a:a + _numel(s)] = True
    return real


def _segment_mask(shapes, active):
    starts = _starts(shapes)
    act = torch.zeros(starts[-1], dtype=torch.bool)
    for i, a in enumerate(active):
        act[starts[i]:starts[i + 1]] = bool(a)
    return act


def _inputs(shapes, active, stat_scale, seed=0, zero_state=False, g_scale=0.05):
    """A non-trivial state: random weights, low halves, m, positive statistics; padding all zero; inactive segments as random as the rest."""
    gen = torch.Generator().manual_seed(seed)
    starts = _starts(shapes)
    n = starts[-1]
    real = _real_mask(shapes)
    z = lambda x: torch.where(real, x, torch.zeros_like(x))
    p = z((torch.randn(n, generator=gen) * 0.02).to(BF))
    lo = z(torch.randint(-32768, 32768, (n,), generator=gen, dtype=torch.int64).to(torch.int16))
    lo = torch.where(p.float() == 0, torch.zeros_like(lo), lo)      # a weight of exactly +-0 with a negative low half is a NaN master (randn does return 0.0)
    g = z((torch.randn(n, generator=gen) * g_scale).to(BF))
    m = z(torch.randn(n, generator=gen) * 0.3)
    lays, (rows, cols, nv) = R.layout(shapes)
    stats = R.zero_stats(shapes)
    for (B, Rr, C, row0, col0, v0), shape, sc in zip(lays, shapes, stat_scale):
        var = (sc * g_scale) ** 2
        pos = lambda k: (0.5 + torch.rand(k, generator=gen))
        if Rr:
            stats["r"][row0:row0 + B * Rr] = var * pos(B * Rr)
            stats["c"][col0:col0 + B * C] = var * pos(B * C)
            stats["res_r"][row0:row0 + B * Rr] = 0.1 * pos(B * Rr)
            stats["res_c"][col0:col0 + B * C] = 0.1 * pos(B * C)
        else:
            stats["v"][v0:v0 + _numel(shape)] = var * pos(_numel(shape))
    if zero_state:
        m.zero_(), lo.zero_()
        stats = R.zero_stats(shapes)
    return dict(p=p, lo=lo, g=g, m=m, stats=stats, shapes=list(shapes), seg_start=torch.tensor(starts, dtype=torch.int64),
                active=torch.tensor(active, dtype=torch.uint8))


def _launch(inp, lr=LR, clip=None, mode=1, poison=float("nan"), **hyper):
    """One ``orv_came_step`` on the GPU -> CPU copies of every buffer and of the (k, rms) pairs."""
    from orv_amd import ops
    dev = _dev()
    h = dict(R.DEFAULTS, **hyper)
    geo = ops.came_geometry(inp["shapes"])
    t = {k: inp[k].to(dev).clone() for k in ("p", "lo", "g", "m", "seg_start", "active")}
    stats = {k: (x.to(dev).clone() if x.numel() else None) for k, x in inp["stats"].items()}
    geom = torch.tensor(geo["table"], dtype=torch.int64, device=dev)
    scratch = torch.full((geo["n_scratch"],), poison, dtype=torch.float32, device=dev)
    cl = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=dev)
    ops.came_step(t["p"], t["g"], t["m"], stats, t["seg_start"], t["active"], geom, geo, scratch, lr, h["betas"], h["eps"], h["clip_threshold"],
                  h["weight_decay"], cl, lo=t["lo"] if mode == 1 else None, mode=mode)
    torch.cuda.synchronize()
    out = {k: x.cpu() for k, x in t.items()}
    out["stats"] = {k: (x.cpu() if x is not None else torch.zeros(0)) for k, x in stats.items()}
    out["k_rms"] = scratch[-2 * len(inp["shapes"]):].view(-1, 2).cpu()
    return out


def _reference(inp, dtype, lr=LR, clip=None, mode=1, **hyper):
    w_old = adamw_ref.rebuild(inp["p"], inp["lo"]) if mode == 1 else inp["p"].float()
    w, m, stats, ks, rmss = R.flat_step(w_old, inp["g"], inp["m"], inp["stats"], inp["shapes"], inp["seg_start"], inp["active"], dtype, lr,
                                        clip=1.0 if clip is None else clip, **hyper)
    return dict(w=w, m=m, stats=stats, k=ks, rms=rmss, w_old=w_old)


def _compare(what, inp, got, r64, r32, betas, mode=1):
    """Prints and returns {quantity: (GPU error, CPU fp32 error, bound)} in units of EPS x the scale of the quantity's terms."""
    shapes, active = inp["shapes"], inp["active"].tolist()
    sel = _real_mask(shapes) & _segment_mask(shapes, active)
    w_old = r64["w_old"].double()
    w_gpu = (adamw_ref.rebuild(got["p"], got["lo"]) if mode == 1 else got["p"].float()).double()
    b1 = R.f32(betas[0])
    scale = {"w": torch.maximum(torch.maximum(w_old.abs(), r64["w"].abs()), (r64["w"] - w_old).abs()),
             "m": b1 * inp["m"].double().abs() + (r64["m"] - b1 * inp["m"].double()).abs()}
    pairs = {"w": (w_gpu, r64["w"], r32["w"].double(), sel), "m": (got["m"].double(), r64["m"], r32["m"].double(), sel)}
    lays, _ = R.layout(shapes)
    for key in R.STATS:
        own = torch.zeros(r64["stats"][key].numel(), dtype=torch.bool)
        for (B, Rr, C, row0, col0, v0), shape, a in zip(lays, shapes, active):
            if a and Rr and key != "v":
                off, cnt = (row0, B * Rr) if key in ("r", "res_r") else (col0, B * C)
                own[off:off + cnt] = True
            elif a and not Rr and key == "v":
                own[v0:v0 + _numel(shape)] = True
        scale[key] = r64["stats"][key].abs()
        pairs[key] = (got["stats"][key].double(), r64["stats"][key], r32["stats"][key].double(), own)
    idx = [i for i, a in enumerate(active) if a]
    k64 = torch.tensor([r64["k"][i] for i in idx], dtype=torch.float64)
    pairs["k"] = (got["k_rms"][idx, 0].double(), k64, torch.tensor([r32["k"][i] for i in idx], dtype=torch.float64), torch.ones(len(idx), dtype=torch.bool))
    scale["k"] = k64
    res = {}
    bad = {key: (int((~torch.isfinite(gpu[own])).sum()), int(own.sum()), (~torch.isfinite(gpu) & own).nonzero().flatten()[:4].tolist())
           for key, (gpu, ref, cpu, own) in pairs.items() if bool(own.any()) and not bool(torch.isfinite(gpu[own]).all())}
    assert not bad, f"{what}: not finite on the GPU - quantity: (count, of, first indices) {bad}"
    for key, (gpu, ref, cpu, own) in pairs.items():
        if not bool(own.any()):
            continue
        # a scale of exactly 0 (m of a parameter whose gradient and m are all zero: a fresh adapter's A) admits no error at all
        rel = lambda x: torch.where(scale[key] > 0, (x - ref).abs() / scale[key], torch.where(x == ref, 0.0, float("inf")).double())
        err = float(rel(gpu)[own].max()) / EPS
        yard = float(rel(cpu)[own].max()) / EPS
        res[key] = (err, yard, max(2 * yard, 4.0))
    print(f"\ncame {what}: error vs float64 in fp32 epsilons of the scale - " +
          ", ".join(f"{k} GPU {e:.2f} / CPU fp32 {y:.2f} (bound {b:.2f})" for k, (e, y, b) in res.items()))
    return res


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _case(wd, betas, clip, mode=1):
    inp = _cached("inputs", lambda: _inputs(SHAPES, ACTIVE, STAT_SCALE))
    hyper = dict(weight_decay=wd, betas=betas)
    refs = _cached(("refs", wd, betas, clip, mode), lambda: (_reference(inp, torch.float64, clip=clip, mode=mode, **hyper),
                                                               _reference(inp, torch.float32, clip=clip, mode=mode, **hyper)))
    return inp, hyper, refs


@pytest.mark.parametrize("clip", [0.37, None])
@pytest.mark.parametrize("betas", [R.DEFAULTS["betas"], R.REFERENCE_BETAS])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_one_step_from_a_non_trivial_state_against_float64(wd, betas, clip):
    """Masters, m, every statistic and k of the layout in the module docstring, split_fp32 mode, lr = 1e-3."""
    inp, hyper, (r64, r32) = _case(wd, betas, clip)
    ks = [k for k in r64["k"] if k is not None]
    assert any(k == 1.0 for k in ks) and any(k > 1.0 for k in ks), ks          # both branches of the clip, on the reference
    got = _launch(inp, clip=clip, **hyper)
    res = _compare(f"one step wd={wd} betas={betas} clip={clip}", inp, got, r64, r32, betas)
    assert set(res) == {"w", "m", "k"} | set(R.STATS)
    for key, (err, yard, bound) in res.items():
        assert err <= bound, (key, err, yard, bound)
    for i, k in enumerate(r64["k"]):
        if k == 1.0:
            assert float(got["k_rms"][i, 0]) == 1.0, i


def test_mode_0_stores_the_nearest_even_bf16_of_the_mode_1_master():
    """Same inputs (low halves zero: the master is the bf16 weight), same arithmetic: mode 0 must store exactly the nearest-even bf16 of the
    master mode 1 produced, and identical m and statistics."""
    inp = dict(_cached("inputs", lambda: _inputs(SHAPES, ACTIVE, STAT_SCALE)))
    inp["lo"] = torch.zeros_like(inp["lo"])
    hyper = dict(weight_decay=1e-2, betas=R.REFERENCE_BETAS)
    one = _launch(inp, clip=0.37, mode=1, **hyper)
    zero = _launch(inp, clip=0.37, mode=0, **hyper)
    master = adamw_ref.rebuild(one["p"], one["lo"])
    assert torch.equal(zero["p"].view(torch.int16), master.to(BF).view(torch.int16))
    assert torch.equal(zero["lo"], inp["lo"])                                   # mode 0 never touches a low-half buffer
    assert torch.equal(zero["m"].view(torch.int32), one["m"].view(torch.int32))
    for key in R.STATS:
        assert torch.equal(zero["stats"][key].view(torch.int32), one["stats"][key].view(torch.int32)), key
    sel = _real_mask(SHAPES) & _segment_mask(SHAPES, ACTIVE)
    assert float((zero["p"] != inp["p"])[sel].float().mean()) > 0.5


def test_real_widths_one_step_against_float64():
    """[1920, 7680] (30 row tiles x 30 column tiles) and [11520, 512] (180 x 2) in one layout: many tiles per row and per column, the
    cross-workgroup partial sums and their fp64 addition."""
    shapes = [(1920, 7680), (11520, 512)]
    inp = _inputs(shapes, [1, 1], [4.0, 0.25], seed=3)
    hyper = dict(weight_decay=1e-2, betas=R.REFERENCE_BETAS)
    r64, r32 = _reference(inp, torch.float64, clip=0.37, **hyper), _reference(inp, torch.float32, clip=0.37, **hyper)
    got = _launch(inp, clip=0.37, **hyper)
    res = _compare("real widths", inp, got, r64, r32, hyper["betas"])
    for key, (err, yard, bound) in res.items():
        assert err <= bound, (key, err, yard, bound)


def _exact_factors(n, gen):
    """Values with two mantissa bits and exponents in [-8, -4]: every product of two of them is exact in bf16."""
    return (1.0 + 0.25 * torch.randint(0, 4, (n,), generator=gen).double()) * 2.0 ** torch.randint(-8, -3, (n,), generator=gen).double()


@pytest.mark.parametrize("betas", [R.DEFAULTS["betas"], R.REFERENCE_BETAS])
def test_closed_forms_from_zero_state(betas):
    """Rank-one gradient on [37, 53]: every weight moves by lr (1-b1) / (b1 sqrt(1-b3)); unfactored [2049]: by lr (1-b1) clip_threshold.
    w0 = 0, so the stored master IS the step.  Bounds from the length of the rounding chain: u (3 roundings), u / k (1), m (2), s through
    u - m = b1 (u - m_old) (errors of u and m amplified by (2 - b1) / b1 = 1.2, doubled by the square: about 5 EPS), halved by the
    rsqrt of Rr and of Cc (about 2.5 EPS each), out (2), the step and its store (2): 16 EPS for the matrix; u (3), k, u / k (1),
    m (1), the step (1): 8 EPS for the vector."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(37, 53), (2049,)]
    inp = _inputs(shapes, [1, 1], [1.0, 1.0], seed=4, zero_state=True)
    inp["p"].zero_()
    a, b = _exact_factors(37, gen), _exact_factors(53, gen) * torch.where(torch.rand(53, generator=gen) < 0.5, -1.0, 1.0)
    g = torch.zeros_like(inp["g"])
    g[:37 * 53] = (a[:, None] * b[None, :]).reshape(-1).to(BF)
    assert torch.equal(g[:37 * 53].double(), (a[:, None] * b[None, :]).reshape(-1))
    vec = (torch.randn(2049, generator=gen) * 0.05).to(BF)
    g[SEG:SEG + 2049] = torch.where(vec == 0, torch.full_like(vec, 0.01), vec)
    inp["g"] = g
    lr = 1e-2
    got = _launch(inp, lr=lr, betas=betas)
    w = adamw_ref.rebuild(got["p"], got["lo"]).double()
    want_m, want_v = R.rank_one_step(lr, betas), R.unfactored_step(lr, betas, 1.0)
    err_m = float((w[:37 * 53] + want_m * g[:37 * 53].double().sign()).abs().max()) / want_m / EPS
    err_v = float((w[SEG:SEG + 2049] + want_v * g[SEG:SEG + 2049].double().sign()).abs().max()) / want_v / EPS
    print(f"\ncame closed forms betas={betas}: matrix step {want_m:.6e} error {err_m:.2f} EPS (bound 16), vector step {want_v:.6e} error {err_v:.2f} EPS (bound 8); "
          f"k {got['k_rms'][:, 0].tolist()}")
    assert err_m <= 16 and err_v <= 8
    b2 = R.f32(betas[1])
    for i in range(2):
        assert abs(float(got["k_rms"][i, 0]) * (1 - b2) ** 0.5 - 1) <= 8 * EPS


def _bytes_equal(a, b):
    same = all(torch.equal(a[k].view(torch.int16) if a[k].dtype == BF else a[k], b[k].view(torch.int16) if b[k].dtype == BF else b[k])
               for k in ("p", "lo", "m"))
    return same and all(torch.equal(a["stats"][k].view(torch.int32), b["stats"][k].view(torch.int32)) for k in R.STATS) \
        and torch.equal(a["k_rms"][:11].view(torch.int32), b["k_rms"][:11].view(torch.int32))


def test_two_runs_give_identical_bytes_and_inactive_segments_and_padding_keep_theirs():
    """Scratch poisoned with NaN in one run and with 7.0 in the other: the outputs depend on neither, so every value read was written first."""
    inp = _cached("inputs", lambda: _inputs(SHAPES, ACTIVE, STAT_SCALE))
    hyper = dict(weight_decay=1e-2, betas=R.REFERENCE_BETAS)
    a = _launch(inp, clip=0.37, **hyper)
    b = _launch(inp, clip=0.37, poison=7.0, **hyper)
    assert _bytes_equal(a, b)
    starts = _starts(SHAPES)
    lo, hi = starts[11], starts[12]
    for k in ("p", "lo", "m"):
        view = torch.int16 if a[k].element_size() == 2 else torch.int32
        assert torch.equal(a[k][lo:hi].view(view), inp[k][lo:hi].view(view)), k                       # the inactive [33, 65]
        assert bool(inp[k][lo:lo + 33 * 65].view(view).any())
        assert not bool(a[k][~_real_mask(SHAPES)].view(view).any()), k                                  # padding
    B, Rr, C, row0, col0, v0 = R.layout(SHAPES)[0][11]
    for key, off, cnt in (("r", row0, Rr), ("res_r", row0, Rr), ("c", col0, C), ("res_c", col0, C)):
        assert torch.equal(a["stats"][key][off:off + cnt].view(torch.int32), inp["stats"][key][off:off + cnt].view(torch.int32)), key
    # v past the end of an unfactored parameter (its padding to 2048) stays zero; the pair of the inactive segment keeps the poison
    v = a["stats"]["v"]
    assert not bool(v[2049:4096].any()) and not bool(v[4097:].any()) and bool(v[:2049].all()) and bool(v[4096] != 0)
    assert bool(torch.isnan(a["k_rms"][11]).all()) and b["k_rms"][11].tolist() == [7.0, 7.0]
    sel = _real_mask(SHAPES) & _segment_mask(SHAPES, ACTIVE)
    assert float((adamw_ref.rebuild(a["p"], a["lo"]) != adamw_ref.rebuild(inp["p"], inp["lo"]))[sel].float().mean()) > 0.99


def test_all_zero_gradient_on_active_parameters():
    """From zero state, weight_decay 0.1: everything stays finite, m stays 0, the weights move by the decay only."""
    shapes = [(130, 257), (9,)]
    inp = _inputs(shapes, [1, 1], [1.0, 1.0], seed=5, zero_state=True)
    inp["g"].zero_()
    got = _launch(inp, lr=1e-2, weight_decay=0.1)
    assert not bool(got["m"].any())
    for key in R.STATS:
        assert bool(torch.isfinite(got["stats"][key]).all()), key
    assert bool((got["stats"]["r"] > 0).all()) and bool((got["stats"]["res_c"] > 0).all()) and bool((got["stats"]["v"][:9] > 0).all())
    assert got["k_rms"].tolist() == [[1.0, 0.0], [1.0, 0.0]]
    w_old = adamw_ref.rebuild(inp["p"], inp["lo"])
    T = lambda x: torch.tensor(R.f32(x))
    assert torch.equal(adamw_ref.rebuild(got["p"], got["lo"]), w_old - (T(0.1) * T(1e-2)) * w_old)


# ---- FusedCAME ----
def _shape_params(dev, seed=5, shapes=SHAPES):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.02).to(BF).to(dev)) for s in shapes]


def _feed(params, t, dev):
    for i, p in enumerate(params):
        gen = torch.Generator().manual_seed(1000 * t + i)
        p.grad = None if i == len(params) - 1 else (torch.randn(p.shape, generator=gen) * 0.05).to(BF).to(dev)


def _snapshot(opt):
    torch.cuda.synchronize()
    f = opt._flat
    snap = {k: f[k].cpu().clone() for k in ("p", "m") + (("lo",) if "lo" in f else ())}
    snap.update({"stat_" + k: t.cpu().clone() for k, t in f["came_stats"].items() if t is not None})
    return snap


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.int16) if a[k].dtype == BF else a[k], b[k].view(torch.int16) if b[k].dtype == BF else b[k]) for k in a)


def _run(steps, dev, precision, save_at=None):
    from orv_amd.optim import FusedCAME
    kw = dict(betas=R.REFERENCE_BETAS, weight_decay=1e-2, max_grad_norm=0.0, param_precision=precision)      # no clip: orv_sumsq's atomics stay out
    params = _shape_params(dev)
    opt = FusedCAME(params, 1e-3, **kw)
    for t in range(steps):
        if t == save_at:
            sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
            weights = [p.detach().clone() for p in params]
            params = _shape_params(dev, seed=6)
            with torch.no_grad():
                for p, w in zip(params, weights):
                    p.copy_(w)
            opt = FusedCAME(params, 1e-3, **kw)
            opt.load_state_dict(sd)
        _feed(params, t, dev)
        opt.step()
        opt.zero_grad()
    return opt


@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_state_dict_resume_is_bit_identical_and_other_checkpoints_are_refused(precision):
    from orv_amd import optim
    dev = _dev()
    a, b = _snapshot(_run(6, dev, precision)), _snapshot(_run(6, dev, precision, save_at=3))
    assert _same(a, b) and bool(a["m"].any()) and ("lo" in a) == (precision == "split_fp32")
    came = _run(1, dev, precision)
    assert came.state_dict()["optimizer"] == "came"
    adamw = optim.FusedAdamW(_shape_params(dev), lr=1e-3, max_grad_norm=0.0)
    prodigy = optim.FusedProdigy(_shape_params(dev), max_grad_norm=0.0)
    for opt in (adamw, prodigy):
        _feed(opt.params, 0, dev)
        opt.step()
    with pytest.raises(ValueError, match=r"FusedCAME.load_state_dict: the checkpoint was written by the 'adamw' optimizer"):
        came.load_state_dict(adamw.state_dict())
    with pytest.raises(ValueError, match=r"FusedCAME.load_state_dict: the checkpoint was written by the 'prodigy' optimizer"):
        came.load_state_dict(prodigy.state_dict())
    with pytest.raises(ValueError, match=r"written by the 'came' optimizer"):
        adamw.load_state_dict(came.state_dict())


def _quadratic_reference(dtype, shapes, targets, steps, hyper):
    """-> per parameter the loss after every step and the RMS of u of every step, the rule evaluated in ``dtype``."""
    losses, rmss = [], []
    for shape, target in zip(shapes, targets):
        w, st = torch.zeros(shape, dtype=dtype), R.new_state(shape, dtype)
        ls, rs = [], []
        for _ in range(steps):
            g = (w - target.to(dtype)).to(BF)
            w, _, rms = R.param_step(w, g, st, dtype, 1e-3, **hyper)
            ls.append(float(((w.double() - target.double()) ** 2).mean()))
            rs.append(float(rms))
        losses.append(ls), rmss.append(rs)
    return losses, rmss


def test_thirty_steps_on_the_quadratic_follow_the_float64_reference():
    """w0 = 0, target N(0, 0.02^2), loss mean (w - target)^2, gradient w - target rounded to bf16, lr 1e-3, betas 0.9 / 0.95 / 0.98,
    weight_decay 1e-2, on [130, 257] and [2049] (one optimizer, split_fp32, no global clip).  At every step the loss and the RMS of u
    must lie within twice the largest deviation the CPU fp32 run has shown from the float64 run up to that step (floor 4 EPS relative):
    a deviation is carried along the trajectory - a last-place difference in w can flip the bf16 rounding of a gradient element - so the
    deviation of a single step can be zero by chance while the run has already drifted."""
    from orv_amd.optim import FusedCAME
    dev = _dev()
    shapes = [(130, 257), (2049,)]
    gen = torch.Generator().manual_seed(21)
    targets = [torch.randn(s, generator=gen) * 0.02 for s in shapes]
    hyper = dict(betas=R.REFERENCE_BETAS, weight_decay=1e-2)
    l64, r64 = _quadratic_reference(torch.float64, shapes, targets, 30, hyper)
    l32, r32 = _quadratic_reference(torch.float32, shapes, targets, 30, hyper)
    params = [torch.nn.Parameter(torch.zeros(s, dtype=BF, device=dev)) for s in shapes]
    tg = [t.to(dev) for t in targets]
    opt = FusedCAME(params, 1e-3, max_grad_norm=0.0, param_precision="split_fp32", **hyper)
    loss, rms = [[], []], [[], []]
    for _ in range(30):
        masters = opt.master_params()
        for p, w, t in zip(params, masters, tg):
            p.grad = (w - t).to(BF)
        opt.step()
        r = opt.last_clip()[1].tolist()
        for i, (w, t) in enumerate(zip(opt.master_params(), tg)):
            loss[i].append(float(((w.double() - t.double()) ** 2).mean()))
            rms[i].append(r[i])
    ok = True
    for i, shape in enumerate(shapes):
        worst = {}
        for name, gpu, a64, a32 in (("loss", loss[i], l64[i], l32[i]), ("rms", rms[i], r64[i], r32[i])):
            yard, w_err, w_yard = 0.0, 0.0, 0.0
            for t in range(30):
                yard = max(yard, abs(a32[t] - a64[t]) / a64[t])
                err = abs(gpu[t] - a64[t]) / a64[t]
                if err / max(2 * yard, 4 * EPS) > w_err:
                    w_err, w_yard = err / max(2 * yard, 4 * EPS), yard
            worst[name] = (w_err, w_yard)
            ok = ok and w_err <= 1.0
        print(f"\ncame 30 steps on {list(shape)}: loss {float((targets[i].double() ** 2).mean()):.3e} -> {loss[i][-1]:.3e} (float64 {l64[i][-1]:.3e}, "
              f"CPU fp32 {l32[i][-1]:.3e}); worst error / bound: loss {worst['loss'][0]:.3f}, rms of u {worst['rms'][0]:.3f}; "
              f"rms of u first / last {rms[i][0]:.4f} / {rms[i][-1]:.4f}")
        assert loss[i][-1] < float((targets[i].double() ** 2).mean())
    assert ok


def test_in_the_model_three_sft_steps_on_a_fresh_adapter():
    """The tiny fwd_actions configuration with add_adapter(r=16), FusedCAME(lr=1e-3, the reference's betas, weight_decay 1e-2, split_fp32),
    three sft_steps.  After each step every adapter master is compared with the reference fed the state the step started from and the
    gradients the GPU produced (bound of the one-step test); after three, every adapter weight has moved and no base weight has."""
    from conftest import load_golden
    from orv_amd import FusedCAME, schedulers, sft
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
    hyper = dict(betas=R.REFERENCE_BETAS, weight_decay=1e-2)
    opt = FusedCAME(params, 1e-3, max_grad_norm=1.0, param_precision="split_fp32", **hyper)
    opt._build()
    f = opt._flat
    n = f["p"].numel()
    shapes = [tuple(p.shape) for p in opt.params]
    first = [x.cpu().clone() for x in opt.master_params()]
    for step in range(3):
        torch.cuda.synchronize()
        before = dict(p=f["p"].cpu().clone(), lo=f["lo"].cpu().clone(), m=f["m"].cpu().clone(),
                      stats={k: (t.cpu().clone() if t is not None else torch.zeros(0)) for k, t in f["came_stats"].items()})
        loss, parts = sft.sft_step(m, sched, opt, batch, generator=torch.Generator(device=dev).manual_seed(100 + step))
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and parts["grad_norm"] > 0
        clip = float(torch.clamp(1.0 / (torch.tensor(parts["grad_norm"], dtype=torch.float32) + 1e-6), max=1.0))
        inp = dict(before, g=f["g"][:n].cpu(), shapes=shapes, seg_start=f["seg_start"].cpu(), active=f["active"].cpu())
        assert bool(inp["active"].all())
        r64, r32 = (_reference(inp, dt, clip=clip, **hyper) for dt in (torch.float64, torch.float32))
        got = dict(p=f["p"].cpu(), lo=f["lo"].cpu(), m=f["m"].cpu(), stats={k: (t.cpu() if t is not None else torch.zeros(0)) for k, t in f["came_stats"].items()},
                   k_rms=torch.stack(opt.last_clip(), 1).cpu())
        res = _compare(f"in the model, step {step + 1} (loss {float(loss):.4f})", inp, got, r64, r32, hyper["betas"])
        for key, (err, yard, bound) in res.items():
            assert err <= bound, (step, key, err, yard, bound)
    now = m.state_dict()
    assert all(torch.equal(now[k], base0[k]) for k in base0), "a base weight moved"
    for a, b in zip(first, opt.master_params()):
        assert bool((a != b.cpu()).any()), "an adapter weight never moved"


def _all_tensors(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _all_tensors(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from _all_tensors(v)


def test_memory_from_the_allocated_buffers():
    """[1920,1920], [7680,1920], [1920,7680], [1920]: m is the only fp32 buffer of the parameters' size, state = m + statistics is
    4 + 8 (R + C) / (R C) bytes per element of a matrix (four vectors of R or C floats; 4.008 for [1920,1920]) - at most 4.01 -, the scratch
    4 (R ceil(C / 256) + C ceil(R / 64) + ceil(R / 64) ceil(C / 256) + R + C) bytes per matrix - at most 0.25 per element."""
    from orv_amd.optim import FusedCAME
    dev = _dev()
    shapes = [(1920, 1920), (7680, 1920), (1920, 7680), (1920,)]
    params = [torch.nn.Parameter(torch.zeros(s, dtype=BF, device=dev)) for s in shapes]
    opt = FusedCAME(params, 1e-3)
    opt._build()
    f = opt._flat
    total, elements = f["p"].numel(), sum(_numel(s) for s in shapes)
    seen, big32 = set(), []
    for t in _all_tensors(f):
        base = t.untyped_storage().data_ptr()
        if t.is_cuda and base not in seen:
            seen.add(base)
            if t.untyped_storage().nbytes() >= 4 * elements:
                big32.append(t)
    assert len(big32) == 1 and big32[0].data_ptr() == f["m"].data_ptr(), [tuple(t.shape) for t in big32]
    assert "v" not in f and f["came_stats"]["v"].numel() == 2048
    state, scratch = opt.state_bytes()
    print(f"\ncame memory: {elements} elements ({total} padded), state {state} B = {state / elements:.5f} B / element, scratch {scratch} B = "
          f"{scratch / elements:.5f} B / element")
    assert state / elements <= 4.01 and scratch / elements <= 0.25
    assert scratch == 4 * f["came_scratch"].numel() and state >= 4 * elements


def test_argument_validation_returns_a_status_and_a_message_without_a_launch():
    from orv_amd import _lib
    h = _lib.lib()
    dev = _dev()
    buf = torch.zeros(8192, dtype=torch.float64, device=dev)
    p = buf.data_ptr()
    msg = lambda: h.orv_last_error().decode()

    def desc(**kw):
        d = dict(p=p, lo=p, g=p, m=p, r=p, c=p, res_r=p, res_c=p, v=p, n=2048, n_rows=3, n_cols=5, n_v=0, seg_start=p, seg_active=p, nseg=1,
                 geom=p, n_tiles=1, n_mats=1, n_rowp=3, n_colp=5, scratch=p, n_scratch=19, clip_coef=None, lr=1e-3, beta1=0.9, beta2=0.999,
                 beta3=0.9999, eps1=1e-30, eps2=1e-16, clip_threshold=1.0, weight_decay=0.0, mode=1)
        d.update(kw)
        return _lib.Came(**d)

    assert h.orv_came_step(None, None) != 0 and "null descriptor" in msg()
    assert h.orv_came_launch(desc(), 7, None) != 0 and "which=7" in msg()
    for n in (2047, 0):
        assert h.orv_came_step(desc(n=n), None) != 0 and "multiple of 2048" in msg()
    assert h.orv_came_step(desc(mode=2), None) != 0 and "mode=2" in msg()
    for name in ("p", "g", "m", "seg_start", "seg_active", "geom", "scratch", "lo", "r", "res_c"):
        assert h.orv_came_step(desc(**{name: None}), None) != 0 and "null buffer" in msg(), name
    assert h.orv_came_step(desc(n_v=2048, v=None), None) != 0 and "null buffer" in msg()
    assert h.orv_came_step(desc(n_v=100), None) != 0 and "bad sizes" in msg()
    assert h.orv_came_step(desc(eps1=0.0), None) != 0 and "eps1=0" in msg()
    assert h.orv_came_step(desc(clip_threshold=0.0), None) != 0 and "clip_threshold=0" in msg()
    assert h.orv_came_step(desc(n_scratch=18), None) != 0 and "scratch holds 18 floats, the layout needs 19" in msg()
    assert h.orv_came_step(desc(n_tiles=0), None) != 0 and "n_tiles=0" in msg()
    assert h.orv_came_step(desc(n_mats=0), None) != 0 and "zero together" in msg()
    torch.cuda.synchronize()
    assert not bool(buf.any())                                 # nothing was launched: the buffer every pointer named is untouched
