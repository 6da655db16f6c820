"""The float64 restatements of ``tests/forward_ref.py`` against independent sources (``torch.nn.functional``, ``oracle/leaf.py``),
and the conditions on the inputs of ``tests/test_gpu_forward_edges.py`` that can be checked without a GPU (the tie cap)."""
import math

import pytest
import torch
import torch.nn.functional as F

import forward_ref as ref
from oracle import leaf

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_round_bf16_ties_rounds_to_nearest_even_and_flags_the_boundaries():
    v = torch.randn(20000, generator=gen(1)).double() * torch.tensor([1e-3, 1.0, 300.0]).double().repeat(20000)[:20000]
    r, m = ref.round_bf16_ties(v, 0.0)
    assert torch.equal(r.to(BF).double(), r)                                    # bf16 values
    assert torch.equal(r, v.float().to(BF).double())                            # fp32-representable inputs: torch rounds them once
    assert ((r - v).abs() <= ref.ulp_bf16(v) / 2).all() and not m.any()
    mid = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(2 + 2.0 ** -7), 2.0 ** -133 * 2.5, 2.0 ** -127 * 1.5, 0.0], dtype=F64)
    r, m = ref.round_bf16_ties(mid, 0.0)
    assert r.tolist() == [1.0, 1 + 2.0 ** -6, -2.0, 2.0 ** -132, 2.0 ** -127 * 1.5, 0.0] and m.tolist() == [True, True, True, True, False, False]
    near = torch.tensor([1 + 2.0 ** -8 + 1e-6, 1 + 2.0 ** -8 - 1e-6, 1.0 + 1e-6, 2.0 - 2.0 ** -8 + 1e-6], dtype=F64)
    assert ref.round_bf16_ties(near, 1e-5)[1].tolist() == [True, True, False, True]
    assert ref.round_bf16_ties(near, 1e-7)[1].tolist() == [False, False, False, False]
    assert ref.round_bf16_ties(near, 0.0)[0].tolist() == [1 + 2.0 ** -7, 1.0, 1.0, 2.0]


@pytest.mark.parametrize("form", ["full", "gamma_beta", "gamma", "beta", "table", "nothing"])
@pytest.mark.parametrize("mapped", [False, True])
def test_layernorm_modulate_against_functional_layer_norm(form, mapped):
    batch, nv, nt, per, D = 2, 32, 5, 8, 72
    has_g, has_b, has_t = {"full": (1, 1, 1), "gamma_beta": (1, 1, 0), "gamma": (1, 0, 0), "beta": (0, 1, 0), "table": (0, 0, 1),
                           "nothing": (0, 0, 0)}[form]
    grp = (nv, 0, per)
    i = ref.ln_inputs(D, batch, nv, 0, per, True, 3, rows_x=batch * (nv + nt) if mapped else None, ldx=D + 64)
    xmap = (nv, nv + nt, nt) if mapped else None
    gamma, beta = (i["gamma"] if has_g else None), (i["beta"] if has_b else None)
    got = ref.layernorm_modulate(i["x"], gamma, beta, i["scale"] if has_t else None, i["shift"] if has_t else None, grp, batch, D, 1e-5, xmap)
    x = i["x"][:, :D].double()
    if mapped:
        x = x.view(batch, nv + nt, D)[:, nt:].reshape(-1, D)
    want = F.layer_norm(x, (D,), None if gamma is None else gamma.double(), None if beta is None else beta.double(), ref._f32(1e-5))
    if gamma is None and beta is not None:
        want = F.layer_norm(x, (D,), None, None, ref._f32(1e-5)) + beta.double()
    if has_t:
        want = want.view(batch, nv // per, per, D) * (1 + i["scale"].double()[:, 1:, None]) + i["shift"].double()[:, 1:, None]
    torch.testing.assert_close(got, want.reshape(-1, D), rtol=1e-12, atol=1e-12)
    g32 = ref.layernorm_modulate(i["x"], gamma, beta, i["scale"] if has_t else None, i["shift"] if has_t else None, grp, batch, D, 1e-5, xmap, F32)
    assert g32.dtype == F32 and (g32.double() - got).abs().max() < 1e-5


def test_group_lookup_matches_the_device_function():
    for seq, nt, per in [(25, 3, 5), (683, 7, 97), (131, 7, 31), (32, 0, 8), (20, 4, 0), (5, 5, 3)]:
        want = [0 if s < nt else (1 + (s - nt) // per if per > 0 else 1) for s in range(seq)]
        assert ref.group_of_rows(seq, nt, per).tolist() == want


@pytest.mark.parametrize("rows,D", [(16, 32), (75, 32), (75, 1920), (256, 64), (2049, 2048), (1, 32)])
def test_pack_p16_is_a_bijection_onto_the_packed_buffer(rows, D):
    pos = ref.pack_p16(rows, D)
    full_rows = -(-rows // 16) * 16
    flat = pos.flatten()
    assert flat.min() >= 0 and flat.max() < full_rows * D and flat.unique().numel() == rows * D
    full = ref.pack_p16(full_rows, D)
    assert torch.equal(full.flatten().sort().values, torch.arange(full_rows * D))          # whole 16-row blocks: onto
    assert torch.equal(full[:rows], pos)                                                   # the pad rows own the remaining slots
    # the definition, spelled out per 16-byte chunk
    for r, c in [(0, 0), (rows - 1, D // 8 - 1), (rows // 2, (D // 8) // 2)]:
        want = (((r >> 4) * (D >> 5) + (c >> 2)) * 64 + (c & 3) * 16 + (r & 15)) * 8
        assert pos[r, c * 8:c * 8 + 8].tolist() == list(range(want, want + 8))


@pytest.mark.parametrize("idx", range(len(ref.QKV_CASES)))
def test_qkv_prep_against_layer_norm_and_apply_rotary_emb(idx):
    case = ref.QKV_CASES[idx]
    S, H = case[0], case[1]
    inp = ref.qkv_inputs(case, ref.QKV_SEEDS[idx])
    B, nt = inp["B"], inp["n_text"]
    pm = ref.QKV_PREMULS[1]
    got = ref.qkv_reference(case, inp, pm)
    x = inp["src"].view(B, S, 3, H, 64)
    dbl = lambda t: None if t is None else t.double()
    for which, name in ((0, "q"), (1, "k")):
        y = F.layer_norm(x[:, :, which].double(), (64,), dbl(inp["g" + name]), dbl(inp["b" + name]), ref._f32(1e-6))
        tol = torch.full_like(y, 1e-12)
        if nt < S:
            rounded = y[:, nt:].float().to(BF).double()
            # leaf.apply_rotary_emb multiplies in float32: 2^-22 of the two products; a flagged element may round the other way
            rot = leaf.apply_rotary_emb(rounded.permute(0, 2, 1, 3), inp["rope"]).permute(0, 2, 1, 3)
            y = torch.cat([y[:, :nt], rot], dim=1)
            cos, sin = (t.double().abs().max().item() for t in inp["rope"])
            tol[:, nt:] = 2.0 ** -22 * 2 * (cos + sin) * rounded.abs().amax(-1, keepdim=True) + got["flip_" + name][:, nt:] / (pm if which == 0 else 1)
        if which == 0:
            y, tol = y * ref._f32(pm), tol * pm
        assert ((got[name] - y).abs() <= tol).all(), name
    assert torch.equal(got["v"], x[:, :, 2])
    s_pad = (S + 63) // 64 * 64
    assert got["vT"].shape == (B, H, 64, s_pad)
    for s in range(s_pad):
        p = (s & ~12) | ((s & 4) << 1) | ((s & 8) >> 1)
        want = x[:, s, 2].permute(0, 1, 2) if s < S else torch.zeros(B, H, 64, dtype=BF)
        assert torch.equal(got["vT"][..., p], want), s
    k1 = ref.qkv_reference(case, inp, 1.0)
    assert torch.equal(k1["k"], got["k"]) and torch.equal(k1["q"] * ref._f32(pm), got["q"])


def test_activations_against_functional():
    v = torch.randn(4000, generator=gen(2)).double() * 4
    torch.testing.assert_close(ref.silu(v), F.silu(v), rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(ref.gelu_tanh(v), F.gelu(v, approximate="tanh"), rtol=1e-13, atol=1e-15)
    w = torch.linspace(-8, 8, 200001, dtype=F64, requires_grad=True)
    for name, fn in (("silu", ref.silu), ("gelu_tanh", ref.gelu_tanh)):
        (slope,) = torch.autograd.grad(fn(w).sum(), w)
        assert slope.abs().max().item() <= ref.ACT_SLOPE[name]


@pytest.mark.parametrize("idx", range(len(ref.MOD_CASES)))
def test_modulation_tables_against_functional_linear(idx):
    inp = ref.mod_inputs(ref.MOD_CASES[idx], ref.MOD_SEEDS[idx])
    got = ref.mod_reference(inp)
    B, T, width, text = inp["B"], inp["T"], inp["width"], inp["text"]
    temb = inp["temb"].double()
    cv = temb[:, None] if inp["act"] is None else (inp["temb"][:, None] + inp["act"]).double()      # bf16 + bf16 in torch: the model-dtype add
    cv, ct = F.silu(cv).float().to(BF).double(), F.silu(temb).float().to(BF).double()
    for i, W in enumerate(inp["Ws"]):
        b = None if inp["bs"] is None or inp["bs"][i] is None else inp["bs"][i].double()
        want = F.linear(cv, W[:width].double(), None if b is None else b[:width])
        tol = got["tie"][i] + 1e-12
        assert ((got["out"][i, :, 1:] - want).abs() <= tol[:, 1:]).all()
        if text:
            want = F.linear(ct, W[width:].double(), None if b is None else b[width:])
            assert ((got["out"][i, :, 0] - want).abs() <= tol[:, 0]).all()
        else:
            assert (got["out"][i, :, 0] == 0).all()
    assert (got["abs_terms"] >= got["out"].abs() - 1e-12).all()


@pytest.mark.parametrize("name", list(ref.SKINNY_CASES))
def test_skinny_linear_against_functional_linear(name):
    inp = ref.skinny_inputs(name, ref.SKINNY_SEEDS[name])
    got = ref.skinny_reference(inp)
    act = {None: lambda v: v, "silu": F.silu, "gelu_tanh": lambda v: F.gelu(v, approximate="tanh")}
    x = inp["x"]
    if inp["xb"] is not None:
        x = x + inp["xb"][torch.arange(x.shape[0]) // inp["xb_rep"]]               # bf16 add in torch
    st = act[inp["act_in"]](x.double()).float().to(BF).double()
    want = act[inp["act_out"]](F.linear(st, inp["W"].double(), None if inp["bias"] is None else inp["bias"].double()))
    assert ((got["out"] - want).abs() <= got["tie"] + 1e-12).all()
    assert (got["abs_terms"] >= got["pre"].abs() - 1e-12).all()
    o32 = ref.skinny_reference(inp, F32)["out"]
    assert o32.dtype == F32 and (o32.double() - got["out"]).abs().max() <= 1e-4 * got["abs_terms"].max()


@pytest.mark.parametrize("dim", ref.TS_DIMS)
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shift", [0.0, 1.0])
def test_timestep_embedding_against_the_oracle(dim, flip, shift):
    t = torch.tensor(ref.TS_VALUES)
    got = ref.timestep_embedding(t, dim, flip, shift)
    want = leaf.get_timestep_embedding(t, dim, flip, shift).double()
    if dim // 2 - shift == 0:
        assert torch.isnan(got[:, :2]).all() and torch.isnan(want[:, :2]).all()      # 0 / 0 in the exponent, there as here
        return
    # the oracle evaluates in float32: its angle t f carries up to 999 * 2^-22
    assert (got - want).abs().max().item() <= 999 * 2.0 ** -22 + 2.0 ** -22
    if dim % 2:
        assert (got[:, -1] == 0).all()
    assert torch.equal(got[:1], ref.timestep_embedding(t[:1], dim, flip, shift))


@pytest.mark.parametrize("cidx", range(12))
def test_sched_step_against_the_oracle_schedulers(cidx):
    c = ref.sched_coefficients()[cidx]
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
              set_alpha_to_one=True, prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=3.0,
              timestep_spacing="trailing")
    g = gen(40 + cidx)
    x, vc, vu = (ref.rb(g, 257) for _ in range(3))
    old = torch.randn(257, generator=g)
    gs = 6.0
    v = vu.double() + gs * (vc.double() - vu.double())
    tol = dict(rtol=0, atol=2e-6)                       # the restatement rounds the coefficients to float32
    if not c["dpm"]:
        s = leaf.CogVideoXDDIMScheduler(**kw)
        s.set_timesteps(c["steps"])
        want_x, want_x0 = s.step(v, c["t"], x.double(), return_dict=False)
        got = ref.sched_step(x, vc, vu, gs, None, None, c["sa"], c["sb"], 0.0, 0.0, c["cx"], c["cd"], 0.0)
        torch.testing.assert_close(got["x"], want_x, **tol)
        torch.testing.assert_close(got["x0"], want_x0, **tol)
        assert got["n_x0"] == 4 and (got["abs_x0"] >= got["x0"].abs() - 1e-12).all()
        return
    s = leaf.CogVideoXDPMScheduler(**kw)
    s.set_timesteps(c["steps"])
    for with_old in (False, True):
        if with_old and c["m3"] is None:
            continue
        noise = torch.randn(257, generator=gen(5), dtype=F64)
        if with_old:
            noise = torch.randn(257, generator=(g2 := gen(5)), dtype=F64), torch.randn(257, generator=g2, dtype=F64)
            noise = noise[1]                            # the oracle draws twice on a second-order step and uses the second draw
        want_x, want_x0 = s.step(v, old.double() if with_old else None, c["t"], c["t_back"], x.double(), generator=gen(5))
        got = ref.sched_step(x, vc, vu, gs, old if with_old else None, noise.float(), c["sa"], c["sb"], c["m3"] or 0.0, c["m4"] or 0.0,
                             c["cx"], c["cd"], c["cn"])
        torch.testing.assert_close(got["x"], want_x, rtol=0, atol=2e-6 + 2.0 ** -23 * 5 * abs(c["cn"]))   # + the fp32 rounding of the noise
        torch.testing.assert_close(got["x0"], want_x0, **tol)


def test_row_kernels_restatements():
    g = gen(3)
    D, seq, nt, Bv = 16, 10, 3, 3
    a, b = ref.rb(g, 2 * 9, D + 8), ref.rb(g, 8, D)
    out = ref.add_rows(a, (4, 9, 2), b, 8, D)
    for m in range(8):
        want = (a[(m // 4) * 9 + 2 + m % 4, :D].double() + b[m].double()).float().to(BF)
        assert torch.equal(out[m], want)
    idx = torch.tensor([5, 5, 0, 17], dtype=torch.int32)
    assert torch.equal(ref.gather_rows(a, idx, D), torch.stack([a[5, :D], a[5, :D], a[0, :D], a[17, :D]]))
    x, y = ref.rb(g, Bv * seq, D), ref.rb(g, 6, D)
    gate = torch.randn(Bv, D, generator=g)
    idx = torch.tensor([4, 12, 0, 29, 21, 13], dtype=torch.int32)        # rows 12 and 0 and 21 are text rows (s = 2, 0, 1)
    got, touched = ref.scatter_gated_rows(x, y, idx, gate, seq, nt, D)
    want = x.double().clone()
    for r, t in enumerate(idx.tolist()):
        if t % seq >= nt:
            want[t] += gate[t // seq].double() * y[r].double()
    assert torch.equal(got, want) and touched.nonzero().flatten().tolist() == [4, 13, 29]


_TIE = ref.tie_cases()


@pytest.mark.parametrize("k", range(len(_TIE)), ids=[f"{f}-{i}" for f, i, _ in _TIE])
def test_tie_cap_of_every_case_with_an_inner_rounding(k):
    """At most 2 % of the rounded intermediates of a case may lie within the window (16 x the float32-vs-float64 error of that
    intermediate on the case's own inputs) of a bf16 rounding boundary: a condition on the inputs, from the reference alone."""
    family, ident, thunk = _TIE[k]
    frac = thunk()["tie_frac"]
    assert frac <= 0.02, (family, ident, frac)


def test_case_tables_cover_the_forms_the_issue_lists():
    assert {c[0] for c in ref.QKV_CASES if c[1] == 1} == {1, 8, 15, 16, 17, 63, 64, 65, 129}
    assert {c[2] for c in ref.QKV_CASES} == {"inplace_vt", "inplace", "from_vt", "from"}
    assert {c[3] for c in ref.QKV_CASES} == {"all", "nobias", "none"} and {c[4] for c in ref.QKV_CASES} == {"nt0", "nt5", "ntS-1", "ntS"}
    assert {c[2] for c in ref.MOD_CASES} == {64, 128, 256, 512} and {c[3] for c in ref.MOD_CASES} == {32, 96, 544}
    for E in (64, 128, 256, 512):
        assert {c[0] * (c[1] if c[5] else 1) for c in ref.MOD_CASES if c[2] == E} >= {1, 32, 33}
    assert {(c["M"], c["N"], c["K"]) for c in ref.SKINNY_CASES.values()} >= {(1, 1, 8), (16, 5, 64), (17, 28, 28), (3, 9, 4), (5, 7, 60),
                                                                             (33, 40, 520), (3, 8, 2056), (3, 8, 5120)}
    assert sorted({c[1] for c in ref.SCHED_CASES}) == list(range(12))
    for bit in range(2, 6):
        assert {c[bit] for c in ref.SCHED_CASES} == {False, True}
    coefs = ref.sched_coefficients()
    kept = [c for c in ref.SCHED_CASES if c[3] and coefs[c[1]]["m3"] is not None]        # old_x0 is dropped where m3 / m4 are not finite
    assert len(kept) >= 2 and all(coefs[c[1]]["dpm"] for c in kept)
    # the one-row LayerNorm kernel: CH = 1, 2, 4 through the partial forms, 6 and 8 through the full form above D = 2048
    assert set(ref.LN_PARTIAL_WIDTHS.values()) == {1, 2, 4}
    assert all((D // 8 + 63) // 64 <= ch and ((D // 8 + 63) // 64 > ch // 2) for D, ch in ref.LN_PARTIAL_WIDTHS.items())
    assert {(D // 8 + 63) // 64 for D in ref.LN_ONE_ROW_WIDTHS} == {5, 6, 7, 8}
    c = ref.SKINNY_CASES["16x2051x8"]                # the launcher halves npw from 8 while ceil(N / (4 npw)) * ceil(M / 16) < 256
    npw = 8
    while npw > 1 and -(-c["N"] // (4 * npw)) * -(-c["M"] // 16) < 256:
        npw //= 2
    assert npw == 2 and c["N"] % npw == 1
    assert len(ref.QKV_SEEDS) == len(ref.QKV_CASES) and len(ref.MOD_SEEDS) == len(ref.MOD_CASES) and len(ref.SKINNY_SEEDS) == len(ref.SKINNY_CASES)
    assert math.isclose(ref.QKV_PREMULS[1], 0.125 * math.log2(math.e))
