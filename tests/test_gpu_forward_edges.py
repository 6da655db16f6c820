"""The small forward kernels of the DiT trunk (``orv_amd/csrc/norm.hip``, ``embed.hip``) against the float64 restatements of
``tests/forward_ref.py``, at every launch form the library has and at the smallest shapes where each path can still go wrong.  The
case tables (with the kernel instantiation each entry reaches) live in ``forward_ref.py``; ``tests/test_forward_ref_host.py`` checks the
restatements and the inputs without a GPU.

Rules of every test here: a buffer the kernel overwrites is NaN-filled first; memory it must not touch (the gap between D and
ldx / ldy / ldo, text rows, rows of a joint buffer outside a row map, pad rows of a packed buffer, and PAD rows past the last live
row of every row-major output: what a lost ``row < rows`` guard of a ragged last wave or block would store to) carries a random sentinel
compared bit for bit.

Bounds (none of them comes from what a kernel returns):
  * index work (gather, the packed layout, V^T, the v third, out-of-place copies, add_rows): bit-exact.  add_rows is one fp32 add of two
    bf16 values rounded once: it equals (a.float() + b.float()).to(bf16).
  * bf16 outputs of all-fp32 arithmetic (LayerNorm-modulate, q / k, skinny_linear's bf16 output, timestep embedding, sched_step x,
    gated scatter): |err| <= 2^-8 |ref64| + 4 A, A = max |float32 evaluation - float64 evaluation| of the same restatement: the
    ``bf16_ok`` rule of ``test_gpu_backward_edges.py``, imported from there.
  * fp32 outputs that are sums (modulation tables, skinny_linear with out_f32, sched_step x0): |err| <= n 2^-23 sum|term| + 4 A_act,
    n = E, K, or the number of products of x0; A_act = float32-vs-float64 error of the output activation (0 without one).  The sum term
    is stated on the value before the activation; an activation's slope is at most 1.13 (forward_ref.ACT_SLOPE), and a worst-case
    fp32 accumulation of n terms loses n 2^-24 sum|term|, half the term, so the slope is covered.
  * tie term: the restatements round three intermediates to bf16 (the conditioning of the modulation tables, skinny_linear's staged
    input after act_in, the normalised q / k before RoPE) and flag the elements within 16 x (float32-vs-float64 error of that
    intermediate) of a rounding boundary.  A flagged element k adds |w_k| ulp_bf16(c_k) to every output it feeds (times the slope bound
    of act_out where there is one); a flagged RoPE input adds 2^-8 (|a cos| + |c sin|) to its pair.  Unflagged elements add nothing.
The measured maxima, as fractions of these bounds, are in ``profiles/forward_edge_parity.txt`` (``ORV_PARITY_REPORT=<file>`` makes a
run of this module write them).
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import forward_ref as ref
import test_gpu_backward_edges as bwd

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
PAD = 16                 # sentinel rows past the last live row of an output: one 16-row block, four workgroups of the one-row kernels
_MEASURED = {}


def _dev():
    return torch.device("cuda:0")


def _note(family, ratio):
    _MEASURED[family] = max(_MEASURED.get(family, 0.0), float(ratio))
    print(f"parity {family}: {float(ratio):.4f} of the bound")


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("ORV_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            for k in sorted(_MEASURED):
                f.write(f"{k:<44s} {_MEASURED[k]:.4f}\n")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def sentinel(seed, *shape, dtype=BF):
    """Random finite values whose bit patterns a stray store would change."""
    return (torch.randn(*shape, generator=gen(seed)) * 3).to(dtype)


def d(t):
    return None if t is None else t.to(_dev())


def bf16_ok(family, got, want64, want32, tie=None):
    """|err| <= 2^-8 |ref64| + 4 A (+ the tie term): ``test_gpu_backward_edges.bf16_ok`` itself where there is no tie term."""
    if tie is None:
        return bwd.bf16_ok(family, got, want64, want32, note=_note)
    got = got.double().cpu()
    assert torch.isfinite(got).all(), family
    A = (want32.double() - want64).abs().max().item()
    bound = 2.0 ** -8 * want64.abs() + 4 * A + tie
    ratio = ((got - want64).abs() / bound.clamp_min(1e-300)).max().item()
    _note(family, ratio)
    assert ratio <= 1.0, (family, ratio, A)


def sum_ok(family, got, want64, abs_terms, n_terms, a_act=0.0, tie=None):
    """fp32 accumulation bound: |err| <= n_terms 2^-23 sum|term| + 4 A_act (+ the tie term)."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), family
    bound = n_terms * 2.0 ** -23 * abs_terms + 4 * a_act
    if tie is not None:
        bound = bound + tie
    err = (got - want64).abs()
    assert (err[bound == 0] == 0).all(), family
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    _note(family, ratio)
    assert ratio <= 1.0, (family, ratio)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm-modulate
# ---------------------------------------------------------------------------------------------------------------------------
def _run_ln(D, batch, seq, n_text, per_group, wide, seed, gamma=True, beta=True, table=True, xmap=None, rows_x=None, ldx=None, ldy=None,
            x=None, packed=False):
    """One orv_layernorm_modulate(_packed) call.  -> (inputs, y on the host, its sentinel); row-major: the live rows of both, after the
    PAD rows behind them were compared."""
    from orv_amd import ops
    i = ref.ln_inputs(D, batch, seq, n_text, per_group, wide, seed, rows_x, ldx)
    if x is not None:
        i["x"] = x
    R = batch * seq
    tab = d(i["tab"])
    sc, sh, mb, mg = (tab[..., D:2 * D], tab[..., :D], i["mod_b"], i["mod_g"]) if table else (None, None, 0, 0)
    i["gamma"], i["beta"] = (i["gamma"] if gamma else None), (i["beta"] if beta else None)
    if not table:
        i["scale"] = i["shift"] = None
    if packed:
        sent = sentinel(seed + 1, ops.packed_rows(R) * D)
        y = sent.clone()
        y[ref.pack_p16(R, D).flatten()] = NAN
    else:
        sent = sentinel(seed + 1, R + PAD, ldy or D)
        y = sent.clone()
        y[:R, :D] = NAN
    y = d(y)
    ops.layernorm_modulate(d(i["x"]), y, d(i["gamma"]), d(i["beta"]), sc, sh, mb, mg, ops.groups(seq, n_text, per_group), batch, D, 1e-5,
                           ldx=ldx, ldy=ldy, xmap=ops.rowmap(*xmap) if xmap else None, out_packed=packed)
    y = y.cpu()
    if packed:
        return i, y, sent
    assert same_bits(y[R:], sent[R:])                                           # rows past batch * seq
    return i, y[:R], sent[:R]


def _ln_refs(i, grp, batch, D, xmap=None):
    args = (i["x"], i["gamma"], i["beta"], i["scale"], i["shift"], grp, batch, D, 1e-5, xmap)
    return ref.layernorm_modulate(*args), ref.layernorm_modulate(*args, dtype=F32)


@pytest.mark.parametrize("name", list(ref.LN_ROWS_CASES))
def test_layernorm_modulate_rows_kernel(name):
    D, batch, seq, nt, per, wide = ref.LN_ROWS_CASES[name]
    i, y, sent = _run_ln(D, batch, seq, nt, per, wide, 11 + D)
    r64, r32 = _ln_refs(i, (seq, nt, per), batch, D)
    bf16_ok("ln_mod rows", y, r64, r32)


@pytest.mark.parametrize("name", list(ref.LN_PACKED_CASES))
def test_layernorm_modulate_packed_output(name):
    """The P16 output is the row-major output of the same call, re-indexed; pad rows and pad blocks keep the sentinel."""
    D, batch, seq, nt, per, wide = ref.LN_PACKED_CASES[name]
    R = batch * seq
    i, y, _ = _run_ln(D, batch, seq, nt, per, wide, 21 + D)
    r64, r32 = _ln_refs(i, (seq, nt, per), batch, D)
    bf16_ok("ln_mod rows (row-major twin of packed)", y, r64, r32)
    _, yp, sent = _run_ln(D, batch, seq, nt, per, wide, 21 + D, packed=True)
    pos = ref.pack_p16(R, D)
    assert same_bits(yp[pos], y)
    rest = torch.ones(yp.numel(), dtype=torch.bool)
    rest[pos.flatten()] = False
    assert int(rest.sum()) > 0 and same_bits(yp[rest], sent[rest])


@pytest.mark.parametrize("D", list(ref.LN_ONE_ROW_WIDTHS))
def test_layernorm_modulate_one_row_kernel_widths(D):
    batch, seq, nt, per = ref.LN_ONE_ROW_GRP
    i, y, _ = _run_ln(D, batch, seq, nt, per, True, 31 + D)
    r64, r32 = _ln_refs(i, (seq, nt, per), batch, D)
    bf16_ok("ln_mod one-row full", y, r64, r32)


# "all" is not a partial form: with a row map it is ln_mod_kernel<CH, true> behind a map, without one the rows kernel at ldx / ldy != D
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("form", list(ref.LN_PARTIAL_FORMS) + ["all"])
@pytest.mark.parametrize("D", list(ref.LN_PARTIAL_WIDTHS))
def test_layernorm_modulate_partial_forms(D, form, mapped):
    batch, nv, nt, per = ref.LN_PARTIAL_GEOM
    has_g, has_b, has_t = ref.LN_PARTIAL_FORMS.get(form, (True, True, True))
    xmap = (nv, nv + nt, nt) if mapped else None
    i, y, sent = _run_ln(D, batch, nv, 0, per, True, 41 + D + len(form), has_g, has_b, has_t, xmap, batch * (nv + nt) if mapped else None,
                         D + 64, D + 8)
    r64, r32 = _ln_refs(i, (nv, 0, per), batch, D, xmap)
    bf16_ok(f"ln_mod partial[{form}]", y[:, :D], r64, r32)
    assert same_bits(y[:, D:], sent[:, D:])                                     # the gap between D and ldy


def test_layernorm_modulate_input_conditioning():
    """Cancellation in the variance, variance 0, one dominant element: the rows kernel at the model width."""
    D, batch, seq, nt, per = 1920, 3, 25, 3, 5
    g = gen(5)
    x = torch.empty(75, D)
    x[:25] = 100 + 0.5 * torch.randn(25, D, generator=g)
    x[25:50] = (0.3 * torch.arange(1, 26))[:, None]
    x[50:] = 0.01 * torch.randn(25, D, generator=g)
    x[50:, 7::77][:, :1] *= 2.0 ** 10
    x = x.to(BF)
    i, y, _ = _run_ln(D, batch, seq, nt, per, True, 51, x=x)
    r64, r32 = _ln_refs(i, (seq, nt, per), batch, D)
    for kind, rows in (("cancellation", slice(0, 25)), ("constant", slice(25, 50)), ("spike", slice(50, 75))):
        bf16_ok(f"ln_mod conditioning[{kind}]", y[rows], r64[rows], r32[rows])
    grp = ref.group_of_rows(seq, nt, per)
    const = i["beta"].double() * (1 + i["scale"].double()[1, grp]) + i["shift"].double()[1, grp]
    assert torch.equal(r64[25:50], const)                                       # variance 0: the result is beta (1 + scale) + shift


# ---------------------------------------------------------------------------------------------------------------------------
# qkv_prep
# ---------------------------------------------------------------------------------------------------------------------------
def _run_qkv(idx, pm):
    from orv_amd import ops
    case = ref.QKV_CASES[idx]
    S, H, form = case[0], case[1], case[2]
    inp = ref.qkv_inputs(case, ref.QKV_SEEDS[idx])
    B, nt = inp["B"], inp["n_text"]
    s_pad = (S + 63) // 64 * 64
    src = d(inp["src"])
    out_of_place = form.startswith("from")
    tail = sentinel(idx, PAD, 3 * H * 64)                                       # rows past B * S, and one head's worth of V^T rows
    qkv = torch.cat([torch.full_like(src, NAN) if out_of_place else src, d(tail)])
    vtail = sentinel(idx + 1, 64, s_pad)
    vT = torch.cat([torch.full((B * H * 64, s_pad), NAN, dtype=BF, device=_dev()), d(vtail)]) if form.endswith("_vt") else None
    ops.qkv_prep(qkv, vT, d(inp["gq"]), d(inp["bq"]), d(inp["gk"]), d(inp["bk"]), (d(inp["rope"][0]), d(inp["rope"][1])), B, S, H, nt,
                 s_pad, 1e-6, q_premul=pm, src=src if out_of_place else None)
    qkv = qkv.cpu()
    assert same_bits(qkv[B * S:], tail)
    if vT is not None:
        vT = vT.cpu()
        assert same_bits(vT[B * H * 64:], vtail)
        vT = vT[:B * H * 64].view(B, H, 64, s_pad)
    return case, inp, qkv[:B * S].view(B, S, 3, H, 64), vT, src.cpu()


@pytest.mark.parametrize("idx", range(len(ref.QKV_CASES)), ids=["-".join(map(str, c)) for c in ref.QKV_CASES])
def test_qkv_prep_forms(idx):
    runs = []
    for pm in ref.QKV_PREMULS:
        case, inp, qkv, vT, src = _run_qkv(idx, pm)
        r64, r32 = ref.qkv_reference(case, inp, pm), ref.qkv_reference(case, inp, pm, F32)
        for which, name in ((0, "q"), (1, "k")):
            bf16_ok(f"qkv_prep {name}", qkv[:, :, which], r64[name], r32[name], tie=r64["tie_" + name])
            # what the issue's tie term leaves of a flipped rounding (ulp_bf16(a) > 2^-8 |a|): recorded, not asserted
            A = (r32[name].double() - r64[name]).abs().max().item()
            full = 2.0 ** -8 * r64[name].abs() + 4 * A + torch.maximum(r64["tie_" + name], r64["flip_" + name])
            _note(f"qkv_prep {name} [tie term = a full ulp]", ((qkv[:, :, which].double() - r64[name]).abs() / full.clamp_min(1e-300)).max())
        assert same_bits(qkv[:, :, 2], inp["src"].view(qkv.shape)[:, :, 2])     # the v third: in place untouched, out of place copied
        assert same_bits(src, inp["src"])                                       # src= is read only
        if vT is not None:
            assert same_bits(vT, r64["vT"])                                     # bits 2 / 3 of the key exchanged, zero padding
        runs.append((qkv, vT))
    (q0, v0), (q1, v1) = runs
    assert same_bits(q0[:, :, 1:], q1[:, :, 1:])                                # k and v do not depend on q_premul
    assert (v0 is None and v1 is None) or same_bits(v0, v1)
    assert not same_bits(q0[:, :, 0], q1[:, :, 0])


# ---------------------------------------------------------------------------------------------------------------------------
# modulation tables
# ---------------------------------------------------------------------------------------------------------------------------
def _launch_mod(inp):
    """-> out fp32 [n_tab, B, 1 + T, width] on the host.  Rows the kernel writes are NaN-filled; with text off row 0 is zero-filled."""
    from orv_amd import ops
    dev = _dev()
    B, T, E, width, text = inp["B"], inp["T"], inp["E"], inp["width"], inp["text"]
    Ws = [w.to(dev) for w in inp["Ws"]]
    bs = None if inp["bs"] is None else [None if b is None else b.to(dev) for b in inp["bs"]]
    wp = torch.tensor([w.data_ptr() for w in Ws], dtype=torch.int64, device=dev)
    bp = None if bs is None else torch.tensor([0 if b is None else b.data_ptr() for b in bs], dtype=torch.int64, device=dev)
    out = torch.full((len(Ws), B, 1 + T, width), NAN, dtype=F32, device=dev)
    if not text:
        out[:, :, 0] = 0
    ops.modulation_tables(d(inp["temb"]), d(inp["act"]), wp, bp, len(Ws), B, T, E, width, text, out=out)
    torch.cuda.synchronize()
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _run_mod(idx):
    inp = ref.mod_inputs(ref.MOD_CASES[idx], ref.MOD_SEEDS[idx])
    return inp, _launch_mod(inp), ref.mod_reference(inp)


def _check_mod(family, inp, out, r64):
    sum_ok(family, out, r64["out"], r64["abs_terms"], inp["E"], tie=r64["tie"])
    if not inp["text"]:
        assert (bits(out[:, :, 0]) == 0).all()                                  # text off: row 0 stays zero


@pytest.mark.parametrize("idx", range(len(ref.MOD_CASES)), ids=["-".join(map(str, c)) for c in ref.MOD_CASES])
def test_modulation_tables_forms(idx):
    inp, out, r64 = _run_mod(idx)
    _check_mod(f"mod_tables E={inp['E']}", inp, out, r64)


_MOD_CHILD = r"""
import sys, torch
sys.path.insert(0, "tests")
import forward_ref as ref
import test_gpu_forward_edges as t
inp = ref.mod_inputs(ref.MOD_CHILD_CASE, ref.MOD_CHILD_SEED)
torch.save(t._launch_mod(inp), sys.argv[1])
print("CHILD-OK")
"""


def test_modulation_tables_direct_load_kernel_at_e512(tmp_path):
    """ORV_MOD_TABLES_LDS=0 (read once per process): mod_tables_kernel<32> in a fresh process.  It issues the MFMA sequence of the LDS
    kernel on the same operands, so the two outputs are expected to be bit-identical; the fp32 bound holds in any case."""
    idx = ref.MOD_CASES.index(ref.MOD_CHILD_CASE)
    inp, out, r64 = _run_mod(idx)
    path = str(tmp_path / "child.pt")
    r = subprocess.run([sys.executable, "-c", _MOD_CHILD, path], cwd=ROOT, env=dict(os.environ, ORV_MOD_TABLES_LDS="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    child = torch.load(path)
    _check_mod("mod_tables E=512 ORV_MOD_TABLES_LDS=0", inp, child, r64)
    differ = int((bits(child) != bits(out)).sum())
    _note("mod_tables LDS=0 vs LDS=1 differing elements", differ)
    assert differ == 0


# ---------------------------------------------------------------------------------------------------------------------------
# skinny_linear
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.SKINNY_CASES))
def test_skinny_linear_forms(name):
    from orv_amd import ops
    c = ref.SKINNY_CASES[name]
    inp = ref.skinny_inputs(name, ref.SKINNY_SEEDS[name])
    M, N, K = c["M"], c["N"], c["K"]
    f32 = c.get("out") == "f32"
    ldo, omap = N + c.get("ldo_pad", 0), c.get("omap")
    rows = ref.mapped_rows(M, omap)
    n_rows = ((M // omap[0]) * omap[1] if omap else M) + PAD
    sent = sentinel(7 + M + N + K, n_rows, ldo, dtype=F32 if f32 else BF)
    out = sent.clone()
    out[rows, :N] = NAN
    out = d(out)
    ops.skinny_linear(d(inp["x"]), d(inp["W"]), d(inp["bias"]), xb=d(inp["xb"]), xb_rep=inp["xb_rep"], act_in=inp["act_in"],
                      act_out=inp["act_out"], out=out, ldo=ldo, omap=ops.rowmap(*omap) if omap else None)
    out = out.cpu()
    r64 = ref.skinny_reference(inp)
    tie = r64["tie"] if inp["act_in"] else None
    if f32:
        sum_ok("skinny_linear f32", out[rows, :N], r64["out"], r64["abs_terms"], K, r64["a_act"], tie)
    else:
        bf16_ok("skinny_linear bf16", out[rows, :N], r64["out"], ref.skinny_reference(inp, F32)["out"], tie)
    untouched = torch.ones(out.shape, dtype=torch.bool)
    untouched[rows, :N] = False
    assert same_bits(out[untouched], sent[untouched])                           # ldo gap, rows outside the map, rows past M


# ---------------------------------------------------------------------------------------------------------------------------
# timestep embedding, sched_step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 1.0])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("dim", ref.TS_DIMS)
def test_timestep_embedding_forms(dim, flip, shift):
    from orv_amd import ops
    for ts in [ref.TS_VALUES] + [(v,) for v in ref.TS_VALUES]:                  # batch 4, and each value as a batch of 1
        t = torch.tensor(ts, dtype=F32)
        got = ops.timestep_embedding(d(t), dim, flip, shift).cpu()
        assert got.shape == (len(ts), dim)
        r64, r32 = ref.timestep_embedding(t, dim, flip, shift), ref.timestep_embedding(t, dim, flip, shift, F32)
        if dim // 2 - shift == 0:                                               # one frequency and freq_shift = 1: 0 / 0 in the reference too
            assert torch.isnan(r64[:, :2]).all() and torch.isnan(got.float()[:, :2]).all()
            continue
        bf16_ok("timestep_embedding", got, r64, r32)


@pytest.mark.parametrize("k", range(len(ref.SCHED_CASES)))
def test_sched_step_forms(k):
    from orv_amd import ops
    n, cidx, with_u, with_old, with_noise, want_x0 = ref.SCHED_CASES[k]
    c = _sched_coefficients()[cidx]
    with_old = with_old and c["m3"] is not None
    g = gen(60 + k)
    x, vc, vu = ref.rb(g, n), ref.rb(g, n), ref.rb(g, n)
    old, noise = torch.randn(n, generator=g), torch.randn(n, generator=g)
    args = (x, vc, vu if with_u else None, 6.0, old if with_old else None, noise if with_noise else None, c["sa"], c["sb"], c["m3"] or 0.0,
            c["m4"] or 0.0, c["cx"], c["cd"], c["cn"])
    xo, x0 = ops.sched_step(*(d(a) if torch.is_tensor(a) else a for a in args), want_x0=want_x0)
    r64, r32 = ref.sched_step(*args), ref.sched_step(*args, dtype=F32)
    bf16_ok("sched_step x", xo.cpu(), r64["x"], r32["x"])
    assert (x0 is not None) == want_x0
    if want_x0:
        sum_ok("sched_step x0", x0.cpu(), r64["x0"], r64["abs_x0"], r64["n_x0"])


@functools.lru_cache(maxsize=None)
def _sched_coefficients():
    return ref.sched_coefficients()


# ---------------------------------------------------------------------------------------------------------------------------
# add_rows, gather_rows, scatter_gated_rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["row_map", "col_off", "in_place"])
@pytest.mark.parametrize("D", ref.ROW_DS)
def test_add_rows_forms(D, form):
    """Bit-exact: one fp32 add of two bf16 values, rounded once."""
    from orv_amd import ops
    g = gen(D + len(form))
    B, nv, nt = 2, 25, 4
    M = B * nv
    b = ref.rb(g, M, D)
    if form == "row_map":                           # a is the video part of a joint buffer with lda > D
        a, amap, lda, ldo, col = ref.rb(g, B * (nv + nt), D + 8), (nv, nv + nt, nt), D + 8, D, 0
    elif form == "col_off":                         # the stages.py form: out is a column block of a wider buffer
        a, amap, lda, ldo, col = ref.rb(g, M, D), None, D, 2 * D + 16, 16
    else:                                           # the training.py form: out is a
        a, amap, lda, ldo, col = ref.rb(g, M + PAD, D), None, D, D, 0
    want = ref.add_rows(a, amap, b, M, D)
    sent = sentinel(D, M + PAD, ldo)
    ad = d(a)
    if form == "in_place":
        out = ad
    else:
        out = sent.clone()
        out[:M, col:col + D] = NAN
        out = d(out)
    ops.add_rows(ad, ops.rowmap(*amap) if amap else None, d(b), out, col, M, D, lda=lda, ldo=ldo)
    out = out.cpu()
    assert same_bits(out[:M, col:col + D], want)
    assert same_bits(out[M:], (a if form == "in_place" else sent)[M:])          # rows past M
    if form != "in_place":
        assert same_bits(out[:, :col], sent[:, :col]) and same_bits(out[:, col + D:], sent[:, col + D:])
        assert same_bits(ad.cpu(), a)


@pytest.mark.parametrize("D", ref.ROW_DS)
def test_gather_rows_with_repeats_and_strides(D):
    from orv_amd import ops
    g = gen(D)
    Rs, R = 40, 50
    src = ref.rb(g, Rs, D + 8)
    idx = torch.randint(0, Rs, (R,), generator=g).to(torch.int32)
    idx[1] = idx[0]
    sent = sentinel(D + 1, R + PAD, D + 16)
    dst = sent.clone()
    dst[:R, :D] = NAN
    dst = d(dst)
    ops.gather_rows(d(src), d(idx), dst, R, D, ld_src=D + 8, ld_dst=D + 16)
    dst = dst.cpu()
    assert same_bits(dst[:R, :D], ref.gather_rows(src, idx, D)) and same_bits(dst[:, D:], sent[:, D:]) and same_bits(dst[R:], sent[R:])


@pytest.mark.parametrize("D", ref.ROW_DS)
def test_scatter_gated_rows_against_float64(D):
    """Distinct targets; text-row targets, untargeted rows and the ldx gap stay bit for bit; the updated rows meet the bf16 bound."""
    from orv_amd import ops
    g = gen(D + 3)
    Bv, seq, nt, R = 4, 20, 4, 50
    x, y = ref.rb(g, Bv * seq, D + 8), ref.rb(g, R, D + 16)
    idx = torch.randperm(Bv * seq, generator=g)[:R].to(torch.int32)
    gate = torch.randn(Bv, 3 * D, generator=g)
    gd = d(gate)
    xd = d(x)
    ops.scatter_gated_rows(d(y), d(idx), gd[:, 2 * D:], 3 * D, xd, R, D, seq, nt, ldy=D + 16, ldx=D + 8)
    got = xd.cpu()
    (r64, touched), (r32, _) = (ref.scatter_gated_rows(x, y, idx, gate[:, 2 * D:], seq, nt, D, dt) for dt in (F64, F32))
    assert 0 < int(touched.sum()) < R                                           # some targets are text rows
    bf16_ok("scatter_gated_rows", got[touched, :D], r64[touched], r32[touched])
    assert same_bits(got[~touched], x[~touched]) and same_bits(got[:, D:], x[:, D:])
