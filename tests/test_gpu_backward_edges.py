"""The hand-written backward kernels against the float64 restatements of ``tests/backward_ref.py``, at the operand forms
``orv_amd/training.py`` calls them in and at the shapes where their block decompositions change path.

Rules of every test here: a buffer the kernel overwrites is NaN-filled first, an accumulated output is preloaded with random
fp32 / bf16 values (added to the reference), memory the kernel must not touch carries a sentinel compared bit for bit.

Bounds (none of them comes from what the kernels return):
  * fp32 sums over rows (dgamma, dbeta, dscale, dshift, dgate, dgq .., db, gb, the fp32 dx / d_cond): the inputs are exact in fp32,
    so the only error is fp32 accumulation: |err| <= n_terms * 2^-23 * sum|term| elementwise (``colsum_ok``), and never looser
    than ``test_gpu_backward.close``.  One dropped row costs about sum|term| / n_terms: dozens of times the bound.
  * bf16 outputs of the all-fp32 kernels (dx, dy, dW, gW, the q / k thirds of dqkv): one bf16 rounding plus four times what the
    float32 CPU evaluation of the same formulas loses against float64: |err| <= 2^-8 |ref| + 4 A (``bf16_ok``).
  * attention backward: P and dS pass through bf16 inside the MFMA chain; the bounds of ``test_gpu_backward.test_attention_backward``.
  * accumulation: result(preloaded) - result(zeros) equals the preload within 1e-5 max|result|.
The measured maxima, as fractions of these bounds, are in ``profiles/backward_edge_parity.txt`` (``ORV_PARITY_REPORT=<file>`` makes
a run of this module write them).
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import backward_ref as ref
from test_gpu_backward import close

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
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


def rb(g, *shape, mul=1.0, add=0.0):
    """bf16-representable random values, as bf16."""
    return (torch.randn(*shape, generator=g) * mul + add).to(BF)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def colsum_ok(family, got, want, abs_terms, n_terms, preload=None, widen=1.0):
    """fp32 accumulation bound: |err| <= n_terms 2^-23 sum|term|, the preload counted as one more term."""
    got = got.double().cpu()
    scale = abs_terms.clone()
    n = n_terms
    if preload is not None:
        want, scale, n = want + preload.double().cpu(), scale + preload.double().cpu().abs(), n + 1
    assert torch.isfinite(got).all(), family
    bound = widen * n * 2.0 ** -23 * scale
    err = (got - want).abs()
    assert (err[bound == 0] == 0).all(), family
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    _note(family, ratio)
    assert ratio <= 1.0, (family, ratio)
    close(got, want)


def bf16_ok(family, got, want64, want32, note=None):
    """One bf16 rounding of the float64 value + 4 x the error of the float32 evaluation of the same restatement.
    ``note``: where the measured ratio is recorded (another module's ``_note``); this module's by default."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), family
    A = (want32.double() - want64).abs().max().item()
    bound = 2.0 ** -8 * want64.abs() + 4 * A
    ratio = ((got - want64).abs() / bound.clamp_min(1e-300)).max().item()
    (note or _note)(family, ratio)
    assert ratio <= 1.0, (family, ratio, A)


def accumulates(family, with_preload, with_zeros, preload):
    a, z, p = with_preload.double().cpu(), with_zeros.double().cpu(), preload.double().cpu()
    err = (a - z - p).abs().max().item()
    lim = 1e-5 * a.abs().max().item()
    _note(family + " accumulate", err / lim)
    assert err <= lim, (family, err, lim)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm-modulate backward
# ---------------------------------------------------------------------------------------------------------------------------
LN_B, LN_NT, LN_P, LN_NG = 2, 70, 100, 3                 # S = 370: bt = 5, bg = 7 (last block 4 rows), 52 blocks > 3 LNP_SLICE slabs
LN_S = LN_NT + LN_P * LN_NG
LN_NV = LN_S - LN_NT
LN_FORMS = {
    # grp (seq, n_text, per_group), xmap, table entries (None: no modulation), dres, affine
    "all": ((LN_S, LN_NT, LN_P), None, 1 + LN_NG, True, True),
    "no_dres": ((LN_S, LN_NT, LN_P), None, 1 + LN_NG, False, True),                      # norm_out
    "norm_final": ((LN_NV, 0, 0), (LN_NV, LN_S, LN_NT), None, False, True),              # row map, no table, text rows untouched
    "no_affine": ((LN_S, LN_NT, LN_P), None, 1 + LN_NG, True, False),
    "no_text": ((LN_NV, 0, LN_P), None, 1 + LN_NG, True, True),                          # table entry 0 has no rows
    "two_entry": ((LN_S, LN_NT, 0), None, 2, True, True),                                # MVBlock.norm1: text + one whole-video group
}


def _run_ln(D, form, preload, seed):
    """One orv_layernorm_modulate_bwd call; the tables are laid out as in training ([B, G, 3 D] = shift | scale | gate)."""
    from orv_amd import ops
    dev = _dev()
    grp, xmap, G, with_res, affine = LN_FORMS[form]
    seq = grp[0]
    R = LN_B * seq
    Rx = LN_B * LN_S if xmap else R
    g = torch.Generator().manual_seed(seed)
    c = {"dy": rb(g, R, D), "x": rb(g, Rx, D, mul=2.0, add=0.3), "dres": rb(g, Rx, D) if with_res else None,
         "gamma": rb(g, D) if affine else None, "beta": rb(g, D) if affine else None,
         "tab": torch.randn(LN_B, G, 3 * D, generator=g) * 0.5 if G else None}
    pre = {"dgamma": torch.randn(D, generator=g), "dbeta": torch.randn(D, generator=g),
           "dtab": torch.randn(LN_B, G, 3 * D, generator=g) * 3 if G else None}
    if not preload:
        pre = {k: None if v is None else torch.zeros_like(v) for k, v in pre.items()}
    d = lambda t: None if t is None else t.to(dev)
    dx = torch.full((Rx, D), NAN, dtype=BF, device=dev)
    sentinel = rb(g, Rx, D)
    if xmap:
        dx.copy_(sentinel)
    dgam, dbet = (d(pre["dgamma"]), d(pre["dbeta"])) if affine else (None, None)
    tab, dtab = d(c["tab"]), d(pre["dtab"])
    sc = dsc = dsh = None
    mb = mg = 0
    if G:
        sc, dsc, dsh, mb, mg = tab[..., D:2 * D], dtab[..., D:2 * D], dtab[..., :D], G * 3 * D, 3 * D
    ops.layernorm_modulate_bwd(d(c["dy"]), d(c["x"]), d(c["dres"]), dx, d(c["gamma"]), d(c["beta"]), sc, dsc, dsh, dgam, dbet, mb, mg,
                               ops.groups(*grp), LN_B, D, 1e-5, xmap=ops.rowmap(*xmap) if xmap else None)
    cpu = lambda t: None if t is None else t.cpu()
    return c, pre, {"dx": cpu(dx), "dgamma": cpu(dgam), "dbeta": cpu(dbet), "dtab": cpu(dtab), "sentinel": sentinel}


def _check_ln(D, form, seed):
    grp, xmap, G, with_res, affine = LN_FORMS[form]
    fam = f"ln_mod_bwd[{form}]"
    c, pre, got = _run_ln(D, form, True, seed)
    _, _, got0 = _run_ln(D, form, False, seed)
    args = (c["dy"], c["x"], c["dres"], c["gamma"], c["beta"], None if c["tab"] is None else c["tab"][..., D:2 * D], grp, 1e-5, xmap)
    r64, r32 = ref.ln_mod_bwd(*args), ref.ln_mod_bwd(*args, dtype=F32)
    rows = r64["rows"]
    bf16_ok(fam + " dx", got["dx"][rows], r64["dx"][rows], r32["dx"][rows])
    assert torch.equal(bits(got["dx"]), bits(got0["dx"]))                       # dx does not depend on the accumulators
    if xmap:
        untouched = torch.ones(got["dx"].shape[0], dtype=torch.bool)
        untouched[rows] = False
        assert int(untouched.sum()) == LN_B * LN_NT
        assert torch.equal(bits(got["dx"][untouched]), bits(got["sentinel"][untouched]))
    n_rows = c["dy"].shape[0]
    if affine:
        for k in ("dgamma", "dbeta"):
            colsum_ok(f"{fam} {k}", got[k], r64[k], r64["abs_" + k], n_rows, pre[k])
            accumulates(f"{fam} {k}", got[k], got0[k], pre[k])
    if G:
        cnt = r64["group_rows"][..., None].double()
        for k, sl in (("dshift", slice(0, D)), ("dscale", slice(D, 2 * D))):
            colsum_ok(f"{fam} {k}", got["dtab"][..., sl], r64[k], r64["abs_" + k], cnt, pre["dtab"][..., sl])
            accumulates(f"{fam} {k}", got["dtab"][..., sl], got0["dtab"][..., sl], pre["dtab"][..., sl])
        assert torch.equal(bits(got["dtab"][..., 2 * D:]), bits(pre["dtab"][..., 2 * D:]))          # the gate third is not this kernel's
        empty = r64["group_rows"] == 0
        assert bool(empty.any()) == (form == "no_text")
        assert torch.equal(bits(got["dtab"][empty]), bits(pre["dtab"][empty]))                      # an entry without rows is not written


@pytest.mark.parametrize("D", [72, 1920, 2048, 2056, 3072, 4096])
def test_layernorm_modulate_bwd_widths(D):
    """9 chunks, dead lanes in CH = 1, all lanes live, a single live lane in chunk 1, the 5B width, the maximum."""
    _check_ln(D, "all", D)


@pytest.mark.parametrize("form", ["all", "no_dres", "norm_final", "no_affine", "no_text", "two_entry"])
@pytest.mark.parametrize("D", [128, 3072])
def test_layernorm_modulate_bwd_operand_forms(D, form):
    _check_ln(D, form, D + len(form))


# ---------------------------------------------------------------------------------------------------------------------------
# gated-residual backward
# ---------------------------------------------------------------------------------------------------------------------------
GT_B, GT_NT, GT_P, GT_NG = 2, 70, 150, 2                 # GRB = 32: bt = 3 (6-row tail), bg = 5 (22-row tail)


def _run_gated(D, multiview, preload, seed):
    from orv_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    if multiview:               # [Bm, 1 + nv, D] gate table, entry 0 (text) without rows
        grp, G, width, col0 = (GT_P * GT_NG, 0, GT_P), 1 + GT_NG, D, 0
    else:                       # the gate third of a [B, G, 3 D] modulation table
        grp, G, width, col0 = (GT_NT + GT_P * GT_NG, GT_NT, GT_P), 1 + GT_NG, 3 * D, 2 * D
    R = GT_B * grp[0]
    c = {"dout": rb(g, R, D), "y": rb(g, R, D), "tab": torch.randn(GT_B, G, width, generator=g)}
    pre = torch.randn(GT_B, G, width, generator=g) * 3
    if not preload:
        pre = torch.zeros_like(pre)
    tab, dtab = c["tab"].to(dev), pre.to(dev)
    dy = torch.full((R, D), NAN, dtype=BF, device=dev)
    ops.gated_residual_bwd(c["dout"].to(dev), c["y"].to(dev), tab[..., col0:col0 + D], dtab[..., col0:col0 + D], dy, G * width, width,
                           ops.groups(*grp), GT_B, D)
    return c, pre, grp, col0, {"dy": dy.cpu(), "dtab": dtab.cpu()}


@pytest.mark.parametrize("D,multiview", [(72, False), (1920, False), (3072, False), (4096, False), (1920, True), (3072, True)])
def test_gated_residual_bwd_widths_and_multiview_table(D, multiview):
    fam = "gated_bwd[multiview]" if multiview else "gated_bwd"
    c, pre, grp, col0, got = _run_gated(D, multiview, True, D)
    _, _, _, _, got0 = _run_gated(D, multiview, False, D)
    gate = c["tab"][..., col0:col0 + D]
    r64, r32 = ref.gated_bwd(c["dout"], c["y"], gate, grp), ref.gated_bwd(c["dout"], c["y"], gate, grp, dtype=F32)
    bf16_ok(fam + " dy", got["dy"], r64["dy"], r32["dy"])
    assert torch.equal(bits(got["dy"]), bits(got0["dy"]))
    sl = slice(col0, col0 + D)
    colsum_ok(fam + " dgate", got["dtab"][..., sl], r64["dgate"], r64["abs_dgate"], r64["group_rows"][..., None].double(), pre[..., sl])
    accumulates(fam + " dgate", got["dtab"][..., sl], got0["dtab"][..., sl], pre[..., sl])
    other = torch.ones(pre.shape[-1], dtype=torch.bool)
    other[sl] = False
    assert torch.equal(bits(got["dtab"][..., other]), bits(pre[..., other]))
    empty = r64["group_rows"] == 0
    assert bool(empty.any()) == multiview
    assert torch.equal(bits(got["dtab"][empty]), bits(pre[empty]))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: the error of ops.check, nothing launched
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["ragged_groups", "D_not_8", "D_too_wide"])
def test_norm_and_gate_backward_refuse_unsupported_shapes(what):
    from orv_amd import ops
    dev = _dev()
    D = {"ragged_groups": 128, "D_not_8": 68, "D_too_wide": 4104}[what]
    grp = (52, 7, 11) if what == "ragged_groups" else (51, 7, 11)              # 45 video rows are no whole number of groups of 11; 44 are
    B, G = 2, 6
    g = torch.Generator().manual_seed(1)
    R = B * grp[0]
    a, b_ = rb(g, R, D).to(dev), rb(g, R, D).to(dev)
    tab = torch.randn(B, G, 3 * D, generator=g).to(dev)
    keep = {"dx": rb(g, R, D).to(dev), "dtab": torch.randn(B, G, 3 * D, generator=g).to(dev), "dg": torch.randn(D, generator=g).to(dev),
            "db": torch.randn(D, generator=g).to(dev)}
    before = {k: bits(v) for k, v in keep.items()}
    match = "whole number of groups" if what == "ragged_groups" else "unsupported"
    with pytest.raises(RuntimeError, match=match):
        ops.layernorm_modulate_bwd(a, b_, None, keep["dx"], None, None, tab[..., D:2 * D], keep["dtab"][..., D:2 * D], keep["dtab"][..., :D],
                                   keep["dg"], keep["db"], G * 3 * D, 3 * D, ops.groups(*grp), B, D, 1e-5)
    with pytest.raises(RuntimeError, match=match):
        ops.gated_residual_bwd(a, b_, tab[..., 2 * D:], keep["dtab"][..., 2 * D:], keep["dx"], G * 3 * D, 3 * D, ops.groups(*grp), B, D)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(bits(v), before[k]), k


def test_small_linear_bwd_refuses_more_than_4096_rows():
    from orv_amd import ops
    dev = _dev()
    R, N, K = 4097, 8, 8
    g = torch.Generator().manual_seed(2)
    keep = {"dW": rb(g, N, K).to(dev), "db": torch.randn(N, generator=g).to(dev), "dx": torch.randn(R, K, generator=g).to(dev)}
    before = {k: bits(v) for k, v in keep.items()}
    with pytest.raises(RuntimeError, match="bad arguments"):
        ops.small_linear_bwd(torch.randn(R, N, generator=g).to(dev), rb(g, R, K).to(dev), rb(g, N, K).to(dev), keep["dW"], keep["db"],
                             keep["dx"], R, N, K)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(bits(v), before[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# small-linear backward
# ---------------------------------------------------------------------------------------------------------------------------
def _run_small(R, N, K, accumulate, form, preload, seed):
    """form: "plain", "no_dx" (W = None, dx = None), "strided" (dy / x / dx are column blocks of wider buffers)."""
    from orv_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    c = {"dy": torch.randn(R, N, generator=g), "x": rb(g, R, K), "W": rb(g, N, K, mul=0.1)}
    pre = {"dW": rb(g, N, K), "db": torch.randn(N, generator=g), "dx": torch.randn(R, K, generator=g)}
    if not preload:
        pre = {k: torch.zeros_like(v) for k, v in pre.items()}
    if accumulate:
        dW, db = pre["dW"].to(dev), pre["db"].to(dev)
    else:
        dW, db = torch.full((N, K), NAN, dtype=BF, device=dev), torch.full((N,), NAN, device=dev)
    kw = {}
    pad = (3, 5) if form == "strided" else (0, 0)          # columns before / behind the block
    wide = lambda t, fill: torch.cat([fill(t.shape[0], pad[0]), t, fill(t.shape[0], pad[1])], dim=1).contiguous()
    dyw = wide(c["dy"], lambda r, n: torch.full((r, n), NAN)).to(dev)
    xw = wide(c["x"], lambda r, n: torch.full((r, n), NAN, dtype=BF)).to(dev)
    dx_host = wide(pre["dx"], lambda r, n: torch.randn(r, n, generator=g))
    dxw = dx_host.to(dev)
    if form == "strided":
        kw = {"ldy": dyw.shape[1], "ldx": xw.shape[1], "lddx": dxw.shape[1]}
    no_dx = form == "no_dx"
    ops.small_linear_bwd(dyw[:, pad[0]:], xw[:, pad[0]:], None if no_dx else c["W"].to(dev), dW, db, None if no_dx else dxw[:, pad[0]:],
                         R, N, K, accumulate=accumulate, **kw)
    return c, pre, {"dW": dW.cpu(), "db": db.cpu(), "dxw": dxw.cpu(), "dx_host": dx_host, "pad": pad}


@pytest.mark.parametrize("form", ["plain", "no_dx", "strided"])
@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("R,N,K", [(1, 64, 256), (33, 100, 300), (64, 640, 512), (45, 28, 2048), (24, 2048, 28)])
def test_small_linear_bwd_shapes_and_forms(R, N, K, accumulate, form):
    """One row; a second 32-row pass with one row, a ragged n-slab and K % 256 != 0; two full passes; the two conditioning-MLP shapes."""
    fam = f"small_linear_bwd[{form}]"
    seed = R * 7 + N
    c, pre, got = _run_small(R, N, K, accumulate, form, True, seed)
    _, _, got0 = _run_small(R, N, K, accumulate, form, False, seed)
    W = None if form == "no_dx" else c["W"]
    r64, r32 = ref.small_linear_bwd(c["dy"], c["x"], W), ref.small_linear_bwd(c["dy"], c["x"], W, dtype=F32)
    if accumulate:
        bf16_ok(fam + " dW", got["dW"], r64["dW"] + pre["dW"].double(), r32["dW"] + pre["dW"].float())
        colsum_ok(fam + " db", got["db"], r64["db"], r64["abs_db"], R, pre["db"])
        accumulates(fam + " db", got["db"], got0["db"], pre["db"])
    else:
        bf16_ok(fam + " dW", got["dW"], r64["dW"], r32["dW"])
        colsum_ok(fam + " db", got["db"], r64["db"], r64["abs_db"], R)
        assert torch.equal(bits(got["dW"]), bits(got0["dW"])) and torch.equal(bits(got["db"]), bits(got0["db"]))
    lo, hi = got["pad"][0], got["pad"][0] + K
    if form == "no_dx":
        assert torch.equal(bits(got["dxw"]), bits(got["dx_host"]))
    else:
        colsum_ok(fam + " dx", got["dxw"][:, lo:hi], r64["dx"], r64["abs_dx"], N, pre["dx"])        # always accumulated
        accumulates(fam + " dx", got["dxw"][:, lo:hi], got0["dxw"][:, lo:hi], pre["dx"])
        assert torch.equal(bits(got["dxw"][:, :lo]), bits(got["dx_host"][:, :lo]))
        assert torch.equal(bits(got["dxw"][:, hi:]), bits(got["dx_host"][:, hi:]))


# ---------------------------------------------------------------------------------------------------------------------------
# qkv-prep backward alone
# ---------------------------------------------------------------------------------------------------------------------------
def _run_qkv_prep(B, S, H, nt, use_rope, preload, seed):
    from orv_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    D = H * 64
    c = {"raw": rb(g, B, S, 3, H, 64, mul=1.5), "d": rb(g, B, S, 3, H, 64), "gq": rb(g, 64, mul=0.5, add=1.0), "gk": rb(g, 64, mul=0.5, add=1.0),
         "rope": None}
    if use_rope:
        ang = torch.rand(S - nt, 32, generator=g) * 6.28
        c["rope"] = (ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous())
    pre = [torch.randn(64, generator=g) * 5 for _ in range(4)]
    if not preload:
        pre = [torch.zeros(64) for _ in range(4)]
    acc = [p.to(dev) for p in pre]
    dqkv = c["d"].reshape(B * S, 3 * D).to(dev)
    rd = None if c["rope"] is None else tuple(r.to(dev) for r in c["rope"])
    ops.qkv_prep_bwd(c["raw"].reshape(B * S, 3 * D).to(dev), dqkv, c["gq"].to(dev), c["gk"].to(dev), rd, *acc, B, S, H, nt, 1e-6)
    return c, pre, {"dqkv": dqkv.cpu().view(B, S, 3, H, 64), "acc": [a.cpu() for a in acc]}


@pytest.mark.parametrize("B,S,H,nt,use_rope", [(1, 17, 1, 0, False), (2, 100, 3, 13, True), (1, 65, 2, 64, True), (3, 700, 7, 30, True)])
def test_qkv_prep_bwd_alone(B, S, H, nt, use_rope):
    """Random dq and dk (so d/d beta_k has a real reference), the n_text boundary inside a 64-row block and on its last row, 231 block
    partials (more than three reduce slabs); the dv third is not this kernel's."""
    fam = "qkv_prep_bwd"
    c, pre, got = _run_qkv_prep(B, S, H, nt, use_rope, True, S)
    _, _, got0 = _run_qkv_prep(B, S, H, nt, use_rope, False, S)
    args = (c["raw"], c["d"][:, :, 0], c["d"][:, :, 1], c["gq"], c["gk"], c["rope"], nt, 1e-6)
    r64, r32 = ref.qkv_prep_bwd(*args), ref.qkv_prep_bwd(*args, dtype=F32)
    bf16_ok(fam + " draw_q", got["dqkv"][:, :, 0], r64["draw_q"], r32["draw_q"])
    bf16_ok(fam + " draw_k", got["dqkv"][:, :, 1], r64["draw_k"], r32["draw_k"])
    assert torch.equal(bits(got["dqkv"][:, :, 2]), bits(c["d"][:, :, 2]))
    assert torch.equal(bits(got["dqkv"]), bits(got0["dqkv"]))
    for i, k in enumerate(("dgq", "dbq", "dgk", "dbk")):
        assert r64[k].abs().max().item() > 0.05 * r64["abs_" + k].max().item() / (B * S * H) ** 0.5        # a real, nonzero reference
        colsum_ok(f"{fam} {k}", got["acc"][i], r64[k], r64["abs_" + k], B * S * H, pre[i])
        accumulates(f"{fam} {k}", got["acc"][i], got0["acc"][i], pre[i])


# ---------------------------------------------------------------------------------------------------------------------------
# attention backward alone
# ---------------------------------------------------------------------------------------------------------------------------
ATTN_SCALE = 0.125
ATTN_SWEEP = [(1, s, 1, False) for s in (1, 17, 63, 65, 127, 128, 129, 191, 193, 255, 256, 257, 320, 321)]      # (B, S, H, peaked)
ATTN_GRIDS = [(3, 100, 5, False), (2, 700, 7, False), (1, 513, 3, False)]                                      # grids off the 8 XCDs
ATTN_CASES = ATTN_SWEEP + ATTN_GRIDS + [(1, 320, 1, True)]


@functools.lru_cache(maxsize=None)
def _attn_case(B, S, H, peaked):
    """Stored q' | k | v, dO, and out / lse / the gradients by the float64 reference (computed once per process and shape)."""
    g = torch.Generator().manual_seed(S * 10 + H + (5 if peaked else 0))
    qs = (torch.randn(B, S, H, 64, generator=g) * (ATTN_SCALE * ref.LOG2E)).to(BF)
    k, v, do = rb(g, B, S, H, 64), rb(g, B, S, H, 64), rb(g, B, S, H, 64)
    if peaked:                  # k[300] is 8 x q[5]: one softmax row of (almost) a single key, late in the sequence
        k[0, 300, 0] = (qs[0, 5, 0].float() / (ATTN_SCALE * ref.LOG2E) * 8).to(BF)
    t = lambda a: a.permute(0, 2, 1, 3)
    r = ref.attention_bwd(t(qs), t(k), t(v), t(do), ATTN_SCALE)
    if peaked:
        p_row = torch.softmax(ATTN_SCALE * (t(qs).double()[0, 0, 5] / (ATTN_SCALE * ref.LOG2E)) @ t(k).double()[0, 0].T, dim=-1)
        assert p_row[300].item() > 0.99
    return {"qkv": torch.stack([qs, k, v], dim=2).reshape(B * S, 3 * H * 64), "do": do.reshape(B * S, H * 64),
            "out": t(r["out"]).reshape(B * S, H * 64).to(BF), "lse": r["lse"].to(F32).contiguous(),
            "dq": t(r["dq"]).reshape(B * S, H * 64), "dk": t(r["dk"]).reshape(B * S, H * 64), "dv": t(r["dv"]).reshape(B * S, H * 64)}


def _run_attn(B, S, H, peaked, transposed_copies=False):
    """orv_attention_bwd alone; qT / kT / doT None (the shipped form) unless the older kernels are to run."""
    from orv_amd import ops
    dev = _dev()
    c = _attn_case(B, S, H, peaked)
    D = H * 64
    s_pad = (S + 63) // 64 * 64
    work, dod = c["qkv"].to(dev), c["do"].to(dev)
    qT = kT = doT = None
    if transposed_copies:
        qT, kT, doT = (torch.zeros(B, H, 64, s_pad, dtype=BF, device=dev) for _ in range(3))
        ops.head_transpose(work, 0, qT, B, S, H, s_pad, ld=3 * D)
        ops.head_transpose(work, D, kT, B, S, H, s_pad, ld=3 * D)
        ops.head_transpose(dod, 0, doT, B, S, H, s_pad, ld=D)
    nl, nd = (torch.full((B, H, s_pad), NAN, dtype=F32, device=dev) for _ in range(2))
    dqkv = torch.full((B * S, 3 * D), NAN, dtype=BF, device=dev)
    ops.attention_bwd(work, qT, kT, c["out"].to(dev), dod, doT, c["lse"].to(dev), nl, nd, dqkv, B, S, H, s_pad, ATTN_SCALE)
    return dqkv.cpu(), nl.cpu(), nd.cpu()


def _check_attn(B, S, H, peaked, got):
    dqkv, nl, nd = got
    c = _attn_case(B, S, H, peaked)
    D = H * 64
    assert not torch.isnan(dqkv).any(), "a row of dqkv was not written"
    assert (nl[..., S:] == 0).all() and (nd[..., S:] == 0).all()
    assert torch.isfinite(nl).all() and torch.isfinite(nd).all()
    close(nl[..., :S], -c["lse"] * ref.LOG2E, rtol=1e-6, afrac=1e-7)
    fam = "attention_bwd[peaked]" if peaked else "attention_bwd"
    for name, col, afrac in (("dv", 2, 1.5e-2), ("dk", 1, 2e-2), ("dq", 0, 2e-2)):
        g_, r_ = dqkv[:, col * D:(col + 1) * D].double(), c[name]
        lim = 2e-2 * r_.abs() + afrac * r_.abs().max().item() + 1e-6
        _note(f"{fam} {name}", ((g_ - r_).abs() / lim).max().item())
        close(g_, r_, afrac=afrac)


@pytest.mark.parametrize("B,S,H,peaked", ATTN_CASES)
def test_attention_bwd_alone(B, S, H, peaked):
    """Key-tile counts 1 ... 6 (prologue / epilogue of the two-ahead staging, the first slot wrap), S % 64 of 1 and 63, S < 32, a second
    256-row query item with one live row, grids that are no multiple of the 8 XCDs, one peaked softmax row."""
    _check_attn(B, S, H, peaked, _run_attn(B, S, H, peaked))


def _child_main(forked_path):
    """The attention cases once more in this (fresh) process, under the ORV_ATTN_BWD_* switches of its environment: in order, the first
    mismatch or HIP error ends the process with a non-zero status."""
    forked = torch.load(forked_path)
    older = os.environ.get("ORV_ATTN_BWD_PP") == "0"
    for i, case in enumerate(ATTN_CASES):
        got = _run_attn(*case, transposed_copies=older)
        _check_attn(*case, got)
        if not older:           # the same two kernels, launched back to back: the same bits
            assert torch.equal(bits(got[0]), bits(forked[i])), case
    print(f"CHILD-OK {len(ATTN_CASES)}")


@pytest.mark.parametrize("switch", ["ORV_ATTN_BWD_FORK", "ORV_ATTN_BWD_PP"])
def test_attention_bwd_switches_in_a_child_process(switch, tmp_path):
    """ORV_ATTN_BWD_FORK=0 (back-to-back launch: also the fallback when the fork fails) and ORV_ATTN_BWD_PP=0 with the head-transposed
    copies (the older kernels) are read once per process: every case again in a fresh child each."""
    path = str(tmp_path / "forked.pt")
    torch.save([_run_attn(*case)[0] for case in ATTN_CASES], path)
    env = dict(os.environ, **{switch: "0"})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"CHILD-OK {len(ATTN_CASES)}" in r.stdout, (switch, r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------------
# modulation-tables backward at the real conditioning width
# ---------------------------------------------------------------------------------------------------------------------------
def _run_mod_tables(B, T, text, n_tab, E, width, preload, seed):
    from orv_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    ntot = width * (2 if text else 1)
    c = {"Ws": [rb(g, ntot, E, mul=0.2) for _ in range(n_tab)], "cond_v": rb(g, B * T, E), "cond_t": rb(g, B, E),
         "dtab": torch.randn(n_tab, B, 1 + T, width, generator=g)}
    pre = {"dcv": torch.randn(B * T, E, generator=g) * 3, "dct": torch.randn(B, E, generator=g) * 3}
    if not preload:
        pre = {k: torch.zeros_like(v) for k, v in pre.items()}
    Wd = [w.to(dev) for w in c["Ws"]]
    ptrs = torch.tensor([w.data_ptr() for w in Wd], dtype=torch.int64, device=dev)
    dcv, dct = pre["dcv"].to(dev), pre["dct"].to(dev)
    gW, gb = ops.modulation_tables_bwd(c["dtab"].to(dev), c["cond_v"].to(dev), c["cond_t"].to(dev), ptrs, dcv, dct, n_tab, B, T, E, width, text)
    return c, pre, {"gW": gW.cpu(), "gb": gb.cpu(), "dcv": dcv.cpu(), "dct": dct.cpu()}


def test_modulation_tables_bwd_at_the_real_embedding_width():
    """E = 512: mod_bwd_dgrad_kernel's grid is ((E + 255) / 256) * 4 wide, and E = 64 never reaches its second column block."""
    B, T, text, n_tab, E, width = 2, 5, True, 2, 512, 384
    fam = "mod_tables_bwd"
    c, pre, got = _run_mod_tables(B, T, text, n_tab, E, width, True, 9)
    _, _, got0 = _run_mod_tables(B, T, text, n_tab, E, width, False, 9)
    args = (c["dtab"], c["cond_v"], c["cond_t"], c["Ws"], text)
    r64, r32 = ref.mod_tables_bwd(*args), ref.mod_tables_bwd(*args, dtype=F32)
    bf16_ok(fam + " gW", got["gW"], r64["gW"], r32["gW"])
    assert torch.equal(bits(got["gW"]), bits(got0["gW"])) and torch.equal(bits(got["gb"]), bits(got0["gb"]))
    n_gb = torch.cat([torch.full((width,), float(B * T)), torch.full((width,), float(B))]).double()
    colsum_ok(fam + " gb", got["gb"], r64["gb"], r64["abs_gb"], n_gb)
    colsum_ok(fam + " d_cond_v", got["dcv"], r64["d_cond_v"], r64["abs_d_cond_v"], n_tab * width, pre["dcv"])
    colsum_ok(fam + " d_cond_t", got["dct"], r64["d_cond_t"], r64["abs_d_cond_t"], n_tab * width, pre["dct"])
    accumulates(fam + " d_cond_v", got["dcv"], got0["dcv"], pre["dcv"])
    accumulates(fam + " d_cond_t", got["dct"], got0["dct"], pre["dct"])


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    _child_main(sys.argv[1])
